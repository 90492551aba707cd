/* avc.h -- C ABI of libavc.so, the MI355X (gfx950) implementation of the AvatarCLIP AppearanceGen hot path.
 *
 * The reference (hongfz16/AvatarCLIP) has no FFI of its own: the hot path is the Python call chain
 *   AvatarGen/AppearanceGen/main.py:418-420   Runner.train_clip -> NeuSRenderer.render
 *   AvatarGen/AppearanceGen/models/renderer.py:302-397 (render), :133-193 (up_sample/cat_z_vals), :195-300 (render_core)
 *   AvatarGen/AppearanceGen/models/fields.py:72-107,154-185 (SDFNetwork / RenderingNetwork)
 *   AvatarGen/AppearanceGen/main.py:512 (perceptor.encode_image -- OpenAI CLIP ViT-B/32, un-vendored)
 * Each entry point below names the reference lines it replaces.  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions: every pointer is a DEVICE pointer (hipMalloc / torch allocation) unless marked host; buffers are
 * caller-allocated, no ownership transfer; `stream` is a hipStream_t; all kernels are enqueued on it and the
 * call returns without synchronising.  Return value 0 = ok, otherwise avc_last_error() describes the failure.
 * No CPU fallback exists: with no GPU the calls fail.
 */
#ifndef AVC_H
#define AVC_H
#ifdef __cplusplus
extern "C" {
#endif

#define AVC_NET_FULL 0  /* confs/examples (all 144):   SDF 39-256-256-256-217(+39)-257, colour 262-256-256-{3,3} */
#define AVC_NET_SMALL 1 /* confs/examples_small:        SDF 39-128-128-89(+39)-129,     colour 134-128-{3,3}     */
/* the scaled-down shapes: d_hidden in {64, 128, 256} x depth in {SDF n_layers 4 + colour n_layers 2, SDF 3 + colour 1} */
#define AVC_NET_H128_DEEP 2    /* a full-size conf, d_hidden 128: SDF 39-128-128-128-89(+39)-129, colour 134-128-128-{3,3} */
#define AVC_NET_H256_SHALLOW 3 /* the small conf's depth, d_hidden 256: SDF 39-256-256-217(+39)-257, colour 262-256-{3,3}  */
#define AVC_NET_H64_DEEP 4     /* a full-size conf, d_hidden 64:  SDF 39-64-64-64-25(+39)-65,     colour 70-64-64-{3,3}    */
#define AVC_NET_H64_SHALLOW 5  /* the small conf's depth, d_hidden 64:  SDF 39-64-64-25(+39)-65,  colour 70-64-{3,3}       */
#define AVC_NET_COUNT 6        /* ids 0 .. AVC_NET_COUNT-1 are instantiated; every other id is refused by the launchers    */

/* Interface revision of this header.  It changes whenever an existing entry point's argument list or meaning changes (2: round 5 put
 * `colsum` into avc_render_points_bwd and moved the second-order row-0 term out of the weight-gradient products; 3: the rasteriser's
 * batched forward with save and its backward, avc_rasterize_mesh_save / avc_rasterize_mesh_grad; 4: avc_vit_linear_packed has the
 * arguments gelu_pre and y_pre, serves any M and replaces the separate entry for up to 128 rows), so a caller built
 * against an older header can refuse the library instead of passing arguments in the wrong slots:
 *     if (avc_version() != AVC_ABI_VERSION) abort();       (avatarclip_amd/lib.py: load() does exactly this)
 * An ADDED entry point does not change the number: a library that lacks a symbol declared here is refused at load, by the symbol's name. */
#define AVC_ABI_VERSION 4

const char* avc_last_error(void);
int avc_version(void);
/* number of int32 slots in the `offs` arrays below (== OFF_COUNT of csrc/avc_common.h) */
int avc_num_offsets(void);

/* SDFNetwork.sdf (fields.py:90-91) without autograd: renderer.py:337-338 (coarse), :187 (new samples),
 * :403 (extract_geometry query).  Points are either pts[N,3] or rays_o/rays_d[R,3] + z[R,ldz] (S per ray).
 * If slot != NULL the value of sample (ray,j) is scattered to sdf_out[ray*ld_out + slot[ray*S+j]]
 * (the merge of cat_z_vals, renderer.py:179-193). wf16/tab/offs: packed parameters (avatarclip_amd/packing.py). */
int avc_sdf_forward(int net, const float* pts, const float* rays_o, const float* rays_d, const float* z, int S,
                    int ldz, long npts, const void* wf16, const float* tab, const int* offs /* host */,
                    float* sdf_out, const int* slot, int ld_out, void* stream);

/* One step of NeuSRenderer.up_sample + sample_pdf(det=True) + the sort/merge of cat_z_vals
 * (renderer.py:133-177, 39-69, 179-193) for R rays with n current samples, producing m new ones.
 * z_out/sdf_out [R, n+m] receive the merged z and the old sdf values at their merged positions; z_new/slot_new
 * [R,m] the new depths and their positions in the merged row (sdf of those is filled by avc_sdf_forward). */
int avc_upsample_step(const float* rays_o, const float* rays_d, const float* z_in, const float* sdf_in, int R,
                      int n, int m, float inv_s, float* z_out, float* sdf_out, float* z_new, int* slot_new,
                      void* stream);
/* the same with the work distribution as an argument: lanes_per_ray = 0 (chosen from n and m: 16 / 32 lanes per ray for n + m <= 64 /
 * 128, avc_upsample_step's choice) or 64 (one wavefront per ray: the cross-check of the grouped kernels) */
int avc_upsample_step_lanes(const float* rays_o, const float* rays_d, const float* z_in, const float* sdf_in, int R,
                            int n, int m, float inv_s, float* z_out, float* sdf_out, float* z_new, int* slot_new,
                            int lanes_per_ray, void* stream);

/* sdf_network(pts) + sdf_network.gradient(pts) + color_network(...) of render_core (renderer.py:221-232) at the
 * section mid-points of z[R,S] (or at pts[N,3]): sdf[N], normal[N,3] (= d sdf/dx), rgb[N,6] = sigmoid([rgb ; extra]). */
int avc_render_points_fwd(int net, const float* pts, const float* rays_o, const float* rays_d, const float* z,
                          int S, int ldz, float sample_dist, long npts, const void* wf16, const float* tab,
                          const int* offs /* host */, float* sdf_out, float* normal_out, float* rgb_out, long max_waves,
                          void* scratch /* max_waves * avc_fwd_scratch_bytes_per_wave(net) bytes */, void* stream);
/* bytes of the per-wavefront slot in which avc_render_points_fwd parks the trunk activations between the forward and the
 * normal sweep (persistent workgroups of 8 wavefronts; max_waves bounds the resident grid) */
long avc_fwd_scratch_bytes_per_wave(int net);

/* NeuS alpha + compositing of render_core (renderer.py:234-286), one wavefront per ray.
 * bg_mode 0: none, 1: bg[3] shared, 2: bg[R] grey per ray (main.py:387-415); background is composited into
 * `extra` only (renderer.py:277-281).  Outputs: color[R,3], extra[R,3], weights[R,S], cdf[R,S], mid_z[R,S],
 * inside[R,S], eik[R,2] = per-ray (sum relax*(|n|-1)^2, sum relax); optional (NULL = skip) per-ray reductions of the weights
 * that the callers of render() take next: wstat[2][R] = (sum_i w_i, max_i w_i) (renderer.py:391-392 weight_sum / weight_max)
 * and nsum[R,3] = sum_i w_i n_i (the shading normal of main.py:428 before its normalisation). */
int avc_composite_fwd(const float* sdf, const float* normal, const float* rgb, const float* z, const float* rays_o,
                      const float* rays_d, int R, int S, const float* inv_s /* device scalar */, float sample_dist,
                      float cos_anneal, const float* bg, int bg_mode, float* color, float* extra, float* weights,
                      float* cdf, float* mid_z, float* inside, float* eik, float* wstat, float* nsum, void* stream);

/* The scalar reductions around the compositing kernels in one launch each: column sums of x [R,C] (C <= 4) in a fixed order; mode 1
 * (x = avc_composite_fwd's eik): out[1] = sum x[:,1] + 1e-5, out[0] = sum x[:,0] / out[1] = the eikonal term of renderer.py:283-285.
 * avc_inv_s: out[0] = exp(10 variance).clip(1e-6, 1e6), out[1] = 1 / out[0] (fields.py:275-276, renderer.py:234,288); with g != NULL:
 * out[0] = its backward g[0] * d/dv. */
long avc_colsum_scratch_bytes(void);   /* zero-initialised once by the caller; every call leaves its ticket word zero */
int avc_colsum(const float* x, long R, int C, int mode, float* out, void* scratch, void* stream);
int avc_inv_s(const float* variance, const float* g, float* out, void* stream);

/* Reverse of avc_composite_fwd.  Upstream: d_color[R,3], d_extra[R,3], d_weights[R,S] (may be NULL), d_normal_up[R,S,3] (may
 * be NULL), d_wsum[R] / d_nsum[R,3] = gradients of wstat[:,0] / nsum (may be NULL), eik_scale = d(loss)/d(eik) / (sum relax +
 * 1e-5) (device scalar).  Outputs: d_sdf[R,S], d_normal[R,S,3], d_rgb[R,S,6], d_inv_s[R] (per-ray partial of d loss / d inv_s). */
int avc_composite_bwd(const float* sdf, const float* normal, const float* rgb, const float* z, const float* rays_o,
                      const float* rays_d, int R, int S, const float* inv_s, float sample_dist, float cos_anneal,
                      const float* bg, int bg_mode, const float* d_color, const float* d_extra,
                      const float* d_weights, const float* d_normal_up, const float* d_wsum, const float* d_nsum,
                      const float* eik_scale, float* d_sdf, float* d_normal, float* d_rgb, float* d_inv_s, void* stream);

/* The differentiable forward of render_core (renderer.py:221-232, once per iteration as in the reference): the same outputs
 * as avc_render_points_fwd, plus everything the backward pass and the weight-gradient products need from the forward pass,
 * written to the F REGION of the OPERAND PANELS: per 32-point block avc_fwd_panel_tiles(net) tiles of 2 KiB, each tile = the
 * two 16-bit B-operand fragments [k-step][lane = point + 32 half][8 features] of 32 features x 32 points (f16: PE values,
 * h_l, g_a,l, feature vector, [x,n], r1, r2), and the ReLU masks of r1 / r2 (avc_mask_u16_per_block(net) x 16 bits per
 * block: [layer][tile][lane], bit (r >> 1) + 8 (r & 1) = feature row r of the lane's 16 rows is > 0 -- opaque to the caller, the
 * backward kernel is the only reader).  Both buffers need (nblk + 1) blocks, nblk = ceil(npts / 32): the last block is a sink for wavefronts past the end.
 * The gradient-type operands (bf16: gbar_h, abar, delta, ybar) live in a separate G REGION of avc_grad_panel_tiles(net) tiles
 * per block that only ever holds one SLAB of blocks (see avc_render_points_bwd). */
int avc_fwd_panel_tiles(int net);
int avc_grad_panel_tiles(int net);
int avc_mask_u16_per_block(int net);
int avc_render_points_fwd_train(int net, const float* pts, const float* rays_o, const float* rays_d, const float* z,
                                int S, int ldz, float sample_dist, long npts, const void* wf16, const float* tab,
                                const int* offs /* host */, float* sdf_out, float* normal_out, float* rgb_out,
                                long max_waves, void* fpanels, void* masks, void* stream);

/* Backward of avc_render_points_fwd_train wrt every dense weight (autograd incl. the double backward of
 * SDFNetwork.gradient, fields.py:96-107; main.py:537) for one SLAB of npts points (a block-aligned sub-range of the forward's
 * points: the ray / z / gradient pointers and fpanels / masks point at the slab's first ray resp. first block).  Recomputes
 * nothing of the forward: reads h_l, g_a,l (fpanels), the masks and the colours (rgb_fwd = the forward's rgb_out) back, runs
 * the colour backward, the second-order sweep and the reverse sweep (bf16 operands) and writes the gradient-type operand
 * tiles of the slab to gpanels ((nblk + 1) blocks of avc_grad_panel_tiles(net) tiles, block 0 = the slab's first block);
 * avc_weight_grad_all then contracts both regions over the slab's points.  max_waves bounds the resident grid (persistent
 * workgroups of 8 wavefronts).
 * One term of the weight gradient is not a product and does not go through the panels: the second-order term of row 0 of the last
 * SDF layer, dW_last[0, :] += sum_points [gbar_hs ; gbar_h0] / sqrt2 (fields.py:96-107 under main.py:537).  The kernel
 * reduces it over each wavefront's points and writes colsum[avc_bwd_colsum_rows(npts, max_waves)][avc_bwd_colsum_floats(net)]: per row
 * [ST tiles][2 halves][16 accumulator registers] of gbar_hs, then [3 fragments][2 halves][8 slots] of gbar_h0; the caller adds the rows
 * (and the slabs) up and scatters them into the dense gradient (packing.Layout.cs_src / cs_tgt / cs_scale). */
int avc_bwd_colsum_floats(int net);
long avc_bwd_colsum_rows(long npts, long max_waves);
int avc_render_points_bwd(int net, const float* pts, const float* rays_o, const float* rays_d, const float* z,
                          int S, int ldz, float sample_dist, long npts, const void* wbf16, const float* tab,
                          const int* offs /* host */, const float* d_sdf, const float* d_normal, const float* d_rgb,
                          const float* rgb_fwd, const void* fpanels, void* gpanels, const void* masks, float* colsum,
                          long max_waves, void* stream);

/* Every weight-gradient product of one slab in one launch.  pairs (host) = npairs x {pa, ta, pb, tb, out_off, bias_off,
 * type_a, type_b}: pair i contracts A tiles pa .. pa+ta-1 with B tiles pb .. pb+tb-1 (1 <= ta <= 8, 1 <= tb <= 9, or the merged
 * last-layer product ta = tb = 9) over the points of `nblk` blocks; type selects the operand's region and element type: 0 = F
 * region (fpanels, ftiles tiles per block, f16), 1 = G region (gpanels, gtiles per block, bf16), tile indices are
 * region-local.  The tiles are copied to LDS by global->LDS DMA in a chunk order that lets gfx950's LDS transpose read
 * (ds_read_b64_tr_b16) hand every lane its feature-major fragment, f16 operands are converted to bf16 after the read, and the
 * products accumulate in fp32.  partial[split][out_off + ((ta_i * tb + tb_j) * 64 + lane) * 16 + r] = element
 * dW[32 ta_i + (r&3)+8(r>>2)+4h][32 tb_j + n] of lane (n,h); bias_partial[split][bias_off + 32 ta_i + n] = sum_points
 * A[:, 32 ta_i + n] (bias_off < 0: none).  nsplit = split-K factor (grid x); split s writes its slab at
 * partial + s*out_stride (bias_partial + s*bias_stride), floats; the caller sums the slabs (no atomics).  A table that would leave its buffers is refused
 * before the launch (returns 1): types outside {0, 1}, a tile range outside [0, ftiles) resp. [0, gtiles), out_off + ta*tb*1024 >
 * out_stride, bias_off + 32*ta > bias_stride. */
int avc_weight_grad_all(const void* fpanels, int ftiles, const void* gpanels, int gtiles, int npairs,
                        const int* pairs /* host */, long nblk, float* partial, float* bias_partial, int nsplit,
                        int out_stride, int bias_stride, void* stream);

/* What follows avc_weight_grad_all (the tail of main.py:537's backward for the MLP weights): acc [gout_size + gbias_size] (+)= the sum
 * over the nsplit slabs of partial / bias_partial, added in split order (accumulate != 0: on top of acc, i.e. the previous slab of
 * points); then grad[t] = sum_{k = off[t] .. off[t+1]-1} acc[src[k]] * scale[k] maps the products' tile layout back to the dense
 * parameter vector (device tables built from packing.Layout.un_* / ub_*, engine._DevLayout). */
int avc_weight_grad_reduce(const float* partial, const float* bias_partial, int nsplit, int out_stride, int bias_stride, int gout_size,
                           int gbias_size, float* acc, int accumulate, void* stream);
int avc_weight_grad_unpack(const float* acc, const int* off, const int* src, const float* scale, int nparam, float* grad, void* stream);

/* The per-pixel glue between the renderer and CLIP in one launch each way (main.py:426-453 random-light Lambert shading of the rendered
 * normals, :461-487 scatter of the silhouette rays into full images over the augmentation background, :491-492 / :497 the per-pixel terms
 * of the colour L1 and mask BCE losses).  P pixels of the H x W image; ray_of_pixel[P] = the ray of a pixel or -1 (NULL: pixel p = ray p,
 * the full-frame mode); color / extra [R,3], wsum [R], nsum [R,3] = sum_i w_i n_i (NULL: no shading, both images = extra_color);
 * true_rgb [P,3], mask [P] (what the losses use); bg [P] grey background outside the silhouette (NULL: bg_const); light = device
 * [4] (unit light direction, ambience).  Outputs: images [2][P][3] (0 = texture_shading, or extra_color if img0_is_extra; 1 =
 * rand_shading_rgb), partial [avc_shade_loss_blocks(P)][4] = per-block sums of (|color - true| mask, mask, BCE term, (color - true)^2
 * mask: the logged psnr of main.py:493) and sums [4] = their totals, added up in a fixed order by the block that finishes last
 * (ticket: one zero-initialised device word per stream of calls; the kernel leaves it zero).  The backward takes dimg0 / dimg1 [P,3] (NULL:
 * unused image) and gs = device [4], the gradient of `sums` ([0]: d loss / d l1-sum, [2]: d loss / d bce-sum), and writes dcolor / dextra
 * [R,3], dwsum [R], dnsum [R,3] for every ray that owns a pixel. */
int avc_shade_loss_blocks(int P);
int avc_shade_loss_fwd(const float* color, const float* extra, const float* wsum, const float* nsum, const float* true_rgb,
                       const float* mask, const int* ray_of_pixel, const float* bg, float bg_const, const float* light, int P,
                       int img0_is_extra, float* images, float* partial, float* sums, unsigned* ticket, void* stream);
int avc_shade_loss_bwd(const float* color, const float* extra, const float* wsum, const float* nsum, const float* true_rgb,
                       const float* mask, const int* ray_of_pixel, const float* light, int P, int img0_is_extra, const float* dimg0,
                       const float* dimg1, const float* gs, float* dcolor, float* dextra, float* dwsum, float* dnsum, void* stream);
/* engine.Packed in one launch: w_f16 / w_bf16 [n16] = flat[idx16] * scale16 (both 16-bit types), tab [n32] = flat[idx32] * scale32; an
 * index >= nparam reads the appended zero (packing.py: the blobs are pure index gathers of the dense vector, fields.py:65-66,139-143). */
int avc_pack_params(const float* flat, int nparam, const long* idx16, const float* scale16, int n16, const long* idx32,
                    const float* scale32, int n32, void* w_f16, void* w_bf16, float* tab, void* stream);
/* renderer.py:311-322: z [R,n] = near + (far - near) * linspace(0, 1, n) (+ (jitter - 0.5) * 2 / n; jitter [R] or NULL), rounded like
 * the torch ops */
int avc_coarse_z(const float* near_, const float* far_, const float* jitter, int R, int n, float* z, void* stream);
/* The scalar tail of the loss (main.py:491-534) in one launch each way: cos_b = torch.cosine_similarity(torch.mean(enc[b:b+1], 0),
 * torch.mean(text, 0), dim=0) for the B images (enc [B,512], text [T,512]) and
 *   loss = sums[0] / (sums[1] + 1e-5) + eikonal * igr_weight + (sums[2] / P) * mask_weight + sum_b (1 - cos_b) * clip_weight
 * (the reference's order of additions).  loss: device scalar; out [8] = loss, colour loss, mask loss, cos_0 .. cos_{B-1}, 0 (statistics); saved
 * [4 B + 1]: what the backward needs.  The backward takes g = d L / d loss (device scalar) and writes d_enc [B,512] and dd [8]: [0..3] the
 * gradient of sums (what avc_shade_loss_bwd takes as gs), [4] that of the eikonal term. */
int avc_loss_tail_fwd(const float* enc, const float* text, int B, int T, int D, const float* sums, const float* eikonal, float igr_weight,
                      float mask_weight, float clip_weight, float P, float* loss, float* out, float* saved, void* stream);
int avc_loss_tail_bwd(const float* g, const float* enc, const float* text, int B, int T, int D, const float* sums, const float* saved,
                      float igr_weight, float mask_weight, float clip_weight, float P, float* d_enc, float* dd, void* stream);
/* CLIP's preprocessing (main.py:261-267,510-511: RandomResizedCrop(224, scale=(1,1)) of a square image = bilinear resize,
 * align_corners = False, no antialias; Normalize): images [B,H,W,3] -> out [B,3,224,224] = (resize - mean) / std, and its transpose
 * (dimages is overwritten).  mean / std: HOST arrays of 3 floats. */
int avc_resize_norm_fwd(const float* images, int B, int H, int W, const float* mean, const float* stdv, float* out, void* stream);
int avc_resize_norm_bwd(const float* dout, int B, int H, int W, const float* mean, const float* stdv, float* dimages, void* stream);

/* The rays of a view in one launch (dataset.py:277-293 gen_rays_pose: pixel centres linspace(0, W - 1, Wn) x linspace(0, H - 1, Hn) of the
 * dataset's pinhole camera (W, H, focal), direction = pose[:3,:3] p / |p| with p = ((x - W/2) / f, -(y - H/2) / f, -1), origin = pose[:3,3];
 * sel != NULL: only the R listed row-major pixels, the selected rays of gen_rays_silhouettes :252-275) with near / far from the unit
 * sphere (:331-342), and -- prior != NULL -- the prior render [Hp,Wp,3] resampled to the Hn x Wn grid (main.py:376-380: nearest) as
 * true_rgb [Hn*Wn,3] and mask [Hn*Wn] = (true_rgb[..., 0] != 0).  pose: device [16], camera-to-world, row major. */
int avc_gen_rays(const float* pose, const long* sel, const float* prior, int Hp, int Wp, float W, float H, float focal, int Wn, int Hn,
                 int R, float* rays_o, float* rays_d, float* near, float* far, float* true_rgb, float* mask, void* stream);
/* main.py:398-405: the blurred chess-board background of the augmentation, out [H*W] (0.2 / 0.8 squares of chess_length pixels,
 * GaussianBlur kernel (5, 9) with reflect padding; taps = device [14]: the 5 normalised taps along x, then the 9 along y). */
int avc_chess_background(float* out, int H, int W, int chess_length, const float* taps, void* stream);

/* Dense-parameter assembly of one optimisation step: W_l = g_l * v_l / ||v_l||_row (nn.utils.weight_norm, fields.py:65-66,139-143;
 * g[l] == NULL: the plain weight) and the biases of `n` linears written into the flat dense vector `flat` at w_off[l] (row-major
 * [rows, cols]) / b_off[l] (floats), and the backward of that map: dflat -> dv[l], dg[l], db[l] (b[l] / db[l] may be NULL).
 * The arrays of pointers / shapes are HOST arrays (n <= 16). */
int avc_dense_params_fwd(int n, const void* const* v, const void* const* g, const void* const* b, const int* rows,
                         const int* cols, const long* w_off, const long* b_off, float* flat, void* stream);
int avc_dense_params_bwd(int n, const void* const* v, const void* const* g, void* const* dv, void* const* dg, void* const* db,
                         const int* rows, const int* cols, const long* w_off, const long* b_off, const float* dflat,
                         void* stream);

/* ---- mesh extraction (Runner.validate_mesh, main.py:850-919; renderer.py:10-36; mcubes.marching_cubes) ----
 * Marching cubes over u[nx][ny][nz] (row-major, the reference's extract_fields layout) at iso level `iso`, inside = u > iso,
 * one welded vertex per sign-changing grid edge.  Pass 1 writes, per grid point p, the flags of the three edges it owns
 * (vflag[3p + axis]) and the triangle count of the cell whose low corner it is (ccount[p]); the caller turns both into
 * exclusive prefix sums (vid, coff); pass 2 writes vertices (index coordinates, float32: the caller applies
 * renderer.py:35) and triangles (vertex ids).  ntri_table[256], tri_table[256][5][3], edge_table[12][4] = (dx,dy,dz,axis):
 * device copies of avatarclip_amd/mc_tables.py. */
int avc_mc_classify(const float* u, int nx, int ny, int nz, float iso, const int* ntri_table, int* vflag, int* ccount,
                    void* stream);
int avc_mc_emit(const float* u, int nx, int ny, int nz, float iso, const int* vflag, const int* vid, const int* ccount,
                const int* coff, const signed char* tri_table, const int* edge_table, float* verts, int* tris, void* stream);

/* ---- CLIP ViT-B/32 image encoder (perceptor.encode_image, main.py:512,518,524; OpenAI clip/model.py) ----
 * y[M,N] = act(x[M,K] W^T + bias) (+ residual); W pre-packed bf16 [N/32][K/16][64][8] (lane (n,h): W[32t+n][16s+8h+j]).
 * act 1 = QuickGELU (y_pre, if given, receives the pre-activation for the backward).  The backward dX = dY W is the same
 * call with the packed W^T (weights are frozen in AvatarCLIP: main.py:260).  N % 32 == 0, K % 16 == 0.  Up to 128 rows (the
 * per-iteration calls, the text tower's 77) one 8-wavefront split-K workgroup per (32 columns, 32 rows), every combination of the
 * arguments.  More than 128 rows (batched scoring, every ViT-B/16 call, gradient calls of 3+ images) an LDS-staged GEMM, one
 * 4-wavefront workgroup per 128 x 128 output block (csrc/avc_vit_gemm.hip), which covers N % 128 == 0, K % 32 == 0 and no residual
 * together with an activation -- every linear of both CLIP towers, forward and transposed (N, K in {512, 768, 1536, 2048, 2304,
 * 3072}); anything else returns 1 with the condition in avc_last_error(), there is no slower kernel behind it. */
int avc_vit_linear(const float* x, const void* w_packed, const float* bias, const float* residual, float* y,
                   float* y_pre, int M, int N, int K, int act, void* workspace /* avc_vit_workspace_bytes(M, K) */,
                   void* stream);
/* backward through a QuickGELU layer and the linear in front of it in one call: dx[M,N] = (dy[M,K] * gelu'(pre[M,K])) W, with
 * the packed W^T (N = the layer's input width, K = its output width); the activation derivative is applied while dy is packed. */
int avc_vit_linear_bwd_gelu(const float* dy, const float* pre, const void* wt_packed, float* dx, int M, int N, int K,
                            void* workspace, void* stream);
/* bytes of the bf16 fragment copy of x that avc_vit_linear builds in `workspace` */
long avc_vit_workspace_bytes(int M, int K);
/* The 12 residual blocks (clip_vit.BlocksFn: clip/model.py ResidualAttentionBlock as one autograd node; weights frozen, main.py:260)
 * keep the activations between the kernels as packed bf16 operands ([row tile][k-step][lane (row, half)][8], avc_vit_workspace_bytes(M, K)
 * bytes for an [M,K] activation) instead of fp32 rows + a packing pass per linear -- forward AND backward for any M: the batched scoring
 * calls (no gradient, hundreds of images: ShapeGen/main.py:104-128, AvatarAnimate pose_generation.py:79-110), the per-iteration call of
 * the training loop (main.py:512,524: 1-2 images WITH a gradient to the pixels, 50-100 rows of ViT-B/32, 197-394 of ViT-B/16) and the
 * 5-view batches of AvatarAnimate's CLIP-guided optimisers (250 rows and more):
 *   avc_vit_ln_pack               LayerNorm(x[M,768]; gamma, beta, eps) (clip/model.py LayerNorm, fp32 statistics) -> packed
 *   avc_vit_attention_fwd_packed  attention with its output packed for the out-projection (rows = b * T + token; 1 <= T <= 256 as
 *                                 avc_vit_attention_fwd; rows past B * T of the last row tile are not written)
 *   avc_vit_pack                  fp32 rows (optionally times QuickGELU'(gelu_pre)) -> packed operand
 *   avc_vit_linear_packed         y = f(xs W^T + b) (+ residual) from a packed operand; act 0 identity, 1 QuickGELU (y_pre, if given,
 *                                 receives the pre-activation), 2 times QuickGELU'(gelu_pre[M,N]) (backward of a QuickGELU layer; act 2
 *                                 if and only if gelu_pre != NULL); the result leaves as fp32 rows y and / or as the packed operand
 *                                 ys_packed of the next linear (one of the two must be given).  Kernels and shapes as avc_vit_linear:
 *                                 up to 128 rows every combination; more than 128 rows N % 128 == 0, K % 32 == 0, no residual with
 *                                 an activation, with ys_packed neither y nor a residual, y_pre beside ys_packed only with act 1
 *                                 (c_fc of a forward that keeps what its backward reads: nothing of y_pre past row M is written),
 *                                 and act 2 only into ys_packed (c_proj^T of the backward: no row of gelu_pre past M is read, the
 *                                 packed rows past M of the last group of four row tiles are zeros) -- else it returns 1
 *   avc_vit_ln_bwd                dx = (d LayerNorm(x; gamma) / dx)^T dy (+ residual_grad): fp32 rows and, xs_packed != NULL, the packed
 *                                 operand of the transposed linear behind it (statistics recomputed from x, eps as in avc_vit_ln_pack;
 *                                 rows past M of xs_packed are not touched: up to 128 rows the caller's buffer holds zeros there) */
int avc_vit_ln_pack(const float* x, const float* gamma, const float* beta, float eps, int M, int K, void* xs_packed, void* stream);
int avc_vit_linear_packed(const void* xs_packed, const void* w_packed, const float* bias, const float* residual, const float* gelu_pre,
                          float* y, float* y_pre, void* ys_packed, int M, int N, int K, int act, void* stream);
int avc_vit_attention_fwd_packed(const float* qkv, void* out_packed, int B, int T, int width, int heads, void* stream);
int avc_vit_pack(const float* x, const float* gelu_pre, void* xs_packed, int M, int K, void* stream);
/* avc_vit_attention_bwd with dqkv leaving as the packed operand ([B * T, 3 W]; 1 <= T <= 256; T = 50 is ViT-B/32, 197 is ViT-B/16) of
 * the transposed in-projection; rows past B * T of the last row tile are not written (the convention of avc_vit_ln_bwd) */
int avc_vit_attention_bwd_packed(const float* qkv, const float* dout, void* dqkv_packed, int B, int T, int width, int heads, void* stream);
int avc_vit_ln_bwd(const float* dy, const float* x, const float* gamma, float eps, const float* residual_grad, float* dx,
                   void* xs_packed, int M, int K, void* stream);
/* multi-head self-attention of ResidualAttentionBlock over 1 <= T <= 256 tokens (T = 50 is ViT-B/32, 197 is ViT-B/16), head dim 64,
 * width == heads * 64: qkv[B,T,3W] -> out[B,T,W].  bf16 operands on the matrix core, fp32 accumulation and softmax statistics; T = 50
 * runs in one 64-key tile, every other T in 32-key tiles; another T or head dim returns 1.  No atomics: an image's result is the same
 * bits in every run, every batch and at every place in a batch. */
int avc_vit_attention_fwd(const float* qkv, float* out, int B, int T, int width, int heads, void* stream);
/* text tower (perceptor.encode_text, main.py:276-288; clip/model.py): self-attention over T <= 128 tokens, head dim 64, with
 * the causal mask of CLIP's text transformer when `causal` != 0.  Forward only (prompts are encoded once, detached). */
int avc_text_attention_fwd(const float* qkv, float* out, int B, int T, int width, int heads, int causal, void* stream);
/* its backward: dout[B,T,W] -> dqkv[B,T,3W] (q, k, v gradients side by side as in qkv); 1 <= T <= 256 as above, the softmax is recomputed
 * from qkv */
int avc_vit_attention_bwd(const float* qkv, const float* dout, float* dqkv, int B, int T, int width, int heads,
                          void* stream);

/* test hook: one v_mfma_f32_32x32x16_{f16,bf16} on caller-provided per-lane fragments (64 lanes x 8 / x16) */
int avc_probe_mfma(const void* a_f16, const void* b_f16, float* d, const void* a_bf16, const void* b_bf16, float* d_bf,
                   void* stream);

/* The forward pass of neural_renderer as the SMPL prior uses it (AvatarGen/AppearanceGen/models/utils.py:108-125,
 * render_one_batch -> nr.Renderer(camera_mode='look')(vertices, faces, white textures); main.py:360): nearest front-facing
 * face per pixel of an image_size x image_size grid (the caller passes the 2x super-sampled size and average-pools,
 * anti_aliasing=True), value = that face's light intensity, 0 = background.
 * faces[F,9]: per face three vertices (x, y in NDC after look + perspective, z = camera depth), the fill_back copies
 * (reversed vertex order) included by the caller; light[F]: ambient + directional intensity per face
 * (lighting.py, world space).  image[image_size, image_size], row 0 = top (rasterize.py's final flip applied).  scratch: the
 * z-buffer of 64-bit (depth bits, face index) keys the faces race into with atomicMin + the list of the faces too large for that
 * (handled tile by tile) -- avc_rasterize_scratch_bytes(F, image_size) bytes that the caller fills with 0xFF once; every call hands
 * them back that way.
 * All three forward entry points launch one set of kernels (csrc/avc_raster.hip; the face-list form and avc_rasterize_mesh are the N = 1 case of
 * avc_rasterize_mesh_save's), so their images agree to the bit. */
/* The same from the world-space mesh in four launches (projection look.py / perspective.py -> rasteriser at the 2 x super-sampled size on
 * faces gathered through idx [F,3] -> 2 x 2 average, optional x flip (models/utils.py:124) and three equal channels): v_world [V,3], cam =
 * device [12] (eye, x / y / z axis of the look frame), width = tan(viewing angle); ndc [V,3] scratch; out [S,S] or [S,S,3];
 * scratch: avc_rasterize_scratch_bytes(F, 2 S). */
int avc_rasterize_mesh(const float* v_world, int V, const int* idx, int F, const float* cam, float width, const float* light, int S,
                       float near_, float far_, float* ndc, float* out, int flip_x, int channels, void* scratch, void* stream);
long avc_rasterize_scratch_bytes(int F, int image_size);
int avc_rasterize_faces(const float* faces, const float* light, int F, int image_size, float near_, float far_,
                        float* image, void* scratch /* avc_rasterize_scratch_bytes, 0xFF-filled on entry; left so */, void* stream);

/* The differentiable form of the same render, for AvatarAnimate's CLIP-guided optimisers (AvatarAnimate/models/render.py:10-39: the
 * renders of the posed body are differentiated with respect to its vertices).  Backward = the approximate gradient of Kato, Ushiku and
 * Harada, "Neural 3D Mesh Renderer" (CVPR 2018) section 3.3, neural_renderer's published rasteriser backward, restated (DESIGN.md
 * section 8; tests/nr_grad_restatement.py).
 * avc_rasterize_mesh_save: N renders in one call, render i = the world-space mesh v_world[i] [V,3] (one topology idx [F,3], fill_back
 * copies included) seen by camera cam[i] [12] (as avc_rasterize_mesh) with face light light[i] [F].  Outputs: image [N,S,S] (the pooled
 * grey image, no x flip: avc_rasterize_mesh's with flip_x = 0, channels = 1, the same kernels), ndc [N,V,3], fidx int32 [N,2S,2S] = the
 * winning face of every super-sampled pixel, z-buffer orientation (row 0 = bottom), -1 = background.  scratch: N x
 * avc_rasterize_scratch_bytes(F, 2 S) bytes, 0xFF-filled on entry, left so. */
int avc_rasterize_mesh_save(const float* v_world, int N, int V, const int* idx, int F, const float* cam, float width, const float* light, int S,
                            float near_, float far_, float* ndc, float* image, int* fidx, void* scratch, void* stream);
/* avc_rasterize_mesh_grad: grad_image [N,S,S] + the saved ndc / fidx (and light, idx) -> grad_ndc [N,V,3] (z = 0: the pseudo-gradient moves
 * x and y only) and grad_light [N,F] (sum of the pixel gradients over each face's pixels).  eps: neural_renderer's DEFAULT_EPS (1e-4).
 * vf_ptr [V+1] / vf_ent: the vertex -> (3 face + corner) CSR of idx (one per topology); face_grad: scratch of N x F x 6 floats.
 * Deterministic (no float atomics). */
int avc_rasterize_mesh_grad(const float* grad_image, const float* ndc, int N, int V, const int* idx, int F, const float* light, const int* fidx,
                            int S, float eps, const int* vf_ptr, const int* vf_ent, float* face_grad, float* grad_ndc, float* grad_light,
                            void* stream);

/* ---- driving the avatar with a motion (AvatarGen/AppearanceGen/drive.py, generate_animation :308-376; avatarclip_amd/drive.py) ----
 * M = 0 (or T = 0) is a no-op that returns 0.
 * avc_nearest_point: find_nearest_ind (drive.py:235-240): idx[m] = argmin_k ((ref[k] - q[m]) ** 2).sum() for q [M,3], ref [K,3] float32,
 * distances in fp64 with numpy's operation order (subtract, square, (dx^2 + dy^2) + dz^2, no FMA), ties to the lowest k: bit-identical
 * to the reference's np.argmin.  Inputs are finite. */
int avc_nearest_point(const float* q, int M, const float* ref, int K, int* idx, void* stream);
/* cleanup_mesh (drive.py:172-210), the largest island of the triangle-edge graph, in three calls.  Triangles tris [F,3] int32 with a
 * corner outside [0, NV) are ignored (the caller checks them).
 * avc_mesh_components: label [NV] = the smallest vertex index of each vertex's connected component (a vertex in no triangle is its own).
 * avc_mesh_largest_island: the component to keep -- the most vertices, a tie to the smallest label (the reference's BFS order with its
 * strict `>`) -- as vflag [NV] and tflag [F] (1 = kept, int32); count [NV] int32 and best (one 64-bit word) are scratch.
 * avc_mesh_compact: with vid / tid = the exclusive prefix sums of vflag / tflag (the caller's scan): v_out [vid[v]] = v [v] (float32 x 3),
 * c_out [vid[v]] = colors [v] (one 32-bit RGBA word per vertex; colors may be NULL), t_out [tid[f]] = vid[tris[f]]: order kept. */
int avc_mesh_components(const int* tris, int F, int NV, int* label, void* stream);
int avc_mesh_largest_island(const int* tris, int F, int NV, const int* label, int* count, unsigned long long* best, int* vflag, int* tflag,
                            void* stream);
int avc_mesh_compact(const float* v, const unsigned* colors, const int* tris, int F, int NV, const int* vflag, const int* vid, const int* tflag,
                     const int* tid, float* v_out, unsigned* c_out, int* t_out, void* stream);
/* inv_lbs / lbs (drive.py:242-265) with one transform per TEMPLATE vertex: out [T,M,3] with out[t,m] = xf[t, idx[m]] (p[m], 1), where
 * xf [T,K,12] float32 = rows 0..2 of the 4 x 4 per-template transforms (the inverses for the unposing, T = 1), idx [M] int32 (from
 * avc_nearest_point), p [M,3].  xf and out 16-byte aligned.  Contract: every idx in [0, K); an index outside writes NaN for that vertex and
 * reads nothing (avatarclip_amd/drive.py checks idx before the call). */
int avc_skin_apply(const float* xf, const int* idx, const float* p, int M, int K, int T, float* out, void* stream);

/* ---- rigging the avatar (Avatar2FBX/export_fbx.py:49-109, utils/ply_utils.py; avatarclip_amd/rig.py, csrc/avc_rig.hip) ----
 * Empty inputs are no-ops that return 0.  No float atomics: every result is bit-identical from run to run.
 *
 * simplify_mesh (ply_utils.py:16-19, open3d's simplify_vertex_clustering with contraction Average) in three calls around the caller's
 * sort and scan.
 * avc_rig_cell_keys: keyed [N] = (cell key << 32 | vertex index), cell = floor((v - origin) / voxel_size) per axis in fp64 (these two
 * operations, in this order), 10 bits per axis: voxel_divisor in [1, AVC_RIG_MAX_DIVISOR] (indices lie in [0, voxel_divisor + 1]).
 * avc_rig_cluster_heads: sorted = keyed in ascending order; first_flag [N] = 1 for the first (lowest) vertex of every cell, else 0.
 * avc_rig_cluster_average: first_rank = the exclusive prefix sum of first_flag (the caller's scan; M = its total): the cell whose first
 * vertex is v becomes output vertex first_rank[v], so the outputs are in the order the cells are first met walking the input.  v_out [M,3]
 * = the fp64 mean of the cell's vertices, summed in increasing input index, rounded to float32; c_out [M,3] float32 = the fp64 mean of
 * c / 255 likewise (colors: csize = 3 or 4 bytes per vertex, the first three used; NULL: no colours); vmap [N] = each vertex's output. */
#define AVC_RIG_MAX_DIVISOR 1022
int avc_rig_cell_keys(const float* v, int N, double ox, double oy, double oz, double voxel_size, int voxel_divisor, long long* keyed,
                      void* stream);
int avc_rig_cluster_heads(const long long* sorted, int N, int* first_flag, void* stream);
int avc_rig_cluster_average(const long long* sorted, int N, const float* v, const unsigned char* colors, int csize, const int* first_rank,
                            int M, float* v_out, float* c_out, int* vmap, void* stream);
/* The triangles of the clustered mesh (open3d's rules: a triangle with two corners in one cell is dropped, the others are rotated so
 * that their smallest index comes first, exact duplicates are removed, opposite orientations both stay).
 * avc_rig_tri_keys: tri_out [F,3] = the mapped, rotated triangle; key [F] = a << 42 | b << 21 | c, or AVC_RIG_TRI_DROP for a dropped one
 * (also one naming a vertex outside [0, N)).  M <= AVC_RIG_MAX_KEYED_VERTICES = 2^21, else an error: three indices must fit 63 bits.
 * avc_rig_tri_unique: sorted_key / order = the keys sorted STABLY and the permutation that sorts them (int64): tflag [F] = 1 for the
 * first input occurrence of every surviving triangle.
 * avc_rig_tri_compact: tid = the exclusive prefix sum of tflag, F_out its total: t_out [tid[f]] = tri_out [f], input order kept. */
#define AVC_RIG_MAX_KEYED_VERTICES (1 << 21)
#define AVC_RIG_TRI_DROP 0x7FFFFFFFFFFFFFFFLL
int avc_rig_tri_keys(const int* tris, int F, int N, const int* vmap, int M, int* tri_out, long long* key, void* stream);
int avc_rig_tri_unique(const long long* sorted_key, const long long* order, int F, int* tflag, void* stream);
int avc_rig_tri_compact(const int* tri_in, int F, const int* tflag, const int* tid, int F_out, int* t_out, void* stream);
/* The skin (export_fbx.py:73 the gather of the nearest template vertex's blend weights, :88 the permute to [24, M]) and its packing
 * into glTF's JOINTS_n / WEIGHTS_n.  weights [K,24] float32 = SMPL's lbs_weights.
 * avc_skin_sort_template: per template vertex its non-zero weights sorted by weight descending, then joint ascending: tj [K,24] uint8
 * and tw [K,24] float32 (unused slots: joint 0, weight 0), count [K].  keep > 0: only the `keep` largest, divided by their float32 sum.
 * avc_skin_pack: joints [sets,M,4] uint8 and wout [sets,M,4] float32 = the first 4 * sets entries of the list of nearest[m]; blend_weights
 * [24,M] (may be NULL) = weights[nearest[m], j].  sets <= 6.  A nearest index outside [0, K) writes zeros and reads nothing. */
int avc_skin_sort_template(const float* weights, int K, int keep, unsigned char* tj, float* tw, int* count, void* stream);
int avc_skin_pack(const float* weights, const unsigned char* tj, const float* tw, int K, const int* nearest, int M, int sets,
                  unsigned char* joints, float* wout, float* blend_weights, void* stream);
/* The animation tracks (the reference's TODO "Add animation", fbx_utils.py:320): R [n,3,3] float32 rotation matrices -> q [n,4] unit
 * quaternions (x, y, z, w) with w >= 0, Shepperd's method in fp64, rounded to float32.  q 16-byte aligned. */
int avc_rot_to_quat(const float* R, long n, float* q, void* stream);

/* ---- looking at the results (avatarclip_amd/preview.py, csrc/avc_preview.hip; tests/preview_restatement.py restates every rule) ----
 * A batched, z-buffered, vertex-colour triangle renderer of this project's own (no counterpart in the reference, which renders through
 * pyrender): exact integer coverage and depth, a watertight top-left fill rule, both windings drawn.  Not neural_renderer's rules -- those
 * stay with avc_rasterize_*.  A plain launch chain on the caller's stream; no float atomics: bit-identical from run to run.  N = 0 is a
 * no-op that returns 0; at most 65535 frames a call.  R = raster size = S * ss <= AVC_PREVIEW_MAX_RASTER, larger sizes are an error.
 *
 * avc_preview_project: v [N,V,3] float32 world space, cams [N,12] (eye, x / y / z axis of the look frame: the layout of avc_rasterize_mesh),
 * width = tan(fov / 2), 0 < near < far -> proj [N,V] of four int32 (16-byte aligned): X, Y, Z, bits of the float32 1 / c_z.  In fp64, one
 * rounded operation each, no FMA: d = v - eye; c_j = (d0 a_j0 + d1 a_j1) + d2 a_j2; s = c_z width; X = floor((c_x / s + 1) (R / 2) 256 + 0.5),
 * Y = floor((1 - c_y / s) (R / 2) 256 + 0.5) (8 sub-pixel bits, y down: row 0 is the top row, the centre of pixel (i, j) is
 * (256 i + 128, 256 j + 128)); Z = floor(((c_z - near) far) / (c_z (far - near)) (2^24 - 1) + 0.5) (24 bits of NDC z).  A vertex is invalid
 * (Z = -1) unless near < c_z <= far and -2^16 <= X, Y <= 256 R + 2^16 (a guard band of 256 raster pixels).
 * A FACE WITH AN INVALID VERTEX IS DROPPED, NOT CLIPPED: a camera inside the mesh, or nearer to it than `near`, loses whole faces.
 * preview.frame_cameras never produces one for the whole mesh; a close-up or a caller's own camera can.  csrc/avc_preview_clip.h declares
 * avc_preview_raster_clip / avc_preview_shade_clip, which take the place of the two calls below and CLIP such a face instead.
 *
 * avc_preview_raster: tris [F,3] int32 (a corner outside [0, V) drops the face).  Oriented area2 = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0):
 * 0 skips the face, < 0 swaps vertices 1 and 2 (no back-face culling).  Edge i (opposite vertex i) runs a -> b: 1 -> 2, 2 -> 0, 0 -> 1;
 * w_i(p) = (bx - ax)(py - ay) - (by - ay)(px - ax) in int64 at the pixel centre p; covered <=> w_i >= 0 for all i and w_i > 0 for every
 * edge that is not top-left (top-left: by < ay, or by == ay and bx > ax).  depth = floor((w_0 Z_0 + w_1 Z_1 + w_2 Z_2) / area2); the
 * winner of a pixel is the minimum of (depth << 32 | face), by 64-bit atomicMin: nearest face, ties to the lower face index.  No int64
 * product overflows up to AVC_PREVIEW_MAX_RASTER (the proof is in csrc/avc_preview.hip).  Faces whose box holds more than 1024 pixel centres
 * are handled per (face, 16 x 16 tile).  scratch: N x avc_preview_scratch_bytes(F, R) bytes (-1: a size outside the limits), 8-byte
 * aligned, which the caller fills with 0xFF once; avc_preview_shade hands them back that way.
 *
 * avc_preview_shade: image uint8 [N,S,S,3], row 0 = top.  Per raster pixel the winner's weights are recomputed; colour = sum_i l_i c_i /
 * sum_i l_i with l_i = w_i * (1 / c_z of vertex i) (perspective-correct) from colors uint8 [V,csize] (csize 3 or 4, the first three
 * used), or the constant `grey` (0..255) when colors is NULL; times the face's flat two-sided shade ambient + (1 - ambient) |n . l| /
 * (|n| |l|), n = (v1 - v0) x (v2 - v0) in world space, l = lights [N,3] (no direction in either: ambient alone); the background
 * (bg_r, bg_g, bg_b; 0..255) elsewhere; then the ss x ss box average (ss = 1 or 2), floor(x + 0.5), clamped.  face_ids (may be NULL): int32 [N,R,R], the
 * winning face of every raster pixel, -1 = background, row 0 = top. */
#define AVC_PREVIEW_MAX_RASTER 2048
long avc_preview_scratch_bytes(int F, int raster_size);
int avc_preview_project(const float* v, int N, int V, const float* cams, float width, float near_, float far_, int raster_size, int* proj,
                        void* stream);
int avc_preview_raster(const int* proj, int N, int V, const int* tris, int F, int raster_size, void* scratch, void* stream);
int avc_preview_shade(const int* proj, const float* v, int N, int V, const int* tris, int F, const unsigned char* colors, int csize,
                      const float* lights, float ambient, float bg_r, float bg_g, float bg_b, float grey, int S, int ss, void* scratch,
                      unsigned char* image, int* face_ids, void* stream);
/* Four-influence linear blend skinning, for playing a .glb back: out [T,M,3], out[t,m] = sum_k weights[m,k] (joint_mats[t, joints[m,k]]
 * (rest[m], 1)), k = 0..3 in this order, float32.  joints uint8 [M,4] (4-byte aligned), weights float32 [M,4] and joint_mats [T,J,12] =
 * rows 0..2 of the 4 x 4 joint matrices (both 16-byte aligned), rest [M,3].  1 <= J <= 256.  Contract: every joint below J; one outside
 * writes NaN for that vertex and reads nothing.  (avc_skin_apply is a different thing: ONE template transform per vertex.) */
int avc_skin_blend4(const unsigned char* joints, const float* weights, const float* joint_mats, const float* rest, int M, int J, int T,
                    float* out, void* stream);

/* ---- posing the SMPL body without a gradient (avatarclip_amd/smpl_lbs.py pose_hip, csrc/avc_smpl.hip) ----
 * The forward of smpl_lbs.lbs (models/utils.py:176-224 with batch_rodrigues :72-106 and smplx's batch_rigid_transform) as two launches, for
 * the previews the reference renders from smplx's vertices (AvatarAnimate/visualize.py:98-102 render_pose, :115-119 render_motion).  fp32,
 * every multiply-add one fused operation in the order csrc/avc_smpl.h's header states, no atomics: a frame's result is the same bits in
 * every run, every batch and at every place in a batch.  T = 0 (or V = 0) returns 0 without a launch; a NULL or misaligned buffer is an error.
 *
 * avc_smpl_joint_mats: pose [T,24,3] axis-angle, joints [24,3] rest joints (J_regressor v_shaped, computed by the caller), parents int32 [24]
 * with 0 <= parents[i] < i for i >= 1 (parents[0] is not read) -> feat [T,207] = (R_j - I), j = 1..23, row-major (lbs's pose_feature) and
 * A [T,24,12] (16-byte aligned) = rows 0..2 of the rest-pose-relative joint transforms.  R = I + sin K + (1 - cos) K^2 with
 * angle = |r + 1e-8| and K from r / angle (batch_rodrigues, its quirk at tiny angles kept); world_i = world_parent(i) [R_i | j_i - j_parent(i)],
 * A_i = world_i - [0 | world_i.R j_i].  Contract: the caller checks the tree; a joint whose parent does not come before it gets NaN and reads
 * nothing.
 *
 * avc_smpl_pose: v_shaped [V,3], posedirs [207, 3V], weights [V,24] dense (16-byte aligned), feat and A (16-byte aligned) as above ->
 * out [T,V,3]: v_posed[t,v] = (sum_k feat[t,k] posedirs[k, 3v..3v+2]) + v_shaped[v], k ascending from 0; M = sum_j weights[v,j] A[t,j],
 * j ascending from 0; out[t,v] = M (v_posed[t,v], 1).  Any T: the wrapper splits what one grid does not take. */
int avc_smpl_joint_mats(const float* pose, const float* joints, const int* parents, int T, float* feat, float* A, void* stream);
int avc_smpl_pose(const float* v_shaped, const float* posedirs, const float* weights, const float* feat, const float* A, int V, int T,
                  float* out, void* stream);

/* ---- the gradient of posing the SMPL body with respect to the pose (avatarclip_amd/smpl_lbs.py pose_hip_grad, csrc/avc_smpl_grad.hip) ----
 * The exact adjoint of avc_smpl_joint_mats + avc_smpl_pose, to the POSE only: v_shaped, the rest joints and the SMPL arrays are
 * constants.  fp32, every multiply-add one fused operation in the order csrc/avc_smpl_grad.hip's header states, no atomics: every sum over
 * vertices is a fixed tree that depends on V only, so a frame's gradient is the same bits in every run, every batch and at every place in a
 * batch.  T = 0 (or V = 0) returns 0 without a launch; a NULL or misaligned buffer is an error.  Shapes as above: v_shaped [V,3], posedirs
 * [207, 3V], weights [V,24] dense, feat [T,207] and A [T,24,12] as avc_smpl_joint_mats wrote them, pose [T,24,3], joints [24,3], parents int32
 * [24] with 0 <= parents[i] < i. */

/* bytes of avc_smpl_grad_tiles' scratch: ceil(V / 256) vertex tiles x T frames x (24 x 12 + 207) floats */
long avc_smpl_grad_scratch_bytes(int V, int T);

/* The adjoint of lbs's skinning and pose blend shapes (smpl_lbs.py:50-56, lbs: `v_posed = pose_feature posedirs + v_shaped`, `T = W A`,
 * `verts = T (v_posed, 1)`), per tile of 256 vertices x 8 frames.  g [T,V,3] = dL/d out.  v_posed is RECOMPUTED from feat (the forward saves
 * nothing of size [T,V,..]), M = sum_j weights[v,j] A[t,j] rebuilt as avc_smpl_pose does, and
 *   g_vp[t,v] = M.R^T g[t,v]                                               (dL/d v_posed; written to g_vp [T,V,3] unless g_vp is NULL)
 *   dA[t,j]   = sum_v weights[v,j] g[t,v] (x) (v_posed[t,v], 1)             (3 x 4; the tile's vertices in index order)
 *   dfeat[t,k] = sum_e posedirs[k,e] g_vp[t,e]                              (the tile's 768 elements in a fixed butterfly)
 * The tile's dA and dfeat go to scratch [vertex tile][T][24 x 12 + 207] (avc_smpl_grad_scratch_bytes; every float of it is written).
 * weights and A 16-byte aligned.  posedirs is read twice per 8 frames.  Any T: the wrapper splits what one grid does not take. */
int avc_smpl_grad_tiles(const float* v_shaped, const float* posedirs, const float* weights, const float* feat, const float* A, const float* g,
                        int V, int T, float* g_vp, float* scratch, void* stream);

/* The sums over vertices of lbs's two matmuls (smpl_lbs.py:51, :54), finished: dA [T,24,12] (16-byte aligned) and dfeat [T,207] = the vertex tiles'
 * partial sums of avc_smpl_grad_tiles' scratch (same V and T) added in tile order. */
int avc_smpl_grad_reduce(const float* scratch, int V, int T, float* dA, float* dfeat, void* stream);

/* The adjoint of batch_rigid_transform (smpl_lbs.py:25-42), of lbs's `pose_feature = rot_mats[:, 1:] - ident` (:50) and of batch_rodrigues
 * (:11-22, its `+ epsilon` under the norm included), one lane per frame: dA (16-byte aligned) and dfeat as above -> dpose [T,24,3] = dL/d pose.  With W_i the world
 * transform of joint i, q its parent, rel_i = j_i - j_q:  dW_i = [dA_i.R - dA_i.t (x) j_i | dA_i.t];  for i = 23..1:
 * dR_i = W_q.R^T dW_i.R + dfeat[t, 9 (i - 1) .. + 8],  dW_q.R += dW_i.R R_i^T + dW_i.t (x) rel_i,  dW_q.t += dW_i.t;  dR_0 = dW_0.R;  then
 * with e = r + 1e-8, a = |e|, K = skew(r / a):  dK = sin a dR + (1 - cos a)(dR K^T + K^T dR),  dd = (dK21 - dK12, dK02 - dK20, dK10 - dK01),
 * da = <dR, K> cos a + <dR, K^2> sin a - (dd . r) / a^2,  dr = dd / a + da e / a.  Contract: the caller checks the tree; a joint whose parent
 * does not come before it gets NaN and reads nothing. */
int avc_smpl_grad_chain(const float* pose, const float* joints, const int* parents, const float* dA, const float* dfeat, int T, float* dpose,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
