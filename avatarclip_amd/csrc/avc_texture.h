/* avc_texture.h -- the textured-render entry points of libavc.so (csrc/avc_raster_tex.hip), a second part of the C ABI of include/avc.h.
 *
 * Same conventions as include/avc.h: every pointer is a DEVICE pointer, buffers are caller-allocated, `stream` is a hipStream_t, the calls
 * enqueue and return without synchronising, 0 = ok, otherwise avc_last_error() describes the failure.  The interface revision is that header's
 * AVC_ABI_VERSION (4; avc_version() reports it): added entry points do not change it.  avatarclip_amd/lib.py parses both headers and binds
 * the union of their prototypes.
 */
#ifndef AVC_TEXTURE_H
#define AVC_TEXTURE_H
#ifdef __cplusplus
extern "C" {
#endif

/* avc_rasterize_mesh_save with neural_renderer's texture sampling, for the renders the reference scores: AvatarAnimate/models/render.py:6-35
 * and AvatarGen/ShapeGen/utils.py:6-28 hand nr.Renderer the [F,ts,ts,ts,3] texture cubes that nr.load_obj(data/smpl_uv.obj,
 * load_texture=True, texture_size=8) made (avatarclip_amd/texture.py restates that loader).  Inputs as avc_rasterize_mesh_save (include/avc.h)
 * + textures [Ft,ts,ts,ts,3] fp32: F = Ft, or F = 2 Ft where face f >= Ft (a fill_back copy, vertex order reversed) reads the cube of f - Ft
 * with axes 0 and 2 swapped; 2 <= ts <= 256; eps = 1e-4 (neural_renderer's).  Coverage and depth are the grey entry point's launches, so ndc
 * and fidx are its bits.  Per super-sampled pixel won by face f with clamped barycentrics w_k (sum ws) and depth zp as the coverage computes
 * them: t_k = w_k / ws * (ts - 1) * (zp / z_k), clamped to [0, ts - 1 - eps]; i_k = (int)t_k, r_k = t_k - i_k; unlit colour U_c = sum over pn
 * = 0..7 ascending of prod_k (bit k of pn ? r_k : 1 - r_k) * cube[i0 + b0][i1 + b1][i2 + b2][c]; background U = 0; lit colour light[f] * U_c.
 * Outputs: ndc [N,V,3], fidx int32 [N,2S,2S] and unlit [N,2S,2S,3] in z-buffer orientation (row 0 = bottom), image [N,S,S,3] = the lit colours'
 * 2 x 2 average ((a + b) + c) + d, / 4, rows flipped (row 0 = top), no x flip.  scratch: N x avc_rasterize_scratch_bytes(F, 2 S) bytes,
 * 0xFF-filled on entry, left so. */
int avc_rasterize_mesh_tex_save(const float* v_world, int N, int V, const int* idx, int F, const float* cam, float width, const float* light,
                                const float* textures, int Ft, int ts, float eps, int S, float near_, float far_, float* ndc, float* image,
                                float* unlit, int* fidx, void* scratch, void* stream);
/* its backward, avc_rasterize_mesh_grad's rules (neural_renderer's approximate gradient, which AvatarAnimate/models/render.py:10-39
 * differentiates the textured renders with) with the colour C = light[I] * U of the saved unlit map (0 on background):
 * grad_image [N,S,S,3]; every Delta = sum over c ascending of (C_c(w) - C_c(w_ref)) G_c(w); grad_light[f] = sum over f's pixels of sum_c G_c
 * U_c; grad_ndc z = 0.  Nothing flows through the sampling weights and the cubes get no gradient, as in neural_renderer.  eps here is the
 * backward's (DEFAULT_EPS 1e-4).  vf_ptr / vf_ent / face_grad as avc_rasterize_mesh_grad.  Deterministic (no float atomics). */
int avc_rasterize_mesh_tex_grad(const float* grad_image, const float* ndc, int N, int V, const int* idx, int F, const float* light,
                                const float* unlit, const int* fidx, int S, float eps, const int* vf_ptr, const int* vf_ent, float* face_grad,
                                float* grad_ndc, float* grad_light, void* stream);

#ifdef __cplusplus
}
#endif
#endif
