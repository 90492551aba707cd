// Preview renderer (avatarclip_amd/preview.py): a batched, z-buffered, vertex-colour triangle renderer for looking at what the pipeline
// writes -- Runner.validate_mesh's .ply, drive's .pc2 frames, rig's .glb.  NOT neural_renderer's rules (csrc/avc_raster.hip keeps those
// for the SMPL prior and the CLIP-guided optimisers): coverage and depth here are exact integer arithmetic with a watertight fill rule,
// so the winning face of every pixel is a pure function of the inputs, the same on every run and on every machine, and
// tests/preview_restatement.py can be matched with no tolerance.  A plain launch chain on the caller's stream: no graphs, no extra
// streams, no float atomics (the only atomics are 64-bit integer minima and the append to the large-face list).
//
// 1. avc_preview_project, N frames x V vertices, fp64 without fused multiply-adds (every operation below is one correctly rounded IEEE
//    operation, in this order):
//      d = v - eye;   c_j = (d0 a_j0 + d1 a_j1) + d2 a_j2  for the look frame's axes j = x, y, z;   s = c_z * width
//      px = (c_x / s + 1) * (R / 2),   py = (1 - c_y / s) * (R / 2)          R = raster size; y DOWN: row 0 is the top row
//      X = floor(px * 256 + 0.5),  Y likewise                                 8 sub-pixel bits; pixel (i, j)'s centre is (256 i + 128, 256 j + 128)
//      Z = floor(((c_z - near) * far) / (c_z * (far - near)) * (2^24 - 1) + 0.5)   24 bits of NDC z: 0 at near, 2^24 - 1 at far
//      1/w = (float)(1 / c_z)
//    A vertex is INVALID (Z = -1) unless near < c_z <= far and -PV_GUARD <= X, Y <= 256 R + PV_GUARD (NaN fails the comparisons).
//    A face with an invalid vertex is dropped, not clipped (csrc/avc_preview_clip.hip clips it: the same device functions, csrc/avc_preview.h).
// 2. avc_preview_raster.  A face is oriented first: area2 = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0); 0: skipped; < 0: vertices 1 and 2
//    change places (both windings are drawn, the depth test alone decides visibility).  With edge i the one opposite vertex i, from a to b
//    (edge 0: 1 -> 2, edge 1: 2 -> 0, edge 2: 0 -> 1), the weight of a pixel centre p is w_i = (bx - ax)(py - ay) - (by - ay)(px - ax)
//    (w_0 + w_1 + w_2 = area2 > 0) and p is covered when every w_i >= 0 and w_i > 0 for the edges that are not top-left; edge a -> b is
//    top-left when by < ay (a left edge: y is down and the interior is where w > 0) or by == ay and bx > ax (a top edge).  Two faces that
//    share an edge walk it in opposite directions once oriented, so exactly one of them owns the pixel centres on it.
//    depth = floor((w_0 Z_0 + w_1 Z_1 + w_2 Z_2) / area2) (NDC z is affine in screen space); the pixel's winner is the minimum of the
//    key (depth << 32 | face): the nearest face, a tie to the lower face index, whatever order the atomics arrive in.
//    NO int64 OVERFLOW at R <= AVC_PREVIEW_MAX_RASTER = 2048 with PV_GUARD = 2^16 (256 raster pixels each way):  every valid coordinate
//    and every pixel centre lies in [-2^16, 2^19 + 2^16], a span D = 2^19 + 2^17 = 655 360.  Every factor of an edge function is a
//    coordinate difference, |.| <= D < 2^20 (an int32); every product <= D^2 = 429 496 729 600 < 2^39; an edge function is twice the
//    signed area of a triangle with its corners in a D x D box, so |w_i| <= D^2 and area2 <= D^2 too.  The depth sum is taken at covered
//    pixels only, where all w_i >= 0: every term and every partial sum is <= (w_0 + w_1 + w_2) (2^24 - 1) = area2 (2^24 - 1) < 2^39 2^24
//    = 2^63.  The floor division is done as trunc(sum * (1.0 / area2)) in fp64 (off by at most one: the quotient is below 2^24 and the
//    two roundings move it by less than 2^-26) followed by an exact integer correction with q area2 <= sum < 2^63.
//    Work split: one lane sets up one face.  A face whose box holds at most PV_SERIAL pixel centres (most faces of a dense mesh hold none)
//    is finished by its own lane; a box of up to PV_LARGE centres is walked by the whole wavefront, lanes = pixels, one such face after
//    the other (ballot + broadcast of the face index); a larger box is only listed, and a tile-parallel launch gives every 16 x 16 tile of
//    every frame a scan over that frame's list -- each (face, tile) pair is one workgroup's 256 lanes, and a face that fills the view
//    costs what one tile costs.  PV_LARGE = 1024 is avc_raster.hip's threshold, which was measured for THAT kernel (16 trips of one
//    wavefront before a face is worth a whole launch's attention); here it is reasoned, not measured.
//    64-bit atomicMin is one global_atomic_umin_x2 per covered pixel, executed at the memory side; a pixel has as many as the mesh has
//    layers there (depth complexity 2-4 for a body), so the raster's atomic traffic is a few times 8 B per covered pixel.
// 3. avc_preview_shade, one lane per OUTPUT pixel: for each of its ss x ss raster pixels the winner's weights are recomputed (the same
//    integers), colour = sum_i (w_i / w'_i) c_i / sum_i (w_i / w'_i) with the saved 1 / w' of the three corners (perspective-correct),
//    times the face's flat two-sided shade ambient + (1 - ambient) |n . l| / (|n| |l|) (n = the world-space face normal, l = the frame's
//    light direction; a face or a light without direction: ambient alone); background pixels take the constant background; the box is
//    averaged and rounded to nearest (floor(x + 0.5), clamped to [0, 255]).  The keys are set back to all-ones on the way, the large-face
//    lists by one strided fill after it: the scratch leaves as it came, every byte 0xFF.
// 4. avc_skin_blend4: out[t, m] = sum_k weights[m, k] (joint_mats[t, joints[m, k]] (rest[m], 1)), k = 0..3 in this order, fp32.
#include "avc_preview.h"         // the device functions shared with csrc/avc_preview_clip.hip: set-up, weights, key, the passes' pieces
#include "../../include/avc.h"
#include "avc_bake.h"            // avc_preview_shade_tex
#include <stdio.h>

#pragma clang fp contract(off)   // the projection must be the restatement's operation by operation

// ------------------------------------------------------------------------------------------------------------- projection
__global__ __launch_bounds__(PV_THREADS) void pv_project_kernel(const float* __restrict__ v, int V, const float* __restrict__ cams, double width,
                                                                double near, double far, int R, i4* __restrict__ proj) {
  const int i = blockIdx.x * PV_THREADS + threadIdx.x, n = blockIdx.y;
  if (i >= V) return;
  double c[3];
  pv_camera_point(v + 3 * ((long)n * V + i), cams + 12 * (long)n, c);
  i4 o = {0, 0, -1, 0};
  if (c[2] > near && c[2] <= far) {
    double X, Y, Z;
    pv_snap(c[0], c[1], c[2], width, near, far, R, X, Y, Z);
    const double hi = 256.0 * (double)R + (double)PV_GUARD;
    if (X >= -(double)PV_GUARD && X <= hi && Y >= -(double)PV_GUARD && Y <= hi)
      o = i4{(int)X, (int)Y, (int)Z, (int)__float_as_uint((float)(1.0 / c[2]))};
  }
  proj[(long)n * V + i] = o;
}

// ------------------------------------------------------------------------------------------------------------- raster
__global__ __launch_bounds__(PV_THREADS) void pv_raster_kernel(const i4* __restrict__ proj_all, const int* __restrict__ tris, int F, int V, int R,
                                                               void* __restrict__ scratch, long stride) {
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const int f = blockIdx.x * PV_THREADS + threadIdx.x;
  const i4* proj = proj_all + (long)n * V;
  unsigned long long* zbuf = pv_zbuf(scratch, stride, n);
  unsigned* large = (unsigned*)(zbuf + (long)R * R);
  PvFace e;
  const bool ok = f < F && pv_setup(proj, tris, f, V, R, e);
  const int cnt = ok ? pv_centres(e) : 0;
  if (ok && cnt <= PV_SERIAL) pv_walk(e, f, 0, 1, R, zbuf);
  if (ok && cnt > PV_LARGE) pv_list(large, F, f);
  unsigned long long todo = __ballot(ok && cnt > PV_SERIAL && cnt <= PV_LARGE);             // wave-uniform from here on
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int fs = __shfl(f, src);
    PvFace g;
    if (!pv_setup(proj, tris, fs, V, R, g)) continue;                                       // (it passed in lane src: never taken)
    pv_walk(g, fs, lane, 64, R, zbuf);
  }
}

// the listed faces, tile-parallel: lane = pixel of a 16 x 16 tile of frame blockIdx.z; the running minimum joins the key the other
// faces left (plain read-modify-write: one lane per pixel, and the launch above has finished)
__global__ __launch_bounds__(PV_THREADS) void pv_large_kernel(const i4* __restrict__ proj_all, const int* __restrict__ tris, int F, int V, int R,
                                                              void* __restrict__ scratch, long stride) {
  const int n = blockIdx.z;
  const i4* proj = proj_all + (long)n * V;
  unsigned long long* zbuf = pv_zbuf(scratch, stride, n);
  const unsigned* large = (const unsigned*)(zbuf + (long)R * R);
  unsigned nl = large[0] + 1u;
  if (nl == 0u) return;
  if (nl > (unsigned)F) nl = (unsigned)F;
  const int tx0 = blockIdx.x * PV_TILE, ty0 = blockIdx.y * PV_TILE;
  const int xi = tx0 + (threadIdx.x & 15), yi = ty0 + (threadIdx.x >> 4);
  const bool inside = xi < R && yi < R;
  unsigned long long best = PV_EMPTY;
  for (unsigned q = 0; q < nl; ++q) {
    const int f = (int)large[1 + q];
    if ((unsigned)f >= (unsigned)F) continue;
    PvFace e;
    if (!pv_setup(proj, tris, f, V, R, e)) continue;
    pv_tile_key(e, f, tx0, ty0, xi, yi, inside, best);
  }
  if (inside && best != PV_EMPTY) {
    unsigned long long* z = &zbuf[(long)yi * R + xi];
    if (best < *z) *z = best;
  }
}

extern "C" long avc_preview_scratch_bytes(int F, int raster_size) {
  if (F < 0 || raster_size <= 0 || raster_size > AVC_PREVIEW_MAX_RASTER) return -1;
  return (long)raster_size * raster_size * 8 + (((long)F + 2) * 4 + 7) / 8 * 8;
}

extern "C" int avc_preview_project(const float* v, int N, int V, const float* cams, float width, float near, float far, int raster_size,
                                   int* proj, void* stream) {
  if (N < 0 || V < 0 || N > 65535) { avc_set_error("avc_preview_project: bad sizes (at most 65535 frames a call)"); return 1; }
  if (raster_size <= 0 || raster_size > AVC_PREVIEW_MAX_RASTER) { avc_set_error("avc_preview_project: raster size outside [1, 2048]"); return 1; }
  if (!(width > 0.f) || !(near > 0.f) || !(far > near)) { avc_set_error("avc_preview_project: needs width > 0 and 0 < near < far"); return 1; }
  if (N == 0 || V == 0) return 0;
  if (!v || !cams || !proj) { avc_set_error("avc_preview_project: NULL buffer"); return 1; }
  if ((unsigned long long)proj & 15ull) { avc_set_error("avc_preview_project: proj not 16-byte aligned"); return 1; }
  hipLaunchKernelGGL(pv_project_kernel, dim3((V + PV_THREADS - 1) / PV_THREADS, N), dim3(PV_THREADS), 0, (hipStream_t)stream, v, V, cams,
                     (double)width, (double)near, (double)far, raster_size, (i4*)proj);
  return avc_check_launch("avc_preview_project");
}

extern "C" int avc_preview_raster(const int* proj, int N, int V, const int* tris, int F, int raster_size, void* scratch, void* stream) {
  if (N < 0 || V < 0 || F < 0 || N > 65535) { avc_set_error("avc_preview_raster: bad sizes (at most 65535 frames a call)"); return 1; }
  if (raster_size <= 0 || raster_size > AVC_PREVIEW_MAX_RASTER) { avc_set_error("avc_preview_raster: raster size outside [1, 2048]"); return 1; }
  if (N == 0 || F == 0 || V == 0) return 0;
  if (!proj || !tris || !scratch) { avc_set_error("avc_preview_raster: NULL buffer"); return 1; }
  if (((unsigned long long)proj & 15ull) || ((unsigned long long)scratch & 7ull)) { avc_set_error("avc_preview_raster: proj not 16-byte or scratch not 8-byte aligned"); return 1; }
  hipStream_t s = (hipStream_t)stream;
  const long stride = avc_preview_scratch_bytes(F, raster_size);
  hipLaunchKernelGGL(pv_raster_kernel, dim3((F + PV_THREADS - 1) / PV_THREADS, N), dim3(PV_THREADS), 0, s, (const i4*)proj, tris, F, V, raster_size,
                     scratch, stride);
  const int nt = (raster_size + PV_TILE - 1) / PV_TILE;
  hipLaunchKernelGGL(pv_large_kernel, dim3(nt, nt, N), dim3(PV_THREADS), 0, s, (const i4*)proj, tris, F, V, raster_size, scratch, stride);
  return avc_check_launch("avc_preview_raster");
}

// ------------------------------------------------------------------------------------------------------------- shading
// Src: where the unlit colour comes from (csrc/avc_preview.h: PvVertexColours, PvTexture); everything else is one body
template <typename Src>
__global__ __launch_bounds__(PV_THREADS) void pv_shade_kernel(const i4* __restrict__ proj_all, const float* __restrict__ v_all, int V,
                                                              const int* __restrict__ tris, int F, const Src src,
                                                              const float* __restrict__ lights, float ambient, float bg0, float bg1,
                                                              float bg2, int S, int ss, void* __restrict__ scratch, long stride,
                                                              unsigned char* __restrict__ image, int* __restrict__ face_ids) {
  const int n = blockIdx.y;
  const int p = blockIdx.x * PV_THREADS + threadIdx.x;
  const int R = S * ss;
  unsigned long long* zbuf = pv_zbuf(scratch, stride, n);
  if (p >= S * S) return;
  const i4* proj = proj_all + (long)n * V;
  const float* vw = v_all + 3 * (long)n * V;
  const float* l = lights + 3 * (long)n;
  const int y = p / S, x = p % S;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int dy = 0; dy < ss; ++dy)
    for (int dx = 0; dx < ss; ++dx) {
      const int xi = ss * x + dx, yi = ss * y + dy;
      unsigned long long* z = &zbuf[(long)yi * R + xi];
      const unsigned long long key = *z;
      *z = PV_EMPTY;
      const int f = (int)(unsigned)(key & 0xFFFFFFFFull);
      float c[3] = {bg0, bg1, bg2};
      int id = -1;
      PvFace e;
      if (key != PV_EMPTY && (unsigned)f < (unsigned)F && pv_setup(proj, tris, f, V, R, e)) {
        id = f;
        pv_shade_face(e, proj, vw, src, l, ambient, xi, yi, c);
      }
      if (face_ids) face_ids[((long)n * R + yi) * R + xi] = id;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) acc[ch] += c[ch];
    }
  pv_store_pixel(image, (long)n * S * S + p, acc, ss);
}

// the checks, the launch and the scratch's way back to all-ones that both shade entry points share
template <typename Src>
static int pv_shade_launch(const char* what, const int* proj, const float* v, int N, int V, const int* tris, int F, const Src& src, const float* lights,
                           float ambient, float bg_r, float bg_g, float bg_b, int S, int ss, void* scratch, unsigned char* image, int* face_ids,
                           void* stream) {
  char msg[160];
  const char* bad = nullptr;
  if (N < 0 || V < 0 || F < 0 || N > 65535 || S <= 0) bad = "bad sizes (at most 65535 frames a call)";
  else if (ss != 1 && ss != 2) bad = "ss must be 1 or 2";
  else if ((long)S * ss > AVC_PREVIEW_MAX_RASTER) bad = "raster size S * ss above 2048";
  else if (!(ambient >= 0.f && ambient <= 1.f)) bad = "ambient outside [0, 1]";
  if (bad) { snprintf(msg, sizeof msg, "%s: %s", what, bad); avc_set_error(msg); return 1; }
  if (N == 0) return 0;
  if (!scratch || !image || !lights || (F && V && (!proj || !v || !tris))) bad = "NULL buffer";
  else if (((unsigned long long)proj & 15ull) || ((unsigned long long)scratch & 7ull)) bad = "proj not 16-byte or scratch not 8-byte aligned";
  if (bad) { snprintf(msg, sizeof msg, "%s: %s", what, bad); avc_set_error(msg); return 1; }
  const int Fe = V ? F : 0;                                   // no vertices: no face can have won
  const long stride = avc_preview_scratch_bytes(F, S * ss);
  hipLaunchKernelGGL(pv_shade_kernel<Src>, dim3((S * S + PV_THREADS - 1) / PV_THREADS, N), dim3(PV_THREADS), 0, (hipStream_t)stream, (const i4*)proj, v, V,
                     tris, Fe, src, lights, ambient, bg_r, bg_g, bg_b, S, ss, scratch, stride, image, face_ids);
  // the large-face lists (count and entries) back to all-ones: one strided fill over the N frames
  const long R = (long)S * ss;
  if (hipMemset2DAsync((char*)scratch + R * R * 8, (size_t)stride, 0xFF, (size_t)(stride - R * R * 8), (size_t)N, (hipStream_t)stream) != hipSuccess) {
    snprintf(msg, sizeof msg, "%s: hipMemset2DAsync failed", what);
    avc_set_error(msg);
    return 1;
  }
  return avc_check_launch(what);
}

extern "C" int avc_preview_shade(const int* proj, const float* v, int N, int V, const int* tris, int F, const unsigned char* colors, int csize,
                                 const float* lights, float ambient, float bg_r, float bg_g, float bg_b, float grey, int S, int ss,
                                 void* scratch, unsigned char* image, int* face_ids, void* stream) {
  if (colors && csize != 3 && csize != 4) { avc_set_error("avc_preview_shade: colours are 3 or 4 bytes per vertex"); return 1; }
  return pv_shade_launch("avc_preview_shade", proj, v, N, V, tris, F, PvVertexColours{colors, csize, grey}, lights, ambient, bg_r, bg_g, bg_b, S, ss,
                         scratch, image, face_ids, stream);
}

// csrc/avc_bake.h declares it: the same shade with the colour fetched from a texture
extern "C" int avc_preview_shade_tex(const int* proj, const float* v, int N, int V, const int* tris, int F, const float* uv, const unsigned char* texels,
                                     int T, const float* lights, float ambient, float bg_r, float bg_g, float bg_b, int S, int ss, void* scratch,
                                     unsigned char* image, int* face_ids, void* stream) {
  if (T < 1 || T > 4096) { avc_set_error("avc_preview_shade_tex: texture size outside [1, 4096]"); return 1; }
  if (!texels || (V && !uv)) { avc_set_error("avc_preview_shade_tex: NULL uv or texels"); return 1; }
  return pv_shade_launch("avc_preview_shade_tex", proj, v, N, V, tris, F, PvTexture{uv, texels, T}, lights, ambient, bg_r, bg_g, bg_b, S, ss, scratch,
                         image, face_ids, stream);
}

// ------------------------------------------------------------------------------------------------------------- four-influence skinning
__global__ __launch_bounds__(PV_THREADS) void pv_skin_blend4_kernel(const unsigned* __restrict__ joints, const f4* __restrict__ weights,
                                                                    const f4* __restrict__ mats, const float* __restrict__ rest, int M, int J,
                                                                    float* __restrict__ out) {
  const int m = blockIdx.x * PV_THREADS + threadIdx.x, t = blockIdx.y;
  if (m >= M) return;
  const unsigned jw = joints[m];
  const f4 w = weights[m];
  const float x = rest[3 * (long)m], y = rest[3 * (long)m + 1], z = rest[3 * (long)m + 2];
  float o[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned j = (jw >> (8 * k)) & 255u;
    if (j >= (unsigned)J) { o[0] = o[1] = o[2] = __uint_as_float(0x7FC00000u); continue; }    // (the caller checks the joints: reads nothing)
    const f4* A = mats + 3 * ((long)t * J + j);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const f4 a = A[r];
      o[r] += w[k] * (((a[0] * x + a[1] * y) + a[2] * z) + a[3]);
    }
  }
  float* dst = out + 3 * ((long)t * M + m);
  dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
}

extern "C" int avc_skin_blend4(const unsigned char* joints, const float* weights, const float* joint_mats, const float* rest, int M, int J, int T,
                               float* out, void* stream) {
  if (M < 0 || T < 0 || J <= 0 || J > 256 || T > 65535) { avc_set_error("avc_skin_blend4: bad sizes (1 <= J <= 256, at most 65535 frames a call)"); return 1; }
  if (M == 0 || T == 0) return 0;
  if (!joints || !weights || !joint_mats || !rest || !out) { avc_set_error("avc_skin_blend4: NULL buffer"); return 1; }
  if (((unsigned long long)joints & 3ull) || ((unsigned long long)weights & 15ull) || ((unsigned long long)joint_mats & 15ull)) {
    avc_set_error("avc_skin_blend4: joints not 4-byte or weights / joint_mats not 16-byte aligned");
    return 1;
  }
  hipLaunchKernelGGL(pv_skin_blend4_kernel, dim3((M + PV_THREADS - 1) / PV_THREADS, T), dim3(PV_THREADS), 0, (hipStream_t)stream,
                     (const unsigned*)joints, (const f4*)weights, (const f4*)joint_mats, rest, M, J, out);
  return avc_check_launch("avc_skin_blend4");
}
