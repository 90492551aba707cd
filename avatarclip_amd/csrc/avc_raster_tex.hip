// Textured renders of the posed body (AvatarAnimate/models/render.py:6-35 and ShapeGen/utils.py:6-28, where
// nr.Renderer takes the [F,ts,ts,ts,3] texture cubes of data/smpl_uv.obj): neural_renderer's texture sampling on the rasteriser of
// avc_raster.hip, forward with save and the approximate backward.  Rules: DESIGN.md section 8, restated in tests/nr_texture_restatement.py
// (unpinned against neural_renderer itself).
//
// Forward, avc_rasterize_mesh_tex_save: coverage and depth are raster_coverage's launches (avc_raster.hip) -- the z-buffer, hence the face-index
// map, is the grey entry point's bit for bit.  Only the resolve is new: one thread per super-sampled pixel, the four threads of a 2 x 2 window in
// neighbouring lanes.  A thread recomputes its winner's clamped barycentrics and depth (face_weights: the arithmetic the coverage tested with),
// blends the eight texels around t_k = w_k (ts - 1) zp / z_k of the face's cube (a fill-back copy f >= Ft reads the cube of f - Ft with axes 0
// and 2 swapped, by indexing), writes that unlit colour for the backward, multiplies by the face light and hands the product to the window's
// first lane, which pools ((a + b) + c) + d, / 4.  24 scattered texel reads per thread, neighbours mostly in the same 6-KB cube.
//
// Backward, avc_rasterize_mesh_tex_grad: the walk of avc_raster_grad.h with the colour C = light[I] U (three channels, U read back from the
// saved unlit map), Delta = sum_c (C_c(w) - C_c(w_ref)) G_c(w), grad_light[f] = sum over f's pixels of sum_c G_c U_c.  Nothing flows through the
// sampling weights and the cubes are constants, as in neural_renderer.  One wavefront per (render, face), CSR gather, no float atomics.
#include "avc_common.h"
#include "avc_texture.h"         // the C ABI of this file (lib.py parses it beside include/avc.h)
#include "avc_raster_grad.h"     // the walk + avc_raster.h: FaceEq, face_setup, face_weights, load_face, raster_coverage, RS_EMPTY

#pragma clang fp contract(off)   // same roundings as the fp32 restatement

// the unlit colour of face fn at super-sampled pixel (xi, yi) of an is x is grid: the trilinear blend of the face's cube at the pixel's
// perspective-corrected barycentrics
__device__ __forceinline__ void sample_cube(const float* __restrict__ nd, const int* __restrict__ idx, int fn, int xi, int yi, int is,
                                            const float* __restrict__ tex, int Ft, int ts, float eps, float (&U)[3]) {
  float f[9];
  load_face(nd, idx, fn, f);
  FaceEq e;
  face_setup(f, is, e);                 // (the face won this pixel: it is front-facing and den != 0)
  float w[3], ws, zp;
  face_weights(e, xi, yi, is, w, ws, zp);
  const float z[3] = {e.z0, e.z1, e.z2};
  int i[3];
  float r[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float t = w[k] / ws * (float)(ts - 1) * (zp / z[k]);
    t = fminf(fmaxf(t, 0.f), (float)(ts - 1) - eps);
    i[k] = min((int)t, ts - 2);         // (t <= ts - 1 - eps already gives this for any eps that fp32 resolves against ts - 1; i + 1 stays inside the cube)
    r[k] = t - (float)i[k];
  }
  const bool back = fn >= Ft;           // the fill-back copy: axes 0 and 2 of the cube of fn - Ft swapped
  const float* cube = tex + (long)(back ? fn - Ft : fn) * ts * ts * ts * 3;
  const int s0 = (back ? 1 : ts * ts) * 3, s1 = ts * 3, s2 = (back ? ts * ts : 1) * 3;
  U[0] = U[1] = U[2] = 0.f;
#pragma unroll
  for (int pn = 0; pn < 8; ++pn) {
    const int b0 = pn & 1, b1 = (pn >> 1) & 1, b2 = pn >> 2;
    const float wt = (b0 ? r[0] : 1.f - r[0]) * (b1 ? r[1] : 1.f - r[1]) * (b2 ? r[2] : 1.f - r[2]);
    const float* t = cube + (i[0] + b0) * s0 + (i[1] + b1) * s1 + (i[2] + b2) * s2;
#pragma unroll
    for (int c = 0; c < 3; ++c) U[c] += wt * t[c];
  }
}

// thread = super-sampled pixel k = gid & 3 ((dy, dx) = (k >> 1, k & 1), image rows: 0 = top) of pooled pixel gid >> 2 of render b = blockIdx.y:
// face index, unlit colour [N,is,is,3] (both in z-buffer orientation), the key put back to empty, and the lit 2 x 2 average -> image [N,S,S,3]
__global__ __launch_bounds__(256) void raster_resolve_tex_kernel(unsigned long long* __restrict__ zbufs, const float* __restrict__ ndc, int V,
                                                                 const int* __restrict__ idx, int F, const float* __restrict__ light,
                                                                 const float* __restrict__ tex, int Ft, int ts, float eps, int is,
                                                                 float* __restrict__ image, float* __restrict__ unlit, int* __restrict__ fidx,
                                                                 unsigned* __restrict__ larges) {
  const int S = is >> 1, b = blockIdx.y;
  const int gid = blockIdx.x * 256 + threadIdx.x, p = gid >> 2, k = gid & 3;
  if (gid == 0) larges[(long)b * (F + 2)] = 0xFFFFFFFFu;
  float C[3] = {0.f, 0.f, 0.f};
  if (p < S * S) {
    const int y = p / S, x = p % S;
    const int yi = is - 1 - (2 * y + (k >> 1)), xi = 2 * x + (k & 1);            // image row r (0 = top) is z-buffer row is - 1 - r
    const long q = (long)b * is * is + (long)yi * is + xi;
    const unsigned long long key = zbufs[q];
    zbufs[q] = RS_EMPTY;
    const bool bg = key == RS_EMPTY;
    const int face = (int)(unsigned)(key & 0xFFFFFFFFull);
    fidx[q] = bg ? -1 : face;
    float U[3] = {0.f, 0.f, 0.f};
    if (!bg) {
      sample_cube(ndc + (long)b * V * 3, idx, face, xi, yi, is, tex, Ft, ts, eps, U);
      const float l = light[(long)b * F + face];
#pragma unroll
      for (int c = 0; c < 3; ++c) C[c] = l * U[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) unlit[q * 3 + c] = U[c];
  }
  // the window's four colours to its first lane (every lane of the wavefront takes part), summed in the order (dy, dx) = (0,0), (0,1), (1,0), (1,1)
  const int lane0 = (threadIdx.x & 63) & ~3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float c0 = __shfl(C[c], lane0), c1 = __shfl(C[c], lane0 + 1), c2 = __shfl(C[c], lane0 + 2), c3 = __shfl(C[c], lane0 + 3);
    if (k == 0 && p < S * S) image[((long)b * S * S + p) * 3 + c] = (((c0 + c1) + c2) + c3) / 4.f;
  }
}

// the textured render's colour term: C = light[I] U (0 on background), three channels
struct TexGradView {
  struct Colour { float c[3]; };
  struct Args {
    const float* grad_image;   // [N,S,S,3], row 0 = top
    const float* light;        // [N,F]
    const float* unlit;        // [N,n,n,3], y up
  };
  const float* gi;
  const float* lt;
  const float* un;
  const int* I;
  int S, n;
  __device__ __forceinline__ TexGradView(const Args& a, int b, int F, int S_, const int* I_)
      : gi(a.grad_image + (long)b * S_ * S_ * 3), lt(a.light + (long)b * F), un(a.unlit + (long)b * 4 * S_ * S_ * 3), I(I_), S(S_), n(2 * S_) {}
  // G_c(x, y): the 2 x 2 average's backward with the row flip undone
  __device__ __forceinline__ float G(int x, int y, int c) const { return gi[((long)((n - 1 - y) >> 1) * S + (x >> 1)) * 3 + c] * 0.25f; }
  __device__ __forceinline__ Colour colour(int x, int y, int f) const {
    Colour o = {{0.f, 0.f, 0.f}};
    if (f >= 0) {
      const float l = lt[f];
      const float* u = un + ((long)y * n + x) * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c) o.c[c] = l * u[c];
    }
    return o;
  }
  __device__ __forceinline__ float delta(const Colour& a, const Colour& b, int x, int y) const {
    float d = (a.c[0] - b.c[0]) * G(x, y, 0);
    d += (a.c[1] - b.c[1]) * G(x, y, 1);
    d += (a.c[2] - b.c[2]) * G(x, y, 2);
    return d;
  }
  __device__ __forceinline__ float light_term(int x, int y) const {
    const float* u = un + ((long)y * n + x) * 3;
    float s = G(x, y, 0) * u[0];
    s += G(x, y, 1) * u[1];
    s += G(x, y, 2) * u[2];
    return s;
  }
};

// the sizes both entry points refuse: F faces of which the first Ft (F = Ft) or each half (F = 2 Ft: fill-back copies) own a cube of ts^3 texels
static bool tex_sizes_ok(int F, int Ft, int ts, float eps) {
  return Ft >= 0 && (F == Ft || F == 2 * Ft) && ts >= 2 && ts <= 256 && eps >= 0.f && eps < 1.f;
}

extern "C" int avc_rasterize_mesh_tex_save(const float* v_world, int N, int V, const int* idx, int F, const float* cam, float width, const float* light,
                                           const float* textures, int Ft, int ts, float eps, int S, float near, float far, float* ndc, float* image,
                                           float* unlit, int* fidx, void* scratch, void* stream) {
  if (N <= 0 || S <= 0 || V <= 0 || F < 0 || near < 0.f) { avc_set_error("avc_rasterize_mesh_tex_save: bad sizes"); return 1; }
  if (!tex_sizes_ok(F, Ft, ts, eps)) { avc_set_error("avc_rasterize_mesh_tex_save: F is not Ft or 2 Ft, ts is outside [2, 256] or eps outside [0, 1)"); return 1; }
  if (!v_world || !cam || !ndc || !image || !unlit || !fidx || !scratch || (F && (!idx || !light || !textures))) {
    avc_set_error("avc_rasterize_mesh_tex_save: NULL buffer");
    return 1;
  }
  const int is = 2 * S;
  raster_coverage(v_world, N, V, idx, F, cam, width, is, near, far, ndc, scratch, stream);
  unsigned long long* zbufs = (unsigned long long*)scratch;
  unsigned* larges = (unsigned*)(zbufs + (long)N * is * is);
  hipLaunchKernelGGL(raster_resolve_tex_kernel, dim3((is * is + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, zbufs, ndc, V, idx, F, light, textures,
                     Ft, ts, eps, is, image, unlit, fidx, larges);
  return avc_check_launch("avc_rasterize_mesh_tex_save");
}

extern "C" int avc_rasterize_mesh_tex_grad(const float* grad_image, const float* ndc, int N, int V, const int* idx, int F, const float* light,
                                           const float* unlit, const int* fidx, int S, float eps, const int* vf_ptr, const int* vf_ent,
                                           float* face_grad, float* grad_ndc, float* grad_light, void* stream) {
  if (N <= 0 || S <= 0 || V <= 0 || F < 0 || !(eps >= 0.f)) { avc_set_error("avc_rasterize_mesh_tex_grad: bad sizes"); return 1; }
  if (!grad_image || !ndc || !unlit || !fidx || !vf_ptr || !grad_ndc || (F && (!idx || !light || !vf_ent || !face_grad || !grad_light))) {
    avc_set_error("avc_rasterize_mesh_tex_grad: NULL buffer");
    return 1;
  }
  if (F)
    hipLaunchKernelGGL(rg_face_grad_kernel<TexGradView>, dim3((F + 3) / 4, N), dim3(256), 0, (hipStream_t)stream,
                       TexGradView::Args{grad_image, light, unlit}, ndc, V, idx, F, fidx, S, eps, face_grad, grad_light);
  rg_gather(face_grad, N, F, V, vf_ptr, vf_ent, grad_ndc, stream);
  return avc_check_launch("avc_rasterize_mesh_tex_grad");
}
