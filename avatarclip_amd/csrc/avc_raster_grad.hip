// The rasteriser's backward pass for AvatarAnimate (AvatarAnimate/models/render.py:10-39, where
// neural_renderer's renders of the posed body are differentiated with respect to the vertices): the approximate gradient of Kato,
// Ushiku and Harada, "Neural 3D Mesh Renderer" (CVPR 2018) section 3.3, restated from the paper and the published kernel in
// tests/nr_grad_restatement.py (DESIGN.md section 8 states the rules; unpinned against neural_renderer itself).
//
// The forward with save (avc_rasterize_mesh_save: N renders in one call, the pooled images + the super-sampled face-index map) is in
// avc_raster.hip with the other forward entry points.  Here, avc_rasterize_mesh_grad: one wavefront per (render, face).  Light gradient = sum of
// the upstream gradient over the pixels the face won (its box, as raster_faces_kernel walks it).  Pseudo-gradient: for every edge, axis and scan
// line the edge crosses, the "out" run from the pixel just outside the edge to the image border and the "in" run across the face, lanes over the
// run's pixels; every lane accumulates its own contributions to the face's three vertices in registers, a fixed-order wave reduction sums them.
// Then one thread per (render, vertex) gathers its faces' sums through a vertex -> face CSR.  No float atomics: the result is deterministic.
#include "avc_common.h"
#include "../../include/avc.h"
#include "avc_raster_grad.h"     // edge_axis, rg_face_grad_kernel<View>: the walk, shared with the textured backward (avc_raster_tex.hip)

#pragma clang fp contract(off)   // the floors / ceilings of the crossings must be the fp32 restatement's

// the grey render's colour term: c = light[I] (0 on background), one channel
struct GradView {
  typedef float Colour;
  struct Args {
    const float* grad_image;   // [N,S,S], row 0 = top
    const float* light;        // [N,F]
  };
  const float* gi;    // upstream gradient of render b [S,S], row 0 = top
  const float* lt;    // light of render b [F]
  const int* I;       // face index map of render b [n,n], y up
  int S, n;
  __device__ __forceinline__ GradView(const Args& a, int b, int F, int S_, const int* I_)
      : gi(a.grad_image + (long)b * S_ * S_), lt(a.light + (long)b * F), I(I_), S(S_), n(2 * S_) {}
  // G(x, y): the 2 x 2 average's backward with the row flip undone
  __device__ __forceinline__ float G(int x, int y) const { return gi[(long)((n - 1 - y) >> 1) * S + (x >> 1)] * 0.25f; }
  __device__ __forceinline__ float colour(int, int, int f) const { return f >= 0 ? lt[f] : 0.f; }
  __device__ __forceinline__ float delta(float a, float b, int x, int y) const { return (a - b) * G(x, y); }
  __device__ __forceinline__ float light_term(int x, int y) const { return G(x, y); }
};

// grad_ndc[b, v] = (sum over the (face, corner) entries of vertex v of face_grad, in CSR order, 0); one thread per (render, vertex)
__global__ __launch_bounds__(256) void rg_gather_kernel(const float* __restrict__ face_grad, int F, int V, const int* __restrict__ vf_ptr,
                                                        const int* __restrict__ vf_ent, float* __restrict__ grad_ndc) {
  const int v = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (v >= V) return;
  const float* fg = face_grad + (long)b * F * 6;
  float gx = 0.f, gy = 0.f;
  for (int k = vf_ptr[v]; k < vf_ptr[v + 1]; ++k) {
    const int ent = vf_ent[k];                     // 3 * face + corner
    const long o = (long)(ent / 3) * 6 + 2 * (ent % 3);
    gx += fg[o];
    gy += fg[o + 1];
  }
  float* out = grad_ndc + ((long)b * V + v) * 3;
  out[0] = gx;
  out[1] = gy;
  out[2] = 0.f;
}

void rg_gather(const float* face_grad, int N, int F, int V, const int* vf_ptr, const int* vf_ent, float* grad_ndc, void* stream) {
  hipLaunchKernelGGL(rg_gather_kernel, dim3((V + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, face_grad, F, V, vf_ptr, vf_ent, grad_ndc);
}

extern "C" int avc_rasterize_mesh_grad(const float* grad_image, const float* ndc, int N, int V, const int* idx, int F, const float* light,
                                       const int* fidx, int S, float eps, const int* vf_ptr, const int* vf_ent, float* face_grad,
                                       float* grad_ndc, float* grad_light, void* stream) {
  if (N <= 0 || S <= 0 || V <= 0 || F < 0 || !(eps >= 0.f)) { avc_set_error("avc_rasterize_mesh_grad: bad sizes"); return 1; }
  if (!grad_image || !ndc || !fidx || !vf_ptr || !grad_ndc || (F && (!idx || !light || !vf_ent || !face_grad || !grad_light))) {
    avc_set_error("avc_rasterize_mesh_grad: NULL buffer");
    return 1;
  }
  hipStream_t s = (hipStream_t)stream;
  if (F)
    hipLaunchKernelGGL(rg_face_grad_kernel<GradView>, dim3((F + 3) / 4, N), dim3(256), 0, s, GradView::Args{grad_image, light}, ndc, V, idx, F, fidx, S,
                       eps, face_grad, grad_light);
  rg_gather(face_grad, N, F, V, vf_ptr, vf_ent, grad_ndc, stream);
  return avc_check_launch("avc_rasterize_mesh_grad");
}
