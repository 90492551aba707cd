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
#include "avc_raster.h"

#pragma clang fp contract(off)   // the floors / ceilings of the crossings must be the fp32 restatement's

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

struct GradView {
  const float* gi;    // upstream gradient of render b [S,S], row 0 = top
  const float* lt;    // light of render b [F]
  const int* I;       // face index map of render b [n,n], y up
  int S, n;
  // G(x, y): the 2 x 2 average's backward with the row flip undone
  __device__ __forceinline__ float G(int x, int y) const { return gi[(long)((n - 1 - y) >> 1) * S + (x >> 1)] * 0.25f; }
  __device__ __forceinline__ float c(int f) const { return f >= 0 ? lt[f] : 0.f; }
};

// one (edge, axis) of a front-facing face: the rules of DESIGN.md section 8 (tests/nr_grad_restatement.py), lanes over the runs' pixels.
// E = edge (a = E, b = E + 1, o = E + 2, mod 3), AX = 0: u = x, w = y (vertical runs, ndc y gets the gradient), AX = 1: u = y, w = x.
template <int E, int AX>
__device__ __forceinline__ void edge_axis(const GradView& g, int fn, const float (&px)[3], const float (&py)[3], float eps, int lane,
                                          float (&acc)[3][2]) {
  constexpr int A = E, B = (E + 1) % 3, O = (E + 2) % 3, C = AX == 0 ? 1 : 0;
  const int n = g.n;
  const float ua = AX == 0 ? px[A] : py[A], wa = AX == 0 ? py[A] : px[A];
  const float ub = AX == 0 ? px[B] : py[B], wb = AX == 0 ? py[B] : px[B];
  const float uo = AX == 0 ? px[O] : py[O], wo = AX == 0 ? py[O] : px[O];
  const int dir = AX == 0 ? (ua < ub ? -1 : 1) : (ua < ub ? 1 : -1);
  const float lo = fmaxf(ceilf(fminf(ua, ub)), 0.f), hi = fminf(fmaxf(ua, ub), (float)(n - 1));
  if (!(lo <= (float)(n - 1)) || !(hi > -1.f)) return;                 // (float tests first: no int holds 1e30)
  const int u_lo = (int)lo, u_hi = (int)hi;                             // C truncation, as the published kernel
  for (int u0 = u_lo; u0 <= u_hi; ++u0) {
    const float fu = (float)u0;
    const float wx = (wb - wa) / (ub - ua) * (fu - ua) + wa;
    const float win_f = dir > 0 ? floorf(wx) : ceilf(wx);
    const float wout_f = win_f + (float)dir;
    if (!(win_f >= 0.f && win_f < (float)n && wout_f >= 0.f && wout_f < (float)n)) continue;
    const int w_in = (int)win_f, w_out = (int)wout_f;
    // pixel (x, y) of scan-line position w
    auto X = [&](int w) { return AX == 0 ? u0 : w; };
    auto Y = [&](int w) { return AX == 0 ? w : u0; };
    auto face_at = [&](int w) { return g.I[(long)Y(w) * n + X(w)]; };
    // the vertex displacement that moves the edge through the centre of pixel w (pushed away from zero by eps); Delta / d per vertex
    auto update = [&](int w, float delta) {
      const float dw = (float)w - wx;
      if (ub != fu) {
        float d = (ub - ua) / (ub - fu) * dw * 2.f / (float)n;
        d = d > 0.f ? d + eps : d - eps;
        acc[A][C] -= delta / d;
      }
      if (ua != fu) {
        float d = (ub - ua) / (fu - ua) * dw * 2.f / (float)n;
        d = d > 0.f ? d + eps : d - eps;
        acc[B][C] -= delta / d;
      }
    };
    const int f_in = face_at(w_in);
    // out run: the face grows over w_out .. border
    if (f_in == fn) {
      const float c_in = g.c(f_in);
      const int len = dir > 0 ? n - w_out : w_out + 1;
      for (int k = lane; k < len; k += 64) {
        const int w = w_out + dir * k;
        const float delta = (g.c(face_at(w)) - c_in) * g.G(X(w), Y(w));
        if (delta > 0.f) update(w, delta);
      }
    }
    // in run: the face shrinks, its pixels from w_in to the opposite side
    const float wx2 = (fu - ua) * (fu - uo) < 0.f ? (wo - wa) / (uo - ua) * (fu - ua) + wa : (wb - wo) / (ub - uo) * (fu - uo) + wo;
    const float lim = dir > 0 ? ceilf(wx2) : floorf(wx2);
    const float r_lo = fmaxf(fminf(win_f, lim), 0.f), r_hi = fminf(fmaxf(win_f, lim), (float)(n - 1));   // (fmin / fmax: a NaN limit -> w_in alone)
    const int i_lo = (int)r_lo, i_hi = (int)r_hi;
    const float c_out = g.c(face_at(w_out));
    for (int w = i_lo + lane; w <= i_hi; w += 64) {
      if (face_at(w) != fn) continue;
      const float delta = (g.c(fn) - c_out) * g.G(X(w), Y(w));
      if (delta > 0.f) update(w, delta);
    }
  }
}

// one wavefront per (render b = blockIdx.y, face): grad_light[b, f] and the face's three vertex gradients (x, y) -> face_grad [N, F, 6]
__global__ __launch_bounds__(256) void rg_face_grad_kernel(const float* __restrict__ grad_image, const float* __restrict__ ndc, int V,
                                                           const int* __restrict__ idx, int F, const float* __restrict__ light,
                                                           const int* __restrict__ fidx, int S, float eps, float* __restrict__ face_grad,
                                                           float* __restrict__ grad_light) {
  const int fn = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, b = blockIdx.y;
  if (fn >= F) return;
  const int n = 2 * S;
  GradView g{grad_image + (long)b * S * S, light + (long)b * F, fidx + (long)b * n * n, S, n};
  float f[9];
  load_face(ndc + (long)b * V * 3, idx, fn, f);
  FaceEq e{};
  const bool front = face_setup(f, n, e);
  // light: the face's pixels lie in its box (raster_faces_kernel / raster_large_kernel rasterise nothing outside it)
  float gl = 0.f;
  int xa, xb, ya, yb;
  if (front && face_box(e, n, xa, xb, ya, yb)) {
    const int w = xb - xa + 1, np = w * (yb - ya + 1);
    for (int k = lane; k < np; k += 64) {
      const int x = xa + k % w, y = ya + k / w;
      if (g.I[(long)y * n + x] == fn) gl += g.G(x, y);
    }
  }
  gl = wave_sum(gl);
  float acc[3][2] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
  const float px[3] = {e.p0x, e.p1x, e.p2x}, py[3] = {e.p0y, e.p1y, e.p2y};
  const bool finite = front && isfinite(px[0]) && isfinite(px[1]) && isfinite(px[2]) && isfinite(py[0]) && isfinite(py[1]) && isfinite(py[2]);
  if (finite) {
    edge_axis<0, 0>(g, fn, px, py, eps, lane, acc);
    edge_axis<0, 1>(g, fn, px, py, eps, lane, acc);
    edge_axis<1, 0>(g, fn, px, py, eps, lane, acc);
    edge_axis<1, 1>(g, fn, px, py, eps, lane, acc);
    edge_axis<2, 0>(g, fn, px, py, eps, lane, acc);
    edge_axis<2, 1>(g, fn, px, py, eps, lane, acc);
  }
  float out[6];
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    out[2 * v] = wave_sum(acc[v][0]);
    out[2 * v + 1] = wave_sum(acc[v][1]);
  }
  if (lane == 0) {
    float* fg = face_grad + ((long)b * F + fn) * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) fg[k] = out[k];
    grad_light[(long)b * F + fn] = gl;
  }
}

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

extern "C" int avc_rasterize_mesh_grad(const float* grad_image, const float* ndc, int N, int V, const int* idx, int F, const float* light,
                                       const int* fidx, int S, float eps, const int* vf_ptr, const int* vf_ent, float* face_grad,
                                       float* grad_ndc, float* grad_light, void* stream) {
  if (N <= 0 || S <= 0 || V <= 0 || F < 0 || !(eps >= 0.f)) { avc_set_error("avc_rasterize_mesh_grad: bad sizes"); return 1; }
  if (!grad_image || !ndc || !fidx || !vf_ptr || !grad_ndc || (F && (!idx || !light || !vf_ent || !face_grad || !grad_light))) {
    avc_set_error("avc_rasterize_mesh_grad: NULL buffer");
    return 1;
  }
  hipStream_t s = (hipStream_t)stream;
  if (F) hipLaunchKernelGGL(rg_face_grad_kernel, dim3((F + 3) / 4, N), dim3(256), 0, s, grad_image, ndc, V, idx, F, light, fidx, S, eps, face_grad, grad_light);
  hipLaunchKernelGGL(rg_gather_kernel, dim3((V + 255) / 256, N), dim3(256), 0, s, face_grad, F, V, vf_ptr, vf_ent, grad_ndc);
  return avc_check_launch("avc_rasterize_mesh_grad");
}
