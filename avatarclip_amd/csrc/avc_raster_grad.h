// The scan-line walk of the rasteriser's pseudo-gradient (tests/nr_grad_restatement.py), shared by the grey backward
// (avc_raster_grad.hip) and the textured one (avc_raster_tex.hip).  The walk is a template on a View, which supplies what differs between them:
//   Colour                     the colour of a pixel (one float / three)
//   I, n, S                    the face-index map of the render [n,n] (y up), n = 2 S
//   colour(x, y, f)            the colour of pixel (x, y), whose winning face f the caller has read (f < 0: background, colour 0)
//   delta(a, b, x, y)          (a - b) weighted by the pooled upstream gradient at (x, y), summed over the channels ascending
//   light_term(x, y)           what pixel (x, y) adds to the light gradient of the face that won it
// and is built from (Args, render b, F, S, fidx of render b).  Both translation units compile this under `fp contract(off)`.
#pragma once
#include "avc_raster.h"

#pragma clang fp contract(off)   // the floors / ceilings of the crossings must be the fp32 restatement's

// one (edge, axis) of a front-facing face: the rules of DESIGN.md section 8 (tests/nr_grad_restatement.py), lanes over the runs' pixels.
// E = edge (a = E, b = E + 1, o = E + 2, mod 3), AX = 0: u = x, w = y (vertical runs, ndc y gets the gradient), AX = 1: u = y, w = x.
template <int E, int AX, class View>
__device__ __forceinline__ void edge_axis(const View& g, int fn, const float (&px)[3], const float (&py)[3], float eps, int lane,
                                          float (&acc)[3][2]) {
  typedef typename View::Colour Colour;
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
      const Colour c_in = g.colour(X(w_in), Y(w_in), f_in);
      const int len = dir > 0 ? n - w_out : w_out + 1;
      for (int k = lane; k < len; k += 64) {
        const int w = w_out + dir * k;
        const float delta = g.delta(g.colour(X(w), Y(w), face_at(w)), c_in, X(w), Y(w));
        if (delta > 0.f) update(w, delta);
      }
    }
    // in run: the face shrinks, its pixels from w_in to the opposite side
    const float wx2 = (fu - ua) * (fu - uo) < 0.f ? (wo - wa) / (uo - ua) * (fu - ua) + wa : (wb - wo) / (ub - uo) * (fu - uo) + wo;
    const float lim = dir > 0 ? ceilf(wx2) : floorf(wx2);
    const float r_lo = fmaxf(fminf(win_f, lim), 0.f), r_hi = fminf(fmaxf(win_f, lim), (float)(n - 1));   // (fmin / fmax: a NaN limit -> w_in alone)
    const int i_lo = (int)r_lo, i_hi = (int)r_hi;
    const Colour c_out = g.colour(X(w_out), Y(w_out), face_at(w_out));
    for (int w = i_lo + lane; w <= i_hi; w += 64) {
      if (face_at(w) != fn) continue;
      const float delta = g.delta(g.colour(X(w), Y(w), fn), c_out, X(w), Y(w));
      if (delta > 0.f) update(w, delta);
    }
  }
}

// one wavefront per (render b = blockIdx.y, face): grad_light[b, f] and the face's three vertex gradients (x, y) -> face_grad [N, F, 6]
template <class View>
__global__ __launch_bounds__(256) void rg_face_grad_kernel(typename View::Args args, const float* __restrict__ ndc, int V,
                                                           const int* __restrict__ idx, int F, const int* __restrict__ fidx, int S, float eps,
                                                           float* __restrict__ face_grad, float* __restrict__ grad_light) {
  const int fn = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, b = blockIdx.y;
  if (fn >= F) return;
  const int n = 2 * S;
  const View g(args, b, F, S, fidx + (long)b * n * n);
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
      if (g.I[(long)y * n + x] == fn) gl += g.light_term(x, y);
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

// the gather launch of avc_raster_grad.hip: grad_ndc[b, v] = (sum over the (face, corner) entries of vertex v of face_grad, in CSR order, 0)
void rg_gather(const float* face_grad, int N, int F, int V, const int* vf_ptr, const int* vf_ent, float* grad_ndc, void* stream);
