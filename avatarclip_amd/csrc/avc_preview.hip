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
//    A face with an invalid vertex is dropped, not clipped.
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
#include "avc_common.h"
#include "../../include/avc.h"

#pragma clang fp contract(off)   // the projection must be the restatement's operation by operation

#define PV_THREADS 256
#define PV_GUARD 65536           // sub-pixel units beyond the raster on each side within which a vertex stays valid (256 raster pixels)
#define PV_SERIAL 4              // pixel centres in a face's box up to which its own lane finishes it
#define PV_LARGE 1024            // ... from which it goes to the tile-parallel pass
#define PV_TILE 16
#define PV_EMPTY 0xFFFFFFFFFFFFFFFFull
#define PV_ZMAX 16777215.0       // 2^24 - 1

typedef int i4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------------------- projection
__global__ __launch_bounds__(PV_THREADS) void pv_project_kernel(const float* __restrict__ v, int V, const float* __restrict__ cams, double width,
                                                                double near, double far, int R, i4* __restrict__ proj) {
  const int i = blockIdx.x * PV_THREADS + threadIdx.x, n = blockIdx.y;
  if (i >= V) return;
  const float* cam = cams + 12 * (long)n;
  const float* p = v + 3 * ((long)n * V + i);
  const double d0 = (double)p[0] - (double)cam[0], d1 = (double)p[1] - (double)cam[1], d2 = (double)p[2] - (double)cam[2];
  double c[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) c[j] = (d0 * (double)cam[3 + 3 * j] + d1 * (double)cam[4 + 3 * j]) + d2 * (double)cam[5 + 3 * j];
  i4 o = {0, 0, -1, 0};
  if (c[2] > near && c[2] <= far) {
    const double s = c[2] * width, half = (double)R * 0.5;
    const double X = floor((c[0] / s + 1.0) * half * 256.0 + 0.5), Y = floor((1.0 - c[1] / s) * half * 256.0 + 0.5);
    const double hi = 256.0 * (double)R + (double)PV_GUARD;
    if (X >= -(double)PV_GUARD && X <= hi && Y >= -(double)PV_GUARD && Y <= hi) {
      double Z = floor(((c[2] - near) * far) / (c[2] * (far - near)) * PV_ZMAX + 0.5);
      Z = fmin(fmax(Z, 0.0), PV_ZMAX);
      o = i4{(int)X, (int)Y, (int)Z, (int)__float_as_uint((float)(1.0 / c[2]))};
    }
  }
  proj[(long)n * V + i] = o;
}

// ------------------------------------------------------------------------------------------------------------- the face
struct PvFace {
  int x0, y0, x1, y1, x2, y2, z0, z1, z2;
  int b0, b1, b2;                  // 0 for a top-left edge, 1 otherwise: covered <=> w_i >= b_i
  long long area2;
  double inv_area2;
  int xa, xb, ya, yb;              // pixels whose centres can be covered (clamped to the raster)
  int i0, i1, i2;                  // the vertices, in oriented order
};
__device__ __forceinline__ long long pv_edge(int ax, int ay, int bx, int by, int px, int py) {
  return (long long)(bx - ax) * (long long)(py - ay) - (long long)(by - ay) * (long long)(px - ax);
}
__device__ __forceinline__ int pv_bias(int ax, int ay, int bx, int by) { return (by < ay || (by == ay && bx > ax)) ? 0 : 1; }

// false: dropped (a corner outside [0, V), an invalid corner, zero area) or no pixel centre inside the raster can be covered
__device__ __forceinline__ bool pv_setup(const i4* __restrict__ proj, const int* __restrict__ tris, int f, int V, int R, PvFace& e) {
  e.i0 = tris[3 * (long)f];
  e.i1 = tris[3 * (long)f + 1];
  e.i2 = tris[3 * (long)f + 2];
  if ((unsigned)e.i0 >= (unsigned)V || (unsigned)e.i1 >= (unsigned)V || (unsigned)e.i2 >= (unsigned)V) return false;
  i4 a = proj[e.i0], b = proj[e.i1], c = proj[e.i2];
  if (a[2] < 0 || b[2] < 0 || c[2] < 0) return false;
  long long area2 = pv_edge(a[0], a[1], b[0], b[1], c[0], c[1]);
  if (area2 == 0) return false;
  if (area2 < 0) {
    const i4 t = b; b = c; c = t;
    const int ti = e.i1; e.i1 = e.i2; e.i2 = ti;
    area2 = -area2;
  }
  e.x0 = a[0]; e.y0 = a[1]; e.z0 = a[2];
  e.x1 = b[0]; e.y1 = b[1]; e.z1 = b[2];
  e.x2 = c[0]; e.y2 = c[1]; e.z2 = c[2];
  e.area2 = area2;
  e.inv_area2 = 1.0 / (double)area2;
  e.b0 = pv_bias(e.x1, e.y1, e.x2, e.y2);
  e.b1 = pv_bias(e.x2, e.y2, e.x0, e.y0);
  e.b2 = pv_bias(e.x0, e.y0, e.x1, e.y1);
  // centre 256 i + 128 in [lo, hi]  <=>  ceil((lo - 128) / 256) <= i <= floor((hi - 128) / 256)   (>> of an int: floor)
  e.xa = max(0, (min(e.x0, min(e.x1, e.x2)) + 127) >> 8); e.xb = min(R - 1, (max(e.x0, max(e.x1, e.x2)) - 128) >> 8);
  e.ya = max(0, (min(e.y0, min(e.y1, e.y2)) + 127) >> 8); e.yb = min(R - 1, (max(e.y0, max(e.y1, e.y2)) - 128) >> 8);
  return e.xb >= e.xa && e.yb >= e.ya;
}
// the three weights at pixel (xi, yi); true: covered
__device__ __forceinline__ bool pv_weights(const PvFace& e, int xi, int yi, long long& w0, long long& w1, long long& w2) {
  const int px = 256 * xi + 128, py = 256 * yi + 128;
  w0 = pv_edge(e.x1, e.y1, e.x2, e.y2, px, py);
  w1 = pv_edge(e.x2, e.y2, e.x0, e.y0, px, py);
  w2 = e.area2 - w0 - w1;
  return w0 >= e.b0 && w1 >= e.b1 && w2 >= e.b2;
}
// the key of face f at a covered pixel
__device__ __forceinline__ unsigned long long pv_key(const PvFace& e, long long w0, long long w1, long long w2, int f) {
  const long long sum = w0 * e.z0 + w1 * e.z1 + w2 * e.z2;
  long long q = (long long)((double)sum * e.inv_area2);
  long long r = sum - q * e.area2;
  if (r < 0) { --q; r += e.area2; }
  if (r >= e.area2) ++q;
  return ((unsigned long long)q << 32) | (unsigned)f;
}

// ------------------------------------------------------------------------------------------------------------- raster
// per frame: zbuf [R*R] keys, then large = [count - 1 (0xFFFFFFFF: none), face indices ...]
__device__ __forceinline__ unsigned long long* pv_zbuf(void* scratch, long stride, int n) { return (unsigned long long*)((char*)scratch + stride * n); }

__global__ __launch_bounds__(PV_THREADS) void pv_raster_kernel(const i4* __restrict__ proj_all, const int* __restrict__ tris, int F, int V, int R,
                                                               void* __restrict__ scratch, long stride) {
  const int n = blockIdx.y, lane = threadIdx.x & 63;
  const int f = blockIdx.x * PV_THREADS + threadIdx.x;
  const i4* proj = proj_all + (long)n * V;
  unsigned long long* zbuf = pv_zbuf(scratch, stride, n);
  unsigned* large = (unsigned*)(zbuf + (long)R * R);
  PvFace e;
  const bool ok = f < F && pv_setup(proj, tris, f, V, R, e);
  int w = 0, cnt = 0;
  if (ok) {
    w = e.xb - e.xa + 1;
    cnt = w * (e.yb - e.ya + 1);
  }
  if (ok && cnt <= PV_SERIAL) {
    for (int k = 0; k < cnt; ++k) {
      const int xi = e.xa + k % w, yi = e.ya + k / w;
      long long w0, w1, w2;
      if (pv_weights(e, xi, yi, w0, w1, w2)) atomicMin(&zbuf[(long)yi * R + xi], pv_key(e, w0, w1, w2, f));
    }
  }
  if (ok && cnt > PV_LARGE) {                                 // every face once: at most F entries (a scratch that did not come in as
    const unsigned slot = atomicAdd(&large[0], 1u) + 1u;      // 0xFF starts the count anywhere: nothing is written past the list)
    if (slot < (unsigned)F) large[1 + slot] = (unsigned)f;
  }
  unsigned long long todo = __ballot(ok && cnt > PV_SERIAL && cnt <= PV_LARGE);             // wave-uniform from here on
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int fs = __shfl(f, src);
    PvFace g;
    if (!pv_setup(proj, tris, fs, V, R, g)) continue;                                       // (it passed in lane src: never taken)
    const int gw = g.xb - g.xa + 1, gn = gw * (g.yb - g.ya + 1);
    for (int k = lane; k < gn; k += 64) {
      const int xi = g.xa + k % gw, yi = g.ya + k / gw;
      long long w0, w1, w2;
      if (pv_weights(g, xi, yi, w0, w1, w2)) atomicMin(&zbuf[(long)yi * R + xi], pv_key(g, w0, w1, w2, fs));
    }
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
    if (e.xb < tx0 || e.xa > tx0 + PV_TILE - 1 || e.yb < ty0 || e.ya > ty0 + PV_TILE - 1) continue;     // (uniform over the workgroup)
    long long w0, w1, w2;
    if (!inside || !pv_weights(e, xi, yi, w0, w1, w2)) continue;
    const unsigned long long key = pv_key(e, w0, w1, w2, f);
    best = key < best ? key : best;
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
__global__ __launch_bounds__(PV_THREADS) void pv_shade_kernel(const i4* __restrict__ proj_all, const float* __restrict__ v_all, int V,
                                                              const int* __restrict__ tris, int F, const unsigned char* __restrict__ colors,
                                                              int csize, const float* __restrict__ lights, float ambient, float bg0, float bg1,
                                                              float bg2, float grey, int S, int ss, void* __restrict__ scratch, long stride,
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
        long long w0, w1, w2;
        pv_weights(e, xi, yi, w0, w1, w2);
        const float l0 = (float)w0 * __uint_as_float((unsigned)proj[e.i0][3]);
        const float l1 = (float)w1 * __uint_as_float((unsigned)proj[e.i1][3]);
        const float l2 = (float)w2 * __uint_as_float((unsigned)proj[e.i2][3]);
        const float den = (l0 + l1) + l2;
        const float* a = vw + 3 * (long)e.i0;
        const float* b = vw + 3 * (long)e.i1;
        const float* d = vw + 3 * (long)e.i2;
        const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], tx = d[0] - a[0], ty = d[1] - a[1], tz = d[2] - a[2];
        const float nx = uy * tz - uz * ty, ny = uz * tx - ux * tz, nz = ux * ty - uy * tx;
        const float nn = sqrtf((nx * nx + ny * ny) + nz * nz) * sqrtf((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2]);
        const float shade = nn > 0.f ? ambient + (1.f - ambient) * fminf(fabsf((nx * l[0] + ny * l[1]) + nz * l[2]) / nn, 1.f) : ambient;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          float col = grey;
          if (colors)
            col = ((l0 * (float)colors[(long)csize * e.i0 + ch] + l1 * (float)colors[(long)csize * e.i1 + ch]) +
                   l2 * (float)colors[(long)csize * e.i2 + ch]) / den;
          c[ch] = col * shade;
        }
      }
      if (face_ids) face_ids[((long)n * R + yi) * R + xi] = id;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) acc[ch] += c[ch];
    }
  const float inv = 1.f / (float)(ss * ss);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
    image[((long)n * S * S + p) * 3 + ch] = (unsigned char)fminf(fmaxf(floorf(acc[ch] * inv + 0.5f), 0.f), 255.f);
}

extern "C" int avc_preview_shade(const int* proj, const float* v, int N, int V, const int* tris, int F, const unsigned char* colors, int csize,
                                 const float* lights, float ambient, float bg_r, float bg_g, float bg_b, float grey, int S, int ss,
                                 void* scratch, unsigned char* image, int* face_ids, void* stream) {
  if (N < 0 || V < 0 || F < 0 || N > 65535 || S <= 0) { avc_set_error("avc_preview_shade: bad sizes (at most 65535 frames a call)"); return 1; }
  if (ss != 1 && ss != 2) { avc_set_error("avc_preview_shade: ss must be 1 or 2"); return 1; }
  if ((long)S * ss > AVC_PREVIEW_MAX_RASTER) { avc_set_error("avc_preview_shade: raster size S * ss above 2048"); return 1; }
  if (colors && csize != 3 && csize != 4) { avc_set_error("avc_preview_shade: colours are 3 or 4 bytes per vertex"); return 1; }
  if (!(ambient >= 0.f && ambient <= 1.f)) { avc_set_error("avc_preview_shade: ambient outside [0, 1]"); return 1; }
  if (N == 0) return 0;
  if (!scratch || !image || !lights || (F && V && (!proj || !v || !tris))) { avc_set_error("avc_preview_shade: NULL buffer"); return 1; }
  if (((unsigned long long)proj & 15ull) || ((unsigned long long)scratch & 7ull)) { avc_set_error("avc_preview_shade: proj not 16-byte or scratch not 8-byte aligned"); return 1; }
  const int Fe = V ? F : 0;                                   // no vertices: no face can have won
  const long stride = avc_preview_scratch_bytes(F, S * ss);
  hipLaunchKernelGGL(pv_shade_kernel, dim3((S * S + PV_THREADS - 1) / PV_THREADS, N), dim3(PV_THREADS), 0, (hipStream_t)stream, (const i4*)proj, v, V,
                     tris, Fe, colors, csize, lights, ambient, bg_r, bg_g, bg_b, grey, S, ss, scratch,
                     stride, image, face_ids);
  // the large-face lists (count and entries) back to all-ones: one strided fill over the N frames
  const long R = (long)S * ss;
  if (hipMemset2DAsync((char*)scratch + R * R * 8, (size_t)stride, 0xFF, (size_t)(stride - R * R * 8), (size_t)N, (hipStream_t)stream) != hipSuccess) {
    avc_set_error("avc_preview_shade: hipMemset2DAsync failed");
    return 1;
  }
  return avc_check_launch("avc_preview_shade");
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
