// The device functions csrc/avc_preview.hip and csrc/avc_preview_clip.hip share: the projection's arithmetic, the face set-up, the coverage
// weights, the depth key, and the per-face pieces of the three passes (the wavefront's walk of a box, a tile's test of a listed face, the
// flat shade).  One copy of the coverage and depth arithmetic, not two that agree; csrc/avc_preview.hip's header states the rules.
#ifndef AVC_PREVIEW_DEVICE_H
#define AVC_PREVIEW_DEVICE_H
#include "avc_common.h"

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
// c_j = (d0 a_j0 + d1 a_j1) + d2 a_j2, d = p - eye
__device__ __forceinline__ void pv_camera_point(const float* __restrict__ p, const float* __restrict__ cam, double c[3]) {
  const double d0 = (double)p[0] - (double)cam[0], d1 = (double)p[1] - (double)cam[1], d2 = (double)p[2] - (double)cam[2];
#pragma unroll
  for (int j = 0; j < 3; ++j) c[j] = (d0 * (double)cam[3 + 3 * j] + d1 * (double)cam[4 + 3 * j]) + d2 * (double)cam[5 + 3 * j];
}
// the snapped X, Y (not yet range-checked) and Z (clamped to its 24 bits) of a camera-space point with c_z > 0
__device__ __forceinline__ void pv_snap(double cx, double cy, double cz, double width, double near, double far, int R, double& X, double& Y,
                                        double& Z) {
  const double s = cz * width, half = (double)R * 0.5;
  X = floor((cx / s + 1.0) * half * 256.0 + 0.5);
  Y = floor((1.0 - cy / s) * half * 256.0 + 0.5);
  Z = floor(((cz - near) * far) / (cz * (far - near)) * PV_ZMAX + 0.5);
  Z = fmin(fmax(Z, 0.0), PV_ZMAX);
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

// three snapped corners (valid: Z >= 0) named i0, i1, i2; false: zero area, or no pixel centre inside the raster can be covered
__device__ __forceinline__ bool pv_setup3(i4 a, i4 b, i4 c, int i0, int i1, int i2, int R, PvFace& e) {
  e.i0 = i0; e.i1 = i1; e.i2 = i2;
  long long area2 = pv_edge(a[0], a[1], b[0], b[1], c[0], c[1]);
  if (area2 == 0) return false;
  if (area2 < 0) {
    const i4 t = b; b = c; c = t;
    e.i1 = i2; e.i2 = i1;
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
// false: dropped (a corner outside [0, V), an invalid corner, zero area) or no pixel centre inside the raster can be covered
__device__ __forceinline__ bool pv_setup(const i4* __restrict__ proj, const int* __restrict__ tris, int f, int V, int R, PvFace& e) {
  const int i0 = tris[3 * (long)f], i1 = tris[3 * (long)f + 1], i2 = tris[3 * (long)f + 2];
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;
  const i4 a = proj[i0], b = proj[i1], c = proj[i2];
  if (a[2] < 0 || b[2] < 0 || c[2] < 0) return false;
  return pv_setup3(a, b, c, i0, i1, i2, R, e);
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
__device__ __forceinline__ int pv_centres(const PvFace& e) { return (e.xb - e.xa + 1) * (e.yb - e.ya + 1); }

// ------------------------------------------------------------------------------------------------------------- pieces of the passes
// per frame: zbuf [R*R] keys, then large = [count - 1 (0xFFFFFFFF: none), face indices ...]
__device__ __forceinline__ unsigned long long* pv_zbuf(void* scratch, long stride, int n) { return (unsigned long long*)((char*)scratch + stride * n); }

// the pixel centres first, first + step, ... of the face's box, under face index f
__device__ __forceinline__ void pv_walk(const PvFace& e, int f, int first, int step, int R, unsigned long long* __restrict__ zbuf) {
  const int w = e.xb - e.xa + 1, cnt = w * (e.yb - e.ya + 1);
  for (int k = first; k < cnt; k += step) {
    const int xi = e.xa + k % w, yi = e.ya + k / w;
    long long w0, w1, w2;
    if (pv_weights(e, xi, yi, w0, w1, w2)) atomicMin(&zbuf[(long)yi * R + xi], pv_key(e, w0, w1, w2, f));
  }
}
// every face once: at most F entries (a scratch that did not come in as 0xFF starts the count anywhere: nothing is written past the list)
__device__ __forceinline__ void pv_list(unsigned* __restrict__ large, int F, int f) {
  const unsigned slot = atomicAdd(&large[0], 1u) + 1u;
  if (slot < (unsigned)F) large[1 + slot] = (unsigned)f;
}
// a tile's lane (pixel xi, yi; `inside` the raster) takes a listed face's key into its running minimum
__device__ __forceinline__ void pv_tile_key(const PvFace& e, int f, int tx0, int ty0, int xi, int yi, bool inside, unsigned long long& best) {
  if (e.xb < tx0 || e.xa > tx0 + PV_TILE - 1 || e.yb < ty0 || e.ya > ty0 + PV_TILE - 1) return;     // (uniform over the workgroup)
  long long w0, w1, w2;
  if (!inside || !pv_weights(e, xi, yi, w0, w1, w2)) return;
  const unsigned long long key = pv_key(e, w0, w1, w2, f);
  best = key < best ? key : best;
}
// ambient + (1 - ambient) |n . l| / (|n| |l|) with the world-space normal of (i0, i1, i2)
__device__ __forceinline__ float pv_flat_shade(const float* __restrict__ vw, int i0, int i1, int i2, const float* __restrict__ l, float ambient) {
  const float* a = vw + 3 * (long)i0;
  const float* b = vw + 3 * (long)i1;
  const float* d = vw + 3 * (long)i2;
  const float ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], tx = d[0] - a[0], ty = d[1] - a[1], tz = d[2] - a[2];
  const float nx = uy * tz - uz * ty, ny = uz * tx - ux * tz, nz = ux * ty - uy * tx;
  const float nn = sqrtf((nx * nx + ny * ny) + nz * nz) * sqrtf((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2]);
  return nn > 0.f ? ambient + (1.f - ambient) * fminf(fabsf((nx * l[0] + ny * l[1]) + nz * l[2]) / nn, 1.f) : ambient;
}
// Where a shaded pixel takes its unlit colour from, given the winner's oriented corners and their perspective-correct weights l_i (den =
// (l0 + l1) + l2): the corners' colours (a mesh without colours: a constant grey), or a texture under the corners' UVs (csrc/avc_bake.h).
struct PvVertexColours {
  const unsigned char* __restrict__ colors;
  int csize;
  float grey;
  __device__ __forceinline__ void fetch(const PvFace& e, float l0, float l1, float l2, float den, float col[3]) const {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      col[ch] = grey;
      if (colors)
        col[ch] = ((l0 * (float)colors[(long)csize * e.i0 + ch] + l1 * (float)colors[(long)csize * e.i1 + ch]) +
                   l2 * (float)colors[(long)csize * e.i2 + ch]) / den;
    }
  }
};
struct PvTexture {
  const float* __restrict__ uv;                // [V,2]
  const unsigned char* __restrict__ texels;    // [T,T,3]
  int T;
  __device__ __forceinline__ void fetch(const PvFace& e, float l0, float l1, float l2, float den, float col[3]) const {
    const float* a = uv + 2 * (long)e.i0;
    const float* b = uv + 2 * (long)e.i1;
    const float* c = uv + 2 * (long)e.i2;
    const float u = ((l0 * a[0] + l1 * b[0]) + l2 * c[0]) / den, v = ((l0 * a[1] + l1 * b[1]) + l2 * c[1]) / den;
    const float x = u * (float)T - 0.5f, y = v * (float)T - 0.5f;
    const float xf = floorf(x), yf = floorf(y);
    const float fx = x - xf, fy = y - yf;
    // clamp-to-edge (a NaN goes to texel 0: fminf / fmaxf return the other operand)
    const int x0 = (int)fminf(fmaxf(xf, 0.f), (float)(T - 1)), x1 = (int)fminf(fmaxf(xf + 1.f, 0.f), (float)(T - 1));
    const int y0 = (int)fminf(fmaxf(yf, 0.f), (float)(T - 1)), y1 = (int)fminf(fmaxf(yf + 1.f, 0.f), (float)(T - 1));
    const unsigned char* r0 = texels + 3 * (long)y0 * T;
    const unsigned char* r1 = texels + 3 * (long)y1 * T;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float top = (float)r0[3 * x0 + ch] * (1.f - fx) + (float)r0[3 * x1 + ch] * fx;
      const float bottom = (float)r1[3 * x0 + ch] * (1.f - fx) + (float)r1[3 * x1 + ch] * fx;
      col[ch] = top * (1.f - fy) + bottom * fy;
    }
  }
};
// the colour of pixel (xi, yi), which the untouched face e won: the source's perspective-correct colour times the flat shade
template <typename Src>
__device__ __forceinline__ void pv_shade_face(const PvFace& e, const i4* __restrict__ proj, const float* __restrict__ vw, const Src& src,
                                              const float* __restrict__ l, float ambient, int xi, int yi, float c[3]) {
  long long w0, w1, w2;
  pv_weights(e, xi, yi, w0, w1, w2);
  const float l0 = (float)w0 * __uint_as_float((unsigned)proj[e.i0][3]);
  const float l1 = (float)w1 * __uint_as_float((unsigned)proj[e.i1][3]);
  const float l2 = (float)w2 * __uint_as_float((unsigned)proj[e.i2][3]);
  const float den = (l0 + l1) + l2;
  const float shade = pv_flat_shade(vw, e.i0, e.i1, e.i2, l, ambient);
  float col[3];
  src.fetch(e, l0, l1, l2, den, col);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) c[ch] = col[ch] * shade;
}
__device__ __forceinline__ void pv_shade_plain(const PvFace& e, const i4* __restrict__ proj, const float* __restrict__ vw,
                                               const unsigned char* __restrict__ colors, int csize, const float* __restrict__ l, float ambient,
                                               float grey, int xi, int yi, float c[3]) {
  pv_shade_face(e, proj, vw, PvVertexColours{colors, csize, grey}, l, ambient, xi, yi, c);
}
// the box average of an output pixel, rounded to nearest
__device__ __forceinline__ void pv_store_pixel(unsigned char* __restrict__ image, long at, const float acc[3], int ss) {
  const float inv = 1.f / (float)(ss * ss);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) image[at * 3 + ch] = (unsigned char)fminf(fmaxf(floorf(acc[ch] * inv + 0.5f), 0.f), 255.f);
}
#endif
