// Texture bake (avatarclip_amd/bake.py): the colour of a dense mesh carried onto the texture atlas of a simplified one.  The hot path is
// the closest point of a triangle soup for millions of fp64 queries; csrc/avc_bake.h states the arithmetic, the grid and the atlas.
//
// 1. avc_bake_tri_keys / avc_bake_cell_starts: a uniform grid over the dense triangles, binned by centroid cell.  The caller sorts the
//    64-bit keys (torch.sort, as rig.simplify_mesh sorts its cell keys); a cell is then a run of the sorted array with its triangles in
//    ascending index, and one lane per position writes the starts of the cells between its predecessor's and its own -- the flag (a cell
//    changes here) and the fill in one pass, no scan.  Degenerate triangles sort behind the last cell and are never visited.
// 2. avc_bake_query: one query per lane, every candidate corner in registers, no LDS: the queries of a bake arrive chart by chart, so the
//    lanes of a wavefront walk the same cells and their loads of a triangle's corners hit the same cache lines.  A row of cells along x is
//    ONE run of the sorted array, so a shell of Chebyshev radius k costs O(k^2) pairs of starts, not O(k^3).  The result is exact whatever
//    the triangle sizes: an unvisited triangle's centroid lies at least sqrt(o2 + ((k - 1) cell)^2) from the query (o2 = squared distance
//    from the query to the grid's box, which is convex and holds every centroid; the query's clamped image lies in cell k = 0 and any
//    cell of shell >= k is more than (k - 1) cells away from it along one axis), and the triangle within r_max of its centroid.  A huge
//    triangle makes r_max large and the walk long; it never makes the answer wrong.
//    256 lanes per workgroup: nothing is shared between lanes, so the block size only sets the launch granularity; the kernel is fp64
//    VALU work (three corners, the query, the dots, the winner: hipcc gives it 116 VGPRs, no scratch, 4 waves per SIMD, which a larger
//    or smaller block would not change).  Reasoned, not swept (profiles/texture_bake.md).
// 3. avc_bake_texel_points / avc_bake_colors: the two ends of a bake, a few fp64 operations per owned texel.
#include "avc_common.h"
#include "avc_bake.h"

#pragma clang fp contract(off)   // every product and sum below is tests/bake_restatement.py's, one rounding each

#define BK_THREADS 256
#define BK_MAX_AXIS 256

__device__ __forceinline__ double bk_dot(const double x[3], const double y[3]) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

// the corners of triangle f widened to fp64; false: an index outside [0, V)
__device__ __forceinline__ bool bk_corners(const float* __restrict__ v, int V, const int* __restrict__ t, int f, double a[3], double b[3], double c[3]) {
  const int i0 = t[3 * (long)f], i1 = t[3 * (long)f + 1], i2 = t[3 * (long)f + 2];
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a[k] = (double)v[3 * (long)i0 + k];
    b[k] = (double)v[3 * (long)i1 + k];
    c[k] = (double)v[3 * (long)i2 + k];
  }
  return true;
}
__device__ __forceinline__ bool bk_degenerate(const double a[3], const double b[3], const double c[3]) {
  double ab[3], ac[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; }
  const double n0 = ab[1] * ac[2] - ab[2] * ac[1], n1 = ab[2] * ac[0] - ab[0] * ac[2], n2 = ab[0] * ac[1] - ab[1] * ac[0];
  return n0 == 0.0 && n1 == 0.0 && n2 == 0.0;
}
// Ericson 5.1.5 in the order of csrc/avc_bake.h: barycentrics of the closest point and its squared distance
__device__ __forceinline__ void bk_closest(const double p[3], const double a[3], const double b[3], const double c[3], double bc[3], double& dist2) {
  double ab[3], ac[3], ap[3], bp[3], cp[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; bp[k] = p[k] - b[k]; cp[k] = p[k] - c[k]; }
  const double d1 = bk_dot(ab, ap), d2 = bk_dot(ac, ap), d3 = bk_dot(ab, bp), d4 = bk_dot(ac, bp), d5 = bk_dot(ab, cp), d6 = bk_dot(ac, cp);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  if (d1 <= 0.0 && d2 <= 0.0) { bc[0] = 1.0; bc[1] = 0.0; bc[2] = 0.0; }
  else if (d3 >= 0.0 && d4 <= d3) { bc[0] = 0.0; bc[1] = 1.0; bc[2] = 0.0; }
  else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { const double s = d1 / (d1 - d3); bc[0] = 1.0 - s; bc[1] = s; bc[2] = 0.0; }
  else if (d6 >= 0.0 && d5 <= d6) { bc[0] = 0.0; bc[1] = 0.0; bc[2] = 1.0; }
  else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { const double w = d2 / (d2 - d6); bc[0] = 1.0 - w; bc[1] = 0.0; bc[2] = w; }
  else if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
    const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    bc[0] = 0.0; bc[1] = 1.0 - w; bc[2] = w;
  } else {
    const double g = 1.0 / ((va + vb) + vc), s = vb * g, w = vc * g;
    bc[0] = (1.0 - s) - w; bc[1] = s; bc[2] = w;
  }
  double e[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) e[k] = p[k] - ((bc[0] * a[k] + bc[1] * b[k]) + bc[2] * c[k]);
  dist2 = bk_dot(e, e);
}
// min(max(floor((x - origin) / cell), 0), n - 1); NaN goes to cell 0
__device__ __forceinline__ int bk_cell(double x, double origin, double cell, int n) {
  const double q = floor((x - origin) / cell);
  return q >= (double)(n - 1) ? n - 1 : (q >= 0.0 ? (int)q : 0);
}

// ------------------------------------------------------------------------------------------------------------- the grid
__global__ __launch_bounds__(BK_THREADS) void bk_tri_keys_kernel(const float* __restrict__ v, int V, const int* __restrict__ t, int F, double ox,
                                                                 double oy, double oz, double cell, int nx, int ny, int nz,
                                                                 long long* __restrict__ keys, double* __restrict__ r2) {
  const int f = blockIdx.x * BK_THREADS + threadIdx.x;
  if (f >= F) return;
  double a[3], b[3], c[3];
  long long ci = (long long)nx * ny * nz;
  double r = 0.0;
  if (bk_corners(v, V, t, f, a, b, c) && !bk_degenerate(a, b, c)) {
    double g[3], ea[3], eb[3], ec[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      g[k] = ((a[k] + b[k]) + c[k]) / 3.0;
      ea[k] = a[k] - g[k]; eb[k] = b[k] - g[k]; ec[k] = c[k] - g[k];
    }
    r = fmax(bk_dot(ea, ea), fmax(bk_dot(eb, eb), bk_dot(ec, ec)));
    ci = ((long long)bk_cell(g[2], oz, cell, nz) * ny + bk_cell(g[1], oy, cell, ny)) * nx + bk_cell(g[0], ox, cell, nx);
  }
  keys[f] = (ci << 32) | (long long)(unsigned)f;
  r2[f] = r;
}

__global__ __launch_bounds__(BK_THREADS) void bk_cell_starts_kernel(const long long* __restrict__ keys, int F, int ncells, int* __restrict__ starts) {
  const int i = blockIdx.x * BK_THREADS + threadIdx.x;
  if (i > F) return;                                                      // lane F closes the table
  const long long lo = i == 0 ? 0 : min((long long)ncells, (keys[i - 1] >> 32)) + 1;     // the first cell this lane may have to fill
  const long long hi = i == F ? (long long)ncells : min((long long)ncells, keys[i] >> 32);
  for (long long c = max(lo, 0ll); c <= hi; ++c) starts[c] = i;
}

extern "C" int avc_bake_tri_keys(const float* v, int V, const int* t, int F, double origin_x, double origin_y, double origin_z, double cell, int nx,
                                 int ny, int nz, long long* keys, double* r2, void* stream) {
  if (V < 0 || F < 0) { avc_set_error("avc_bake_tri_keys: bad sizes"); return 1; }
  if (nx < 1 || ny < 1 || nz < 1 || nx > BK_MAX_AXIS || ny > BK_MAX_AXIS || nz > BK_MAX_AXIS) { avc_set_error("avc_bake_tri_keys: grid axes outside [1, 256]"); return 1; }
  if (!(cell > 0.0) || !(cell < __builtin_inf())) { avc_set_error("avc_bake_tri_keys: the cell size must be positive and finite"); return 1; }
  if (F == 0) return 0;
  if (!t || !keys || !r2 || (V && !v)) { avc_set_error("avc_bake_tri_keys: NULL buffer"); return 1; }
  hipLaunchKernelGGL(bk_tri_keys_kernel, dim3(avc_div_up(F, BK_THREADS)), dim3(BK_THREADS), 0, (hipStream_t)stream, v, V, t, F, origin_x, origin_y,
                     origin_z, cell, nx, ny, nz, keys, r2);
  return avc_check_launch("avc_bake_tri_keys");
}

extern "C" int avc_bake_cell_starts(const long long* keys, int F, int ncells, int* starts, void* stream) {
  if (F < 0 || ncells < 1 || ncells > BK_MAX_AXIS * BK_MAX_AXIS * BK_MAX_AXIS) { avc_set_error("avc_bake_cell_starts: bad sizes"); return 1; }
  if (!starts || (F && !keys)) { avc_set_error("avc_bake_cell_starts: NULL buffer"); return 1; }
  hipLaunchKernelGGL(bk_cell_starts_kernel, dim3(avc_div_up(F + 1, BK_THREADS)), dim3(BK_THREADS), 0, (hipStream_t)stream, keys, F, ncells, starts);
  return avc_check_launch("avc_bake_cell_starts");
}

// ------------------------------------------------------------------------------------------------------------- the query
struct BkBest {
  double d2, b[3];
  int tri, seen;
};
// the candidates of cells x0..x1 of row (y, z): one run of the sorted keys
__device__ __forceinline__ void bk_row(const double p[3], const float* __restrict__ v, int V, const int* __restrict__ t, int F,
                                       const long long* __restrict__ keys, const int* __restrict__ starts, long row, int x0, int x1, BkBest& best) {
  const int s = starts[row + x0], e = min(starts[row + x1 + 1], F);
  for (int i = max(s, 0); i < e; ++i) {
    const int f = (int)(unsigned)(keys[i] & 0xFFFFFFFFll);
    double a[3], b[3], c[3], bc[3], d2;
    if ((unsigned)f >= (unsigned)F || !bk_corners(v, V, t, f, a, b, c)) continue;        // (never taken on the keys of avc_bake_tri_keys)
    bk_closest(p, a, b, c, bc, d2);
    ++best.seen;
    if (d2 < best.d2 || (d2 == best.d2 && f < best.tri)) {
      best.d2 = d2; best.tri = f;
      best.b[0] = bc[0]; best.b[1] = bc[1]; best.b[2] = bc[2];
    }
  }
}

__global__ __launch_bounds__(BK_THREADS) void bk_query_kernel(const double* __restrict__ points, int Q, const float* __restrict__ v, int V,
                                                              const int* __restrict__ t, int F, const long long* __restrict__ keys,
                                                              const int* __restrict__ starts, double ox, double oy, double oz, double cell, int nx,
                                                              int ny, int nz, double r_max, int* __restrict__ tri, double* __restrict__ bary,
                                                              double* __restrict__ dist2, int* __restrict__ visited) {
  const long q = (long)blockIdx.x * BK_THREADS + threadIdx.x;
  if (q >= Q) return;
  const double p[3] = {points[3 * q], points[3 * q + 1], points[3 * q + 2]};
  const double o[3] = {ox, oy, oz};
  const int n[3] = {nx, ny, nz};
  int c[3];
  double o2 = 0.0;                                         // squared distance from the query to the grid's box
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c[k] = bk_cell(p[k], o[k], cell, n[k]);
    const double hi = o[k] + (double)n[k] * cell;
    const double e = p[k] < o[k] ? o[k] - p[k] : (p[k] > hi ? p[k] - hi : 0.0);
    o2 = o2 + e * e;
  }
  BkBest best;
  best.d2 = __builtin_inf(); best.tri = 0x7FFFFFFF; best.seen = 0;
  best.b[0] = best.b[1] = best.b[2] = 0.0;
  const int kmax = max(max(max(c[0], nx - 1 - c[0]), max(c[1], ny - 1 - c[1])), max(c[2], nz - 1 - c[2]));
  for (int k = 0; k <= kmax; ++k) {
    if (k >= 1) {
      const double in = (double)(k - 1) * cell;
      const double lb = sqrt(o2 + in * in) - r_max;
      if (lb > 0.0 && lb * lb > best.d2) break;
    }
    const int z0 = max(0, c[2] - k), z1 = min(nz - 1, c[2] + k), y0 = max(0, c[1] - k), y1 = min(ny - 1, c[1] + k);
    const int xl = c[0] - k, xr = c[0] + k;
    for (int z = z0; z <= z1; ++z)
      for (int y = y0; y <= y1; ++y) {
        const long row = ((long)z * ny + y) * nx;
        if (z - c[2] == k || c[2] - z == k || y - c[1] == k || c[1] - y == k) {
          bk_row(p, v, V, t, F, keys, starts, row, max(0, xl), min(nx - 1, xr), best);         // a face of the shell: the whole row
        } else {                                                                              // (k >= 1 here) its two ends
          if (xl >= 0) bk_row(p, v, V, t, F, keys, starts, row, xl, xl, best);
          if (xr <= nx - 1) bk_row(p, v, V, t, F, keys, starts, row, xr, xr, best);
        }
      }
  }
  const bool hit = best.tri != 0x7FFFFFFF;
  tri[q] = hit ? best.tri : -1;
  bary[3 * q] = best.b[0]; bary[3 * q + 1] = best.b[1]; bary[3 * q + 2] = best.b[2];
  dist2[q] = best.d2;
  if (visited) visited[q] = best.seen;
}

extern "C" int avc_bake_query(const double* points, int Q, const float* v, int V, const int* t, int F, const long long* keys, const int* starts,
                              double origin_x, double origin_y, double origin_z, double cell, int nx, int ny, int nz, double r_max, int* tri,
                              double* bary, double* dist2, int* visited, void* stream) {
  if (Q < 0 || V < 0 || F < 0) { avc_set_error("avc_bake_query: bad sizes"); return 1; }
  if (nx < 1 || ny < 1 || nz < 1 || nx > BK_MAX_AXIS || ny > BK_MAX_AXIS || nz > BK_MAX_AXIS) { avc_set_error("avc_bake_query: grid axes outside [1, 256]"); return 1; }
  if (!(cell > 0.0) || !(cell < __builtin_inf()) || !(r_max >= 0.0)) { avc_set_error("avc_bake_query: needs a positive finite cell size and r_max >= 0"); return 1; }
  if (Q == 0) return 0;
  if (!points || !starts || !tri || !bary || !dist2 || (F && (!v || !t || !keys))) { avc_set_error("avc_bake_query: NULL buffer"); return 1; }
  hipLaunchKernelGGL(bk_query_kernel, dim3((unsigned)(((long)Q + BK_THREADS - 1) / BK_THREADS)), dim3(BK_THREADS), 0, (hipStream_t)stream, points, Q, v,
                     V, t, F, keys, starts, origin_x, origin_y, origin_z, cell, nx, ny, nz, r_max, tri, bary, dist2, visited);
  return avc_check_launch("avc_bake_query");
}

// ------------------------------------------------------------------------------------------------------------- the two ends of a bake
__global__ __launch_bounds__(BK_THREADS) void bk_texel_points_kernel(const int* __restrict__ texels, int Q, int size, int P, int G,
                                                                     const float* __restrict__ sv, int SV, const int* __restrict__ st, int SF,
                                                                     double* __restrict__ points) {
  const long q = (long)blockIdx.x * BK_THREADS + threadIdx.x;
  if (q >= Q) return;
  const int tx = texels[q];
  double out[3] = {__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
  if (tx >= 0 && tx < size * size) {
    const int i = tx % size, j = tx / size;
    const int col = i / P, row = j / P;
    const int a = i - col * P, b = P - 1 - (j - row * P);
    const bool lower = a + b <= P - 1;
    const long f = 2L * ((long)row * G + col) + (lower ? 0 : 1);
    double v0[3], v1[3], v2[3];
    if (col < G && row < G && f < SF && bk_corners(sv, SV, st, (int)f, v0, v1, v2)) {
      const double b1 = lower ? (double)(a - 1) / (double)(P - 4) : (double)(P - 2 - a) / (double)(P - 5);
      const double b2 = lower ? (double)(b - 1) / (double)(P - 4) : (double)(P - 2 - b) / (double)(P - 5);
      const double b0 = (1.0 - b1) - b2;
#pragma unroll
      for (int k = 0; k < 3; ++k) out[k] = (b0 * v0[k] + b1 * v1[k]) + b2 * v2[k];
    }
  }
  points[3 * q] = out[0]; points[3 * q + 1] = out[1]; points[3 * q + 2] = out[2];
}

__global__ __launch_bounds__(BK_THREADS) void bk_colors_kernel(const int* __restrict__ texels, int Q, int size, const int* __restrict__ tri,
                                                               const double* __restrict__ bary, const int* __restrict__ t, int F,
                                                               const unsigned char* __restrict__ colors, int csize, int V,
                                                               unsigned char* __restrict__ image) {
  const long q = (long)blockIdx.x * BK_THREADS + threadIdx.x;
  if (q >= Q) return;
  const int tx = texels[q], f = tri[q];
  if (tx < 0 || tx >= size * size || (unsigned)f >= (unsigned)F) return;
  const int i0 = t[3 * (long)f], i1 = t[3 * (long)f + 1], i2 = t[3 * (long)f + 2];
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return;
  const double b0 = bary[3 * q], b1 = bary[3 * q + 1], b2 = bary[3 * q + 2];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const double x = (b0 * (double)colors[(long)csize * i0 + ch] + b1 * (double)colors[(long)csize * i1 + ch]) + b2 * (double)colors[(long)csize * i2 + ch];
    image[3 * (long)tx + ch] = (unsigned char)fmin(fmax(rint(x), 0.0), 255.0);
  }
}

extern "C" int avc_bake_texel_points(const int* texels, int Q, int size, int P, int G, const float* sv, int SV, const int* st, int SF, double* points,
                                     void* stream) {
  if (Q < 0 || SV < 0 || SF < 0) { avc_set_error("avc_bake_texel_points: bad sizes"); return 1; }
  if (size < 1 || size > 4096 || P < 6 || G < 1 || (long)P * G > size) { avc_set_error("avc_bake_texel_points: needs P >= 6 and P G <= size <= 4096"); return 1; }
  if (Q == 0) return 0;
  if (!texels || !points || !sv || !st) { avc_set_error("avc_bake_texel_points: NULL buffer"); return 1; }
  hipLaunchKernelGGL(bk_texel_points_kernel, dim3((unsigned)(((long)Q + BK_THREADS - 1) / BK_THREADS)), dim3(BK_THREADS), 0, (hipStream_t)stream, texels,
                     Q, size, P, G, sv, SV, st, SF, points);
  return avc_check_launch("avc_bake_texel_points");
}

extern "C" int avc_bake_colors(const int* texels, int Q, int size, const int* tri, const double* bary, const int* t, int F, const unsigned char* colors,
                               int csize, int V, unsigned char* image, void* stream) {
  if (Q < 0 || V < 0 || F < 0 || size < 1 || size > 4096) { avc_set_error("avc_bake_colors: bad sizes"); return 1; }
  if (csize != 3 && csize != 4) { avc_set_error("avc_bake_colors: colours are 3 or 4 bytes per vertex"); return 1; }
  if (Q == 0 || F == 0) return 0;
  if (!texels || !tri || !bary || !t || !colors || !image) { avc_set_error("avc_bake_colors: NULL buffer"); return 1; }
  hipLaunchKernelGGL(bk_colors_kernel, dim3((unsigned)(((long)Q + BK_THREADS - 1) / BK_THREADS)), dim3(BK_THREADS), 0, (hipStream_t)stream, texels, Q,
                     size, tri, bary, t, F, colors, csize, V, image);
  return avc_check_launch("avc_bake_colors");
}
