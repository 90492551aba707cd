// Rigging the generated avatar (Avatar2FBX/export_fbx.py:49-109 and utils/ply_utils.py; avatarclip_amd/rig.py): the steps of that script
// whose cost grows with the mesh, plus the packing of the skin for a glTF file.  Integer atomics are not needed and float atomics are not
// used anywhere: every result is a pure function of its inputs, bit-identical from run to run.
//
// 1. Vertex clustering (simplify_mesh, ply_utils.py:16-19 = open3d's simplify_vertex_clustering with contraction Average, restated from
//    the published algorithm).  avc_rig_cell_keys gives every vertex the word (cell key << 32 | vertex index), the cell index being
//    floor((v - origin) / voxel_size) per axis in fp64, these two operations in this order (no reciprocal, no FMA: the pragma below).  The
//    caller sorts the words (any sort: they are distinct), so a cell is a run whose vertices ascend.  avc_rig_cluster_heads marks the first
//    vertex of every run in VERTEX order; the caller's exclusive scan of those marks is the rank of each cell by its first vertex, i.e.
//    the order in which the cells are first met walking the input.  avc_rig_cluster_average owns one run per lane and sums it
//    sequentially, in increasing input index, in fp64 (runs hold about 4-10 vertices at production settings); position = sum / n rounded
//    to float32, colour = sum of c / 255 over n rounded to float32.
// 2. Triangles.  avc_rig_tri_keys maps the corners to their cells' output indices, rotates the triangle so that its smallest index comes
//    first (orientation kept) and packs three 21-bit indices into one 63-bit key; a triangle with two equal corners gets AVC_RIG_TRI_DROP.
//    The caller sorts the keys STABLY; avc_rig_tri_unique keeps the first triangle of every run of equal keys, which after a stable sort
//    is its first occurrence in the input; avc_rig_tri_compact writes the survivors in input order (the caller's exclusive scan, the
//    pattern of avc_mesh_compact).  Triangles of opposite orientation have different keys: both stay, as in open3d.
// 3. avc_skin_sort_template / avc_skin_pack: the gather + permute of export_fbx.py:73,88 and the influence lists of the file in one pass.
//    The non-zero weights are sorted once per TEMPLATE vertex (K = 6890), weight descending then joint ascending; every mesh vertex then
//    copies its nearest template vertex's list into JOINTS_n / WEIGHTS_n and its dense row into blend_weights [24, M].
// 4. avc_rot_to_quat: rotation matrices -> unit quaternions (x, y, z, w), w >= 0, by Shepperd's method (the largest of the trace and
//    the three diagonal entries picks the component that is computed from a square root; the others follow by division).
#include "avc_common.h"
#include "../../include/avc.h"

#pragma clang fp contract(off)   // the cell indices and the means must be the restatement's: no fused multiply-adds

#define RIG_THREADS 256
#define RIG_JOINTS 24
static inline unsigned rig_blocks(long n) { return (unsigned)((n + RIG_THREADS - 1) / RIG_THREADS); }

// ------------------------------------------------------------------------------------------------------------- clustering
__device__ __forceinline__ unsigned rig_cell_axis(float x, double origin, double voxel) {
  const double c = floor(((double)x - origin) / voxel);
  return (unsigned)fmin(fmax(c, 0.0), 1023.0);             // [0, divisor + 1] for finite input; 10 bits whatever comes
}

__global__ __launch_bounds__(RIG_THREADS) void rig_cell_keys_kernel(const float* __restrict__ v, int N, double ox, double oy, double oz,
                                                                    double voxel, unsigned long long* __restrict__ keyed) {
  const long i = (long)blockIdx.x * RIG_THREADS + threadIdx.x;
  if (i >= N) return;
  const unsigned key = (rig_cell_axis(v[3 * i], ox, voxel) << 20) | (rig_cell_axis(v[3 * i + 1], oy, voxel) << 10) |
                       rig_cell_axis(v[3 * i + 2], oz, voxel);
  keyed[i] = ((unsigned long long)key << 32) | (unsigned long long)(unsigned)i;
}

extern "C" int avc_rig_cell_keys(const float* v, int N, double ox, double oy, double oz, double voxel_size, int voxel_divisor,
                                 long long* keyed, void* stream) {
  if (N < 0) { avc_set_error("avc_rig_cell_keys: bad size"); return 1; }
  if (voxel_divisor < 1 || voxel_divisor > AVC_RIG_MAX_DIVISOR) { avc_set_error("avc_rig_cell_keys: voxel_divisor outside [1, 1022] (10-bit cell indices)"); return 1; }
  if (!(voxel_size > 0.0)) { avc_set_error("avc_rig_cell_keys: voxel_size must be positive"); return 1; }
  if (N == 0) return 0;
  if (!v || !keyed) { avc_set_error("avc_rig_cell_keys: NULL buffer"); return 1; }
  hipLaunchKernelGGL(rig_cell_keys_kernel, dim3(rig_blocks(N)), dim3(RIG_THREADS), 0, (hipStream_t)stream, v, N, ox, oy, oz, voxel_size,
                     (unsigned long long*)keyed);
  return avc_check_launch("avc_rig_cell_keys");
}

__device__ __forceinline__ bool rig_run_head(const unsigned long long* sorted, long i) {
  return i == 0 || (sorted[i] >> 32) != (sorted[i - 1] >> 32);
}
// the vertex of a sorted word; an index outside [0, N) (the caller did not pass what avc_rig_cell_keys wrote) reads and writes nothing
__device__ __forceinline__ bool rig_vertex(unsigned long long w, int N, long& vtx) {
  vtx = (long)(w & 0xFFFFFFFFull);
  return vtx < N;
}

__global__ __launch_bounds__(RIG_THREADS) void rig_cluster_heads_kernel(const unsigned long long* __restrict__ sorted, int N,
                                                                        int* __restrict__ first_flag) {
  const long i = (long)blockIdx.x * RIG_THREADS + threadIdx.x;
  if (i >= N || !rig_run_head(sorted, i)) return;
  long vtx;
  if (rig_vertex(sorted[i], N, vtx)) first_flag[vtx] = 1;
}

extern "C" int avc_rig_cluster_heads(const long long* sorted, int N, int* first_flag, void* stream) {
  if (N < 0) { avc_set_error("avc_rig_cluster_heads: bad size"); return 1; }
  if (N == 0) return 0;
  if (!sorted || !first_flag) { avc_set_error("avc_rig_cluster_heads: NULL buffer"); return 1; }
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(first_flag, 0, sizeof(int) * (size_t)N, s) != hipSuccess) { avc_set_error("avc_rig_cluster_heads: hipMemsetAsync failed"); return 1; }
  hipLaunchKernelGGL(rig_cluster_heads_kernel, dim3(rig_blocks(N)), dim3(RIG_THREADS), 0, s, (const unsigned long long*)sorted, N, first_flag);
  return avc_check_launch("avc_rig_cluster_heads");
}

// one lane per run (the lanes of the other positions leave at once): the run's vertices ascend, so the sums below are the sequential
// fp64 sums in input-index order.  colors: csize bytes per vertex (3 or 4), the first three are used; NULL = no colours.
__global__ __launch_bounds__(RIG_THREADS) void rig_cluster_average_kernel(const unsigned long long* __restrict__ sorted, int N,
                                                                          const float* __restrict__ v, const unsigned char* __restrict__ colors,
                                                                          int csize, const int* __restrict__ first_rank, int M,
                                                                          float* __restrict__ v_out, float* __restrict__ c_out,
                                                                          int* __restrict__ vmap) {
  const long i = (long)blockIdx.x * RIG_THREADS + threadIdx.x;
  if (i >= N || !rig_run_head(sorted, i)) return;
  long vtx;
  if (!rig_vertex(sorted[i], N, vtx)) return;
  const int o = first_rank[vtx];
  if ((unsigned)o >= (unsigned)M) return;                  // (first_rank is not the scan of avc_rig_cluster_heads' marks)
  const unsigned long long cell = sorted[i] >> 32;
  double sx = 0.0, sy = 0.0, sz = 0.0, cr = 0.0, cg = 0.0, cb = 0.0;
  long n = 0;
  for (long j = i; j < N && (sorted[j] >> 32) == cell; ++j) {
    if (!rig_vertex(sorted[j], N, vtx)) continue;
    sx += (double)v[3 * vtx];
    sy += (double)v[3 * vtx + 1];
    sz += (double)v[3 * vtx + 2];
    if (colors) {
      const unsigned char* c = colors + (long)csize * vtx;
      cr += (double)c[0] / 255.0;
      cg += (double)c[1] / 255.0;
      cb += (double)c[2] / 255.0;
    }
    vmap[vtx] = o;
    ++n;
  }
  const double dn = (double)n;
  v_out[3L * o] = (float)(sx / dn);
  v_out[3L * o + 1] = (float)(sy / dn);
  v_out[3L * o + 2] = (float)(sz / dn);
  if (colors) {
    c_out[3L * o] = (float)(cr / dn);
    c_out[3L * o + 1] = (float)(cg / dn);
    c_out[3L * o + 2] = (float)(cb / dn);
  }
}

extern "C" int avc_rig_cluster_average(const long long* sorted, int N, const float* v, const unsigned char* colors, int csize,
                                       const int* first_rank, int M, float* v_out, float* c_out, int* vmap, void* stream) {
  if (N < 0 || M < 0 || M > N) { avc_set_error("avc_rig_cluster_average: bad sizes"); return 1; }
  if (N == 0) return 0;
  if (!sorted || !v || !first_rank || !v_out || !vmap || (colors && !c_out)) { avc_set_error("avc_rig_cluster_average: NULL buffer"); return 1; }
  if (colors && csize != 3 && csize != 4) { avc_set_error("avc_rig_cluster_average: colours are 3 or 4 bytes per vertex"); return 1; }
  hipLaunchKernelGGL(rig_cluster_average_kernel, dim3(rig_blocks(N)), dim3(RIG_THREADS), 0, (hipStream_t)stream,
                     (const unsigned long long*)sorted, N, v, colors, csize, first_rank, M, v_out, c_out, vmap);
  return avc_check_launch("avc_rig_cluster_average");
}

// ------------------------------------------------------------------------------------------------------------- triangles
__global__ __launch_bounds__(RIG_THREADS) void rig_tri_keys_kernel(const int* __restrict__ tris, int F, int N, const int* __restrict__ vmap, int M,
                                                                   int* __restrict__ tri_out, long long* __restrict__ key) {
  const long f = (long)blockIdx.x * RIG_THREADS + threadIdx.x;
  if (f >= F) return;
  const int i0 = tris[3 * f], i1 = tris[3 * f + 1], i2 = tris[3 * f + 2];
  int a = -1, b = -1, c = -1;
  if ((unsigned)i0 < (unsigned)N && (unsigned)i1 < (unsigned)N && (unsigned)i2 < (unsigned)N) {
    a = vmap[i0];
    b = vmap[i1];
    c = vmap[i2];
  }
  const bool ok = (unsigned)a < (unsigned)M && (unsigned)b < (unsigned)M && (unsigned)c < (unsigned)M && a != b && b != c && a != c;
  if (ok) {                                                // rotate, never swap: the orientation stays
    if (b < a && b < c) {
      const int t = a;
      a = b; b = c; c = t;
    } else if (c < a && c < b) {
      const int t = c;
      c = b; b = a; a = t;
    }
  }
  tri_out[3 * f] = a;
  tri_out[3 * f + 1] = b;
  tri_out[3 * f + 2] = c;
  key[f] = ok ? (((long long)a << 42) | ((long long)b << 21) | (long long)c) : AVC_RIG_TRI_DROP;
}

extern "C" int avc_rig_tri_keys(const int* tris, int F, int N, const int* vmap, int M, int* tri_out, long long* key, void* stream) {
  if (F < 0 || N < 0 || M < 0) { avc_set_error("avc_rig_tri_keys: bad sizes"); return 1; }
  if (M > AVC_RIG_MAX_KEYED_VERTICES) { avc_set_error("avc_rig_tri_keys: more than 2^21 output vertices do not fit the 63-bit triangle key"); return 1; }
  if (F == 0) return 0;
  if (!tris || !vmap || !tri_out || !key) { avc_set_error("avc_rig_tri_keys: NULL buffer"); return 1; }
  hipLaunchKernelGGL(rig_tri_keys_kernel, dim3(rig_blocks(F)), dim3(RIG_THREADS), 0, (hipStream_t)stream, tris, F, N, vmap, M, tri_out, key);
  return avc_check_launch("avc_rig_tri_keys");
}

__global__ __launch_bounds__(RIG_THREADS) void rig_tri_unique_kernel(const long long* __restrict__ sorted_key, const long long* __restrict__ order,
                                                                     int F, int* __restrict__ tflag) {
  const long i = (long)blockIdx.x * RIG_THREADS + threadIdx.x;
  if (i >= F) return;
  const long long k = sorted_key[i];
  if (k == AVC_RIG_TRI_DROP || (i > 0 && sorted_key[i - 1] == k)) return;
  const long long f = order[i];
  if (f >= 0 && f < F) tflag[f] = 1;
}

extern "C" int avc_rig_tri_unique(const long long* sorted_key, const long long* order, int F, int* tflag, void* stream) {
  if (F < 0) { avc_set_error("avc_rig_tri_unique: bad size"); return 1; }
  if (F == 0) return 0;
  if (!sorted_key || !order || !tflag) { avc_set_error("avc_rig_tri_unique: NULL buffer"); return 1; }
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(tflag, 0, sizeof(int) * (size_t)F, s) != hipSuccess) { avc_set_error("avc_rig_tri_unique: hipMemsetAsync failed"); return 1; }
  hipLaunchKernelGGL(rig_tri_unique_kernel, dim3(rig_blocks(F)), dim3(RIG_THREADS), 0, s, sorted_key, order, F, tflag);
  return avc_check_launch("avc_rig_tri_unique");
}

__global__ __launch_bounds__(RIG_THREADS) void rig_tri_compact_kernel(const int* __restrict__ tri_in, int F, const int* __restrict__ tflag,
                                                                      const int* __restrict__ tid, int F_out, int* __restrict__ t_out) {
  const long f = (long)blockIdx.x * RIG_THREADS + threadIdx.x;
  if (f >= F || !tflag[f]) return;
  const long o = tid[f];
  if (o < 0 || o >= F_out) return;
  t_out[3 * o] = tri_in[3 * f];
  t_out[3 * o + 1] = tri_in[3 * f + 1];
  t_out[3 * o + 2] = tri_in[3 * f + 2];
}

extern "C" int avc_rig_tri_compact(const int* tri_in, int F, const int* tflag, const int* tid, int F_out, int* t_out, void* stream) {
  if (F < 0 || F_out < 0 || F_out > F) { avc_set_error("avc_rig_tri_compact: bad sizes"); return 1; }
  if (F == 0 || F_out == 0) return 0;
  if (!tri_in || !tflag || !tid || !t_out) { avc_set_error("avc_rig_tri_compact: NULL buffer"); return 1; }
  hipLaunchKernelGGL(rig_tri_compact_kernel, dim3(rig_blocks(F)), dim3(RIG_THREADS), 0, (hipStream_t)stream, tri_in, F, tflag, tid, F_out, t_out);
  return avc_check_launch("avc_rig_tri_compact");
}

// ------------------------------------------------------------------------------------------------------------- skin packing
// One lane per template vertex: insertion sort of its non-zero weights (at most 24; K is a few thousand, the lists live in scratch).
// keep > 0: only the `keep` largest stay and are divided by their fp32 sum, added in list order.
__global__ __launch_bounds__(RIG_THREADS) void rig_skin_sort_kernel(const float* __restrict__ w, int K, int keep, unsigned char* __restrict__ tj,
                                                                    float* __restrict__ tw, int* __restrict__ count) {
  const int k = blockIdx.x * RIG_THREADS + threadIdx.x;
  if (k >= K) return;
  float ws[RIG_JOINTS];
  int js[RIG_JOINTS];
  int n = 0;
  for (int j = 0; j < RIG_JOINTS; ++j) {
    const float x = w[(long)k * RIG_JOINTS + j];
    if (x == 0.f || x != x) continue;                      // (joints ascend: among equal weights the earlier joint stays in front)
    int p = n++;
    while (p > 0 && ws[p - 1] < x) {
      ws[p] = ws[p - 1];
      js[p] = js[p - 1];
      --p;
    }
    ws[p] = x;
    js[p] = j;
  }
  if (keep > 0 && n > keep) n = keep;
  if (keep > 0 && n > 0) {
    float s = 0.f;
    for (int i = 0; i < n; ++i) s += ws[i];
    for (int i = 0; i < n; ++i) ws[i] = ws[i] / s;
  }
  for (int i = 0; i < RIG_JOINTS; ++i) {
    tj[(long)k * RIG_JOINTS + i] = i < n ? (unsigned char)js[i] : (unsigned char)0;
    tw[(long)k * RIG_JOINTS + i] = i < n ? ws[i] : 0.f;
  }
  count[k] = n;
}

extern "C" int avc_skin_sort_template(const float* weights, int K, int keep, unsigned char* tj, float* tw, int* count, void* stream) {
  if (K < 0 || keep < 0) { avc_set_error("avc_skin_sort_template: bad sizes"); return 1; }
  if (K == 0) return 0;
  if (!weights || !tj || !tw || !count) { avc_set_error("avc_skin_sort_template: NULL buffer"); return 1; }
  if (((unsigned long long)tj & 3ull) || ((unsigned long long)tw & 15ull)) { avc_set_error("avc_skin_sort_template: tj / tw not 4- / 16-byte aligned"); return 1; }
  hipLaunchKernelGGL(rig_skin_sort_kernel, dim3(rig_blocks(K)), dim3(RIG_THREADS), 0, (hipStream_t)stream, weights, K, keep, tj, tw, count);
  return avc_check_launch("avc_skin_sort_template");
}

// One lane per mesh vertex: `sets` 4-byte joint words and 16-byte weight vectors copied from the template's sorted list (24 entries per
// template vertex = 6 words / 6 vectors, aligned), and the 24 dense weights written down the columns of blend_weights [24, M] (every
// store of a wavefront is 256 contiguous bytes).  A nearest index outside [0, K) writes zeros and reads nothing.
__global__ __launch_bounds__(RIG_THREADS) void rig_skin_pack_kernel(const float* __restrict__ w, const unsigned* __restrict__ tj,
                                                                    const f4* __restrict__ tw, int K, const int* __restrict__ nearest, int M,
                                                                    int sets, unsigned* __restrict__ joints, f4* __restrict__ wout,
                                                                    float* __restrict__ blend) {
  const long m = (long)blockIdx.x * RIG_THREADS + threadIdx.x;
  if (m >= M) return;
  const int k = nearest[m];
  const bool ok = (unsigned)k < (unsigned)K;
  for (int s = 0; s < sets; ++s) {
    joints[(long)s * M + m] = ok ? tj[(long)k * 6 + s] : 0u;
    wout[(long)s * M + m] = ok ? tw[(long)k * 6 + s] : f4{0.f, 0.f, 0.f, 0.f};
  }
  if (blend) {
#pragma unroll
    for (int j = 0; j < RIG_JOINTS; ++j) blend[(long)j * M + m] = ok ? w[(long)k * RIG_JOINTS + j] : 0.f;
  }
}

extern "C" int avc_skin_pack(const float* weights, const unsigned char* tj, const float* tw, int K, const int* nearest, int M, int sets,
                             unsigned char* joints, float* wout, float* blend_weights, void* stream) {
  if (K <= 0 || M < 0 || sets < 0 || sets > 6) { avc_set_error("avc_skin_pack: bad sizes (at most 6 sets of 4 influences: 24 joints)"); return 1; }
  if (M == 0) return 0;
  if (!weights || !tj || !tw || !nearest || (sets && (!joints || !wout))) { avc_set_error("avc_skin_pack: NULL buffer"); return 1; }
  if (((unsigned long long)tj & 3ull) || ((unsigned long long)joints & 3ull) || ((unsigned long long)tw & 15ull) || ((unsigned long long)wout & 15ull)) {
    avc_set_error("avc_skin_pack: joint buffers not 4-byte or weight buffers not 16-byte aligned");
    return 1;
  }
  hipLaunchKernelGGL(rig_skin_pack_kernel, dim3(rig_blocks(M)), dim3(RIG_THREADS), 0, (hipStream_t)stream, weights, (const unsigned*)tj,
                     (const f4*)tw, K, nearest, M, sets, (unsigned*)joints, (f4*)wout, blend_weights);
  return avc_check_launch("avc_skin_pack");
}

// ------------------------------------------------------------------------------------------------------------- rotations -> quaternions
// Shepperd's method in fp64 on the float32 matrix: of w, x, y, z the one with the largest square (4 q^2 = 1 +- the diagonal) comes from
// the square root, the other three from sums / differences of off-diagonal entries divided by it -- never a division by a small number.
// Then normalised (batch_rodrigues' matrices are orthonormal to float32 rounding only), w made non-negative, rounded to float32.
__global__ __launch_bounds__(RIG_THREADS) void rig_rot_to_quat_kernel(const float* __restrict__ R, long n, f4* __restrict__ q) {
  const long i = (long)blockIdx.x * RIG_THREADS + threadIdx.x;
  if (i >= n) return;
  double m[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) m[e] = (double)R[9 * i + e];
  const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
  const double tr = m00 + m11 + m22;
  double x, y, z, w;
  if (tr >= m00 && tr >= m11 && tr >= m22) {
    w = sqrt(fmax(1.0 + tr, 0.0)) * 0.5;
    const double d = 0.25 / w;
    x = (m21 - m12) * d;
    y = (m02 - m20) * d;
    z = (m10 - m01) * d;
  } else if (m00 >= m11 && m00 >= m22) {
    x = sqrt(fmax(1.0 + m00 - m11 - m22, 0.0)) * 0.5;
    const double d = 0.25 / x;
    w = (m21 - m12) * d;
    y = (m01 + m10) * d;
    z = (m02 + m20) * d;
  } else if (m11 >= m22) {
    y = sqrt(fmax(1.0 - m00 + m11 - m22, 0.0)) * 0.5;
    const double d = 0.25 / y;
    w = (m02 - m20) * d;
    x = (m01 + m10) * d;
    z = (m12 + m21) * d;
  } else {
    z = sqrt(fmax(1.0 - m00 - m11 + m22, 0.0)) * 0.5;
    const double d = 0.25 / z;
    w = (m10 - m01) * d;
    x = (m02 + m20) * d;
    y = (m12 + m21) * d;
  }
  const double len = sqrt(x * x + y * y + z * z + w * w);
  const double s = (w < 0.0 ? -1.0 : 1.0) / len;
  q[i] = f4{(float)(x * s), (float)(y * s), (float)(z * s), (float)fabs(w * s)};
}

extern "C" int avc_rot_to_quat(const float* R, long n, float* q, void* stream) {
  if (n < 0) { avc_set_error("avc_rot_to_quat: bad size"); return 1; }
  if (n == 0) return 0;
  if (!R || !q) { avc_set_error("avc_rot_to_quat: NULL buffer"); return 1; }
  if ((unsigned long long)q & 15ull) { avc_set_error("avc_rot_to_quat: q not 16-byte aligned"); return 1; }
  hipLaunchKernelGGL(rig_rot_to_quat_kernel, dim3(rig_blocks(n)), dim3(RIG_THREADS), 0, (hipStream_t)stream, R, n, (f4*)q);
  return avc_check_launch("avc_rot_to_quat");
}
