// Driving the generated avatar with a motion (AvatarGen/AppearanceGen/drive.py, generate_animation :308-376): the three steps of that
// script whose cost grows with the mesh.
//
// 1. avc_nearest_point: find_nearest_ind (drive.py:235-240), the nearest template vertex of every mesh vertex.  The reference builds the
//    [M, K, 3] float64 difference array and takes np.argmin of ((t - q) ** 2).sum(-1); here one lane owns NP_QPL queries and walks the
//    template in ascending index order through LDS tiles (every lane reads the same address: broadcast), with the SAME fp64 arithmetic --
//    the float32 inputs widened exactly, a subtraction, a square, (dx^2 + dy^2) + dz^2 left to right, no FMA contraction (the pragma below)
//    -- and a strict `<` running minimum, i.e. np.argmin's first-index rule on ties.  The result is bit-identical to the reference's.
// 2. avc_mesh_components / avc_mesh_largest_island / avc_mesh_compact: cleanup_mesh (drive.py:172-210), the largest connected island of
//    the triangle-edge graph.  Components by hooking with atomicCAS onto the smaller root plus path halving (Jaiganesh and Burtscher,
//    "A High-Performance Connected Components Implementation for GPUs", HPDC 2018): one pass over the triangles, no rounds, so the cost
//    does not grow with the graph's diameter.  Every parent pointer points at a smaller index, so a root is the smallest vertex of its
//    tree and the final label -- the smallest vertex index of the component -- does not depend on scheduling.  The reference's BFS
//    discovers islands from the lowest unvisited vertex and keeps the first of equally large ones (strict `>`): the biggest count wins,
//    a tie goes to the smallest label, which one 64-bit atomicMax of (count, ~label) picks.  Compaction keeps the order (exclusive scans
//    by the caller) and remaps the triangles.  Integer atomics only.
// 3. avc_skin_apply: inv_lbs / lbs (drive.py:242-265) once the per-template transforms are known: every mesh vertex takes the 3 x 4
//    transform of its nearest template vertex, out[t, m] = xf[t, idx[m]] (p[m], 1).  Bound by the write of out.
#include "avc_common.h"
#include "../../include/avc.h"

#pragma clang fp contract(off)   // the nearest-point distances must be numpy's: no fused multiply-adds

// ------------------------------------------------------------------------------------------------------------- nearest point
#define NP_THREADS 256
#define NP_QPL 2          // queries per lane
#define NP_TILE 1024      // template points per LDS tile (24 KiB of fp64)
typedef double d2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(NP_THREADS) void np_nearest_kernel(const float* __restrict__ q, int M, const float* __restrict__ ref, int K,
                                                               int* __restrict__ idx) {
  __shared__ d2 s_xy[NP_TILE];
  __shared__ double s_z[NP_TILE];
  const int tid = threadIdx.x;
  const long base = (long)blockIdx.x * (NP_THREADS * NP_QPL);
  double qx[NP_QPL], qy[NP_QPL], qz[NP_QPL], best[NP_QPL];
  int bi[NP_QPL];
#pragma unroll
  for (int r = 0; r < NP_QPL; ++r) {
    const long m = base + r * NP_THREADS + tid;
    const bool ok = m < M;
    qx[r] = ok ? (double)q[3 * m] : 0.0;
    qy[r] = ok ? (double)q[3 * m + 1] : 0.0;
    qz[r] = ok ? (double)q[3 * m + 2] : 0.0;
    best[r] = __builtin_inf();
    bi[r] = 0;
  }
  for (int k0 = 0; k0 < K; k0 += NP_TILE) {
    const int n = min(NP_TILE, K - k0);
    __syncthreads();                                   // every lane is done with the previous tile
    for (int i = tid; i < n; i += NP_THREADS) {
      const float* t = ref + 3L * (k0 + i);
      s_xy[i] = d2{(double)t[0], (double)t[1]};
      s_z[i] = (double)t[2];
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < n; ++i) {
      const d2 xy = s_xy[i];
      const double tz = s_z[i];
#pragma unroll
      for (int r = 0; r < NP_QPL; ++r) {
        // numpy: (tv - new_vertices) ** 2, then .sum(-1) left to right
        const double dx = xy.x - qx[r], dy = xy.y - qy[r], dz = tz - qz[r];
        const double s = (dx * dx + dy * dy) + dz * dz;
        if (s < best[r]) {
          best[r] = s;
          bi[r] = k0 + i;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < NP_QPL; ++r) {
    const long m = base + r * NP_THREADS + tid;
    if (m < M) idx[m] = bi[r];
  }
}

extern "C" int avc_nearest_point(const float* q, int M, const float* ref, int K, int* idx, void* stream) {
  if (M < 0 || K < 0 || (M > 0 && K == 0)) { avc_set_error("avc_nearest_point: bad sizes"); return 1; }
  if (M == 0) return 0;
  if (!q || !ref || !idx) { avc_set_error("avc_nearest_point: NULL buffer"); return 1; }
  const int per_block = NP_THREADS * NP_QPL;
  hipLaunchKernelGGL(np_nearest_kernel, dim3((M + per_block - 1) / per_block), dim3(NP_THREADS), 0, (hipStream_t)stream, q, M, ref, K, idx);
  return avc_check_launch("avc_nearest_point");
}

// ------------------------------------------------------------------------------------------------------------- connected components
// parent[] is read while other lanes hook roots: relaxed agent-scope atomics, so no lane keeps working from a stale cached copy
__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void cc_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of v's tree with path halving (every pointer written is an ancestor of its vertex: the forest stays valid)
__device__ __forceinline__ int cc_find(int* parent, int v) {
  int par = cc_load(parent + v);
  if (par != v) {
    int prev = v, next;
    while (par > (next = cc_load(parent + par))) {
      cc_store(parent + prev, next);
      prev = par;
      par = next;
    }
  }
  return par;
}

// join the trees of a and b: the larger root is hooked onto the smaller one; a failed CAS means that root was hooked meanwhile
__device__ __forceinline__ void cc_union(int* parent, int a, int b) {
  int ra = cc_find(parent, a), rb = cc_find(parent, b);
  while (ra != rb) {
    if (ra < rb) {
      const int old = atomicCAS(parent + rb, rb, ra);
      if (old == rb) break;
      rb = cc_find(parent, old);
    } else {
      const int old = atomicCAS(parent + ra, ra, rb);
      if (old == ra) break;
      ra = cc_find(parent, old);
    }
  }
}

// the corners of triangle f; false if one lies outside [0, NV) (such a triangle is ignored: nothing is read or written through it)
__device__ __forceinline__ bool cc_tri(const int* tris, long f, int NV, int& a, int& b, int& c) {
  a = tris[3 * f];
  b = tris[3 * f + 1];
  c = tris[3 * f + 2];
  return (unsigned)a < (unsigned)NV && (unsigned)b < (unsigned)NV && (unsigned)c < (unsigned)NV;
}

__global__ __launch_bounds__(256) void cc_init_kernel(int* __restrict__ parent, int NV) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v < NV) parent[v] = (int)v;
}

// one thread per triangle: the edges a-b and b-c connect all three corners
__global__ __launch_bounds__(256) void cc_hook_kernel(const int* __restrict__ tris, int F, int NV, int* parent) {
  const long f = (long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F) return;
  int a, b, c;
  if (!cc_tri(tris, f, NV, a, b, c)) return;
  cc_union(parent, a, b);
  cc_union(parent, b, c);
}

// after the hooking: every vertex points straight at its root (roots do not change any more)
__global__ __launch_bounds__(256) void cc_flatten_kernel(int* parent, int NV) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v >= NV) return;
  int r = cc_load(parent + v);
  const int first = r;
  int next;
  while (r != (next = cc_load(parent + r))) r = next;
  if (r != first) cc_store(parent + v, r);
}

extern "C" int avc_mesh_components(const int* tris, int F, int NV, int* label, void* stream) {
  if (F < 0 || NV < 0) { avc_set_error("avc_mesh_components: bad sizes"); return 1; }
  if (NV == 0) return 0;
  if (!label || (F && !tris)) { avc_set_error("avc_mesh_components: NULL buffer"); return 1; }
  hipStream_t s = (hipStream_t)stream;
  const int gv = (NV + 255) / 256;
  hipLaunchKernelGGL(cc_init_kernel, dim3(gv), dim3(256), 0, s, label, NV);
  if (F) hipLaunchKernelGGL(cc_hook_kernel, dim3((F + 255) / 256), dim3(256), 0, s, tris, F, NV, label);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(gv), dim3(256), 0, s, label, NV);
  return avc_check_launch("avc_mesh_components");
}

// Island sizes.  One atomicAdd per vertex would serialise on the big island's counter (measured 27 ms for 2.3 M vertices at 512^3,
// profiles/r08_drive_summary.md): marching-cubes vertex order is spatially coherent, so a lane counts runs of equal labels over
// CC_RUN consecutive vertices and the wavefront sums the lanes whose last run has the first lane's label before one atomic.
#define CC_RUN 16
__global__ __launch_bounds__(256) void cc_count_kernel(const int* __restrict__ label, int NV, int* __restrict__ count) {
  const long v0 = ((long)blockIdx.x * 256 + threadIdx.x) * CC_RUN;
  int cur = -1, n = 0;
  for (int i = 0; i < CC_RUN; ++i) {
    const long v = v0 + i;
    if (v >= NV) break;
    const int l = label[v];
    if (l != cur) {
      if (n) atomicAdd(count + cur, n);
      cur = l;
      n = 0;
    }
    ++n;
  }
  const int lead = __shfl(cur, 0);                       // (lanes past the end hold cur = -1, n = 0)
  const int s = wave_sum(cur == lead ? n : 0);
  if (cur != lead && n) atomicAdd(count + cur, n);
  if ((threadIdx.x & 63) == 0 && lead >= 0 && s) atomicAdd(count + lead, s);
}

// the island to keep: largest count, ties to the smallest label = the maximum of (count << 32 | ~label)
__global__ __launch_bounds__(256) void cc_pick_kernel(const int* __restrict__ label, int NV, const int* __restrict__ count,
                                                      unsigned long long* __restrict__ best) {
  const long v = (long)blockIdx.x * 256 + threadIdx.x;
  if (v >= NV || label[v] != (int)v) return;
  atomicMax(best, ((unsigned long long)(unsigned)count[v] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)v));
}

// vflag[v] = v is in the kept island; tflag[f] = triangle f is (its corners share a label: the first corner decides)
__global__ __launch_bounds__(256) void cc_flag_kernel(const int* __restrict__ tris, int F, int NV, const int* __restrict__ label,
                                                      const unsigned long long* __restrict__ best, int* __restrict__ vflag, int* __restrict__ tflag) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const int keep = (int)(0xFFFFFFFFu - (unsigned)(*best & 0xFFFFFFFFull));
  if (i < NV) vflag[i] = label[i] == keep ? 1 : 0;
  if (i < F) {
    int a, b, c;
    tflag[i] = cc_tri(tris, i, NV, a, b, c) && label[a] == keep ? 1 : 0;
  }
}

extern "C" int avc_mesh_largest_island(const int* tris, int F, int NV, const int* label, int* count, unsigned long long* best, int* vflag,
                                       int* tflag, void* stream) {
  if (F < 0 || NV < 0) { avc_set_error("avc_mesh_largest_island: bad sizes"); return 1; }
  if (NV == 0) return 0;
  if (!label || !count || !best || !vflag || (F && (!tris || !tflag))) { avc_set_error("avc_mesh_largest_island: NULL buffer"); return 1; }
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(count, 0, sizeof(int) * (size_t)NV, s) != hipSuccess || hipMemsetAsync(best, 0, sizeof(*best), s) != hipSuccess) {
    avc_set_error("avc_mesh_largest_island: hipMemsetAsync failed");
    return 1;
  }
  const int gv = (NV + 255) / 256;
  hipLaunchKernelGGL(cc_count_kernel, dim3((NV + 256 * CC_RUN - 1) / (256 * CC_RUN)), dim3(256), 0, s, label, NV, count);
  hipLaunchKernelGGL(cc_pick_kernel, dim3(gv), dim3(256), 0, s, label, NV, count, best);
  hipLaunchKernelGGL(cc_flag_kernel, dim3((max(NV, F) + 255) / 256), dim3(256), 0, s, tris, F, NV, label, best, vflag, tflag);
  return avc_check_launch("avc_mesh_largest_island");
}

__global__ __launch_bounds__(256) void cc_compact_vertices_kernel(const float* __restrict__ v, const unsigned* __restrict__ colors, int NV,
                                                                  const int* __restrict__ vflag, const int* __restrict__ vid,
                                                                  float* __restrict__ v_out, unsigned* __restrict__ c_out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= NV || !vflag[i]) return;
  const long o = vid[i];
  v_out[3 * o] = v[3 * i];
  v_out[3 * o + 1] = v[3 * i + 1];
  v_out[3 * o + 2] = v[3 * i + 2];
  if (colors) c_out[o] = colors[i];
}

__global__ __launch_bounds__(256) void cc_compact_triangles_kernel(const int* __restrict__ tris, int F, const int* __restrict__ vid,
                                                                   const int* __restrict__ tflag, const int* __restrict__ tid,
                                                                   int* __restrict__ t_out) {
  const long f = (long)blockIdx.x * 256 + threadIdx.x;
  if (f >= F || !tflag[f]) return;
  const long o = tid[f];
  t_out[3 * o] = vid[tris[3 * f]];
  t_out[3 * o + 1] = vid[tris[3 * f + 1]];
  t_out[3 * o + 2] = vid[tris[3 * f + 2]];
}

extern "C" int avc_mesh_compact(const float* v, const unsigned* colors, const int* tris, int F, int NV, const int* vflag, const int* vid,
                                const int* tflag, const int* tid, float* v_out, unsigned* c_out, int* t_out, void* stream) {
  if (F < 0 || NV < 0) { avc_set_error("avc_mesh_compact: bad sizes"); return 1; }
  if (NV == 0) return 0;
  if (!v || !vflag || !vid || !v_out || (colors && !c_out) || (F && (!tris || !tflag || !tid || !t_out))) {
    avc_set_error("avc_mesh_compact: NULL buffer");
    return 1;
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cc_compact_vertices_kernel, dim3((NV + 255) / 256), dim3(256), 0, s, v, colors, NV, vflag, vid, v_out, c_out);
  if (F) hipLaunchKernelGGL(cc_compact_triangles_kernel, dim3((F + 255) / 256), dim3(256), 0, s, tris, F, vid, tflag, tid, t_out);
  return avc_check_launch("avc_mesh_compact");
}

// ------------------------------------------------------------------------------------------------------------- skinning gather
// out viewed as T * M vertices of 12 bytes: lane j writes vertices 4j .. 4j + 3 = 48 bytes = three 16-byte stores (16-byte aligned
// whatever M is); xf (K x 48 bytes per frame) stays in L2.  An index outside [0, K) writes NaN and reads nothing (include/avc.h: the
// caller checks idx).
__device__ __forceinline__ void skin_one(const float* __restrict__ xf, const int* __restrict__ idx, const float* __restrict__ p, int K, long t,
                                         long m, float* o) {
  const int k = idx[m];
  if ((unsigned)k >= (unsigned)K) {
    o[0] = o[1] = o[2] = __builtin_nanf("");
    return;
  }
  const f4* a = reinterpret_cast<const f4*>(xf + (t * K + k) * 12);
  const f4 r0 = a[0], r1 = a[1], r2 = a[2];
  const float x = p[3 * m], y = p[3 * m + 1], z = p[3 * m + 2];
  o[0] = __builtin_fmaf(r0[0], x, __builtin_fmaf(r0[1], y, __builtin_fmaf(r0[2], z, r0[3])));
  o[1] = __builtin_fmaf(r1[0], x, __builtin_fmaf(r1[1], y, __builtin_fmaf(r1[2], z, r1[3])));
  o[2] = __builtin_fmaf(r2[0], x, __builtin_fmaf(r2[1], y, __builtin_fmaf(r2[2], z, r2[3])));
}

__global__ __launch_bounds__(256) void skin_apply_kernel(const float* __restrict__ xf, const int* __restrict__ idx, const float* __restrict__ p,
                                                         int M, int K, long total, float* __restrict__ out) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  const long e0 = 4 * j;
  if (e0 >= total) return;
  long t = e0 / M, m = e0 - t * M;
  float o[12];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (e0 + u < total) skin_one(xf, idx, p, K, t, m, o + 3 * u);
    if (++m == M) {
      m = 0;
      ++t;
    }
  }
  if (e0 + 4 <= total) {
    f4* dst = reinterpret_cast<f4*>(out + 3 * e0);
    AVC_NT_STORE((f4{o[0], o[1], o[2], o[3]}), dst);
    AVC_NT_STORE((f4{o[4], o[5], o[6], o[7]}), dst + 1);
    AVC_NT_STORE((f4{o[8], o[9], o[10], o[11]}), dst + 2);
  } else {
    for (long u = 0; u < 3 * (total - e0); ++u) out[3 * e0 + u] = o[u];
  }
}

extern "C" int avc_skin_apply(const float* xf, const int* idx, const float* p, int M, int K, int T, float* out, void* stream) {
  if (M < 0 || T < 0 || K <= 0) { avc_set_error("avc_skin_apply: bad sizes"); return 1; }
  if (M == 0 || T == 0) return 0;
  if (!xf || !idx || !p || !out) { avc_set_error("avc_skin_apply: NULL buffer"); return 1; }
  if (((unsigned long long)out & 15ull) || ((unsigned long long)xf & 15ull)) { avc_set_error("avc_skin_apply: out / xf not 16-byte aligned"); return 1; }
  const long total = (long)T * M;
  const long lanes = (total + 3) / 4;
  hipLaunchKernelGGL(skin_apply_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, xf, idx, p, M, K, total, out);
  return avc_check_launch("avc_skin_apply");
}
