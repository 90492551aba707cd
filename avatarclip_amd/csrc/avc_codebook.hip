// K-means for the shape and pose CLIP codebooks (avatarclip_amd/kmeans.py, avatarclip_amd/codebook.py): the assignment of every point to
// its nearest centre and the recomputation of the centres.  The reference only loads the two codebooks (AvatarGen/ShapeGen/main.py:86-91,
// AvatarAnimate/models/pose_generation.py:298-300); the paper makes them by K-Means over latents of the shape VAE and of VPoser.
//
// 1. avc_kmeans_assign.  A lane owns KM_P points and keeps their D coordinates in VGPRs for the whole launch.  The centres are walked in
//    ascending k by the whole wavefront at once: k is wave-uniform, so a centre's D values are SCALAR loads into SGPRs and enter the
//    subtractions as scalar operands -- no LDS, no barrier, no centre tile (kmeans.CENTRE_TILE = 0), and the D-wide read of a centre is
//    paid once per wavefront, i.e. once per 64 KM_P distances.  Per (point, centre) the distance is ONE fp32 chain over d ascending,
//    acc = fma(t, t, acc) with t = x - c: the direct form, so a point equal to a centre gets exactly 0.  A later centre replaces the
//    best only when strictly nearer: ties go to the lower index, whatever the unrolling of the k loop.  profiles/codebook.md says why the
//    scalar path and what bounds the kernel (fp32 VALU issue: 2 D instructions per distance).
// 2. avc_kmeans_update.  The caller sorts the words (assign << 32) | index (the pattern of avc_rig_cell_keys / rig.simplify_mesh), so
//    cluster k is the run [lower_bound(k << 32), lower_bound((k + 1) << 32)) and its point indices ascend.  One lane per (cluster,
//    dimension) finds the run by two binary searches and sums it sequentially in that order in fp32, then divides by the count: one fixed
//    order, no atomics, the same bits every time.  The D lanes of a cluster read consecutive floats of every row.
#include "avc_common.h"
#include "avc_codebook.h"

#pragma clang fp contract(off)   // the sums and the chain are the restatement's: the only fused operations are the fmaf() written below

#define KM_THREADS 256
#define KM_P 4                   // points per lane: 4 independent chains per lane, 4 * 32 coordinate VGPRs at D = 32
#define KM_MAX_K 65536

template <int D>
__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(const float* __restrict__ x, int N, const float* __restrict__ c, int K,
                                                                   int* __restrict__ assign, float* __restrict__ dist) {
  const long base = (long)blockIdx.x * (KM_THREADS * KM_P) + threadIdx.x;
  float xv[KM_P][D];
  float best[KM_P];
  int bi[KM_P];
#pragma unroll
  for (int p = 0; p < KM_P; ++p) {
    const long i = base + (long)p * KM_THREADS;
    best[p] = __builtin_inff();
    bi[p] = 0;
    if (i < N) {
      const f4* row = reinterpret_cast<const f4*>(x + i * D);          // (rows are 64 or 128 bytes: 16-byte aligned with the tensor)
#pragma unroll
      for (int q = 0; q < D / 4; ++q) {
        const f4 v = row[q];
        xv[p][4 * q] = v[0]; xv[p][4 * q + 1] = v[1]; xv[p][4 * q + 2] = v[2]; xv[p][4 * q + 3] = v[3];
      }
    } else {
#pragma unroll
      for (int d = 0; d < D; ++d) xv[p][d] = 0.f;
    }
  }
#pragma unroll 2
  for (int k = 0; k < K; ++k) {
    const float* __restrict__ ck = c + (long)k * D;                    // wave-uniform address: scalar loads
    float cv[D];
#pragma unroll
    for (int d = 0; d < D; ++d) cv[d] = ck[d];
#pragma unroll
    for (int p = 0; p < KM_P; ++p) {
      float acc = 0.f;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const float t = xv[p][d] - cv[d];
        acc = __builtin_fmaf(t, t, acc);
      }
      if (acc < best[p]) {                                             // strictly nearer only: the lower index keeps a tie
        best[p] = acc;
        bi[p] = k;
      }
    }
  }
#pragma unroll
  for (int p = 0; p < KM_P; ++p) {
    const long i = base + (long)p * KM_THREADS;
    if (i < N) {
      assign[i] = bi[p];
      dist[i] = best[p];
    }
  }
}

extern "C" int avc_kmeans_assign(const float* x, int N, int D, const float* c, int K, int* assign, float* dist, void* stream) {
  if (D != 16 && D != 32) { avc_set_error("avc_kmeans_assign: D must be 16 or 32"); return 1; }
  if (N < 1 || K < 1 || K > KM_MAX_K || (long)N * D >= (1L << 31)) { avc_set_error("avc_kmeans_assign: bad sizes (1 <= N, N D < 2^31, 1 <= K <= 65536)"); return 1; }
  if (!x || !c || !assign || !dist) { avc_set_error("avc_kmeans_assign: NULL buffer"); return 1; }
  if (((uintptr_t)x & 15) != 0) { avc_set_error("avc_kmeans_assign: x must be 16-byte aligned"); return 1; }
  const unsigned blocks = (unsigned)(((long)N + KM_THREADS * KM_P - 1) / (KM_THREADS * KM_P));
  hipStream_t s = (hipStream_t)stream;
  if (D == 16) hipLaunchKernelGGL(kmeans_assign_kernel<16>, dim3(blocks), dim3(KM_THREADS), 0, s, x, N, c, K, assign, dist);
  else hipLaunchKernelGGL(kmeans_assign_kernel<32>, dim3(blocks), dim3(KM_THREADS), 0, s, x, N, c, K, assign, dist);
  return avc_check_launch("avc_kmeans_assign");
}

// first position of sorted[0..N) whose word is >= key
__device__ __forceinline__ int km_lower_bound(const unsigned long long* __restrict__ sorted, int N, unsigned long long key) {
  int lo = 0, hi = N;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (sorted[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// one lane per (cluster k, dimension d); D is 16 or 32, so a wavefront holds 4 or 2 whole clusters
__global__ __launch_bounds__(KM_THREADS) void kmeans_update_kernel(const unsigned long long* __restrict__ sorted, int N, const float* __restrict__ x,
                                                                   int D, float* __restrict__ c, int K, int* __restrict__ counts) {
  const long t = (long)blockIdx.x * KM_THREADS + threadIdx.x;
  if (t >= (long)K * D) return;
  const int k = (int)(t / D), d = (int)(t % D);
  const int lo = km_lower_bound(sorted, N, (unsigned long long)k << 32);
  const int hi = km_lower_bound(sorted, N, ((unsigned long long)k + 1ull) << 32);
  float s = 0.f;
  int n = 0;
  for (int j = lo; j < hi; ++j) {                                      // ascending point index: the one summation order
    const unsigned long long i = sorted[j] & 0xffffffffull;
    if (i >= (unsigned long long)N) continue;
    s += x[(long)i * D + d];
    ++n;
  }
  if (d == 0) counts[k] = n;
  if (n > 0) c[(long)k * D + d] = s / (float)n;
}

extern "C" int avc_kmeans_update(const long long* sorted, int N, const float* x, int D, float* c, int K, int* counts, void* stream) {
  if (D != 16 && D != 32) { avc_set_error("avc_kmeans_update: D must be 16 or 32"); return 1; }
  if (N < 1 || K < 1 || K > KM_MAX_K || (long)N * D >= (1L << 31)) { avc_set_error("avc_kmeans_update: bad sizes (1 <= N, N D < 2^31, 1 <= K <= 65536)"); return 1; }
  if (!sorted || !x || !c || !counts) { avc_set_error("avc_kmeans_update: NULL buffer"); return 1; }
  const unsigned blocks = (unsigned)(((long)K * D + KM_THREADS - 1) / KM_THREADS);
  hipLaunchKernelGGL(kmeans_update_kernel, dim3(blocks), dim3(KM_THREADS), 0, (hipStream_t)stream, (const unsigned long long*)sorted, N, x, D, c, K,
                     counts);
  return avc_check_launch("avc_kmeans_update");
}
