// Weight-gradient GEMM of the NeuS MLP backward (main.py:537): dW = sum_points A^T B from the operand panels written by
// avc_render_points_fwd_train (forward-type operands, f16) and avc_render_points_bwd (gradient-type operands, bf16).
#include "avc_common.h"
#include "../../include/avc.h"
#include <type_traits>

// ---------------------------------------------------------------------------------------------
// partial[split][ta][tb] = sum over the split's 32-point blocks, sum_kappa A[blk][ta][kappa] x B[blk][tb][kappa]
// One 8-wave workgroup per (K-split, pair).  Per block the (ta+tb) panel tiles are copied ONCE into an LDS ring by
// global->LDS DMA (WG_DEPTH - 1 blocks in flight under the work on the current one).  The tiles arrive in the producers'
// FRAGMENT layout (lane = point, 8 features per k-step); the contraction over points needs them feature-major (lane =
// feature, 8 points per lane).  gfx950's LDS transpose read does that on the way into the registers: ds_read_b64_tr_b16
// hands lane i of a 16-lane group element (i & 3) of the 8 bytes addressed by lane 4 j + (i >> 2) of the group, for j = 0..3,
// i.e. the column i of a [4 points][16 features] block.  The DMA therefore deals the 16-byte chunks of a tile (chunk (s,h,p)
// = features 16 s + 8 (j >> 2) + 4 h + (j & 3) of point p) to the LDS position (p >> 2) * 16 + (2 s + h) * 4 + (p & 3): the 32
// lanes of a half-wave then read 256 contiguous bytes (no bank conflict) and every DMA instruction still reads whole
// 256-byte runs of the panel.  (Round 1 transposed in the producers; the first round-2 kernel transposed on the matrix core
// in a separate pass through LDS: 68 KiB of extra LDS traffic and one more pipeline stage per block.)
// The 8 waves split the ta x tb output tiles 4 x 2 (2 A tiles x 4 B tiles per wave: 6 tile reads for 8 products) when both
// sides are wide, 8 x 1 or 1 x 8 otherwise.  One operand of every pair is f16 (forward-type), the other bf16: the f16 side is
// converted after the read.  Partials are written with plain stores and summed on the host side of the ABI (no atomics).
// HBM-bound by construction: 2 KiB per tile per block is read exactly once per pair it takes part in.
// ---------------------------------------------------------------------------------------------
// LDS ring geometry, counted vmcnt waits, the LDS transpose read that turns a fragment-layout tile (lane = point) into the
// feature-major MFMA operand, f16 -> bf16
#define WG_TB_MAX 9
#define WG_TILES_MAX 18
#define WG_BUF_BYTES (WG_TILES_MAX * 2048)
constexpr int WG_DEPTH = 4;   // blocks in the LDS ring: one being contracted, WG_DEPTH - 1 copies in flight
// cache policy of the panel -> LDS copies (aux operand of global_load_lds): 2 = nt -- every tile is read exactly once by exactly one
// workgroup.  (Measured at 4 Mi points, profiles/r03_ab_kernels.txt: nt 10.15 ms vs default 10.22; a ring as deep as the LDS allows per
// pair -- 8 slots for the 9/10-tile products, 5 for the 15/16-tile ones -- 10.22 vs 10.23: the kernel does not lack bytes in flight.)
constexpr int WG_DMA_AUX = 2;

// the two operand regions (csrc/avc_mlp.h: PanelLayout): [0] = F region (forward-type, f16), [1] = G region (gradient-type, bf16)
struct WgRegions { const char* base[2]; long stride[2]; };   // byte address of block 0 of the slab, bytes per block

typedef short vs4 __attribute__((__vector_size__(4 * sizeof(short))));
typedef __attribute__((address_space(3))) char lds_char;

// wait until at most `n` of this wave's vector-memory operations are outstanding (n is wave-uniform; the count is an immediate)
__device__ __forceinline__ void wait_vmcnt(int n) {
#define WG_W(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
  switch (n) {
    WG_W(0) WG_W(1) WG_W(2) WG_W(3) WG_W(4) WG_W(5) WG_W(6) WG_W(7) WG_W(8) WG_W(9) WG_W(10) WG_W(11) WG_W(12) WG_W(13) WG_W(14) WG_W(15)
    WG_W(16) WG_W(17) WG_W(18) WG_W(19) WG_W(20) WG_W(21) WG_W(22) WG_W(23) WG_W(24) WG_W(25) WG_W(26) WG_W(27) WG_W(28) WG_W(29) WG_W(30)
    WG_W(31) WG_W(32) WG_W(33) WG_W(34) WG_W(35) WG_W(36)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;   // any other count: conservative
  }
#undef WG_W
}

// operand fragment of k-step t (points 16 t .. 16 t + 15) of the tile at LDS address `tile` (+ this lane's offset): lane
// (feature m = lane & 31, hh = lane >> 5) receives points 16 t + 8 hh + 0..7
__device__ __forceinline__ b8 tr_frag(lds_char* p, int t) {
  struct { vs4 lo, hi; } r;
  r.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<__attribute__((address_space(3))) vs4*>(p + t * 1024));
  r.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<__attribute__((address_space(3))) vs4*>(p + t * 1024 + 256));
  return __builtin_bit_cast(b8, r);
}
__device__ __forceinline__ b8 f16_to_bf16(b8 v) {
  const h8 x = __builtin_bit_cast(h8, v);
  b8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (__bf16)(float)x[j];
  return o;
}

// NI x NK output tiles per wave: A tiles wa + WA i, B tiles wb + WB k
template <int NI, int NK>
__device__ __forceinline__ void weight_grad_body(char* lds, const WgRegions& rg, int pa, int ta_n, int pb,
                                                 int tb_n, int type_a, int type_b, long nblk, float* __restrict__ partial,
                                                 float* __restrict__ bias_partial, int out_elems, int bias_elems, int WA) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int WB = 8 / WA;
  const int wa = wv % WA, wb = wv / WA;
  const int split = blockIdx.x, nsplit = gridDim.x;   // (the pair index is blockIdx.y)
  const long b0 = nblk * split / nsplit, b1 = nblk * (split + 1) / nsplit;
  const int ntile = ta_n + tb_n;
  const int nchunk = ntile * 2;
  const int my_chunks = (nchunk - wv + 7) >> 3;   // DMA instructions this wave issues per block
  constexpr int slot_bytes = WG_BUF_BYTES, depth = WG_DEPTH;
  // source chunk of this lane in DMA instruction c of a tile: LDS position 64 c + lane = (p >> 2) * 16 + (2 s + h) * 4 + (p & 3)
  const int src_lo = ((lane >> 2) & 3) * 32 + 4 * (lane >> 4) + (lane & 3);   // (2 s + h) * 32 + p with p = 4 (lane >> 4) + (lane & 3)
  // operand A lives in region type_a, operand B in region type_b (0 = F region: f16 forward-type tiles, 1 = G region: bf16)
  const char* const base_a = (type_a ? rg.base[1] : rg.base[0]) + (long)pa * 2048;
  const char* const base_b = (type_b ? rg.base[1] : rg.base[0]) + (long)pb * 2048;
  const long stride_a = type_a ? rg.stride[1] : rg.stride[0], stride_b = type_b ? rg.stride[1] : rg.stride[0];
  auto issue = [&](long blk, int slot) {
    for (int c = wv; c < nchunk; c += 8) {
      const int tix = c >> 1;
      const char* tb_ = tix < ta_n ? base_a + blk * stride_a + (long)tix * 2048 : base_b + blk * stride_b + (long)(tix - ta_n) * 2048;
      const char* g = tb_ + (src_lo + (c & 1) * 16) * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                       (__attribute__((address_space(3))) void*)(lds + slot * slot_bytes + c * 1024), 16, 0, WG_DMA_AUX);
    }
  };
  // this lane's byte offset inside a tile for the transpose reads: group g = lane >> 4 = 2 hh + s, i = lane & 15 supplies
  // the 8 bytes (half c >> 1 of chunk (s, h' = c & 1, p = p0 + r)), r = i >> 2, c = i & 3;  p0 = 16 t + 8 hh + 4 u
  const int lane_off = (((lane >> 5) * 2) * 16 + (((lane >> 4) & 1) * 2 + (lane & 1)) * 4 + ((lane & 15) >> 2)) * 16 + 8 * ((lane & 3) >> 1);
  facc acc[NI * NK];
#pragma unroll
  for (int q = 0; q < NI * NK; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
  float bsum[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) bsum[i] = 0.f;
  // Ring of `depth` block buffers, ONE barrier per block: it publishes block blk (every wave has waited for its own chunks) and
  // frees the slot of block blk - 1, which the next copy then overwrites.  Raw barriers + counted vmcnt throughout:
  // __syncthreads() would drain the copies in flight.
  for (int d = 0; d < depth - 1; ++d)
    if (b0 + d < b1) issue(b0 + d, d);
  int slot = 0;
  for (long blk = b0; blk < b1; ++blk) {
    // LDS-DMA completes in issue order: block blk has landed when at most the chunks of the younger blocks are outstanding
    long younger = b1 - 1 - blk;
    if (younger > depth - 2) younger = depth - 2;
    wait_vmcnt((int)younger * my_chunks);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // my reads of block blk - 1 are done
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (blk + depth - 1 < b1) { int ns = slot + depth - 1; if (ns >= depth) ns -= depth; issue(blk + depth - 1, ns); }
    lds_char* buf = (lds_char*)(lds + slot * slot_bytes) + lane_off;
    b8 a[NI][2];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int ta = wa + WA * i;
      if (ta < ta_n) {
        a[i][0] = tr_frag(buf + ta * 2048, 0);
        a[i][1] = tr_frag(buf + ta * 2048, 1);
      }
    }
    b8 bv[NK][2];
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int tb = wb + WB * k;
      if (tb < tb_n) {
        bv[k][0] = tr_frag(buf + (ta_n + tb) * 2048, 0);
        bv[k][1] = tr_frag(buf + (ta_n + tb) * 2048, 1);
      }
    }
    if (type_a == 0) {
#pragma unroll
      for (int i = 0; i < NI; ++i) { a[i][0] = f16_to_bf16(a[i][0]); a[i][1] = f16_to_bf16(a[i][1]); }
    }
    if (type_b == 0) {
#pragma unroll
      for (int k = 0; k < NK; ++k) { bv[k][0] = f16_to_bf16(bv[k][0]); bv[k][1] = f16_to_bf16(bv[k][1]); }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      if (wa + WA * i < ta_n) {
        if (bias_partial && wb == i) {   // the bias row sums of A tile i are the job of the wave column wb = i (balanced across waves)
#pragma unroll
          for (int j = 0; j < 8; ++j) bsum[i] += (float)a[i][0][j] + (float)a[i][1][j];
        }
#pragma unroll
        for (int k = 0; k < NK; ++k) {
          if (wb + WB * k < tb_n) {
            acc[i * NK + k] = MF<b8>::mma(a[i][0], bv[k][0], acc[i * NK + k]);
            acc[i * NK + k] = MF<b8>::mma(a[i][1], bv[k][1], acc[i * NK + k]);
          }
        }
      }
    }
    if (++slot == depth) slot = 0;
  }
  float* dst = partial + (long)split * out_elems;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int ta = wa + WA * i;
    if (ta >= ta_n) continue;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
      const int tb = wb + WB * k;
      if (tb >= tb_n) continue;
      f4* d4 = reinterpret_cast<f4*>(dst + ((long)(ta * tb_n + tb) * 64 + lane) * 16);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f4 v;
        v[0] = acc[i * NK + k][4 * q]; v[1] = acc[i * NK + k][4 * q + 1]; v[2] = acc[i * NK + k][4 * q + 2]; v[3] = acc[i * NK + k][4 * q + 3];
        d4[q] = v;
      }
    }
    if (bias_partial && wb == i) {
      const float s = xhalf_sum(bsum[i]);
      if (lane < 32) bias_partial[(long)split * bias_elems + ta * 32 + lane] = s;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The products the full nets launch (packing.build_layout), with everything the block loop branches on in the run-time bodies made
// a compile-time constant: the tile counts, the wave split, the operand types and whether the pair has a bias.  What depends on the
// wave is chosen ONCE, before the loop (weight_grad_shipped, weight_grad_shipped_9x9).  The block loop is then one straight-line
// region: one counted vmcnt immediate, the barrier, the copy of block blk + WG_DEPTH - 1, the transpose reads, the MFMAs.  Every
// accumulator still receives k-step 0, then k-step 1 of each block, blocks ascending, and the bias sums keep the order of their
// additions: the same bits as the run-time bodies.
// ---------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void wait_vmcnt_imm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// The MC copies one wave issues per block of a TA + TB tile product (chunk c = wv + 8 j of the block, j < MC).  The copies of a
// split are issued block after block, so instruction j keeps the address of its chunk in the next block to copy and steps by its
// region's bytes per block: the addresses of weight_grad_body's issue().
template <int MC, int TA, int TYA, int TYB>
struct WgCopies {
  const char* next[MC];
  long step[MC];
  unsigned src_lo;
  int wv;
  __device__ __forceinline__ WgCopies(const WgRegions& rg, int pa, int pb, long b0, int wv_, int lane) : wv(wv_) {
    src_lo = (((lane >> 2) & 3) * 32 + 4 * (lane >> 4) + (lane & 3)) * 16;
#pragma unroll
    for (int j = 0; j < MC; ++j) {
      const int c = wv + 8 * j, tix = c >> 1;
      const bool in_a = tix < TA;
      step[j] = in_a ? rg.stride[TYA] : rg.stride[TYB];
      next[j] = (in_a ? rg.base[TYA] + (long)(pa + tix) * 2048 : rg.base[TYB] + (long)(pb + tix - TA) * 2048) + b0 * step[j] + (c & 1) * 256;
    }
  }
  __device__ __forceinline__ void issue(char* lds, int slot) {
#pragma unroll
    for (int j = 0; j < MC; ++j) {
      asm("" : "+s"(next[j]));   // the running address stays a scalar; the lanes share one offset register
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(next[j] + src_lo),
                                       (__attribute__((address_space(3))) void*)(lds + slot * WG_BUF_BYTES + (wv + 8 * j) * 1024), 16, 0,
                                       WG_DMA_AUX);
      next[j] += step[j];
    }
  }
};

// The ring of weight_grad_body around contract(buffer of the block): the last WG_DEPTH - 1 blocks of a split, which issue no copy
// and wait for fewer, run in a peeled tail, so that the steady state waits with ONE immediate and issues unconditionally.
template <int MC, class Copies, class Contract>
__device__ __forceinline__ void wg_ring(char* lds, Copies& cp, long b0, long b1, Contract&& contract) {
  constexpr int depth = WG_DEPTH;
  const int n = (int)(b1 - b0);
  for (int d = 0; d < depth - 1; ++d)
    if (d < n) cp.issue(lds, d);
  int slot = 0;
  auto block = [&](auto ahead) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // my reads of block blk - 1 are done
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (decltype(ahead)::value) cp.issue(lds, slot == 0 ? depth - 1 : slot - 1);
    contract(lds + slot * WG_BUF_BYTES);
    if (++slot == depth) slot = 0;
  };
  int i = 0;
  for (; i + depth - 1 < n; ++i) {
    wait_vmcnt_imm<(depth - 2) * MC>();   // LDS-DMA completes in issue order: block b0 + i has landed
    block(std::true_type{});
  }
  for (; i < n; ++i) {
    int younger = n - 1 - i;
    if (younger > depth - 2) younger = depth - 2;
    wait_vmcnt(younger * MC);
    block(std::false_type{});
  }
}

__device__ __forceinline__ int wg_lane_off(int lane) {   // weight_grad_body's lane_off
  return (((lane >> 5) * 2) * 16 + (((lane >> 4) & 1) * 2 + (lane & 1)) * 4 + ((lane & 15) >> 2)) * 16 + 8 * ((lane & 3) >> 1);
}
__device__ __forceinline__ void wg_store_tile(float* dst, int tile, int lane, const facc& v16) {
  f4* d4 = reinterpret_cast<f4*>(dst + ((long)tile * 64 + lane) * 16);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f4 v;
    v[0] = v16[4 * q]; v[1] = v16[4 * q + 1]; v[2] = v16[4 * q + 2]; v[3] = v16[4 * q + 3];
    d4[q] = v;
  }
}
// bsum + the 16 values of the two fragments of an A tile, in weight_grad_body's order
__device__ __forceinline__ float wg_row_sum(float bsum, b8 s0, b8 s1) {
#pragma unroll
  for (int j = 0; j < 8; ++j) bsum += (float)s0[j] + (float)s1[j];
  return bsum;
}

// weight_grad_body<NI, NK> with WA for one TA x TB product.  LASTA / LASTB = this wave has its last A / B slot (the seventh A tile
// of a 7 x 8 product exists only for wa = 0, the ninth B tile of 8 x 9 only for wb = 0), HI = it issues the larger of the two
// possible numbers of copies per block.  k-step 0 of every tile is read first and its MFMAs go over all accumulators before
// k-step 1's, so that no MFMA waits for the one before it.  The bias row sums of A slot i are the job of wave column wb = i: the
// fragments are picked by a select; a wave that is responsible for no slot sums something it never stores.
template <int NI, int NK, int TA, int TB, int WA, int TYA, int TYB, bool BIAS, bool LASTA, bool LASTB, bool HI>
__device__ __forceinline__ void weight_grad_fixed(char* lds, const WgRegions& rg, int pa, int pb, long nblk, float* __restrict__ partial,
                                                  float* __restrict__ bias_partial, int out_elems, int bias_elems) {
  constexpr int WB = 8 / WA, nchunk = 2 * (TA + TB);
  constexpr int MC = HI ? (nchunk + 7) / 8 : nchunk / 8;              // DMA instructions this wave issues per block
  constexpr int NIW = LASTA ? NI : NI - 1, NKW = LASTB ? NK : NK - 1;   // A / B slots of this wave
  static_assert(WA * (NI - 1) < TA && WA * (NI - 2) + WA - 1 < TA && WB * (NK - 1) < TB && WB * (NK - 2) + WB - 1 < TB,
                "only the last slot of either side may be missing for some waves");
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) & 7;
  const int wa = wv % WA, wb = wv / WA;
  const int split = blockIdx.x, nsplit = gridDim.x;
  const long b0 = nblk * split / nsplit, b1 = nblk * (split + 1) / nsplit;
  WgCopies<MC, TA, TYA, TYB> cp(rg, pa, pb, b0, wv, lane);
  const int lane_off = wg_lane_off(lane);
  facc acc[NI * NK];
#pragma unroll
  for (int q = 0; q < NI * NK; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
  float bsum = 0.f;
  wg_ring<MC>(lds, cp, b0, b1, [&](char* slot_buf) {
    lds_char* buf = (lds_char*)slot_buf + lane_off;
    b8 a[NI][2], bv[NK][2];
    auto read = [&](int t) {
#pragma unroll
      for (int i = 0; i < NIW; ++i) a[i][t] = tr_frag(buf + (wa + WA * i) * 2048, t);
#pragma unroll
      for (int k = 0; k < NKW; ++k) bv[k][t] = tr_frag(buf + (TA + wb + WB * k) * 2048, t);
    };
    auto convert = [&](int t) {
      if constexpr (TYA == 0) {
#pragma unroll
        for (int i = 0; i < NIW; ++i) a[i][t] = f16_to_bf16(a[i][t]);
      }
      if constexpr (TYB == 0) {
#pragma unroll
        for (int k = 0; k < NKW; ++k) bv[k][t] = f16_to_bf16(bv[k][t]);
      }
    };
    auto mfmas = [&](int t) {
#pragma unroll
      for (int i = 0; i < NIW; ++i)
#pragma unroll
        for (int k = 0; k < NKW; ++k) acc[i * NK + k] = MF<b8>::mma(a[i][t], bv[k][t], acc[i * NK + k]);
    };
    // While an LDS-DMA is in flight the compiler waits for ALL outstanding LDS reads at the first use of any of them (it cannot
    // count past a FLAT-encoded operation), so the order is pinned: the reads of k-step 0, their conversion (the one full wait),
    // then the reads of k-step 1 under the MFMAs of k-step 0.
    read(0);
    __builtin_amdgcn_sched_barrier(0);
    convert(0);
    __builtin_amdgcn_sched_barrier(0);
    read(1);
    mfmas(0);
    __builtin_amdgcn_sched_barrier(0);
    convert(1);
    mfmas(1);
    if constexpr (BIAS) {
      b8 s0 = a[0][0], s1 = a[0][1];
#pragma unroll
      for (int i = 1; i < NIW; ++i) { s0 = wb == i ? a[i][0] : s0; s1 = wb == i ? a[i][1] : s1; }
      bsum = wg_row_sum(bsum, s0, s1);
    }
  });
  float* dst = partial + (long)split * out_elems;
#pragma unroll
  for (int i = 0; i < NIW; ++i)
#pragma unroll
    for (int k = 0; k < NKW; ++k) wg_store_tile(dst, (wa + WA * i) * TB + wb + WB * k, lane, acc[i * NK + k]);
  if constexpr (BIAS) {
    if (wb < NIW) {
      const float s = xhalf_sum(bsum);
      if (lane < 32) bias_partial[(long)split * bias_elems + (wa + WA * wb) * 32 + lane] = s;
    }
  }
}

// the roles of this wave in a shipped product, picked once
template <int NI, int NK, int TA, int TB, int WA, int TYA, int TYB, bool BIAS>
__device__ __forceinline__ void weight_grad_shipped(char* lds, const WgRegions& rg, int pa, int pb, long nblk, float* __restrict__ partial,
                                                    float* __restrict__ bias_partial, int out_elems, int bias_elems) {
  constexpr int WB = 8 / WA, nchunk = 2 * (TA + TB);
  constexpr bool role_a = WA * (NI - 1) + WA - 1 >= TA, role_b = WB * (NK - 1) + WB - 1 >= TB, role_hi = (nchunk & 7) != 0;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) & 7;
  const bool lasta = !role_a || wv % WA + WA * (NI - 1) < TA, lastb = !role_b || wv / WA + WB * (NK - 1) < TB;
  const bool hi = !role_hi || wv < (nchunk & 7);
#define WG_ROLE(LA, LB, H)                                                                                                            \
  if ((LA || role_a) && (LB || role_b) && (H || role_hi) && lasta == LA && lastb == LB && hi == H)                                  \
    return weight_grad_fixed<NI, NK, TA, TB, WA, TYA, TYB, BIAS, LA || !role_a, LB || !role_b, H || !role_hi>(                        \
        lds, rg, pa, pb, nblk, partial, bias_partial, out_elems, bias_elems);
  WG_ROLE(true, true, true) WG_ROLE(true, true, false) WG_ROLE(true, false, true) WG_ROLE(true, false, false)
  WG_ROLE(false, true, true) WG_ROLE(false, true, false) WG_ROLE(false, false, true) WG_ROLE(false, false, false)
#undef WG_ROLE
}

// weight_grad_body_9x9 (below) for one role of the wave (wa, wb):
//   ROLE 0: wave (0, 0): B tiles 0, 2, .., 8 against A tiles 0 and 4, and B tile 8 against the ninth A tile;
//   ROLE 1: waves (1..3, 0): B tiles 0, 2, .., 8 against A tiles wa and wa + 4;
//   ROLE 2: waves (1..3, 1): B tiles 1, 3, 5, 7 against A tiles wa and wa + 4, B tiles 2 wa + 1 and 2 wa against the ninth A tile;
//   ROLE 3: wave (0, 1): as ROLE 2, and the bias row sums of the ninth A tile.
// A wave of column 1 takes its four B tiles in the order 2 wa + 1, 2 wa + 3, .. (mod 8), so that the one that also meets the ninth A
// tile is slot 0 for every wa: which tile an accumulator belongs to is an address, not a register number.
template <int ROLE, int TYA, int TYB, bool BIAS>
__device__ __forceinline__ void weight_grad_fixed_9x9(char* lds, const WgRegions& rg, int pa, int pb, long nblk, float* __restrict__ partial,
                                                      float* __restrict__ bias_partial, int out_elems, int bias_elems) {
  constexpr int TA = 9, TB = 9;
  constexpr bool COL1 = ROLE >= 2, HAS_X = ROLE != 1;
  constexpr int MC = COL1 ? 4 : 5;      // 36 chunks: five copies per block for waves 0..3, four for waves 4..7
  constexpr int NR = COL1 ? 4 : 5;      // B tiles against A tiles wa, wa + 4
  constexpr int XK = COL1 ? 0 : 4;      // the one of them that also meets the ninth A tile
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) & 7;
  const int wa = wv & 3;
  const int split = blockIdx.x, nsplit = gridDim.x;
  const long b0 = nblk * split / nsplit, b1 = nblk * (split + 1) / nsplit;
  WgCopies<MC, TA, TYA, TYB> cp(rg, pa, pb, b0, wv, lane);
  const int lane_off = wg_lane_off(lane);
  int tb_of[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) tb_of[k] = COL1 ? 1 + 2 * ((wa + k) & 3) : 2 * k;
  facc acc[2 * NR], ex[2];
#pragma unroll
  for (int q = 0; q < 2 * NR; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) ex[q][r] = 0.f;
  float bsum = 0.f, xsum = 0.f;
  wg_ring<MC>(lds, cp, b0, b1, [&](char* slot_buf) {
    lds_char* buf = (lds_char*)slot_buf + lane_off;
    b8 a[2][2], sa[2], bv[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      a[0][t] = tr_frag(buf + wa * 2048, t);
      a[1][t] = tr_frag(buf + (wa + 4) * 2048, t);
      if constexpr (HAS_X) sa[t] = tr_frag(buf + 8 * 2048, t);
      if constexpr (TYA == 0) {
        a[0][t] = f16_to_bf16(a[0][t]); a[1][t] = f16_to_bf16(a[1][t]);
        if constexpr (HAS_X) sa[t] = f16_to_bf16(sa[t]);
      }
    }
    if constexpr (BIAS) bsum = wg_row_sum(bsum, a[COL1][0], a[COL1][1]);      // wave (wa, wb): row sums of A tile wa + 4 wb
    if constexpr (BIAS && ROLE == 3) xsum = wg_row_sum(xsum, sa[0], sa[1]);
    // B fragments are streamed one tile ahead of their MFMAs, as in weight_grad_body_9x9 (all of them do not fit beside 11 accumulators)
    auto load_b = [&](int k, b8* f) {      // (column 1: slot NR is B tile 2 wa, which meets the ninth A tile only)
      const int tb = k < NR ? tb_of[k < NR ? k : 0] : 2 * wa;
      f[0] = tr_frag(buf + (TA + tb) * 2048, 0);
      f[1] = tr_frag(buf + (TA + tb) * 2048, 1);
    };
    b8 nx[2];
    load_b(0, bv);
    nx[0] = bv[0]; nx[1] = bv[1];
#pragma unroll
    for (int k = 0; k < NR + COL1; ++k) {
      if (k + 1 < NR + COL1) load_b(k + 1, nx);
      asm volatile("" : "+v"(nx[0]), "+v"(nx[1]));
      if constexpr (TYB == 0) { bv[0] = f16_to_bf16(bv[0]); bv[1] = f16_to_bf16(bv[1]); }
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (k < NR) {
          acc[k] = MF<b8>::mma(a[0][t], bv[t], acc[k]);
          acc[NR + k] = MF<b8>::mma(a[1][t], bv[t], acc[NR + k]);
          if constexpr (HAS_X) {
            if (k == XK) ex[0] = MF<b8>::mma(sa[t], bv[t], ex[0]);
          }
        } else {
          ex[1] = MF<b8>::mma(sa[t], bv[t], ex[1]);
        }
      }
      bv[0] = nx[0]; bv[1] = nx[1];
    }
  });
  float* dst = partial + (long)split * out_elems;
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    wg_store_tile(dst, wa * TB + tb_of[k], lane, acc[k]);
    wg_store_tile(dst, (wa + 4) * TB + tb_of[k], lane, acc[NR + k]);
  }
  if constexpr (HAS_X) wg_store_tile(dst, 8 * TB + tb_of[XK], lane, ex[0]);
  if constexpr (COL1) wg_store_tile(dst, 8 * TB + 2 * wa, lane, ex[1]);
  if constexpr (BIAS) {
    const float sx = xhalf_sum(bsum);
    if (lane < 32) bias_partial[(long)split * bias_elems + (wa + 4 * COL1) * 32 + lane] = sx;
    if constexpr (ROLE == 3) {
      const float sy = xhalf_sum(xsum);
      if (lane < 32) bias_partial[(long)split * bias_elems + 8 * 32 + lane] = sy;
    }
  }
}
template <int TYA, int TYB, bool BIAS>
__device__ __forceinline__ void weight_grad_shipped_9x9(char* lds, const WgRegions& rg, int pa, int pb, long nblk, float* __restrict__ partial,
                                                        float* __restrict__ bias_partial, int out_elems, int bias_elems) {
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) & 7;
#define WG_ROLE(R) weight_grad_fixed_9x9<R, TYA, TYB, BIAS>(lds, rg, pa, pb, nblk, partial, bias_partial, out_elems, bias_elems)
  if (wv == 0) WG_ROLE(0);
  else if (wv < 4) WG_ROLE(1);
  else if (wv > 4) WG_ROLE(2);
  else WG_ROLE(3);
#undef WG_ROLE
}

// The merged last-layer product: A = [ybar[1:] (8 tiles) | d_sdf row (1 tile)], B = [hs (7) | pe (2)], 9 x 9 output tiles, so that
// [hs | pe] is read from HBM once for the 256 feature rows AND the sdf row.  Waves 4 x 2 over the 8 x 9 part as in the generic
// body (A tiles wa, wa + 4; B tiles wb, wb + 2, ..: 10 products for wb = 0, 8 for wb = 1); the nine products of the ninth A tile go to
// the waves that have the matching B tile in registers anyway: wave (wa, 1) takes B tile 2 wa + 1 and -- one more LDS read -- 2 wa,
// wave (0, 0) takes B tile 8: 12 accumulators at most.  B fragments are streamed one tile ahead of their MFMAs (all five at once,
// as in the generic body, do not fit beside 12 accumulators).
__device__ __forceinline__ void weight_grad_body_9x9(char* lds, const WgRegions& rg, int pa, int pb, int type_a,
                                                     int type_b, long nblk, float* __restrict__ partial,
                                                     float* __restrict__ bias_partial, int out_elems, int bias_elems) {
  constexpr int TA = 9, TB = 9, NT = TA + TB;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int wa = wv & 3, wb = wv >> 2;
  const int split = blockIdx.x, nsplit = gridDim.x;
  const long b0 = nblk * split / nsplit, b1 = nblk * (split + 1) / nsplit;
  constexpr int nchunk = NT * 2;
  const int my_chunks = (nchunk - wv + 7) >> 3;
  const int src_lo = ((lane >> 2) & 3) * 32 + 4 * (lane >> 4) + (lane & 3);
  const char* const base_a = (type_a ? rg.base[1] : rg.base[0]) + (long)pa * 2048;
  const char* const base_b = (type_b ? rg.base[1] : rg.base[0]) + (long)pb * 2048;
  const long stride_a = type_a ? rg.stride[1] : rg.stride[0], stride_b = type_b ? rg.stride[1] : rg.stride[0];
  auto issue = [&](long blk, int slot) {
    for (int c = wv; c < nchunk; c += 8) {
      const int tix = c >> 1;
      const char* tb_ = tix < TA ? base_a + blk * stride_a + (long)tix * 2048 : base_b + blk * stride_b + (long)(tix - TA) * 2048;
      const char* g = tb_ + (src_lo + (c & 1) * 16) * 16;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                       (__attribute__((address_space(3))) void*)(lds + slot * WG_BUF_BYTES + c * 1024), 16, 0, WG_DMA_AUX);
    }
  };
  const int lane_off = (((lane >> 5) * 2) * 16 + (((lane >> 4) & 1) * 2 + (lane & 1)) * 4 + ((lane & 15) >> 2)) * 16 + 8 * ((lane & 3) >> 1);
  facc acc[10], ex[2];
#pragma unroll
  for (int q = 0; q < 10; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) ex[q][r] = 0.f;
  float bsum[2] = {0.f, 0.f}, xsum = 0.f;
  const bool has_x = wb == 1 || wa == 0;          // waves that hold products of the ninth A tile
  const int xk = wb == 1 ? wa : 4;                 // the regular B slot k whose tile also meets the ninth A tile
  for (int d = 0; d < WG_DEPTH - 1; ++d)
    if (b0 + d < b1) issue(b0 + d, d);
  int slot = 0;
  for (long blk = b0; blk < b1; ++blk) {
    long younger = b1 - 1 - blk;
    if (younger > WG_DEPTH - 2) younger = WG_DEPTH - 2;
    wait_vmcnt((int)younger * my_chunks);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (blk + WG_DEPTH - 1 < b1) issue(blk + WG_DEPTH - 1, (slot + WG_DEPTH - 1) % WG_DEPTH);
    lds_char* buf = (lds_char*)(lds + slot * WG_BUF_BYTES) + lane_off;
    auto load_b = [&](int tb, b8& f0, b8& f1) {
      f0 = tr_frag(buf + (TA + tb) * 2048, 0);
      f1 = tr_frag(buf + (TA + tb) * 2048, 1);
    };
    b8 a[2][2], sa[2], c0, c1, n0, n1;
    load_b(wb, c0, c1);
    n0 = c0; n1 = c1;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      a[i][0] = tr_frag(buf + (wa + 4 * i) * 2048, 0);
      a[i][1] = tr_frag(buf + (wa + 4 * i) * 2048, 1);
    }
    if (has_x) { sa[0] = tr_frag(buf + 8 * 2048, 0); sa[1] = tr_frag(buf + 8 * 2048, 1); }
    if (type_a == 0) {
#pragma unroll
      for (int i = 0; i < 2; ++i) { a[i][0] = f16_to_bf16(a[i][0]); a[i][1] = f16_to_bf16(a[i][1]); }
      if (has_x) { sa[0] = f16_to_bf16(sa[0]); sa[1] = f16_to_bf16(sa[1]); }
    }
    if (bias_partial) {   // wave (wa, wb): row sums of A tile wa + 4 wb
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (wb == i) {
#pragma unroll
          for (int j = 0; j < 8; ++j) bsum[i] += (float)a[i][0][j] + (float)a[i][1][j];
        }
    }
    if (bias_partial && wv == 4) {   // wave (0, 1): row sums of the ninth A tile
#pragma unroll
      for (int j = 0; j < 8; ++j) xsum += (float)sa[0][j] + (float)sa[1][j];
    }
    // regular slots k = 0..4 (B tile wb + 2 k), then -- waves with wb = 1 -- the extra B tile 2 wa; each tile is requested before
    // the MFMAs of the previous one
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const int tb_next = (k + 1 < 5) ? wb + 2 * (k + 1) : 2 * wa;
      const bool next_ok = (k + 1 < 5) ? (tb_next < TB) : (k + 1 == 5 && wb == 1);
      if (next_ok) load_b(tb_next, n0, n1);
      asm volatile("" : "+v"(n0), "+v"(n1));
      const bool cur_ok = (k < 5) ? (wb + 2 * k < TB) : (wb == 1);
      if (cur_ok) {
        if (type_b == 0) { c0 = f16_to_bf16(c0); c1 = f16_to_bf16(c1); }
        if (k < 5) {
          acc[k] = MF<b8>::mma(a[0][0], c0, acc[k]);
          acc[k] = MF<b8>::mma(a[0][1], c1, acc[k]);
          acc[5 + k] = MF<b8>::mma(a[1][0], c0, acc[5 + k]);
          acc[5 + k] = MF<b8>::mma(a[1][1], c1, acc[5 + k]);
          if (has_x && k == xk) {
            ex[0] = MF<b8>::mma(sa[0], c0, ex[0]);
            ex[0] = MF<b8>::mma(sa[1], c1, ex[0]);
          }
        } else {
          ex[1] = MF<b8>::mma(sa[0], c0, ex[1]);
          ex[1] = MF<b8>::mma(sa[1], c1, ex[1]);
        }
      }
      c0 = n0; c1 = n1;
    }
    slot = (slot + 1) % WG_DEPTH;
  }
  float* dst = partial + (long)split * out_elems;
  auto store_tile = [&](int ta, int tb, const facc& v16) {
    f4* d4 = reinterpret_cast<f4*>(dst + ((long)(ta * TB + tb) * 64 + lane) * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f4 v;
      v[0] = v16[4 * q]; v[1] = v16[4 * q + 1]; v[2] = v16[4 * q + 2]; v[3] = v16[4 * q + 3];
      d4[q] = v;
    }
  };
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    if (wb + 2 * k < TB) {
      store_tile(wa, wb + 2 * k, acc[k]);
      store_tile(wa + 4, wb + 2 * k, acc[5 + k]);
    }
  }
  if (has_x) store_tile(8, wb + 2 * xk, ex[0]);
  if (wb == 1) store_tile(8, 2 * wa, ex[1]);
  if (bias_partial) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (wb == i) {
        const float sx = xhalf_sum(bsum[i]);
        if (lane < 32) bias_partial[(long)split * bias_elems + (wa + 4 * i) * 32 + lane] = sx;
      }
    }
    if (wv == 4) {
      const float sx = xhalf_sum(xsum);
      if (lane < 32) bias_partial[(long)split * bias_elems + 8 * 32 + lane] = sx;
    }
  }
}

// every product of one backward pass in ONE launch: blockIdx.y = pair, blockIdx.x = K-split.  Workgroups are dispatched
// x-fastest, so the tail of one pair's splits overlaps the head of the next pair's instead of draining the chip 17 times.
#define WG_MAX_PAIRS 24
struct WgPairs { int v[WG_MAX_PAIRS][8]; };   // pa, ta, pb, tb, out_off, bias_off (-1 = no bias), type_a, type_b
__global__ __launch_bounds__(512) void weight_grad_all_kernel(WgRegions rg, WgPairs pp, long nblk,
                                                              float* __restrict__ partial, float* __restrict__ bias_partial,
                                                              int out_elems, int bias_elems) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int* d = pp.v[blockIdx.y];
  float* bp = d[5] >= 0 ? bias_partial + d[5] : nullptr;
  // wide x wide: 2 x 4 (or 4 x 2) tiles per wave, the f16 operand on the side with fewer tiles per wave (it is converted to bf16
  // after the read); narrow pairs: 8 x 1 or 1 x 8 waves
#define WG_ARGS lds, rg, d[0], d[1], d[2], d[3], d[6], d[7], nblk, partial + d[4], bp, out_elems, bias_elems
  // the products of the full nets: <NI, NK, TA, TB, WA, type_a, type_b, bias>, the wave split of the run-time bodies below
#define WG_SHIPPED(...) weight_grad_shipped<__VA_ARGS__>(lds, rg, d[0], d[2], nblk, partial + d[4], bp, out_elems, bias_elems)
  const bool gxf_bias = d[6] == 1 && d[7] == 0 && bp, fxg_plain = d[6] == 0 && d[7] == 1 && !bp;
  if (gxf_bias && d[1] == 8 && d[3] == 8) {
    WG_SHIPPED(4, 2, 8, 8, 2, 1, 0, true);
  } else if (fxg_plain && d[1] == 8 && d[3] == 8) {
    WG_SHIPPED(2, 4, 8, 8, 4, 0, 1, false);
  } else if (gxf_bias && d[1] == 7 && d[3] == 8) {
    WG_SHIPPED(4, 2, 7, 8, 2, 1, 0, true);
  } else if (fxg_plain && d[1] == 7 && d[3] == 8) {
    WG_SHIPPED(2, 4, 7, 8, 4, 0, 1, false);
  } else if (gxf_bias && d[1] == 8 && d[3] == 9) {
    WG_SHIPPED(2, 5, 8, 9, 4, 1, 0, true);
  } else if (gxf_bias && d[1] == 8 && d[3] == 2) {
    WG_SHIPPED(1, 2, 8, 2, 8, 1, 0, true);
  } else if (fxg_plain && d[1] == 8 && d[3] == 2) {
    WG_SHIPPED(1, 2, 8, 2, 8, 0, 1, false);
  } else if (gxf_bias && d[1] == 1 && d[3] == 8) {
    WG_SHIPPED(1, 1, 1, 8, 1, 1, 0, true);
  } else if (d[1] > 1 && d[3] > 2 && d[3] <= 8) {
    if (d[7] == 0) weight_grad_body<4, 2>(WG_ARGS, 2);
    else weight_grad_body<2, 4>(WG_ARGS, 4);
  } else if (gxf_bias && d[1] == 9 && d[3] == 9) {
    weight_grad_shipped_9x9<1, 0, true>(lds, rg, d[0], d[2], nblk, partial + d[4], bp, out_elems, bias_elems);
  } else if (d[1] == 9 && d[3] == 9) {
    weight_grad_body_9x9(lds, rg, d[0], d[2], d[6], d[7], nblk, partial + d[4], bp, out_elems, bias_elems);
  } else if (d[1] > 1 && d[3] > 8) {
    weight_grad_body<2, 5>(WG_ARGS, 4);
  } else if (d[1] > 1) {
    weight_grad_body<1, 2>(WG_ARGS, 8);      // tb <= 2: one A tile x both B tiles per wave
  } else {
    weight_grad_body<1, 2>(WG_ARGS, 1);      // a single A tile: 1 x 8 waves, one (or two) B tiles each
  }
#undef WG_SHIPPED
#undef WG_ARGS
}

extern "C" int avc_weight_grad_all(const void* fpanels, int ftiles, const void* gpanels, int gtiles, int npairs, const int* pairs,
                                   long nblk, float* partial, float* bias_partial, int nsplit, int out_stride, int bias_stride,
                                   void* stream) {
  if (nblk <= 0 || npairs <= 0) return 0;
  if (!fpanels || !gpanels) { avc_set_error("avc_weight_grad_all: fpanels / gpanels == NULL"); return 1; }
  if (npairs > WG_MAX_PAIRS) { avc_set_error("avc_weight_grad_all: too many pairs"); return 1; }
  WgPairs pp;
  for (int i = 0; i < npairs; ++i) {
    for (int k = 0; k < 8; ++k) pp.v[i][k] = pairs[i * 8 + k];
    const bool merged = pp.v[i][1] == 9 && pp.v[i][3] == 9;
    if (!merged && (pp.v[i][1] < 1 || pp.v[i][1] > 8 || pp.v[i][3] < 1 || pp.v[i][3] > WG_TB_MAX)) {
      avc_set_error("avc_weight_grad_all: 1 <= ta <= 8, 1 <= tb <= 9 (or the 9 x 9 product)");
      return 1;
    }
    // a table that would read outside a block's region or write outside a split's row is refused here, before anything is launched
    const int* d = pp.v[i];
    if ((d[6] != 0 && d[6] != 1) || (d[7] != 0 && d[7] != 1)) {
      avc_set_error("avc_weight_grad_all: operand types are 0 (F region) or 1 (G region)");
      return 1;
    }
    const long tiles_a = d[6] ? gtiles : ftiles, tiles_b = d[7] ? gtiles : ftiles;
    if (d[0] < 0 || (long)d[0] + d[1] > tiles_a || d[2] < 0 || (long)d[2] + d[3] > tiles_b) {
      avc_set_error("avc_weight_grad_all: a pair's tiles lie outside their region");
      return 1;
    }
    if (d[4] < 0 || (long)d[4] + (long)d[1] * d[3] * 1024 > out_stride) {
      avc_set_error("avc_weight_grad_all: a pair's products lie outside out_stride");
      return 1;
    }
    if (d[5] >= 0 && (long)d[5] + 32 * d[1] > bias_stride) {
      avc_set_error("avc_weight_grad_all: a pair's bias sums lie outside bias_stride");
      return 1;
    }
  }
  if (nsplit < 1) nsplit = 1;
  const int lds_bytes = WG_DEPTH * WG_BUF_BYTES;
  static unsigned long long attr_seen = 0;
  if (avc_first_use_on_device(attr_seen)) {
    (void)hipFuncSetAttribute((const void*)weight_grad_all_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  }
  WgRegions rg;
  rg.base[0] = (const char*)fpanels; rg.stride[0] = (long)ftiles * 2048;
  rg.base[1] = (const char*)gpanels; rg.stride[1] = (long)gtiles * 2048;
  hipLaunchKernelGGL(weight_grad_all_kernel, dim3(nsplit, npairs), dim3(512), lds_bytes, (hipStream_t)stream, rg, pp, nblk, partial,
                     bias_partial, out_stride, bias_stride);
  return avc_check_launch("avc_weight_grad_all");
}

// ---- split sums and the way back to the dense parameter vector (what the caller of avc_weight_grad_all does next) ----
// acc[j] (+)= sum_s partial[s][j] for the gout_size weight-product floats followed by the gbias_size bias floats, splits added in
// order (deterministic), 4 floats per thread: ns x 1.7 MB of streaming reads, one launch instead of two torch reductions + two adds
// per slab.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ bpartial, int ns,
                                                           long stride, long bstride, int gout4, int gbias4, float* __restrict__ acc,
                                                           int accumulate) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= gout4 + gbias4) return;
  const f4* src = j < gout4 ? reinterpret_cast<const f4*>(partial) + j : reinterpret_cast<const f4*>(bpartial) + (j - gout4);
  const long st4 = (j < gout4 ? stride : bstride) >> 2;
  f4 a = {0.f, 0.f, 0.f, 0.f};
  int s = 0;
  for (; s + 8 <= ns; s += 8) {
    f4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(src + (long)(s + u) * st4);
#pragma unroll
    for (int u = 0; u < 8; ++u) a += v[u];
  }
  for (; s < ns; ++s) a += __builtin_nontemporal_load(src + (long)s * st4);
  f4* out = reinterpret_cast<f4*>(acc) + j;
  if (accumulate) a += *out;
  *out = a;
}
// grad[t] = sum_{k in [off[t], off[t+1])} acc[src[k]] * scale[k]: the tile layout of the products -> the dense parameter vector (a
// parameter that several tile entries map to -- the hi + lo slots of the merged last-layer product -- adds them in list order)
__global__ __launch_bounds__(256) void wgrad_unpack_kernel(const float* __restrict__ acc, const int* __restrict__ off, const int* __restrict__ src,
                                                           const float* __restrict__ scale, int nparam, float* __restrict__ grad) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nparam) return;
  float g = 0.f;
  for (int k = off[t]; k < off[t + 1]; ++k) g += acc[src[k]] * scale[k];
  grad[t] = g;
}
extern "C" int avc_weight_grad_reduce(const float* partial, const float* bias_partial, int nsplit, int out_stride, int bias_stride,
                                      int gout_size, int gbias_size, float* acc, int accumulate, void* stream) {
  if ((gout_size & 3) || (gbias_size & 3) || (out_stride & 3) || (bias_stride & 3)) {
    avc_set_error("avc_weight_grad_reduce: sizes and strides must be multiples of 4 floats");
    return 1;
  }
  if (nsplit < 1 || !partial || !acc || (gbias_size && !bias_partial)) { avc_set_error("avc_weight_grad_reduce: bad arguments"); return 1; }
  const int n4 = (gout_size + gbias_size) / 4;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((n4 + 255) / 256), dim3(256), 0, (hipStream_t)stream, partial, bias_partial, nsplit,
                     (long)out_stride, (long)bias_stride, gout_size / 4, gbias_size / 4, acc, accumulate);
  return avc_check_launch("avc_weight_grad_reduce");
}
extern "C" int avc_weight_grad_unpack(const float* acc, const int* off, const int* src, const float* scale, int nparam, float* grad,
                                      void* stream) {
  if (nparam <= 0) return 0;
  if (!acc || !off || !src || !scale || !grad) { avc_set_error("avc_weight_grad_unpack: NULL buffer"); return 1; }
  hipLaunchKernelGGL(wgrad_unpack_kernel, dim3((nparam + 255) / 256), dim3(256), 0, (hipStream_t)stream, acc, off, src, scale, nparam, grad);
  return avc_check_launch("avc_weight_grad_unpack");
}
