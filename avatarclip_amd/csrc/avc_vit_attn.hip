// Multi-head self-attention of CLIP's ResidualAttentionBlock (OpenAI clip/model.py; perceptor.encode_image, main.py:512,524) on
// the matrix core: 50 tokens (padded to 64), head dim 64, one 4-wavefront workgroup per (image, head), bf16 operands with fp32
// accumulation (the class the reference's fp16 CLIP runs in), softmax statistics in fp32.
//
// Everything is computed TRANSPOSED, S^T = K Q^T, so that a wavefront's accumulator tile (v_mfma_f32_32x32x16_bf16 C layout: lane
// = column, 16 rows in registers, the other 16 rows in lane ^ 32) holds, for ITS query (column), all keys of the tile in registers:
// the softmax reductions over the keys are register loops plus one lane-32 exchange, no LDS.  As in the MLP engine
// (avc_common.h), the accumulator tile -- after the softmax and a cvt to bf16 -- IS the B operand of the next product
// (O^T = V^T P^T, dQ^T = K^T dS^T): its k-slot (s, h, j) carries key kappa(s,h,j) = 32 (s >> 1) + 16 (s & 1) + 8 (j >> 2) + 4 h + (j & 3),
// and the A operand (V^T, K^T from LDS, stored [d][key]) is read with the same permutation (two 8-byte reads per fragment).
// The products that contract over the QUERIES (dV = P^T dO, dK = dS^T Q) need P^T / dS^T as A operands, lane = key row: those two
// tiles go through LDS once ([key][query], bf16).
#include "avc_vit.h"
#include "../../include/avc.h"

#define ATM_TP 64     // padded tokens (ATM_T, ATM_D: avc_vit.h)
#define ATM_LD 72     // row stride of the bf16 LDS matrices (144 B: 16-byte aligned rows, 36-bank skew)

typedef __bf16 bf;
typedef short s4v __attribute__((ext_vector_type(4)));

struct AtmMats {        // bf16 matrices of one (image, head) in LDS
  bf Q[ATM_TP][ATM_LD];     // [token][d], pre-scaled by 1/sqrt(d)
  bf K[ATM_TP][ATM_LD];
  bf VT[ATM_D][ATM_LD];     // [d][token]
};
struct AtmMatsBwd {
  bf Q[ATM_TP][ATM_LD], K[ATM_TP][ATM_LD], V[ATM_TP][ATM_LD], dO[ATM_TP][ATM_LD];   // [token][d]
  bf KT[ATM_D][ATM_LD], QT[ATM_D][ATM_LD], dOT[ATM_D][ATM_LD];                      // [d][token]
  bf PT[ATM_TP][ATM_LD], dST[ATM_TP][ATM_LD];                                       // [key][query]
};

// natural fragment: row (or column) `r`, k-slots 16 s + 8 h + 0..7 of a [.][k] row-major matrix
__device__ __forceinline__ b8 frag_nat(const bf (*m)[ATM_LD], int r, int s, int h) {
  return *reinterpret_cast<const b8*>(&m[r][16 * s + 8 * h]);
}
// permuted fragment: k-slot j of k-step s carries column kappa(s,h,j) (see the header): 4 + 4 contiguous entries
__device__ __forceinline__ b8 frag_perm(const bf (*m)[ATM_LD], int r, int s, int h) {
  const int k0 = 32 * (s >> 1) + 16 * (s & 1) + 4 * h;
  struct { s4v lo, hi; } v;
  v.lo = *reinterpret_cast<const s4v*>(&m[r][k0]);
  v.hi = *reinterpret_cast<const s4v*>(&m[r][k0 + 8]);
  return __builtin_bit_cast(b8, v);
}

// S^T tiles of query tile `ti` (columns) against both key tiles, then the softmax over the keys: on return p[tj][r] = P[i][j] for
// query i = 32 ti + (lane & 31), key j = 32 tj + acc_row(r, h)
__device__ __forceinline__ void scores_softmax(const bf (*Q)[ATM_LD], const bf (*K)[ATM_LD], int ti, int lane, facc (&p)[2]) {
  const int n = lane & 31, h = lane >> 5;
#pragma unroll
  for (int tj = 0; tj < 2; ++tj) {
#pragma unroll
    for (int r = 0; r < 16; ++r) p[tj][r] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) p[tj] = MF<b8>::mma(frag_nat(K, 32 * tj + n, s, h), frag_nat(Q, 32 * ti + n, s, h), p[tj]);
  }
  float mx = -1e30f;
#pragma unroll
  for (int tj = 0; tj < 2; ++tj)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (32 * tj + acc_row(r, h) >= ATM_T) p[tj][r] = -1e30f;   // padded keys
      mx = fmaxf(mx, p[tj][r]);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  float sum = 0.f;
#pragma unroll
  for (int tj = 0; tj < 2; ++tj)
#pragma unroll
    for (int r = 0; r < 16; ++r) { p[tj][r] = __expf(p[tj][r] - mx); sum += p[tj][r]; }
  sum += __shfl_xor(sum, 32);
  const float inv = 1.f / sum;
#pragma unroll
  for (int tj = 0; tj < 2; ++tj)
#pragma unroll
    for (int r = 0; r < 16; ++r) p[tj][r] *= inv;
}
// accumulator tiles [key tile][16] (x scale) -> the four B-operand k-steps over the keys
__device__ __forceinline__ void acc_to_b(const facc (&a)[2], float scale, b8 (&f)[4]) {
#pragma unroll
  for (int tj = 0; tj < 2; ++tj)
#pragma unroll
    for (int j = 0; j < 8; ++j) { f[2 * tj][j] = (bf)(a[tj][j] * scale); f[2 * tj + 1][j] = (bf)(a[tj][8 + j] * scale); }
}

// PACKED: `out` is the packed bf16 operand of the out-projection ([row tile][k-step][lane (row, half)][8 columns], rows = b * 50 +
// token) instead of fp32 [B,T,W] -- the batched scoring pipeline (avc_vit_attention_fwd_packed)
template <bool PACKED>
__global__ __launch_bounds__(256) void vit_attn_fwd_mfma_kernel(const float* __restrict__ qkv, float* __restrict__ out, int Wd, int heads,
                                                                float scale) {
  __shared__ __attribute__((aligned(16))) AtmMats m;
  const int b = blockIdx.x / heads, hd = blockIdx.x % heads;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float* base = qkv + (long)b * ATM_T * 3 * Wd + hd * ATM_D;
  for (int e = threadIdx.x; e < ATM_TP * (ATM_D / 4); e += 256) {
    const int r = e / (ATM_D / 4), c = 4 * (e % (ATM_D / 4));
    f4 q = {0.f, 0.f, 0.f, 0.f}, k = q, v = q;
    if (r < ATM_T) {
      const float* rp = base + (long)r * 3 * Wd + c;
      q = *reinterpret_cast<const f4*>(rp) * scale; k = *reinterpret_cast<const f4*>(rp + Wd); v = *reinterpret_cast<const f4*>(rp + 2 * Wd);
    }
    put4(&m.Q[r][c], q); put4(&m.K[r][c], k);
#pragma unroll
    for (int u = 0; u < 4; ++u) m.VT[c + u][r] = (bf)v[u];
  }
  __syncthreads();
  if (wv >= 2) return;              // one wavefront per 32-query tile
  const int ti = wv, n = lane & 31, h = lane >> 5;
  facc p[2];
  scores_softmax(m.Q, m.K, ti, lane, p);
  b8 pf[4];
  acc_to_b(p, 1.f, pf);
  const int i = 32 * ti + n;
#pragma unroll
  for (int td = 0; td < 2; ++td) {   // O^T tile: rows d, column = this lane's query
    facc o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) o = MF<b8>::mma(frag_perm(m.VT, 32 * td + n, s, h), pf[s], o);
    if (PACKED) {
      // 2-byte stores straight from the accumulator registers (a version that assembled whole 16-byte chunks through a lane-pair
      // exchange indexed the accumulator by the lane's half -- a dynamic register index -- and took 9.1 instead of 5.3 us)
      if (i < ATM_T) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          put_packed_elem(reinterpret_cast<bf*>(out), Wd >> 4, (long)b * ATM_T + i, hd * ATM_D + 32 * td + acc_row(r, h), o[r]);
      }
    } else if (i < ATM_T) {
      float* op = out + ((long)b * ATM_T + i) * Wd + hd * ATM_D + 32 * td;
#pragma unroll
      for (int r = 0; r < 16; ++r) op[acc_row(r, h)] = o[r];
    }
  }
}

// PACKED: dqkv leaves as the packed operand of the transposed in-projection (K = 3 W) instead of fp32 rows: the per-iteration training
// pipeline (clip_vit.BlocksFn)
template <bool PACKED>
__global__ __launch_bounds__(256) void vit_attn_bwd_mfma_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                float* __restrict__ dqkv, int Wd, int heads, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  AtmMatsBwd& m = *reinterpret_cast<AtmMatsBwd*>(smem);
  const int b = blockIdx.x / heads, hd = blockIdx.x % heads;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = lane & 31, h = lane >> 5;
  const float* base = qkv + (long)b * ATM_T * 3 * Wd + hd * ATM_D;
  const float* dob = dout + (long)b * ATM_T * Wd + hd * ATM_D;
  for (int e = threadIdx.x; e < ATM_TP * (ATM_D / 4); e += 256) {
    const int r = e / (ATM_D / 4), c = 4 * (e % (ATM_D / 4));
    f4 q = {0.f, 0.f, 0.f, 0.f}, k = q, v = q, d = q;
    if (r < ATM_T) {
      const float* rp = base + (long)r * 3 * Wd + c;
      q = *reinterpret_cast<const f4*>(rp) * scale; k = *reinterpret_cast<const f4*>(rp + Wd); v = *reinterpret_cast<const f4*>(rp + 2 * Wd);
      d = *reinterpret_cast<const f4*>(dob + (long)r * Wd + c);
    }
    put4(&m.Q[r][c], q); put4(&m.K[r][c], k); put4(&m.V[r][c], v); put4(&m.dO[r][c], d);
#pragma unroll
    for (int u = 0; u < 4; ++u) { m.QT[c + u][r] = (bf)q[u]; m.KT[c + u][r] = (bf)k[u]; m.dOT[c + u][r] = (bf)d[u]; }
  }
  __syncthreads();
  if (wv < 2) {
    // ---- per query tile: P^T, dP^T = V dO^T, dS^T = P^T (dP^T - sum_j P dP), dQ^T = K^T dS^T (x scale)
    const int ti = wv;
    facc p[2], dp[2];
    scores_softmax(m.Q, m.K, ti, lane, p);
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) {
#pragma unroll
      for (int r = 0; r < 16; ++r) dp[tj][r] = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) dp[tj] = MF<b8>::mma(frag_nat(m.V, 32 * tj + n, s, h), frag_nat(m.dO, 32 * ti + n, s, h), dp[tj]);
    }
    float dsum = 0.f;
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) dsum += p[tj][r] * dp[tj][r];
    dsum += __shfl_xor(dsum, 32);
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) dp[tj][r] = p[tj][r] * (dp[tj][r] - dsum);      // dS^T (w.r.t. the scaled scores)
    b8 dsf[4];
    acc_to_b(dp, scale, dsf);                       // dQ = scale * dS K
    const int i = 32 * ti + n;
#pragma unroll
    for (int td = 0; td < 2; ++td) {
      facc o;
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s) o = MF<b8>::mma(frag_perm(m.KT, 32 * td + n, s, h), dsf[s], o);
      if (i < ATM_T) {
        if (PACKED) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            put_packed_elem(reinterpret_cast<bf*>(dqkv), (3 * Wd) >> 4, (long)b * ATM_T + i, hd * ATM_D + 32 * td + acc_row(r, h), o[r]);
        } else {
          float* qp = dqkv + ((long)b * ATM_T + i) * 3 * Wd + hd * ATM_D + 32 * td;
#pragma unroll
          for (int r = 0; r < 16; ++r) qp[acc_row(r, h)] = o[r];
        }
      }
    }
    // P^T and dS^T to LDS as [key][query] for the products that contract over the queries
#pragma unroll
    for (int tj = 0; tj < 2; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = 32 * tj + acc_row(r, h);
        m.PT[j][i] = (bf)p[tj][r];
        m.dST[j][i] = (bf)dp[tj][r];
      }
  }
  __syncthreads();
  // ---- dV = P^T dO, dK = dS^T Q_scaled: 4 + 4 tiles [key tile][d tile], two of each per wavefront; contraction over all 64 queries
  const int tj = wv & 1, td = wv >> 1;
  facc dv, dk;
#pragma unroll
  for (int r = 0; r < 16; ++r) { dv[r] = 0.f; dk[r] = 0.f; }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    dv = MF<b8>::mma(frag_nat(m.PT, 32 * tj + n, s, h), frag_nat(m.dOT, 32 * td + n, s, h), dv);
    dk = MF<b8>::mma(frag_nat(m.dST, 32 * tj + n, s, h), frag_nat(m.QT, 32 * td + n, s, h), dk);
  }
  // C layout: lane = column d = 32 td + n, rows = keys 32 tj + acc_row(r, h)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int j = 32 * tj + acc_row(r, h);
    if (j < ATM_T) {
      if (PACKED) {
        const int col = hd * ATM_D + 32 * td + n;
        put_packed_elem(reinterpret_cast<bf*>(dqkv), (3 * Wd) >> 4, (long)b * ATM_T + j, Wd + col, dk[r]);
        put_packed_elem(reinterpret_cast<bf*>(dqkv), (3 * Wd) >> 4, (long)b * ATM_T + j, 2 * Wd + col, dv[r]);
      } else {
        float* kp = dqkv + ((long)b * ATM_T + j) * 3 * Wd + hd * ATM_D + 32 * td + n;
        kp[Wd] = dk[r];
        kp[2 * Wd] = dv[r];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// 1 <= T <= 256 tokens (every T but 50, which stays on the kernels above; 197 = ViT-B/16): the keys no longer fit one 64-key tile,
// so the sequence is walked in 32-key tiles, NT = ceil(T / 32) <= 8 of them.  Same transposed products, same fragments and the same
// arithmetic class as above.  Where each operand is rounded to bf16:
//   q / 8, k, v, dO   when they are read from the fp32 rows (q AFTER the scaling by 1/8, which is exact);
//   P                 AFTER normalisation: a first pass over the key tiles takes the row maximum m and the row sum l of exp(s - m) in
//                     fp32 (running maximum, l rescaled when m grows), a second pass recomputes the scores and rounds p = exp(s - m) / l
//                     -- the T = 50 kernels' rounding point; nothing unnormalised is ever rounded;
//   dS                = P (dP - D) from the fp32 P and dP and the fp32 D = sum_j P dP, rounded once; dQ's copy is rounded after the
//                     (exact) scaling by 1/8.
// Ragged T: K / V / Q / dO rows past T are ZERO-FILLED BY SELECTION when they are staged (the fp32 rows past b * T + T belong to the
// next image or to nobody and are never read), key columns past T are taken out of the maximum, the sum and P by selection (s = -1e30,
// p = 0), query rows past T are never stored.  Every output element is written by exactly one lane, every sum runs in one fixed
// order and nothing depends on the image's place in the batch: no atomics, results are the same bits in every run and every batch.
//   forward   one 4-wavefront workgroup per (image, head, 128 queries): K [key][d] and V^T [d][key] of the whole sequence in LDS
//             (<= 69 KiB: two workgroups per CU), one wavefront per 32-query tile with its q fragments in registers.
//   backward  one 8-wavefront workgroup per (image, head) -- dK and dV contract over ALL queries of the pair, and the entry points
//             carry no workspace for statistics or partial sums.  Phase 1 (LDS: K, V, K^T): wavefront w owns query tile w; pass A takes
//             m, l and D (D = sum_j exp(s - m) dP / l, rescaled with l) in one sweep over the key tiles, pass B recomputes s and dP,
//             forms dS and accumulates dQ^T = K^T dS^T; m, 1/l, D go to LDS.  Phase 2 (LDS re-staged: Q, dO, Q^T, dO^T): wavefront w
//             owns KEY tile w with its k / v fragments in registers and walks the query tiles in order 0 .. NT-1 with the products the
//             other way round (S = Q K^T: lane = key, registers = queries), so that P and dS ARE the B operands of dV^T = dO^T P and
//             dK^T = Q^T dS: no [key][query] round trip through LDS.  141 KiB of LDS: one workgroup per CU.
#define ATL_TMAX 256
#define ATL_LDT 264   // row stride of the [d][token] matrices (528 B: 8-byte aligned fragments, 4-bank skew per row)
#define ATL_NAT (ATL_TMAX * ATM_LD * 2)      // bytes of a [token][d] matrix
#define ATL_TR (ATM_D * ATL_LDT * 2)         // bytes of a [d][token] matrix
#define ATL_BWD_LDS (2 * ATL_NAT + 2 * ATL_TR + 3 * ATL_TMAX * 4)

__device__ __forceinline__ b8 frag_perm_t(const bf (*m)[ATL_LDT], int r, int s, int h) {   // frag_perm over up to 16 k-steps
  const int k0 = 32 * (s >> 1) + 16 * (s & 1) + 4 * h;
  struct { s4v lo, hi; } v;
  v.lo = *reinterpret_cast<const s4v*>(&m[r][k0]);
  v.hi = *reinterpret_cast<const s4v*>(&m[r][k0 + 8]);
  return __builtin_bit_cast(b8, v);
}
// the four k-steps (over d) of row `rp` (64 fp32 values, NULL: a row past T) as a B operand: lane (n, h) holds d = 16 s + 8 h + 0..7
__device__ __forceinline__ void row_frags(const float* rp, int h, float scale, b8 (&f)[4]) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    f4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
    if (rp) { lo = *reinterpret_cast<const f4*>(rp + 16 * s + 8 * h) * scale; hi = *reinterpret_cast<const f4*>(rp + 16 * s + 8 * h + 4) * scale; }
#pragma unroll
    for (int j = 0; j < 4; ++j) { f[s][j] = (bf)lo[j]; f[s][4 + j] = (bf)hi[j]; }
  }
}
// one accumulator tile (x scale) -> its two B-operand k-steps (slot (s, h, j) = row acc_row(8 s + j, h) of the tile)
__device__ __forceinline__ void acc_to_b2(const facc& a, float scale, b8 (&f)[2]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) { f[0][j] = (bf)(a[j] * scale); f[1][j] = (bf)(a[8 + j] * scale); }
}
__device__ __forceinline__ facc tile_product(const bf (*A)[ATM_LD], int row, const b8 (&f)[4], int h) {
  facc c;
#pragma unroll
  for (int r = 0; r < 16; ++r) c[r] = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) c = MF<b8>::mma(frag_nat(A, row, s, h), f[s], c);
  return c;
}

template <bool PACKED>
__global__ __launch_bounds__(256) void vit_attn_fwd_tiled_kernel(const float* __restrict__ qkv, float* __restrict__ out, int T, int Wd,
                                                                 int heads, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int NT = (T + 31) >> 5;
  bf (*K)[ATM_LD] = reinterpret_cast<bf (*)[ATM_LD]>(smem);                                     // [32 NT][72]
  bf (*VT)[ATL_LDT] = reinterpret_cast<bf (*)[ATL_LDT]>(smem + (size_t)NT * 32 * ATM_LD * 2);    // [64][264]
  const int b = blockIdx.x / heads, hd = blockIdx.x % heads;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = lane & 31, h = lane >> 5;
  const float* base = qkv + (long)b * T * 3 * Wd + hd * ATM_D;
  for (int e = threadIdx.x; e < NT * 32 * (ATM_D / 4); e += 256) {
    const int r = e / (ATM_D / 4), c = 4 * (e % (ATM_D / 4));
    f4 k = {0.f, 0.f, 0.f, 0.f}, v = k;
    if (r < T) {
      const float* rp = base + (long)r * 3 * Wd + c;
      k = *reinterpret_cast<const f4*>(rp + Wd); v = *reinterpret_cast<const f4*>(rp + 2 * Wd);
    }
    put4(&K[r][c], k);
#pragma unroll
    for (int u = 0; u < 4; ++u) VT[c + u][r] = (bf)v[u];
  }
  const int ti = 4 * blockIdx.y + wv, i = 32 * ti + n;
  b8 qf[4];
  row_frags(ti < NT && i < T ? base + (long)i * 3 * Wd : nullptr, h, scale, qf);
  __syncthreads();
  if (ti >= NT) return;              // (no barrier below)
  // pass A: row maximum and row sum over the key tiles
  float mx = -1e30f, sum = 0.f;
  for (int tj = 0; tj < NT; ++tj) {
    facc s = tile_product(K, 32 * tj + n, qf, h);
    float tm = -1e30f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = 32 * tj + acc_row(r, h) < T ? s[r] : -1e30f;      // keys past T
      tm = fmaxf(tm, s[r]);
    }
    tm = fmaxf(tm, __shfl_xor(tm, 32));
    const float mn = fmaxf(mx, tm);
    sum *= __expf(mx - mn);
#pragma unroll
    for (int r = 0; r < 16; ++r) sum += __expf(s[r] - mn);
    mx = mn;
  }
  sum += __shfl_xor(sum, 32);
  const float inv = 1.f / sum;
  // pass B: P, rounded after normalisation, and O^T = V^T P^T
  facc o[2];
#pragma unroll
  for (int td = 0; td < 2; ++td)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[td][r] = 0.f;
  for (int tj = 0; tj < NT; ++tj) {
    facc s = tile_product(K, 32 * tj + n, qf, h);
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 32 * tj + acc_row(r, h) < T ? __expf(s[r] - mx) * inv : 0.f;
    b8 pf[2];
    acc_to_b2(s, 1.f, pf);
#pragma unroll
    for (int td = 0; td < 2; ++td)
#pragma unroll
      for (int u = 0; u < 2; ++u) o[td] = MF<b8>::mma(frag_perm_t(VT, 32 * td + n, 2 * tj + u, h), pf[u], o[td]);
  }
  if (i >= T) return;                // query rows past T are never stored
#pragma unroll
  for (int td = 0; td < 2; ++td) {
    if (PACKED) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        put_packed_elem(reinterpret_cast<bf*>(out), Wd >> 4, (long)b * T + i, hd * ATM_D + 32 * td + acc_row(r, h), o[td][r]);
    } else {
      float* op = out + ((long)b * T + i) * Wd + hd * ATM_D + 32 * td;
#pragma unroll
      for (int r = 0; r < 16; ++r) op[acc_row(r, h)] = o[td][r];
    }
  }
}

template <bool PACKED>
__global__ __launch_bounds__(512) void vit_attn_bwd_tiled_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                 float* __restrict__ dqkv, int T, int Wd, int heads, float scale) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int NT = (T + 31) >> 5;
  // phase 1: K, V [token][d], K^T [d][token]; phase 2 (over them): Q, dO [token][d], Q^T, dO^T [d][token]; the statistics behind both
  bf (*M0)[ATM_LD] = reinterpret_cast<bf (*)[ATM_LD]>(smem);
  bf (*M1)[ATM_LD] = reinterpret_cast<bf (*)[ATM_LD]>(smem + ATL_NAT);
  bf (*T0)[ATL_LDT] = reinterpret_cast<bf (*)[ATL_LDT]>(smem + 2 * ATL_NAT);
  bf (*T1)[ATL_LDT] = reinterpret_cast<bf (*)[ATL_LDT]>(smem + 2 * ATL_NAT + ATL_TR);
  float* st_m = reinterpret_cast<float*>(smem + 2 * ATL_NAT + 2 * ATL_TR);
  float* st_inv = st_m + ATL_TMAX;
  float* st_d = st_inv + ATL_TMAX;
  const int b = blockIdx.x / heads, hd = blockIdx.x % heads;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = lane & 31, h = lane >> 5;
  const float* base = qkv + (long)b * T * 3 * Wd + hd * ATM_D;
  const float* dob = dout + (long)b * T * Wd + hd * ATM_D;
  const int own = 32 * wv + n;       // this lane's query (phase 1) / key (phase 2)
  const bool live = wv < NT;         // the wavefront owns a tile
  for (int e = threadIdx.x; e < NT * 32 * (ATM_D / 4); e += 512) {
    const int r = e / (ATM_D / 4), c = 4 * (e % (ATM_D / 4));
    f4 k = {0.f, 0.f, 0.f, 0.f}, v = k;
    if (r < T) {
      const float* rp = base + (long)r * 3 * Wd + c;
      k = *reinterpret_cast<const f4*>(rp + Wd); v = *reinterpret_cast<const f4*>(rp + 2 * Wd);
    }
    put4(&M0[r][c], k); put4(&M1[r][c], v);
#pragma unroll
    for (int u = 0; u < 4; ++u) T0[c + u][r] = (bf)k[u];
  }
  __syncthreads();
  if (live) {
    // ---- phase 1, query tile wv: S^T = K Q^T and dP^T = V dO^T per key tile (lane = query, registers = keys)
    b8 qf[4], dof[4];
    row_frags(own < T ? base + (long)own * 3 * Wd : nullptr, h, scale, qf);
    row_frags(own < T ? dob + (long)own * Wd : nullptr, h, 1.f, dof);
    float mx = -1e30f, sum = 0.f, dacc = 0.f;
    for (int tj = 0; tj < NT; ++tj) {
      facc s = tile_product(M0, 32 * tj + n, qf, h);
      const facc dp = tile_product(M1, 32 * tj + n, dof, h);
      float tm = -1e30f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[r] = 32 * tj + acc_row(r, h) < T ? s[r] : -1e30f;
        tm = fmaxf(tm, s[r]);
      }
      tm = fmaxf(tm, __shfl_xor(tm, 32));
      const float mn = fmaxf(mx, tm), corr = __expf(mx - mn);
      sum *= corr; dacc *= corr;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float e = 32 * tj + acc_row(r, h) < T ? __expf(s[r] - mn) : 0.f;
        sum += e; dacc += e * dp[r];
      }
      mx = mn;
    }
    sum += __shfl_xor(sum, 32);
    dacc += __shfl_xor(dacc, 32);
    const float inv = 1.f / sum, dsum = dacc * inv;      // D = sum_j P dP
    facc dq[2];
#pragma unroll
    for (int td = 0; td < 2; ++td)
#pragma unroll
      for (int r = 0; r < 16; ++r) dq[td][r] = 0.f;
    for (int tj = 0; tj < NT; ++tj) {
      facc s = tile_product(M0, 32 * tj + n, qf, h);
      const facc dp = tile_product(M1, 32 * tj + n, dof, h);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = 32 * tj + acc_row(r, h) < T ? __expf(s[r] - mx) * inv : 0.f;
        s[r] = p * (dp[r] - dsum);                       // dS^T (w.r.t. the scaled scores)
      }
      b8 dsf[2];
      acc_to_b2(s, scale, dsf);                          // dQ = scale * dS K
#pragma unroll
      for (int td = 0; td < 2; ++td)
#pragma unroll
        for (int u = 0; u < 2; ++u) dq[td] = MF<b8>::mma(frag_perm_t(T0, 32 * td + n, 2 * tj + u, h), dsf[u], dq[td]);
    }
    if (h == 0) { st_m[own] = mx; st_inv[own] = inv; st_d[own] = dsum; }
    if (own < T) {
#pragma unroll
      for (int td = 0; td < 2; ++td) {
        if (PACKED) {
#pragma unroll
          for (int r = 0; r < 16; ++r)
            put_packed_elem(reinterpret_cast<bf*>(dqkv), (3 * Wd) >> 4, (long)b * T + own, hd * ATM_D + 32 * td + acc_row(r, h), dq[td][r]);
        } else {
          float* qp = dqkv + ((long)b * T + own) * 3 * Wd + hd * ATM_D + 32 * td;
#pragma unroll
          for (int r = 0; r < 16; ++r) qp[acc_row(r, h)] = dq[td][r];
        }
      }
    }
  }
  __syncthreads();                   // every wavefront is done with K, V, K^T
  for (int e = threadIdx.x; e < NT * 32 * (ATM_D / 4); e += 512) {
    const int r = e / (ATM_D / 4), c = 4 * (e % (ATM_D / 4));
    f4 q = {0.f, 0.f, 0.f, 0.f}, d = q;
    if (r < T) {
      q = *reinterpret_cast<const f4*>(base + (long)r * 3 * Wd + c) * scale;
      d = *reinterpret_cast<const f4*>(dob + (long)r * Wd + c);
    }
    put4(&M0[r][c], q); put4(&M1[r][c], d);
#pragma unroll
    for (int u = 0; u < 4; ++u) { T0[c + u][r] = (bf)q[u]; T1[c + u][r] = (bf)d[u]; }
  }
  __syncthreads();
  if (!live) return;                 // (no barrier below)
  // ---- phase 2, key tile wv: S = Q K^T and dP = dO V^T per query tile (lane = key, registers = queries), query tiles in order
  b8 kf[4], vf[4];
  row_frags(own < T ? base + (long)own * 3 * Wd + Wd : nullptr, h, 1.f, kf);
  row_frags(own < T ? base + (long)own * 3 * Wd + 2 * Wd : nullptr, h, 1.f, vf);
  facc dk[2], dv[2];
#pragma unroll
  for (int td = 0; td < 2; ++td)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk[td][r] = 0.f; dv[td][r] = 0.f; }
  for (int ti = 0; ti < NT; ++ti) {
    facc p = tile_product(M0, 32 * ti + n, kf, h);
    facc ds = tile_product(M1, 32 * ti + n, vf, h);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qi = 32 * ti + acc_row(r, h);
      p[r] = (qi < T && own < T) ? __expf(p[r] - st_m[qi]) * st_inv[qi] : 0.f;     // rows and columns past T by selection
      ds[r] = p[r] * (ds[r] - st_d[qi]);
    }
    b8 pf[2], dsf[2];
    acc_to_b2(p, 1.f, pf);
    acc_to_b2(ds, 1.f, dsf);
#pragma unroll
    for (int td = 0; td < 2; ++td)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        dv[td] = MF<b8>::mma(frag_perm_t(T1, 32 * td + n, 2 * ti + u, h), pf[u], dv[td]);      // dV^T = dO^T P
        dk[td] = MF<b8>::mma(frag_perm_t(T0, 32 * td + n, 2 * ti + u, h), dsf[u], dk[td]);     // dK^T = Q_scaled^T dS
      }
  }
  if (own >= T) return;
#pragma unroll
  for (int td = 0; td < 2; ++td) {
    if (PACKED) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int col = hd * ATM_D + 32 * td + acc_row(r, h);
        put_packed_elem(reinterpret_cast<bf*>(dqkv), (3 * Wd) >> 4, (long)b * T + own, Wd + col, dk[td][r]);
        put_packed_elem(reinterpret_cast<bf*>(dqkv), (3 * Wd) >> 4, (long)b * T + own, 2 * Wd + col, dv[td][r]);
      }
    } else {
      float* kp = dqkv + ((long)b * T + own) * 3 * Wd + hd * ATM_D + 32 * td;
#pragma unroll
      for (int r = 0; r < 16; ++r) { kp[Wd + acc_row(r, h)] = dk[td][r]; kp[2 * Wd + acc_row(r, h)] = dv[td][r]; }
    }
  }
}

template <bool PACKED>
static int attn_fwd_tiled(const float* qkv, void* out, int B, int T, int width, int heads, void* stream, const char* what) {
  const int NT = (T + 31) >> 5;
  const int lds = NT * 32 * ATM_LD * 2 + ATL_TR;
  static unsigned long long attr_seen = 0;
  if (avc_first_use_on_device(attr_seen))
    (void)hipFuncSetAttribute((const void*)vit_attn_fwd_tiled_kernel<PACKED>, hipFuncAttributeMaxDynamicSharedMemorySize, ATL_NAT + ATL_TR);
  hipLaunchKernelGGL(vit_attn_fwd_tiled_kernel<PACKED>, dim3(B * heads, (NT + 3) / 4), dim3(256), lds, (hipStream_t)stream, qkv, (float*)out, T,
                     width, heads, 0.125f);
  return avc_check_launch(what);
}
template <bool PACKED>
static int attn_bwd_tiled(const float* qkv, const float* dout, void* dqkv, int B, int T, int width, int heads, void* stream, const char* what) {
  static unsigned long long attr_seen = 0;
  if (avc_first_use_on_device(attr_seen))
    (void)hipFuncSetAttribute((const void*)vit_attn_bwd_tiled_kernel<PACKED>, hipFuncAttributeMaxDynamicSharedMemorySize, ATL_BWD_LDS);
  hipLaunchKernelGGL(vit_attn_bwd_tiled_kernel<PACKED>, dim3(B * heads), dim3(512), ATL_BWD_LDS, (hipStream_t)stream, qkv, dout, (float*)dqkv, T,
                     width, heads, 0.125f);
  return avc_check_launch(what);
}
int avc_attn_fwd_tiled(const float* qkv, float* out, int B, int T, int width, int heads, void* stream) {
  return attn_fwd_tiled<false>(qkv, out, B, T, width, heads, stream, "avc_vit_attention_fwd");
}
int avc_attn_fwd_tiled_packed(const float* qkv, void* out_packed, int B, int T, int width, int heads, void* stream) {
  return attn_fwd_tiled<true>(qkv, out_packed, B, T, width, heads, stream, "avc_vit_attention_fwd_packed");
}
int avc_attn_bwd_tiled(const float* qkv, const float* dout, float* dqkv, int B, int T, int width, int heads, void* stream) {
  return attn_bwd_tiled<false>(qkv, dout, dqkv, B, T, width, heads, stream, "avc_vit_attention_bwd");
}
int avc_attn_bwd_tiled_packed(const float* qkv, const float* dout, void* dqkv_packed, int B, int T, int width, int heads, void* stream) {
  return attn_bwd_tiled<true>(qkv, dout, dqkv_packed, B, T, width, heads, stream, "avc_vit_attention_bwd_packed");
}

int avc_attn_fwd_mfma(const float* qkv, float* out, int B, int width, int heads, void* stream) {
  hipLaunchKernelGGL(vit_attn_fwd_mfma_kernel<false>, dim3(B * heads), dim3(256), 0, (hipStream_t)stream, qkv, out, width, heads, 0.125f);
  return avc_check_launch("avc_vit_attention_fwd");
}
int avc_attn_fwd_mfma_packed(const float* qkv, void* out_packed, int B, int width, int heads, void* stream) {
  hipLaunchKernelGGL(vit_attn_fwd_mfma_kernel<true>, dim3(B * heads), dim3(256), 0, (hipStream_t)stream, qkv, (float*)out_packed, width, heads,
                     0.125f);
  return avc_check_launch("avc_vit_attention_fwd_packed");
}
int avc_attn_bwd_mfma(const float* qkv, const float* dout, float* dqkv, int B, int width, int heads, void* stream) {
  const int lds = (int)sizeof(AtmMatsBwd);
  static unsigned long long attr_seen = 0;
  if (avc_first_use_on_device(attr_seen))
    (void)hipFuncSetAttribute((const void*)vit_attn_bwd_mfma_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL(vit_attn_bwd_mfma_kernel<false>, dim3(B * heads), dim3(256), lds, (hipStream_t)stream, qkv, dout, dqkv, width, heads, 0.125f);
  return avc_check_launch("avc_vit_attention_bwd");
}
int avc_attn_bwd_mfma_packed(const float* qkv, const float* dout, void* dqkv_packed, int B, int width, int heads, void* stream) {
  const int lds = (int)sizeof(AtmMatsBwd);
  static unsigned long long attr_seen = 0;
  if (avc_first_use_on_device(attr_seen))
    (void)hipFuncSetAttribute((const void*)vit_attn_bwd_mfma_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  hipLaunchKernelGGL(vit_attn_bwd_mfma_kernel<true>, dim3(B * heads), dim3(256), lds, (hipStream_t)stream, qkv, dout, (float*)dqkv_packed, width,
                     heads, 0.125f);
  return avc_check_launch("avc_vit_attention_bwd_packed");
}
