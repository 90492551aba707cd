// CLIP ViT-B/32 image-encoder kernels (perceptor.encode_image, main.py:512; OpenAI clip/model.py VisionTransformer) and the entry
// points of the whole tower (the shared device helpers and the other two sources' launchers: avc_vit.h).
//   avc_vit_linear(_packed, _bwd_gelu)   Y[M,N] = act(X[M,K] W[N,K]^T + b) (+ residual) -- bf16 MFMA 32x32x16, fp32 accumulate; the same
//                    kernels compute dX = dY W with the pre-packed W^T (weights are frozen: no dW).  Up to 128 rows the GEMM is weight-
//                    streaming / latency bound: W is pre-packed in B-operand fragment order and X packed into A-operand fragments (one
//                    coalesced 16-B load per lane per k-step for both), the K range is dealt to the 8 wavefronts of a workgroup and reduced
//                    through LDS, one workgroup per (32 output columns, 32 rows).  More rows: the LDS-staged GEMM of avc_vit_gemm.hip.
//   avc_vit_pack, avc_vit_ln_pack, avc_vit_ln_bwd   the packed pipeline's hand-offs: fp32 rows, LayerNorm and its backward straight into
//                    the packed operand of the next linear.
//   avc_vit_attention_fwd / _bwd (_packed)   the image tower's attention: one route rule, the matrix-core kernels of avc_vit_attn.hip
//                    (50 tokens, or 1 .. 256 walked in 32-key tiles).
//   avc_text_attention_fwd   the text tower's causal attention (<= 128 tokens), fp32 with an online softmax, forward only.
#include "avc_vit.h"
#include "../../include/avc.h"

#define VIT_MAX_MT 4   // up to 128 rows (tokens): the latency kernel (one row tile per workgroup); more rows: avc_vit_gemm.hip, groups of 4
#define VIT_WAVES 8    // wavefronts per workgroup = K-split factor

// X[M,K] fp32 -> the packed bf16 operand (avc_vit.h).
// With `pre` (the pre-activation of a QuickGELU layer, same shape as X) the rows are multiplied by gelu'(pre) on the way: the
// backward of the activation is folded into the packing pass of the GEMM that follows it (dX = (dY * gelu'(pre)) W).
__global__ __launch_bounds__(64) void vit_pack_x_kernel(const float* __restrict__ X, const float* __restrict__ pre,
                                                        b8* __restrict__ xs, int M, int K) {
  const int s = blockIdx.x, m = blockIdx.y, KS = K >> 4;
  const int lane = threadIdx.x, n = lane & 31, h = lane >> 5;
  const int row = 32 * m + n;
  b8 xf;
  if (row < M) {
    const f4* xp = reinterpret_cast<const f4*>(X + (long)row * K + 16 * s + 8 * h);
    f4 a = xp[0], b = xp[1];
    if (pre) {
      const f4* pp = reinterpret_cast<const f4*>(pre + (long)row * K + 16 * s + 8 * h);
      const f4 pa = pp[0], pb = pp[1];
#pragma unroll
      for (int j = 0; j < 4; ++j) { a[j] *= quick_gelu_grad(pa[j]); b[j] *= quick_gelu_grad(pb[j]); }
    }
    xf[0] = (__bf16)a[0]; xf[1] = (__bf16)a[1]; xf[2] = (__bf16)a[2]; xf[3] = (__bf16)a[3];
    xf[4] = (__bf16)b[0]; xf[5] = (__bf16)b[1]; xf[6] = (__bf16)b[2]; xf[7] = (__bf16)b[3];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) xf[j] = (__bf16)0.f;
  }
  xs[packed_chunk(m, s, KS, lane)] = xf;
}

// One workgroup per 32 output columns; the K range is dealt round-robin to 8 wavefronts (k-step s goes to wave s % 8), each
// wave keeps 6 k-steps of loads in flight (the GEMM is a latency chain otherwise: M <= 128 rows give the matrix core nothing
// to hide a round trip behind).  Every wave parks its partial tiles in LDS ([wave][m-tile][row][lane]: conflict-free both
// ways), ONE barrier, then the 16 MT accumulator rows are dealt to the 8 waves: each sums the 8 partials of its rows in a fixed
// order (deterministic) and runs the epilogue (bias, QuickGELU, residual, store) for them -- a tree reduction with the whole
// epilogue on wave 0 cost three barrier pairs and 64 serial load / store pairs on one wave.
// NB = k-steps a wave loads as ONE batch before their MFMAs: the per-iteration calls leave most of the chip idle (96-384 workgroups),
// so the only way to shorten a K = 3072 linear (24 k-steps per wave) is to have all of its loads in flight at once instead of four
// rounds of six -- 14.7 -> see profiles/r04_ab_kernels.txt
template <int MT, int NB = 6>
__global__ __launch_bounds__(64 * VIT_WAVES) void vit_linear_kernel(const b8* __restrict__ Xs, const b8* __restrict__ Wp,
                                                                    const float* __restrict__ bias, const float* __restrict__ res,
                                                                    float* __restrict__ Y, float* __restrict__ Ypre, int M, int N,
                                                                    int K, int act, __bf16* __restrict__ Ys = nullptr,
                                                                    const float* __restrict__ gpre = nullptr) {
  extern __shared__ __attribute__((aligned(16))) float red[];   // [VIT_WAVES][MT][16][64]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int n = lane & 31, h = lane >> 5;
  const int t = blockIdx.x;           // output column tile
  const int KS = K >> 4;              // k-steps of 16
  // blockIdx.y = group of MT 32-row tiles of the rows.  Per-iteration calls (M <= 128 rows): MT = 1, one workgroup per (column tile,
  // row tile) -- it then reads a quarter of the packed activations (the K = 3072 linears re-read 768 KB of them per workgroup from
  // L2 otherwise: 35 us) and the four workgroups that share a weight tile sit on one XCD (block id = x + gridDim.x * y, gridDim.x a
  // multiple of 8), i.e. share its L2.  (MT = 4, a weight fragment feeding four MFMAs, was the batched kernel before avc_vit_gemm.hip.)
  const int mb = blockIdx.y;
  Xs += (long)mb * MT * KS * 64;
  const int row0 = 32 * MT * mb;
  facc acc[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[m][r] = 0.f;
  const b8* wp = Wp + ((long)t * KS) * 64 + lane;
  const b8* xp = Xs + lane;
  for (int s0 = wv; s0 < KS; s0 += VIT_WAVES * NB) {
    b8 w[NB], x[MT][NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const int s = s0 + j * VIT_WAVES;
      if (s < KS) {
        w[j] = wp[(long)s * 64];
#pragma unroll
        for (int m = 0; m < MT; ++m) x[m][j] = xp[((long)m * KS + s) * 64];
      }
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (s0 + j * VIT_WAVES < KS) {
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = MF<b8>::mma(x[m][j], w[j], acc[m]);
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int r = 0; r < 16; ++r) red[((wv * MT + m) * 16 + r) * 64 + lane] = acc[m][r];
  __syncthreads();
  const int col = 32 * t + n;
  const float bv = bias ? bias[col] : 0.f;
  constexpr int PER_WAVE = MT * 16 / VIT_WAVES;   // accumulator rows per wave: 2 MT
#pragma unroll
  for (int q = 0; q < PER_WAVE; ++q) {
    const int item = wv * PER_WAVE + q, m = item >> 4, r = item & 15;
    const int row = row0 + 32 * m + acc_row(r, h);
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < VIT_WAVES; ++w) v += red[((w * MT + m) * 16 + r) * 64 + lane];
    if (row < M) {
      v += bv;
      const long o = (long)row * N + col;
      if (act == 1) {
        if (Ypre) Ypre[o] = v;
        v = quick_gelu(v);
      } else if (act == 2) {          // backward of a QuickGELU layer: this product is the gradient of its OUTPUT
        v *= quick_gelu_grad(gpre[o]);
      }
      if (res) v += res[o];
      if (Y) Y[o] = v;
    } else {
      v = 0.f;
    }
    // the packed pipeline (avc_vit_linear_packed): the result leaves (also) as the packed bf16 operand of the linear
    // behind it; the rows of the last tile past M are written as zeros
    if (Ys) Ys[packed_elem(row, col, N >> 4)] = (__bf16)v;
  }
}

// (batched calls: the LDS-staged GEMM of avc_vit_gemm.hip -- 128 x 128 blocks; 12.7 ms per encoder pass against 20.3 for the direct-from-L1
// kernel above, profiles/r03_score_bench.txt)
extern "C" long avc_vit_workspace_bytes(int M, int K) {
  const long mt = ((M + 127) / 128) * 4;   // whole groups of 4 row tiles (the rows past M are packed as zeros)
  return mt * (K / 16) * 1024L;
}

// The one dispatch of the file: y = f(xs W^T + b) (+ residual) from a packed operand (rows packed as avc_vit_workspace_bytes lays them
// out).  Up to 128 rows the latency kernel, one row tile per workgroup, with all of its modes (the batch of loads a wave keeps in flight
// covers its whole share of K up to K = 3072); more rows: the LDS-staged GEMM, or an error for what that does not cover.
static int vit_linear_dispatch(const char* who, const void* xs, const void* wp, const float* bias, const float* res, const float* gpre,
                               float* y, float* y_pre, void* ys, int M, int N, int K, int act, void* stream) {
  if (M <= 0) return 0;
  if ((N & 31) || (K & 15)) { avc_set_error("avc_vit_linear: need N % 32 == 0, K % 16 == 0"); return 1; }
  if ((act == 2) != (gpre != nullptr) || (!y && !ys)) { avc_set_error("avc_vit_linear: act 2 <=> gelu_pre; y or ys_packed"); return 1; }
  if (M <= 32 * VIT_MAX_MT) {
    const int per_wave = ((K >> 4) + VIT_WAVES - 1) / VIT_WAVES;
    const dim3 grid(N / 32, (M + 31) / 32), block(64 * VIT_WAVES);
    const int lds = VIT_WAVES * 4096;
    hipStream_t s = (hipStream_t)stream;
    const b8 *x8 = (const b8*)xs, *w8 = (const b8*)wp;
    __bf16* y8 = (__bf16*)ys;
    if (per_wave <= 6) hipLaunchKernelGGL((vit_linear_kernel<1, 6>), grid, block, lds, s, x8, w8, bias, res, y, y_pre, M, N, K, act, y8, gpre);
    else if (per_wave <= 12) hipLaunchKernelGGL((vit_linear_kernel<1, 12>), grid, block, lds, s, x8, w8, bias, res, y, y_pre, M, N, K, act, y8, gpre);
    else if (per_wave <= 18) hipLaunchKernelGGL((vit_linear_kernel<1, 18>), grid, block, lds, s, x8, w8, bias, res, y, y_pre, M, N, K, act, y8, gpre);
    else hipLaunchKernelGGL((vit_linear_kernel<1, 24>), grid, block, lds, s, x8, w8, bias, res, y, y_pre, M, N, K, act, y8, gpre);
  } else if (!avc_vit_gemm_lds(xs, wp, bias, res, gpre, y, y_pre, ys, M, N, K, act, ((M + 127) / 128) * 4, stream)) {
    avc_set_error("avc_vit_linear: more than 128 rows need N % 128 == 0, K % 32 == 0, no residual with an activation, neither y nor a "
                  "residual with a packed output, y_pre beside a packed output only with act 1, and a packed output with act 2");
    return 1;
  }
  return avc_check_launch(who);
}

// fp32 rows in: the packing pre-pass into `workspace` (whole groups of 4 row tiles above 128 rows), then the dispatch above
static int vit_linear_impl(const char* who, const float* x, const float* x_gelu_pre, const void* w_packed, const float* bias,
                           const float* residual, float* y, float* y_pre, int M, int N, int K, int act, void* workspace, void* stream) {
  if (M <= 0) return 0;
  if ((N & 31) || (K & 15)) { avc_set_error("avc_vit_linear: need N % 32 == 0, K % 16 == 0"); return 1; }
  if (!workspace) { avc_set_error("avc_vit_linear: workspace == NULL (avc_vit_workspace_bytes)"); return 1; }
  const int mt = M <= 32 * VIT_MAX_MT ? (M + 31) / 32 : ((M + 127) / 128) * 4;
  hipLaunchKernelGGL(vit_pack_x_kernel, dim3(K / 16, mt), dim3(64), 0, (hipStream_t)stream, x, x_gelu_pre, (b8*)workspace, M, K);
  return vit_linear_dispatch(who, workspace, w_packed, bias, residual, nullptr, y, y_pre, nullptr, M, N, K, act, stream);
}

extern "C" int avc_vit_linear(const float* x, const void* w_packed, const float* bias, const float* residual, float* y,
                              float* y_pre, int M, int N, int K, int act, void* workspace, void* stream) {
  return vit_linear_impl("avc_vit_linear", x, nullptr, w_packed, bias, residual, y, y_pre, M, N, K, act, workspace, stream);
}
extern "C" int avc_vit_linear_bwd_gelu(const float* dy, const float* pre, const void* wt_packed, float* dx, int M, int N, int K,
                                       void* workspace, void* stream) {
  return vit_linear_impl("avc_vit_linear_bwd_gelu", dy, pre, wt_packed, nullptr, nullptr, dx, nullptr, M, N, K, 0, workspace, stream);
}

// ---- the packed pipeline (clip_vit.BlocksFn): activations stay packed bf16 between the kernels ----
// a row's LayerNorm statistics (two-pass, fp32): a lane holds the 12 values 4 (lane + 64 c) + 0..3 of the 768
__device__ __forceinline__ void ln_row_stats(f4 (&v)[3], float eps, float& rstd) {   // on return v = x - mean
  constexpr int K = 768;
  float s1 = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) s1 += v[c][0] + v[c][1] + v[c][2] + v[c][3];
  const float mean = wave_sum(s1) * (1.f / K);
  float s2 = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int u = 0; u < 4; ++u) { v[c][u] -= mean; s2 += v[c][u] * v[c][u]; }
  rstd = rsqrtf(wave_sum(s2) * (1.f / K) + eps);
}
// LayerNorm (fp32 statistics, eps inside the square root like torch) of x[M,K] straight into the packed operand of the next linear.
// One workgroup per 32-row tile: a wavefront normalises 8 rows into an LDS image of the tile, then the fragments go out whole.
#define LNP_LD (768 + 8)
__global__ __launch_bounds__(256) void vit_ln_pack_kernel(const float* __restrict__ X, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps, b8* __restrict__ xs, int M) {
  __shared__ __attribute__((aligned(16))) __bf16 tile[32][LNP_LD];
  constexpr int K = 768, KS = K / 16;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, mt = blockIdx.x;
  f4 g[3], bt[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    g[c] = *reinterpret_cast<const f4*>(gamma + 4 * (lane + 64 * c));
    bt[c] = *reinterpret_cast<const f4*>(beta + 4 * (lane + 64 * c));
  }
  for (int q = 0; q < 8; ++q) {
    const int i = 8 * wv + q, row = 32 * mt + i;
    f4 v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = row < M ? *reinterpret_cast<const f4*>(X + (long)row * K + 4 * (lane + 64 * c)) : f4{0.f, 0.f, 0.f, 0.f};
    float rstd;
    ln_row_stats(v, eps, rstd);
#pragma unroll
    for (int c = 0; c < 3; ++c) put4(&tile[i][4 * (lane + 64 * c)], v[c] * rstd * g[c] + bt[c]);
  }
  __syncthreads();
  const int n = lane & 31, h = lane >> 5;
  for (int s = wv; s < KS; s += 4) xs[packed_chunk(mt, s, KS, lane)] = *reinterpret_cast<const b8*>(&tile[n][16 * s + 8 * h]);
}
// Up to 128 rows (the per-iteration calls) the tile kernel above is four workgroups walking 8 rows per wavefront one after the
// other -- a latency chain.  Here: one wavefront per row, all of a row's loads in flight at once, and no LDS: a lane holds 4
// consecutive columns of its row = one 8-byte half of a packed 16-byte chunk.  Rows past M are not touched (the caller's buffer holds zeros there).
__global__ __launch_bounds__(256) void vit_ln_pack_rows_kernel(const float* __restrict__ X, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, b8* __restrict__ xs, int M) {
  constexpr int K = 768;
  const int lane = threadIdx.x & 63, row = 4 * blockIdx.x + (threadIdx.x >> 6);
  if (row >= M) return;
  f4 v[3], g[3], bt[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    v[c] = *reinterpret_cast<const f4*>(X + (long)row * K + 4 * (lane + 64 * c));
    g[c] = *reinterpret_cast<const f4*>(gamma + 4 * (lane + 64 * c));
    bt[c] = *reinterpret_cast<const f4*>(beta + 4 * (lane + 64 * c));
  }
  float rstd;
  ln_row_stats(v, eps, rstd);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f4 o;
#pragma unroll
    for (int u = 0; u < 4; ++u) o[u] = v[c][u] * rstd * g[c][u] + bt[c][u];
    put_packed4(xs, K / 16, row, 4 * (lane + 64 * c), o);
  }
}
extern "C" int avc_vit_ln_pack(const float* x, const float* gamma, const float* beta, float eps, int M, int K, void* xs_packed,
                               void* stream) {
  if (K != 768) { avc_set_error("avc_vit_ln_pack: built for the ViT-B/32 width 768"); return 1; }
  if (M <= 0) return 0;
  if (M <= 32 * VIT_MAX_MT) {
    hipLaunchKernelGGL(vit_ln_pack_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, eps, (b8*)xs_packed, M);
    return avc_check_launch("avc_vit_ln_pack");
  }
  const int mt = ((M + 127) / 128) * 4;          // the row-tile groups of avc_vit_workspace_bytes (rows past M: LayerNorm of zeros = beta)
  hipLaunchKernelGGL(vit_ln_pack_kernel, dim3(mt), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, eps, (b8*)xs_packed, M);
  return avc_check_launch("avc_vit_ln_pack");
}
// y = f(xs W^T + b) (+ residual) from an already packed operand (avc_vit_ln_pack, avc_vit_pack, avc_vit_attention_*_packed, avc_vit_ln_bwd
// or a previous call's ys_packed).  act 0: identity; 1: QuickGELU (y_pre, if given, receives the pre-activation); 2: times
// QuickGELU'(gelu_pre[M,N]) (the backward of a QuickGELU layer folded into the product that yields the gradient of its output).  y (fp32
// rows) and ys_packed (the operand of the next linear) are both optional; which combinations more than 128 rows allow: include/avc.h
extern "C" int avc_vit_linear_packed(const void* xs_packed, const void* w_packed, const float* bias, const float* residual,
                                     const float* gelu_pre, float* y, float* y_pre, void* ys_packed, int M, int N, int K, int act,
                                     void* stream) {
  return vit_linear_dispatch("avc_vit_linear_packed", xs_packed, w_packed, bias, residual, gelu_pre, y, y_pre, ys_packed, M, N, K, act, stream);
}

// ---- the training pipeline (images WITH a gradient to the pixels; any M: up to 128 rows the latency kernel, more the GEMM of
// avc_vit_gemm.hip with its y_pre and act 2 epilogues): the same packed hand-offs forward and backward (clip_vit.BlocksFn).  Per block 7 launches forward (ln_pack, qkv, attention, out +
// residual, ln_pack, fc -> pre + packed QuickGELU, proj + residual) and 8 backward instead of 11 + 14 torch-autograd nodes with a
// packing launch in front of every linear, torch LayerNorm kernels and AccumulateGrad adds between them.
extern "C" int avc_vit_pack(const float* x, const float* gelu_pre, void* xs_packed, int M, int K, void* stream) {
  if (M <= 0) return 0;
  if (K & 15) { avc_set_error("avc_vit_pack: need K % 16 == 0"); return 1; }
  const int mt = (M + 31) / 32;
  hipLaunchKernelGGL(vit_pack_x_kernel, dim3(K / 16, mt), dim3(64), 0, (hipStream_t)stream, x, gelu_pre, (b8*)xs_packed, M, K);
  return avc_check_launch("avc_vit_pack");
}
// backward of LayerNorm over the last dimension (768) + the residual branch's gradient: dx = LN'(x; gamma)^T dy (+ res), written as
// fp32 rows and (xs_packed != NULL) as the packed operand of the transposed linear that consumes it.  Statistics recomputed from x
// in fp32 (two-pass, like vit_ln_pack_kernel); one wavefront per row (vit_ln_pack_rows_kernel); rows past M of xs are not touched.
__global__ __launch_bounds__(256) void vit_ln_bwd_kernel(const float* __restrict__ dY, const float* __restrict__ X,
                                                         const float* __restrict__ gamma, float eps, const float* __restrict__ res,
                                                         float* __restrict__ dX, b8* __restrict__ xs, int M) {
  constexpr int K = 768;
  const int lane = threadIdx.x & 63, row = 4 * blockIdx.x + (threadIdx.x >> 6);
  if (row >= M) return;
  f4 v[3], gy[3], rs[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long o = (long)row * K + 4 * (lane + 64 * c);
    v[c] = *reinterpret_cast<const f4*>(X + o);
    gy[c] = *reinterpret_cast<const f4*>(dY + o) * *reinterpret_cast<const f4*>(gamma + 4 * (lane + 64 * c));
    rs[c] = res ? *reinterpret_cast<const f4*>(res + o) : f4{0.f, 0.f, 0.f, 0.f};
  }
  float rstd;
  ln_row_stats(v, eps, rstd);
  float c1 = 0.f, c2 = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int u = 0; u < 4; ++u) { v[c][u] *= rstd; c1 += gy[c][u]; c2 += gy[c][u] * v[c][u]; }
  c1 = wave_sum(c1) * (1.f / K); c2 = wave_sum(c2) * (1.f / K);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    f4 dx;
#pragma unroll
    for (int u = 0; u < 4; ++u) dx[u] = rstd * (gy[c][u] - c1 - v[c][u] * c2) + rs[c][u];
    *reinterpret_cast<f4*>(dX + (long)row * K + 4 * (lane + 64 * c)) = dx;
    if (xs) put_packed4(xs, K / 16, row, 4 * (lane + 64 * c), dx);
  }
}
extern "C" int avc_vit_ln_bwd(const float* dy, const float* x, const float* gamma, float eps, const float* residual_grad, float* dx,
                              void* xs_packed, int M, int K, void* stream) {
  if (K != 768) { avc_set_error("avc_vit_ln_bwd: built for the ViT-B/32 width 768"); return 1; }
  if (M <= 0) return 0;
  hipLaunchKernelGGL(vit_ln_bwd_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, dy, x, gamma, eps, residual_grad, dx,
                     (b8*)xs_packed, M);
  return avc_check_launch("avc_vit_ln_bwd");
}

// ---------------------------------------------------------------------------------------------------------
// attention: qkv [B,T,3*W] (q | k | v, head hd at column hd*64), out [B,T,W].  The image tower's kernels are the matrix-core ones of
// avc_vit_attn.hip; the fp32 VALU kernels they replaced in round 3 (profiles/r03_ab_kernels.txt) are gone.
// ---------------------------------------------------------------------------------------------------------
#define TA_LD (ATM_D + 1)   // +1 padding: thread i reads row i -> conflict-free

// Text tower (clip/model.py encode_text: 77 tokens, 8 heads of 64, causal mask): forward only -- prompts are encoded once per
// run (main.py:273-288).  One workgroup per (sequence, head), thread i = query row i, K/V rows in LDS, online softmax.
#define TA_TMAX 128
__global__ __launch_bounds__(TA_TMAX) void text_attn_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, int T,
                                                                int Wd, int heads, float scale, int causal) {
  extern __shared__ __attribute__((aligned(16))) float tsm[];
  float (*Ks)[TA_LD] = reinterpret_cast<float (*)[TA_LD]>(tsm);
  float (*Vs)[TA_LD] = Ks + T;
  const int b = blockIdx.x / heads, hd = blockIdx.x % heads;
  const int i = threadIdx.x;
  const float* base = qkv + (long)b * T * 3 * Wd + hd * ATM_D;
  for (int e = threadIdx.x; e < T * ATM_D; e += TA_TMAX) {
    const int r = e / ATM_D, c = e % ATM_D;
    Ks[r][c] = base[(long)r * 3 * Wd + Wd + c];
    Vs[r][c] = base[(long)r * 3 * Wd + 2 * Wd + c];
  }
  __syncthreads();
  if (i >= T) return;
  float q[ATM_D], o[ATM_D];
#pragma unroll
  for (int c = 0; c < ATM_D; ++c) { q[c] = base[(long)i * 3 * Wd + c] * scale; o[c] = 0.f; }
  float mx = -1e30f, sum = 0.f;
  const int jend = causal ? i + 1 : T;
  for (int j = 0; j < jend; ++j) {
    float sc = 0.f;
#pragma unroll
    for (int c = 0; c < ATM_D; ++c) sc += q[c] * Ks[j][c];
    const float mn = fmaxf(mx, sc);
    const float corr = __expf(mx - mn), pj = __expf(sc - mn);
    sum = sum * corr + pj;
#pragma unroll
    for (int c = 0; c < ATM_D; ++c) o[c] = o[c] * corr + pj * Vs[j][c];
    mx = mn;
  }
  const float inv = 1.f / sum;
  float* op = out + ((long)b * T + i) * Wd + hd * ATM_D;
#pragma unroll
  for (int c = 0; c < ATM_D; ++c) op[c] = o[c] * inv;
}

// one rule for the four entry points: 0 = refused (avc_last_error() says why), 1 = the 50-token kernels, 2 = the tiled ones
static int vit_attn_route(int T, int width, int heads) {
  if (T < 1 || T > 256 || heads < 1 || width != heads * ATM_D) {
    avc_set_error("avc_vit_attention: 1 <= T <= 256 tokens, head dim 64 (width == heads * 64)");
    return 0;
  }
  return T == ATM_T ? 1 : 2;
}
extern "C" int avc_vit_attention_bwd_packed(const float* qkv, const float* dout, void* dqkv_packed, int B, int T, int width, int heads,
                                            void* stream) {
  const int route = vit_attn_route(T, width, heads);
  if (!route) return 1;
  if (route == 2) return B <= 0 ? 0 : avc_attn_bwd_tiled_packed(qkv, dout, dqkv_packed, B, T, width, heads, stream);
  return avc_attn_bwd_mfma_packed(qkv, dout, dqkv_packed, B, width, heads, stream);
}
extern "C" int avc_vit_attention_fwd_packed(const float* qkv, void* out_packed, int B, int T, int width, int heads, void* stream) {
  const int route = vit_attn_route(T, width, heads);
  if (!route) return 1;
  if (route == 2) return B <= 0 ? 0 : avc_attn_fwd_tiled_packed(qkv, out_packed, B, T, width, heads, stream);
  return avc_attn_fwd_mfma_packed(qkv, out_packed, B, width, heads, stream);
}

extern "C" int avc_vit_attention_fwd(const float* qkv, float* out, int B, int T, int width, int heads, void* stream) {
  const int route = vit_attn_route(T, width, heads);
  if (!route) return 1;
  if (route == 2) return B <= 0 ? 0 : avc_attn_fwd_tiled(qkv, out, B, T, width, heads, stream);
  return avc_attn_fwd_mfma(qkv, out, B, width, heads, stream);
}
extern "C" int avc_text_attention_fwd(const float* qkv, float* out, int B, int T, int width, int heads, int causal, void* stream) {
  if (T < 1 || T > TA_TMAX || width != heads * ATM_D) { avc_set_error("avc_text_attention_fwd: 1 <= T <= 128, head dim 64"); return 1; }
  if (B <= 0) return 0;
  const size_t lds = 2 * (size_t)T * TA_LD * sizeof(float);
  static unsigned long long attr_seen = 0;
  if (avc_first_use_on_device(attr_seen)) {
    hipFuncSetAttribute((const void*)text_attn_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * TA_TMAX * TA_LD * 4);
  }
  hipLaunchKernelGGL(text_attn_fwd_kernel, dim3(B * heads), dim3(TA_TMAX), lds, (hipStream_t)stream, qkv, out, T, width, heads,
                     0.125f, causal);
  return avc_check_launch("avc_text_attention_fwd");
}
extern "C" int avc_vit_attention_bwd(const float* qkv, const float* dout, float* dqkv, int B, int T, int width, int heads,
                                     void* stream) {
  const int route = vit_attn_route(T, width, heads);
  if (!route) return 1;
  if (route == 2) return B <= 0 ? 0 : avc_attn_bwd_tiled(qkv, dout, dqkv, B, T, width, heads, stream);
  return avc_attn_bwd_mfma(qkv, dout, dqkv, B, width, heads, stream);
}
