// What the three CLIP tower sources (avc_vit.hip, avc_vit_gemm.hip, avc_vit_attn.hip) share: the packed bf16 operand layout, the MFMA
// accumulator row map, QuickGELU, and the prototypes of the launchers that avc_vit.hip's entry points dispatch to.
#pragma once
#include "avc_common.h"

#define ATM_T 50      // tokens of a ViT-B/32 image (the 50-token attention kernels)
#define ATM_D 64      // head dim of every attention kernel, image and text tower

// row of register r of a 32x32 MFMA accumulator tile in lane half h (avc_common.h, C/D layout)
__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// Packed bf16 operand of a linear: [row tile of 32][k-step of 16 columns][lane (row & 31, half)][8 columns], KS k-steps per row tile --
// lane (i, h) of k-step s of row tile m holds X[32 m + i][16 s + 8 h + 0..7], one 16-byte chunk, so both GEMMs read their activations
// with the same coalesced 16-B-per-lane loads as their weights.
// packed_chunk: the chunk's index (in b8 units).  Element (row, col) is slot col & 7 of lane (row & 31, (col >> 3) & 1) of k-step col >> 4
// of row tile row >> 5: packed_chunk_of = that chunk, packed_elem = the element's index in bf16 units.  S, R = int or long, as the caller's
// k-step and row are.
template <typename S>
__device__ __forceinline__ long packed_chunk(long mt, S s, int KS, int lane) { return (mt * KS + s) * 64 + lane; }
template <typename R>
__device__ __forceinline__ long packed_chunk_of(R row, int col, int KS) {
  return (((long)(row >> 5)) * KS + (col >> 4)) * 64 + (row & 31) + 32 * ((col >> 3) & 1);
}
template <typename R>
__device__ __forceinline__ long packed_elem(R row, int col, int KS) { return packed_chunk_of(row, col, KS) * 8 + (col & 7); }
__device__ __forceinline__ void put4(__bf16* p, f4 v) {   // 4 consecutive bf16 (p 8-byte aligned)
  typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
  bf4 o = {(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
  *reinterpret_cast<bf4*>(p) = o;
}
__device__ __forceinline__ void put_packed_elem(__bf16* xs, int KS, long row, int col, float v) { xs[packed_elem(row, col, KS)] = (__bf16)v; }
__device__ __forceinline__ void put_packed4(b8* xs, int KS, int row, int col, f4 v) {   // 4 consecutive columns from col (col % 4 == 0)
  put4(reinterpret_cast<__bf16*>(xs + packed_chunk_of(row, col, KS)) + (col & 7), v);
}

// QuickGELU (clip/model.py: x * sigmoid(1.702 x)) and its derivative at the pre-activation
__device__ __forceinline__ float quick_gelu(float v) { return v * sigmoidf_(1.702f * v); }
__device__ __forceinline__ float quick_gelu_grad(float pre) {
  const float sg = sigmoidf_(1.702f * pre);
  return sg + 1.702f * pre * sg * (1.f - sg);
}

// avc_vit_gemm.hip: the LDS-staged GEMM of the batched calls (more than 128 rows, whole groups of 4 row tiles packed); false = a shape it
// does not cover
bool avc_vit_gemm_lds(const void* xs, const void* wp, const float* bias, const float* res, const float* gpre, float* y, float* y_pre,
                      void* ys, int M, int N, int K, int act, int mt_packed, void* stream);
// avc_vit_attn.hip: matrix-core attention over 50 tokens ...
int avc_attn_fwd_mfma(const float* qkv, float* out, int B, int width, int heads, void* stream);
int avc_attn_bwd_mfma(const float* qkv, const float* dout, float* dqkv, int B, int width, int heads, void* stream);
int avc_attn_fwd_mfma_packed(const float* qkv, void* out_packed, int B, int width, int heads, void* stream);
int avc_attn_bwd_mfma_packed(const float* qkv, const float* dout, void* dqkv_packed, int B, int width, int heads, void* stream);
// ... and over every other T in [1, 256]: the keys walked in 32-key tiles
int avc_attn_fwd_tiled(const float* qkv, float* out, int B, int T, int width, int heads, void* stream);
int avc_attn_bwd_tiled(const float* qkv, const float* dout, float* dqkv, int B, int T, int width, int heads, void* stream);
int avc_attn_fwd_tiled_packed(const float* qkv, void* out_packed, int B, int T, int width, int heads, void* stream);
int avc_attn_bwd_tiled_packed(const float* qkv, const float* dout, void* dqkv_packed, int B, int T, int width, int heads, void* stream);
