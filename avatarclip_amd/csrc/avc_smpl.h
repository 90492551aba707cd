// Device code shared by posing the SMPL body (avc_smpl.hip) and its gradient to the pose (avc_smpl_grad.hip): the gradient is the exact
// adjoint of the forward "rebuilt as the forward does", and what it rebuilds is compiled from the functions below, not restated.  Everything
// is fp32, every multiply-add is ONE fused operation written as such (no contraction left to the compiler), and the ORDER of the operations
// is the contract: the numpy restatements in tests/ follow it.  The arithmetic is smpl_lbs's: batch_rodrigues, batch_rigid_transform, lbs.
//
// smpl_rodrigues (batch_rodrigues, its quirk at tiny angles included):
//      r' = r + 1e-8 (each component); angle = sqrt((r'x r'x + r'y r'y) + r'z r'z); d = r / angle; s = sin(angle), c1 = 1 - cos(angle)
//      K = [[0, -dz, dy], [dz, 0, -dx], [-dy, dx, 0]];  K2[a][b] = (K[a][0] K[0][b] + K[a][1] K[1][b]) + K[a][2] K[2][b]
//      R[a][b] = (I[a][b] + s K[a][b]) + c1 K2[a][b]
// smpl_world_rot (batch_rigid_transform's chain, rotations; a parent comes before its child: 0 <= parents[i] < i):
//      world_0.R = R_0;  world_i.R[a][b] = (P.R[a][0] R_i[0][b] + P.R[a][1] R_i[1][b]) + P.R[a][2] R_i[2][b]      (P = world of the parent)
//    The worlds of a frame stay in the caller's LDS, one column per lane ([joint][3 rows of ROW floats][LANES lanes]: conflict-free).
// The tile of the two vertex kernels: a workgroup owns SMPL_VT = 256 vertices x SMPL_FT = 8 frames.
// smpl_stage_tile: feat as [k][frame of the tile] and A as [frame][joint][row] into LDS; a frame past the end is zeros.
// smpl_blend_lanes, smpl_blend_shapes (lbs's pose blend shapes), per ELEMENT e = 3 v + c of the tile: lane l owns elements l, l + 256,
//    l + 512 of the tile's 768, so every load of a posedirs row segment is contiguous across the wavefront.  acc = 0;
//    acc = fma(feat[t, k], posedirs[k, e], acc) for k = 0..206 ascending; the caller stores v_posed[e] = acc + v_shaped[e].  A row segment is
//    loaded once and used for all the tile's frames (3 x 8 accumulators in registers, SMPL_KU = 9 rows = one joint's block of posedirs in
//    flight), the frames' feat values are read from LDS by broadcast (two 16-byte reads per k).
// smpl_blend_transform (lbs's T = W A): M = 0 (3 x NC); M[r][q] = fma(weights[v, j], A[t, j][r][q], M[r][q]) for j = 0..23 ascending.  A is
//    read from LDS by broadcast, the vertex's 24 weights (smpl_vertex_weights) sit in registers for all the tile's frames.
#pragma once
#include "avc_common.h"

#define SMPL_J 24
#define SMPL_K 207
#define SMPL_VT 256       // vertices per tile = threads
#define SMPL_FT 8         // frames per tile
#define SMPL_KU 9         // posedirs rows in flight per lane (207 = 23 x 9)
#define SMPL_MAX_FRAMES (65535 * SMPL_FT) // frames one launch's grid takes

static_assert(SMPL_K % SMPL_KU == 0 && SMPL_K == 9 * (SMPL_J - 1), "207 pose-blend rows = 23 joints x 9 = 23 groups of SMPL_KU");
static_assert(SMPL_FT == 8, "the feat tile is read as two f4 per row");

struct SmplRot {
  float K[3][3], R[3][3];
  float angle, s, c, c1;
};
__device__ __forceinline__ void smpl_rodrigues(float rx, float ry, float rz, SmplRot& o) {
  const float ex = rx + 1e-8f, ey = ry + 1e-8f, ez = rz + 1e-8f;
  o.angle = __builtin_sqrtf(__builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex)));
  const float dx = rx / o.angle, dy = ry / o.angle, dz = rz / o.angle;
  o.s = sinf(o.angle);
  o.c = cosf(o.angle);
  o.c1 = 1.f - o.c;
  o.K[0][0] = 0.f; o.K[0][1] = -dz; o.K[0][2] = dy;
  o.K[1][0] = dz;  o.K[1][1] = 0.f; o.K[1][2] = -dx;
  o.K[2][0] = -dy; o.K[2][1] = dx;  o.K[2][2] = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const float k2 = __builtin_fmaf(o.K[a][2], o.K[2][b], __builtin_fmaf(o.K[a][1], o.K[1][b], o.K[a][0] * o.K[0][b]));
      o.R[a][b] = __builtin_fmaf(o.c1, k2, __builtin_fmaf(o.s, o.K[a][b], a == b ? 1.f : 0.f));
    }
}

// W[a][0..2] = the world rotation of joint i with parent p and own rotation R; w = the lane's column of the worlds so far, element b of row a
// of joint q at w[(3 ROW q + ROW a + b) * LANES].  (the caller checks the tree: a parent that does not come first reads nothing and gives NaN)
template <int LANES, int ROW, int NC>
__device__ __forceinline__ void smpl_world_rot(const float* w, int i, int p, const float (&R)[3][3], float (&W)[3][NC]) {
  if (i == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      W[a][0] = R[a][0]; W[a][1] = R[a][1]; W[a][2] = R[a][2];
    }
  } else if ((unsigned)p < (unsigned)i) {
    const float* pw = w + 3 * ROW * p * LANES;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float p0 = pw[(ROW * a) * LANES], p1 = pw[(ROW * a + 1) * LANES], p2 = pw[(ROW * a + 2) * LANES];
#pragma unroll
      for (int b = 0; b < 3; ++b) W[a][b] = __builtin_fmaf(p2, R[2][b], __builtin_fmaf(p1, R[1][b], p0 * R[0][b]));
    }
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) W[a][0] = W[a][1] = W[a][2] = __uint_as_float(0x7FC00000u);
  }
}

// feat / A point at the first frame of the launch; t0 = the tile's first frame, nf = its frames that exist.  The caller's barrier follows.
__device__ __forceinline__ void smpl_stage_tile(const float* __restrict__ feat, const f4* __restrict__ A, long t0, int nf, f4* s_feat, f4* s_A) {
  const int tid = threadIdx.x;
  float* sf = reinterpret_cast<float*>(s_feat);
  for (int i = tid; i < SMPL_K * SMPL_FT; i += SMPL_VT) {
    const int k = i / SMPL_FT, f = i - k * SMPL_FT;
    sf[i] = f < nf ? feat[(t0 + f) * SMPL_K + k] : 0.f;          // (a frame past the end: zeros, computed and never stored)
  }
  for (int i = tid; i < SMPL_FT * SMPL_J * 3; i += SMPL_VT) {
    const int f = i / (SMPL_J * 3);
    s_A[i] = f < nf ? A[t0 * (SMPL_J * 3) + i] : f4{0.f, 0.f, 0.f, 0.f};
  }
}

// the lane's elements e0 + tid + 256 c, c = 0..2, of the E = 3 V of a posedirs row: which exist, and where their column starts
__device__ __forceinline__ void smpl_blend_lanes(const float* __restrict__ posedirs, long e0, long E, bool (&ok)[3], const float* (&pd)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long e = e0 + threadIdx.x + SMPL_VT * c;
    ok[c] = e < E;
    pd[c] = posedirs + (ok[c] ? e : 0);
  }
}

__device__ __forceinline__ void smpl_blend_shapes(const bool (&ok)[3], const float* const (&pd)[3], long E, const f4* s_feat,
                                                  float (&acc)[SMPL_FT][3]) {
#pragma unroll
  for (int f = 0; f < SMPL_FT; ++f) acc[f][0] = acc[f][1] = acc[f][2] = 0.f;
  for (int k0 = 0; k0 < SMPL_K; k0 += SMPL_KU) {
    float p[SMPL_KU][3];
#pragma unroll
    for (int u = 0; u < SMPL_KU; ++u)
#pragma unroll
      for (int c = 0; c < 3; ++c) p[u][c] = ok[c] ? pd[c][(k0 + u) * E] : 0.f;
#pragma unroll
    for (int u = 0; u < SMPL_KU; ++u) {
      const f4 fa = s_feat[2 * (k0 + u)], fb = s_feat[2 * (k0 + u) + 1];
#pragma unroll
      for (int f = 0; f < SMPL_FT; ++f) {
        const float x = f < 4 ? fa[f & 3] : fb[f & 3];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[f][c] = __builtin_fmaf(x, p[u][c], acc[f][c]);
      }
    }
  }
}

__device__ __forceinline__ void smpl_vertex_weights(const f4* __restrict__ weights, long v, float (&wv)[SMPL_J]) {
#pragma unroll
  for (int q = 0; q < SMPL_J / 4; ++q) {
    const f4 w4 = weights[v * (SMPL_J / 4) + q];
    wv[4 * q] = w4[0]; wv[4 * q + 1] = w4[1]; wv[4 * q + 2] = w4[2]; wv[4 * q + 3] = w4[3];
  }
}

// columns 0..NC-1 of frame f's blended transform: NC = 4 for [M.R | M.t], 3 for M.R alone
template <int NC>
__device__ __forceinline__ void smpl_blend_transform(const f4* s_A, int f, const float (&wv)[SMPL_J], float (&M)[3][NC]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < NC; ++q) M[r][q] = 0.f;
#pragma unroll
  for (int j = 0; j < SMPL_J; ++j) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const f4 a = s_A[(f * SMPL_J + j) * 3 + r];
#pragma unroll
      for (int q = 0; q < NC; ++q) M[r][q] = __builtin_fmaf(wv[j], a[q], M[r][q]);
    }
  }
}

static inline long smpl_vertex_tiles(int V) { return ((long)V + SMPL_VT - 1) / SMPL_VT; }

// launch(grid, t0, n) for every run of n <= SMPL_MAX_FRAMES frames from frame t0: a launch's grid takes 65535 frame tiles
template <class F>
static inline void smpl_split_frames(int V, int T, F launch) {
  const unsigned gx = (unsigned)smpl_vertex_tiles(V);
  for (long t0 = 0; t0 < T; t0 += SMPL_MAX_FRAMES) {
    const int n = (int)min((long)SMPL_MAX_FRAMES, (long)T - t0);
    launch(dim3(gx, (unsigned)((n + SMPL_FT - 1) / SMPL_FT)), t0, n);
  }
}
