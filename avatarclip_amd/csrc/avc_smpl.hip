// Posing the SMPL body without a gradient (avatarclip_amd/smpl_lbs.py pose_hip): what smpl_lbs.lbs computes with about a hundred small torch
// kernels and a [T, V, 4, 4] transform tensor, as two launches.  The reference poses through smplx (AvatarAnimate/visualize.py:98-102,
// :115-119 for its previews); the arithmetic restated here is smpl_lbs's: batch_rodrigues, batch_rigid_transform, lbs.  Everything is fp32,
// every multiply-add below is ONE fused operation written as such (no contraction left to the compiler), there is no atomic: the result
// of a frame is the same bits in every run, in every batch and at every place in a batch.
//
// 1. avc_smpl_joint_mats: one lane per frame walks the 24 joints in index order (a parent comes before its child: 0 <= parents[i] < i).
//      r' = r + 1e-8 (each component); angle = sqrt((r'x r'x + r'y r'y) + r'z r'z); d = r / angle; s = sin(angle), c1 = 1 - cos(angle)
//      K = [[0, -dz, dy], [dz, 0, -dx], [-dy, dx, 0]];  K2[a][b] = (K[a][0] K[0][b] + K[a][1] K[1][b]) + K[a][2] K[2][b]
//      R[a][b] = (I[a][b] + s K[a][b]) + c1 K2[a][b]                    (batch_rodrigues, its quirk at tiny angles included)
//      feat[t, 9 (i - 1) + 3 a + b] = R_i[a][b] - I[a][b], i = 1..23    (lbs's pose_feature)
//      rel_i = j_i - j_parent(i) (rel_0 = j_0);  world_0 = [R_0 | j_0]
//      world_i.R[a][b] = (P.R[a][0] R_i[0][b] + P.R[a][1] R_i[1][b]) + P.R[a][2] R_i[2][b]          (P = world of the parent)
//      world_i.t[a]    = ((P.R[a][0] rel_i[0] + P.R[a][1] rel_i[1]) + P.R[a][2] rel_i[2]) + P.t[a]
//      A_i = [world_i.R | world_i.t - ((W.R[a][0] j_i[0] + W.R[a][1] j_i[1]) + W.R[a][2] j_i[2])]   (batch_rigid_transform's A, rows 0..2)
//    The worlds of a frame stay in LDS, one column per lane ([joint][12][lane]: conflict-free).  A chain of 23 small products per lane:
//    bound by latency, not by throughput.
// 2. avc_smpl_pose: a workgroup owns SP_VT = 256 vertices x SP_FT = 8 frames.
//    a. pose blend shapes, per ELEMENT e = 3 v + c of the tile (lane l owns elements l, l + 256, l + 512 of the tile's 768, so every
//       load of a posedirs row segment is contiguous across the wavefront): acc = 0; acc = fma(feat[t, k], posedirs[k, e], acc) for
//       k = 0..206 ascending; v_posed[e] = acc + v_shaped[e].  A row segment is loaded once and used for all the tile's frames (3 x 8
//       accumulators in registers), the frames' feat values are read from LDS by broadcast ([k][frame]: two 16-byte reads per k).
//    b. v_posed goes through LDS to the lane that owns the vertex (stride-3 reads: conflict-free).
//    c. blend: M = 0 (3 x 4); M[r][q] = fma(weights[v, j], A[t, j][r][q], M[r][q]) for j = 0..23 ascending (lbs's T = W A);
//       out[t, v][r] = fma(M[r][0], x, fma(M[r][1], y, fma(M[r][2], z, M[r][3]))).  A is read from LDS by broadcast, the vertex's 24
//       weights sit in registers for all the tile's frames.
//    d. the results go back through LDS and are stored contiguously.
//    posedirs (17 MB for SMPL) is read ceil(T / 8) times instead of T times; the kernel is bound by that stream (0.5 GFLOP at T = 60).
//    The 256 x 8 tile: 24 accumulators, 27 loads in flight (9 rows: one joint's block of posedirs), then 24 weights + 12 blend sums; the
//    compiler takes 186 registers for it, two workgroups a CU, and LDS is 6.5 KiB (feat) + 9 KiB (A) + 24 KiB (v_posed) = 39.5 KiB, which
//    would admit three.  16 frames would halve the posedirs traffic again but double the accumulators and the LDS, and at T = 60 (27 x 8
//    = 216 tiles for SMPL's 6890 vertices, on 256 CUs) leave half of the CUs without a tile.
#include "avc_common.h"
#include "../../include/avc.h"

#define SJ_LANES 32       // frames per workgroup of the joint kernel (24 x 12 x 32 floats of LDS = 36 KiB)
#define SP_VT 256         // vertices per tile = threads
#define SP_FT 8           // frames per tile
#define SP_KU 9           // posedirs rows in flight per lane (207 = 23 x 9)
#define SMPL_J 24
#define SMPL_K 207
#define SP_MAX_FRAMES (65535 * SP_FT)     // frames one launch's grid takes

static_assert(SMPL_K % SP_KU == 0 && SMPL_K == 9 * (SMPL_J - 1), "207 pose-blend rows = 23 joints x 9 = 23 groups of SP_KU");
static_assert(SP_FT == 8, "the feat tile is read as two f4 per row");

// ------------------------------------------------------------------------------------------------------------- joint matrices
__global__ __launch_bounds__(SJ_LANES) void smpl_joint_mats_kernel(const float* __restrict__ pose, const float* __restrict__ joints,
                                                                   const int* __restrict__ parents, int T, float* __restrict__ feat,
                                                                   f4* __restrict__ A) {
  __shared__ float s_w[SMPL_J * 12 * SJ_LANES];
  __shared__ float s_j[SMPL_J * 3];
  __shared__ int s_p[SMPL_J];
  const int lane = threadIdx.x;
  for (int i = lane; i < SMPL_J * 3; i += SJ_LANES) s_j[i] = joints[i];
  if (lane < SMPL_J) s_p[lane] = parents[lane];
  __syncthreads();                                              // the only barrier: lanes past the end may leave now
  const long t = (long)blockIdx.x * SJ_LANES + lane;
  if (t >= T) return;
  const float* r = pose + t * (SMPL_J * 3);
  float* w = s_w + lane;                                        // w[(12 i + e) * SJ_LANES]: element e of world_i, rows [R | t]
  for (int i = 0; i < SMPL_J; ++i) {
    const float rx = r[3 * i], ry = r[3 * i + 1], rz = r[3 * i + 2];
    const float ex = rx + 1e-8f, ey = ry + 1e-8f, ez = rz + 1e-8f;
    const float angle = __builtin_sqrtf(__builtin_fmaf(ez, ez, __builtin_fmaf(ey, ey, ex * ex)));
    const float dx = rx / angle, dy = ry / angle, dz = rz / angle;
    const float s = sinf(angle), c1 = 1.f - cosf(angle);
    const float K[3][3] = {{0.f, -dz, dy}, {dz, 0.f, -dx}, {-dy, dx, 0.f}};
    float R[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        const float k2 = __builtin_fmaf(K[a][2], K[2][b], __builtin_fmaf(K[a][1], K[1][b], K[a][0] * K[0][b]));
        R[a][b] = __builtin_fmaf(c1, k2, __builtin_fmaf(s, K[a][b], a == b ? 1.f : 0.f));
      }
    if (i > 0) {
      float* f = feat + t * SMPL_K + 9 * (i - 1);
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) f[3 * a + b] = R[a][b] - (a == b ? 1.f : 0.f);
    }
    const float jx = s_j[3 * i], jy = s_j[3 * i + 1], jz = s_j[3 * i + 2];
    float W[3][4];
    const int p = s_p[i];
    if (i == 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        W[a][0] = R[a][0]; W[a][1] = R[a][1]; W[a][2] = R[a][2];
      }
      W[0][3] = jx; W[1][3] = jy; W[2][3] = jz;
    } else if ((unsigned)p < (unsigned)i) {
      const float lx = jx - s_j[3 * p], ly = jy - s_j[3 * p + 1], lz = jz - s_j[3 * p + 2];
      const float* pw = w + 12 * p * SJ_LANES;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float p0 = pw[(4 * a) * SJ_LANES], p1 = pw[(4 * a + 1) * SJ_LANES], p2 = pw[(4 * a + 2) * SJ_LANES], p3 = pw[(4 * a + 3) * SJ_LANES];
#pragma unroll
        for (int b = 0; b < 3; ++b) W[a][b] = __builtin_fmaf(p2, R[2][b], __builtin_fmaf(p1, R[1][b], p0 * R[0][b]));
        W[a][3] = __builtin_fmaf(p2, lz, __builtin_fmaf(p1, ly, p0 * lx)) + p3;
      }
    } else {                                                    // (the caller checks the tree: a parent that does not come first reads nothing)
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) W[a][b] = __uint_as_float(0x7FC00000u);
    }
    f4* dst = A + (t * SMPL_J + i) * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 4; ++b) w[(12 * i + 4 * a + b) * SJ_LANES] = W[a][b];
      const float back = __builtin_fmaf(W[a][2], jz, __builtin_fmaf(W[a][1], jy, W[a][0] * jx));
      dst[a] = f4{W[a][0], W[a][1], W[a][2], W[a][3] - back};
    }
  }
}

extern "C" int avc_smpl_joint_mats(const float* pose, const float* joints, const int* parents, int T, float* feat, float* A, void* stream) {
  if (T < 0) { avc_set_error("avc_smpl_joint_mats: bad sizes"); return 1; }
  if (T == 0) return 0;
  if (!pose || !joints || !parents || !feat || !A) { avc_set_error("avc_smpl_joint_mats: NULL buffer"); return 1; }
  if (((unsigned long long)A & 15ull) || (((unsigned long long)pose | (unsigned long long)joints | (unsigned long long)parents | (unsigned long long)feat) & 3ull)) {
    avc_set_error("avc_smpl_joint_mats: A not 16-byte or pose / joints / parents / feat not 4-byte aligned");
    return 1;
  }
  hipLaunchKernelGGL(smpl_joint_mats_kernel, dim3((unsigned)(((long)T + SJ_LANES - 1) / SJ_LANES)), dim3(SJ_LANES), 0, (hipStream_t)stream, pose,
                     joints, parents, T, feat, (f4*)A);
  return avc_check_launch("avc_smpl_joint_mats");
}

// ------------------------------------------------------------------------------------------------------------- blend shapes and skinning
// feat / A / out point at frame t0 of the call; T = the frames of this launch (gridDim.y = ceil(T / SP_FT))
__global__ __launch_bounds__(SP_VT) void smpl_pose_kernel(const float* __restrict__ v_shaped, const float* __restrict__ posedirs,
                                                          const f4* __restrict__ weights, const float* __restrict__ feat,
                                                          const f4* __restrict__ A, int V, int T, float* __restrict__ out) {
  __shared__ f4 s_feat[SMPL_K * 2];                             // [k][frame of the tile]
  __shared__ f4 s_A[SP_FT * SMPL_J * 3];                        // [frame][joint][row]
  __shared__ float s_vp[SP_FT * SP_VT * 3];                     // [frame][element of the tile]
  const int tid = threadIdx.x;
  const long v0 = (long)blockIdx.x * SP_VT;
  const long t0 = (long)blockIdx.y * SP_FT;
  const int nf = (int)min((long)SP_FT, (long)T - t0);           // frames of this tile that exist (>= 1)
  const long E = 3L * V;                                        // elements of a posedirs row
  const long e0 = 3 * v0;

  {
    float* sf = reinterpret_cast<float*>(s_feat);
    for (int i = tid; i < SMPL_K * SP_FT; i += SP_VT) {
      const int k = i / SP_FT, f = i - k * SP_FT;
      sf[i] = f < nf ? feat[(t0 + f) * SMPL_K + k] : 0.f;        // (a frame past the end: zeros, computed and never stored)
    }
    for (int i = tid; i < SP_FT * SMPL_J * 3; i += SP_VT) {
      const int f = i / (SMPL_J * 3);
      s_A[i] = f < nf ? A[t0 * (SMPL_J * 3) + i] : f4{0.f, 0.f, 0.f, 0.f};
    }
  }
  __syncthreads();

  // a. pose blend shapes of elements e0 + tid + 256 c, c = 0..2
  bool ok[3];
  const float* pd[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long e = e0 + tid + SP_VT * c;
    ok[c] = e < E;
    pd[c] = posedirs + (ok[c] ? e : 0);
  }
  float acc[SP_FT][3];
#pragma unroll
  for (int f = 0; f < SP_FT; ++f) acc[f][0] = acc[f][1] = acc[f][2] = 0.f;
  for (int k0 = 0; k0 < SMPL_K; k0 += SP_KU) {
    float p[SP_KU][3];
#pragma unroll
    for (int u = 0; u < SP_KU; ++u)
#pragma unroll
      for (int c = 0; c < 3; ++c) p[u][c] = ok[c] ? pd[c][(k0 + u) * E] : 0.f;
#pragma unroll
    for (int u = 0; u < SP_KU; ++u) {
      const f4 fa = s_feat[2 * (k0 + u)], fb = s_feat[2 * (k0 + u) + 1];
#pragma unroll
      for (int f = 0; f < SP_FT; ++f) {
        const float x = f < 4 ? fa[f & 3] : fb[f & 3];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[f][c] = __builtin_fmaf(x, p[u][c], acc[f][c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float vs = ok[c] ? v_shaped[e0 + tid + SP_VT * c] : 0.f;
#pragma unroll
    for (int f = 0; f < SP_FT; ++f) s_vp[f * (SP_VT * 3) + tid + SP_VT * c] = acc[f][c] + vs;
  }
  __syncthreads();

  // b, c. the lane's own vertex: its three elements from LDS, the blended transform, the product
  const long v = v0 + tid;
  if (v < V) {
    f4 wv[SMPL_J / 4];
#pragma unroll
    for (int q = 0; q < SMPL_J / 4; ++q) wv[q] = weights[v * (SMPL_J / 4) + q];
#pragma unroll 2
    for (int f = 0; f < SP_FT; ++f) {
      f4 M[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) M[r] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < SMPL_J; ++j) {
        const float wj = wv[j >> 2][j & 3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const f4 a = s_A[(f * SMPL_J + j) * 3 + r];
#pragma unroll
          for (int q = 0; q < 4; ++q) M[r][q] = __builtin_fmaf(wj, a[q], M[r][q]);
        }
      }
      float* vp = s_vp + f * (SP_VT * 3) + 3 * tid;             // only this lane reads or writes these three
      const float x = vp[0], y = vp[1], z = vp[2];
#pragma unroll
      for (int r = 0; r < 3; ++r) vp[r] = __builtin_fmaf(M[r][0], x, __builtin_fmaf(M[r][1], y, __builtin_fmaf(M[r][2], z, M[r][3])));
    }
  }
  __syncthreads();

  // d. contiguous stores of the tile's elements
  for (int f = 0; f < nf; ++f) {
    float* o = out + (t0 + f) * E + e0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (ok[c]) o[tid + SP_VT * c] = s_vp[f * (SP_VT * 3) + tid + SP_VT * c];
  }
}

extern "C" int avc_smpl_pose(const float* v_shaped, const float* posedirs, const float* weights, const float* feat, const float* A, int V, int T,
                             float* out, void* stream) {
  if (V < 0 || T < 0) { avc_set_error("avc_smpl_pose: bad sizes"); return 1; }
  if (V == 0 || T == 0) return 0;
  if (!v_shaped || !posedirs || !weights || !feat || !A || !out) { avc_set_error("avc_smpl_pose: NULL buffer"); return 1; }
  if ((((unsigned long long)weights | (unsigned long long)A) & 15ull) ||
      (((unsigned long long)v_shaped | (unsigned long long)posedirs | (unsigned long long)feat | (unsigned long long)out) & 3ull)) {
    avc_set_error("avc_smpl_pose: weights / A not 16-byte or v_shaped / posedirs / feat / out not 4-byte aligned");
    return 1;
  }
  const unsigned gx = (unsigned)(((long)V + SP_VT - 1) / SP_VT);
  for (long t0 = 0; t0 < T; t0 += SP_MAX_FRAMES) {              // a launch's grid takes 65535 frame tiles
    const int n = (int)min((long)SP_MAX_FRAMES, (long)T - t0);
    hipLaunchKernelGGL(smpl_pose_kernel, dim3(gx, (unsigned)((n + SP_FT - 1) / SP_FT)), dim3(SP_VT), 0, (hipStream_t)stream, v_shaped, posedirs,
                       (const f4*)weights, feat + t0 * SMPL_K, (const f4*)(A + t0 * (SMPL_J * 12)), V, n, out + t0 * 3L * V);
  }
  return avc_check_launch("avc_smpl_pose");
}
