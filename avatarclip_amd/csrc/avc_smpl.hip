// Posing the SMPL body without a gradient (avatarclip_amd/smpl_lbs.py pose_hip): what smpl_lbs.lbs computes with about a hundred small torch
// kernels and a [T, V, 4, 4] transform tensor, as two launches.  The reference poses through smplx (AvatarAnimate/visualize.py:98-102,
// :115-119 for its previews).  The arithmetic shared with the gradient (avc_smpl_grad.hip) -- Rodrigues, the chain's rotations, the pose
// blend shapes, the blended transform -- is stated and written once, in avc_smpl.h; below is what the forward alone does.  There is no
// atomic: the result of a frame is the same bits in every run, in every batch and at every place in a batch.
//
// 1. avc_smpl_joint_mats: one lane per frame walks the 24 joints in index order.
//      feat[t, 9 (i - 1) + 3 a + b] = R_i[a][b] - I[a][b], i = 1..23    (lbs's pose_feature)
//      rel_i = j_i - j_parent(i) (rel_0 = j_0);  world_0 = [R_0 | j_0];  world_i.R by smpl_world_rot
//      world_i.t[a]    = ((P.R[a][0] rel_i[0] + P.R[a][1] rel_i[1]) + P.R[a][2] rel_i[2]) + P.t[a]          (P = world of the parent)
//      A_i = [world_i.R | world_i.t - ((W.R[a][0] j_i[0] + W.R[a][1] j_i[1]) + W.R[a][2] j_i[2])]   (batch_rigid_transform's A, rows 0..2)
//    The worlds of a frame stay in LDS, one column per lane ([joint][12][lane]: conflict-free).  A chain of 23 small products per lane:
//    bound by latency, not by throughput.
// 2. avc_smpl_pose: a workgroup owns SMPL_VT = 256 vertices x SMPL_FT = 8 frames.
//    a. pose blend shapes (smpl_blend_shapes): v_posed[e] = acc + v_shaped[e].
//    b. v_posed goes through LDS to the lane that owns the vertex (stride-3 reads: conflict-free).
//    c. blend: M = smpl_blend_transform (3 x 4);  out[t, v][r] = fma(M[r][0], x, fma(M[r][1], y, fma(M[r][2], z, M[r][3]))).
//    d. the results go back through LDS and are stored contiguously.
//    posedirs (17 MB for SMPL) is read ceil(T / 8) times instead of T times; the kernel is bound by that stream (0.5 GFLOP at T = 60).
//    The 256 x 8 tile: 24 accumulators, 27 loads in flight (9 rows: one joint's block of posedirs), then 24 weights + 12 blend sums; the
//    compiler takes 182 registers for it, two workgroups a CU, and LDS is 6.5 KiB (feat) + 9 KiB (A) + 24 KiB (v_posed) = 39.5 KiB, which
//    would admit three.  16 frames would halve the posedirs traffic again but double the accumulators and the LDS, and at T = 60 (27 x 8
//    = 216 tiles for SMPL's 6890 vertices, on 256 CUs) leave half of the CUs without a tile.
#include "avc_smpl.h"
#include "../../include/avc.h"

#define SJ_LANES 32       // frames per workgroup of the joint kernel (24 x 12 x 32 floats of LDS = 36 KiB)

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
    SmplRot o;
    smpl_rodrigues(r[3 * i], r[3 * i + 1], r[3 * i + 2], o);
    if (i > 0) {
      float* f = feat + t * SMPL_K + 9 * (i - 1);
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) f[3 * a + b] = o.R[a][b] - (a == b ? 1.f : 0.f);
    }
    const float jx = s_j[3 * i], jy = s_j[3 * i + 1], jz = s_j[3 * i + 2];
    float W[3][4];
    const int p = s_p[i];
    smpl_world_rot<SJ_LANES, 4>(w, i, p, o.R, W);
    if (i == 0) {
      W[0][3] = jx; W[1][3] = jy; W[2][3] = jz;
    } else if ((unsigned)p < (unsigned)i) {
      const float lx = jx - s_j[3 * p], ly = jy - s_j[3 * p + 1], lz = jz - s_j[3 * p + 2];
      const float* pw = w + 12 * p * SJ_LANES;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float p0 = pw[(4 * a) * SJ_LANES], p1 = pw[(4 * a + 1) * SJ_LANES], p2 = pw[(4 * a + 2) * SJ_LANES], p3 = pw[(4 * a + 3) * SJ_LANES];
        W[a][3] = __builtin_fmaf(p2, lz, __builtin_fmaf(p1, ly, p0 * lx)) + p3;
      }
    } else {
      W[0][3] = W[1][3] = W[2][3] = __uint_as_float(0x7FC00000u);
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
// feat / A / out point at frame t0 of the call; T = the frames of this launch (gridDim.y = ceil(T / SMPL_FT))
__global__ __launch_bounds__(SMPL_VT) void smpl_pose_kernel(const float* __restrict__ v_shaped, const float* __restrict__ posedirs,
                                                            const f4* __restrict__ weights, const float* __restrict__ feat,
                                                            const f4* __restrict__ A, int V, int T, float* __restrict__ out) {
  __shared__ f4 s_feat[SMPL_K * 2];                             // [k][frame of the tile]
  __shared__ f4 s_A[SMPL_FT * SMPL_J * 3];                      // [frame][joint][row]
  __shared__ float s_vp[SMPL_FT * SMPL_VT * 3];                 // [frame][element of the tile]
  const int tid = threadIdx.x;
  const long v0 = (long)blockIdx.x * SMPL_VT;
  const long t0 = (long)blockIdx.y * SMPL_FT;
  const int nf = (int)min((long)SMPL_FT, (long)T - t0);         // frames of this tile that exist (>= 1)
  const long E = 3L * V;                                        // elements of a posedirs row
  const long e0 = 3 * v0;

  smpl_stage_tile(feat, A, t0, nf, s_feat, s_A);
  __syncthreads();

  // a. pose blend shapes of elements e0 + tid + 256 c, c = 0..2
  bool ok[3];
  const float* pd[3];
  smpl_blend_lanes(posedirs, e0, E, ok, pd);
  float acc[SMPL_FT][3];
  smpl_blend_shapes(ok, pd, E, s_feat, acc);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float vs = ok[c] ? v_shaped[e0 + tid + SMPL_VT * c] : 0.f;
#pragma unroll
    for (int f = 0; f < SMPL_FT; ++f) s_vp[f * (SMPL_VT * 3) + tid + SMPL_VT * c] = acc[f][c] + vs;
  }
  __syncthreads();

  // b, c. the lane's own vertex: its three elements from LDS, the blended transform, the product
  const long v = v0 + tid;
  if (v < V) {
    float wv[SMPL_J];
    smpl_vertex_weights(weights, v, wv);
#pragma unroll 2
    for (int f = 0; f < SMPL_FT; ++f) {
      float M[3][4];
      smpl_blend_transform(s_A, f, wv, M);
      float* vp = s_vp + f * (SMPL_VT * 3) + 3 * tid;           // only this lane reads or writes these three
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
      if (ok[c]) o[tid + SMPL_VT * c] = s_vp[f * (SMPL_VT * 3) + tid + SMPL_VT * c];
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
  smpl_split_frames(V, T, [&](dim3 grid, long t0, int n) {
    hipLaunchKernelGGL(smpl_pose_kernel, grid, dim3(SMPL_VT), 0, (hipStream_t)stream, v_shaped, posedirs, (const f4*)weights, feat + t0 * SMPL_K,
                       (const f4*)(A + t0 * (SMPL_J * 12)), V, n, out + t0 * 3L * V);
  });
  return avc_check_launch("avc_smpl_pose");
}
