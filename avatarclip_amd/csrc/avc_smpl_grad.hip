// The gradient of posing the SMPL body with respect to the POSE (avatarclip_amd/smpl_lbs.py pose_hip_grad): the exact adjoint of the two
// launches of csrc/avc_smpl.hip.  What it rebuilds of the forward (Rodrigues, the chain's rotations, the tile's staging, the pose blend
// shapes, the blended transform) it rebuilds by calling the forward's own functions in avc_smpl.h, whose header states that arithmetic.
// v_shaped, the rest joints and the SMPL arrays are constants.  Everything is fp32, every multiply-add below is ONE fused operation written as
// such, there is no atomic: every sum over vertices is a fixed tree that depends on V only, so a frame's gradient is the same bits in every
// run, in every batch and at every place in a batch.
// Notation: g = dL/d out [T,V,3]; vp = the blend-shaped vertex (v_posed); M[t,v] = sum_j w[v,j] A[t,j] (3 x 4); j_i = the rest joints.
//
// 1. avc_smpl_grad_tiles: a workgroup owns SMPL_VT = 256 vertices x SMPL_FT = 8 frames, the forward's tile.
//    a. vp is RECOMPUTED in the tile, by the forward's own loop, smpl_blend_shapes (nothing of [T,V,..] is saved by the forward): the
//       first of the two passes over posedirs.
//    b. the lane that owns a vertex takes its 24 weights into registers and lays its g beside vp in LDS.
//    c. dA[t,j][r][q] = sum_v (w[v,j] g[t,v][r]) (vp[t,v], 1)[q]: a 24 x 256 by 256 x 12 product per frame, with lanes owning OUTPUTS.
//       Lane (frame, joint) -- wavefront w takes frames 2 w and 2 w + 1, one per half, lanes 24..31 of a half idle -- runs over the tile's
//       vertices in index order with 12 accumulators; g and vp are broadcast reads, the weights come from a 64-vertex chunk the owning
//       wavefront lays out in LDS ([vertex][25]: conflict-free both ways).  A vertex past V contributes fma(0, ., acc): nothing.
//    d. the lane that owns a vertex rebuilds M.R by smpl_blend_transform and takes  g_vp[c] = (M[0][c] g[0] + M[1][c] g[1]) + M[2][c] g[2]
//       (lbs's verts = M.R vp + M.t, transposed), which replaces vp in LDS.
//       dfeat[t,k] = sum_e posedirs[k,e] g_vp[t,e], the second pass over posedirs: lane l owns elements l, l + 256, l + 512 of the tile
//       (contiguous loads, as in the forward) and holds their g_vp for the 8 frames.  For SG_KU = 8 rows at a time a lane forms the 64
//       products-of-three (row, frame); a transposing butterfly (6 steps, 63 exchanges: a lane keeps one half of its values and hands the
//       other half to its partner at distance 32, 16, .., 1) leaves lane l of each wavefront with the wavefront's sum of value l; the four
//       wavefronts' sums meet in LDS and are added in wavefront order.
//    The tile's dA [8][24][12] and dfeat [8][207] go to the scratch [vertex tile][T][495]; g_vp [T,V,3] is written only when asked for.
//    LDS: 15.5 KiB (feat | A; the weight chunk later lies over feat) + 2 x 24.1 KiB (vp, g; frames 772 floats apart so that the
//    frames a wavefront reads sit in different banks; later g_vp in element order, then the wavefronts' dfeat sums) = 63.7 KiB: one
//    workgroup a CU, which is what the grid asks for anyway (27 vertex tiles for SMPL).  The tile is the forward's, for its reason
//    (posedirs is streamed twice per 8 frames); SG_KU = 8 is what makes a butterfly of a wavefront; neither is measured against another.
// 2. avc_smpl_grad_reduce: dA[t] and dfeat[t] = the tiles' partial sums added in tile order (one lane per output).
// 3. avc_smpl_grad_chain: one lane per frame, SG_LANES = 16 frames per workgroup (24 x (9 + 12) x 16 floats of LDS = 31.5 KiB).  The lane
//    re-walks the forward chain, keeping every world rotation, and seeds  dW_i.R = dA_i.R - dA_i.t (x) j_i,  dW_i.t = dA_i.t  (the
//    adjoint of A_i = [W_i.R | W_i.t - W_i.R j_i]).  Then for i = 23..1 with parent q (every child of i has been through by then):
//      G = W_q.R^T dW_i.R + reshape(dfeat[t, 9 (i - 1) .. + 8]);   dW_q.R += dW_i.R R_i^T + dW_i.t (x) rel_i;   dW_q.t += dW_i.t
//    and G = dW_0.R for the root.  Rodrigues' adjoint through batch_rodrigues as written (e = r + 1e-8, a = |e|, d = r / a, K = skew(d),
//    s = sin a, c1 = 1 - cos a, R = I + s K + c1 K^2):
//      ds = <G, K>;  dc1 = <G, K^2>;  dK = s G + c1 (G K^T + K^T G);  dd = (dK21 - dK12, dK02 - dK20, dK10 - dK01)
//      da = ds cos a + dc1 sin a - (dd . r) / a^2;   dr = dd / a + da e / a.
#include "avc_smpl.h"
#include "../../include/avc.h"

#define SG_KU 8           // posedirs rows per butterfly (SG_KU x SMPL_FT = the 64 lanes of a wavefront)
#define SG_FS 772         // floats between two frames of a tile in LDS (768 elements + 4: consecutive frames in different banks)
#define SG_WS 25          // floats between two vertices of the weight chunk
#define SG_LANES 16       // frames per workgroup of the chain kernel
#define SG_OUT (SMPL_J * 12 + SMPL_K)         // floats of a frame's partial sums: dA [24][12], then dfeat [207]
#define SG_GROUPS ((SMPL_K + SG_KU - 1) / SG_KU)
#define SG_HEAD (SMPL_K * SMPL_FT + SMPL_FT * SMPL_J * 12)      // feat | A

static_assert(SG_KU * SMPL_FT == 64 && SMPL_VT == 256, "one butterfly value per lane");
static_assert(64 * SG_WS <= SMPL_K * SMPL_FT, "the weight chunk lies over the feat tile");
static_assert(4 * SG_GROUPS * 64 <= 2 * SMPL_FT * SG_FS, "the wavefronts' dfeat sums lie over vp and g");
static_assert((SG_HEAD + 2 * SMPL_FT * SG_FS) * 4 <= 65536 && (SMPL_K * SMPL_FT) % 4 == 0 && SG_HEAD % 4 == 0, "LDS");

// ------------------------------------------------------------------------------------------------------------- skinning and blend shapes
// feat / A / g / g_vp point at frame tbase of the call; T = the frames of this launch, Tall = the frames of the call (the scratch's stride)
__global__ __launch_bounds__(SMPL_VT) void smpl_grad_tiles_kernel(const float* __restrict__ v_shaped, const float* __restrict__ posedirs,
                                                                  const f4* __restrict__ weights, const float* __restrict__ feat,
                                                                  const f4* __restrict__ A, const float* __restrict__ g, int V, int T, long Tall,
                                                                  long tbase, float* __restrict__ g_vp, float* __restrict__ part) {
  __shared__ f4 s_all[(SG_HEAD + 2 * SMPL_FT * SG_FS) / 4];
  float* const s_base = reinterpret_cast<float*>(s_all);
  f4* const s_feat = s_all;                                     // [k][frame of the tile]
  f4* const s_A = s_all + SMPL_K * SMPL_FT / 4;                 // [frame][joint][row]
  float* const s_wc = s_base;                                   // [vertex of the chunk][SG_WS]   (over feat, once a. is done)
  float* const s_vp = s_base + SG_HEAD;                         // [frame][element of the tile], frames SG_FS apart
  float* const s_g = s_vp + SMPL_FT * SG_FS;                    // the same for g
  float* const s_red = s_vp;                                    // [wavefront][k][frame]          (over vp and g, once c. is done)
  const int tid = threadIdx.x;
  const long v0 = (long)blockIdx.x * SMPL_VT;
  const long t0 = (long)blockIdx.y * SMPL_FT;
  const int nf = (int)min((long)SMPL_FT, (long)T - t0);         // frames of this tile that exist (>= 1)
  const long E = 3L * V;                                        // elements of a posedirs row
  const long e0 = 3 * v0;

  smpl_stage_tile(feat, A, t0, nf, s_feat, s_A);
  __syncthreads();

  // a. vp of elements e0 + tid + 256 c, c = 0..2: the forward's loop
  bool ok[3];
  const float* pd[3];
  smpl_blend_lanes(posedirs, e0, E, ok, pd);
  {
    float acc[SMPL_FT][3];
    smpl_blend_shapes(ok, pd, E, s_feat, acc);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float vs = ok[c] ? v_shaped[e0 + tid + SMPL_VT * c] : 0.f;
#pragma unroll
      for (int f = 0; f < SMPL_FT; ++f) s_vp[f * SG_FS + tid + SMPL_VT * c] = acc[f][c] + vs;      // (an element past the end: 0)
    }
  }

  // b. the lane's own vertex: its weights into registers, its g into LDS
  const long v = v0 + tid;
  float wv[SMPL_J];
  if (v < V) {
    smpl_vertex_weights(weights, v, wv);
  } else {
#pragma unroll
    for (int j = 0; j < SMPL_J; ++j) wv[j] = 0.f;
  }
  for (int f = 0; f < SMPL_FT; ++f) {
    const bool live = v < V && f < nf;
#pragma unroll
    for (int r = 0; r < 3; ++r) s_g[f * SG_FS + 3 * tid + r] = live ? g[(t0 + f) * E + 3 * v + r] : 0.f;
  }

  // c. dA of (frame fa, joint ja): the tile's vertices in index order, 64 at a time
  const int wave = tid >> 6, lane = tid & 63;
  const int fa = 2 * wave + (lane >> 5), ja = lane & 31;
  const bool act = ja < SMPL_J;
  float dacc[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) dacc[i] = 0.f;
  for (int c = 0; c < SMPL_VT / 64; ++c) {
    __syncthreads();                                            // vp, g (and the previous chunk's readers) are through
    if (wave == c) {
#pragma unroll
      for (int j = 0; j < SMPL_J; ++j) s_wc[lane * SG_WS + j] = wv[j];
    }
    __syncthreads();
    if (act) {
      const float* gp = s_g + fa * SG_FS + 3 * 64 * c;
      const float* xp = s_vp + fa * SG_FS + 3 * 64 * c;
#pragma unroll 4
      for (int u = 0; u < 64; ++u) {
        const float w = s_wc[u * SG_WS + ja];
        const float x = xp[3 * u], y = xp[3 * u + 1], z = xp[3 * u + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const float gr = gp[3 * u + r], wg = w * gr;
          dacc[4 * r] = __builtin_fmaf(wg, x, dacc[4 * r]);
          dacc[4 * r + 1] = __builtin_fmaf(wg, y, dacc[4 * r + 1]);
          dacc[4 * r + 2] = __builtin_fmaf(wg, z, dacc[4 * r + 2]);
          dacc[4 * r + 3] = __builtin_fmaf(w, gr, dacc[4 * r + 3]);
        }
      }
    }
  }
  if (act && fa < nf) {
    float* o = part + ((long)blockIdx.x * Tall + tbase + t0 + fa) * SG_OUT + 12 * ja;
#pragma unroll
    for (int i = 0; i < 12; ++i) o[i] = dacc[i];
  }
  __syncthreads();                                              // everybody has read vp and g

  // d. g_vp = M.R^T g with M as the forward blends it, through LDS into element order, then dfeat
#pragma unroll 2
  for (int f = 0; f < SMPL_FT; ++f) {
    float M[3][3];
    smpl_blend_transform(s_A, f, wv, M);
    const float* gp = s_g + f * SG_FS + 3 * tid;               // only this lane reads or writes these three of g and of vp
    const float g0 = gp[0], g1 = gp[1], g2 = gp[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) s_vp[f * SG_FS + 3 * tid + c] = __builtin_fmaf(M[2][c], g2, __builtin_fmaf(M[1][c], g1, M[0][c] * g0));
  }
  __syncthreads();
  float gv[SMPL_FT][3];
#pragma unroll
  for (int f = 0; f < SMPL_FT; ++f)
#pragma unroll
    for (int c = 0; c < 3; ++c) gv[f][c] = s_vp[f * SG_FS + tid + SMPL_VT * c];
  if (g_vp) {
    for (int f = 0; f < nf; ++f) {
      float* o = g_vp + (t0 + f) * E + e0;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (ok[c]) o[tid + SMPL_VT * c] = gv[f][c];
    }
  }
  __syncthreads();                                              // s_red lies over what was just read
  for (int grp = 0; grp < SG_GROUPS; ++grp) {
    const int k0 = grp * SG_KU;
    float p[SG_KU][3];
#pragma unroll
    for (int u = 0; u < SG_KU; ++u)
#pragma unroll
      for (int c = 0; c < 3; ++c) p[u][c] = (ok[c] && k0 + u < SMPL_K) ? pd[c][(k0 + u) * E] : 0.f;
    float val[SG_KU * SMPL_FT];
#pragma unroll
    for (int u = 0; u < SG_KU; ++u)
#pragma unroll
      for (int f = 0; f < SMPL_FT; ++f)
        val[u * SMPL_FT + f] = __builtin_fmaf(p[u][2], gv[f][2], __builtin_fmaf(p[u][1], gv[f][1], p[u][0] * gv[f][0]));
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const bool up = (lane & s) != 0;
#pragma unroll
      for (int i = 0; i < s; ++i) {
        const float keep = up ? val[i + s] : val[i];
        const float send = up ? val[i] : val[i + s];
        val[i] = keep + __shfl_xor(send, s);
      }
    }
    s_red[(wave * SG_GROUPS + grp) * 64 + lane] = val[0];        // value lane = 8 (k - k0) + frame: [wavefront][k][frame]
  }
  __syncthreads();
  for (int i = tid; i < SMPL_K * SMPL_FT; i += SMPL_VT) {
    const int k = i / SMPL_FT, f = i - k * SMPL_FT;
    if (f < nf) {
      const float sum = ((s_red[i] + s_red[SG_GROUPS * 64 + i]) + s_red[2 * SG_GROUPS * 64 + i]) + s_red[3 * SG_GROUPS * 64 + i];
      part[((long)blockIdx.x * Tall + tbase + t0 + f) * SG_OUT + SMPL_J * 12 + k] = sum;
    }
  }
}

extern "C" long avc_smpl_grad_scratch_bytes(int V, int T) {
  if (V <= 0 || T <= 0) return 0;
  return smpl_vertex_tiles(V) * (long)T * SG_OUT * (long)sizeof(float);
}

extern "C" int avc_smpl_grad_tiles(const float* v_shaped, const float* posedirs, const float* weights, const float* feat, const float* A,
                                   const float* g, int V, int T, float* g_vp, float* scratch, void* stream) {
  if (V < 0 || T < 0) { avc_set_error("avc_smpl_grad_tiles: bad sizes"); return 1; }
  if (V == 0 || T == 0) return 0;
  if (!v_shaped || !posedirs || !weights || !feat || !A || !g || !scratch) { avc_set_error("avc_smpl_grad_tiles: NULL buffer"); return 1; }
  if ((((unsigned long long)weights | (unsigned long long)A) & 15ull) ||
      (((unsigned long long)v_shaped | (unsigned long long)posedirs | (unsigned long long)feat | (unsigned long long)g | (unsigned long long)g_vp |
        (unsigned long long)scratch) & 3ull)) {
    avc_set_error("avc_smpl_grad_tiles: weights / A not 16-byte or v_shaped / posedirs / feat / g / g_vp / scratch not 4-byte aligned");
    return 1;
  }
  smpl_split_frames(V, T, [&](dim3 grid, long t0, int n) {
    hipLaunchKernelGGL(smpl_grad_tiles_kernel, grid, dim3(SMPL_VT), 0, (hipStream_t)stream, v_shaped, posedirs, (const f4*)weights,
                       feat + t0 * SMPL_K, (const f4*)(A + t0 * (SMPL_J * 12)), g + t0 * 3L * V, V, n, (long)T, t0,
                       g_vp ? g_vp + t0 * 3L * V : (float*)nullptr, scratch);
  });
  return avc_check_launch("avc_smpl_grad_tiles");
}

// ------------------------------------------------------------------------------------------------------------- the tiles' sums, in tile order
__global__ __launch_bounds__(256) void smpl_grad_reduce_kernel(const float* __restrict__ part, int tiles, long T, float* __restrict__ dA,
                                                               float* __restrict__ dfeat) {
  const long t = blockIdx.x;
  for (int o = threadIdx.x; o < SG_OUT; o += 256) {
    float acc = part[t * SG_OUT + o];
    for (int b = 1; b < tiles; ++b) acc = acc + part[((long)b * T + t) * SG_OUT + o];
    if (o < SMPL_J * 12) dA[t * (SMPL_J * 12) + o] = acc;
    else dfeat[t * SMPL_K + (o - SMPL_J * 12)] = acc;
  }
}

extern "C" int avc_smpl_grad_reduce(const float* scratch, int V, int T, float* dA, float* dfeat, void* stream) {
  if (V < 0 || T < 0) { avc_set_error("avc_smpl_grad_reduce: bad sizes"); return 1; }
  if (V == 0 || T == 0) return 0;
  if (!scratch || !dA || !dfeat) { avc_set_error("avc_smpl_grad_reduce: NULL buffer"); return 1; }
  if (((unsigned long long)dA & 15ull) || (((unsigned long long)scratch | (unsigned long long)dfeat) & 3ull)) {
    avc_set_error("avc_smpl_grad_reduce: dA not 16-byte or scratch / dfeat not 4-byte aligned");
    return 1;
  }
  hipLaunchKernelGGL(smpl_grad_reduce_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, scratch, (int)smpl_vertex_tiles(V), (long)T, dA, dfeat);
  return avc_check_launch("avc_smpl_grad_reduce");
}

// ------------------------------------------------------------------------------------------------------------- joint chain and Rodrigues
// G = dL/dR -> dL/dr, o = smpl_rodrigues of r
__device__ __forceinline__ void sg_rodrigues_adjoint(const SmplRot& o, const float (&G)[3][3], float rx, float ry, float rz, float* dr) {
  float ds = 0.f, dc1 = 0.f, dK[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const float k2 = __builtin_fmaf(o.K[a][2], o.K[2][b], __builtin_fmaf(o.K[a][1], o.K[1][b], o.K[a][0] * o.K[0][b]));
      ds = __builtin_fmaf(G[a][b], o.K[a][b], ds);
      dc1 = __builtin_fmaf(G[a][b], k2, dc1);
      const float gkt = __builtin_fmaf(G[a][2], o.K[b][2], __builtin_fmaf(G[a][1], o.K[b][1], G[a][0] * o.K[b][0]));
      const float ktg = __builtin_fmaf(o.K[2][a], G[2][b], __builtin_fmaf(o.K[1][a], G[1][b], o.K[0][a] * G[0][b]));
      dK[a][b] = __builtin_fmaf(o.c1, gkt + ktg, o.s * G[a][b]);
    }
  const float ddx = dK[2][1] - dK[1][2], ddy = dK[0][2] - dK[2][0], ddz = dK[1][0] - dK[0][1];
  const float dot = __builtin_fmaf(ddz, rz, __builtin_fmaf(ddy, ry, ddx * rx));
  const float da = __builtin_fmaf(dc1, o.s, ds * o.c) - dot / (o.angle * o.angle);
  const float k = da / o.angle;
  dr[0] = __builtin_fmaf(k, rx + 1e-8f, ddx / o.angle);
  dr[1] = __builtin_fmaf(k, ry + 1e-8f, ddy / o.angle);
  dr[2] = __builtin_fmaf(k, rz + 1e-8f, ddz / o.angle);
}

__global__ __launch_bounds__(SG_LANES) void smpl_grad_chain_kernel(const float* __restrict__ pose, const float* __restrict__ joints,
                                                                   const int* __restrict__ parents, const f4* __restrict__ dA,
                                                                   const float* __restrict__ dfeat, int T, float* __restrict__ dpose) {
  __shared__ float s_r[SMPL_J * 9 * SG_LANES];                  // [joint][element of world_i.R][lane]
  __shared__ float s_d[SMPL_J * 12 * SG_LANES];                 // [joint][element of dW_i, rows [R | t]][lane]
  __shared__ float s_j[SMPL_J * 3];
  __shared__ int s_p[SMPL_J];
  const int lane = threadIdx.x;
  for (int i = lane; i < SMPL_J * 3; i += SG_LANES) s_j[i] = joints[i];
  for (int i = lane; i < SMPL_J; i += SG_LANES) s_p[i] = parents[i];
  __syncthreads();                                              // the only barrier: lanes past the end may leave now
  const long t = (long)blockIdx.x * SG_LANES + lane;
  if (t >= T) return;
  const float* r = pose + t * (SMPL_J * 3);
  float* wr = s_r + lane;
  float* wd = s_d + lane;
  // the forward chain (rotations only) and the seeds of dW
  for (int i = 0; i < SMPL_J; ++i) {
    SmplRot o;
    smpl_rodrigues(r[3 * i], r[3 * i + 1], r[3 * i + 2], o);
    float W[3][3];
    smpl_world_rot<SG_LANES, 3>(wr, i, s_p[i], o.R, W);
    const float jx = s_j[3 * i], jy = s_j[3 * i + 1], jz = s_j[3 * i + 2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int b = 0; b < 3; ++b) wr[(9 * i + 3 * a + b) * SG_LANES] = W[a][b];
      const f4 d = dA[(t * SMPL_J + i) * 3 + a];
      wd[(12 * i + 4 * a) * SG_LANES] = __builtin_fmaf(-d[3], jx, d[0]);
      wd[(12 * i + 4 * a + 1) * SG_LANES] = __builtin_fmaf(-d[3], jy, d[1]);
      wd[(12 * i + 4 * a + 2) * SG_LANES] = __builtin_fmaf(-d[3], jz, d[2]);
      wd[(12 * i + 4 * a + 3) * SG_LANES] = d[3];
    }
  }
  // back along the chain
  for (int i = SMPL_J - 1; i >= 0; --i) {
    const float rx = r[3 * i], ry = r[3 * i + 1], rz = r[3 * i + 2];
    SmplRot o;
    smpl_rodrigues(rx, ry, rz, o);
    float D[3][4], G[3][3];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) D[a][b] = wd[(12 * i + 4 * a + b) * SG_LANES];
    const int p = s_p[i];
    if (i == 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) { G[a][0] = D[a][0]; G[a][1] = D[a][1]; G[a][2] = D[a][2]; }
    } else if ((unsigned)p < (unsigned)i) {
      const float* pw = wr + 9 * p * SG_LANES;
      const float* f = dfeat + t * SMPL_K + 9 * (i - 1);
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b)
          G[a][b] = __builtin_fmaf(pw[(6 + a) * SG_LANES], D[2][b], __builtin_fmaf(pw[(3 + a) * SG_LANES], D[1][b], pw[a * SG_LANES] * D[0][b])) + f[3 * a + b];
      const float lx = s_j[3 * i] - s_j[3 * p], ly = s_j[3 * i + 1] - s_j[3 * p + 1], lz = s_j[3 * i + 2] - s_j[3 * p + 2];
      const float l[3] = {lx, ly, lz};
      float* pd = wd + 12 * p * SG_LANES;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          const float add = __builtin_fmaf(D[a][3], l[b], __builtin_fmaf(D[a][2], o.R[b][2], __builtin_fmaf(D[a][1], o.R[b][1], D[a][0] * o.R[b][0])));
          pd[(4 * a + b) * SG_LANES] += add;
        }
        pd[(4 * a + 3) * SG_LANES] += D[a][3];
      }
    } else {
#pragma unroll
      for (int a = 0; a < 3; ++a) G[a][0] = G[a][1] = G[a][2] = __uint_as_float(0x7FC00000u);
    }
    sg_rodrigues_adjoint(o, G, rx, ry, rz, dpose + t * (SMPL_J * 3) + 3 * i);
  }
}

extern "C" int avc_smpl_grad_chain(const float* pose, const float* joints, const int* parents, const float* dA, const float* dfeat, int T,
                                   float* dpose, void* stream) {
  if (T < 0) { avc_set_error("avc_smpl_grad_chain: bad sizes"); return 1; }
  if (T == 0) return 0;
  if (!pose || !joints || !parents || !dA || !dfeat || !dpose) { avc_set_error("avc_smpl_grad_chain: NULL buffer"); return 1; }
  if (((unsigned long long)dA & 15ull) || (((unsigned long long)pose | (unsigned long long)joints | (unsigned long long)parents |
                                            (unsigned long long)dfeat | (unsigned long long)dpose) & 3ull)) {
    avc_set_error("avc_smpl_grad_chain: dA not 16-byte or pose / joints / parents / dfeat / dpose not 4-byte aligned");
    return 1;
  }
  hipLaunchKernelGGL(smpl_grad_chain_kernel, dim3((unsigned)(((long)T + SG_LANES - 1) / SG_LANES)), dim3(SG_LANES), 0, (hipStream_t)stream, pose,
                     joints, parents, (const f4*)dA, dfeat, T, dpose);
  return avc_check_launch("avc_smpl_grad_chain");
}
