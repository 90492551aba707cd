/*
 * libavc.so -- the gradient of posing the SMPL body with respect to the pose (avatarclip_amd/smpl_lbs.py pose_hip_grad,
 * csrc/avc_smpl_grad.hip).  A second header beside avc.h, in its style and under its conventions (device pointers, the caller's stream, no
 * synchronisation, 0 = ok and avc_last_error() otherwise); avc.h's AVC_ABI_VERSION does not count these entry points: a library without them
 * is one to rebuild.  avatarclip_amd/lib.py parses this file after avc.h and binds it into the same table.
 *
 * The exact adjoint of avc.h's avc_smpl_joint_mats + avc_smpl_pose, to the POSE only: v_shaped, the rest joints and the SMPL arrays are
 * constants.  fp32, every multiply-add one fused operation in the order csrc/avc_smpl_grad.hip's header states, no atomics: every sum over
 * vertices is a fixed tree that depends on V only, so a frame's gradient is the same bits in every run, every batch and at every place in a
 * batch.  T = 0 (or V = 0) returns 0 without a launch; a NULL or misaligned buffer is an error.  Shapes as in avc.h: v_shaped [V,3], posedirs
 * [207, 3V], weights [V,24] dense, feat [T,207] and A [T,24,12] as avc_smpl_joint_mats wrote them, pose [T,24,3], joints [24,3], parents int32
 * [24] with 0 <= parents[i] < i.
 */
#ifndef AVC_SMPL_GRAD_H
#define AVC_SMPL_GRAD_H
#ifdef __cplusplus
extern "C" {
#endif

/* bytes of avc_smpl_grad_tiles' scratch: ceil(V / 256) vertex tiles x T frames x (24 x 12 + 207) floats */
long avc_smpl_grad_scratch_bytes(int V, int T);

/* The adjoint of lbs's skinning and pose blend shapes (smpl_lbs.py:50-56, lbs: `v_posed = pose_feature posedirs + v_shaped`, `T = W A`,
 * `verts = T (v_posed, 1)`), per tile of 256 vertices x 8 frames.  g [T,V,3] = dL/d out.  v_posed is RECOMPUTED from feat (the forward saves
 * nothing of size [T,V,..]), M = sum_j weights[v,j] A[t,j] rebuilt as avc_smpl_pose does, and
 *   g_vp[t,v] = M.R^T g[t,v]                                               (dL/d v_posed; written to g_vp [T,V,3] unless g_vp is NULL)
 *   dA[t,j]   = sum_v weights[v,j] g[t,v] (x) (v_posed[t,v], 1)             (3 x 4; the tile's vertices in index order)
 *   dfeat[t,k] = sum_e posedirs[k,e] g_vp[t,e]                              (the tile's 768 elements in a fixed butterfly)
 * The tile's dA and dfeat go to scratch [vertex tile][T][24 x 12 + 207] (avc_smpl_grad_scratch_bytes; every float of it is written).
 * weights and A 16-byte aligned.  posedirs is read twice per 8 frames.  Any T: the wrapper splits what one grid does not take. */
int avc_smpl_grad_tiles(const float* v_shaped, const float* posedirs, const float* weights, const float* feat, const float* A, const float* g,
                        int V, int T, float* g_vp, float* scratch, void* stream);

/* The sums over vertices of lbs's two matmuls (smpl_lbs.py:51, :54), finished: dA [T,24,12] (16-byte aligned) and dfeat [T,207] = the vertex tiles'
 * partial sums of avc_smpl_grad_tiles' scratch (same V and T) added in tile order. */
int avc_smpl_grad_reduce(const float* scratch, int V, int T, float* dA, float* dfeat, void* stream);

/* The adjoint of batch_rigid_transform (smpl_lbs.py:25-42), of lbs's `pose_feature = rot_mats[:, 1:] - ident` (:50) and of batch_rodrigues
 * (:11-22, its `+ epsilon` under the norm included), one lane per frame: dA (16-byte aligned) and dfeat as above -> dpose [T,24,3] = dL/d pose.  With W_i the world
 * transform of joint i, q its parent, rel_i = j_i - j_q:  dW_i = [dA_i.R - dA_i.t (x) j_i | dA_i.t];  for i = 23..1:
 * dR_i = W_q.R^T dW_i.R + dfeat[t, 9 (i - 1) .. + 8],  dW_q.R += dW_i.R R_i^T + dW_i.t (x) rel_i,  dW_q.t += dW_i.t;  dR_0 = dW_0.R;  then
 * with e = r + 1e-8, a = |e|, K = skew(r / a):  dK = sin a dR + (1 - cos a)(dR K^T + K^T dR),  dd = (dK21 - dK12, dK02 - dK20, dK10 - dK01),
 * da = <dR, K> cos a + <dR, K^2> sin a - (dd . r) / a^2,  dr = dd / a + da e / a.  Contract: the caller checks the tree; a joint whose parent
 * does not come before it gets NaN and reads nothing. */
int avc_smpl_grad_chain(const float* pose, const float* joints, const int* parents, const float* dA, const float* dfeat, int T, float* dpose,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
