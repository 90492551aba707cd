"""The gradient of SMPL posing with respect to the pose, restated in numpy float64 from the comments of include/avc.h (its
posing-gradient section, and the posing section for the forward it differentiates), not from the kernels: test infrastructure for tests/test_pose_grad_cpu.py, which checks
it against float64 autograd of smpl_lbs.batch_rodrigues + smpl_lbs.lbs, and for tests/test_gpu_pose_grad.py, which checks every launch of
csrc/avc_smpl_grad.hip against it.  Notation: g = dL/d out [T,V,3]; vp = the blend-shaped vertex; M[t,v] = sum_j w[v,j] A[t,j] (3 x 4)."""
import numpy as np

EPS = 1e-8


def _np(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)


def skew(d):
    """[...,3] -> [...,3,3]"""
    K = np.zeros(d.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2] = -d[..., 2], d[..., 1]
    K[..., 1, 0], K[..., 1, 2] = d[..., 2], -d[..., 0]
    K[..., 2, 0], K[..., 2, 1] = -d[..., 1], d[..., 0]
    return K


def rodrigues(r):
    """batch_rodrigues as written: e = r + 1e-8, a = |e|, d = r / a, R = I + sin a K + (1 - cos a) K^2.  r [...,3] -> R [...,3,3]"""
    a = np.linalg.norm(r + EPS, axis=-1)[..., None, None]
    K = skew(r / a[..., 0])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def rodrigues_adjoint(r, G):
    """dL/dr [...,3] of dL/dR = G [...,3,3]"""
    e = r + EPS
    a = np.linalg.norm(e, axis=-1, keepdims=True)
    K = skew(r / a)
    s, c1 = np.sin(a)[..., None], (1 - np.cos(a))[..., None]
    Kt = np.swapaxes(K, -1, -2)
    ds = (G * K).sum((-1, -2))[..., None]
    dc1 = (G * (K @ K)).sum((-1, -2))[..., None]
    dK = s * G + c1 * (G @ Kt + Kt @ G)
    dd = np.stack([dK[..., 2, 1] - dK[..., 1, 2], dK[..., 0, 2] - dK[..., 2, 0], dK[..., 1, 0] - dK[..., 0, 1]], -1)
    da = ds * np.cos(a) + dc1 * np.sin(a) - (dd * r).sum(-1, keepdims=True) / a ** 2
    return dd / a + da * e / a


def forward(arrays, pose, v_shaped=None):
    """pose [T,24,3] -> dict(out [T,V,3], vp [T,V,3], M [T,V,3,4], feat [T,207], A [T,24,3,4], R [T,24,3,3], W [T,24,3,4], joints [24,3])"""
    pose = _np(pose).reshape(-1, 24, 3)
    T = pose.shape[0]
    vs = _np(arrays["v_template"] if v_shaped is None else v_shaped)
    w, pd = _np(arrays["lbs_weights"]), _np(arrays["posedirs"])
    parents = [int(p) for p in np.asarray(arrays["parents"]).reshape(-1)]
    joints = _np(arrays["J_regressor"]) @ vs
    R = rodrigues(pose)
    feat = (R[:, 1:] - np.eye(3)).reshape(T, 207)
    W = np.zeros((T, 24, 3, 4))
    W[:, 0, :, :3], W[:, 0, :, 3] = R[:, 0], joints[0]
    for i in range(1, 24):
        q = parents[i]
        W[:, i, :, :3] = W[:, q, :, :3] @ R[:, i]
        W[:, i, :, 3] = W[:, q, :, :3] @ (joints[i] - joints[q]) + W[:, q, :, 3]
    A = W.copy()
    A[..., 3] -= np.einsum("tjab,jb->tja", W[..., :3], joints)
    vp = (feat @ pd).reshape(T, -1, 3) + vs
    M = np.einsum("vj,tjab->tvab", w, A)
    out = np.einsum("tvab,tvb->tva", M[..., :3], vp) + M[..., 3]
    return dict(out=out, vp=vp, M=M, feat=feat, A=A, R=R, W=W, joints=joints)


def skin_adjoint(arrays, fwd, g):
    """g [T,V,3] -> (g_vp [T,V,3], dA [T,24,3,4], dfeat [T,207])"""
    g = _np(g)
    w, pd = _np(arrays["lbs_weights"]), _np(arrays["posedirs"])
    T = g.shape[0]
    g_vp = np.einsum("tvab,tva->tvb", fwd["M"][..., :3], g)
    vp1 = np.concatenate([fwd["vp"], np.ones(fwd["vp"].shape[:2] + (1,))], -1)
    dA = np.einsum("vj,tva,tvb->tjab", w, g, vp1)
    dfeat = g_vp.reshape(T, -1) @ pd.T
    return g_vp, dA, dfeat


def chain_adjoint(pose, joints, parents, dA, dfeat):
    """dA [T,24,3,4], dfeat [T,207] -> dpose [T,24,3]"""
    pose, joints, dA, dfeat = _np(pose).reshape(-1, 24, 3), _np(joints), _np(dA).reshape(-1, 24, 3, 4), _np(dfeat)
    parents = [int(p) for p in np.asarray(parents).reshape(-1)]
    T = pose.shape[0]
    R = rodrigues(pose)
    WR = np.zeros((T, 24, 3, 3))
    WR[:, 0] = R[:, 0]
    for i in range(1, 24):
        WR[:, i] = WR[:, parents[i]] @ R[:, i]
    dWR = dA[..., :3] - dA[..., 3][..., :, None] * joints[None, :, None, :]
    dWt = dA[..., 3].copy()
    dR = np.zeros((T, 24, 3, 3))
    for i in range(23, 0, -1):
        q = parents[i]
        dR[:, i] = np.swapaxes(WR[:, q], -1, -2) @ dWR[:, i] + dfeat[:, 9 * (i - 1):9 * i].reshape(T, 3, 3)
        dWR[:, q] += dWR[:, i] @ np.swapaxes(R[:, i], -1, -2) + dWt[:, i][:, :, None] * (joints[i] - joints[q])[None, None, :]
        dWt[:, q] += dWt[:, i]
    dR[:, 0] = dWR[:, 0]
    return rodrigues_adjoint(pose, dR)


def backward(arrays, pose, g, v_shaped=None):
    """dict(dpose [T,24,3], g_vp, dA, dfeat) of the upstream gradient g [T,V,3]"""
    fwd = forward(arrays, pose, v_shaped)
    g_vp, dA, dfeat = skin_adjoint(arrays, fwd, g)
    dpose = chain_adjoint(pose, fwd["joints"], arrays["parents"], dA, dfeat)
    return dict(dpose=dpose, g_vp=g_vp, dA=dA, dfeat=dfeat, out=fwd["out"])
