"""Linear blend skinning of the SMPL template (the `my_lbs` of AvatarGen/AppearanceGen/models/utils.py:176-224 and the
smplx.lbs helpers it calls: batch_rodrigues :72-106, vertices2joints, batch_rigid_transform), as plain torch on whatever device
the arrays live on.  The licensed SMPL arrays (v_template, posedirs, J_regressor, parents, lbs_weights, faces) are INPUTS:
`load_smpl_arrays` reads them from an .npz export or from the official pickle."""
import os

import numpy as np
import torch


def batch_rodrigues(rot_vecs: torch.Tensor, epsilon: float = 1e-8) -> torch.Tensor:
    """models/utils.py:72-106: axis-angle [N,3] -> rotation matrices [N,3,3]"""
    n = rot_vecs.shape[0]
    angle = torch.norm(rot_vecs + epsilon, dim=1, keepdim=True, p=2)
    rot_dir = rot_vecs / angle
    cos = torch.unsqueeze(torch.cos(angle), dim=1)
    sin = torch.unsqueeze(torch.sin(angle), dim=1)
    rx, ry, rz = torch.split(rot_dir, 1, dim=1)
    zeros = torch.zeros((n, 1), dtype=rot_vecs.dtype, device=rot_vecs.device)
    K = torch.cat([zeros, -rz, ry, rz, zeros, -rx, -ry, rx, zeros], dim=1).view((n, 3, 3))
    ident = torch.eye(3, dtype=rot_vecs.dtype, device=rot_vecs.device).unsqueeze(dim=0)
    return ident + sin * K + (1 - cos) * torch.bmm(K, K)


def batch_rigid_transform(rot_mats, joints, parents):
    """smplx.lbs.batch_rigid_transform: world transforms of the kinematic chain and their rest-pose-relative form A."""
    B, J = joints.shape[0], joints.shape[1]
    joints = joints.unsqueeze(-1)
    rel = joints.clone()
    rel[:, 1:] = rel[:, 1:] - joints[:, parents[1:]]
    T = torch.zeros(B, J, 4, 4, dtype=rot_mats.dtype, device=rot_mats.device)
    T[:, :, :3, :3] = rot_mats
    T[:, :, :3, 3] = rel[..., 0]
    T[:, :, 3, 3] = 1
    chain = [T[:, 0]]
    for i in range(1, J):
        chain.append(torch.matmul(chain[int(parents[i])], T[:, i]))
    world = torch.stack(chain, dim=1)
    posed_joints = world[:, :, :3, 3]
    jh = torch.cat([joints, torch.zeros(B, J, 1, 1, dtype=joints.dtype, device=joints.device)], dim=2)
    A = world - torch.nn.functional.pad(torch.matmul(world, jh), [3, 0, 0, 0, 0, 0, 0, 0])
    return posed_joints, A


def lbs(v_shaped, rot_mats, posedirs, J_regressor, parents, lbs_weights):
    """models/utils.py:176-224 with pose2rot=False: v_shaped [B,V,3] (shape already applied), rot_mats [B,J,3,3] -> (verts, joints)"""
    B = rot_mats.shape[0]
    J = torch.einsum("bik,ji->bjk", v_shaped, J_regressor)
    ident = torch.eye(3, dtype=rot_mats.dtype, device=rot_mats.device)
    pose_feature = (rot_mats[:, 1:] - ident).reshape(B, -1)
    v_posed = torch.matmul(pose_feature, posedirs).view(B, -1, 3) + v_shaped
    J_transformed, A = batch_rigid_transform(rot_mats, J, parents)
    nj = J_regressor.shape[0]
    T = torch.matmul(lbs_weights.unsqueeze(0).expand(B, -1, -1), A.view(B, nj, 16)).view(B, -1, 4, 4)
    vh = torch.cat([v_posed, torch.ones(B, v_posed.shape[1], 1, dtype=v_posed.dtype, device=v_posed.device)], dim=2)
    verts = torch.matmul(T, vh.unsqueeze(-1))[:, :, :3, 0]
    return verts, J_transformed


def _check_pose_hip(smpl_arrays, pose, v_shaped):
    """the shapes pose_hip's kernels are written for; returns (T, V)"""
    a = smpl_arrays
    for k in ("v_template", "posedirs", "J_regressor", "parents", "lbs_weights"):
        if k not in a:
            raise ValueError("pose_hip: the SMPL arrays lack %r" % k)
    vt, pd, jr, w = a["v_template"], a["posedirs"], a["J_regressor"], a["lbs_weights"]
    parents = [int(p) for p in np.asarray(a["parents"].cpu() if torch.is_tensor(a["parents"]) else a["parents"]).reshape(-1)]
    if vt.dim() != 2 or vt.shape[1] != 3:
        raise ValueError("pose_hip: v_template must be [V, 3], got %s" % (tuple(vt.shape),))
    V = vt.shape[0]
    if len(parents) != 24 or jr.dim() != 2 or jr.shape[0] != 24 or w.dim() != 2 or w.shape[1] != 24:
        raise ValueError("pose_hip poses SMPL's 24 joints, got %d parents, J_regressor %s, lbs_weights %s"
                         % (len(parents), tuple(jr.shape), tuple(w.shape)))
    if jr.shape[1] != V or w.shape[0] != V:
        raise ValueError("pose_hip: J_regressor %s / lbs_weights %s do not fit %d vertices" % (tuple(jr.shape), tuple(w.shape), V))
    if pd.dim() != 2 or pd.shape[0] != 207:
        raise ValueError("pose_hip: posedirs must hold 207 = 23 x 9 pose-blend rows, got %s" % (tuple(pd.shape),))
    if pd.shape[1] != 3 * V:
        raise ValueError("pose_hip: posedirs must be [207, %d], got %s" % (3 * V, tuple(pd.shape)))
    for i in range(1, 24):
        if not 0 <= parents[i] < i:
            raise ValueError("pose_hip: parents[%d] = %d, a parent must come before its child (0 <= parents[i] < i)" % (i, parents[i]))
    if not (pose.dim() == 2 and pose.shape[1] == 72) and not (pose.dim() == 3 and tuple(pose.shape[1:]) == (24, 3)):
        raise ValueError("pose_hip: pose must be [T, 72] or [T, 24, 3] axis-angle, got %s" % (tuple(pose.shape),))
    if v_shaped is not None and tuple(v_shaped.shape) != (V, 3):
        raise ValueError("pose_hip: v_shaped must be [%d, 3], got %s" % (V, tuple(v_shaped.shape)))
    return pose.shape[0], V


def _hip_device(v_template):
    """the arrays' device when they live on one, else the current cuda device"""
    return v_template.device if v_template.is_cuda else torch.device("cuda")


def _pose_hip_operands(smpl_arrays, pose, v_shaped, grad):
    """What pose_hip and pose_hip_grad do before a launch, the checks first (they need no library): the operands of the launches, every one
    a contiguous device tensor, float32 (parents int32): (pose [T,72], v_shaped, rest joints, parents, posedirs, weights).  With `grad` the
    pose is cast and moved by ordinary differentiable torch ops, so its gradient returns the same way."""
    as_t = lambda x: x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    pose = as_t(pose)
    v_shaped = None if v_shaped is None else as_t(v_shaped)
    a = dict(smpl_arrays)
    for k in ("v_template", "posedirs", "J_regressor", "lbs_weights"):
        if k in a:
            a[k] = as_t(a[k])
    T, V = _check_pose_hip(a, pose, v_shaped)
    if grad and v_shaped is not None and v_shaped.requires_grad:
        raise ValueError("pose_hip_grad: v_shaped requires grad, but the gradient goes to the pose only (v_shaped, the rest joints and the "
                         "SMPL arrays are constants); detach it, or pose with smpl_lbs.lbs")
    dev = _hip_device(a["v_template"])
    f32 = lambda x: x.detach().to(device=dev, dtype=torch.float32).contiguous()
    vs = f32(a["v_template"] if v_shaped is None else v_shaped)
    joints = torch.matmul(f32(a["J_regressor"]), vs).contiguous()
    parents = torch.as_tensor(np.asarray(as_t(a["parents"]).cpu()).reshape(-1)).to(device=dev, dtype=torch.int32).contiguous()
    pose_d = (pose if grad else pose.detach()).to(device=dev, dtype=torch.float32).reshape(T, 72).contiguous()
    return pose_d, vs, joints, parents, f32(a["posedirs"]), f32(a["lbs_weights"])


def _pose_hip_launch(pose, vs, joints, parents, posedirs, weights):
    """csrc/avc_smpl.hip's two launches on _pose_hip_operands' operands, into fresh (out [T,V,3], feat [T,207], A [T,24,12]); an empty batch
    launches nothing.  (every operand is an argument, alive to the end: memory a launch reads is not handed back before it is enqueued)"""
    from . import lib as L
    T, V = pose.shape[0], vs.shape[0]
    out, feat, A = (torch.empty(T, *shape, device=pose.device, dtype=torch.float32) for shape in ((V, 3), (207,), (24, 12)))
    if T > 0 and V > 0:
        s = L.stream()
        L.call("avc_smpl_joint_mats", pose, joints, parents, T, feat, A, stream=s)
        L.call("avc_smpl_pose", vs, posedirs, weights, feat, A, V, T, out, stream=s)
    return out, feat, A


def pose_hip(smpl_arrays, pose, v_shaped=None):
    """SMPL vertices float32 [T,V,3] (a device tensor) of axis-angle poses [T,72] or [T,24,3], FORWARD ONLY: two HIP launches
    (csrc/avc_smpl.hip: avc_smpl_joint_mats, avc_smpl_pose) instead of lbs's hundred small kernels, no [T,V,4,4] tensor, no gradient.
    pose_hip_grad is the same with a gradient to the pose; `lbs` remains the default differentiable path, and the one whose arithmetic the
    pinned scores were taken with (the two agree to fp32 rounding, not bit for bit).  v_shaped [V,3] defaults to v_template (betas = 0); the
    rest joints are J_regressor v_shaped, in torch.
    smpl_arrays: load_smpl_arrays' dict.  The device is the arrays' when they live on one, else the current cuda device."""
    return _pose_hip_launch(*_pose_hip_operands(smpl_arrays, pose, v_shaped, grad=False))[0]


class _PoseHipGrad(torch.autograd.Function):
    """pose_hip's two launches, and csrc/avc_smpl_grad.hip's three as their backward; every operand is device float32 (int32), contiguous"""

    @staticmethod
    def forward(ctx, pose, vs, joints, parents, posedirs, weights):
        out, feat, A = _pose_hip_launch(pose, vs, joints, parents, posedirs, weights)
        ctx.save_for_backward(pose, vs, joints, parents, posedirs, weights, feat, A)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        from . import lib as L
        pose, vs, joints, parents, posedirs, weights, feat, A = ctx.saved_tensors
        T, V = pose.shape[0], vs.shape[0]
        dpose = torch.zeros_like(pose)
        if T > 0 and V > 0:
            g = g.to(dtype=torch.float32).contiguous()      # autograd hands over expanded and strided gradients
            scratch = torch.empty(L.load().avc_smpl_grad_scratch_bytes(V, T) // 4, device=pose.device, dtype=torch.float32)
            dA = torch.empty(T, 24, 12, device=pose.device, dtype=torch.float32)
            dfeat = torch.empty(T, 207, device=pose.device, dtype=torch.float32)
            s = L.stream()                                  # torch's current stream, the one the caching allocator frees these buffers on
            L.call("avc_smpl_grad_tiles", vs, posedirs, weights, feat, A, g, V, T, None, scratch, stream=s)
            L.call("avc_smpl_grad_reduce", scratch, V, T, dA, dfeat, stream=s)
            L.call("avc_smpl_grad_chain", pose, joints, parents, dA, dfeat, T, dpose, stream=s)
        return dpose, None, None, None, None, None


def pose_hip_grad(smpl_arrays, pose, v_shaped=None):
    """pose_hip WITH a gradient to the pose: the same checks, the same two launches and the same float32 [T,V,3] bit for bit, returned from
    an autograd.Function whose backward is csrc/avc_smpl_grad.hip (include/avc.h: avc_smpl_grad_tiles, _reduce, _chain, on torch's
    current stream) instead of the few hundred kernels autograd issues behind `lbs`.  The gradient goes to `pose` ONLY, in its own dtype and
    on its own device (the cast and the move are ordinary torch ops outside the Function): v_shaped, the rest joints and the SMPL arrays are
    constants, and a v_shaped that requires grad is refused.  No double backward.  The backward recomputes the blend-shaped vertices per
    tile, so the forward saves nothing of size [T,V,..].  `lbs` remains the default of AnimateContext and the path whose arithmetic the
    pinned scores were taken with: the two agree to fp32 rounding, forward and backward, not bit for bit."""
    return _PoseHipGrad.apply(*_pose_hip_operands(smpl_arrays, pose, v_shaped, grad=True))


def load_smpl_arrays(path, device="cpu"):
    """.npz with the SMPL field names, or the official SMPL_*.pkl (chumpy objects are read through their `.r` array when the
    chumpy package is importable; posedirs is reshaped to [(J-1)*9, V*3] like smplx does)."""
    if path.endswith(".npz"):
        try:
            d = dict(np.load(path, allow_pickle=False))      # plain arrays: nothing from the file is executed
        except ValueError:
            if os.environ.get("AVC_ALLOW_UNSAFE_PICKLE") != "1":
                raise RuntimeError("%s holds pickled objects; loading it would execute code from the file (set AVC_ALLOW_UNSAFE_PICKLE=1 "
                                   "to allow that, or re-save the arrays with np.savez)" % path)
            d = dict(np.load(path, allow_pickle=True))
    else:
        # the official SMPL_*.pkl IS a pickle (of chumpy objects): reading it executes code from the file, as smplx / the reference do
        import logging
        import pickle
        logging.warning("%s is a pickle: loading it executes code from the file (convert it to .npz to avoid that)", path)
        with open(path, "rb") as f:
            d = pickle.load(f, encoding="latin1")
    g = lambda k: np.asarray(d[k].r if hasattr(d[k], "r") else (d[k].todense() if hasattr(d[k], "todense") else d[k]))
    t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(device)
    posedirs = g("posedirs")
    if posedirs.ndim == 3:
        posedirs = posedirs.reshape(-1, posedirs.shape[-1]).T
    parents = np.asarray(g("kintree_table"))[0].astype(np.int64) if "kintree_table" in d else np.asarray(g("parents")).astype(np.int64)
    parents[0] = -1
    return dict(v_template=t(g("v_template")), posedirs=t(posedirs), J_regressor=t(g("J_regressor")), parents=torch.as_tensor(parents),
                lbs_weights=t(g("weights") if "weights" in d else g("lbs_weights")), faces=np.asarray(g("f") if "f" in d else g("faces")).astype(np.int32))
