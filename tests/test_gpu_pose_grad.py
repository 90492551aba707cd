"""smpl_lbs.pose_hip_grad and the launches of csrc/avc_smpl_grad.hip (include/avc.h) on the device: the forward bit for bit
against pose_hip, the gradient against float64 autograd of smpl_lbs's own torch functions from the same float32 inputs, every launch on its
own against the numpy restatement (tests/smpl_grad_restatement.py), the bitwise properties, the gradients autograd really sends, and the
switch of AnimateContext.  Stand-ins, poses and bound are test_gpu_pose_preview's: V and T sit on the edges of the 256 x 8 tile and of the
chain kernel's workgroup; BOUND = 1e-5 of a frame's largest entry (fp32 torch autograd of the same chain stays within 6.8e-7)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import animate_clip_standins as AS
from tests import smpl_grad_restatement as R
from tests.test_gpu_pose_preview import BOUND, DEV, VS, _poses, _template, _template_dev

pytestmark = pytest.mark.gpu
TS = (1, 2, 7, 8, 9, 17, 33)
T_ALL = 33


@functools.lru_cache(maxsize=None)
def _upstream(V):
    """the seeded normal dL/d out of all 33 frames, float32 on the CPU"""
    return torch.from_numpy(np.random.RandomState(100 + V).randn(T_ALL, V, 3).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _reference(V):
    """float64 autograd of batch_rodrigues + lbs from the float32 inputs, all 33 frames under _upstream(V): computed once per V, shared,
    never written to.  The frames are independent, so the first T rows are the reference of a batch of T."""
    from avatarclip_amd import smpl_lbs
    a, pose = _template(V), _poses().double().requires_grad_(True)
    rot = smpl_lbs.batch_rodrigues(pose.reshape(-1, 3)).reshape(T_ALL, 24, 3, 3)
    d = lambda x: x.double()
    v, _ = smpl_lbs.lbs(d(a["v_template"])[None].expand(T_ALL, -1, -1), rot, d(a["posedirs"]), d(a["J_regressor"]), a["parents"], d(a["lbs_weights"]))
    v.backward(_upstream(V).double())
    return pose.grad.detach()


def _ratio(got, want):
    """worst over the frames of max |got - want| / the frame's largest |want|; got: a device or CPU tensor, want: float64"""
    got = got.detach().cpu().double().reshape(want.shape[0], -1)
    want = torch.as_tensor(want).double().reshape(want.shape[0], -1)
    assert torch.isfinite(got).all()
    scale = want.abs().max(1).values
    assert (scale > 0).all()
    return float(((got - want).abs().max(1).values / scale).max())


@pytest.mark.parametrize("V", VS)
def test_forward_is_pose_hip_bit_for_bit_and_the_gradient_matches_float64(V):
    from avatarclip_amd import smpl_lbs
    a, ref, g = _template_dev(V), _reference(V), _upstream(V).to(DEV)
    worst = 0.0
    for T in TS:
        pose = _poses()[:T].to(DEV).requires_grad_(True)
        out = smpl_lbs.pose_hip_grad(a, pose)
        assert out.shape == (T, V, 3) and out.dtype == torch.float32 and out.is_cuda and out.requires_grad
        assert torch.equal(out.detach(), smpl_lbs.pose_hip(a, pose.detach()))
        out.backward(g[:T])
        assert pose.grad.shape == (T, 24, 3) and pose.grad.dtype == torch.float32 and pose.grad.is_cuda
        assert torch.isfinite(pose.grad).all()                                                # the all-zero frame and the 1e-9 joint included
        worst = max(worst, _ratio(pose.grad, ref[:T]))
    print("pose_hip_grad V = %d: worst |dpose - fp64 autograd| / frame's largest entry over T in %s = %.3e" % (V, TS, worst))
    assert worst <= BOUND


@pytest.mark.parametrize("V,T", ((1, 1), (65, 2), (256, 8), (257, 9), (700, 33)))
def test_each_launch_on_its_own_against_the_restatement(V, T):
    from avatarclip_amd import lib as L
    a, ad, pose = _template(V), _template_dev(V), _poses()[:T].contiguous()
    nan = lambda *shape: torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)
    g = _upstream(V)[:T].contiguous()
    joints = torch.matmul(a["J_regressor"], a["v_template"])                                  # fp32: what the kernels are handed
    pose_d, joints_d, parents_d, g_d = pose.to(DEV), joints.to(DEV), a["parents"].to(device=DEV, dtype=torch.int32), g.to(DEV)
    feat, A = nan(T, 207), nan(T, 24, 12)
    L.call("avc_smpl_joint_mats", pose_d, joints_d, parents_d, T, feat, A)
    nbytes = L.load().avc_smpl_grad_scratch_bytes(V, T)
    assert nbytes == -(-V // 256) * T * 495 * 4
    scratch, g_vp, dA, dfeat = nan(nbytes // 4), nan(T, V, 3), nan(T, 24, 12), nan(T, 207)
    L.call("avc_smpl_grad_tiles", ad["v_template"], ad["posedirs"], ad["lbs_weights"], feat, A, g_d, V, T, g_vp, scratch)
    L.call("avc_smpl_grad_reduce", scratch, V, T, dA, dfeat)
    torch.cuda.synchronize()
    assert torch.isfinite(scratch).all()                                                      # every float of the scratch is written
    fwd = R.forward(a, pose)
    r_gvp, r_dA, r_dfeat = R.skin_adjoint(a, fwd, g)
    e = dict(g_vp=_ratio(g_vp, r_gvp), dA=_ratio(dA, r_dA), dfeat=_ratio(dfeat, r_dfeat))
    # the same launch without the optional output leaves the same sums
    scratch2 = nan(nbytes // 4)
    L.call("avc_smpl_grad_tiles", ad["v_template"], ad["posedirs"], ad["lbs_weights"], feat, A, g_d, V, T, None, scratch2)
    assert torch.equal(scratch2, scratch)
    # the chain on a dA and a dfeat of its own
    rs = np.random.RandomState(7 * V + T)
    dA_r = torch.from_numpy(rs.randn(T, 24, 12).astype(np.float32))
    dfeat_r = torch.from_numpy(rs.randn(T, 207).astype(np.float32))
    dA_rd, dfeat_rd, dpose = dA_r.to(DEV), dfeat_r.to(DEV), nan(T, 24, 3)
    L.call("avc_smpl_grad_chain", pose_d, joints_d, parents_d, dA_rd, dfeat_rd, T, dpose)
    torch.cuda.synchronize()
    e["dpose"] = _ratio(dpose, R.chain_adjoint(pose, joints, a["parents"], dA_r, dfeat_r))
    print("V = %d, T = %d: worst error / frame's largest entry: %s" % (V, T, ", ".join("%s %.3e" % kv for kv in e.items())))
    assert max(e.values()) <= BOUND


def test_refused_and_empty_arguments_launch_nothing():
    from avatarclip_amd import lib as L
    lib, s = L.load(), L.stream()
    buf = torch.zeros(1024, device=DEV)
    p = buf.data_ptr()
    assert lib.avc_smpl_grad_scratch_bytes(0, 5) == 0 and lib.avc_smpl_grad_scratch_bytes(5, 0) == 0
    assert lib.avc_smpl_grad_tiles(None, None, None, None, None, None, 0, 3, None, None, s) == 0
    assert lib.avc_smpl_grad_tiles(None, None, None, None, None, None, 3, 0, None, None, s) == 0
    assert lib.avc_smpl_grad_reduce(None, 0, 3, None, None, s) == 0 and lib.avc_smpl_grad_reduce(None, 3, 0, None, None, s) == 0
    assert lib.avc_smpl_grad_chain(None, None, None, None, None, 0, None, s) == 0
    assert lib.avc_smpl_grad_tiles(p, p, p, p, p, None, 1, 1, None, p, s) == 1 and b"NULL" in lib.avc_last_error()
    assert lib.avc_smpl_grad_tiles(p, p, p + 4, p, p, p, 1, 1, None, p, s) == 1 and b"aligned" in lib.avc_last_error()
    assert lib.avc_smpl_grad_tiles(p, p, p, p, p, p, -1, 1, None, p, s) == 1 and b"sizes" in lib.avc_last_error()
    assert lib.avc_smpl_grad_reduce(p, 1, 1, None, p, s) == 1 and b"NULL" in lib.avc_last_error()
    assert lib.avc_smpl_grad_reduce(p, 1, 1, p + 4, p, s) == 1 and b"aligned" in lib.avc_last_error()
    assert lib.avc_smpl_grad_chain(p, p, p, p, None, 1, p, s) == 1 and b"NULL" in lib.avc_last_error()
    assert lib.avc_smpl_grad_chain(p, p, p, p + 8, p, 1, p, s) == 1 and b"aligned" in lib.avc_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf, torch.zeros_like(buf))


def _grad(a, pose, g):
    from avatarclip_amd import smpl_lbs
    pose = pose.detach().clone().requires_grad_(True)
    smpl_lbs.pose_hip_grad(a, pose).backward(g)
    return pose.grad


def test_two_runs_agree_and_a_batch_equals_its_single_frames():
    a, pose, g = _template_dev(700), _poses()[:17].to(DEV), _upstream(700)[:17].to(DEV)
    batch = _grad(a, pose, g)
    assert torch.equal(batch, _grad(a, pose, g))                                              # determinism: bit-identical
    for t in range(17):
        assert torch.equal(_grad(a, pose[t:t + 1], g[t:t + 1])[0], batch[t]), t
    assert torch.equal(_grad(a, pose.reshape(17, 72), g).reshape(17, 24, 3), batch)           # [T,72] and [T,24,3] are one thing


def test_upstream_gradients_as_autograd_sends_them():
    from avatarclip_amd import smpl_lbs
    V, T = 257, 9
    a, pose = _template_dev(V), _poses()[:T].to(DEV)
    # v.sum(): an expanded gradient (every stride 0)
    p = pose.clone().requires_grad_(True)
    smpl_lbs.pose_hip_grad(a, p).sum().backward()
    assert torch.equal(p.grad, _grad(a, pose, torch.ones(T, V, 3, device=DEV)))
    # v[:, ::2].square().sum(): a gradient that is zero at every other vertex, handed over as autograd builds it
    p = pose.clone().requires_grad_(True)
    v = smpl_lbs.pose_hip_grad(a, p)
    v[:, ::2].square().sum().backward()
    g = torch.zeros(T, V, 3, device=DEV)
    g[:, ::2] = 2 * v.detach()[:, ::2]
    assert torch.equal(p.grad, _grad(a, pose, g))
    # a float64 CPU leaf gets a float64 CPU gradient, the float32 one widened
    leaf = _poses()[:T].double().requires_grad_(True)
    out = smpl_lbs.pose_hip_grad(a, leaf)
    assert out.dtype == torch.float32 and out.is_cuda
    out.backward(_upstream(V)[:T].to(DEV))
    assert leaf.grad.dtype == torch.float64 and leaf.grad.device.type == "cpu" and leaf.grad.shape == (T, 24, 3)
    assert torch.equal(leaf.grad, _grad(a, pose, _upstream(V)[:T].to(DEV)).cpu().double())
    # a v_shaped of its own is a constant of the gradient too
    vs = (_template(V)["v_template"] * 1.1).to(DEV)
    p = pose.clone().requires_grad_(True)
    out_s = smpl_lbs.pose_hip_grad(a, p, v_shaped=vs)
    assert torch.equal(out_s.detach(), smpl_lbs.pose_hip(a, pose, v_shaped=vs))
    out_s.backward(_upstream(V)[:T].to(DEV))
    assert torch.isfinite(p.grad).all() and not torch.equal(p.grad, _grad(a, pose, _upstream(V)[:T].to(DEV)))
    # no double backward: the gradient of a gradient that itself carries a graph raises, one of a constant upstream gradient has no graph at all
    p = pose.clone().requires_grad_(True)
    up = torch.ones(T, V, 3, device=DEV, requires_grad=True)
    (gp,) = torch.autograd.grad(smpl_lbs.pose_hip_grad(a, p), p, grad_outputs=up, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gp.sum().backward()
    (gp,) = torch.autograd.grad(smpl_lbs.pose_hip_grad(a, p).sum(), p, create_graph=True)
    assert not gp.requires_grad


def test_empty_batch(monkeypatch):
    from avatarclip_amd import lib as L
    from avatarclip_amd import smpl_lbs
    a = _template_dev(257)
    L.load()
    calls = []
    real = L.call
    monkeypatch.setattr(L, "call", lambda name, *args, **kw: (calls.append(name), real(name, *args, **kw))[1])
    pose = torch.zeros(0, 24, 3, device=DEV, requires_grad=True)
    out = smpl_lbs.pose_hip_grad(a, pose)
    assert out.shape == (0, 257, 3) and out.requires_grad
    out.sum().backward()
    assert pose.grad is not None and pose.grad.shape == (0, 24, 3)
    assert calls == []                                                                        # neither way launched anything
    smpl_lbs.pose_hip_grad(a, torch.zeros(1, 72, device=DEV, requires_grad=True)).sum().backward()
    assert calls == ["avc_smpl_joint_mats", "avc_smpl_pose", "avc_smpl_grad_tiles", "avc_smpl_grad_reduce", "avc_smpl_grad_chain"]


# --------------------------------------------------------------------------------------------------- through AnimateContext
NV, RES = AS.NV, AS.RES


def _device_standins():
    """animate_clip_standins' body with pose blend shapes of its own, its smooth render (sigmoid of a fixed linear map of the vertices; the
    elevations drawn from numpy's generator in its order) and its linear perceptor, with their weights on the device"""
    import math
    smpl = {k: (x.to(DEV) if torch.is_tensor(x) and k != "parents" else x) for k, x in AS.smpl_arrays().items()}
    smpl["posedirs"] = torch.from_numpy((np.random.RandomState(5).randn(207, 3 * NV) * 0.02).astype(np.float32)).to(DEV)
    W = torch.from_numpy(np.random.RandomState(7).randn(RES * RES, 3 * NV).astype(np.float32) * 0.4).to(DEV)

    def render(vertices, faces, angles):
        elev = [np.random.randn() * 0.3 for _ in angles]
        out = []
        for ang, e in zip(angles, elev):
            az, el = math.radians(ang), math.radians(e)
            ca, sa, ce, se = math.cos(az), math.sin(az), math.cos(el), math.sin(el)
            rot = torch.tensor([[ca, 0.0, sa], [0.0, 1.0, 0.0], [-sa, 0.0, ca]]) @ torch.tensor([[1.0, 0.0, 0.0], [0.0, ce, -se], [0.0, se, ce]])
            v = vertices @ rot.to(vertices.device)
            out.append(torch.sigmoid(v.reshape(v.shape[0], -1) @ W.t()).reshape(-1, 1, RES, RES).expand(-1, 3, -1, -1))
        return torch.cat(out, 0)
    return smpl, render, AS.Perceptor(0).to(DEV)


def test_through_the_context_both_posings_give_the_same_gradient_and_the_optimizer_runs():
    from avatarclip_amd import animate as A
    smpl, render, perceptor = _device_standins()
    text = F.normalize(torch.from_numpy(np.random.RandomState(9).randn(512).astype(np.float32)), dim=0).to(DEV)
    body = torch.from_numpy((np.random.RandomState(2).randn(2, 63) * 0.4).astype(np.float32))
    grads, losses = {}, {}
    for posing in A.AnimateContext.POSINGS:
        ctx = A.AnimateContext(perceptor, lambda t: text, smpl, None, render_fn=render, device=DEV, renderer_gradient=True, posing=posing)
        pose = body.clone().to(DEV).requires_grad_(True)
        np.random.seed(3)
        feature = ctx.get_pose_feature(pose)
        assert feature.shape == (2, 512)
        loss = (1 - F.cosine_similarity(feature, text[None], dim=-1)).sum()
        loss.backward()
        grads[posing], losses[posing] = pose.grad.clone(), float(loss.detach())
    scale = float(grads["torch"].abs().max())
    err = float((grads["hip"] - grads["torch"]).abs().max()) / scale
    print('d(1 - cos)/d pose, posing="hip" against "torch": worst difference / largest entry = %.3e (losses %.7f, %.7f)'
          % (err, losses["hip"], losses["torch"]))
    assert scale > 0 and torch.isfinite(grads["hip"]).all() and err <= 1e-4
    ctx = A.AnimateContext(perceptor, lambda t: text, smpl, None, render_fn=render, device=DEV, renderer_gradient=True, posing="hip")
    np.random.seed(4)
    torch.manual_seed(4)
    first = torch.randn(63)
    torch.manual_seed(4)
    got = A.PoseOptimizer(ctx, num_iteration=3).get_pose(ctx.get_text_feature("a rendered 3d man is arguing"))
    assert got.shape == (69,) and torch.isfinite(got).all()
    assert float((got[:63].cpu() - first).abs().max()) > 1e-3 and torch.equal(got[63:].cpu(), torch.zeros(6))   # three Adam steps moved it
