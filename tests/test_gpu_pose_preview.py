"""The forward-only SMPL posing kernels (csrc/avc_smpl.hip through smpl_lbs.pose_hip) against smpl_lbs's own torch functions run in
float64 on the CPU from the same float32 inputs, at every edge of a power-of-two tile up to 256 vertices x 16 frames; and the SMPL-body
source of preview / animate's --preview end to end on stand-ins.  The bound is the project's posing bound (the drive fixture's): 1e-5 m,
and 1e-5 on the dimensionless pose feature; the same fp32 arithmetic measured 5e-7 there, so anything above 2e-6 wants a cause."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import animate_clip_standins as AS
from tests import drive_standins as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 1e-5
VS = (1, 63, 64, 65, 255, 256, 257, 700)
TS = (1, 2, 7, 8, 9, 15, 16, 17, 33)
T_ALL = 33


@functools.lru_cache(maxsize=None)
def _poses():
    """float32 [33,24,3]: frame 0 of drive_standins.motion, then the hand-made frames (all zeros; one joint at 1e-9; one at angle 3.1; one
    at 4.0; every joint bent at once), then the rest of the motion -- every T >= 7 holds all of them"""
    m = S.motion(T_ALL).reshape(T_ALL, 24, 3).copy()
    hand = np.zeros((5, 24, 3), np.float32)
    hand[1, 7, 0] = 1e-9
    hand[2, 4] = np.array([3.1, 0.0, 0.0], np.float32)
    hand[3, 16] = np.array([0.0, 2.4, -3.2], np.float32)                 # |r| = 4.0
    hand[4] = np.random.RandomState(11).uniform(0.6, 1.4, (24, 3)) * np.random.RandomState(12).choice([-1.0, 1.0], (24, 3))
    p = torch.from_numpy(np.concatenate([m[:1], hand, m[1:T_ALL - 5]]).astype(np.float32))
    assert p.shape == (T_ALL, 24, 3)
    return p


@functools.lru_cache(maxsize=None)
def _template(V):
    """drive_standins.template_arrays() sliced to V vertices (CPU float32): the rest joints follow from the sliced arrays"""
    a = S.template_arrays()
    K = a["v_template"].shape[0]
    return dict(v_template=a["v_template"][:V].contiguous(), posedirs=a["posedirs"].reshape(207, K, 3)[:, :V].reshape(207, 3 * V).contiguous(),
                J_regressor=a["J_regressor"][:, :V].contiguous(), parents=a["parents"], lbs_weights=a["lbs_weights"][:V].contiguous())


@functools.lru_cache(maxsize=None)
def _template_dev(V):
    return {k: x.to(DEV) for k, x in _template(V).items()}


def _lbs64(a, pose, v_shaped=None):
    """smpl_lbs.lbs in float64 on the CPU from the float32 arrays"""
    from avatarclip_amd import smpl_lbs
    d = lambda x: x.detach().cpu().double()
    T = pose.shape[0]
    rot = smpl_lbs.batch_rodrigues(d(pose).reshape(-1, 3)).reshape(T, 24, 3, 3)
    vs = d(a["v_template"] if v_shaped is None else v_shaped)
    v, _ = smpl_lbs.lbs(vs[None].expand(T, -1, -1), rot, d(a["posedirs"]), d(a["J_regressor"]), a["parents"], d(a["lbs_weights"]))
    return v


@functools.lru_cache(maxsize=None)
def _reference(V):
    """the float64 vertices of all 33 frames: computed once per V, shared, never written to"""
    return _lbs64(_template(V), _poses())


def test_joint_matrices_against_float64():
    from avatarclip_amd import lib as L
    from avatarclip_amd import smpl_lbs
    a, pose = _template(700), _poses()
    T = pose.shape[0]
    joints = torch.matmul(a["J_regressor"], a["v_template"])                                  # fp32: what the kernel is handed
    rot = smpl_lbs.batch_rodrigues(pose.double().reshape(-1, 3)).reshape(T, 24, 3, 3)
    feat_ref = (rot[:, 1:] - torch.eye(3, dtype=torch.float64)).reshape(T, 207)
    _, A_ref = smpl_lbs.batch_rigid_transform(rot, joints.double()[None].expand(T, -1, -1), a["parents"])
    feat = torch.full((T, 207), float("nan"), device=DEV)
    A = torch.full((T, 24, 12), float("nan"), device=DEV)
    pose_d, joints_d, parents_d = pose.to(DEV).contiguous(), joints.to(DEV), a["parents"].to(device=DEV, dtype=torch.int32)    # (held until the work is done)
    lib, s = L.load(), L.stream()
    L.check(lib.avc_smpl_joint_mats(L.ptr(pose_d), L.ptr(joints_d), L.ptr(parents_d), T, L.ptr(feat), L.ptr(A), s), "avc_smpl_joint_mats")
    torch.cuda.synchronize()
    e_feat = float((feat.cpu().double() - feat_ref).abs().max())
    e_A = float((A.cpu().double().reshape(T, 24, 3, 4) - A_ref[:, :, :3, :]).abs().max())
    print("avc_smpl_joint_mats: worst |feat - fp64| = %.3e, worst |A - fp64| = %.3e" % (e_feat, e_A))
    assert e_feat <= BOUND and e_A <= BOUND
    assert torch.equal(feat[1], torch.zeros(207, device=DEV))                                 # the all-zero frame: R = I exactly
    # empty and refused inputs: no launch
    assert lib.avc_smpl_joint_mats(None, None, None, 0, None, None, s) == 0
    assert lib.avc_smpl_joint_mats(None, L.ptr(joints_d), L.ptr(parents_d), 1, L.ptr(feat), L.ptr(A), s) == 1
    assert b"NULL" in lib.avc_last_error()
    assert lib.avc_smpl_joint_mats(L.ptr(pose_d), L.ptr(joints_d), L.ptr(parents_d), 1, L.ptr(feat), A.data_ptr() + 4, s) == 1
    assert b"aligned" in lib.avc_last_error()
    assert lib.avc_smpl_pose(None, None, None, None, None, 0, 3, None, s) == 0
    assert lib.avc_smpl_pose(None, None, None, None, None, 3, 0, None, s) == 0
    assert lib.avc_smpl_pose(None, None, None, L.ptr(feat), L.ptr(A), 3, 1, None, s) == 1
    assert b"NULL" in lib.avc_last_error()


@pytest.mark.parametrize("V", VS)
def test_vertices_against_float64_lbs(V):
    from avatarclip_amd import smpl_lbs
    a, ref, pose = _template_dev(V), _reference(V), _poses().to(DEV)
    worst = 0.0
    for T in TS:
        out = smpl_lbs.pose_hip(a, pose[:T])
        assert out.shape == (T, V, 3) and out.dtype == torch.float32 and out.is_cuda and not out.requires_grad
        worst = max(worst, float((out.cpu().double() - ref[:T]).abs().max()))
    print("pose_hip V = %d: worst |vertex - fp64 lbs| over T in %s = %.3e m" % (V, TS, worst))
    assert worst <= BOUND
    assert float((ref[0] - ref[1]).abs().max()) > 1e-2                                        # the poses do move the body


def test_a_batch_equals_its_single_frames_and_two_runs_agree():
    from avatarclip_amd import smpl_lbs
    a, pose = _template_dev(700), _poses().to(DEV)[:19]
    batch = smpl_lbs.pose_hip(a, pose)
    again = smpl_lbs.pose_hip(a, pose)
    assert torch.equal(batch, again)                                                          # determinism: bit-identical
    for t in range(19):
        assert torch.equal(smpl_lbs.pose_hip(a, pose[t:t + 1])[0], batch[t]), t
    assert torch.equal(smpl_lbs.pose_hip(a, pose.reshape(19, 72)), batch)                     # [T,72] and [T,24,3] are one thing
    assert smpl_lbs.pose_hip(a, pose[:0]).shape == (0, 700, 3)


def test_non_contiguous_pose_and_a_v_shaped_of_its_own():
    from avatarclip_amd import smpl_lbs
    a, pose = _template_dev(257), _poses()
    wide = torch.zeros(9, 24, 6)
    wide[:, :, ::2] = pose[:9]
    strided = wide.to(DEV)[:, :, ::2]
    assert not strided.is_contiguous()
    out = smpl_lbs.pose_hip(a, strided)
    assert torch.equal(out, smpl_lbs.pose_hip(a, pose[:9].to(DEV)))
    g = torch.Generator().manual_seed(5)
    v_shaped = (_template(257)["v_template"] * 1.1 + 0.02 * torch.randn(257, 3, generator=g))
    vs2 = torch.zeros(257, 6)
    vs2[:, ::2] = v_shaped
    out_s = smpl_lbs.pose_hip(a, pose[:9].to(DEV), v_shaped=vs2.to(DEV)[:, ::2])
    ref = _lbs64(_template(257), pose[:9], v_shaped)
    err = float((out_s.cpu().double() - ref).abs().max())
    print("pose_hip with its own v_shaped: worst |vertex - fp64 lbs| = %.3e m" % err)
    assert err <= BOUND
    assert float((out_s - out).abs().max()) > 1e-2                                            # v_shaped is honoured, not v_template
    assert float((out.cpu().double() - _reference(257)[:9]).abs().max()) <= BOUND


def test_preview_of_the_smpl_body_small(tmp_path):
    from PIL import Image
    from avatarclip_amd import preview, smpl_lbs
    smpl = AS.smpl_arrays()
    poses = (np.random.RandomState(2).randn(5, 69) * 0.3).astype(np.float32)
    out, images = preview.preview(str(tmp_path / "p.gif"), smpl=smpl, poses=poses, size=64, ss=1)
    assert images.shape == (5, 64, 64, 3) and images.dtype == torch.uint8
    with Image.open(out) as im:
        assert im.n_frames == 5 and im.size == (64, 64)
    img = images.cpu().numpy()
    assert all((img[i] != 255).any() for i in range(5))                                       # the body is in every frame
    assert any((img[i] != img[0]).any() for i in range(1, 5))                                 # and it moves
    v = smpl_lbs.pose_hip(smpl, torch.from_numpy(preview.body_pose(poses)))
    assert v.shape == (5, AS.NV, 3)
    eyes, ats, near, far = preview.frame_cameras(v, 1, up="y")
    direct = preview.render_frames(v, smpl["faces"], None, eyes, ats, up="y", image_size=64, ss=1, near=near, far=far)
    assert torch.equal(images, direct)
    # one pose is a static source: a turn-table of --views frames, the front view for a .png
    out4, turn = preview.preview(str(tmp_path / "one.gif"), smpl=smpl, poses=poses[0], views=4, size=64, ss=1)
    assert turn.shape == (4, 64, 64, 3)
    with Image.open(out4) as im:
        assert im.n_frames == 4
    assert any((turn[i] != turn[0]).any() for i in range(1, 4))
    png, _ = preview.preview(str(tmp_path / "one.png"), smpl=smpl, poses=poses[0], views=4, size=64, ss=1)
    with Image.open(png) as im:
        assert getattr(im, "n_frames", 1) == 1 and im.size == (64, 64)
        assert np.array_equal(np.asarray(im.convert("RGB")), turn[0].cpu().numpy())


def test_animate_run_writes_its_previews_and_returns_the_same_tensors(tmp_path):
    from PIL import Image
    from avatarclip_amd import animate as A
    from avatarclip_amd.conf import ConfigFactory
    from tests import test_animate as TA
    dev = torch.device(DEV)
    ctx = TA._ctx(dev, smpl=TA._synthetic_smpl(dev))                   # (the codebook retrieval and the interpolation need no image tower)
    g = TA._gold()
    assets = dict(codebook=g["cb_codebook"], codebook_embedding=g["cb_embedding"])
    results = {}
    for name, kw in (("with", dict(preview=True, preview_size=64)), ("without", dict())):
        conf = ConfigFactory.parse_string(TA.CONF.format(out=str(tmp_path / name), mode="motion", pose="VPoserCodebook", motion="MotionInterpolation", extra=""))
        np.random.seed(4)
        torch.manual_seed(4)
        poses, motion = A.run(conf, ctx, pose_assets=assets, **kw)
        results[name] = (poses.clone(), motion.clone(), np.random.rand(), float(torch.rand(1)))
    assert sorted(os.listdir(str(tmp_path / "with"))) == sorted(["candidate_%d.npy" % i for i in range(5)] + ["candidate_%d.png" % i for i in range(5)]
                                                                + ["motion.gif", "motion.npy"])
    assert sorted(os.listdir(str(tmp_path / "without"))) == ["candidate_%d.npy" % i for i in range(5)] + ["motion.npy"]
    with Image.open(str(tmp_path / "with" / "motion.gif")) as im:
        assert im.n_frames == 60 and im.size == (64, 64)
    pictures = []
    for i in range(5):
        with Image.open(str(tmp_path / "with" / ("candidate_%d.png" % i))) as im:
            assert im.size == (64, 64)
            pictures.append(np.asarray(im.convert("RGB")))
            assert (pictures[-1] != 255).any()
    assert any((pictures[i] != pictures[0]).any() for i in range(1, 5))
    (p1, m1, n1, t1), (p0, m0, n0, t0) = results["with"], results["without"]
    assert torch.equal(p1, p0) and torch.equal(m1, m0) and p1.shape == (5, 63) and m1.shape == (60, 69)
    assert n1 == n0 and t1 == t0                                       # the preview drew from neither global generator
