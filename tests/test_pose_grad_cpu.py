"""The posing gradient without a device: the numpy restatement of the rules of include/avc.h's posing-gradient section
(tests/smpl_grad_restatement.py) against float64 autograd of smpl_lbs.batch_rodrigues + smpl_lbs.lbs; that section of the header and its
binding; pose_hip_grad's argument errors; the operands the two host entry points hand the forward launches; AnimateContext's posing switch."""
import os
import re

import numpy as np
import pytest
import torch

from tests import drive_standins as S
from tests import smpl_grad_restatement as R
from tests.test_gpu_pose_preview import _lbs64, _poses, _template

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "avc.h")
LAUNCHES = ("avc_smpl_grad_tiles", "avc_smpl_grad_reduce", "avc_smpl_grad_chain")


@pytest.mark.parametrize("V", (1, 257))
def test_restatement_against_float64_autograd(V):
    """bound: 1e-12 of each frame's largest entry (both sides are float64 arithmetic of a few hundred operations per entry)"""
    a = _template(V)
    pose = _poses().double().requires_grad_(True)
    g = torch.from_numpy(np.random.RandomState(V).randn(pose.shape[0], V, 3))
    out = _lbs64_with_grad(a, pose)
    out.backward(g)
    r = R.backward(a, pose.detach(), g)
    assert float(np.abs(r["out"] - out.detach().numpy()).max()) <= 1e-12
    want, got = pose.grad.numpy(), r["dpose"]
    scale = np.abs(want).reshape(want.shape[0], -1).max(1)
    ratio = np.abs(got - want).reshape(want.shape[0], -1).max(1) / scale
    print("V = %d: worst |restated dpose - autograd| / frame's largest entry = %.3e" % (V, ratio.max()))
    assert (scale > 0).all() and np.isfinite(got).all()                 # the all-zero frame and the 1e-9 joint included
    assert ratio.max() <= 1e-12
    # the intermediates the GPU tests compare launches with: the same objects by another route (autograd to the joint transforms)
    assert r["g_vp"].shape == (33, V, 3) and r["dA"].shape == (33, 24, 3, 4) and r["dfeat"].shape == (33, 207)


def _lbs64_with_grad(a, pose):
    """test_gpu_pose_preview._lbs64 detaches its pose; the same call with the graph kept"""
    from avatarclip_amd import smpl_lbs
    d = lambda x: x.detach().cpu().double()
    T = pose.shape[0]
    rot = smpl_lbs.batch_rodrigues(pose.reshape(-1, 3)).reshape(T, 24, 3, 3)
    v, _ = smpl_lbs.lbs(d(a["v_template"])[None].expand(T, -1, -1), rot, d(a["posedirs"]), d(a["J_regressor"]), a["parents"], d(a["lbs_weights"]))
    assert torch.equal(v.detach(), _lbs64(a, pose.detach()))
    return v


def test_restated_intermediates_against_autograd_of_lbs():
    """g_vp, dA and dfeat are the gradients of lbs's output to v_posed, A and pose_feature: checked by making those three leaves"""
    a = _template(257)
    T = 6
    fwd = R.forward(a, _poses()[:T])
    g = np.random.RandomState(3).randn(T, 257, 3)
    vs, w, pd = (a[k].double() for k in ("v_template", "lbs_weights", "posedirs"))
    feat = torch.from_numpy(fwd["feat"]).requires_grad_(True)
    A = torch.from_numpy(fwd["A"]).requires_grad_(True)
    v_posed = (feat @ pd).reshape(T, -1, 3) + vs
    v_posed.retain_grad()
    M = torch.einsum("vj,tjab->tvab", w, A)
    out = torch.einsum("tvab,tvb->tva", M[..., :3], v_posed) + M[..., 3]
    assert float((out.detach() - torch.from_numpy(fwd["out"])).abs().max()) <= 1e-12
    out.backward(torch.from_numpy(g))
    g_vp, dA, dfeat = R.skin_adjoint(a, fwd, g)
    for name, got, want in (("g_vp", g_vp, v_posed.grad), ("dA", dA, A.grad), ("dfeat", dfeat, feat.grad)):
        want = want.numpy()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), name


def test_the_posing_gradient_section_of_avc_h_parses_and_is_listed():
    from avatarclip_amd import build, lib
    raw = open(HEADER).read()
    protos, abi = lib.parse_header(raw)
    assert len(protos) == 81 and abi == 4                               # added entry points do not change the revision
    assert sorted(n for n in protos if n.startswith("avc_smpl_grad")) == sorted(LAUNCHES + ("avc_smpl_grad_scratch_bytes",))
    for name in LAUNCHES:
        p = protos[name]
        assert p.launch and p.restype is lib.c_int and p.params[-1] == lib.Param("stream", lib.c_void_p, "void*", "void", False), name
    q = protos["avc_smpl_grad_scratch_bytes"]
    assert not q.launch and q.restype is lib.c_long and q.argtypes == [lib.c_int, lib.c_int]
    assert [x.name for x in protos["avc_smpl_grad_tiles"].params] == ["v_shaped", "posedirs", "weights", "feat", "A", "g", "V", "T", "g_vp", "scratch", "stream"]
    assert [x.name for x in protos["avc_smpl_grad_reduce"].params] == ["scratch", "V", "T", "dA", "dfeat", "stream"]
    assert [x.name for x in protos["avc_smpl_grad_chain"].params] == ["pose", "joints", "parents", "dA", "dfeat", "T", "dpose", "stream"]
    assert protos["avc_smpl_grad_chain"].params[2].elem == "int"
    for name in LAUNCHES:                                               # each cites the smpl_lbs lines it differentiates
        comment = raw[:raw.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert re.search(r"smpl_lbs\.py:\d+", comment), name
    assert not os.path.exists(os.path.join(ROOT, "include", "avc_smpl_grad.h")) and os.listdir(os.path.join(ROOT, "include")) == ["avc.h"]
    for src in ("avc_smpl.hip", "avc_smpl_grad.hip"):
        assert src in build.SOURCES and os.path.exists(os.path.join(build.CSRC, src)), src
    assert "avc_smpl.h" in build.HEADERS and build.ABI_HEADER in build.HEADERS and os.path.exists(os.path.join(build.CSRC, "avc_smpl.h"))
    assert os.path.samefile(os.path.join(build.CSRC, build.ABI_HEADER), HEADER) and os.path.samefile(lib.HEADER, HEADER)
    assert not hasattr(lib, "SMPL_GRAD_HEADER")


def test_load_binds_the_posing_gradient_and_names_a_library_that_lacks_a_symbol(monkeypatch, tmp_path):
    from avatarclip_amd import lib
    bound = lib.load()
    for name in LAUNCHES:
        assert name in lib._launches and getattr(bound, name).restype is lib.c_int, name
    assert bound.avc_smpl_grad_scratch_bytes.restype is lib.c_long
    assert bound.avc_smpl_grad_scratch_bytes(257, 9) == 2 * 9 * (24 * 12 + 207) * 4 and bound.avc_smpl_grad_scratch_bytes(0, 9) == 0
    assert bound.avc_smpl_grad_scratch_bytes(256, 1) == (24 * 12 + 207) * 4
    # a library from before an entry point was added has the right revision and lacks the symbol: the header of a later day stands in for it
    later = tmp_path / "avc.h"
    head, tail = open(HEADER).read().rsplit("#ifdef __cplusplus", 1)    # (after the last declaration, inside the extern "C" block)
    later.write_text(head + "int avc_smpl_grad_of_a_later_day(const float* pose, int T, void* stream);\n\n#ifdef __cplusplus" + tail)
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "HEADER", str(later))
    with pytest.raises(RuntimeError, match="lacks avc_smpl_grad_of_a_later_day of include/.*: rebuild the library") as e:
        lib.load()
    assert lib._lib is None
    text = str(e.value)
    assert lib.lib_path() in text and "revision 4" in text and "include/avc.h" in text
    assert text.endswith("rebuild the library (python -m avatarclip_amd.build --force)")


def test_pose_hip_grad_checks_its_arguments_before_it_loads_anything(monkeypatch):
    from avatarclip_amd import lib, smpl_lbs

    def no_library():
        raise AssertionError("the checks come before the library is loaded")
    monkeypatch.setattr(lib, "load", no_library)
    monkeypatch.setattr(lib, "call", lambda *a, **k: no_library())
    a, pose = S.template_arrays(), torch.zeros(2, 72, requires_grad=True)
    for bad in (torch.zeros(2, 69), torch.zeros(72), torch.zeros(2, 23, 3), torch.zeros(2, 24, 4)):
        with pytest.raises(ValueError, match="pose"):
            smpl_lbs.pose_hip_grad(a, bad)
    with pytest.raises(ValueError, match="v_shaped"):
        smpl_lbs.pose_hip_grad(a, pose, v_shaped=torch.zeros(699, 3))
    with pytest.raises(ValueError, match="v_shaped requires grad.*pose only"):
        smpl_lbs.pose_hip_grad(a, pose, v_shaped=a["v_template"].clone().requires_grad_(True))
    b = dict(a, posedirs=a["posedirs"][:206])
    with pytest.raises(ValueError, match="207"):
        smpl_lbs.pose_hip_grad(b, pose)
    b = dict(a, parents=a["parents"].clone())
    b["parents"][5] = 7
    with pytest.raises(ValueError, match="parent"):
        smpl_lbs.pose_hip_grad(b, pose)
    doc = smpl_lbs.pose_hip_grad.__doc__
    assert "bit for bit" in doc and "pose" in doc and "double backward" in doc.lower()


def test_both_entry_points_hand_the_forward_launches_the_same_operands(monkeypatch):
    """the host path has no bitwise pin on the device: with the launches recorded and the operands kept on the CPU, pose_hip issues exactly
    the two forward launches, and pose_hip_grad hands the same two the same shapes, dtypes and values"""
    from avatarclip_amd import lib, smpl_lbs
    calls = []
    monkeypatch.setattr(smpl_lbs, "_hip_device", lambda v_template: torch.device("cpu"))
    monkeypatch.setattr(lib, "stream", lambda: 0)
    monkeypatch.setattr(lib, "call", lambda name, *args, stream=None: calls.append((name, args, stream)))
    a = _template(65)
    pose = _poses()[:2].double().reshape(2, 24, 3)                      # a dtype and a shape the operands are not handed over in
    v_shaped = a["v_template"].double() * 1.25
    out = smpl_lbs.pose_hip(a, pose.clone().requires_grad_(True), v_shaped=v_shaped)
    assert [c[0] for c in calls] == ["avc_smpl_joint_mats", "avc_smpl_pose"]
    assert out.shape == (2, 65, 3) and out.dtype == torch.float32 and not out.requires_grad and out.grad_fn is None
    leaf = pose.clone().requires_grad_(True)
    out_g = smpl_lbs.pose_hip_grad(a, leaf, v_shaped=v_shaped)
    assert [c[0] for c in calls[2:]] == ["avc_smpl_joint_mats", "avc_smpl_pose"]
    assert out_g.shape == (2, 65, 3) and out_g.dtype == torch.float32 and out_g.requires_grad
    for (name, plain, s0), (_, graded, s1) in zip(calls[:2], calls[2:]):
        assert len(plain) == len(graded) and s0 == s1 == 0, name
        for i, (x, y) in enumerate(zip(plain, graded)):
            if torch.is_tensor(x):
                assert torch.is_tensor(y) and x.shape == y.shape and x.dtype == y.dtype and x.is_contiguous() and y.is_contiguous(), (name, i)
            else:
                assert type(x) is type(y) is int and x == y, (name, i)
    # the inputs of the two launches by value (their outputs are fresh, uninitialised buffers here: nothing ran)
    (p0, j0, par0, T0, feat0, A0), (p1, j1, par1, T1, feat1, A1) = calls[0][1], calls[2][1]
    assert T0 == 2 and p0.shape == (2, 72) and torch.equal(p0, pose.float().reshape(2, 72)) and torch.equal(p0, p1)
    assert torch.equal(j0, j1) and torch.equal(j0, a["J_regressor"] @ v_shaped.float())
    assert par0.dtype == torch.int32 and torch.equal(par0, par1) and par0.tolist() == [int(x) for x in a["parents"]]
    assert feat0.shape == (2, 207) and A0.shape == (2, 24, 12)
    for i in (0, 1, 2):                                                 # v_shaped, posedirs, weights
        assert torch.equal(calls[1][1][i], calls[3][1][i]), i
    assert torch.equal(calls[1][1][0], v_shaped.float()) and calls[1][1][5:7] == (65, 2) == calls[3][1][5:7]
    assert calls[1][1][3] is feat0 and calls[1][1][4] is A0 and calls[1][1][7] is out
    # an empty batch launches nothing, in either direction
    del calls[:]
    empty = torch.zeros(0, 72, requires_grad=True)
    assert smpl_lbs.pose_hip(a, empty).shape == (0, 65, 3)
    out_e = smpl_lbs.pose_hip_grad(a, empty)
    out_e.sum().backward()
    assert out_e.shape == (0, 65, 3) and empty.grad.shape == (0, 72) and calls == []


def test_context_posing_switch(monkeypatch):
    import math
    from avatarclip_amd import animate as A
    from avatarclip_amd import smpl_lbs
    from tests import animate_clip_standins as AS
    smpl = AS.smpl_arrays()
    mk = lambda **kw: A.AnimateContext(None, None, smpl, None, device="cpu", **kw)
    with pytest.raises(ValueError, match=r'"torch".*"hip".*bogus'):
        mk(posing="bogus")
    assert mk().posing == "torch" and mk(posing="hip").posing == "hip"
    seen = []

    def recorder(arrays, pose, v_shaped=None):
        seen.append((arrays, pose, v_shaped))
        return torch.zeros(pose.shape[0], AS.NV, 3)
    monkeypatch.setattr(smpl_lbs, "pose_hip_grad", recorder)
    body = torch.from_numpy(np.random.RandomState(1).randn(3, 63).astype(np.float32))
    v = mk(posing="hip").posed_vertices(body)
    assert v.shape == (3, AS.NV, 3) and len(seen) == 1
    arrays, full, v_shaped = seen[0]
    assert arrays is smpl and v_shaped is None and full.shape == (3, 24, 3) and full.dtype == torch.float32
    root = torch.tensor([math.pi / 2, 0.0, 0.0])
    assert torch.equal(full[:, 0], root[None].expand(3, -1))
    assert torch.equal(full[:, 1:22].reshape(3, 63), body) and torch.equal(full[:, 22:], torch.zeros(3, 2, 3))
    mk(posing="hip").posed_vertices(torch.ones(69))                     # one pose of 69 values passes through unpadded
    assert seen[1][1].shape == (1, 24, 3) and torch.equal(seen[1][1][0, 1:].reshape(-1), torch.ones(69))
    # the default never gets there, and is today's arithmetic
    v0 = mk().posed_vertices(body)
    assert len(seen) == 2
    rot = smpl_lbs.batch_rodrigues(full.reshape(-1, 3)).reshape(3, 24, 3, 3)
    want, _ = smpl_lbs.lbs(smpl["v_template"][None].expand(3, -1, -1), rot, smpl["posedirs"], smpl["J_regressor"], smpl["parents"], smpl["lbs_weights"])
    assert torch.equal(v0, want)
    for text in (A.__doc__, A.AnimateContext.__doc__):
        assert "not bit for bit" in text and '"torch"' in text
