"""The host side of the pose and motion previews (preview.body_pose, the argument checks of smpl_lbs.pose_hip and preview.preview, the two
entry points of csrc/avc_smpl.hip in lib.py's table), none of which needs a device or the library."""
import os
import re

import numpy as np
import pytest
import torch

from tests import drive_standins as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_body_pose_takes_every_layout_of_read_pose_my_and_zeroes_the_root():
    from avatarclip_amd import preview
    rs = np.random.RandomState(0)
    full = rs.randn(4, 72).astype(np.float32)
    before = full.copy()
    p = preview.body_pose(full)
    assert p.shape == (4, 72) and p.dtype == np.float32
    assert np.array_equal(p[:, :3], np.zeros((4, 3), np.float32)) and np.array_equal(p[:, 3:], full[:, 3:])
    assert np.array_equal(full, before) and full[:, :3].any()                                          # the caller's array is left alone
    wide = rs.randn(3, 80).astype(np.float32)
    p = preview.body_pose(wide)
    assert p.shape == (3, 72) and np.array_equal(p[:, 3:], wide[:, 3:72]) and not p[:, :3].any()
    body = rs.randn(5, 69).astype(np.float32)
    p = preview.body_pose(body)
    assert p.shape == (5, 72) and np.array_equal(p[:, 3:], body) and not p[:, :3].any()
    short = rs.randn(2, 63).astype(np.float32)
    p = preview.body_pose(short)
    assert p.shape == (2, 72) and np.array_equal(p[:, 3:66], short) and not p[:, :3].any() and not p[:, 66:].any()
    for n in (63, 69, 72, 75):                                                                         # a 1-D pose is one frame
        one = rs.randn(n).astype(np.float64)
        p = preview.body_pose(one)
        assert p.shape == (1, 72) and p.dtype == np.float32 and not p[0, :3].any()
        lo = 3 if n >= 72 else 0
        assert np.array_equal(p[0, 3:3 + min(n - lo, 69)], one.astype(np.float32)[lo:lo + 69])
    assert preview.body_pose(torch.zeros(2, 69)).shape == (2, 72)
    for bad in (np.zeros((3, 70)), np.zeros((2, 3, 72)), np.zeros((0, 72)), np.zeros(70), np.zeros((2, 24, 3))):
        with pytest.raises(ValueError):
            preview.body_pose(bad)


def _arrays():
    return S.template_arrays()


def test_pose_hip_checks_its_arguments_before_it_loads_anything(monkeypatch):
    from avatarclip_amd import lib, smpl_lbs

    def no_library():
        raise AssertionError("the checks come before the library is loaded")
    monkeypatch.setattr(lib, "load", no_library)
    pose = torch.zeros(2, 72)
    a = _arrays()
    a["parents"] = a["parents"].clone()
    a["parents"][5] = 5
    with pytest.raises(ValueError, match="parent"):
        smpl_lbs.pose_hip(a, pose)
    a["parents"][5] = 7
    with pytest.raises(ValueError, match="parent"):
        smpl_lbs.pose_hip(a, pose)
    a["parents"][5] = -1
    with pytest.raises(ValueError, match="parent"):
        smpl_lbs.pose_hip(a, pose)
    a = _arrays()                                                       # 23 joints
    a.update(parents=a["parents"][:23], J_regressor=a["J_regressor"][:23], lbs_weights=a["lbs_weights"][:, :23], posedirs=a["posedirs"][:198])
    with pytest.raises(ValueError, match="24 joints"):
        smpl_lbs.pose_hip(a, torch.zeros(2, 69))
    a = _arrays()
    a["posedirs"] = a["posedirs"][:206]
    with pytest.raises(ValueError, match="207"):
        smpl_lbs.pose_hip(a, pose)
    a = _arrays()
    for bad in (torch.zeros(2, 69), torch.zeros(72), torch.zeros(2, 23, 3), torch.zeros(2, 24, 4)):
        with pytest.raises(ValueError, match="pose"):
            smpl_lbs.pose_hip(a, bad)
    with pytest.raises(ValueError, match="v_shaped"):
        smpl_lbs.pose_hip(a, pose, v_shaped=torch.zeros(699, 3))
    a["lbs_weights"] = a["lbs_weights"][:699]
    with pytest.raises(ValueError):
        smpl_lbs.pose_hip(a, pose)
    a = _arrays()
    a["posedirs"] = a["posedirs"][:, :-3]
    with pytest.raises(ValueError, match="posedirs"):
        smpl_lbs.pose_hip(a, pose)
    assert "forward" in smpl_lbs.pose_hip.__doc__.lower() and "differentiable" in smpl_lbs.pose_hip.__doc__


def test_preview_wants_exactly_one_source(tmp_path):
    from avatarclip_amd import preview
    out = str(tmp_path / "p.gif")
    smpl, poses = {"faces": np.zeros((1, 3), np.int32)}, np.zeros((2, 69), np.float32)
    for kw in (dict(mesh="a.ply", smpl=smpl, poses=poses), dict(glb="a.glb", smpl=smpl, poses=poses), dict(mesh="a.ply", glb="a.glb"), dict()):
        with pytest.raises(ValueError, match="exactly one source"):
            preview.preview(out, **kw)
    with pytest.raises(ValueError, match="--smpl and --poses"):
        preview.preview(out, poses=poses)
    with pytest.raises(ValueError, match="--smpl and --poses"):
        preview.preview(out, smpl=smpl)
    with pytest.raises(ValueError, match="--smpl and --poses"):
        preview.preview(out, mesh="a.ply", poses=poses)
    # the command line says the same and does not get as far as a device
    for argv in (["--smpl", "m.npz", "--out", out], ["--poses", "p.npy", "--out", out],
                 ["--mesh", "a.ply", "--smpl", "m.npz", "--poses", "p.npy", "--out", out]):
        with pytest.raises(SystemExit, match="preview: "):
            preview.main(argv)
    assert not os.path.exists(out)


def test_lib_lists_the_two_entry_points_with_the_headers_argument_counts():
    from ctypes import c_int, c_void_p as P
    from avatarclip_amd import build, lib
    raw = open(os.path.join(ROOT, "include", "avc.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    protos, _ = lib.parse_header(raw)
    bound = lib.load()
    want = {"avc_smpl_joint_mats": [P, P, P, c_int, P, P, P],
            "avc_smpl_pose": [P, P, P, P, P, c_int, c_int, P, P]}
    for name in ("avc_smpl_joint_mats", "avc_smpl_pose"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, "%s is not declared in include/avc.h" % name
        assert name in protos
        res, args = protos[name].restype, protos[name].argtypes
        assert res is lib.c_int and len(args) == len(m.group(1).split(",")), name
        assert args[-1] is P                                            # the stream
        assert args == want[name], name
        assert getattr(bound, name).restype is c_int and list(getattr(bound, name).argtypes) == want[name], name
    assert "avc_smpl.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "avc_smpl.hip"))
    assert lib.ABI_VERSION == 4 and re.search(r"#define\s+AVC_ABI_VERSION\s+4\b", hdr)
