"""The host side of the drive step (avatarclip_amd/drive.py; AvatarGen/AppearanceGen/drive.py) against tests/golden/drive.npz, which
scripts/gen_golden_drive.py produced by RUNNING THE REFERENCE'S OWN drive.py functions (extracted with `ast`; open3d / smplx replaced by the
stand-ins that script documents: unpinned against those packages).  The .pc2 body of the fixture holds every re-posed frame."""
import os

import numpy as np
import pytest
import torch

from tests import drive_standins as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drive.npz")


def _gold():
    return dict(np.load(GOLD))


def _frames(g):
    m = len(g["nearest"])
    return np.frombuffer(g["pc2"][32:].tobytes(), "<f4").reshape(-1, m, 3)


def test_pc2_writer_reproduces_the_reference_bytes(tmp_path):
    from avatarclip_amd import drive
    g = _gold()
    frames = _frames(g)
    assert frames.shape == (8, len(g["nearest"]), 3)
    ref = g["pc2"].tobytes()
    assert drive.pc2_header(frames.shape[1], 8) == ref[:32]
    a = drive.write_pc2(str(tmp_path / "a.pc2"), [torch.from_numpy(f.copy()) for f in frames])        # the reference's list form
    b = drive.write_pc2(str(tmp_path / "b.pc2"), (frames[i:i + 3] for i in range(0, 8, 3)), vcount=frames.shape[1], num_samples=8)
    for p in (a, b):
        with open(p, "rb") as f:
            assert f.read() == ref
    head, back = drive.read_pc2(a)
    assert head[1:] == (1, frames.shape[1], 0.0, 60.0, 8) and np.array_equal(back, frames)
    with pytest.raises(ValueError):
        drive.write_pc2(str(tmp_path / "c.pc2"), [frames[:3]], vcount=frames.shape[1], num_samples=8)


def test_motion_layouts_and_the_root_overwrite():
    from avatarclip_amd import drive, smpl_lbs
    g = _gold()
    mo = g["motion"]
    rot = drive.read_pose_my(mo)
    assert rot.shape == (8, 24, 3, 3) and rot.dtype == torch.float32
    assert torch.allclose(rot, torch.from_numpy(g["frame_rot"]), atol=1e-6)
    root = smpl_lbs.batch_rodrigues(torch.tensor([[np.pi / 2, 0.0, 0.0]], dtype=torch.float32))[0]
    assert torch.equal(rot[:, 0], root.expand(8, 3, 3))
    assert torch.equal(drive.read_pose_my(mo[:, 3:]), rot)                          # [T, 69]: animate.run's body pose, no root
    padded = mo.copy()
    padded[:, 66:] = 0
    assert torch.equal(drive.read_pose_my(mo[:, 3:66]), drive.read_pose_my(padded))  # [T, 63]: 6 zeros appended
    assert torch.equal(drive.read_pose_my(mo[2]), rot[2:3])                          # one pose = one frame
    assert torch.equal(drive.read_pose_my(np.concatenate([mo, mo[:, :6]], 1)), rot)  # more columns: the first 72, as the reference
    before = mo.copy()
    drive.read_pose_my(mo)
    assert np.array_equal(mo, before)                                                # the caller's array is not overwritten
    for bad in (np.zeros((4, 70), np.float32), np.zeros((0, 72), np.float32), np.zeros((2, 3, 72), np.float32), np.zeros(10, np.float32)):
        with pytest.raises(ValueError):
            drive.read_pose_my(bad)


def test_template_and_per_template_transforms_match_the_reference():
    from avatarclip_amd import drive
    g = _gold()
    a = S.template_arrays()
    template, pose_rot = drive.load_template_smpl(a, g["stand_pose"])
    assert torch.allclose(template, torch.from_numpy(g["template_v"]), atol=1e-6)
    T = drive.template_transforms(a, pose_rot)
    W = a["lbs_weights"]
    assert torch.allclose(T[0], (W @ torch.from_numpy(g["stand_A"]).reshape(24, 16)).reshape(-1, 4, 4), atol=1e-6)
    inv = torch.linalg.inv(T)[0]
    assert torch.allclose(inv, torch.from_numpy(g["stand_T_inv"]), atol=1e-5), (inv - torch.from_numpy(g["stand_T_inv"])).abs().max()
    Tf = drive.template_transforms(a, torch.from_numpy(g["frame_rot"]))
    ref = torch.einsum("kj,tjc->tkc", W, torch.from_numpy(g["frame_A"]).reshape(8, 24, 16)).reshape(8, -1, 4, 4)
    assert Tf.shape == (8, 700, 4, 4) and torch.allclose(Tf, ref, atol=1e-6)
    x = drive.rows3(Tf)
    assert x.shape == (8, 700, 12) and torch.equal(x[3, 5, 4:8], Tf[3, 5, 1])
    # the rotation of drive.py:318-323 is exact: the cleaned vertices are rotated input vertices
    rv = drive.rotate_vertices(g["in_v"])
    assert np.array_equal(rv[:, 0], g["in_v"][:, 0]) and np.array_equal(rv[:, 1], -g["in_v"][:, 2]) and np.array_equal(rv[:, 2], g["in_v"][:, 1])
    assert set(map(tuple, g["clean_v"])) <= set(map(tuple, rv))


def test_argument_checks(tmp_path):
    from avatarclip_amd import drive
    a = S.template_arrays()
    with pytest.raises(ValueError):
        drive.load_template_smpl(a, np.zeros(69, np.float32))
    with pytest.raises(ValueError):
        drive.find_nearest_ind(torch.zeros(4, 2), torch.zeros(3, 3))
    with pytest.raises(ValueError):
        drive.find_nearest_ind(torch.zeros(4, 3), torch.zeros(0, 3))
    with pytest.raises(ValueError):
        drive.skin_apply(torch.zeros(1, 5, 16), torch.zeros(3, dtype=torch.int32), torch.zeros(3, 3))
    with pytest.raises(ValueError):
        drive.skin_apply(torch.zeros(1, 5, 12), torch.zeros(3, dtype=torch.int64), torch.zeros(3, 3))
    with pytest.raises(ValueError):
        drive.cleanup_mesh(np.zeros((5, 2), np.float32), np.zeros((1, 3), np.int32))
    with pytest.raises(ValueError):
        drive.cleanup_mesh(np.zeros((5, 3), np.float32), np.zeros((1, 3), np.int32), colors=np.zeros((4, 4), np.uint8))
    with pytest.raises(SystemExit):
        drive.main(["--mesh", "x.ply"])                                          # the other required arguments are missing
