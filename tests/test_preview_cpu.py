"""The host side of the preview renderer (avatarclip_amd/preview.py) and its yardstick (tests/preview_restatement.py), without a GPU: the
restatement's own fill rule and key rule, the auto-framed cameras, the three sources and the command line's refusals."""
import os

import numpy as np
import pytest
import torch

from avatarclip_amd import drive, mesh, preview, rig
from tests import preview_restatement as PR
from tests import preview_scenes as PS


def _cam(sc, up="y"):
    return preview.look_frames(sc["eye"], sc["at"], up)[0]


def _project(sc, R):
    import math
    return PR.project(sc["v"], _cam(sc), math.tan(math.radians(sc["fov"]) * 0.5), sc["near"], sc["far"], R)


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("diagonal", [0, 1])
@pytest.mark.parametrize("winding", [0, 1, 2])
def test_quad_is_covered_exactly_once(diagonal, winding):
    """a quad with corners ON pixel centres and edges THROUGH pixel centres (axis-aligned and 45 degree edges), split along either
    diagonal, both / mixed windings: every pixel centre inside or on the top-left border is covered exactly once, none twice"""
    R = 16
    corners = [(3 * 256 + 128, 2 * 256 + 128), (11 * 256 + 128, 2 * 256 + 128), (13 * 256 + 128, 12 * 256 + 128), (3 * 256 + 128, 12 * 256 + 128)]
    X, Y = np.array([c[0] for c in corners], np.int64), np.array([c[1] for c in corners], np.int64)
    Z = np.full(4, 1000, np.int64)
    tris = [[0, 1, 2], [0, 2, 3]] if diagonal == 0 else [[0, 1, 3], [1, 2, 3]]
    if winding == 1:
        tris = [[a, c, b] for a, b, c in tris]
    if winding == 2:
        tris[1] = [tris[1][0], tris[1][2], tris[1][1]]
    n = PR.coverage_count(X, Y, Z, np.asarray(tris), R)
    assert n.max() == 1
    # the quad as a whole, by the same rule: a point strictly inside is covered; on the left / top border too; on the right / bottom not
    assert n[2, 3] == 1 and n[2, 10] == 1 and n[2, 11] == 0          # the top edge y = 2: owned, except its right end
    assert n[6, 3] == 1 and n[11, 3] == 1 and n[12, 3] == 0          # the left edge x = 3: owned, except its bottom end
    assert n[12, 8] == 0 and n[11, 8] == 1                           # the bottom edge y = 12: not owned
    assert n[7, 12] == 0 and n[7, 11] == 1                           # the right edge passes through the centre of pixel (12, 7): not owned
    assert n[5, 5] == 1 and n[7, 7] == 1 and n[1, 5] == 0 and n[13, 5] == 0      # (5, 5) lies on one diagonal, (7, 7) on both
    both = PR.coverage_count(X, Y, Z, np.asarray([[0, 1, 2], [0, 2, 3]]), R)
    assert np.array_equal(n, both)                                   # the same set whichever diagonal, whichever winding
    assert n.sum() > 60


def test_face_order_matters_only_at_exact_depth_ties():
    sc = PS.random_triangles()
    R = 64
    X, Y, Z, _ = _project(sc, R)
    t = sc["t"]
    key = PR.rasterize(X, Y, Z, t, R)
    assert np.array_equal(key, PR.rasterize(X, Y, Z, t, R, order=range(len(t) - 1, -1, -1)))       # the visiting order never matters
    a, b = 17, 251
    swapped = t.copy()
    swapped[[a, b]] = swapped[[b, a]]
    key2 = PR.rasterize(X, Y, Z, swapped, R)
    ids, ids2 = PR.face_ids(key), PR.face_ids(key2)
    ren = ids2.copy()
    ren[ids2 == a], ren[ids2 == b] = b, a                            # name the faces as before the swap
    diff = ids != ren
    # where the winner changed, the two candidates have the same depth (a tie that went to the lower index both times)
    assert np.array_equal((key >> 32)[diff], (key2 >> 32)[diff])
    copies = np.arange(290, 300)
    assert not np.isin(ids, copies).any()                            # an exact copy of an earlier face never wins a pixel


def test_fixture_has_background_overlaps_and_a_full_sheet():
    sc = PS.random_triangles()
    X, Y, Z, _ = _project(sc, 64)
    n = PR.coverage_count(X, Y, Z, sc["t"], 64)
    assert (n == 0).sum() > 50 and (n >= 3).sum() > 50 and (Z >= 0).all()
    sh = PS.sheet()
    X, Y, Z, _ = _project(sh, 64)
    assert len(sh["t"]) == 128 and np.array_equal(PR.coverage_count(X, Y, Z, sh["t"], 64), np.ones((64, 64), np.int32))
    big = PS.big_behind_small()
    X, Y, Z, _ = _project(big, 256)
    ids = PR.face_ids(PR.rasterize(X, Y, Z, big["t"], 256))
    assert (ids >= 0).all() and (ids == 0).sum() > 256 * 256 // 2 and len(np.unique(ids)) > 40


def test_snapping_rounds_half_up_and_marks_invalid_vertices():
    cam = preview.look_frames([0, 0, 3], [0, 0, 0], "y")[0]
    v = np.array([[0, 0, 0], [0, 0, 2.0], [0, 0, -2.0], [1.0, 1.0, 0], [50.0, 0, 0], [0, 0, -1.5]], np.float32)
    X, Y, Z, iw = PR.project(v, cam, 1.0 / 3.0, 1.5, 4.5, 64)
    assert (X[0], Y[0]) == (32 * 256, 32 * 256) and iw[0] == np.float32(1.0 / 3.0)
    assert Z[1] == -1 and Z[2] == -1                                 # nearer than near, beyond far
    assert (X[3], Y[3]) == (64 * 256, 0)                             # the top right corner of the image: +x right, +y up
    assert Z[4] == -1 and Z[5] == (1 << 24) - 1 and Z[0] > 0         # outside the guard band; exactly at far


# ---------------------------------------------------------------------------------------------------------------- cameras
@pytest.mark.parametrize("up", ["y", "z"])
def test_frame_cameras_keep_every_vertex_inside_the_margin(up):
    import math
    rs = np.random.RandomState(5)
    v = (rs.randn(4, 500, 3) * np.array([0.3, 0.9, 0.2]) + np.array([0.4, -0.2, 1.0])).astype(np.float32)
    fov, margin = 35.0, 0.1
    eyes, ats, near, far = preview.frame_cameras(torch.from_numpy(v), n_views=7, elevation=20.0, up=up, fov=fov, margin=margin)
    assert eyes.shape == (7, 3) and ats.shape == (7, 3)
    cams = preview.look_frames(eyes, ats, up).astype(np.float64)
    width = math.tan(math.radians(fov) * 0.5)
    u = np.asarray(preview._UP[up])
    for cam in cams:
        d = v.reshape(-1, 3) - cam[:3]
        cx, cy, cz = d @ cam[3:6], d @ cam[6:9], d @ cam[9:12]
        assert cz.min() > near and cz.max() < far
        assert np.abs(cx / cz / width).max() <= 1 - margin + 1e-6 and np.abs(cy / cz / width).max() <= 1 - margin + 1e-6
        assert cam[6:9] @ u > 0.9                                    # upright
    h = (eyes - ats) @ u
    assert np.allclose(h, h[0]) and h[0] > 0                         # one circle, above the horizon
    r = np.linalg.norm(eyes - ats, axis=1)
    assert np.allclose(r, r[0])
    front = np.asarray(preview._FRONT[up])
    assert (eyes[0] - ats[0]) @ front > 0.9 * r[0] * math.cos(math.radians(20.0))   # view 0 stands in front of the avatar


# ---------------------------------------------------------------------------------------------------------------- sources
def test_pc2_round_trip_into_the_source(tmp_path):
    v, t, c = PS.icosphere()
    rs = np.random.RandomState(0)
    frames = (v[None] + rs.randn(5, 1, 3).astype(np.float32) * 0.1).astype(np.float32)
    ply, pc2 = str(tmp_path / "a.ply"), str(tmp_path / "m.pc2")
    mesh.write_ply(ply, v, t, c)
    drive.write_pc2(pc2, list(frames))
    fv, ft, fc, moving = preview.mesh_source(ply, pc2)
    assert moving and fv.dtype == np.float32 and np.array_equal(fv, frames) and np.array_equal(ft, t) and np.array_equal(fc, c)
    assert np.array_equal(preview.mesh_source(ply, pc2, every=2)[0], frames[::2])
    sv, _, _, moving = preview.mesh_source(ply)
    assert not moving and np.array_equal(sv, v[None])


def _blend_reference(joints, weights, mats, rest):
    """torch: out[t,m] = sum_s sum_k w[s,m,k] (mats[t, j[s,m,k]] (rest[m], 1))"""
    j = torch.as_tensor(joints).long()
    w = torch.as_tensor(weights).double()
    rest1 = torch.cat([torch.as_tensor(rest).double(), torch.ones(len(rest), 1, dtype=torch.float64)], 1)
    per = torch.einsum("tsmkrc,mc->tsmkr", mats.double()[:, j], rest1)
    return torch.einsum("smk,tsmkr->tmr", w, per)


def test_glb_playback_of_the_two_bone_strip(tmp_path):
    g = rig.read_glb(PS.write_strip_glb(str(tmp_path / "strip.glb")))
    rest, t, c, joints, weights = preview.glb_skin(g)
    assert np.array_equal(rest, PS.STRIP_V) and np.array_equal(t, PS.STRIP_T) and np.array_equal(c, PS.STRIP_C)
    mats, times = preview.glb_joint_matrices(g)
    assert mats.shape == (3, 2, 3, 4) and np.allclose(times, np.arange(3) / 30.0)
    got = _blend_reference(joints, weights, mats, rest).numpy()
    assert np.abs(got - PS.strip_expected()).max() < 1e-6
    assert np.abs(got[0] - PS.STRIP_V).max() < 1e-7
    assert np.allclose(got[2, 4], [0.1, 0.0, 0.0], atol=1e-6)       # the tip folded back onto the root
    # without a track: the rest pose, one frame
    g0 = rig.read_glb(PS.write_strip_glb(str(tmp_path / "rest.glb"), animated=False))
    mats0, _ = preview.glb_joint_matrices(g0)
    assert mats0.shape == (1, 2, 3, 4)
    assert np.abs(_blend_reference(joints, weights, mats0, rest).numpy()[0] - PS.STRIP_V).max() < 1e-7
    assert np.array_equal(preview.glb_joint_matrices(g, every=2)[1], times[::2])


# ---------------------------------------------------------------------------------------------------------------- the command line
def test_cli_refusals(tmp_path):
    v, t, c = PS.icosphere()
    ply, pc2, glb, out = (str(tmp_path / n) for n in ("a.ply", "m.pc2", "s.glb", "o.gif"))
    mesh.write_ply(ply, v, t, c)
    drive.write_pc2(pc2, [v[:-1], v[:-1]])
    PS.write_strip_glb(glb)
    for argv in (["--mesh", ply, "--glb", glb, "--out", out],                   # both sources
                 ["--out", out],                                                # neither
                 ["--pc2", pc2, "--glb", glb, "--out", out],                    # a point cache without its mesh
                 ["--mesh", ply, "--pc2", pc2, "--out", out],                   # 161 vertices per frame against 162
                 ["--mesh", ply, "--out", out, "--size", "1025", "--ss", "2"],  # a 2050 raster: above the kernel's limit
                 ["--mesh", ply, "--out", out, "--size", "2049", "--ss", "1"],
                 ["--mesh", ply, "--out", out, "--ss", "3"],
                 ["--mesh", ply, "--out", str(tmp_path / "o.mp4")],
                 ["--mesh", ply, "--out", out, "--up", "x"],
                 ["--mesh", ply]):
        with pytest.raises(SystemExit) as e:
            preview.main(argv)
        assert e.value.code not in (0, None), argv
    assert not os.path.exists(out)
    assert preview.MAX_RASTER == PR.MAX_RASTER == 2048
    with pytest.raises(ValueError):
        preview.check_raster(1025, 2)
    preview.check_raster(1024, 2)
