"""The preview renderer's frustum clipper without a GPU: tests/preview_clip_restatement.py (the numpy statement of the rules of
csrc/avc_preview_clip.h) against tests/preview_restatement.py where no face is clipped, on the ground-sheet fixture the rules were checked
on, at the edges of the rules (a corner exactly on the near plane, a face behind the camera, a face with no valid corner, the widened
int64 bound), the close-up framing of preview.frame_cameras(focus=...) and the binding of the fourth header."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from avatarclip_amd import preview
from tests import preview_clip_restatement as PC
from tests import preview_restatement as PR
from tests import preview_scenes as PS

AMBIENT, BG = 0.4, (255, 250, 240)


def ground_sheet():
    """preview_scenes.sheet(n = 9) laid flat and scaled by 4 (the plane y = 0, +-5.2), seen from 0.3 above it along -z: faces cross the
    near plane, both sides and the far plane at once"""
    sc = PS.sheet(n=9)
    return dict(sc, v=np.ascontiguousarray(sc["v"][:, [0, 2, 1]] * np.float32(4)), eye=np.array([0.0, 0.3, 0.0]), at=np.array([0.0, 0.3, -1.0]),
                fov=PS.FOV, near=0.05, far=4.0)


def view_filling(scale=100.0):
    """big_behind_small with face 0 replaced by a triangle whose three corners all lie beyond the guard band"""
    sc = PS.big_behind_small()
    v = sc["v"].copy()
    v[:3] = np.array([[-4.0, -3.0, -0.5 / scale], [4.0, -3.0, -0.5 / scale], [0.0, 5.0, -0.5 / scale]], np.float32) * np.float32(scale)
    return dict(sc, v=v)


def _cam(sc):
    return preview.look_frames(sc["eye"], sc["at"], "y")[0]


def _width(sc):
    return math.tan(math.radians(sc["fov"]) * 0.5)


def _raster(sc, R, clip=True, order=None, **kw):
    near, far = kw.get("near", sc["near"]), kw.get("far", sc["far"])
    return PC.rasterize(sc["v"], _cam(sc), _width(sc), near, far, sc["t"], R, order=order, clip=clip)


@functools.lru_cache(maxsize=None)
def _ground(R):
    key, fans, X, Y, Z, _ = _raster(ground_sheet(), R)
    key.setflags(write=False)
    return key, fans, (X, Y, Z)


# ---------------------------------------------------------------------------------------------------------------- no face clipped
@pytest.mark.parametrize("name", ["random_triangles", "sheet", "big_behind_small"])
def test_equal_to_the_unclipped_restatement_where_every_corner_is_valid(name):
    sc = getattr(PS, name)()
    args = (sc["v"], sc["t"], sc["c"], _cam(sc), _width(sc), sc["near"], sc["far"], sc["at"] - sc["eye"], AMBIENT, BG, 64, 1)
    img, ids = PC.render(*args)
    ref_img, ref_ids = PR.render(*args)
    assert np.array_equal(ids, ref_ids) and np.array_equal(img, ref_img)
    assert not _raster(sc, 64)[1]                                      # no face met the clipper
    off_img, off_ids = PC.render(*args, clip=False)
    assert np.array_equal(off_ids, ref_ids) and np.array_equal(off_img, ref_img)


# ---------------------------------------------------------------------------------------------------------------- the ground sheet
@pytest.mark.parametrize("R,first_row", [(64, 39), (128, 77)])
def test_ground_sheet_is_covered_once_and_without_holes(R, first_row):
    sc = ground_sheet()
    key, fans, (X, Y, Z) = _ground(R)
    ids = PR.face_ids(key)
    assert (ids[first_row:] >= 0).all()                                # every pixel below the horizon
    rows = np.nonzero((ids >= 0).any(1))[0]
    assert (ids[rows[0]:rows[-1] + 1] >= 0).any(1).all() and rows[-1] == R - 1
    for r in range(rows[0], R):                                        # no hole inside a row either
        cols = np.nonzero(ids[r] >= 0)[0]
        assert (ids[r, cols[0]:cols[-1] + 1] >= 0).all()
    # at most one face per pixel: the untouched faces and every sub-triangle of every fan, counted
    n = PR.coverage_count(X, Y, Z, sc["t"], R)
    owner = np.where(n > 0, ids, -1)
    for f, fan in fans.items():
        mine = np.zeros((R, R), bool)
        for _, _, xs, ys, _, cov, _ in PC._fan_keys(fan, f, R):
            mine[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] |= cov            # (a face's own sub-triangles may meet; another face may not)
        assert not (mine & (owner >= 0) & (owner != f)).any()
        owner[mine] = f
        n += mine
    assert n.max() == 1 and np.array_equal(n > 0, ids >= 0)
    unclipped = PR.rasterize(X, Y, Z, sc["t"], R)
    assert (unclipped != PR.EMPTY).sum() < (ids >= 0).sum()
    if R == 64:
        assert sum(len(fan[0]) >= 3 for fan in fans.values()) == 36 and (unclipped != PR.EMPTY).sum() == 696 and (ids >= 0).sum() >= 1600
    img, ids2 = PC.render(sc["v"], sc["t"], sc["c"], _cam(sc), _width(sc), sc["near"], sc["far"], sc["at"] - sc["eye"], AMBIENT, BG, R, 1)
    assert np.array_equal(ids2, ids) and (img[first_row:] != np.asarray(BG, np.uint8)).any(-1).all()


def test_the_result_does_not_depend_on_face_order():
    sc = ground_sheet()
    key = _ground(64)[0]
    F = len(sc["t"])
    assert np.array_equal(key, _raster(sc, 64, order=range(F - 1, -1, -1))[0])
    assert np.array_equal(key, _raster(sc, 64, order=np.random.RandomState(3).permutation(F))[0])
    rt = PS.random_triangles()
    a = _raster(rt, 64, near=2.9, far=3.2)
    assert sum(len(fan[0]) >= 3 for fan in a[1].values()) == 164       # faces that cross a plane and leave something
    assert np.array_equal(a[0], _raster(rt, 64, near=2.9, far=3.2, order=range(len(rt["t"]) - 1, -1, -1))[0])


def test_a_shared_edge_is_cut_at_the_same_bits_from_both_sides():
    """two faces that share an edge crossing the near plane walk it in opposite directions; the intersection runs from the inside end to
    the outside end either way, so both get the same point"""
    a, b = (0.01, -0.01, 0.02), (-0.04, 0.05, 0.9)
    one = PC.clip_polygon([a, b, (0.5, 0.5, 0.5)], 0.4, 0.05, 4.0, 64)
    two = PC.clip_polygon([b, a, (-0.5, -0.5, 0.5)], 0.4, 0.05, 4.0, 64)
    cut = lambda poly: [u[:3] for u, corner in poly if corner < 0 and u[2] == 0.05]
    assert any(p == q for p in cut(one) for q in cut(two))
    assert all(sum(u[3:]) == pytest.approx(1.0, abs=1e-12) for u, _ in one + two)


# ---------------------------------------------------------------------------------------------------------------- the edges of the rules
def _one_face(v, near=0.5, far=4.0, R=32):
    sc = dict(v=np.asarray(v, np.float32), t=np.array([[0, 1, 2]], np.int32), eye=np.zeros(3), at=np.array([0.0, 0.0, -1.0]), fov=60.0, near=near, far=far)
    return sc, _raster(sc, R), _raster(sc, R, clip=False)


def test_a_corner_exactly_on_the_near_plane():
    sc, (key, fans, X, Y, Z, _), (plain, _, _, _, _, _) = _one_face([[0, 0, -0.5], [0.3, 0.1, -1.0], [-0.1, 0.4, -1.0]])
    cz = PC.camera_points(sc["v"], _cam(sc))[:, 2]
    assert cz[0] == 0.5 and Z[0] == -1 and Z[1] >= 0 and Z[2] >= 0      # invalid for the projection (c_z > near fails) ...
    poly = PC.clip_polygon(PC.camera_points(sc["v"], _cam(sc)), np.float32(_width(sc)), 0.5, 4.0, 32)
    assert [corner for _, corner in poly] == [0, 1, 2]                 # ... inside for the clipper (d = 0): no intersection is made
    assert fans[0][2][0] == 0 and (fans[0][0][1:] == X[1:]).all()      # snapped to depth 0; the valid corners keep their entries
    assert (plain == PR.EMPTY).all() and (key != PR.EMPTY).sum() > 20 and (PR.face_ids(key) <= 0).all()


def test_a_face_behind_the_camera_draws_nothing():
    _, (key, fans, _, _, Z, _), _ = _one_face([[0, 0, 0.5], [0.3, 0.1, 1.0], [-0.1, 0.4, 2.0]])
    assert (Z == -1).all() and len(fans[0][0]) == 0 and (key == PR.EMPTY).all()
    _, (key, fans, _, _, _, _), _ = _one_face([[0, 0, -0.6], [np.inf, 0.1, -1.0], [-0.1, 0.4, -1.0]])
    assert not fans and (key == PR.EMPTY).all()                        # a non-finite corner: dropped, not clipped


def test_a_face_with_no_valid_corner_covers_the_view():
    sc = view_filling()
    key, fans, _, _, Z, _ = _raster(sc, 64)
    ids = PR.face_ids(key)
    assert (Z[:3] == -1).all() and list(fans) == [0] and (ids >= 0).all() and (ids == 0).sum() > 64 * 64 // 2
    plain = PR.face_ids(_raster(sc, 64, clip=False)[0])
    assert not (plain == 0).any() and np.array_equal(plain[ids != 0], ids[ids != 0])


def test_the_int64_bound_on_clamped_corners_at_the_largest_raster():
    R = PR.MAX_RASTER
    lo, hi = -(PR.GUARD + PC.EXTRA), 256 * R + PR.GUARD + PC.EXTRA
    D = hi - lo
    assert D == (1 << 19) + (1 << 17) + 512 == 655872 and D < 1 << 20 and D * D == 430168080384 and D * D < 1 << 39
    assert D * D * PR.ZMAX < 1 << 63
    cam = preview.look_frames([0, 0, 0], [0, 0, -1], "y")[0]
    pts = []
    for swap in (False, True):                                         # the depth runs from before near to beyond far across x, then across y
        v = np.array([[-9.0, -7.0, 52.0], [9.0, -7.0, -56.0], [0.0, 11.0, -2.0]], np.float32)
        poly = PC.clip_polygon(PC.camera_points(v[:, [1, 0, 2]] if swap else v, cam), 0.5, 0.5, 4.0, R)
        assert len(poly) >= 4
        pts += [PC.snap(u, 0.5, 0.5, 4.0, R) for u, _ in poly]
    xs, ys, zs = ([p[k] for p in pts] for k in range(3))
    assert min(xs) == lo and max(xs) == hi and min(ys) == lo and max(ys) == hi      # the widened corners are reached
    assert min(zs) == 0 and max(zs) == PR.ZMAX
    for a in range(len(pts)):                                          # every product of the edge functions, in Python integers
        for b in range(len(pts)):
            for px, py in ((128, 128), (256 * R - 128, 256 * R - 128), (128, 256 * R - 128)):
                dx, dy = xs[b] - xs[a], ys[b] - ys[a]
                assert abs(dx) < 1 << 20 and abs(dy) < 1 << 20
                assert abs(dx * (py - ys[a])) <= D * D and abs(dy * (px - xs[a])) <= D * D and abs(dx * (py - ys[a]) - dy * (px - xs[a])) <= D * D
    Xl, Yl = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    o = PR.orient(Xl, Yl, np.asarray(zs, np.int64), (0, 1, 2))
    assert o is not None and o[1] <= D * D and o[1] * PR.ZMAX < 1 << 63


# ---------------------------------------------------------------------------------------------------------------- close-up framing
@pytest.mark.parametrize("up", ["y", "z"])
def test_focus_frames_the_band_and_keeps_the_whole_mesh_in_depth(up):
    rs = np.random.RandomState(5)
    axis = 1 if up == "y" else 2
    v = (rs.rand(2, 800, 3) * 0.4 - 0.2).astype(np.float32)
    v[..., axis] = rs.rand(2, 800) * 2.0 - 1.0                          # a 2-unit-tall column
    fov, margin, focus = 35.0, 0.1, (0.84, 1.0)
    eyes, ats, near, far = preview.frame_cameras(torch.from_numpy(v), n_views=5, elevation=15.0, up=up, fov=fov, margin=margin, focus=focus)
    h = v.reshape(-1, 3)[:, axis]
    band = v.reshape(-1, 3)[(h >= h.min() + 0.84 * (h.max() - h.min()))]
    assert 0 < len(band) < 0.3 * h.size
    ctr = (band.min(0).astype(np.float64) + band.max(0)) * 0.5
    assert np.allclose(ats, ctr[None], atol=1e-6)
    width = math.tan(math.radians(fov) * 0.5)
    for cam in preview.look_frames(eyes, ats, up).astype(np.float64):
        d = band - cam[:3]
        cx, cy, cz = d @ cam[3:6], d @ cam[6:9], d @ cam[9:12]
        assert np.abs(cx / cz / width).max() <= 1 - margin + 1e-6 and np.abs(cy / cz / width).max() <= 1 - margin + 1e-6
        cz_all = (v.reshape(-1, 3) - cam[:3]) @ cam[9:12]
        assert cz_all.max() < far and near > 0
        assert (np.abs(((v.reshape(-1, 3) - cam[:3]) @ cam[6:9]) / np.maximum(cz_all, 1e-9) / width) > 1).any()    # the rest runs out of the picture
    assert (near, far) == preview.depth_range(torch.from_numpy(v), eyes) and near >= far * 1e-3
    whole = preview.frame_cameras(torch.from_numpy(v), n_views=5, elevation=15.0, up=up, fov=fov, margin=margin)
    assert np.linalg.norm(eyes[0] - ats[0]) < 0.5 * np.linalg.norm(whole[0][0] - whole[1][0])


def test_the_head_band_of_a_two_unit_strip_needs_the_clipper():
    eyes, ats, near, far = preview.frame_cameras(PS.STRIP_V, 4, 10.0, "y", 40.0, 0.05, focus=preview.FOCUS["head"])
    assert np.allclose(ats[0], [0, 2, 0])
    width = math.tan(math.radians(40.0) * 0.5)
    for cam in preview.look_frames(eyes, ats, "y")[::2]:              # front and back (from the side the flat strip is edge-on)
        assert (PR.project(PS.STRIP_V, cam, width, near, far, 1024)[2] < 0).any()      # (the command line's default raster, 512 x 2)
        key, fans, _, _, Z, _ = PC.rasterize(PS.STRIP_V, cam, width, near, far, PS.STRIP_T, 256)
        assert (Z < 0).any() and len(fans) >= 1                        # a face with an invalid corner: dropped without the clipper
        assert set(np.unique(PR.face_ids(key))) & set(fans)             # ... and it is in the picture with it
    assert (PR.face_ids(PC.rasterize(PS.STRIP_V, preview.look_frames(eyes, ats, "y")[0], width, near, far, PS.STRIP_T, 256)[0])[-1] >= 0).any()


def test_focus_refusals():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [1, 2, 0]], np.float32)
    with pytest.raises(ValueError, match="no vertex lies in the band"):
        preview.frame_cameras(v, focus=(0.4, 0.6))
    for bad in ((0.5, 0.5), (-0.1, 0.5), (0.2, 1.5), (0.9, 0.1)):
        with pytest.raises(ValueError):
            preview.frame_cameras(v, focus=bad)
    assert preview.parse_focus("head") == (0.84, 1.0) and preview.parse_focus("upper") == (0.5, 1.0) and preview.parse_focus("lower") == (0.0, 0.5)
    assert preview.parse_focus("0.25:0.75") == (0.25, 0.75)
    for bad in ("face", "0.5", "0.6:0.4", "a:b", "0:2"):
        with pytest.raises(ValueError):
            preview.parse_focus(bad)


def test_cli_refusals_of_the_close_up_options(tmp_path):
    from avatarclip_amd import mesh
    v, t, c = PS.icosphere()
    ply, out = str(tmp_path / "a.ply"), str(tmp_path / "o.png")
    mesh.write_ply(ply, v, t, c)
    for argv in (["--mesh", ply, "--out", out, "--eye", "0", "0", "3"],                                     # an eye without a target
                 ["--mesh", ply, "--out", out, "--at", "0", "0", "0"],
                 ["--mesh", ply, "--out", out, "--eye", "0", "0", "3", "--at", "0", "0", "0", "--focus", "head"],
                 ["--mesh", ply, "--out", out, "--focus", "nose"],
                 ["--mesh", ply, "--out", out, "--focus", "0.8:0.2"]):
        with pytest.raises(SystemExit) as e:
            preview.main(argv)
        assert e.value.code not in (0, None), argv
    assert not os.path.exists(out)


# ---------------------------------------------------------------------------------------------------------------- the binding
def test_the_fourth_header_parses_to_the_two_entry_points():
    from avatarclip_amd import build, lib
    protos, abi = lib.parse_header(open(lib.PREVIEW_CLIP_HEADER).read())
    assert abi is None and sorted(protos) == ["avc_preview_raster_clip", "avc_preview_shade_clip"]
    for name, p in protos.items():
        assert p.launch and p.restype is lib.c_int and p.params[-1] == lib.Param("stream", lib.c_void_p, "void*", "void", False), name
    assert [q.name for q in protos["avc_preview_raster_clip"].params] == ["proj", "v", "N", "V", "cams", "width", "near", "far", "tris", "F",
                                                                          "raster_size", "scratch", "stream"]
    grey, _ = lib.parse_header(open(lib.HEADER).read())
    plain = [q.name for q in grey["avc_preview_shade"].params]
    clipped = [q.name for q in protos["avc_preview_shade_clip"].params]
    assert [n for n in clipped if n not in ("cams", "width", "near", "far")] == plain       # what avc_preview_shade takes, plus the frustum
    assert lib.headers() == (lib.HEADER, lib.TEXTURE_HEADER, lib.CODEBOOK_HEADER) and lib.added_headers() == (lib.PREVIEW_CLIP_HEADER,)
    assert len(grey) == 81 and not set(grey) & set(protos)
    assert os.path.samefile(lib.PREVIEW_CLIP_HEADER, os.path.join(build.CSRC, build.PREVIEW_CLIP_HEADER))
    assert build.SOURCES[-1] == "avc_preview_clip.hip" and build.HEADERS[-2:] == ["avc_preview.h", build.PREVIEW_CLIP_HEADER]
    for name in ("avc_preview_clip.hip", "avc_preview.h", "avc_preview_clip.h"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    bound = lib.load()
    assert lib.ABI_VERSION == 4 and bound.avc_version() == 4
    for name in protos:
        assert name in lib._launches and len(getattr(bound, name).argtypes) == len(protos[name].params)


def test_a_name_the_fourth_header_declares_twice_is_refused(tmp_path, monkeypatch):
    from avatarclip_amd import lib
    dup = tmp_path / "dup.h"
    dup.write_text("int avc_kmeans_assign(const float* x, int N, void* stream);\n")
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "PREVIEW_CLIP_HEADER", str(dup))
    with pytest.raises(RuntimeError, match="declares avc_kmeans_assign, which .*avc_codebook.h declares already"):
        lib.load()


def test_a_library_without_the_entry_points_names_the_header(tmp_path, monkeypatch):
    from avatarclip_amd import lib
    more = tmp_path / "more.h"
    more.write_text(open(lib.PREVIEW_CLIP_HEADER).read().replace("avc_preview_raster_clip", "avc_preview_raster_clip_absent"))
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "PREVIEW_CLIP_HEADER", str(more))
    with pytest.raises(RuntimeError, match=r"lacks avc_preview_raster_clip_absent of csrc/more\.h: rebuild the library"):
        lib.load()
