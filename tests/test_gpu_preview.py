"""The preview renderer on the device (csrc/avc_preview.hip through avatarclip_amd/preview.py) against tests/preview_restatement.py: the
winning face of every pixel with no tolerance (integer coverage and depth), the uint8 image within one level (float32 against float64
interpolation: only a rounding boundary can differ), the large-face path, batching, edge inputs, the four-influence skinning and the
command line end to end.  The scenes are tests/preview_scenes.py's; tests/test_preview_cpu.py checks that they hold what is relied on here."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import drive_standins as S
from tests import preview_restatement as PR
from tests import preview_scenes as PS

pytestmark = pytest.mark.gpu
DEV = "cuda"
AMBIENT, BG = 0.4, (255, 250, 240)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drive.npz")


@functools.lru_cache(maxsize=None)
def _scene(name):
    return getattr(PS, name)()


@functools.lru_cache(maxsize=None)
def _reference(name, size, ss, colored=True):
    """the restatement's (image, face ids) of a scene: computed once, shared, never written to"""
    from avatarclip_amd import preview
    sc = _scene(name)
    cam = preview.look_frames(sc["eye"], sc["at"], "y")[0]
    img, ids = PR.render(sc["v"], sc["t"], sc["c"] if colored else None, cam, math.tan(math.radians(sc["fov"]) * 0.5), sc["near"], sc["far"],
                         sc["at"] - sc["eye"], AMBIENT, BG, size, ss, grey=preview.GREY)
    img.setflags(write=False)
    ids.setflags(write=False)
    return img, ids


def _render(sc, size, ss, colors="own", **kw):
    from avatarclip_amd import preview
    c = sc["c"] if isinstance(colors, str) else colors
    img, ids = preview.render_frames(sc["v"], sc["t"], c, eyes=sc["eye"], ats=sc["at"], up="y", fov=sc["fov"], image_size=size, ss=ss,
                                     ambient=AMBIENT, background=BG, near=sc["near"], far=sc["far"], return_face_ids=True, **kw)
    torch.cuda.synchronize()
    return img.cpu().numpy(), ids.cpu().numpy()


def _worst(a, b):
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max())


# ---------------------------------------------------------------------------------------------------------------- 1-3: coverage, depth, colour
def test_face_ids_of_random_triangles_are_exact():
    img, ids = _render(_scene("random_triangles"), 64, 1)
    ref_img, ref_ids = _reference("random_triangles", 64, 1)
    assert ids.shape == (1, 64, 64) and np.array_equal(ids[0], ref_ids)
    assert (ids == -1).any() and not np.isin(ids, np.arange(290, 300)).any()        # background; a copy never beats its original
    assert _worst(img[0], ref_img) <= 1


def test_sheet_is_watertight():
    img, ids = _render(_scene("sheet"), 64, 1)
    ref_img, ref_ids = _reference("sheet", 64, 1)
    assert (ids >= 0).all() and np.array_equal(ids[0], ref_ids)
    assert _worst(img[0], ref_img) <= 1


@pytest.mark.parametrize("name,size,ss", [("random_triangles", 64, 1), ("random_triangles", 64, 2), ("sheet", 64, 2), ("random_triangles", 33, 2),
                                          ("sheet", 33, 2)])
def test_colours_and_shading(name, size, ss):
    """33 at ss = 2: a 66^2 raster, no multiple of the 16-pixel tile or of a wavefront"""
    img, ids = _render(_scene(name), size, ss)
    ref_img, ref_ids = _reference(name, size, ss)
    assert img.shape == (1, size, size, 3) and img.dtype == np.uint8
    assert np.array_equal(ids[0], ref_ids)
    worst = _worst(img[0], ref_img)
    print("%s %d x%d: worst |image - restatement| = %d levels, %d pixels differ" % (name, size, ss, worst, (img[0] != ref_img).any(-1).sum()))
    assert worst <= 1
    assert len(np.unique(img[0].reshape(-1, 3), axis=0)) > 100                      # colours are interpolated, not flat


# ---------------------------------------------------------------------------------------------------------------- 4: the large-face path
def test_large_face_behind_small_ones():
    from avatarclip_amd import preview
    sc = _scene("big_behind_small")
    scratch = torch.full((preview.scratch_bytes(len(sc["t"]), 256),), 255, device=DEV, dtype=torch.uint8)
    img, ids = _render(sc, 256, 1, scratch=scratch)
    ref_img, ref_ids = _reference("big_behind_small", 256, 1)
    assert np.array_equal(ids[0], ref_ids) and (ids >= 0).all() and (ids == 0).sum() > 256 * 256 // 2
    assert _worst(img[0], ref_img) <= 1
    assert bool((scratch == 255).all())
    img2, ids2 = _render(sc, 256, 1, scratch=scratch)                                # the scratch it handed back serves the next call
    assert np.array_equal(ids2, ids) and np.array_equal(img2, img) and bool((scratch == 255).all())


def test_guard_band_corners_at_the_largest_raster():
    """the int64 bound of csrc/avc_preview.hip at its edge: a 2048^2 raster, corners on the guard band's corners (the widest differences
    the projection can emit), depths at both ends of the 24 bits.  Two view-filling triangles whose depth ramps run against each other cross
    along a line, so the face-id image is decided by the depth arithmetic at every pixel; it equals the restatement (whose products are
    checked in Python integers) exactly.  The projected vertices are handed to avc_preview_raster directly."""
    from avatarclip_amd import lib as L
    R, lo, hi, zmax = PR.MAX_RASTER, -PR.GUARD, PR.MAX_RASTER * 256 + PR.GUARD, PR.ZMAX
    X = np.array([lo, hi, lo, lo, hi, lo, hi, hi, lo], np.int64)
    Y = np.array([lo, lo, hi, lo, lo, hi, hi, lo, hi], np.int64)
    Z = np.array([0, zmax, zmax, zmax, 0, 0, 5, zmax - 7, 3], np.int64)
    tris = np.array([[0, 1, 2], [3, 5, 4], [6, 7, 8]], np.int32)             # the second one the other way round
    ref = PR.face_ids(PR.rasterize(X, Y, Z, tris, R))
    assert (ref >= 0).all() and all((ref == f).sum() > R * R // 20 for f in range(3))
    lib, s = L.load(), L.stream()
    proj = torch.from_numpy(np.stack([X, Y, Z, np.full(9, np.float32(1).view(np.int32))], 1).astype(np.int32)).to(DEV)
    t = torch.from_numpy(tris).to(DEV)
    nbytes = lib.avc_preview_scratch_bytes(3, R)
    assert nbytes == R * R * 8 + 24 and lib.avc_preview_scratch_bytes(3, R + 1) == -1
    scratch = torch.full((nbytes,), 255, device=DEV, dtype=torch.uint8)
    v = torch.zeros(9, 3, device=DEV)
    light = torch.ones(1, 3, device=DEV)
    img = torch.empty(1, R, R, 3, device=DEV, dtype=torch.uint8)
    ids = torch.empty(1, R, R, device=DEV, dtype=torch.int32)
    L.check(lib.avc_preview_raster(L.ptr(proj), 1, 9, L.ptr(t), 3, R, L.ptr(scratch), s), "avc_preview_raster")
    L.check(lib.avc_preview_shade(L.ptr(proj), L.ptr(v), 1, 9, L.ptr(t), 3, None, 0, L.ptr(light), 0.5, 0.0, 0.0, 0.0, 200.0, R, 1, L.ptr(scratch),
                                  L.ptr(img), L.ptr(ids), s), "avc_preview_shade")
    assert np.array_equal(ids[0].cpu().numpy(), ref)
    assert bool((scratch == 255).all()) and bool((img == 100).all())          # no normal (v = 0): ambient alone, 0.5 x the grey 200
    assert lib.avc_preview_raster(L.ptr(proj), 1, 9, L.ptr(t), 3, R + 1, L.ptr(scratch), s) != 0      # a larger raster is refused


# ---------------------------------------------------------------------------------------------------------------- 5: batches
def test_batch_equals_single_frames_bit_for_bit():
    from avatarclip_amd import preview
    sc = _scene("random_triangles")
    rs = np.random.RandomState(7)
    v = np.stack([sc["v"], sc["v"] + rs.uniform(-0.05, 0.05, sc["v"].shape).astype(np.float32), sc["v"][:, [1, 0, 2]] * np.float32(0.9)])
    eyes = np.array([[0, 0, 3.0], [0.4, 0.2, 2.9], [-0.5, 0.1, 3.1]])
    ats = np.array([[0, 0, 0.0], [0.05, 0, 0], [0, -0.05, 0]])
    kw = dict(up="y", fov=sc["fov"], image_size=48, ss=2, ambient=AMBIENT, background=BG, near=1.0, far=5.0, return_face_ids=True)
    img, ids = preview.render_frames(v, sc["t"], sc["c"], eyes=eyes, ats=ats, **kw)
    img_again, ids_again = preview.render_frames(v, sc["t"], sc["c"], eyes=eyes, ats=ats, **kw)
    assert torch.equal(img, img_again) and torch.equal(ids, ids_again)
    chunked, _ = preview.render_frames(v, sc["t"], sc["c"], eyes=eyes, ats=ats, chunk_bytes=1, **kw)     # one frame per chunk
    assert torch.equal(img, chunked)
    for i in range(3):
        one, one_ids = preview.render_frames(v[i], sc["t"], sc["c"], eyes=eyes[i], ats=ats[i], **kw)
        assert torch.equal(one[0], img[i]) and torch.equal(one_ids[0], ids[i])
    assert not torch.equal(img[0], img[1]) and not torch.equal(img[0], img[2])


# ---------------------------------------------------------------------------------------------------------------- 6: edge inputs
def test_edge_inputs():
    from avatarclip_amd import preview
    sc = _scene("random_triangles")
    kw = dict(eyes=sc["eye"], ats=sc["at"], up="y", fov=sc["fov"], image_size=32, ss=2, ambient=AMBIENT, background=BG, near=sc["near"], far=sc["far"],
              return_face_ids=True)
    bg = torch.tensor(BG, dtype=torch.uint8)
    # no faces: the background everywhere
    img, ids = preview.render_frames(sc["v"], np.zeros((0, 3), np.int32), sc["c"], **kw)
    assert bool((ids == -1).all()) and bool((img.cpu() == bg).all())
    # zero-area faces (a repeated corner, three collinear points) among good ones draw nothing themselves
    v = np.concatenate([sc["v"], np.array([[-0.5, 0, 0.2], [0, 0, 0.2], [0.5, 0, 0.2]], np.float32)])
    n = len(sc["v"])
    t = np.concatenate([np.array([[0, 0, 1], [n, n + 1, n + 2], [5, 5, 5]], np.int32), sc["t"][:40]])
    c = np.concatenate([sc["c"], np.zeros((3, 3), np.uint8)])
    img, ids = preview.render_frames(v, t, c, **kw)
    cam = preview.look_frames(sc["eye"], sc["at"], "y")[0]
    ref_img, ref_ids = PR.render(v, t, c, cam, math.tan(math.radians(sc["fov"]) * 0.5), sc["near"], sc["far"], sc["at"] - sc["eye"], AMBIENT, BG, 32, 2)
    assert np.array_equal(ids[0].cpu().numpy(), ref_ids) and not np.isin(ref_ids, [0, 1, 2]).any() and (ref_ids >= 3).any()
    assert _worst(img[0].cpu().numpy(), ref_img) <= 1
    # one vertex behind the camera: its faces are dropped, the rest is drawn
    v = sc["v"].copy()
    v[sc["t"][3, 0]] = (0.0, 0.0, 3.5)
    hit = (sc["t"] == sc["t"][3, 0]).any(1)
    img, ids = preview.render_frames(v, sc["t"], sc["c"], **kw)
    ref_img, ref_ids = PR.render(v, sc["t"], sc["c"], cam, math.tan(math.radians(sc["fov"]) * 0.5), sc["near"], sc["far"], sc["at"] - sc["eye"], AMBIENT,
                                 BG, 32, 2)
    ids = ids[0].cpu().numpy()
    assert np.array_equal(ids, ref_ids) and not np.isin(ids, np.nonzero(hit)[0]).any() and (ids >= 0).sum() > 1000
    assert _worst(img[0].cpu().numpy(), ref_img) <= 1
    # no colours: a constant grey, shaded; RGBA colours: the alpha is ignored
    img, ids = preview.render_frames(sc["v"], sc["t"], None, **kw)
    ref_img, ref_ids = _reference("random_triangles", 32, 2, colored=False)
    assert np.array_equal(ids[0].cpu().numpy(), ref_ids) and _worst(img[0].cpu().numpy(), ref_img) <= 1
    rgb, _ = preview.render_frames(sc["v"], sc["t"], sc["c"], **kw)
    rgba, _ = preview.render_frames(sc["v"], sc["t"], np.concatenate([sc["c"], np.full((len(sc["c"]), 1), 7, np.uint8)], 1), **kw)
    assert torch.equal(rgb, rgba)
    torch.cuda.synchronize()
    # what the host side refuses
    for bad in (dict(image_size=1025, ss=2), dict(ss=3)):
        with pytest.raises(ValueError):
            preview.render_frames(sc["v"], sc["t"], sc["c"], **{**kw, **bad})
    with pytest.raises(ValueError):
        preview.render_frames(sc["v"], sc["t"] + 1000, sc["c"], **kw)
    assert preview.scratch_bytes(10, 2049) == -1


# ---------------------------------------------------------------------------------------------------------------- 7: skinning
def test_skin_blend4_against_einsum():
    from avatarclip_amd import preview
    M, J, T = 1000, 24, 3
    rs = np.random.RandomState(11)
    joints = rs.randint(0, J, (M, 4)).astype(np.uint8)
    w = rs.uniform(0, 1, (M, 4)).astype(np.float32)
    w[rs.uniform(size=(M, 4)) < 0.3] = 0                                             # some influences unused
    w[:, 0] += (w.sum(1) == 0)
    w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    rest = rs.uniform(-1, 1, (M, 3)).astype(np.float32)
    rot, _ = np.linalg.qr(rs.randn(T, J, 3, 3))
    mats = np.concatenate([rot, rs.uniform(-0.5, 0.5, (T, J, 3, 1))], 3).astype(np.float32)
    out = preview.skin_blend4(joints, w, mats, rest)
    assert out.shape == (T, M, 3) and out.dtype == torch.float32
    rest1 = torch.cat([torch.from_numpy(rest).double(), torch.ones(M, 1, dtype=torch.float64)], 1)
    ref = torch.einsum("mk,tmkrc,mc->tmr", torch.from_numpy(w).double(), torch.from_numpy(mats).double()[:, torch.from_numpy(joints).long()], rest1)
    err = (out.cpu().double() - ref).abs().max().item()
    print("avc_skin_blend4: worst |out - einsum| = %.3e" % err)
    assert err < 1e-5
    two = preview.skin_blend4(np.stack([joints, joints]), np.stack([w * np.float32(0.5), w * np.float32(0.5)]), mats, rest)   # two sets of four
    assert (two.cpu().double() - ref).abs().max().item() < 1e-5
    with pytest.raises(ValueError):
        preview.skin_blend4(joints, w, mats[:, :20], rest)


# ---------------------------------------------------------------------------------------------------------------- 8: end to end
def _gif(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.n_frames, im.size


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"))


def test_cli_on_a_mesh_a_point_cache_and_a_glb(tmp_path, capsys):
    from avatarclip_amd import drive, mesh, preview
    d = str(tmp_path)
    v, t, c = PS.icosphere()
    assert len(t) == 320
    ply, pc2 = os.path.join(d, "ico.ply"), os.path.join(d, "ico.pc2")
    mesh.write_ply(ply, v, t, c)
    preview.main(["--mesh", ply, "--out", os.path.join(d, "turn.gif"), "--views", "4", "--size", "64"])
    assert _gif(os.path.join(d, "turn.gif")) == (4, (64, 64))
    assert capsys.readouterr().out.strip() == os.path.join(d, "turn.gif")
    drive.write_pc2(pc2, [v + np.float32(0.1 * k) * np.array([1, 0, 1], np.float32) for k in range(3)])
    preview.main(["--mesh", ply, "--pc2", pc2, "--out", os.path.join(d, "play.gif"), "--size", "64", "--frames-dir", os.path.join(d, "play")])
    assert _gif(os.path.join(d, "play.gif")) == (3, (64, 64)) and sorted(os.listdir(os.path.join(d, "play"))) == ["0000.png", "0001.png", "0002.png"]
    first = _png(os.path.join(d, "play", "0000.png"))
    assert (first != 255).any() and not np.array_equal(first, _png(os.path.join(d, "play", "0002.png")))
    preview.main(["--mesh", ply, "--out", os.path.join(d, "one.png"), "--size", "64", "--ss", "1"])
    assert _png(os.path.join(d, "one.png")).shape == (64, 64, 3)
    # the strip: its played track, and the rest pose against render_frames on the rest mesh
    preview.main(["--glb", PS.write_strip_glb(os.path.join(d, "strip.glb")), "--out", os.path.join(d, "strip.gif"), "--size", "64", "--orbit"])
    assert _gif(os.path.join(d, "strip.gif")) == (3, (64, 64))
    preview.main(["--glb", PS.write_strip_glb(os.path.join(d, "rest.glb"), animated=False), "--out", os.path.join(d, "rest.gif"), "--views", "4",
                  "--size", "64", "--frames-dir", os.path.join(d, "rest")])
    eyes, ats, near, far = preview.frame_cameras(torch.from_numpy(PS.STRIP_V), 4, 10.0, "y", 40.0, 0.05)
    expect = preview.render_frames(PS.STRIP_V, PS.STRIP_T, PS.STRIP_C, eyes, ats, up="y", fov=40.0, image_size=64, ss=2, near=near, far=far).cpu().numpy()
    for k in range(4):
        assert np.array_equal(_png(os.path.join(d, "rest", "%04d.png" % k)), expect[k])
    assert (expect[0] != 255).any(-1).sum() > 100                                    # the strip is there: upright, 2 units tall
    rows = np.nonzero((expect[0] != 255).any(-1).any(1))[0]
    top, bottom = expect[0][rows[0] + 1], expect[0][rows[-1] - 1]
    assert top[(top != 255).any(-1)][:, 2].mean() > 100 and bottom[(bottom != 255).any(-1)][:, 0].mean() > 100   # blue end up, red end down


def _write_inputs(d, res=24, frames=3):
    from avatarclip_amd import mesh
    v, t, c = S.avatar_mesh(res)
    mesh.write_ply(os.path.join(d, "avatar.ply"), v, t, c)
    np.save(os.path.join(d, "action.npy"), S.motion(frames))
    np.save(os.path.join(d, "stand_pose.npy"), np.load(GOLD)["stand_pose"])
    a = S.template_arrays()
    np.savez(os.path.join(d, "smpl.npz"), v_template=a["v_template"].numpy(), posedirs=a["posedirs"].numpy(), J_regressor=a["J_regressor"].numpy(),
             parents=a["parents"].numpy(), lbs_weights=a["lbs_weights"].numpy(), faces=np.zeros((1, 3), np.int32))
    return [os.path.join(d, n) for n in ("avatar.ply", "action.npy", "smpl.npz", "stand_pose.npy")]


def test_drive_and_rig_preview_flag(tmp_path):
    from avatarclip_amd import drive, rig
    d = str(tmp_path)
    ply, motion, smpl, pose = _write_inputs(d)
    base = ["--mesh", ply, "--motion", motion, "--smpl", smpl, "--pose_npy", pose]
    drive.main(base + ["--out_dir", os.path.join(d, "drive0")])
    assert sorted(os.listdir(os.path.join(d, "drive0"))) == ["General_cleaned_apose.ply", "action.pc2"]
    drive.main(base + ["--out_dir", os.path.join(d, "drive1"), "--preview"])
    assert sorted(os.listdir(os.path.join(d, "drive1"))) == ["General_cleaned_apose.ply", "General_preview.gif", "action.pc2"]
    assert _gif(os.path.join(d, "drive1", "General_preview.gif")) == (3, (512, 512))
    rbase = base + ["--name", "fixture", "--voxel_divisor", "32"]
    rig.main(rbase + ["--out_dir", os.path.join(d, "rig0")])
    assert sorted(os.listdir(os.path.join(d, "rig0"))) == ["fixture.glb", "fixture_rig.npz"]
    rig.main(rbase + ["--out_dir", os.path.join(d, "rig1"), "--preview"])
    assert sorted(os.listdir(os.path.join(d, "rig1"))) == ["fixture.glb", "fixture_preview.gif", "fixture_rig.npz"]
    assert _gif(os.path.join(d, "rig1", "fixture_preview.gif")) == (3, (512, 512))
