"""The preview renderer's frustum clipper on the device (csrc/avc_preview_clip.hip through preview.render_frames(clip=True)) against
tests/preview_clip_restatement.py: in every case the winning face of EVERY pixel with no tolerance and the uint8 image within one level
(float32 against float64 interpolation: only a rounding boundary can differ; the worst difference and the count are printed).  The
fixtures are tests/test_preview_clip_cpu.py's, which checks on the CPU that they hold what is relied on here."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import preview_clip_restatement as PC
from tests import preview_restatement as PR
from tests import preview_scenes as PS
from tests.test_preview_clip_cpu import ground_sheet, view_filling

pytestmark = pytest.mark.gpu
DEV = "cuda"
AMBIENT, BG = 0.4, (255, 250, 240)


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name == "ground_sheet":
        return ground_sheet()
    if name == "view_filling":
        return view_filling()
    if name == "clipped_triangles":                                   # 164 of random_triangles' faces cross the near or the far plane
        return dict(PS.random_triangles(), near=2.9, far=3.2)
    return getattr(PS, name)()


@functools.lru_cache(maxsize=None)
def _reference(name, size, ss):
    """the clip restatement's (image, face ids) of a scene: computed once, shared, never written to"""
    from avatarclip_amd import preview
    sc = _scene(name)
    cam = preview.look_frames(sc["eye"], sc["at"], "y")[0]
    img, ids = PC.render(sc["v"], sc["t"], sc["c"], cam, math.tan(math.radians(sc["fov"]) * 0.5), sc["near"], sc["far"], sc["at"] - sc["eye"],
                         AMBIENT, BG, size, ss, grey=preview.GREY)
    img.setflags(write=False)
    ids.setflags(write=False)
    return img, ids


def _render(sc, size, ss, clip=True, **kw):
    from avatarclip_amd import preview
    kw = {**dict(eyes=sc["eye"], ats=sc["at"], near=sc["near"], far=sc["far"]), **kw}
    img, ids = preview.render_frames(sc["v"], sc["t"], sc["c"], up="y", fov=sc["fov"], image_size=size, ss=ss, ambient=AMBIENT, background=BG,
                                     return_face_ids=True, clip=clip, **kw)
    torch.cuda.synchronize()
    return img.cpu().numpy(), ids.cpu().numpy()


def _check(what, img, ids, ref_img, ref_ids):
    assert ids.shape == ref_ids.shape and ids.dtype == np.int32
    wrong = int((ids != ref_ids).sum())
    worst = int(np.abs(img.astype(np.int32) - ref_img.astype(np.int32)).max())
    print("%s: %d face ids differ; worst |image - restatement| = %d levels, %d pixels differ" % (what, wrong, worst, (img != ref_img).any(-1).sum()))
    assert wrong == 0
    assert worst <= 1


# ---------------------------------------------------------------------------------------------------------------- a, b, c: against the restatement
@pytest.mark.parametrize("size,ss", [(64, 1), (33, 2)])
def test_faces_cut_by_near_and_far(size, ss):
    """a: near = 2.9 and far = 3.2 pass through random_triangles; 33 at ss = 2 is a 66^2 raster, no multiple of the tile or of a wavefront"""
    img, ids = _render(_scene("clipped_triangles"), size, ss)
    ref_img, ref_ids = _reference("clipped_triangles", size, ss)
    _check("a %d x%d" % (size, ss), img[0], ids[0], ref_img, ref_ids)
    plain = _render(_scene("clipped_triangles"), size, ss, clip=False)[1]
    assert (ids >= 0).sum() > (plain >= 0).sum() > 0                   # the clipper adds pixels to what the parent draws


def test_ground_sheet_near_sides_and_far_at_once():
    """b: view-filling sub-triangles take the tile pass"""
    img, ids = _render(_scene("ground_sheet"), 128, 1)
    ref_img, ref_ids = _reference("ground_sheet", 128, 1)
    _check("b", img[0], ids[0], ref_img, ref_ids)
    assert (ids[0, 77:] >= 0).all()


def test_a_face_with_no_valid_corner_fills_the_view():
    """c: big_behind_small with face 0 replaced by a triangle whose corners all lie beyond the guard band; 256^2"""
    img, ids = _render(_scene("view_filling"), 256, 1)
    ref_img, ref_ids = _reference("view_filling", 256, 1)
    _check("c", img[0], ids[0], ref_img, ref_ids)
    assert (ids >= 0).all() and (ids == 0).sum() > 256 * 256 // 2


# ---------------------------------------------------------------------------------------------------------------- d: the widened int64 bound
def test_generated_corners_on_the_widened_corners_of_the_largest_raster():
    """d: a 2048^2 raster; two faces with no valid corner whose fans are clamped to the widened corners (-65536 - 256 and 256 R + 65536 +
    256 both ways, the widest differences the clipper can emit) and whose depth ramps run against each other, so the depth arithmetic
    decides every pixel.  Through the entry points directly."""
    from avatarclip_amd import lib as L
    from avatarclip_amd import preview
    R, width, near, far = PR.MAX_RASTER, 0.5, 0.5, 4.0
    v = np.array([[-900, -700, 178], [900, -700, -182], [0, 1100, -2],             # depth 2 + 0.2 x
                  [-900, -700, -182], [900, -700, 178], [0, 1100, -2]], np.float32)   # depth 2 - 0.2 x
    tris = np.array([[0, 1, 2], [3, 5, 4]], np.int32)
    colors = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]], np.uint8)
    cam = preview.look_frames([0, 0, 0], [0, 0, -1], "y")
    light = np.array([0.0, 0.0, -1.0], np.float32)
    key, fans, X, Y, Z, iw = PC.rasterize(v, cam[0], width, near, far, tris, R)                  # (PC.render, its key kept for the checks below)
    ref_img, ref_ids = PR.resolve(PC.shade_raster(key, fans, X, Y, Z, iw, v, tris, colors, light, 0.5, (0, 0, 0), 200.0), 1)[0], PR.face_ids(key)
    lo, hi = -(PR.GUARD + PC.EXTRA), 256 * R + PR.GUARD + PC.EXTRA
    assert (Z < 0).all() and all({int(f[0].min()), int(f[0].max()), int(f[1].min()), int(f[1].max())} == {lo, hi} for f in fans.values())
    assert (ref_ids >= 0).all() and all((ref_ids == f).sum() > R * R // 4 for f in range(2))
    lib, s = L.load(), L.stream()
    vd, td, cd = torch.from_numpy(v).to(DEV), torch.from_numpy(tris).to(DEV), torch.from_numpy(colors).to(DEV)
    camd, ld = torch.from_numpy(cam).to(DEV), torch.from_numpy(light[None]).to(DEV)
    proj = torch.empty(6, 4, device=DEV, dtype=torch.int32)
    nbytes = lib.avc_preview_scratch_bytes(2, R)
    assert nbytes == R * R * 8 + 16
    scratch = torch.full((nbytes,), 255, device=DEV, dtype=torch.uint8)
    img = torch.empty(1, R, R, 3, device=DEV, dtype=torch.uint8)
    ids = torch.empty(1, R, R, device=DEV, dtype=torch.int32)
    L.check(lib.avc_preview_project(L.ptr(vd), 1, 6, L.ptr(camd), width, near, far, R, L.ptr(proj), s), "avc_preview_project")
    L.check(lib.avc_preview_raster_clip(L.ptr(proj), L.ptr(vd), 1, 6, L.ptr(camd), width, near, far, L.ptr(td), 2, R, L.ptr(scratch), s),
            "avc_preview_raster_clip")
    L.check(lib.avc_preview_shade_clip(L.ptr(proj), L.ptr(vd), 1, 6, L.ptr(camd), width, near, far, L.ptr(td), 2, L.ptr(cd), 3, L.ptr(ld), 0.5,
                                       0.0, 0.0, 0.0, 200.0, R, 1, L.ptr(scratch), L.ptr(img), L.ptr(ids), s), "avc_preview_shade_clip")
    torch.cuda.synchronize()
    _check("d", img[0].cpu().numpy(), ids[0].cpu().numpy(), ref_img, ref_ids)
    assert bool((scratch == 255).all())
    assert lib.avc_preview_raster_clip(L.ptr(proj), L.ptr(vd), 1, 6, L.ptr(camd), width, near, far, L.ptr(td), 2, R + 1, L.ptr(scratch), s) != 0


# ---------------------------------------------------------------------------------------------------------------- e, f: beside the unclipped path
@pytest.mark.parametrize("name,size,ss", [("random_triangles", 64, 2), ("sheet", 33, 2), ("big_behind_small", 256, 1)])
def test_clip_changes_nothing_where_every_corner_is_valid(name, size, ss):
    """e: bit-identical, image and ids"""
    on, off = _render(_scene(name), size, ss, clip=True), _render(_scene(name), size, ss, clip=False)
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1]) and (on[1] >= 0).any()


def test_the_face_with_a_vertex_behind_the_camera_appears():
    """f: tests/test_gpu_preview.py's `one vertex behind the camera` input, which pins that the face is dropped without clip"""
    from avatarclip_amd import preview
    sc = PS.random_triangles()
    v = sc["v"].copy()
    v[sc["t"][3, 0]] = (0.0, 0.0, 3.5)
    hit = np.nonzero((sc["t"] == sc["t"][3, 0]).any(1))[0]
    sc = dict(sc, v=v)
    img, ids = _render(sc, 32, 2)
    cam = preview.look_frames(sc["eye"], sc["at"], "y")[0]
    ref_img, ref_ids = PC.render(v, sc["t"], sc["c"], cam, math.tan(math.radians(sc["fov"]) * 0.5), sc["near"], sc["far"], sc["at"] - sc["eye"], AMBIENT,
                                 BG, 32, 2)
    _check("f", img[0], ids[0], ref_img, ref_ids)
    assert np.isin(ids, hit).any() and not np.isin(_render(sc, 32, 2, clip=False)[1], hit).any()


# ---------------------------------------------------------------------------------------------------------------- g: batches and the scratch
def test_batch_equals_single_frames_and_the_scratch_comes_back():
    from avatarclip_amd import preview
    sc = _scene("ground_sheet")
    v = np.stack([sc["v"], sc["v"] * np.float32(0.9), sc["v"][:, [2, 1, 0]]])
    eyes = np.array([[0, 0.3, 0.0], [0.2, 0.5, 0.1], [-0.3, 0.2, 0.0]])
    ats = np.array([[0, 0.3, -1.0], [0.1, 0.3, -1.0], [0.0, 0.1, -1.0]])
    kw = dict(up="y", fov=sc["fov"], image_size=48, ss=2, ambient=AMBIENT, background=BG, near=0.05, far=4.0, return_face_ids=True, clip=True)
    scratch = torch.full((3 * preview.scratch_bytes(len(sc["t"]), 96),), 255, device=DEV, dtype=torch.uint8)
    img, ids = preview.render_frames(v, sc["t"], sc["c"], eyes=eyes, ats=ats, scratch=scratch, **kw)
    assert bool((scratch == 255).all())
    img2, ids2 = preview.render_frames(v, sc["t"], sc["c"], eyes=eyes, ats=ats, scratch=scratch, **kw)      # it serves a second call
    assert torch.equal(img, img2) and torch.equal(ids, ids2) and bool((scratch == 255).all())
    for i in range(3):
        one, one_ids = preview.render_frames(v[i], sc["t"], sc["c"], eyes=eyes[i], ats=ats[i], **kw)
        assert torch.equal(one[0], img[i]) and torch.equal(one_ids[0], ids[i])
        assert bool((ids[i, -8:] >= 0).all())                          # the ground under the camera: clipped faces, in every frame
    assert not torch.equal(img[0], img[1]) and not torch.equal(img[0], img[2])


# ---------------------------------------------------------------------------------------------------------------- h: the command line
def test_cli_focus_head(tmp_path, capsys):
    from PIL import Image
    from avatarclip_amd import mesh, preview
    ply, out = str(tmp_path / "strip.ply"), str(tmp_path / "face.png")
    mesh.write_ply(ply, PS.STRIP_V, PS.STRIP_T, PS.STRIP_C)
    preview.main(["--mesh", ply, "--focus", "head", "--out", out, "--views", "2", "--size", "128"])
    assert capsys.readouterr().out.strip() == out
    with Image.open(out) as im:
        got = np.asarray(im.convert("RGB"))
    eyes, ats, near, far = preview.frame_cameras(torch.from_numpy(PS.STRIP_V), 2, 10.0, "y", 40.0, 0.05, focus=(0.84, 1))
    kw = dict(up="y", fov=40.0, image_size=128, ss=2, near=near, far=far)
    expect = preview.render_frames(PS.STRIP_V, PS.STRIP_T, PS.STRIP_C, eyes, ats, clip=True, **kw).cpu().numpy()
    assert got.shape == (128, 128, 3) and np.array_equal(got, expect[0])
    assert (got[-1] != 255).any()                                     # the strip runs out of the bottom of the picture ...
    dropped = preview.render_frames(PS.STRIP_V, PS.STRIP_T, PS.STRIP_C, eyes, ats, clip=False, **kw).cpu().numpy()
    assert (dropped[0] == 255).all()                                  # ... and is missing altogether without the clipper
