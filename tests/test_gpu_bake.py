"""The texture bake on the device (csrc/avc_bake.hip through avatarclip_amd/bake.py, rig.py and preview.py) against
tests/bake_restatement.py: the closest point of a triangle soup bit for bit, the bake's image bytes, the rig's textured .glb, and the
preview's textured shade.  The inputs are tests/bake_scenes.py's; tests/test_bake_cpu.py checks with the restatement alone that they hold
what is relied on here and recomputes the recorded reference of the end-to-end case."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import bake_restatement as BR
from tests import bake_scenes as BS
from tests import drive_standins as S
from tests import preview_restatement as PR
from tests import preview_scenes as PS
from tests import rig_standins as RS

pytestmark = pytest.mark.gpu
DEV = "cuda"
AMBIENT, BG = 0.4, (255, 250, 240)
RIG_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rig.npz")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else a.dtype)


def _check_closest(points, v, t, cell=None):
    """tri, bary and d2 of bake.closest_on_mesh bit for bit the brute-force restatement's (every operation of csrc/avc_bake.h is one
    correctly rounded IEEE operation on both sides -- fp64 add, subtract, multiply, divide, no contraction -- so nothing is loosened)"""
    from avatarclip_amd import bake
    tri, bary, d2 = bake.closest_on_mesh(points, v, t, cell=cell)
    torch.cuda.synchronize()
    assert tri.dtype == torch.int32 and bary.dtype == torch.float64 and d2.dtype == torch.float64
    rtri, rbary, rd2 = BR.closest_on_mesh(points, v, t)
    tri, bary, d2 = tri.cpu().numpy(), bary.cpu().numpy(), d2.cpu().numpy()
    assert tri.shape == rtri.shape and bary.shape == rbary.shape and d2.shape == rd2.shape
    assert np.array_equal(tri, rtri), "first difference at query %d" % int(np.flatnonzero(tri != rtri)[0])
    assert np.array_equal(_bits(d2), _bits(rd2)) and np.array_equal(_bits(bary), _bits(rbary))
    return tri, bary, d2


# ---------------------------------------------------------------------------------------------------------------- the closest point
@pytest.mark.parametrize("huge", [True, False])
def test_closest_on_mesh_is_the_restatement_bit_for_bit(huge):
    """the spoilt sphere (a zero-area triangle, a duplicate; with `huge` one triangle that spans the bounding box, so that r_max exceeds the
    sphere and no walk can stop early -- without it the termination rule does the work) and 1 003 queries: on the surface, inside, 10
    diameters outside the grid, one exactly at a shared vertex"""
    v, t = BS.spoilt_sphere(huge)
    q = BS.queries(v, t)
    tri, bary, d2 = _check_closest(q, v, t)
    assert (tri != BS.FLAT).all() and (tri != len(t) - 1).all() and (tri == BS.COPIED).sum() >= 4       # degenerate skipped, the tie to the lower index
    assert d2[-1] == 0.0 and ((tri == BS.HUGE).sum() > 20) == huge
    _check_closest(q[:130], v, t, cell=0.05)                 # a grid far finer than the triangles, one far coarser: the same answers
    _check_closest(q[:130], v, t, cell=10.0)


def test_closest_on_mesh_one_query_one_triangle_and_refusals():
    from avatarclip_amd import bake
    v, t = BS.spoilt_sphere()
    q = BS.queries(v, t)
    _check_closest(q[37:38], v, t)                            # Q = 1
    one_v, one_t = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32), np.array([[0, 1, 2]], np.int32)
    pts = np.array([[1, 1, 3], [2, -1, 0], [-2, 1, 1], [3, 3, 0], [-1, -1, 2], [6, -1, 0], [-1, 7, -1], [1, 2, 0], [100, -50, 30]], np.float64)
    tri, bary, d2 = _check_closest(pts, one_v, one_t)         # F = 1: the hand cases of tests/test_bake_cpu.py
    assert list(d2[:8]) == [9.0, 1.0, 5.0, 2.0, 6.0, 5.0, 11.0, 0.0] and (tri == 0).all()
    tri, _, _ = bake.closest_on_mesh(np.zeros((0, 3)), one_v, one_t)
    assert tri.shape == (0,)
    with pytest.raises(ValueError, match="degenerate"):
        bake.closest_on_mesh(pts, v, t[BS.FLAT:BS.FLAT + 1])
    with pytest.raises(ValueError):
        bake.closest_on_mesh(pts, one_v, np.array([[0, 1, 3]], np.int32))
    with pytest.raises(ValueError):
        bake.closest_on_mesh(np.array([[np.nan, 0, 0]]), one_v, one_t)


# ---------------------------------------------------------------------------------------------------------------- the bake
def test_bake_texture_end_to_end():
    """size 128 on the 64 x 32 sphere simplified at divisor 8 by rig.simplify_mesh: the image bytes are the restatement's over all owned
    texels, free texels are 128.  Then the same geometry split per triangle and painted in 8 flat palette colours: every owned texel --
    everything a bilinear sample inside a chart reads -- holds exactly ONE palette colour, the closest dense triangle's, never a mix of
    two, wherever that triangle is unambiguous (the restatement's nearest triangle of another colour at least 1e-9 of the squared
    bounding-box diagonal farther than the nearest); at most 2 % of the owned texels are left out (tests/test_bake_cpu.py: 1.3 %)."""
    from avatarclip_amd import bake, rig
    case, rec = BS.bake_inputs(), BS.bake_record()
    v, t, c = case["dense"]
    sv, st, _ = rig.simplify_mesh(v, t, c, BS.BAKE_DIVISOR)
    assert np.array_equal(_bits(sv.cpu().numpy()), _bits(case["simple"][0])) and np.array_equal(st.cpu().numpy(), case["simple"][1])
    assert bake.atlas_cells(st.shape[0], BS.BAKE_SIZE)[1] >= 6
    stats = {}
    uv, image = bake.bake_texture(sv, st, v, t, c, BS.BAKE_SIZE, stats=stats)
    owned = case["owner"] >= 0
    assert uv.dtype == np.float32 and np.array_equal(uv, case["uv"]) and image.dtype == np.uint8 and image.shape == (BS.BAKE_SIZE, BS.BAKE_SIZE, 3)
    assert (image[~owned] == 128).all() and np.array_equal(image[owned], rec["image"][owned]) and np.array_equal(image, rec["image"])
    assert stats["texels"] == int(owned.sum()) and 1 <= stats["candidates_per_query"] < len(t) / 4        # the grid prunes
    fv, ft, fc, pick = case["flat"]
    _, flat = bake.bake_texture(sv.cpu().numpy(), st.cpu().numpy(), fv, ft, fc, BS.BAKE_SIZE)
    where, clear = case["where"], ~rec["ambiguous"]
    assert rec["ambiguous"].mean() <= 0.02
    got = flat[where[:, 0], where[:, 1]]
    assert np.array_equal(got[clear], BS.PALETTE[pick[rec["tri"]]][clear]) and np.array_equal(got[clear], rec["flat_image"][where[:, 0], where[:, 1]][clear])
    assert (got[:, None, :] == BS.PALETTE[None]).all(-1).any(-1).all()          # (a tie picks ONE of the tying triangles: still no mix anywhere)
    assert (flat[~owned] == 128).all()
    with pytest.raises(ValueError, match="no colours"):
        bake.bake_texture(sv, st, v, t, None, BS.BAKE_SIZE)
    with pytest.raises(ValueError, match="smallest size that would do is 104"):
        bake.bake_texture(sv, st, v, t, c, 64)


# ---------------------------------------------------------------------------------------------------------------- the rig
def test_build_rig_with_a_baked_texture(tmp_path):
    from avatarclip_amd import bake, rig
    g = np.load(RIG_GOLD)
    v, t, c = S.avatar_mesh(int(g["mesh_res"]))
    a = {k: (x.to(DEV) if k != "parents" else x) for k, x in RS.sparse_template_arrays().items()}
    kw = dict(name="fixture", motion=S.motion(), voxel_divisor=16)
    plain, plain_npz = rig.build_rig((v, t, c), a, g["stand_pose"], str(tmp_path / "plain"), **kw)
    zero, _ = rig.build_rig((v, t, c), a, g["stand_pose"], str(tmp_path / "zero"), bake_texture=0, **kw)
    assert open(plain, "rb").read() == open(zero, "rb").read() and not os.path.exists(str(tmp_path / "zero" / "fixture_texture.png"))
    glb, npz = rig.build_rig((v, t, c), a, g["stand_pose"], str(tmp_path / "baked"), bake_texture=128, **kw)
    p, r = rig.read_glb(plain), rig.read_glb(glb)
    zp, zr = np.load(plain_npz), np.load(npz)
    tris = zp["triangles"]
    F = len(tris)
    assert bake.atlas_cells(F, 128)[1] >= 6
    corner = tris.reshape(-1)
    assert len(r["attributes"]["POSITION"]) == 3 * F and np.array_equal(r["indices"], np.arange(3 * F))
    assert "COLOR_0" not in r["attributes"] and "COLOR_0" in p["attributes"] and p["uv"] is None and p["image"] is None
    for k in p["attributes"]:                                 # position and skin of corner k = those of its shared vertex in the untextured build
        if k != "COLOR_0":
            assert np.array_equal(r["attributes"][k], p["attributes"][k][corner]), k
    assert sorted(r["attributes"]) == sorted([k for k in p["attributes"] if k != "COLOR_0"] + ["TEXCOORD_0"])
    uv, _ = bake.atlas_layout(F, 128)
    assert np.array_equal(r["uv"], uv.reshape(-1, 2)) and np.array_equal(zr["uv"], uv)
    for k in zp.files:                                        # every other key of the .npz: as without the option, unsplit
        assert np.array_equal(zp[k], zr[k]), k
    assert sorted(zr.files) == sorted(zp.files + ["uv"])
    sv, st, _ = rig.simplify_mesh(v, t, c, 16)
    _, image = bake.bake_texture(sv, st, v, t, c, 128)
    assert np.array_equal(r["image"], image) and len(np.unique(image.reshape(-1, 3), axis=0)) > 50
    assert np.array_equal(rig.decode_png(open(str(tmp_path / "baked" / "fixture_texture.png"), "rb").read()), image)
    assert len(r["animation"]) == len(p["animation"]) == 24 and r["json"]["materials"][0]["pbrMetallicRoughness"]["metallicFactor"] == 0


# ---------------------------------------------------------------------------------------------------------------- the preview
def _split(sc):
    """a preview scene on one vertex per corner (the topology a baked .glb has), with the atlas UVs"""
    from avatarclip_amd import bake
    t = np.asarray(sc["t"])
    uv, owner = bake.atlas_layout(len(t), 128)
    return np.ascontiguousarray(sc["v"][t.reshape(-1)]), np.arange(3 * len(t), dtype=np.int32).reshape(-1, 3), uv.reshape(-1, 2), owner


def _restated_textured(v, t, uv, texels, sc, eye, size, ss):
    """tests/preview_restatement.py's frame with the colour taken from the texture: its projection, coverage, depth and shade, and per
    covered raster pixel the float64 bilinear fetch (tests/bake_restatement.bilinear) at the perspective-correct UV"""
    from avatarclip_amd import preview
    R = size * ss
    cam = preview.look_frames(eye, sc["at"], "y")[0]
    X, Y, Z, iw = PR.project(v, cam, math.tan(math.radians(sc["fov"]) * 0.5), sc["near"], sc["far"], R)
    key = PR.rasterize(X, Y, Z, t, R)
    ids = PR.face_ids(key)
    white = PR.shade_raster(key, X, Y, Z, iw, v, t, None, sc["at"] - eye, AMBIENT, BG, grey=1.0)          # colour 1: the flat shade itself
    out = white.copy()
    for f in np.unique(ids[ids >= 0]):
        idx, _ = PR.orient(X, Y, Z, t[f])
        yy, xx = np.nonzero(ids == f)
        px, py = PR.SUBPIXEL * xx + 128, PR.SUBPIXEL * yy + 128
        x, y = [int(X[i]) for i in idx], [int(Y[i]) for i in idx]
        w = [((x[b] - x[a]) * (py - y[a]) - (y[b] - y[a]) * (px - x[a])).astype(np.float64) for a, b in ((1, 2), (2, 0), (0, 1))]
        lam = [w[k] * float(iw[idx[k]]) for k in range(3)]
        den = lam[0] + lam[1] + lam[2]
        u = sum(lam[k] * float(uv[idx[k], 0]) for k in range(3)) / den
        vv = sum(lam[k] * float(uv[idx[k], 1]) for k in range(3)) / den
        out[yy, xx] = BR.bilinear(texels, u, vv) * white[yy, xx]
    return PR.resolve(out, ss)[0], ids


@functools.lru_cache(maxsize=None)
def _textured_scene():
    sc = PS.sheet()
    v, t, uv, owner = _split(sc)
    texels = np.random.RandomState(5).randint(0, 256, (128, 128, 3)).astype(np.uint8)
    return sc, v, t, uv, owner, texels


@pytest.mark.parametrize("eye", [(0.0, 0.0, 3.0), (1.2, 0.8, 2.6)])
def test_textured_shade_against_the_restatement(eye):
    """64 x 64, ss 2, two views of the jittered sheet under a NOISE texture (the steepest gradients a texture can have).  face_ids are
    exact.  The image is within 1 of 255: the kernel interpolates in float32 -- the weights l_i, the UV mix and its division, x = u T -
    0.5, the two lerps, the shade, the box average -- where the restatement uses float64; the fetch is continuous in (u, v) (a floor that
    falls the other way changes the taps, not the value), so the colours differ by ~1e-4 levels and only floor(x + 0.5) of the averaged
    pixel can land on the other side of a boundary."""
    from avatarclip_amd import preview
    sc, v, t, uv, owner, texels = _textured_scene()
    eye = np.asarray(eye, np.float64)
    img, ids = preview.render_frames(v, t, None, eyes=eye, ats=sc["at"], up="y", fov=sc["fov"], image_size=64, ss=2, ambient=AMBIENT, background=BG,
                                     near=sc["near"], far=sc["far"], return_face_ids=True, texture=(uv, texels))
    torch.cuda.synchronize()
    ref_img, ref_ids = _restated_textured(v, t, uv, texels, sc, eye, 64, 2)
    assert np.array_equal(ids[0].cpu().numpy(), ref_ids) and (ref_ids >= 0).mean() > 0.5
    diff = np.abs(img[0].cpu().numpy().astype(np.int32) - ref_img.astype(np.int32))
    print("worst |image - restatement| = %d levels, %d values differ" % (diff.max(), (diff > 0).sum()))
    assert diff.max() <= 1
    assert len(np.unique(ref_img.reshape(-1, 3), axis=0)) > 1000


def test_flat_charts_render_as_per_corner_vertex_colours():
    """a texture that is flat per chart: the textured picture is, within 1 of 255, the vertex-colour picture of the same split mesh with
    that colour on the chart's three corners -- both are convex combinations of ONE value (c (1 - f) + c f and (l0 c + l1 c + l2 c) / den
    may each round away from c by an ulp in float32, hence not equality) -- and clip=True refuses a texture"""
    from avatarclip_amd import preview
    sc, v, t, uv, owner, _ = _textured_scene()
    chart = np.random.RandomState(6).randint(0, 256, (len(t), 3)).astype(np.uint8)
    texels = np.where((owner >= 0)[..., None], chart[np.maximum(owner, 0)], 128).astype(np.uint8)
    kw = dict(eyes=sc["eye"], ats=sc["at"], up="y", fov=sc["fov"], image_size=64, ss=2, ambient=AMBIENT, background=BG, near=sc["near"], far=sc["far"],
              return_face_ids=True)
    tex, tex_ids = preview.render_frames(v, t, None, texture=(uv, texels), **kw)
    col, col_ids = preview.render_frames(v, t, np.repeat(chart, 3, axis=0), **kw)
    torch.cuda.synchronize()
    assert torch.equal(tex_ids, col_ids) and bool((tex_ids >= 0).all())
    diff = (tex.int() - col.int()).abs()
    print("worst |textured - vertex colours| = %d levels" % int(diff.max()))
    assert int(diff.max()) <= 1 and len(torch.unique(col.reshape(-1, 3), dim=0)) > 100
    with pytest.raises(ValueError, match="no textured variant"):
        preview.render_frames(v, t, None, texture=(uv, texels), clip=True, **kw)
    with pytest.raises(ValueError):
        preview.render_frames(v, t, np.repeat(chart, 3, axis=0), texture=(uv, texels), **kw)
    with pytest.raises(ValueError):
        preview.render_frames(v, t, None, texture=(uv[:-1], texels), **kw)


def test_preview_shows_a_baked_glb_textured(tmp_path):
    """preview --glb of a textured file goes through glb_source's texture and avc_preview_shade_tex: the strip of tests/preview_scenes.py
    under a two-colour texture shows both colours and none of the grey of an uncoloured mesh"""
    from avatarclip_amd import bake, preview, rig
    t = PS.STRIP_T
    corner = t.reshape(-1)
    uv, owner = bake.atlas_layout(len(t), 64)
    texels = np.where((owner % 2 == 0)[..., None], np.array([250, 10, 10]), np.array([10, 10, 250])).astype(np.uint8)
    path = rig.write_glb(str(tmp_path / "strip.glb"), PS.STRIP_V[corner], np.arange(len(corner), dtype=np.int32).reshape(-1, 3), None,
                         np.ascontiguousarray(PS.STRIP_JOINTS[:, corner]), np.ascontiguousarray(PS.STRIP_WEIGHTS[:, corner]), PS.STRIP_JOINT_POS,
                         parents=(-1, 0), names=("root", "tip"), name="strip", uv=uv.reshape(-1, 2), texture=texels)
    src = preview.glb_source(path, return_texture=True)
    assert len(src) == 5 and np.array_equal(src[4][1], texels) and len(preview.glb_source(path)) == 4
    out, images = preview.preview(str(tmp_path / "strip.png"), glb=path, views=2, size=64, ss=1)
    px = images[0].reshape(-1, 3).cpu().numpy().astype(np.int32)
    body = px[(px != 255).any(1)]
    assert len(body) > 100 and os.path.exists(out)
    assert ((body[:, 0] > 2 * body[:, 2]) | (body[:, 2] > 2 * body[:, 0])).all()          # red or blue under the shade, never grey
    assert (body[:, 0] > 2 * body[:, 2]).any() and (body[:, 2] > 2 * body[:, 0]).any()
    with pytest.raises(ValueError, match="no clipped preview"):
        preview.preview(str(tmp_path / "strip2.png"), glb=path, views=2, size=64, ss=1, clip=True)
