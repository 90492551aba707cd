"""The texture bake without a GPU: tests/bake_restatement.py (the numpy statement of the rules of csrc/avc_bake.h) on hand cases of the
closest-point routine, the invariants of bake.atlas_layout checked exhaustively, the textured .glb round trip, the untextured writer's
bytes, the binding of the fifth header and the pipeline's fingerprints."""
import dataclasses
import hashlib
import os

import numpy as np
import pytest

from avatarclip_amd import bake
from tests import bake_restatement as BR

# one triangle in the plane z = 0: a = (0,0,0), b = (4,0,0), c = (0,4,0); every coordinate below is exact in binary
TRI_V = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
TRI_T = np.array([[0, 1, 2]], np.int32)


@pytest.mark.parametrize("p,bary,d2", [
    ((1.0, 1.0, 3.0), (0.5, 0.25, 0.25), 9.0),            # over the interior: the foot of the perpendicular
    ((2.0, -1.0, 0.0), (0.5, 0.5, 0.0), 1.0),             # edge ab (in the plane, outside)
    ((-2.0, 1.0, 1.0), (0.75, 0.0, 0.25), 5.0),           # edge ac
    ((3.0, 3.0, 0.0), (0.0, 0.5, 0.5), 2.0),              # edge bc: in the plane but outside
    ((-1.0, -1.0, 2.0), (1.0, 0.0, 0.0), 6.0),            # vertex a
    ((6.0, -1.0, 0.0), (0.0, 1.0, 0.0), 5.0),             # vertex b
    ((-1.0, 7.0, -1.0), (0.0, 0.0, 1.0), 11.0),           # vertex c
    ((1.0, 2.0, 0.0), (0.25, 0.25, 0.5), 0.0),            # on the triangle
])
def test_restated_closest_point_on_hand_cases(p, bary, d2):
    tri, b, d = BR.closest_on_mesh(np.array([p]), TRI_V, TRI_T)
    assert tri[0] == 0 and tuple(b[0]) == bary and d[0] == d2


def test_restated_closest_point_skips_degenerate_triangles_and_breaks_ties_low():
    v = np.concatenate([TRI_V, [[0, 0, 1], [2, 0, 1], [4, 0, 1], [1, 1, 5]]]).astype(np.float32)
    # 0: three collinear points right above the query's side (distance would be 0); 1: a repeated corner; 2 and 3: the triangle, twice
    t = np.array([[3, 4, 5], [6, 6, 0], [0, 1, 2], [0, 1, 2]], np.int32)
    tri, b, d, every = BR.closest_on_mesh(np.array([[2.0, 0.0, 1.0], [1.0, 1.0, 5.0]]), v, t, return_all=True)
    assert list(tri) == [2, 2] and list(d) == [1.0, 25.0]
    assert np.isinf(every[:, :2]).all() and np.array_equal(every[:, 2], every[:, 3])
    with pytest.raises(ValueError):
        BR.closest_on_mesh(np.zeros((1, 3)), v, t[:2])


# ---------------------------------------------------------------------------------------------------------------- the atlas
@pytest.mark.parametrize("F", [1, 2, 3, 50, 51])
def test_atlas_layout_invariants(F):
    size = 64
    uv, owner = bake.atlas_layout(F, size)
    ruv, rowner, corner = BR.layout(F, size)                  # (c): the restatement asserts that it never writes a texel twice
    assert uv.dtype == np.float32 and uv.shape == (F, 3, 2) and owner.dtype == np.int32 and owner.shape == (size, size)
    assert np.array_equal(uv, ruv) and np.array_equal(owner, rowner)
    G, P = BR.cells(F, size)
    assert P >= 6 and (G, P) == bake.atlas_cells(F, size) and np.array_equal(corner, bake.chart_corners(F, G, P))
    assert sorted(np.unique(owner[owner >= 0])) == list(range(F))
    # (a) corners on texel centres, inside the triangle's own cell, on texels it owns
    tex = uv.astype(np.float64) * size - 0.5
    assert np.array_equal(tex, corner)
    for f in range(F):
        col, row = (f // 2) % G, (f // 2) // G
        assert ((corner[f, :, 0] // P == col) & (corner[f, :, 1] // P == row)).all()
        assert (owner[corner[f, :, 1], corner[f, :, 0]] == f).all()
        area2 = np.linalg.det(np.concatenate([corner[f], np.ones((3, 1))], 1).astype(np.float64))
        assert abs(area2) >= 1.0                              # three distinct corners, not in line
    # (b) every texel a bilinear fetch reads anywhere on the closed UV triangle: a barycentric lattice with corners and edges, sampled at
    # the float32 UVs the file carries; all FOUR taps count, a tap of weight zero included
    n = 4 * P
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    keep = i + j <= n
    w = np.stack([i[keep], j[keep], n - i[keep] - j[keep]], 1).astype(np.float64) / n
    for f in range(F):
        u, v = w @ uv[f, :, 0].astype(np.float64), w @ uv[f, :, 1].astype(np.float64)
        x0, x1, y0, y1, _, _ = BR.bilinear_taps(u, v, size)
        for ys, xs in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
            assert (owner[ys, xs] == f).all(), f
    # a gutter of at least one texel: the 4 neighbours of every texel whose centre lies on the closed triangle are the chart's too
    for jj in range(size):
        for ii in range(size):
            tb = BR.texel_barycentrics(ii, jj, F, size)
            if tb is not None and min(tb[1]) >= 0:
                assert jj >= 1 and ii >= 1 and (owner[jj - 1:jj + 2, ii] == tb[0]).all() and (owner[jj, ii - 1:ii + 2] == tb[0]).all()


def test_atlas_layout_refuses_small_charts_and_bad_sizes():
    assert bake.atlas_cells(2 * 10 * 10, 64) == (10, 6)
    with pytest.raises(ValueError, match="smallest size that would do is 68"):
        bake.atlas_layout(2 * 10 * 10 + 1, 64)                # 11 x 11 cells of 5 texels
    assert bake.atlas_cells(2 * 11 * 11, 68) == (11, 6)
    with pytest.raises(ValueError, match="above the limit"):
        bake.atlas_layout(2 * 700 * 700, 4096)
    for size in (60, 66, 4100, 0):
        with pytest.raises(ValueError, match="multiple of 4"):
            bake.atlas_layout(4, size)
    with pytest.raises(ValueError):
        bake.atlas_layout(0, 64)


def test_restated_texel_barycentrics_are_the_charts_affine_map():
    """corner texels get (1,0,0), (0,1,0), (0,0,1) exactly; a gutter texel extrapolates (a negative weight); the weights sum to 1"""
    F, size = 3, 64
    _, owner, corner = BR.layout(F, size)
    for f in range(F):
        for k in range(3):
            g, b = BR.texel_barycentrics(int(corner[f, k, 0]), int(corner[f, k, 1]), F, size)
            assert g == f and tuple(b) == tuple(float(x == k) for x in range(3))
    seen_negative = False
    for j in range(size):
        for i in range(size):
            tb = BR.texel_barycentrics(i, j, F, size)
            assert (tb is None) == (owner[j, i] < 0)
            if tb is not None:
                assert tb[0] == owner[j, i] and abs(sum(tb[1]) - 1.0) < 1e-15
                seen_negative |= min(tb[1]) < 0
    assert seen_negative


# ---------------------------------------------------------------------------------------------------------------- the GPU tests' inputs
def test_the_spoilt_sphere_and_its_queries_hold_what_the_gpu_test_relies_on():
    from tests import bake_scenes as BS
    v, t = BS.spoilt_sphere()
    vv = v.astype(np.float64)
    dead = BR.degenerate(vv[t[:, 0]], vv[t[:, 1]], vv[t[:, 2]])
    assert len(t) == 961 and list(np.flatnonzero(dead)) == [BS.FLAT] and np.array_equal(t[-1], t[BS.COPIED])
    assert np.array_equal(vv.min(0), [-1, -1, -1]) and np.array_equal(vv.max(0), [1, 1, 1])         # the huge triangle spans the box
    q = BS.queries(v, t)
    assert q.shape == (1003, 3) and len(q) % 64 != 0
    tri, bary, d2, every = BR.closest_on_mesh(q, v, t, return_all=True)
    assert (tri != len(t) - 1).all() and (tri == BS.COPIED).sum() >= 4                               # the copy ties and never wins
    assert np.array_equal(every[:, -1], every[:, BS.COPIED]) and (tri != BS.FLAT).all()
    assert (tri == BS.HUGE).sum() > 20                                                               # inside points see the huge triangle
    assert d2[-1] == 0.0 and (every[-1] == 0.0).sum() >= 4 and tri[-1] == np.flatnonzero(every[-1] == 0.0)[0]   # the shared vertex: a tie
    assert (np.sqrt(d2[800:1002]) > 25).all()


def test_the_bake_case_holds_what_the_gpu_test_relies_on():
    """the restatement alone, brute force (the slowest test here, some 20 s): the record the GPU test reads is what the restatement
    computes, and the palette input stays within the cap of 2 % ambiguous texels"""
    from tests import bake_scenes as BS
    case, rec = BS.bake_inputs(), BS.bake_record()
    here = BS.uv_sphere(BS.BAKE_NU, BS.BAKE_NV)[0]
    assert np.abs(here - rec["v"]).max() <= 2.0 ** -23 and np.array_equal(case["dense"][0], rec["v"])    # sin / cos to the last bit or next to it
    sv, st = case["simple"]
    G, P = BR.cells(len(st), BS.BAKE_SIZE)
    ref = BS.bake_reference(case)
    print("bake case: %d simplified triangles, %d x %d cells of %d texels, %d owned texels, %d ambiguous" % (len(st), G, G, P, len(ref["tri"]),
                                                                                                        ref["ambiguous"].sum()))
    assert P >= 6 and len(st) > 100 and len(case["dense"][1]) == 2 * BS.BAKE_NU * (BS.BAKE_NV - 1)
    for k in ("tri", "image", "flat_image", "ambiguous"):
        assert np.array_equal(ref[k], rec[k]), k
    assert ref["ambiguous"].mean() <= 0.02                                           # the cap of the palette test
    clear = ~ref["ambiguous"]
    where, (fv, ft, fc, pick) = case["where"], case["flat"]
    assert sorted(np.unique(pick)) == list(range(8))                                 # all eight colours, one per dense triangle
    got = ref["flat_image"][where[:, 0], where[:, 1]]
    assert np.array_equal(got[clear], BS.PALETTE[pick[ref["tri"]]][clear])           # one palette colour, the closest triangle's: no mix
    assert len(np.unique(pick[ref["tri"]][clear])) == 8
    assert (ref["flat_image"][case["owner"] < 0] == 128).all() and (ref["image"][case["owner"] < 0] == 128).all()
    assert len(np.unique(ref["image"][where[:, 0], where[:, 1]], axis=0)) > 1000     # the smooth colours really vary
    assert ref["min_bary"] >= -1e-15                                                 # closest points lie ON their triangles


# ---------------------------------------------------------------------------------------------------------------- the .glb
def _small_rig(seed=0, F=5):
    rng = np.random.default_rng(seed)
    M = 3 * F
    pos = rng.standard_normal((M, 3)).astype(np.float32)
    tris = np.arange(M, dtype=np.int32).reshape(-1, 3)
    joints = np.zeros((1, M, 4), np.uint8)
    joints[0, :, 1] = 1
    w = rng.random((M, 1)).astype(np.float32)
    weights = np.concatenate([w, 1 - w, np.zeros((M, 2), np.float32)], 1)[None]
    jp = np.array([[0, 0, 0], [0, 1, 0]], np.float64)
    uv, _ = bake.atlas_layout(F, 64)
    image = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    kw = dict(parents=(-1, 0), names=("root", "tip"), name="small")
    return pos, tris, joints, weights, jp, uv.reshape(-1, 2), image, kw


def test_textured_glb_round_trip(tmp_path):
    from avatarclip_amd import rig
    pos, tris, joints, weights, jp, uv, image, kw = _small_rig()
    path = rig.write_glb(str(tmp_path / "t.glb"), pos, tris, None, joints, weights, jp, uv=uv, texture=image, **kw)
    g = rig.read_glb(path)
    assert g["uv"].dtype == np.float32 and np.array_equal(g["uv"], uv) and np.array_equal(g["attributes"]["TEXCOORD_0"], uv)
    assert g["image"].dtype == np.uint8 and np.array_equal(g["image"], image)
    assert "COLOR_0" not in g["attributes"] and np.array_equal(g["attributes"]["POSITION"], pos)
    doc = g["json"]
    assert doc["materials"] == [{"name": "small", "pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0, "roughnessFactor": 1.0}}]
    assert doc["samplers"] == [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]
    assert doc["textures"] == [{"sampler": 0, "source": 0}] and doc["meshes"][0]["primitives"][0]["material"] == 0
    (im,) = doc["images"]
    view = doc["bufferViews"][im["bufferView"]]
    assert im["mimeType"] == "image/png" and "target" not in view and view["byteOffset"] % 4 == 0
    assert all(a["bufferView"] != im["bufferView"] for a in doc["accessors"])
    data = open(path, "rb").read()
    start = 20 + int.from_bytes(data[12:16], "little") + 8 + view["byteOffset"]
    png = data[start:start + view["byteLength"]]
    assert png == rig.encode_png(image) and png[:8] == b"\x89PNG\r\n\x1a\n" and np.array_equal(rig.decode_png(png), image)
    # the reader is as strict with the new parts as with the old
    import json
    import struct

    def rewrite(change, blob_change=None):
        jlen = int.from_bytes(data[12:16], "little")
        d = json.loads(data[20:20 + jlen].decode())
        change(d)
        text = json.dumps(d, separators=(",", ":")).encode()
        text += b" " * (-len(text) % 4)
        blob = bytearray(data[20 + jlen + 8:])
        if blob_change:
            blob_change(blob)
        out = struct.pack("<III", rig.GLB_MAGIC, 2, 12 + 8 + len(text) + 8 + len(blob)) + struct.pack("<II", len(text), rig.GLB_JSON) + text + \
            struct.pack("<II", len(blob), rig.GLB_BIN) + bytes(blob)
        (tmp_path / "bad.glb").write_bytes(out)
        return str(tmp_path / "bad.glb")

    assert np.array_equal(rig.read_glb(rewrite(lambda d: None))["image"], image)
    tex_acc = doc["meshes"][0]["primitives"][0]["attributes"]["TEXCOORD_0"]
    for change in (lambda d: d["textures"][0].update(source=1), lambda d: d["textures"][0].update(sampler=3),
                   lambda d: d["materials"][0]["pbrMetallicRoughness"]["baseColorTexture"].update(index=2),
                   lambda d: d["materials"][0]["pbrMetallicRoughness"].update(metallicFactor=1.0),
                   lambda d: d["samplers"][0].update(wrapS=10497), lambda d: d["samplers"][0].update(magFilter=9728),
                   lambda d: d["images"][0].update(mimeType="image/jpeg"), lambda d: d["images"][0].update(bufferView=99),
                   lambda d: d["bufferViews"][im["bufferView"]].update(byteLength=10 ** 9),
                   lambda d: d["bufferViews"][im["bufferView"]].update(target=34962),
                   lambda d: d["accessors"][tex_acc].update(componentType=5123),
                   lambda d: d["meshes"][0]["primitives"][0].pop("material"),
                   lambda d: d["meshes"][0]["primitives"][0]["attributes"].pop("TEXCOORD_0"),
                   lambda d: d.pop("materials")):
        with pytest.raises(ValueError):
            rig.read_glb(rewrite(change))
    with pytest.raises(ValueError, match="does not decode|PNG"):
        rig.read_glb(rewrite(lambda d: None, lambda blob: blob.__setitem__(slice(view["byteOffset"], view["byteOffset"] + 8), b"notapng!")))
    for bad in (dict(uv=uv), dict(texture=image), dict(uv=uv.astype(np.float64), texture=image), dict(uv=uv[:-1], texture=image),
                dict(uv=uv, texture=image[:, :32]), dict(uv=uv, texture=image.astype(np.float32))):
        with pytest.raises(ValueError):
            rig.write_glb(str(tmp_path / "x.glb"), pos, tris, None, joints, weights, jp, **bad, **kw)


def test_untextured_glb_bytes_do_not_depend_on_the_new_arguments(tmp_path):
    """without a texture the writer's output is what it was: the same bytes whether the new arguments are left out or given as None, no
    material, texture, sampler or image in the document, and the reader reports neither"""
    from avatarclip_amd import rig
    pos, tris, joints, weights, jp, uv, image, kw = _small_rig()
    colors = np.full((len(pos), 4), 255, np.uint8)
    times = np.arange(3, dtype=np.float32) / 60
    rot = np.tile(np.array([0, 0, 0, 1], np.float32), (3, 2, 1))
    a = rig.write_glb(str(tmp_path / "a.glb"), pos, tris, colors, joints, weights, jp, times=times, rotations=rot, **kw)
    b = rig.write_glb(str(tmp_path / "b.glb"), pos, tris, colors, joints, weights, jp, times=times, rotations=rot, uv=None, texture=None, **kw)
    da, db = (hashlib.sha256(open(p, "rb").read()).hexdigest() for p in (a, b))
    assert da == db
    g = rig.read_glb(a)
    assert g["uv"] is None and g["image"] is None
    assert not {"materials", "textures", "samplers", "images"} & set(g["json"]) and "material" not in g["json"]["meshes"][0]["primitives"][0]
    assert sorted(g["json"]) == ["accessors", "animations", "asset", "bufferViews", "buffers", "meshes", "nodes", "scene", "scenes", "skins"]
    assert sorted(g["attributes"]) == ["COLOR_0", "JOINTS_0", "POSITION", "WEIGHTS_0"]
    assert len(g["json"]["bufferViews"]) == len(g["json"]["accessors"])          # no view without an accessor: no image


# ---------------------------------------------------------------------------------------------------------------- the binding
def test_bake_header_binding():
    from avatarclip_amd import build, lib
    protos, abi = lib.parse_header(open(lib.BAKE_HEADER).read())
    assert abi is None and sorted(protos) == ["avc_bake_cell_starts", "avc_bake_colors", "avc_bake_query", "avc_bake_texel_points", "avc_bake_tri_keys",
                                               "avc_preview_shade_tex"]
    for name, p in protos.items():
        assert p.launch and p.restype is lib.c_int and p.params[-1] == lib.Param("stream", lib.c_void_p, "void*", "void", False), name
    others = {}
    for h in lib.headers() + lib.added_headers():
        more, _ = lib.parse_header(open(h).read())
        assert not set(more) & set(protos) and not set(more) & set(others), h
        others.update(more)
    assert len(lib.headers() + lib.added_headers()) == 4
    assert lib.headers() == (lib.HEADER, lib.TEXTURE_HEADER, lib.CODEBOOK_HEADER) and lib.added_headers() == (lib.PREVIEW_CLIP_HEADER,)
    assert lib.later_headers() == (lib.BAKE_HEADER,) and os.path.samefile(lib.BAKE_HEADER, os.path.join(build.CSRC, build.BAKE_HEADER))
    grey, _ = lib.parse_header(open(lib.HEADER).read())
    assert len(grey) == 81
    plain = [q.name for q in grey["avc_preview_shade"].params]
    tex = [q.name for q in protos["avc_preview_shade_tex"].params]
    assert [n for n in plain if n not in ("colors", "csize", "grey")] == [n for n in tex if n not in ("uv", "texels", "T")]
    assert tex[tex.index("uv"):tex.index("uv") + 3] == ["uv", "texels", "T"] and plain.index("colors") == tex.index("uv")
    q = {p.name: p for p in protos["avc_bake_query"].params}
    assert q["points"].elem == "double" and q["points"].const and q["bary"].elem == "double" and q["keys"].elem == "long long" and q["r_max"].decl == "double"
    assert build.SOURCES[-2:] == ["avc_bake.hip", "avc_preview_clip.hip"] and build.HEADERS[-3:] == [build.BAKE_HEADER, "avc_preview.h", build.PREVIEW_CLIP_HEADER]
    for name in ("avc_bake.hip", "avc_bake.h"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    bound = lib.load()
    assert lib.ABI_VERSION == 4 and bound.avc_version() == 4
    for name in protos:
        assert name in lib._launches and len(getattr(bound, name).argtypes) == len(protos[name].params)


def test_a_name_the_bake_header_declares_twice_is_refused(tmp_path, monkeypatch):
    from avatarclip_amd import lib
    dup = tmp_path / "dup.h"
    dup.write_text("int avc_preview_raster_clip(const float* x, int N, void* stream);\n")
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "BAKE_HEADER", str(dup))
    with pytest.raises(RuntimeError, match="declares avc_preview_raster_clip, which .*avc_preview_clip.h declares already"):
        lib.load()


# ---------------------------------------------------------------------------------------------------------------- the pipeline
def test_bake_texture_enters_the_rig_fingerprint_only_when_set(tmp_path):
    from avatarclip_amd import pipeline as P
    from tests import test_pipeline_cpu as TP
    spec = TP._spec(tmp_path)
    assert spec.bake_texture == 0 and P.stage_settings(spec, "rig") == {"name": "avatar", "voxel_divisor": 256}     # what it was before the option
    zero = P.fingerprints(dataclasses.replace(spec, bake_texture=0))
    assert zero == P.fingerprints(spec)
    baked = P.fingerprints(dataclasses.replace(spec, bake_texture=1024))
    assert [st for st in P.STAGES if zero[st] != baked[st]] == ["rig", "preview"]
    assert P.stage_settings(dataclasses.replace(spec, bake_texture=1024), "rig") == {"name": "avatar", "voxel_divisor": 256, "bake_texture": 1024}
    other = P.fingerprints(dataclasses.replace(spec, bake_texture=2048))
    assert other["rig"] != baked["rig"] and other["drive"] == baked["drive"]
    assert P.spec_from_args(["--out_dir", str(tmp_path), "--bake_texture", "512"]).bake_texture == 512
    assert P.spec_from_args(["--out_dir", str(tmp_path)]).bake_texture == 0


def test_render_frames_refuses_a_texture_on_the_clipped_path():
    from avatarclip_amd import preview
    uv = np.zeros((3, 2), np.float32)
    with pytest.raises(ValueError, match="no textured variant"):
        preview.render_frames(np.zeros((3, 3), np.float32), np.array([[0, 1, 2]]), eyes=[0, 0, 3], ats=[0, 0, 0], clip=True,
                              texture=(uv, np.zeros((4, 4, 3), np.uint8)))
