"""The texture path without a device: avatarclip_amd/texture.py's loader against the restatement (tests/nr_texture_restatement.py) on a fixture
written here, its error cases, the restatement's own properties, the second ABI header, render_rgb_batch's refusals, and the --smpl_uv switch of
the three command lines."""
import os

import numpy as np
import pytest
import torch

from tests import nr_grad_restatement as R
from tests import nr_texture_restatement as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

OBJ = """mtllib body.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0.5 0.5 1
v -1 0.5 0.5
vt 0.1 0.2
vt 0.9 0.15
vt 1.0 1.0
vt 0.05 0.8
vt 1.7 -0.3
vt -2.25 3.5
vt 0.5 0.5
usemtl skin
f 1/1 2/2 3/3 4/4
f 1/1/1 2/5/1 5/6/1
usemtl paint
f 2 3 5
usemtl skin
f 4/7 1/3 6/6
"""
MTL = """newmtl paint
Ka 0 0 0
Kd 0.25 0.5 0.75

newmtl skin
Kd 1 1 1
map_Kd skin.png
"""


def _fixture(d, obj=OBJ, mtl=MTL, image=True):
    from PIL import Image
    if image:
        rs = np.random.RandomState(0)
        Image.fromarray(rs.randint(0, 256, (3, 5, 3)).astype(np.uint8)).save(os.path.join(str(d), "skin.png"))      # 5 wide, 3 high: not square
    if mtl is not None:
        with open(os.path.join(str(d), "body.mtl"), "w") as fh:
            fh.write(mtl)
    path = os.path.join(str(d), "body.obj")
    with open(path, "w") as fh:
        fh.write(obj)
    return path


@pytest.mark.parametrize("ts", [8, 2, 3])
def test_loader_equals_the_restatement(tmp_path, ts):
    """one Kd-only material, one map_Kd material on a 5 x 3 image, a quad (fan-triangulated), vt outside [0, 1) and exactly 1.0: the same fp32
    operations in the same order, so every texel is equal"""
    from avatarclip_amd.texture import load_obj_texture
    path = _fixture(tmp_path)
    v, f, tex = load_obj_texture(path, texture_size=ts)
    rv, rf, rtex = T.load_obj_texture(path, ts)
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4], [3, 0, 5]] and np.array_equal(f, rf) and np.array_equal(v, rv)
    assert tex.shape == (5, ts, ts, ts, 3) and tex.dtype == np.float32
    diff = np.abs(tex - rtex)
    print("ts = %d: worst |loader - restatement| = %.3g at" % (ts, diff.max()), np.argwhere(diff == diff.max())[0])
    assert np.array_equal(tex, rtex), (diff.max(), np.argwhere(diff > 0)[:5])
    assert (tex[3] == np.float32([0.25, 0.5, 0.75])).all()                       # Kd alone: the whole cube
    assert tex[:3].std() > 0.05 and tex.min() >= 0 and tex.max() <= 1
    # texel (ts-1, 0, 0) is the image at corner 0's uv: vt 1 = (0.1, 0.2) -> pixel (0.4, 0.4) of the flipped image
    from PIL import Image
    img = (np.asarray(Image.open(os.path.join(str(tmp_path), "skin.png")).convert("RGB")).astype(np.float64) / 255)[::-1]
    want = 0.36 * img[0, 0] + 0.24 * img[1, 0] + 0.24 * img[0, 1] + 0.16 * img[1, 1]
    assert np.abs(tex[0, ts - 1, 0, 0] - want).max() < 1e-6


def test_loader_errors_name_the_file(tmp_path):
    from avatarclip_amd.texture import load_obj_texture
    good = _fixture(tmp_path)
    for ts in (1, 0):
        with pytest.raises(ValueError, match=r"body\.obj.*texture_size = %d" % ts):
            load_obj_texture(good, texture_size=ts)
    cases = {"no_mtl": dict(mtl=None), "no_image": dict(image=False), "no_vt": dict(obj=OBJ.replace("f 4/7 1/3 6/6", "f 4/7 1 6/6")),
             "no_mtllib": dict(obj=OBJ.replace("mtllib body.mtl\n", "")), "unknown": dict(obj=OBJ.replace("usemtl paint", "usemtl ink"))}
    expect = {"no_mtl": r"body\.obj.*body\.mtl does not exist", "no_image": r"body\.obj.*skin\.png does not exist",
              "no_vt": r"body\.obj: face 4 has no vt index.*skin.*map_Kd", "no_mtllib": r"body\.obj names no material file",
              "unknown": r"body\.obj uses the material ink"}
    for name, kw in cases.items():
        d = tmp_path / name
        d.mkdir()
        with pytest.raises(ValueError, match=expect[name]):
            load_obj_texture(_fixture(d, **kw))
    with pytest.raises(ValueError, match="nowhere.obj does not exist"):
        load_obj_texture(str(tmp_path / "nowhere.obj"))


def _random_weights(rs, P):
    w = rs.uniform(0, 1, (3, P)).astype(f32)
    w[:, 0] = (1, 0, 0)
    w[:, 1] = (0, 0, 1)
    return w, np.maximum(w.sum(0, dtype=f32), f32(1e-10))


@pytest.mark.parametrize("ts", [8, 2])
def test_restatement_samples_an_all_ones_texture_to_one(ts):
    rs = np.random.RandomState(1)
    w, ws = _random_weights(rs, 500)
    z = rs.uniform(0.5, 4, 3).astype(f32)
    zp = (f32(1) / ((w[0] / z[0] + w[1] / z[1] + w[2] / z[2]) / ws)).astype(f32)
    U = T.blend(np.ones((ts, ts, ts, 3), f32), w, ws, zp, z)
    assert np.abs(U - 1).max() <= 4 * np.finfo(f32).eps, np.abs(U - 1).max()


@pytest.mark.parametrize("ts", [8, 2])
def test_restatement_at_a_corner_blends_the_last_two_texels_of_that_axis(ts):
    """barycentrics (1, 0, 0): t = (ts - 1 - eps, 0, 0), so U = (1 - r) cube[ts-2,0,0] + r cube[ts-1,0,0] with r = ts - 1 - eps - (ts - 2)"""
    cube = np.random.RandomState(2).uniform(0, 1, (ts, ts, ts, 3)).astype(f32)
    z = np.float32([2, 3, 5])
    w = np.float32([[1], [0], [0]])
    U = T.blend(cube, w, np.float32([1]), z[:1].copy(), z)
    r = f32(f32(ts - 1) - f32(1e-4)) - f32(ts - 2)
    assert 0.9998 < r < 1
    assert np.array_equal(U[0], (f32(1) - r) * cube[ts - 2, 0, 0] + r * cube[ts - 1, 0, 0])


def test_restatement_fill_back_copy_samples_what_the_face_shows_from_the_other_side():
    """the copy's corners are the face's in reversed order, so its weights and depths are reversed and its cube has axes 0 and 2 swapped: the same
    eight texels with the same weights, multiplied and added in another order (8 products of 3 factors <= 1 and 8 additions: 1e-6 on values <= 1)"""
    rs = np.random.RandomState(3)
    tex = rs.uniform(0, 1, (4, 8, 8, 8, 3)).astype(f32)
    w, ws = _random_weights(rs, 300)
    z = rs.uniform(0.5, 4, 3).astype(f32)
    zp = (f32(1) / ((w[0] / z[0] + w[1] / z[1] + w[2] / z[2]) / ws)).astype(f32)
    front = T.blend(T.cube_of(tex, 2), w, ws, zp, z)
    back = T.blend(T.cube_of(tex, 4 + 2), w[::-1], ws, zp, z[::-1])
    assert np.abs(front - back).max() <= 1e-6 and front.std() > 0.01
    assert np.array_equal(T.cube_of(tex, 6)[1, 2, 3], tex[2, 3, 2, 1])


def test_the_one_walk_returns_the_sums_recorded_before_the_two_were_merged():
    """tests/golden/nr_walk.npz holds what pseudo_grad and nr_texture_restatement.backward returned while each had a scan-line walk of its own
    and its own barycentrics (commit 57481df); R.walk with either hook and R.face_weights return the same bits.  The recipe, S = 16, for the
    cases below of tests.test_gpu_raster_grad.synthetic_case: fidx = R.rasterize_index(ndc, F2, 2 S) (stored as int16), G = R.G_map(grads[0]),
    `grad` = R.pseudo_grad(ndc, F2, light, fidx, G, abs_sum=`abs_sum`, count=c), `visits` = (c["out"], c["in"]).  For "borders" also: unlit =
    RandomState(5).uniform(0, 1, (2 S, 2 S, 3)) and g3 = RandomState(6).randn(S, S, 3), both float32, (`tex_grad`, `tex_grad_light`) =
    T.backward(ndc, F2, light, fidx, unlit, g3, abs_sum=`tex_abs_sum`); and (`weights`, `weights_sum`, `weights_zp`) = T.weights(ndc[F2[f]],
    xs, ys, 2 S) at the pixels of the lowest face index f in fidx."""
    from tests.test_gpu_raster_grad import synthetic_case
    gold = np.load(os.path.join(ROOT, "tests", "golden", "nr_walk.npz"))
    S = 16
    for case in ("borders", "degenerate", "behind_camera"):
        vw, ndc, faces, F2, light, zero, grads = synthetic_case(case, S)
        fidx = R.rasterize_index(ndc, F2, 2 * S)
        assert np.array_equal(fidx, gold[case + "_fidx"]), case
        a, c = np.zeros((len(ndc), 3)), {}
        got = R.pseudo_grad(ndc, F2, light, fidx, R.G_map(grads[0]), abs_sum=a, count=c)
        assert np.abs(gold[case + "_grad"]).max() > 0 and np.array_equal(got, gold[case + "_grad"]), case
        assert np.array_equal(a, gold[case + "_abs_sum"]) and [c["out"], c["in"]] == gold[case + "_visits"].tolist(), case
        if case == "borders":
            unlit = np.random.RandomState(5).uniform(0, 1, (2 * S, 2 * S, 3)).astype(f32)
            g3 = np.random.RandomState(6).randn(S, S, 3).astype(f32)
            b = np.zeros((len(ndc), 3))
            gn, gl = T.backward(ndc, F2, light, fidx, unlit, g3, abs_sum=b)
            assert np.abs(gold["borders_tex_grad"]).max() > 0 and np.array_equal(gn, gold["borders_tex_grad"])
            assert np.array_equal(gl, gold["borders_tex_grad_light"]) and np.array_equal(b, gold["borders_tex_abs_sum"])
            f = int(np.unique(fidx[fidx >= 0])[0])
            ys, xs = np.nonzero(fidx == f)
            for got_w, name in zip(T.weights(ndc[F2[f]], xs, ys, 2 * S), ("weights", "weights_sum", "weights_zp")):
                assert got_w.dtype == f32 and np.array_equal(got_w, gold["borders_" + name]), name


def test_rgb_backward_of_an_all_ones_texture_is_the_grey_backward_of_the_channel_sum():
    from tests.test_gpu_raster_grad import synthetic_case
    S = 16
    vw, ndc, faces, F2, light, zero, grads = synthetic_case("borders", S)
    fidx = R.rasterize_index(ndc, F2, 2 * S)
    g3 = np.random.RandomState(4).randn(S, S, 3).astype(f32)
    gn, gl = T.backward(ndc, F2, light, fidx, np.ones((2 * S, 2 * S, 3), f32), g3)
    rn, rl = R.backward(ndc, F2, light, fidx, g3.sum(-1))
    assert np.array_equal(gn != 0, rn != 0) and np.abs(gn - rn).max() <= 1e-4 * np.abs(rn).max()
    assert np.abs(gl - rl).max() <= 1e-5 * np.abs(rl).max()


def test_the_texture_header_parses_and_avc_h_keeps_its_81():
    """the textured entry points live in a second header (include/ holds avc.h alone and avc.h exactly 81 prototypes, both pinned): it parses,
    every entry is a launch ending in `void* stream` that cites the reference lines it replaces, and the binding merges the two"""
    import re
    from avatarclip_amd import build, lib
    raw = open(lib.TEXTURE_HEADER).read()
    protos, abi = lib.parse_header(raw)
    assert abi is None and sorted(protos) == ["avc_rasterize_mesh_tex_grad", "avc_rasterize_mesh_tex_save"]
    for name, p in protos.items():
        assert p.launch and p.restype is lib.c_int and p.params[-1] == lib.Param("stream", lib.c_void_p, "void*", "void", False), name
        comment = raw[:raw.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert re.search(r"models/render\.py:\d+", comment), name
    names = [q.name for q in protos["avc_rasterize_mesh_tex_save"].params]
    grey, _ = lib.parse_header(open(lib.HEADER).read())
    assert len(grey) == 81 and not set(grey) & set(protos)
    base = [q.name for q in grey["avc_rasterize_mesh_save"].params]
    assert [n for n in names if n not in ("textures", "Ft", "ts", "eps", "unlit")] == base         # the grey entry point's inputs, plus these
    assert os.path.samefile(lib.TEXTURE_HEADER, os.path.join(build.CSRC, build.TEXTURE_HEADER)) and build.TEXTURE_HEADER in build.HEADERS
    assert "avc_raster_tex.hip" in build.SOURCES and "avc_raster_grad.h" in build.HEADERS
    bound = lib.load()
    assert lib.ABI_VERSION == 4 and bound.avc_version() == 4
    for name in protos:
        assert name in lib._launches and len(getattr(bound, name).argtypes) == len(protos[name].params)
    assert "avc_rasterize_mesh_save" in lib._launches


def test_render_rgb_batch_refuses_before_any_launch(monkeypatch):
    from avatarclip_amd import lib, mesh_render as M
    monkeypatch.setattr(lib, "call", lambda *a, **k: pytest.fail("a refused call reached the library"))
    v = torch.zeros(1, 4, 3)
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    eye, d = [np.float32([0, 0, 2])], [np.float32([0, 0, -1])]
    with pytest.raises(ValueError, match="cubes of 3 faces, the mesh has 2 faces"):
        M.render_rgb_batch(v, faces, torch.ones(3, 4, 4, 4, 3), eye, d)
    with pytest.raises(ValueError, match="texture_size = 1"):
        M.render_rgb_batch(v, faces, torch.ones(2, 1, 1, 1, 3), eye, d)
    with pytest.raises(ValueError, match="constants"):
        M.render_rgb_batch(v, faces, torch.ones(2, 4, 4, 4, 3, requires_grad=True), eye, d)
    with pytest.raises(ValueError, match=r"cubes \[F,ts,ts,ts,3\]"):
        M.render_rgb_batch(v, faces, torch.ones(2, 4, 4, 3, 3), eye, d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.render_rgb_batch(v, faces, torch.ones(2, 4, 4, 4, 3), eye, d)


def test_the_command_lines_take_smpl_uv_and_the_pipeline_fingerprints_it_only_when_given(tmp_path):
    from avatarclip_amd import pipeline as P
    path = _fixture(tmp_path)
    base = P.texture_fingerprint(None)
    assert base == {}                                                   # nothing joins the fingerprint of a run without a texture
    one = P.texture_fingerprint(path)
    assert set(one) == {"smpl_uv"} and one == P.texture_fingerprint(path)
    spec = P.PipelineSpec(out_dir=str(tmp_path / "out"))
    assert set(P.stage_settings(spec, "shape")) == {"neutral_txt", "target_txt", "latent_dim", "text_embeddings"}
    textured = P.PipelineSpec(out_dir=str(tmp_path / "out"), smpl_uv=path)
    assert P.stage_settings(textured, "shape") == dict(P.stage_settings(spec, "shape"), **one)
    fa, fb = P.fingerprints(spec), P.fingerprints(textured)
    assert fa["shape"] != fb["shape"] and fa == P.fingerprints(P.PipelineSpec(out_dir=str(tmp_path / "out")))
    with open(os.path.join(str(tmp_path), "body.mtl"), "w") as fh:
        fh.write(MTL.replace("Kd 0.25 0.5 0.75", "Kd 0.25 0.5 0.5"))
    assert P.texture_fingerprint(path) != one                           # the cubes are what is hashed: the .mtl and the image are part of it
    assert any("--smpl_uv" in p and "missing.obj" in p for p in P.check(P.PipelineSpec(out_dir=str(tmp_path / "out"), until_stage="shape",
                                                                                        smpl_uv=str(tmp_path / "missing.obj"))))
    assert "--smpl_uv" in P.build_parser().format_help()
    with pytest.raises(SystemExit, match="smpl_uv"):
        P.check_texture(str(tmp_path / "missing.obj"))
    P.check_texture(path)
    P.check_texture(None)


def test_animate_cli_hands_smpl_uv_to_the_context(monkeypatch):
    """python -m avatarclip_amd.animate --smpl_uv X.obj: the path reaches AnimateContext(texture=...), None without the flag (the CLI's
    third-party imports stubbed as in tests/test_animate_clip_cpu.py: only the argument handling is under test)"""
    import sys
    import types
    from avatarclip_amd import animate as A
    from avatarclip_amd import clip_vit, smpl_lbs, tokenizer
    seen = {}

    class Stop(Exception):
        pass

    def fake_ctx(*a, **kw):
        seen.update(kw)
        raise Stop

    class Blob:
        to = eval = lambda self, *a: self

    monkeypatch.setattr(A, "AnimateContext", fake_ctx)
    mods = {n: types.ModuleType(n) for n in ("human_body_prior", "human_body_prior.models", "human_body_prior.tools",
                                             "human_body_prior.models.vposer_model", "human_body_prior.tools.model_loader")}
    mods["human_body_prior.models.vposer_model"].VPoser = object
    mods["human_body_prior.tools.model_loader"].load_model = lambda *a, **k: (Blob(), None)
    for name, mod in mods.items():
        monkeypatch.setitem(sys.modules, name, mod)
    monkeypatch.setattr(clip_vit, "load_state_dict", lambda p: {})
    monkeypatch.setattr(clip_vit, "ClipVisionB32", lambda *a, **k: None)
    monkeypatch.setattr(tokenizer, "SimpleTokenizer", lambda p: None)
    monkeypatch.setattr(smpl_lbs, "load_smpl_arrays", lambda p, d: None)
    args = ["--clip_weights", "w", "--bpe", "b", "--smpl", "s", "--vposer", "v"]
    for extra, want in (([], None), (["--smpl_uv", "body.obj", "--renderer_gradient"], "body.obj")):
        seen.clear()
        with pytest.raises(Stop):
            A.main(args + extra)
        assert seen["texture"] == want and seen["renderer_gradient"] is bool(extra)


def test_animate_context_loads_a_texture_path_and_is_unchanged_without_one(tmp_path):
    from avatarclip_amd import animate as A
    from tests import animate_clip_standins as SI
    path = _fixture(tmp_path)
    ctx = A.AnimateContext(None, None, SI.smpl_arrays(0), None, device="cpu", texture=path)
    assert ctx.texture.shape == (5, 8, 8, 8, 3) and ctx.texture.dtype == torch.float32 and ctx.render_fn.__name__ == "_render_hip"
    assert A.AnimateContext(None, None, SI.smpl_arrays(0), None, device="cpu").texture is None
    with pytest.raises(ValueError, match=r"cubes \[F,ts,ts,ts,3\]"):
        A.AnimateContext(None, None, SI.smpl_arrays(0), None, device="cpu", texture=torch.ones(5, 8, 8, 3))
