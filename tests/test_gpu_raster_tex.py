"""The textured render on the MI355X (csrc/avc_raster_tex.hip behind mesh_render.render_rgb_batch): coverage bit-identical to the grey entry
point, the sampled colours and the backward against the fp32 restatement (tests/nr_texture_restatement.py, fed the device's face-index map), an
all-ones texture against the grey path, batching, determinism, the scratch, the refusals and AnimateContext(texture=...).  A hand-made mesh of
25 triangles seen by 3 cameras, at S = 32 and 17 with ts = 8 and 2; every case takes about a second."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import nr_grad_restatement as R
from tests import nr_texture_restatement as T
from tests.test_gpu_raster_grad import _kernel_grad, _save, _scratch_is_empty

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "third_party_nr_texture.npz")
WIDTH = float(np.tan(np.deg2rad(30.0)))
BOUND = 1e-5        # |image - restatement|, |unlit - restatement|: values in [0, 1]; ~30 rounded fp32 operations give t_k <= 7, slope <= 1 per unit per
#                     axis: under 5e-6, before the 8-term blend and the 4-term pool
CAMS = [(np.array([0.0, 0.0, 2.5]), np.array([0.0, 0.0, 0.0])), (np.array([1.8, 0.6, 1.6]), np.array([0.0, 0.0, 0.0])),
        (np.array([-0.3, 0.2, 1.2]), np.array([0.0, 0.0, -0.2]))]       # (the last one a close-up)


@functools.lru_cache(None)
def mesh():
    """vertices [V,3] (camera space of no one: the cameras look at it from +z) and 25 faces: a triangle larger than every view behind the rest (its
    box exceeds 1024 pixels at both raster sizes: the tile pass), two crossing faces, two with a shared edge, one with a vertex behind every
    camera, a sliver thinner than a pixel (0.01 wide; a pixel of the 64^2 raster is 0.045 at the origin), and 18 small random ones.  With the
    fill-back copies every face is back-facing once."""
    rs = np.random.RandomState(5)
    v = [(-5, -4, -0.5), (5, -4, -0.5), (0, 6, -0.5),                              # 0: larger than the view
         (-0.9, -0.2, 0.3), (0.1, -0.3, -0.3), (-0.4, 0.7, 0.0),                   # 1, 2: crossing
         (-0.9, 0.3, -0.3), (0.2, 0.2, 0.35), (-0.5, -0.7, 0.05),
         (0.3, -0.8, 0.1), (0.9, -0.7, 0.2), (0.8, -0.1, 0.1), (0.25, -0.2, 0.3),   # 3, 4: a shared edge (9 - 11)
         (0.5, 0.5, 0.2), (0.9, 0.8, 0.0), (0.6, 0.9, 4.0),                        # 5: one vertex behind every camera
         (-1.0, 0.85, 0.4), (1.0, 0.9, 0.4), (1.0, 0.91, 0.4)]                     # 6: a sliver
    f = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11), (9, 11, 12), (13, 14, 15), (16, 17, 18)]
    for _ in range(18):
        c = rs.uniform(-1, 1, 3) * (1, 1, 0.3)
        f.append((len(v), len(v) + 1, len(v) + 2))
        v += [tuple(c + rs.uniform(-0.3, 0.3, 3) * (1, 1, 0.3)) for _ in range(3)]
    return np.asarray(v, np.float32), np.asarray(f, np.int64)


def _cam():
    from avatarclip_amd.smpl_prior import camera_frame
    return np.stack([camera_frame(e.astype(np.float32), ((a - e) / np.linalg.norm(a - e)).astype(np.float32)) for e, a in CAMS]).astype(np.float32)


@functools.lru_cache(None)
def inputs(ts):
    """(vw [3,V,3], faces2 int32 [2F,3], cam [3,12], light [3,2F], cubes [F,ts,ts,ts,3]) numpy: shared by the tests, never written"""
    v, f = mesh()
    rs = np.random.RandomState(11 + ts)
    f2 = np.concatenate([f, f[:, ::-1]]).astype(np.int32)
    out = (np.tile(v, (3, 1, 1)), f2, _cam(), rs.uniform(0.5, 1.0, (3, len(f2))).astype(np.float32), rs.uniform(0, 1, (len(f), ts, ts, ts, 3)).astype(np.float32))
    for a in out:
        a.setflags(write=False)
    return out


def _dev(*arrays):
    return [torch.tensor(a).cuda() for a in arrays]        # (a copy: the shared inputs are read-only)


def _tex_save(vw, faces2, cam, light, tex, S, eps=1e-4):
    """avc_rasterize_mesh_tex_save on its own fresh 0xFF scratch, outputs pre-filled with garbage -> (image, unlit, ndc, fidx, scratch)"""
    from avatarclip_amd import lib as L
    from avatarclip_amd.mesh_render import NEAR, FAR
    lib = L.load()
    N, V = vw.shape[:2]
    F2n, (Ft, ts) = faces2.shape[0], tex.shape[:2]
    img = torch.full((N, S, S, 3), float("nan"), device="cuda")
    unlit = torch.full((N, 2 * S, 2 * S, 3), float("nan"), device="cuda")
    ndc = torch.full((N, V, 3), float("nan"), device="cuda")
    fidx = torch.full((N, 2 * S, 2 * S), 7, dtype=torch.int32, device="cuda")
    scratch = torch.full((N * lib.avc_rasterize_scratch_bytes(F2n, 2 * S),), 255, dtype=torch.uint8, device="cuda")
    L.call("avc_rasterize_mesh_tex_save", vw, N, V, faces2, F2n, cam, WIDTH, light, tex, Ft, ts, eps, S, NEAR, FAR, ndc, img, unlit, fidx, scratch)
    return img, unlit, ndc, fidx, scratch


def _tex_grad(g, ndc, fidx, unlit, light, faces2, vf_ptr, vf_ent, S, eps=1e-4):
    """avc_rasterize_mesh_tex_grad on the saved state, outputs pre-filled with NaN (every entry must be written) -> (grad_ndc, grad_light)"""
    from avatarclip_amd import lib as L
    N, V = ndc.shape[:2]
    F2n = faces2.shape[0]
    fg, gn, gl = (torch.full(s, float("nan"), device="cuda") for s in ((N, F2n, 6), (N, V, 3), (N, F2n)))
    L.call("avc_rasterize_mesh_tex_grad", g, ndc, N, V, faces2, F2n, light, unlit, fidx, S, eps, vf_ptr, vf_ent, fg, gn, gl)
    return gn, gl


def _criterion(gn, gl, rg, rl, what):
    """tests/test_gpu_raster_grad.py's: the same non-zero set, 1e-4 of the largest entry, light 1e-5"""
    assert np.array_equal(gn != 0, rg != 0), (what, (gn != 0).sum(), (rg != 0).sum(), np.argwhere((gn != 0) != (rg != 0))[:5])
    tol = 1e-4 * np.abs(rg).max() + 1e-6
    print(what, "worst |grad_ndc - reference| %.3g (bound %.3g), |grad_light - reference| %.3g" % (np.abs(gn - rg).max(), tol, np.abs(gl - rl).max()))
    assert np.abs(gn - rg).max() <= tol, (what, np.abs(gn - rg).max(), tol)
    assert np.array_equal(gl != 0, rl != 0), what
    assert np.abs(gl - rl).max() <= 1e-5 * max(np.abs(rl).max(), 1e-30) + 1e-7, (what, np.abs(gl - rl).max())
    assert (gn[:, 2] == 0).all() and np.abs(rg).max() > 0, what


@gpu
@pytest.mark.parametrize("ts", [8, 2])
@pytest.mark.parametrize("S", [32, 17])
def test_forward(S, ts):
    vw_h, f2_h, cam_h, lt_h, tex_h = inputs(ts)
    vw, f2, cam, lt, tex = _dev(vw_h, f2_h, cam_h, lt_h, tex_h)
    n, Ft = 2 * S, len(tex_h)
    img, unlit, ndc, fidx, scratch = _tex_save(vw, f2, cam, lt, tex, S)
    assert _scratch_is_empty(scratch, 3, len(f2_h), S)                           # left 0xFF
    # coverage and depth are the grey entry point's launches: ndc and the face-index map bit for bit
    gimg, gndc, gfidx, _ = _save(vw, f2, cam, lt, S, WIDTH)
    assert torch.equal(ndc, gndc) and torch.equal(fidx, gfidx)
    fi = fidx.cpu().numpy()
    assert ((fi == 0) | (fi == Ft)).mean() > 0.2 and (fi >= Ft).any() and ((fi > 0) & (fi < Ft)).any()      # the tile pass's face, copies, originals
    assert (ndc[:, 15] == 0).all() and (ndc[:, 14, 2] > 0).all()                # vertex 15 is behind every camera: (0, 0, 0)
    worst = 0.0
    for i in range(3):
        U = T.unlit_map(ndc[i].cpu().numpy(), f2_h, fi[i], tex_h)
        image = T.pooled_image(U, fi[i], lt_h[i])
        eu, ei = np.abs(unlit[i].cpu().numpy() - U).max(), np.abs(img[i].cpu().numpy() - image).max()
        print("S = %d ts = %d render %d: worst |unlit - restatement| %.3g, |image - restatement| %.3g (bound %g); covered %.2f"
              % (S, ts, i, eu, ei, BOUND, (fi[i] >= 0).mean()))
        assert (unlit[i].cpu().numpy()[fi[i] < 0] == 0).all() and U.std() > 0.05
        worst = max(worst, eu, ei)
    assert worst <= BOUND, worst
    # two runs: identical bits
    again = _tex_save(vw, f2, cam, lt, tex, S)
    assert all(torch.equal(a, b) for a, b in zip((img, unlit, ndc, fidx), again))
    # the batch of three against three single renders
    for i in range(3):
        one = _tex_save(vw[i:i + 1].contiguous(), f2, cam[i:i + 1].contiguous(), lt[i:i + 1].contiguous(), tex, S)
        assert all(torch.equal(a[0], b[i]) for a, b in zip(one[:4], (img, unlit, ndc, fidx))), i
        assert _scratch_is_empty(one[4], 1, len(f2_h), S)
    # an all-ones texture is the grey render in every channel
    white = _tex_save(vw, f2, cam, lt, torch.ones_like(tex), S)[0]
    d = (white - gimg[..., None]).abs().max().item()
    print("all-ones texture against the grey entry point: %.3g" % d)
    assert d <= BOUND and gimg.max() > 0.4


@gpu
@pytest.mark.parametrize("ts", [8, 2])
@pytest.mark.parametrize("S", [32, 17])
def test_backward(S, ts):
    from avatarclip_amd import mesh_render as M
    vw_h, f2_h, cam_h, lt_h, tex_h = inputs(ts)
    vw, f2, cam, lt, tex = _dev(vw_h, f2_h, cam_h, lt_h, tex_h)
    _, _, vf_ptr, vf_ent = M._topology(mesh()[1], vw_h.shape[1], "cuda")
    img, unlit, ndc, fidx, _ = _tex_save(vw, f2, cam, lt, tex, S)
    g_h = np.random.RandomState(S + ts).randn(3, S, S, 3).astype(np.float32)
    g, = _dev(g_h)
    outs = [_tex_grad(g, ndc, fidx, unlit, lt, f2, vf_ptr, vf_ent, S) for _ in range(2)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])           # two runs: identical bits
    gn, gl = outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()
    for i in range(3):                                                  # the saved state is the backward's input: the restatement gets the device's
        rg, rl = T.backward(ndc[i].cpu().numpy(), f2_h, lt_h[i], fidx[i].cpu().numpy(), unlit[i].cpu().numpy(), g_h[i])
        _criterion(gn[i], gl[i], rg, rl, "S = %d ts = %d render %d:" % (S, ts, i))
    # an all-ones texture: the grey path's gradients under g_grey = sum_c g_c
    ones = torch.ones_like(tex)
    _, unlit1, ndc1, fidx1, _ = _tex_save(vw, f2, cam, lt, ones, S)
    gn1, gl1 = (t.cpu().numpy() for t in _tex_grad(g, ndc1, fidx1, unlit1, lt, f2, vf_ptr, vf_ent, S))
    kn, kl = (t.cpu().numpy() for t in _kernel_grad(g.sum(-1).contiguous(), ndc1, fidx1, lt, f2, vf_ptr, vf_ent, S))
    for i in range(3):
        _criterion(gn1[i], gl1[i], kn[i].astype(np.float64), kl[i].astype(np.float64), "all-ones, S = %d render %d:" % (S, i))


@gpu
def test_render_rgb_batch_wraps_the_entry_points_with_autograd():
    """the wrapper makes the same calls (rot_mat, face light, cameras) as render_grey_batch: an all-ones texture gives its image in three channels
    and its vertex gradient under the channel sum; the gradient reaches v_world through the projection and the light"""
    from avatarclip_amd import mesh_render as M
    v, f = mesh()
    S = 32
    eyes = [e.astype(np.float32) for e, _ in CAMS]
    dirs = [((a - e) / np.linalg.norm(a - e)).astype(np.float32) for e, a in CAMS]
    tex = torch.from_numpy(inputs(8)[4]).cuda()
    vw = torch.from_numpy(v).cuda()[None].repeat(3, 1, 1).requires_grad_(True)
    img, ndc, fidx, unlit = M.render_rgb_batch(vw, f, tex, eyes, dirs, image_size=S, return_state=True)
    assert img.shape == (3, 3, S, S) and unlit.shape == (3, 2 * S, 2 * S, 3) and img.requires_grad and not fidx.requires_grad
    assert img.std() > 0.05 and (img[:, 0] != img[:, 1]).any()
    g = torch.randn(img.shape, generator=torch.Generator().manual_seed(0)).cuda()
    img.backward(g)
    assert torch.isfinite(vw.grad).all() and vw.grad.abs().max() > 0
    v1 = vw.detach().clone().requires_grad_(True)
    white = M.render_rgb_batch(v1, f, torch.ones_like(tex), eyes, dirs, image_size=S)
    v2 = vw.detach().clone().requires_grad_(True)
    grey = M.render_grey_batch(v2, f, eyes, dirs, image_size=S)
    assert (white - grey[:, None]).abs().max() <= BOUND
    white.backward(g)
    grey.backward(g.sum(1))
    assert (v1.grad - v2.grad).abs().max() <= 1e-4 * v2.grad.abs().max() + 1e-6


@gpu
def test_refusals_come_before_any_launch(monkeypatch):
    from avatarclip_amd import lib, mesh_render as M
    v, f = mesh()
    eyes, dirs = [np.float32([0, 0, 2.5])], [np.float32([0, 0, -1])]
    vw = torch.from_numpy(v).cuda()[None]
    tex = torch.from_numpy(inputs(8)[4]).cuda()
    monkeypatch.setattr(lib, "call", lambda *a, **k: pytest.fail("a refused call reached the library"))
    with pytest.raises(ValueError, match="cubes of %d faces, the mesh has %d faces" % (len(f) - 1, len(f))):
        M.render_rgb_batch(vw, f, tex[:-1], eyes, dirs, image_size=16)
    with pytest.raises(ValueError, match="texture_size = 1"):
        M.render_rgb_batch(vw, f, tex[:, :1, :1, :1], eyes, dirs, image_size=16)
    with pytest.raises(ValueError, match="constants"):
        M.render_rgb_batch(vw, f, tex.clone().requires_grad_(True), eyes, dirs, image_size=16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.render_rgb_batch(vw, f, tex.cpu(), eyes, dirs, image_size=16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.render_rgb_batch(vw.cpu(), f, tex, eyes, dirs, image_size=16)


@gpu
def test_the_c_abi_refuses_sizes_that_would_read_outside_the_cubes():
    vw, f2, cam, lt, tex = _dev(*inputs(8))
    for bad, kw in (("ts", dict(tex=tex[:, :1, :1, :1].contiguous())), ("Ft", dict(tex=tex[:-1].contiguous())), ("eps", dict(eps=1.5))):
        with pytest.raises(RuntimeError, match="F is not Ft or 2 Ft, ts is outside"):
            _tex_save(vw, f2, cam, lt, kw.get("tex", tex), 16, kw.get("eps", 1e-4))


@gpu
def test_animate_context_renders_the_textured_body():
    from avatarclip_amd import animate as A
    from tests import animate_clip_standins as SI
    dev = torch.device("cuda")
    smpl = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in SI.smpl_arrays().items()}
    tex = torch.from_numpy(np.random.RandomState(0).uniform(0, 1, (SI.NF, 8, 8, 8, 3)).astype(np.float32))
    per = SI.Perceptor().to(dev)
    kw = dict(device=dev, image_size=64, renderer_gradient=True)
    white, textured = A.AnimateContext(per, None, smpl, None, **kw), A.AnimateContext(per, None, smpl, None, texture=tex, **kw)
    assert white.texture is None and textured.texture.is_cuda
    pose = torch.zeros(63, device=dev)
    feats, images = [], []
    for ctx in (white, textured):
        np.random.seed(0)
        with torch.no_grad():
            images.append(ctx.render_fn(ctx.posed_vertices(pose), smpl["faces"], A.DEFAULT_ANGLES))
            np.random.seed(0)
            feats.append(ctx.get_pose_feature(pose))
    assert images[0].shape == images[1].shape == (len(A.DEFAULT_ANGLES), 3, 64, 64)
    assert torch.equal(images[0][:, 0], images[0][:, 1]) and torch.equal(images[0][:, 0], images[0][:, 2]) and images[0].max() > 0.4      # still one grey value
    assert (images[1][:, 0] != images[1][:, 1]).any()
    assert (feats[0] - feats[1]).abs().max() > 1e-3
    # without a gradient the same textured path
    plain = A.AnimateContext(per, None, smpl, None, device=dev, image_size=64, texture=tex)
    np.random.seed(0)
    assert torch.equal(plain.render_fn(textured.posed_vertices(pose), smpl["faces"], A.DEFAULT_ANGLES), images[1])
    # the pose gradient through the textured render, and two PoseOptimizer iterations
    p = pose.clone().requires_grad_(True)
    tf = torch.randn(512, generator=torch.Generator().manual_seed(1)).to(dev)
    np.random.seed(1)
    loss = 1 - torch.nn.functional.cosine_similarity(textured.get_pose_feature(p).squeeze(0), tf, dim=-1)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0
    torch.manual_seed(2)
    np.random.seed(2)
    out = A.PoseOptimizer(textured, num_iteration=2, topk=1).get_pose(tf)
    assert out.shape == (69,) and torch.isfinite(out).all()
    with pytest.raises(ValueError, match="cubes of %d faces, the mesh has %d faces" % (SI.NF - 1, SI.NF)):
        A.AnimateContext(per, None, smpl, None, texture=tex[:-1], **kw).get_pose_feature(pose)


@gpu
def test_against_the_neural_renderer_golden_when_it_is_pinned():
    """scripts/pin_third_party.py writes tests/golden/third_party_nr_texture.npz where neural_renderer can be imported; until then the rules
    are unpinned against it and this test says so"""
    if not os.path.exists(GOLDEN):
        print("unpinned: no %s (neural_renderer's own output has not been recorded)" % os.path.relpath(GOLDEN))
        return
    from avatarclip_amd import mesh_render as M
    from avatarclip_amd.texture import load_obj_texture
    from tests.test_texture_cpu import _fixture
    z = np.load(GOLDEN)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        _, lf, lt = load_obj_texture(_fixture(d))
    assert np.array_equal(lf, z["loader_faces"]) and np.abs(lt - z["loader_textures"]).max() <= 1e-6
    tex = torch.from_numpy(z["textures"]).cuda()
    vw = torch.from_numpy(z["vertices"]).cuda().requires_grad_(True)
    img = M.render_rgb_batch(vw, z["faces"], tex, list(z["eyes"]), list(z["directions"]), image_size=int(z["image_size"]))
    assert (img.detach().cpu().numpy() - z["images"]).__abs__().max() <= BOUND
    img.backward(torch.from_numpy(z["grad_images"]).cuda())
    assert np.abs(vw.grad.cpu().numpy() - z["grad_vertices"]).max() <= 1e-4 * np.abs(z["grad_vertices"]).max() + 1e-6
