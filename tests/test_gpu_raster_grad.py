"""The rasteriser's forward entry points and neural_renderer's approximate backward on the MI355X (csrc/avc_raster.hip, avc_raster_grad.hip behind
avatarclip_amd.mesh_render): images bit-identical to MeshPrior's, the face-index map and the backward against the fp32 restatement
(tests/nr_grad_restatement.py) at production size and on adversarial meshes, the single-render and face-list forms against the same restatement,
batched renders against single ones, the scratch the calls leave behind, F = 0 at the C ABI, determinism, and the paper's silhouette-fitting
experiment."""
import os

import numpy as np
import pytest
import torch

from tests import nr_grad_restatement as R

gpu = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smpl_views.npz")
CAMS = [(np.array([0.2, 0.3, 1.6]), np.array([0.0, -0.1, 0.05])), (np.array([-1.3, -0.4, -0.9]), np.array([0.05, 0.1, 0.0])),
        (np.array([0.05, 1.5, 0.6]), np.array([0.0, 0.2, 0.0])), (np.array([1.4, 0.2, -0.6]), np.array([0.0, 0.0, 0.0])),
        (np.array([0.05, 0.35, 0.55]), np.array([0.0, 0.3, 0.0]))]       # (the last one a close-up: faces for the tile-parallel pass)


def _template():
    z = np.load(GOLD)
    return z["mesh_v"].astype(np.float32), z["mesh_f"].astype(np.int64)


def _dirs(cams):
    eyes = [e.astype(np.float32) for e, _ in cams]
    dirs = [((a - e) / np.linalg.norm(a - e)).astype(np.float32) for e, a in cams]
    return eyes, dirs


@gpu
def test_forward_with_save_is_bit_identical_to_the_prior_render():
    from avatarclip_amd.mesh_render import render_grey_batch
    from avatarclip_amd.smpl_prior import MeshPrior
    V, Fc = _template()
    eyes, dirs = _dirs(CAMS)
    vw = torch.from_numpy(V).cuda()[None].expand(len(CAMS), -1, -1).contiguous()
    img, ndc, fidx = render_grey_batch(vw, Fc, eyes, dirs, image_size=256, return_state=True)
    prior = MeshPrior(V, Fc, device="cuda")
    light = prior.light2.cpu().numpy()
    for i, (e, d) in enumerate(zip(eyes, dirs)):
        ref = prior.render_grey(e, d)
        assert torch.equal(img[i], ref), (i, (img[i] - ref).abs().max())
        fi = fidx[i].cpu().numpy()
        assert fi.min() >= -1 and fi.max() < 2 * len(Fc) and (fi >= 0).mean() > 0.01
        assert np.array_equal(R.pooled_image(fi, light), img[i].cpu().numpy())          # pooling light[I] reproduces the image bit for bit
    assert torch.isfinite(ndc).all()


def _random_mesh(rs, nv=40, nf=60):
    v = rs.uniform(-0.6, 0.6, (nv, 3)).astype(np.float32)
    f = np.stack([rs.choice(nv, 3, replace=False) for _ in range(nf)]).astype(np.int64)
    return v, f


# per vertex component |kernel - restatement| <= ABS_K * (the sum of |term| over its terms): the two sum the same fp32 terms in different orders
# (the kernel in fp32 per lane, then a wave reduction and the vertex gather; the restatement in float64).  Measured on the MI355X: at most
# 4.0e-7 over every case here (odd_sizes at S = 100; 2.4e-7 at S = 256).
ABS_K = 2e-6


def _kernel_grad(g, ndc, fidx, light2, faces2, vf_ptr, vf_ent, S, eps=1e-4):
    """avc_rasterize_mesh_grad on the saved state, outputs pre-filled with NaN (every entry must be written) -> (grad_ndc, grad_light)"""
    from avatarclip_amd import lib as L
    N, V = ndc.shape[:2]
    F2n = faces2.shape[0]
    nan = float("nan")
    fg = torch.full((N, F2n, 6), nan, device="cuda")
    gn = torch.full((N, V, 3), nan, device="cuda")
    gl = torch.full((N, F2n), nan, device="cuda")
    L.check(L.load().avc_rasterize_mesh_grad(L.ptr(g), L.ptr(ndc), N, V, L.ptr(faces2), F2n, L.ptr(light2), L.ptr(fidx), S, eps, L.ptr(vf_ptr),
                                             L.ptr(vf_ent), L.ptr(fg), L.ptr(gn), L.ptr(gl), L.stream()), "grad")
    return gn, gl


def _compare(gn, gl, ndc, F2, light, fidx, gi, eps=1e-4, what="", zero_rows=(), nonzero=False):
    """one render's kernel gradients (numpy) against the restatement: _check_backward's assertions + the per-component bound; -> worst
    |gn - rg| / (abs_sum) over the entries with terms"""
    a = np.zeros((ndc.shape[0], 3))
    rg, rl = R.backward(ndc, F2, light, fidx, gi, eps, abs_sum=a)
    assert np.array_equal(gn != 0, rg != 0), (what, (gn != 0).sum(), (rg != 0).sum(), np.argwhere((gn != 0) != (rg != 0))[:5])
    tol = 1e-4 * np.abs(rg).max() + 1e-6
    assert np.abs(gn - rg).max() <= tol, (what, np.abs(gn - rg).max(), tol)
    err = np.abs(gn.astype(np.float64) - rg)
    assert (err <= ABS_K * a + 1e-30).all(), (what, np.argwhere(err > ABS_K * a + 1e-30)[:5], (err / np.maximum(a, 1e-300)).max())
    assert np.array_equal(gl != 0, rl != 0), what
    assert np.abs(gl - rl).max() <= 1e-5 * max(np.abs(rl).max(), 1e-30) + 1e-7, what
    assert (rg[:, 2] == 0).all() and (gn[:, 2] == 0).all(), what
    assert np.abs(rg).max() > 0 or not nonzero, what
    for r in zero_rows:
        assert (gn[r] == 0).all() and (rg[r] == 0).all(), (what, r)
    if not np.asarray(gi).any():
        assert not gn.any() and not gl.any(), what         # no upstream gradient, exactly nothing
    m = a > 0
    return float((err[m] / a[m]).max()) if m.any() else 0.0


def _check_backward(V, Fc, cams, S, seed):
    from avatarclip_amd.mesh_render import render_grey_batch
    eyes, dirs = _dirs(cams)
    vw = torch.from_numpy(V).cuda()[None].repeat(len(cams), 1, 1).requires_grad_(True)
    img, ndc, fidx = render_grey_batch(vw, Fc, eyes, dirs, image_size=S, return_state=True)
    g = torch.randn(img.shape, generator=torch.Generator().manual_seed(seed)).cuda()
    F2 = np.concatenate([Fc, Fc[:, ::-1]])
    from avatarclip_amd import mesh_render as M
    # the kernel's own outputs (grad_ndc, grad_light) for the comparison: the same call the autograd Function makes
    faces2, f, vf_ptr, vf_ent = M._topology(Fc, V.shape[0], vw.device)
    v = vw.detach() @ torch.tensor(M.ROT_MAT, device="cuda")
    light2 = torch.stack([M.face_light(v[i], f) for i in range(len(cams))]).contiguous()
    N = len(cams)
    outs = [_kernel_grad(g, ndc, fidx, light2, faces2, vf_ptr, vf_ent, S) for _ in range(2)]
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])       # deterministic: two calls bit-identical
    gn, gl = outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()
    worst = []
    for i in range(N):
        worst.append(_compare(gn[i], gl[i], ndc[i].cpu().numpy(), F2, light2[i].cpu().numpy(), fidx[i].cpu().numpy(), g[i].cpu().numpy(),
                              what="render %d" % i, nonzero=True))
    print("S = %d: worst |kernel - restatement| / sum|term| per render" % S, ["%.2e" % w for w in worst], "bound %.0e" % ABS_K)
    # and through autograd: the Function returns the projection Jacobian applied to the same grad_ndc
    img.backward(g)
    ref = M.project_vjp(v, M.h2d.upload(np.stack([M.camera_frame(e, d) for e, d in zip(eyes, dirs)]).reshape(-1), "cuda").reshape(N, 12),
                        float(np.tan(np.deg2rad(30.0))), outs[0][0])
    rot = torch.tensor(M.ROT_MAT, device="cuda")
    assert torch.isfinite(vw.grad).all() and vw.grad.abs().max() > 0
    # the light's share through the face normals comes on top of the projection's
    vl = (vw.detach() @ rot).requires_grad_(True)
    torch.autograd.backward([(M.face_light(vl[i], f) * outs[0][1][i]).sum() for i in range(N)])
    assert torch.allclose(vw.grad, (ref + vl.grad) @ rot.t(), rtol=1e-4, atol=1e-5 * float(vw.grad.abs().max()))


@gpu
def test_backward_matches_the_restatement_on_a_small_random_mesh():
    rs = np.random.RandomState(3)
    V, Fc = _random_mesh(rs)
    _check_backward(V, Fc, [(np.array([0.3, 0.2, 2.0]), np.zeros(3)), (np.array([-1.5, 0.5, 1.2]), np.zeros(3))], 32, 0)


@gpu
def test_backward_matches_the_restatement_on_the_template():
    V, Fc = _template()
    _check_backward(V, Fc, [CAMS[0], CAMS[3]], 64, 1)


@gpu
def test_silhouette_fitting_recovers_a_translation():
    """Kato et al.'s experiment: a translation of the template optimised (Adam, L2 on the image) so its render matches a target rendered at a
    known offset; thresholds chosen with the CPU restatement at the same size (there: IoU 0.33 at the start, 0.76 after 60 steps at lr 0.02)"""
    from avatarclip_amd.mesh_render import render_grey_batch
    V, Fc = _template()
    eyes, dirs = _dirs(CAMS[:1])
    v0 = torch.from_numpy(V).cuda()
    off = torch.tensor([0.1, 0.0, 0.08], device="cuda")
    with torch.no_grad():
        target = render_grey_batch((v0 + off)[None], Fc, eyes, dirs, image_size=32)[0]
    t = torch.zeros(3, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([t], lr=0.02)
    iou = lambda a: float(((a > 0) & (target > 0)).sum()) / float(((a > 0) | (target > 0)).sum())
    ious = []
    for _ in range(60):
        img = render_grey_batch((v0 + t)[None], Fc, eyes, dirs, image_size=32)[0]
        ious.append(iou(img.detach()))
        loss = ((img - target) ** 2).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
    print("silhouette fit IoU", ious[0], "->", ious[-1], "t", t.detach().cpu().numpy())
    assert ious[0] < 0.5 and max(ious[-5:]) > FINAL_IOU


FINAL_IOU = 0.7


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Production size, batching, the scratch and the C ABI's edges; adversarial meshes placed in NDC and fed to the entry points directly.

BEHIND = (np.array([0.1, 0.0, 0.22]), np.array([0.0, 0.1, 0.0]))     # test_smpl_prior.py's close-up: part of the body behind the camera
# the camera at the origin with the world axes as its frame and width 1: ndc = (x / z, y / z, z), exact for depths z that are powers of two
IDENT_CAM = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)


def _centre_ndc(k, n):
    """the fp32 ndc closest to (2 k + 1 - n) / n whose pixel coordinate P = 0.5 (ndc n + n - 1) is exactly k, or None (for some k no fp32 is)"""
    c = np.float32((2.0 * k + 1 - n) / n)
    up, dn = [c], [c]
    for _ in range(4):
        up.append(np.nextafter(up[-1], np.float32(np.inf)))
        dn.append(np.nextafter(dn[-1], np.float32(-np.inf)))
    return next((x for pair in zip(up, dn) for x in pair if R.pixel_coords(np.float32([x, x]), n)[0] == k), None)


def _on_centre(t, n):
    """an integer pixel coordinate near t n that a vertex can sit on exactly"""
    return float(next(k for k in (int(t * n) + d for d in (0, 1, -1, 2, -2, 3, -3)) if _centre_ndc(k, n) is not None))


def _px(p, n):
    """the fp32 ndc of pixel coordinates p; an integer p is placed exactly on the pixel centre where an fp32 can be"""
    p = np.asarray(p, np.float64)
    nd = ((2 * p + 1 - n) / n).astype(np.float32)
    for i in zip(*np.nonzero(p == np.round(p))):
        c = _centre_ndc(p[i], n)
        nd[i] = nd[i] if c is None else c
    return nd


def _place(P, z, n):
    """pixel-space positions P [V,2] at depths z [V] (powers of two; <= 0: behind the camera) -> world vertices [V,3] and the ndc the
    projection must give ([V,3], (0, 0, 0) behind the camera)"""
    nd = _px(P, n)
    z = np.broadcast_to(np.asarray(z, np.float32), (len(nd),))
    front = z > 0
    vw = np.concatenate([nd * np.where(front, z, 1)[:, None], z[:, None]], 1).astype(np.float32)
    ndc = np.where(front[:, None], np.concatenate([nd, z[:, None]], 1), 0).astype(np.float32)
    return vw, ndc


def _tri_around(c, r, th, rs):
    return [(c[0] + r * np.cos(th + t + rs.uniform(-0.3, 0.3)), c[1] + r * np.sin(th + t + rs.uniform(-0.3, 0.3))) for t in (0, 2.1, 4.2)]


def _axis_aligned(n, rs):
    """rectangles (two triangles each) and a right triangle: horizontal and vertical edges, corners exactly on pixel centres and off them"""
    k = lambda t: _on_centre(t, n)
    P = [(k(.15), k(.2)), (k(.55), k(.2)), (k(.55), k(.6)), (k(.15), k(.6)),                         # on pixel centres, depth 2
         (k(.4) + .37, k(.45) + .29), (k(.85) + .61, k(.45) + .29), (k(.85) + .61, k(.9) + .5), (k(.4) + .37, k(.9) + .5),   # off them, depth 4
         (k(.3), k(.3)), (k(.42), k(.3)), (k(.3), k(.45) + .5)]                                   # a corner on a centre, depth 1
    z = [2] * 4 + [4] * 4 + [1] * 3
    return P, z, [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7], [8, 9, 10]], []


def _borders(n, rs):
    """a triangle across each border and each corner of the image, and one larger than the whole image behind them (the tile pass)"""
    e = -0.5
    anchors = [(e, .3 * n), (n + e, .6 * n), (.7 * n, e), (.35 * n, n + e), (e, e), (n + e, e), (e, n + e), (n + e, n + e)]
    P = []
    for a in anchors:
        P += _tri_around(a, rs.uniform(.12, .3) * n, rs.uniform(0, 6.3), rs)
    P += [(.5 * (-3 * n + n - 1), .5 * (-3 * n + n - 1)), (.5 * (5 * n + n - 1), .5 * (-3 * n + n - 1)), (.5 * (-3 * n + n - 1), .5 * (5 * n + n - 1))]
    return P, [2] * 24 + [8] * 3, [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(9)], []


def _behind(n, rs):
    """faces with one vertex behind the camera (z < 0 and z = 0: ndc (0, 0, 0)) among ordinary ones"""
    c = (.5 * n + 3.3, .5 * n - 2.1)
    P = [c] + [(c[0] + .3 * n * np.cos(t), c[1] + .3 * n * np.sin(t)) for t in (0.3, 1.9, 3.4, 5.0)] + [(5.0, 7.0), (-3.0, 2.0)]
    z = [2, 2, 2, 2, 2, -1, 0]
    return P, z, [[0, 1, 2], [0, 2, 3], [0, 3, 5], [3, 4, 6], [0, 4, 1], [1, 5, 2]], []


def _degenerate(n, rs):
    """a face, its duplicate and a rotated duplicate (z-ties: the lower index wins), a second face in the same plane over it (ties between
    different faces), a colinear face, a face with two coincident vertices and one with a repeated index"""
    P = [(.2 * n, .2 * n), (.7 * n + .3, .3 * n), (.4 * n, .75 * n + .4),
         (.1 * n, .8 * n), (.5 * n, .9 * n), (.3 * n, .85 * n),          # colinear
         (.8 * n, .1 * n), (.8 * n, .1 * n), (.9 * n, .4 * n),           # two coincident
         (.35 * n, .1 * n), (.9 * n, .6 * n), (.1 * n, .6 * n)]          # the same depth as the first face
    return P, [2] * 12, [[0, 1, 2], [0, 1, 2], [1, 2, 0], [9, 10, 11], [3, 4, 5], [6, 7, 8], [8, 8, 3], [11, 0, 2]], []


def _subpixel(n, rs):
    """faces that cover no pixel centre (inside one pixel, or slivers across a scan line or two): exactly zero gradient on their vertices"""
    P = [(.1 * n, .1 * n), (.9 * n, .2 * n), (.5 * n, .8 * n)]
    z = [4, 4, 4]
    faces = [[0, 1, 2]]
    for (k, j) in [(int(.5 * n), int(.4 * n)), (int(.45 * n), int(.3 * n)), (int(.2 * n), int(.85 * n)), (int(.9 * n), int(.9 * n))]:
        for q in ([(.1, .1), (.45, .15), (.2, .4)], [(.6, .1), (1.4, .2), (.9, .4)], [(.5, 1.3), (1.3, .5), (1.32, .52)]):
            faces.append([len(P), len(P) + 1, len(P) + 2])
            P += [(k + a, j + b) for a, b in q]
            z += [2, 2, 2]
    return P, z, faces, list(range(3, len(P)))


def _fan(n, rs):
    """320 thin faces around one vertex on a pixel centre (its vertex -> face list holds 640 entries), and five isolated vertices"""
    m = 320
    c = (_on_centre(.48, n), _on_centre(.53, n))
    th = 2 * np.pi * np.arange(m) / m + rs.uniform(0, 0.01, m)
    r = n * rs.uniform(.2, .4, m)
    P = [c] + list(zip(c[0] + r * np.cos(th), c[1] + r * np.sin(th))) + [tuple(rs.uniform(0, n, 2)) for _ in range(5)]
    z = [2] + [2, 4] * (m // 2) + [2] * 5
    return P, z, [[0, 1 + i, 1 + (i + 1) % m] for i in range(m)], list(range(m + 1, m + 6))


def _odd(n, rs):
    """V = 257 (not a multiple of the 256-thread blocks) and F = 131 (odd; neither is a multiple of the four waves per block)"""
    V, F = 257, 131
    P = rs.uniform(-.1 * n, 1.1 * n, (V, 2))
    faces = np.stack([rs.choice(V - 7, 3, replace=False) for _ in range(F)])
    faces[0, 0] = V - 1                      # the last vertex has a face; V - 7 .. V - 2 are isolated
    return P, rs.choice([2, 4, 8], V), faces, list(range(V - 7, V - 1))


SYNTH = {"axis_aligned": _axis_aligned, "borders": _borders, "behind_camera": _behind, "degenerate": _degenerate, "subpixel": _subpixel,
         "fan": _fan, "odd_sizes": _odd}


def synthetic_case(name, S, seed=0):
    """(world vertices [V,3], the ndc they project to [V,3], faces [F,3], fill_back face list [2F,3], light [2F], vertices that must get no
    gradient, upstream gradients [5,S,S]: normal, positive, negative, one-hot at a pixel on a face's border, zero) -- numpy, no device"""
    n = 2 * S
    rs = np.random.RandomState(seed)
    P, z, faces, zero = SYNTH[name](n, rs)
    vw, ndc = _place(np.asarray(P, np.float64), np.asarray(z, np.float32), n)
    assert np.isfinite(ndc).all()
    faces = np.asarray(faces, np.int64)
    F2 = np.concatenate([faces, faces[:, ::-1]])
    light = rs.uniform(0.5, 1.0, len(F2)).astype(np.float32)
    alone = np.isin(F2, zero).all(1)
    assert (R.rasterize_index(ndc, F2[alone], n) == -1).all()            # the faces of the zero-gradient vertices cover no pixel centre
    img = R.pooled_image(R.rasterize_index(ndc, F2, n), light)
    g = rs.randn(S, S).astype(np.float32)
    one = np.zeros((S, S), np.float32)
    border = np.argwhere(np.diff(img, axis=1) != 0)
    y, x = border[len(border) // 2] if len(border) else (S // 2, S // 2)
    one[y, x] = 1.0
    grads = np.stack([g, np.abs(g) + 0.1, -np.abs(g) - 0.1, one, np.zeros_like(g)])
    return vw, ndc, faces, F2, light, zero, grads


def _save(vw, faces2, cam, light, S, width=1.0):
    """avc_rasterize_mesh_save on its own fresh 0xFF scratch; outputs pre-filled with garbage -> (image, ndc, fidx, scratch)"""
    from avatarclip_amd import lib as L
    from avatarclip_amd.mesh_render import NEAR, FAR
    lib = L.load()
    N, V = vw.shape[:2]
    F2n = faces2.shape[0] if faces2 is not None else 0
    img = torch.full((N, S, S), float("nan"), device="cuda")
    ndc = torch.full((N, V, 3), float("nan"), device="cuda")
    fidx = torch.full((N, 2 * S, 2 * S), 7, dtype=torch.int32, device="cuda")
    scratch = torch.full((N * lib.avc_rasterize_scratch_bytes(F2n, 2 * S),), 255, dtype=torch.uint8, device="cuda")
    rc = lib.avc_rasterize_mesh_save(L.ptr(vw), N, V, L.ptr(faces2), F2n, L.ptr(cam), width, L.ptr(light), S, NEAR, FAR, L.ptr(ndc), L.ptr(img),
                                     L.ptr(fidx), L.ptr(scratch), L.stream())
    L.check(rc, "avc_rasterize_mesh_save")
    return img, ndc, fidx, scratch


def _scratch_is_empty(scratch, N, F2n, S):
    """the z-buffers all 0xFF and every render's large-face count 0xFFFFFFFF: what the next call assumes"""
    z = scratch.cpu().numpy()
    nz = N * (2 * S) ** 2 * 8
    counts = z[nz:].view(np.uint32)[::F2n + 2]
    return bool((z[:nz] == 255).all()) and len(counts) == N and bool((counts == 0xFFFFFFFF).all())


@gpu
@pytest.mark.parametrize("S", [32, 100])
@pytest.mark.parametrize("case", sorted(SYNTH))
def test_backward_matches_the_restatement_on_adversarial_meshes(case, S):
    from avatarclip_amd import mesh_render as M
    vw, ndc_expect, faces, F2, light, zero, grads = synthetic_case(case, S)
    N, V, n = len(grads), len(vw), 2 * S
    faces2, _, vf_ptr, vf_ent = M._topology(faces, V, "cuda")
    assert np.array_equal(faces2.cpu().numpy(), F2)
    cam = torch.from_numpy(np.tile(IDENT_CAM, (N, 1))).cuda()
    lt = torch.from_numpy(np.tile(light, (N, 1))).cuda()
    img, ndc, fidx, scratch = _save(torch.from_numpy(np.tile(vw, (N, 1, 1))).cuda(), faces2, cam, lt, S)
    assert _scratch_is_empty(scratch, N, len(F2), S)
    nd, fi, im = ndc[0].cpu().numpy(), fidx[0].cpu().numpy(), img[0].cpu().numpy()
    assert np.array_equal(nd, ndc_expect)                                   # the vertices sit where the case put them (pixel centres exact)
    assert all(torch.equal(ndc[i], ndc[0]) and torch.equal(fidx[i], fidx[0]) and torch.equal(img[i], img[0]) for i in range(N))
    assert np.array_equal(fi, R.rasterize_index(nd, F2, n)), np.argwhere(fi != R.rasterize_index(nd, F2, n))[:5]
    assert np.array_equal(R.pooled_image(fi, light), im)
    g = torch.from_numpy(grads).cuda()
    worst = {}
    for eps, pats in ((1e-4, range(N)), (1e-3, [0])):
        outs = [_kernel_grad(g, ndc, fidx, lt, faces2, vf_ptr, vf_ent, S, eps) for _ in range(2)]
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        gn, gl = outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()
        for i in pats:
            worst["eps %g pattern %d" % (eps, i)] = _compare(gn[i], gl[i], nd, F2, light, fi, grads[i], eps, "%s eps %g pattern %d" % (case, eps, i),
                                                             zero, nonzero=i < 3)
    print(case, "S =", S, "worst |kernel - restatement| / sum|term|: %.2e" % max(worst.values()), "bound %.0e" % ABS_K)


@gpu
def test_face_index_map_matches_the_restatement_at_production_size():
    """the saved face-index map bit for bit against the fp32 forward restatement (same arithmetic, ties to the lower face) at S = 256: five
    cameras incl. the close-up CAMS[4] (faces for the tile pass) and BEHIND (vertices behind the camera, faces off the image)"""
    from avatarclip_amd.mesh_render import render_grey_batch
    V, Fc = _template()
    cams = CAMS + [BEHIND]
    eyes, dirs = _dirs(cams)
    vw = torch.from_numpy(V).cuda()[None].expand(len(cams), -1, -1).contiguous()
    with torch.no_grad():
        img, ndc, fidx = render_grey_batch(vw, Fc, eyes, dirs, image_size=256, return_state=True)
    F2 = np.concatenate([Fc, Fc[:, ::-1]])
    for i in range(len(cams)):
        fi, ref = fidx[i].cpu().numpy(), R.rasterize_index(ndc[i].cpu().numpy(), F2, 512)
        assert np.array_equal(fi, ref), (i, (fi != ref).sum(), np.argwhere(fi != ref)[:5])
        assert (fi >= 0).mean() > 0.05


@gpu
def test_backward_matches_the_restatement_at_production_size():
    """image_size = 256 (n = 512: up to 8 passes of the 64-lane run loop) with the ordinary, the close-up and the behind-the-camera view"""
    V, Fc = _template()
    _check_backward(V, Fc, [CAMS[0], CAMS[4], BEHIND], 256, 2)


def _template_batch(N, seed):
    """the template with a per-render offset and small displacements, [N,V,3]"""
    V, Fc = _template()
    rs = np.random.RandomState(seed)
    off = rs.uniform(-0.05, 0.05, (N, 1, 3))
    return (V[None] + off + 0.003 * rs.randn(N, *V.shape)).astype(np.float32), Fc


@gpu
def test_batched_renders_equal_single_renders():
    """N = 6 different vertex sets and cameras in one call: images, ndc, face index, grad_ndc and grad_light bit-identical to six N = 1 calls"""
    from avatarclip_amd import mesh_render as M
    S = 100
    vws, Fc = _template_batch(6, 4)
    cams = CAMS + [BEHIND]
    eyes, dirs = _dirs(cams)
    vw = torch.from_numpy(vws).cuda()
    faces2, f, vf_ptr, vf_ent = M._topology(Fc, vws.shape[1], "cuda")
    with torch.no_grad():
        img_w, ndc_w, fidx_w = M.render_grey_batch(vw, Fc, eyes, dirs, image_size=S, return_state=True)
    v = vw @ torch.tensor(M.ROT_MAT, device="cuda")
    light2 = torch.stack([M.face_light(v[i], f) for i in range(6)]).contiguous()
    cam = torch.from_numpy(np.stack([M.camera_frame(e, d) for e, d in zip(eyes, dirs)])).cuda()
    width = float(np.tan(np.deg2rad(M.VIEWING_ANGLE)))
    img, ndc, fidx, scratch = _save(v.contiguous(), faces2, cam, light2, S, width)
    assert _scratch_is_empty(scratch, 6, faces2.shape[0], S)
    assert torch.equal(img, img_w) and torch.equal(ndc, ndc_w) and torch.equal(fidx, fidx_w)         # the wrapper makes the same call
    g = torch.randn(6, S, S, generator=torch.Generator().manual_seed(5)).cuda()
    gn, gl = _kernel_grad(g, ndc, fidx, light2, faces2, vf_ptr, vf_ent, S)
    for i in range(6):
        im1, nd1, fi1, _ = _save(v[i:i + 1].contiguous(), faces2, cam[i:i + 1].contiguous(), light2[i:i + 1].contiguous(), S, width)
        gn1, gl1 = _kernel_grad(g[i:i + 1].contiguous(), nd1, fi1, light2[i:i + 1].contiguous(), faces2, vf_ptr, vf_ent, S)
        assert torch.equal(im1[0], img[i]) and torch.equal(nd1[0], ndc[i]) and torch.equal(fi1[0], fidx[i]), i
        assert torch.equal(gn1[0], gn[i]) and torch.equal(gl1[0], gl[i]), i
        assert gn1.abs().max() > 0 and (fi1 >= 0).any()
    assert not torch.equal(fidx[0], fidx[1]) and not torch.equal(ndc[0], ndc[1])


@gpu
def test_animate_expand_path_sums_the_per_render_gradients():
    """AnimateContext._render_hip_grad: 5 angles x bs = 2 bodies in one call (render_grey_batch repeats the bodies, one copy per camera); the
    vertices' gradient is the sum of the gradients of the ten renders made one by one"""
    from types import SimpleNamespace
    from avatarclip_amd import animate as A
    from avatarclip_amd.mesh_render import render_grey_batch
    from avatarclip_amd.shapegen_render import get_points_from_angles
    S, bs = 64, 2
    vws, Fc = _template_batch(bs, 6)
    verts = torch.from_numpy(vws).cuda().requires_grad_(True)
    np.random.seed(11)
    out = A.AnimateContext._render_hip_grad(SimpleNamespace(image_size=S), verts, Fc, A.DEFAULT_ANGLES)
    assert out.shape == (len(A.DEFAULT_ANGLES) * bs, 3, S, S)
    g = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).cuda()
    out.backward(g)
    np.random.seed(11)
    eyes = [get_points_from_angles(A.CAMERA_DISTANCE, np.random.randn() * 0.3, a) for a in A.DEFAULT_ANGLES]
    ref = torch.zeros_like(verts)
    for j, e in enumerate(eyes):
        for i in range(bs):
            vi = verts.detach()[i:i + 1].clone().requires_grad_(True)
            img = render_grey_batch(vi, Fc, [e.astype(np.float32)], [(-e / np.linalg.norm(e)).astype(np.float32)], image_size=S)
            assert torch.equal(img[0], out[j * bs + i, 0].detach())
            img.backward(g[j * bs + i].sum(0, keepdim=True))
            ref[i] += vi.grad[0]
    assert verts.grad.abs().max() > 0
    assert torch.allclose(verts.grad, ref, rtol=1e-6, atol=1e-6 * float(ref.abs().max())), (verts.grad - ref).abs().max()


@gpu
def test_scratch_is_left_empty_and_layout_changes_do_not_leak():
    """every call leaves the cached scratch's z-buffers and large-face counts empty; layouts A -> B -> A, and A again after a call the entry
    point rejects (N = 0), all give what the first call gave, bit for bit"""
    from avatarclip_amd import lib as L
    from avatarclip_amd import mesh_render as M
    from avatarclip_amd import smpl_prior as SP
    vws, Fc = _template_batch(3, 8)
    F2n = 2 * len(Fc)

    def run(N, S, cams):
        eyes, dirs = _dirs(cams)
        vw = torch.from_numpy(vws[:N]).cuda().requires_grad_(True)
        img, ndc, fidx = M.render_grey_batch(vw, Fc, eyes, dirs, image_size=S, return_state=True)
        img.backward(torch.randn(img.shape, generator=torch.Generator().manual_seed(N)).cuda())
        need = N * L.load().avc_rasterize_scratch_bytes(F2n, 2 * S)
        key = (str(vw.device), L.stream(), (N, F2n, S), need)
        assert key in SP._scratch
        assert _scratch_is_empty(SP._scratch_for(vw.device, (N, F2n, S), need), N, F2n, S)
        return [t.detach().clone() for t in (img, ndc, fidx, vw.grad)]

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    A1 = run(2, 64, [CAMS[4], BEHIND])            # (close-up, behind the camera: large-face lists in use)
    B1 = run(3, 32, CAMS[:3])
    assert same(run(2, 64, [CAMS[4], BEHIND]), A1)
    assert same(run(3, 32, CAMS[:3]), B1)
    faces2, _, vf_ptr, vf_ent = M._topology(Fc, vws.shape[1], "cuda")
    empty = torch.zeros(0, vws.shape[1], 3, device="cuda")
    with pytest.raises(RuntimeError, match="bad sizes"):
        M._RasterFn.apply(empty, torch.zeros(0, F2n, device="cuda"), torch.zeros(0, 12, device="cuda"), faces2, vf_ptr, vf_ent, 64, 0.5, 1e-4)
    assert same(run(2, 64, [CAMS[4], BEHIND]), A1)


@gpu
def test_no_faces_at_the_c_abi():
    """F = 0: the forward gives an empty image and face index, the backward a zero gradient, both return 0"""
    from avatarclip_amd import lib as L
    N, V, S = 2, 5, 16
    vw = torch.from_numpy(np.random.RandomState(0).uniform(-1, 1, (N, V, 3)).astype(np.float32) + np.float32([0, 0, 3])).cuda()
    cam = torch.from_numpy(np.tile(IDENT_CAM, (N, 1))).cuda()
    img, ndc, fidx, scratch = _save(vw, None, cam, None, S)
    assert (img == 0).all() and (fidx == -1).all() and torch.isfinite(ndc).all()
    assert _scratch_is_empty(scratch, N, 0, S)
    g = torch.randn(N, S, S).cuda()
    gn = torch.full((N, V, 3), float("nan"), device="cuda")
    vf_ptr = torch.zeros(V + 1, dtype=torch.int32, device="cuda")
    assert L.load().avc_rasterize_mesh_grad(L.ptr(g), L.ptr(ndc), N, V, None, 0, None, L.ptr(fidx), S, 1e-4, L.ptr(vf_ptr), None, None, L.ptr(gn),
                                            None, L.stream()) == 0
    torch.cuda.synchronize()
    assert (gn == 0).all()


def _single(vw, faces2, light, S, flip_x, channels):
    """avc_rasterize_mesh (IDENT_CAM, width 1) on its own fresh 0xFF scratch; outputs pre-filled with NaN -> (rc, out, ndc, scratch)"""
    from avatarclip_amd import lib as L
    from avatarclip_amd.mesh_render import NEAR, FAR
    lib = L.load()
    F2n = faces2.shape[0] if faces2 is not None else 0
    out = torch.full((S, S, 3) if channels == 3 else (S, S), float("nan"), device="cuda")
    ndc = torch.full((vw.shape[0], 3), float("nan"), device="cuda")
    scratch = torch.full((lib.avc_rasterize_scratch_bytes(F2n, 2 * S),), 255, dtype=torch.uint8, device="cuda")
    rc = lib.avc_rasterize_mesh(L.ptr(vw), vw.shape[0], L.ptr(faces2), F2n, L.ptr(torch.from_numpy(IDENT_CAM).cuda()), 1.0, L.ptr(light), S, NEAR, FAR,
                                L.ptr(ndc), L.ptr(out), flip_x, channels, L.ptr(scratch), L.stream())
    return rc, out, ndc, scratch


def _face_list(faces9, light, n):
    """avc_rasterize_faces at n x n on its own fresh 0xFF scratch; the image pre-filled with NaN -> (rc, image, scratch)"""
    from avatarclip_amd import lib as L
    from avatarclip_amd.mesh_render import NEAR, FAR
    lib = L.load()
    Fn = faces9.shape[0] if faces9 is not None else 0
    image = torch.full((n, n), float("nan"), device="cuda")
    scratch = torch.full((lib.avc_rasterize_scratch_bytes(Fn, n),), 255, dtype=torch.uint8, device="cuda")
    rc = lib.avc_rasterize_faces(L.ptr(faces9), L.ptr(light), Fn, n, NEAR, FAR, L.ptr(image), L.ptr(scratch), L.stream())
    return rc, image, scratch


@gpu
@pytest.mark.parametrize("case", sorted(SYNTH))
def test_single_render_and_face_list_forms_match_the_restatement(case):
    """avc_rasterize_mesh and avc_rasterize_faces bit for bit against the fp32 restatement on the adversarial meshes (the save form is pinned
    by test_backward_matches_the_restatement_on_adversarial_meshes): ndc, the pooled image plain and x-flipped with three channels, the
    un-pooled face-list image, and the scratch each call leaves"""
    S = 32
    n = 2 * S
    vw, ndc_expect, faces, F2, light, _, _ = synthetic_case(case, S)
    fi = R.rasterize_index(ndc_expect, F2, n)
    pooled = R.pooled_image(fi, light)
    faces2, lt = torch.from_numpy(F2.astype(np.int32)).cuda(), torch.from_numpy(light).cuda()
    for flip_x, channels in ((0, 1), (1, 3)):
        rc, out, ndc, scratch = _single(torch.from_numpy(vw).cuda(), faces2, lt, S, flip_x, channels)
        assert rc == 0
        assert np.array_equal(ndc.cpu().numpy(), ndc_expect)
        out = out.cpu().numpy()
        if channels == 3:
            assert out.shape == (S, S, 3) and all(np.array_equal(out[..., c], pooled[:, ::-1]) for c in range(3))
        else:
            assert np.array_equal(out, pooled), np.argwhere(out != pooled)[:5]
        assert _scratch_is_empty(scratch, 1, len(F2), S)
    rc, image, scratch = _face_list(torch.from_numpy(np.ascontiguousarray(ndc_expect[F2].reshape(-1, 9))).cuda(), lt, n)
    assert rc == 0
    expect = np.where(fi >= 0, light[np.maximum(fi, 0)], np.float32(0))[::-1]
    assert np.array_equal(image.cpu().numpy(), expect), np.argwhere(image.cpu().numpy() != expect)[:5]
    assert _scratch_is_empty(scratch, 1, len(F2), S)


@gpu
def test_no_faces_in_the_single_render_and_face_list_forms():
    """F = 0: both forms return 0, give an all-zero image and leave the scratch empty"""
    S = 32
    vw = torch.from_numpy(np.random.RandomState(0).uniform(-1, 1, (5, 3)).astype(np.float32) + np.float32([0, 0, 3])).cuda()
    for flip_x, channels in ((0, 1), (1, 3)):
        rc, out, ndc, scratch = _single(vw, None, None, S, flip_x, channels)
        assert rc == 0 and (out == 0).all() and torch.isfinite(ndc).all()
        assert _scratch_is_empty(scratch, 1, 0, S)
    rc, image, scratch = _face_list(None, None, 2 * S)
    assert rc == 0 and (image == 0).all()
    assert _scratch_is_empty(scratch, 1, 0, S)


@gpu
def test_render_hip_equals_one_prior_render_per_camera_and_body():
    """AnimateContext._render_hip (one no-gradient batched call) against the statement it replaces: the same elevation draws, then every
    (camera, body) rendered by its own MeshPrior, camera-major -- bit for bit"""
    from avatarclip_amd import animate as A
    from avatarclip_amd.shapegen_render import get_points_from_angles
    from avatarclip_amd.smpl_prior import MeshPrior
    S, bs, angles = 32, 2, A.DEFAULT_ANGLES[:3]
    vws, Fc = _template_batch(bs, 9)
    verts = torch.from_numpy(vws).cuda()
    ctx = A.AnimateContext(None, None, None, None, device="cuda", image_size=S)
    np.random.seed(13)
    out = ctx.render_fn(verts, Fc, angles)
    assert ctx.render_fn.__name__ == "_render_hip" and out.shape == (len(angles) * bs, 3, S, S) and not out.requires_grad
    np.random.seed(13)
    eyes = [get_points_from_angles(A.CAMERA_DISTANCE, np.random.randn() * 0.3, a) for a in angles]
    priors = [MeshPrior(v, Fc, device="cuda", image_size=S) for v in vws]
    for j, eye in enumerate(eyes):
        for i, p in enumerate(priors):
            g = p.render_grey(eye.astype(np.float32), (-eye / np.linalg.norm(eye)).astype(np.float32))
            assert (g > 0).any()
            assert torch.equal(out[j * bs + i], g.unsqueeze(0).expand(3, -1, -1)), (j, i)
