"""The rasteriser's batched forward with save and neural_renderer's approximate backward on the MI355X (csrc/avc_raster_grad.hip behind
avatarclip_amd.mesh_render): images bit-identical to MeshPrior's, the backward against the fp32 restatement (tests/nr_grad_restatement.py),
determinism, and the paper's silhouette-fitting experiment."""
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


def _check_backward(V, Fc, cams, S, seed):
    from avatarclip_amd.mesh_render import render_grey_batch
    eyes, dirs = _dirs(cams)
    vw = torch.from_numpy(V).cuda()[None].repeat(len(cams), 1, 1).requires_grad_(True)
    img, ndc, fidx = render_grey_batch(vw, Fc, eyes, dirs, image_size=S, return_state=True)
    g = torch.randn(img.shape, generator=torch.Generator().manual_seed(seed)).cuda()
    F2 = np.concatenate([Fc, Fc[:, ::-1]])
    from avatarclip_amd import lib as L
    from avatarclip_amd import mesh_render as M
    # the kernel's own outputs (grad_ndc, grad_light) for the comparison: the same call the autograd Function makes
    faces2, f, vf_ptr, vf_ent = M._topology(Fc, V.shape[0], vw.device)
    v = vw.detach() @ torch.tensor(M.ROT_MAT, device="cuda")
    light2 = torch.stack([M.face_light(v[i], f) for i in range(len(cams))]).contiguous()
    N, F2n = len(cams), F2.shape[0]
    outs = []
    for _ in range(2):
        fg = torch.empty(N, F2n, 6, device="cuda"); gn = torch.empty(N, V.shape[0], 3, device="cuda"); gl = torch.empty(N, F2n, device="cuda")
        L.check(L.load().avc_rasterize_mesh_grad(L.ptr(g), L.ptr(ndc), N, V.shape[0], L.ptr(faces2), F2n, L.ptr(light2), L.ptr(fidx), S, 1e-4,
                                                 L.ptr(vf_ptr), L.ptr(vf_ent), L.ptr(fg), L.ptr(gn), L.ptr(gl), L.stream()), "grad")
        outs.append((gn, gl))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])       # deterministic: two calls bit-identical
    gn, gl = outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()
    for i in range(N):
        rg, rl = R.backward(ndc[i].cpu().numpy(), F2, light2[i].cpu().numpy(), fidx[i].cpu().numpy(), g[i].cpu().numpy())
        assert np.array_equal(gn[i] != 0, rg != 0), (i, (gn[i] != 0).sum(), (rg != 0).sum())
        tol = 1e-4 * np.abs(rg).max() + 1e-6
        assert np.abs(gn[i] - rg).max() <= tol, (i, np.abs(gn[i] - rg).max(), tol)
        assert np.array_equal(gl[i] != 0, rl != 0)
        assert np.abs(gl[i] - rl).max() <= 1e-5 * max(np.abs(rl).max(), 1e-30) + 1e-7
        assert (rg[:, 2] == 0).all() and np.abs(rg).max() > 0
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
