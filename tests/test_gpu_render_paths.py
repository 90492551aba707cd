"""ShapeGen's two renders and `apply_rot_mat=False` on the one batched host path of avatarclip_amd.mesh_render, on the MI355X: each against
the statement it replaced, bit for bit.  The 40-vertex / 60-face random mesh of tests/test_gpu_raster_grad.py at S = 32, two cameras."""
import numpy as np
import pytest
import torch

from tests.test_gpu_raster_grad import _random_mesh

gpu = pytest.mark.gpu
S = 32
ANGLES = (150, 30)


def _mesh():
    v, f = _random_mesh(np.random.RandomState(3))
    assert (v != 0).all()           # a signed permutation of non-zero coordinates is exact both ways (no sign of a zero to lose)
    return v, f


@gpu
def test_render_body_equals_one_prior_render_per_angle():
    """shapegen.render_body was a loop over MeshPrior(apply_rot_mat=False).render_grey; it is one render_grey_batch now"""
    from avatarclip_amd import shapegen as SG
    from avatarclip_amd.shapegen_render import get_points_from_angles
    from avatarclip_amd.smpl_prior import MeshPrior
    v, f = _mesh()
    out = SG.render_body(v, f, image_size=S, angles=ANGLES)
    prior = MeshPrior(v, f, image_size=S, apply_rot_mat=False)
    want = []
    for a in ANGLES:
        eye = get_points_from_angles(2.0, 0.0, a)
        want.append(prior.render_grey(eye, -eye / np.linalg.norm(eye))[None].repeat(3, 1, 1))
    want = torch.stack(want)
    assert out.shape == (len(ANGLES), 3, S, S) and out.dtype == torch.float32 and out.is_cuda and not out.requires_grad
    assert torch.equal(out, want), (out - want).abs().max()
    assert 0 <= float(out.min()) and float(out.max()) <= 1 and float((out > 0).float().mean()) > 0.05


@gpu
def test_textured_render_fn_equals_the_render_that_undid_rot_mat_first():
    """shapegen.textured_render_fn multiplied the vertices by ROT_MAT transposed for render_rgb_batch to multiply it back in; it passes
    apply_rot_mat=False now"""
    from avatarclip_amd import shapegen as SG
    from avatarclip_amd.mesh_render import ROT_MAT, render_rgb_batch
    from avatarclip_amd.shapegen_render import get_points_from_angles
    v, f = _mesh()
    cubes = torch.rand(len(f), 4, 4, 4, 3, generator=torch.Generator().manual_seed(7)).cuda()
    out = SG.textured_render_fn(f, cubes, image_size=S, angles=ANGLES)(v)
    eyes = [get_points_from_angles(2.0, 0.0, a).astype(np.float32) for a in ANGLES]
    dirs = [(-e / np.linalg.norm(e)).astype(np.float32) for e in eyes]
    vt = torch.from_numpy(v).cuda()
    with torch.no_grad():
        want = render_rgb_batch((vt @ torch.tensor(ROT_MAT, device="cuda").t())[None], f, cubes, eyes, dirs, image_size=S)
    assert out.shape == (len(ANGLES), 3, S, S) and out.dtype == torch.float32 and out.is_cuda and not out.requires_grad
    assert torch.equal(out, want), (out - want).abs().max()
    assert float(out.std()) > 0.05 and 0 <= float(out.min()) and float(out.max()) <= 1


@gpu
def test_apply_rot_mat_false_projects_what_rot_mat_applied_beforehand_projects():
    from avatarclip_amd.mesh_render import ROT_MAT, render_grey_batch
    from avatarclip_amd.shapegen import look_at_cameras
    v, f = _mesh()
    eyes, dirs = look_at_cameras(2.0, 0.0, ANGLES)
    vt = torch.from_numpy(v).cuda()[None]
    img, ndc, fidx = render_grey_batch(vt, f, eyes, dirs, image_size=S, return_state=True, apply_rot_mat=False)
    img_r, ndc_r, fidx_r = render_grey_batch(vt @ torch.tensor(ROT_MAT, device="cuda").t(), f, eyes, dirs, image_size=S, return_state=True)
    assert torch.equal(ndc, ndc_r) and torch.equal(fidx, fidx_r) and torch.equal(img, img_r)
    assert torch.isfinite(ndc).all() and int((fidx >= 0).sum()) > 0
