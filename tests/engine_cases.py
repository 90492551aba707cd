"""Seeded nets and backward inputs shared by the engine-level GPU tests (tests/test_gpu_kernels.py)."""
import torch


def _nets(small, dev, seed=0):
    from avatarclip_amd import fields, renderer
    torch.manual_seed(seed)
    if small:
        sdf = fields.SDFNetwork(d_out=129, d_in=3, d_hidden=128, n_layers=3, skip_in=[3], multires=6)
        col = fields.RenderingNetwork(d_feature=128, mode="no_view_dir", d_in=6, d_out=3, d_hidden=128, n_layers=1, extra_color=True)
    else:
        sdf = fields.SDFNetwork(d_out=257, d_in=3, d_hidden=256, n_layers=4, skip_in=[4], multires=6)
        col = fields.RenderingNetwork(d_feature=256, mode="no_view_dir", d_in=6, d_out=3, d_hidden=256, n_layers=2, extra_color=True)
    var = fields.SingleVarianceNetwork(0.3)
    sdf, col, var = sdf.to(dev), col.to(dev), var.to(dev)
    return renderer.NeuSRenderer(None, sdf, var, col, 32, 32, 0, 4, 1.0, True)


def _inputs(R, S, dev, seed=1):
    g = torch.Generator(device="cpu").manual_seed(seed)
    ro = (torch.randn(R, 3, generator=g) * 0.1).to(dev)
    rd = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1).to(dev)
    z = torch.sort(torch.rand(R, S, generator=g) * 2, dim=-1)[0].contiguous().to(dev)
    dsdf = torch.randn(R, S, generator=g).to(dev)
    dn = (torch.randn(R, S, 3, generator=g) * 0.1).to(dev)
    drgb = (torch.randn(R, S, 6, generator=g) * 0.1).to(dev)
    return ro, rd, z, dsdf, dn, drgb
