"""Seeded nets and backward inputs shared by the engine-level GPU tests (tests/test_gpu_kernels.py), and the torch statements those
tests hold the engine's single-launch forms against."""
import torch


def pack_statement(dl, flatP):
    """(w_f16, w_bf16, tab) of engine.Packed as torch gathers: the statement avc_pack_params is held to, bit for bit"""
    pz = torch.cat([flatP.detach().float(), flatP.new_zeros(1)])
    w = pz[dl.idx16] * dl.scale16
    return w.to(torch.float16).contiguous(), w.to(torch.bfloat16).contiguous(), (pz[dl.idx32] * dl.scale32).contiguous()


def points_bwd_statement(eng, pk, rays_o, rays_d, z, sample_dist, d_sdf, d_n, d_rgb, rgb, panels_valid=False):
    """Engine.points_bwd with the tail in torch: the product's slab walk (same launches, same partial products), then per slab two
    reductions + two adds, and at the end gather, scale and index_adds -- what avc_weight_grad_reduce / _unpack are held to"""
    lay, dl = eng.dl.lay, eng.dl
    gout = torch.zeros(lay.gout_size, device=eng.device, dtype=torch.float32)
    gbias = torch.zeros(lay.gbias_size, device=eng.device, dtype=torch.float32)
    cs_total = None
    for ns, cs_total in eng.slab_walk(pk, rays_o, rays_d, z, sample_dist, d_sdf, d_n, d_rgb, rgb, panels_valid):
        gout += eng._partials[:ns].sum(0)
        gbias += eng._bpartials[:ns].sum(0)
    grad = torch.zeros(lay.nparam, device=eng.device, dtype=torch.float32)
    grad.index_add_(0, dl.un_tgt, gout[dl.un_src] * dl.un_scale)
    grad.index_add_(0, dl.ub_tgt, gbias[dl.ub_src])
    if cs_total is not None:
        grad.index_add_(0, dl.cs_tgt, cs_total[dl.cs_src] * dl.cs_scale)
    if eng.SDF_BIAS_FP32:
        grad[eng._sdf_bias0] = d_sdf.sum()
    return grad


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
