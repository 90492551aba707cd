"""tests/glue_restatement.py on the CPU (no GPU): the float64 restatement of the glue kernels is pinned against the nine cases of
tests/golden/glue.npz (the reference's own lines, executed), against the product's torch statements -- Runner.shade_and_scatter /
assemble_loss, chess_background, Dataset's ray generation and near_far_from_sphere, coarse_z_torch, clip_vit.clip_preprocess
(F.interpolate) -- and torch.cosine_similarity on the non-degenerate families; the figures the GPU module's tolerances are 4 x of
(`GR.*_F32_ERR`) are measured here, float32 CPU statement against float64 restatement, and kept honest; and each wrong kernel of the
list below, written as ONE overridden decision of `GR.Statement`, is rejected by the criteria of tests/test_gpu_glue_exact.py on a
named case -- or shown to be no wrong kernel (profiles/glue_exact.md has the table)."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import glue_restatement as GR

F32, F64 = torch.float32, torch.float64
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "glue.npz")
GOLD_CASES = ["full_black", "full_white", "full_gauss", "full_chess", "sil_black", "sil_white", "sil_gauss", "sil_chess", "plain"]


def _honest(measured, stored, floor=0.0):
    """a stored figure covers what is measured here and is not slack: measured <= stored <= 2 x measured + floor"""
    return measured <= stored <= 2.0 * measured + floor


def test_constants_are_the_products():
    from avatarclip_amd import clip_vit
    assert GR.CLIP_HI == np.float32(1.0) - np.float32(1e-3) and GR.CLIP_LO == np.float32(1e-3)      # torch's double 0.999 -> float and the kernel's 1.f - 1e-3f
    assert tuple(clip_vit.CLIP_MEAN) == GR.CLIP_MEAN and tuple(clip_vit.CLIP_STD) == GR.CLIP_STD and clip_vit.RES == GR.RES
    from avatarclip_amd import glue
    assert torch.equal(torch.from_numpy(glue.unit_light([0.3, -0.5, 0.8], 0.13)), GR.unit_light32([0.3, -0.5, 0.8], 0.13))


# ------------------------------------------------------------------------------------------------------------------------
# shading, scatter, loss terms
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLD_CASES)
def test_shading_restatement_matches_the_reference_lines(case):
    z = np.load(GOLD)
    d = {k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + "/")}
    H, W, S, R, sil, choice = [int(v) for v in d["meta"][:6]]
    add_no_texture, cast = bool(d["flags"][0]), bool(d["flags"][1])
    T = lambda k: torch.from_numpy(d[k])
    P = H * W
    rop = None
    if sil:
        idx = T("in_dilated_mask").reshape(-1).nonzero().squeeze(1)
        rop = torch.full((P,), -1, dtype=torch.int32)
        rop[idx] = torch.arange(idx.numel(), dtype=torch.int32)
    c = dict(family="golden", P=P, R=R, color=T("in_color_fine"), extra=T("in_extra_color_fine"), wsum=T("in_weight_sum").reshape(-1),
             nsum=(T("in_gradients") * T("in_weights")[:, :, None]).sum(1), true_rgb=T("in_true_rgb"), mask=T("mask").reshape(-1), ray_of_pixel=rop,
             bg=T("background_rgb").reshape(-1) if "background_rgb" in d else torch.zeros(P),
             light=GR.unit_light32(d["light_dir"], float(d["ambience"])))
    bg_mode = "image" if (sil and choice in (1, 2)) else ("const1" if choice == 0 else "const0")
    shading = add_no_texture or cast
    out = GR.shade_loss(c, nsum=shading, img0_is_extra=not cast, bg_mode=bg_mode)
    if cast:
        assert np.abs(out["images"][0].numpy() - d["texture_shading"]).max() < 1e-6
    else:
        assert np.abs(out["images"][0].numpy() - d["extra_color_fine"]).max() < 1e-6
    if shading:
        assert np.abs(out["images"][1].numpy() - d["rand_shading_rgb"]).max() < 1e-6
    s = out["sums"]
    for name, val in (("color_fine_loss", s[0] / (s[1] + 1e-5)), ("mask_loss", s[2] / P)):
        assert abs(float(val) - float(d[name])) < 1e-5 * max(1.0, abs(float(d[name]))), (name, float(val), float(d[name]))


def _runner_stub(sil, enc_w, text):
    from avatarclip_amd import clip_vit
    w = GR.TAIL_W
    return types.SimpleNamespace(device=torch.device("cpu"), add_no_texture=True, texture_cast_light=True, use_silhouettes=sil,
                                 _weighted_normals=lambda ro: ro["nsum"], _shard_group=None, _loss_mask=lambda m: m, writer=None,
                                 _prompt_for=lambda i, v: text, clip_preprocess=clip_vit.clip_preprocess, igr_weight=w["igr"],
                                 mask_weight=w["mask"], clip_weight=w["clip"],
                                 perceptor=types.SimpleNamespace(encode_image=lambda x: x.reshape(x.shape[0], -1) @ enc_w.to(x.dtype)))


@pytest.mark.parametrize("rop", [False, True])
@pytest.mark.parametrize("bg_mode,choice", [("const1", 0), ("image", 1), ("const0", 3)])
def test_restatement_chain_equals_runner_glue(rop, bg_mode, choice):
    """shade_loss -> resize_norm -> (a fixed linear encoder) -> loss_tail in float64 against Runner.shade_and_scatter + assemble_loss
    in float32 on the same inputs (general family, a 15 x 13 image): images, loss and its parts, and the gradients"""
    from avatarclip_amd.runner import Runner
    H, W = 15, 13
    c = GR.shade_case("general", H * W, rop)
    g = torch.Generator().manual_seed(5)
    enc_w = torch.randn(3 * 224 * 224, 512, generator=g, dtype=F64) / 400.0
    text = F.normalize(torch.randn(2, 512, generator=g), dim=-1)
    owned = torch.ones(H * W, dtype=torch.bool) if not rop else c["ray_of_pixel"] >= 0
    sel_idx = None if not rop else torch.argsort(torch.where(owned, c["ray_of_pixel"].long(), 2 ** 30))[:c["R"]]
    view = types.SimpleNamespace(H=H, W=W, true_rgb=c["true_rgb"], mask=c["mask"][:, None], dilated_mask=owned.reshape(H, W), sel_idx=sel_idx)
    leaf = {k: c[k].clone().requires_grad_(True) for k in ("color", "extra", "wsum", "nsum")}
    ro = dict(color_fine=leaf["color"], extra_color_fine=leaf["extra"], weight_sum=leaf["wsum"][:, None], nsum=leaf["nsum"],
              gradient_error=torch.tensor(0.0371), s_val=torch.ones(1, 1))
    stub = _runner_stub(rop, enc_w, text)
    comp = Runner.shade_and_scatter(stub, ro, view, choice, c["bg"][:, None], light=(c["light"][:3].numpy(), float(c["light"][3])))
    loss, parts = Runner.assemble_loss(stub, ro, comp, view, 1)
    loss.backward()
    # the restatement
    l64 = {k: c[k].double().requires_grad_(True) for k in leaf}
    out = GR.shade_loss(c, bg_mode=bg_mode if rop else "image", leaves=l64)
    assert (out["images"][0].detach() - comp["texture_shading"].detach()).abs().max() < 1e-6
    assert (out["images"][1].detach() - comp["rand_shading_rgb"].detach()).abs().max() < 1e-6
    x = GR.resize_norm(out["images"].reshape(2, H, W, 3))
    enc = x.reshape(2, -1) @ enc_w
    tc = dict(enc=enc, text=text, sums=out["sums"], eik=torch.tensor(0.0371), P=float(H * W))
    w = GR.TAIL_W
    unit = lambda v: v / GR.HONEST.clamp_norm(torch.norm(v, dim=-1, keepdim=True))
    cos = (unit(enc) * unit(text.double().mean(0, keepdim=True))).sum(-1)
    s = out["sums"]
    want = s[0] / (s[1] + 1e-5) + float(np.float32(0.0371)) * w["igr"] + s[2] / (H * W) * w["mask"] + (1 - cos[0]) * w["clip"] + (1 - cos[1]) * w["clip"]
    assert abs(float(want.detach()) - float(loss.detach())) < 1e-5 * abs(float(want))
    assert abs(float(GR.loss_tail(tc)["loss"]) - float(want)) < 1e-12
    for name, val in (("color", s[0] / (s[1] + 1e-5)), ("mask", s[2] / (H * W)), ("cosine", cos[0]), ("cosine_shading", cos[1])):
        assert abs(float(val) - float(parts[name])) < 1e-5, name
    want.backward()
    for k in leaf:
        a, b = leaf[k].grad.double(), l64[k].grad
        assert (a - b).norm() <= 2e-5 * b.norm(), (k, float((a - b).norm() / b.norm()))


def _shade_options():
    """(nsum, img0_is_extra, bg_mode) of the GPU table"""
    return [(True, False, "image"), (True, True, "const0"), (False, False, "const1"), (True, False, "const1")]


def test_float32_statement_error_behind_the_shading_tolerances():
    """what the statement in float32 leaves against float64, over every family, size and option of the GPU table; the criteria accept
    the float32 statement everywhere"""
    worst = dict(images=0.0, sums=0.0, bce_exact=0.0, partial=0.0, dextra=0.0, dwsum=0.0, dnsum=0.0)
    for family in GR.SH_FAMILIES:
        for P in GR.SH_P:
            for rop in (False, True):
                c = GR.shade_case(family, P, rop)
                if family == "general":
                    assert GR.shade_margin(c) >= 1e-4
                for nsum, img0x, bg_mode in _shade_options():
                    ref = GR.shade_loss(c, nsum, img0x, bg_mode)
                    f32 = GR.shade_loss(c, nsum, img0x, bg_mode, dtype=F32)
                    fails, fig = GR.judge_shade_fwd(c, f32["images"], f32["sums"], ref)
                    assert not fails, (family, P, rop, nsum, fails)
                    worst["images"] = max(worst["images"], fig["images"])
                    worst["partial"] = max(worst["partial"], GR.partial_err(GR.block_sums(f32["terms"], P), ref["terms"], P))
                    rel = ((f32["sums"].double() - ref["sums"]).abs() / ref["sums"].abs().clamp_min(1e-30))
                    if family == "exact":
                        worst["bce_exact"] = max(worst["bce_exact"], float(rel[2]))
                    else:
                        worst["sums"] = max(worst["sums"], float(rel.max()))
                if P in GR.SH_P_BWD:
                    for nsum, img0x in ((True, False), (True, True), (False, False)):
                        ref = GR.shade_loss_grads(c, nsum, img0x)
                        f32 = GR.shade_loss_grads(c, nsum, img0x, dtype=F32)
                        fails, fig = GR.judge_shade_bwd(c, f32, ref)
                        assert not fails, (family, P, rop, nsum, fails)
                        for k, v in fig.items():
                            worst[k] = max(worst[k], v)
    print("float32 shading statement vs float64:", {k: "%.3g" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert _honest(v, GR.SH_F32_ERR[k], 6e-8), (k, v, GR.SH_F32_ERR[k])


def test_exact_family_sums_are_exact_in_float32():
    """0 / 1 mask and colour differences in quarters: every partial sum of |e| (units of 1/4), of the mask and of e^2 (units of 1/16)
    is an integer below 2^24 units, so float32 addition in any order is exact -- what lets the GPU module use torch.equal"""
    for P in GR.SH_P:
        for rop in (False, True):
            c = GR.shade_case("exact", P, rop)
            t = GR.shade_loss(c)["terms"]
            assert torch.equal(t[:, 0] * 4, (t[:, 0] * 4).round()) and torch.equal(t[:, 3] * 16, (t[:, 3] * 16).round())
            assert float(t[:, 0].sum() * 4) < 2 ** 24 and float(t[:, 3].sum() * 16) < 2 ** 24 and float(t[:, 1].sum()) < 2 ** 24
            perm = torch.randperm(P, generator=torch.Generator().manual_seed(P))
            assert torch.equal(t.float()[perm][:, [0, 1, 3]].sum(0), t[:, [0, 1, 3]].sum(0).float())
            assert float(t[-1, 0]) > 0 and float(t[-1, 1]) == 1 and float(t[-1, 3]) > 0        # the last pixel counts in every sum


def test_threshold_family_sits_on_every_threshold():
    c = GR.shade_case("threshold", 65537, True)
    ws, N, E = c["wsum"], c["nsum"], c["extra"]
    for v in (0.5, float(GR.CLIP_LO), float(GR.CLIP_HI)):
        assert (ws == np.float32(v)).any()
    bgm = ws < 0.5
    assert ((E == 0).all(-1) & bgm).any() and ((E == 1).all(-1) & bgm).any()          # extra * s' exactly 0 and 1 with s' = 1
    l = c["light"][:3]
    assert torch.equal(l, torch.tensor([1.0, 0.0, 0.0]))
    dot = (N * l).sum(-1)
    body = ~bgm
    assert ((dot == 0) & (N.abs().sum(-1) > 0) & body).any() and ((N[:, 1:] == 0).all(-1) & (N[:, 0] > 0) & body).any()    # perpendicular, parallel
    assert ((N == 0).all(-1) & body).any() and (torch.isnan(N).any(-1) & body).any()
    pix = torch.argsort(torch.where(c["ray_of_pixel"] < 0, 2 ** 30, c["ray_of_pixel"].long()))[:c["R"]]
    assert ((c["color"] == c["true_rgb"][pix]).all(-1) & (c["mask"][pix] == 1)).any()
    g = GR.shade_loss_grads(c)
    assert all(torch.isfinite(v).all() for k, v in g.items())
    zero = (N == 0).all(-1) & body & g["owns"]
    assert (g["dnsum"][zero].abs().sum(-1) > 0).any()                                   # the zero normal has the gradient of n / (|n| + 1e-7) at 0


# ------------------------------------------------------------------------------------------------------------------------
# resize + normalise
# ------------------------------------------------------------------------------------------------------------------------
def _interp32(x):
    """clip_vit.clip_preprocess image by image: the float32 CPU statement (F.interpolate)"""
    from avatarclip_amd.clip_vit import clip_preprocess
    return torch.cat([clip_preprocess(x[i]) for i in range(x.shape[0])], dim=0)


def _resize_f32(H, W, case):
    """fx, f0, bw, b1 of judge_resize from F.interpolate and its autograd in float32"""
    x = case["x"].clone().requires_grad_(True)
    fx = _interp32(x)
    bw = torch.autograd.grad((fx * case["w"]).sum(), x)[0]
    f0 = _interp32(torch.zeros_like(case["x"]))
    x1 = torch.zeros(len(GR.ONEHOT_PIXELS), H, W, 3, requires_grad=True)
    b1 = torch.autograd.grad((_interp32(x1) * GR.onehot_dout()).sum(), x1)[0]
    return fx.detach(), f0, bw, b1


@pytest.mark.parametrize("H,W", GR.RS_SHAPES)
def test_resize_restatement_is_interpolate_and_its_float32_error(H, W):
    """float64 restatement == F.interpolate(bilinear, align_corners=False) + Normalize in float64 (to rounding), its transpose ==
    autograd's; then what F.interpolate in float32 leaves against it: the forward offset grows with the input size through the float32
    source coordinate, so the figure is per shape"""
    worst = dict(fwd=0.0, onehot=0.0, transpose=0.0)
    for B in GR.RS_B:
        case = GR.resize_case(H, W, B)
        x64 = case["x"].double().requires_grad_(True)
        mean, std = (t.view(1, 3, 1, 1) for t in GR._norm(F64))                  # (the float32 mean / std the kernel is handed)
        y64 = x64.permute(0, 3, 1, 2)
        if (H, W) != (224, 224):
            y64 = F.interpolate(y64, size=(224, 224), mode="bilinear", align_corners=False)
        y64 = (y64 - mean) / std
        ref = GR.resize_norm(case["x"])
        # (F.interpolate in float64 takes its tap index from the float64 coordinate; the shapes of the table keep every coordinate
        # 1 / 448 or more away from an integer, so the float32 decision is the same)
        assert (y64.detach() - ref).abs().max() < 1e-12
        g64 = torch.autograd.grad((y64 * case["w"].double()).sum(), x64)[0]
        assert (g64 - GR.resize_norm_bwd(case["w"], H, W)).abs().max() < 1e-10
        for draw in range(6 if B == 1 else 1):
            cs = case if draw == 0 else dict(x=torch.rand(B, H, W, 3, generator=torch.Generator().manual_seed(draw)),
                                             w=torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(100 + draw)))
            fx, f0, bw, b1 = _resize_f32(H, W, cs)
            worst["fwd"] = max(worst["fwd"], float((fx.double() - GR.resize_norm(cs["x"])).abs().max()))
            worst["transpose"] = max(worst["transpose"], GR.transpose_gap(fx, f0, cs["w"], cs["x"], bw))
            worst["onehot"] = max(worst["onehot"], float((b1.double() - GR.resize_norm_bwd(GR.onehot_dout(), H, W)).abs().max()))
            if draw == 0:
                fails, fig = GR.judge_resize(H, W, fx, f0, bw, b1, cs)
                assert not fails, fails
    print("RS_F32_ERR[(%d, %d)] = dict(fwd=%.2g, onehot=%.2g, transpose=%.2g)," % (H, W, worst["fwd"], worst["onehot"], worst["transpose"]))
    for k, v in worst.items():
        assert _honest(v, GR.RS_F32_ERR[(H, W)][k], 6e-8 if k != "transpose" else 2e-10), (k, v, GR.RS_F32_ERR[(H, W)][k])


def test_resize_table_keeps_its_source_coordinates_off_the_integers():
    for n in sorted({s for hw in GR.RS_SHAPES for s in hw} - {224}):
        src = (n / 224) * (torch.arange(224, dtype=F64) + 0.5) - 0.5
        src = src[src > 0]
        if src.numel():
            assert float((src - src.round()).abs().min()) >= 1 / 448 - 1e-9, n


# ------------------------------------------------------------------------------------------------------------------------
# the head of a view
# ------------------------------------------------------------------------------------------------------------------------
def test_rays_restatement_is_the_dataset_and_its_float32_error():
    ds = GR.dataset()
    worst = dict(rays_d=0.0, near=0.0, far=0.0)
    for Wn, Hn in GR.GR_GRIDS:
        for sel in GR.GR_SEL:
            for prior in GR.GR_PRIOR:
                c = GR.rays_case(Wn, Hn, sel, prior)
                ref, f32 = GR.gen_rays(c), GR.dataset_rays(ds, c)
                fails, fig = GR.judge_rays(c, f32, ref)
                assert not fails, (Wn, Hn, sel, prior, fails)
                for k in worst:
                    worst[k] = max(worst[k], fig[k])
                mine32 = GR.gen_rays(c, dtype=F32)
                assert (mine32["rays_d"] - f32["rays_d"]).abs().max() < 5e-7
                assert float(ref["near"].min()) > 0.5          # (no ray near the decision `mid - 1 < 0`)
    print("float32 Dataset statement vs float64:", {k: "%.3g" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert _honest(v, GR.GR_F32_ERR[k], 6e-8), (k, v, GR.GR_F32_ERR[k])
    lin = torch.linspace(0, 255, 80)
    assert (torch.from_numpy(GR.linspace32(255, 80)) - lin).abs().max() <= 2 ** -16      # (an ulp at 255; torch's CPU kernel may fuse one product)


# ------------------------------------------------------------------------------------------------------------------------
# chess board, coarse depths, loss tail
# ------------------------------------------------------------------------------------------------------------------------
def test_chess_restatement_is_the_runner_and_its_float32_error():
    from avatarclip_amd.runner import chess_background
    worst = 0.0
    for H, W, L in GR.CH_SHAPES:
        for sigma in GR.CH_SIGMA:
            ref = GR.chess(H, W, L, sigma)
            f32 = chess_background(H, W, L, sigma, "cpu").reshape(H, W)
            worst = max(worst, float((f32.double() - ref).abs().max()))
            k32 = (GR.blur_taps(5, sigma, np.float32), GR.blur_taps(9, sigma, np.float32))
            assert float((GR.chess(H, W, L, sigma, taps=k32) - ref).abs().max()) < 1.2e-7     # the float32 taps the kernel is handed
            if L > max(H, W):
                assert (ref - 0.8).abs().max() < 1e-15 and GR.ALLOW * GR.CH_F32_ERR < 1e-6
    print("float32 chess_background vs float64: %.3g" % worst)
    assert worst <= GR.ALLOW * GR.CH_F32_ERR and _honest(worst, GR.CH_F32_ERR, 6e-8)


def test_coarse_z_statement_is_the_renderers():
    from avatarclip_amd.renderer import coarse_z_torch
    for R in GR.CZ_R:
        for n in GR.CZ_N:
            c = GR.coarse_case(R, n)
            for jit in (False, True):
                assert torch.equal(GR.coarse_z32(c, n, jit), coarse_z_torch(c["near"], c["far"], n, 1.0 if jit else 0.0, c["jitter"]))


def _tail_f32(c):
    """the torch statement of main.py:491-534 in float32 (as tests/test_gpu_glue.py writes it)"""
    w = GR.TAIL_W
    enc, sums, eik = (c[k].clone().requires_grad_(True) for k in ("enc", "sums", "eik"))
    B = enc.shape[0]
    colour, maskl = sums[0] / (sums[1] + 1e-5), sums[2] / w["P"]
    cs = [torch.cosine_similarity(torch.mean(enc[b:b + 1], dim=0), torch.mean(c["text"], dim=0), dim=0) for b in range(B)]
    loss = colour + eik * w["igr"] + maskl * w["mask"]
    for x in cs:
        loss = loss + (1.0 - x) * w["clip"]
    (loss * w["g"]).backward()
    out, dd = torch.zeros(8), torch.zeros(8)
    out[0], out[1], out[2] = loss.detach(), colour.detach(), maskl.detach()
    out[3:3 + B] = torch.stack(cs).detach()
    dd[0], dd[2], dd[4] = sums.grad[0], sums.grad[2], eik.grad
    return dict(loss=loss.detach(), out=out, d_enc=enc.grad, dd=dd)


def test_tail_restatement_is_cosine_similarity_and_its_float32_error():
    worst = dict(loss=0.0, out=0.0, d_enc=0.0, dd=0.0)
    for B in GR.LT_B:
        for T in GR.LT_T:
            c = GR.tail_case("generic", B, T)
            ref = GR.loss_tail(c)
            cs = torch.stack([torch.cosine_similarity(c["enc"][b].double(), c["text"].double().mean(0), dim=0) for b in range(B)])
            assert (cs - ref["cos"]).abs().max() < 1e-14
            for family in GR.LT_FAMILIES:
                c = GR.tail_case(family, B, T)
                ref = GR.loss_tail(c)
                assert all(torch.isfinite(v).all() for v in ref.values())
                if family == "text_mean_zero":
                    assert (c["text"].mean(0) == 0).all() and (ref["cos"] == 0).all() and (ref["d_enc"] == 0).all()
                    s = torch.zeros(512)
                    for t in range(T):
                        s = s + c["text"][t]
                    assert (s == 0).all()                                   # float32, in the order the rows are added
                if family == "degenerate_rows":
                    assert float(c["enc"][0].norm()) == 0 and (B < 2 or 0 < float(c["enc"][1].norm()) < 1e-8)
                if family == "generic":       # (torch.cosine_similarity clamps the product of the norms, not each: another function on the degenerate rows)
                    f32 = _tail_f32(c)
                else:
                    f32 = {k: v.float() for k, v in GR.loss_tail(c, dtype=F32).items()}
                fails, fig = GR.judge_tail(f32, ref)
                assert not fails, (family, B, T, fails)
                for k in worst:
                    worst[k] = max(worst[k], fig[k])
    print("float32 loss-tail statement vs float64:", {k: "%.3g" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert _honest(v, GR.LT_F32_ERR[k], 6e-8), (k, v, GR.LT_F32_ERR[k])


# ------------------------------------------------------------------------------------------------------------------------
# wrong kernels: one overridden decision each
# ------------------------------------------------------------------------------------------------------------------------
class BgRuleLE(GR.Statement):
    def is_background(self, ws32):
        return ws32 <= 0.5


class ClampGradOpen(GR.Statement):
    def outside_unit(self, x32):
        return x32 <= 0, x32 >= 1


class BceGradOpen(GR.Statement):
    def outside_clip(self, ws32):
        return ws32 <= GR.CLIP_LO, ws32 >= GR.CLIP_HI


class L1SignPlus(GR.Statement):
    def l1_sign(self, e32):
        return torch.where(e32 >= 0, torch.ones_like(e32), -torch.ones_like(e32))


class First256Blocks(GR.Statement):
    def summed_pixels(self, P):
        return slice(0, min(P, 256 * GR.BLOCK))


class DropSecondTapAtEnd(GR.Statement):
    def resize_matrix_bwd(self, n_in, dtype=F64):
        i0, i1, w0, w1 = self.taps(n_in, dtype)
        A = torch.zeros(GR.RES, n_in, dtype=dtype)
        A[torch.arange(GR.RES), i0] += w0
        A[torch.arange(GR.RES), i1] += torch.where(i1 == i0, torch.zeros_like(w1), w1)
        return A


class StencilNoMargin(GR.Statement):
    def resize_matrix_bwd(self, n_in, dtype=F64):
        """the gather over lo .. hi of input index i, float32 as the kernel computes them, without the index of margin either way"""
        A = self.resize_matrix(n_in, dtype)
        inv = np.float32(1.0) / (np.float32(n_in) / np.float32(GR.RES))
        i = np.arange(n_in, dtype=np.float32)
        lo = np.floor((i - np.float32(0.5)) * inv - np.float32(0.5)).astype(np.int64)
        hi = np.ceil((i + np.float32(1.5)) * inv - np.float32(0.5)).astype(np.int64)
        lo[0], hi[-1] = 0, GR.RES - 1
        o = torch.arange(GR.RES)[:, None]
        keep = (o >= torch.from_numpy(lo)[None, :]) & (o <= torch.from_numpy(hi)[None, :])
        return A * keep


class NearestByRounding(GR.Statement):
    def nearest_index(self, n_out, n_in):
        s32 = np.float32(n_in) / np.float32(n_out)
        return torch.clamp(torch.floor(torch.arange(n_out).float() * torch.tensor(s32) + 0.5).long(), max=n_in - 1)


class OneSidedLinspace(GR.Statement):
    def linspace_side(self, n):
        return torch.ones(n, dtype=torch.bool)


class ReflectRepeatsEdge(GR.Statement):
    def reflect(self, i, n):
        return torch.where(i < 0, -i - 1, torch.where(i >= n, 2 * n - 1 - i, i))


class NormBranchUnderClamp(GR.Statement):
    def clamp_norm(self, nr):
        return torch.where(nr.detach().float() > 1e-8, nr, 1e-8 + nr - nr.detach())


def _round32(d):
    return {k: (v.float() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in d.items()}


def _shade_fwd_verdicts(st, family, P, rop=True):
    c = GR.shade_case(family, P, rop)
    ref, mut = GR.shade_loss(c), GR.shade_loss(c, st=st)
    return GR.judge_shade_fwd(c, mut["images"].float(), mut["sums"].float(), ref)[0]


def _shade_bwd_verdicts(st, family, P, rop=True):
    c = GR.shade_case(family, P, rop)
    return GR.judge_shade_bwd(c, _round32(GR.shade_loss_grads(c, st=st)), GR.shade_loss_grads(c))[0]


def test_background_rule_with_le_is_rejected():
    """threshold family (wsum == 0.5 exactly is body, not background): images differ; the general family cannot see it"""
    assert _shade_fwd_verdicts(BgRuleLE(), "threshold", 257)
    assert not _shade_fwd_verdicts(BgRuleLE(), "general", 257)


def test_clamp_gradient_that_stops_at_the_ends_is_rejected():
    """threshold family: extra * s' of exactly 0 and 1 (dextra) and a normal exactly perpendicular to the light (dnsum)"""
    v = _shade_bwd_verdicts(ClampGradOpen(), "threshold", 257)
    assert any("dextra" in f for f in v) and any("dnsum" in f for f in v), v
    assert not _shade_fwd_verdicts(ClampGradOpen(), "threshold", 257)           # (same values: only the gradient is wrong)
    assert not _shade_bwd_verdicts(ClampGradOpen(), "general", 257)


def test_bce_gradient_that_stops_at_the_clip_ends_is_rejected():
    v = _shade_bwd_verdicts(BceGradOpen(), "threshold", 257)
    assert any("dwsum" in f for f in v), v
    assert not _shade_bwd_verdicts(BceGradOpen(), "general", 257)


def test_l1_sign_of_plus_one_at_zero_is_rejected():
    v = _shade_bwd_verdicts(L1SignPlus(), "threshold", 257)
    assert v == ["dcolor is not bit-equal"], v
    assert not _shade_bwd_verdicts(L1SignPlus(), "general", 257)


def test_sum_that_leaves_out_the_blocks_from_256_on_is_rejected():
    """exact family, P = 65537 (one pixel in block 256) and 131073: sums[0], [1], [3] are not torch.equal; P = 65536 is all summed"""
    for P in (65537, 131073):
        for rop in (False, True):
            v = _shade_fwd_verdicts(First256Blocks(), "exact", P, rop)
            assert any("exact sums differ" in f for f in v), (P, rop, v)
    assert not _shade_fwd_verdicts(First256Blocks(), "exact", 65536)
    assert _shade_fwd_verdicts(First256Blocks(), "general", 131073)            # (half the pixels missing: the 4 x margin sees that too)


def _resize_verdicts(st, H, W):
    case = GR.resize_case(H, W, 1)
    fx, f0 = GR.resize_norm(case["x"]).float(), GR.resize_norm(torch.zeros_like(case["x"])).float()
    bw, b1 = GR.resize_norm_bwd(case["w"], H, W, st).float(), GR.resize_norm_bwd(GR.onehot_dout(), H, W, st).float()
    return GR.judge_resize(H, W, fx, f0, bw, b1, case)[0]


def test_resize_backward_that_drops_the_second_tap_on_the_last_index_is_rejected():
    """(1, 1), (2, 3), (3, 2) and every other size: the outputs whose source coordinate lies past the last pixel's centre have both
    taps there; the transpose identity and the one-hot at the far corner see it"""
    for H, W in ((1, 1), (2, 3), (3, 2), (7, 5), (1000, 37)):
        v = _resize_verdicts(DropSecondTapAtEnd(), H, W)
        assert any("transpose" in f for f in v) and any("one-hot" in f for f in v), (H, W, v)
    for H, W in GR.RS_SHAPES:
        assert not _resize_verdicts(GR.HONEST, H, W), (H, W)


def test_resize_stencil_range_without_its_margin_is_the_same_gather_on_this_table():
    """NO WRONG KERNEL on the sizes of the table: the float32 lo / hi without the one-index margin still hold every output whose
    stencil touches the input index, so the gather is the honest one element for element.  The margin guards sizes where float32
    rounding of (i -+ 0.5) / scale crosses an integer; none of the table's does, and the transpose criterion would see it if one did."""
    for n in sorted({s for hw in GR.RS_SHAPES for s in hw} - {224}):
        assert torch.equal(StencilNoMargin().resize_matrix_bwd(n), GR.HONEST.resize_matrix_bwd(n)), n
    broken = StencilNoMargin().resize_matrix_bwd(1000).clone()                     # (a range one index short IS seen)
    keep = torch.ones_like(broken)
    keep[torch.arange(224), GR.HONEST.taps(1000)[1]] = 0
    st = types.SimpleNamespace(resize_matrix_bwd=lambda n, dtype=F64: GR.HONEST.resize_matrix(n, dtype) * (keep if n == 1000 else 1))
    case = GR.resize_case(1000, 37, 1)
    fx, f0 = GR.resize_norm(case["x"]).float(), GR.resize_norm(torch.zeros_like(case["x"])).float()
    v = GR.judge_resize(1000, 37, fx, f0, GR.resize_norm_bwd(case["w"], 1000, 37, st).float(), GR.resize_norm_bwd(GR.onehot_dout(), 1000, 37, st).float(), case)[0]
    assert any("transpose" in f for f in v), v


def test_nearest_resample_by_rounding_is_rejected():
    """prior `odd` (Hn + 3 x 2 Wn + 1) and `smaller` (Hn // 2 x Wn // 2) on the 5 x 9 grid: true_rgb is not bit-equal; `equal` and
    `larger` (2 Hn x 3 Wn: whole ratios) give the same index either way"""
    for prior, bad in (("larger", False), ("odd", True), ("smaller", True), ("equal", False)):
        c = GR.rays_case(5, 9, "none", prior)
        v = GR.judge_rays(c, _round32(GR.gen_rays(c, st=NearestByRounding())), GR.gen_rays(c))[0]
        assert bool(v) == bad and (not bad or "true_rgb is not bit-equal" in v), (prior, v)


def test_one_sided_linspace_is_rejected_by_bit_equality_only():
    """start + i step throughout is the same real number: in float64 the rays move by 1e-13 and the 4 x margin accepts them.  In float32
    the upper half of the pixel centres moves by an ulp: the bit-equality checks (avc_coarse_z against the torch ops at n = 63 and 64
    -- at n = 65 the step 1 / 64 is exact and both sides give the same floats --
    avc_gen_rays' pixel centres against torch.linspace on the 64 x 80 grid) are what rejects it"""
    c = GR.rays_case(64, 80, "none", "none")
    assert not GR.judge_rays(c, _round32(GR.gen_rays(c, st=OneSidedLinspace())), GR.gen_rays(c))[0]
    side = OneSidedLinspace().linspace_side
    assert not np.array_equal(GR.linspace32(255, 80, side(80)), GR.linspace32(255, 80))
    assert not torch.equal(GR.gen_rays(c, st=OneSidedLinspace(), dtype=F32)["rays_d"], GR.gen_rays(c, dtype=F32)["rays_d"])
    for n, differs in ((1, False), (2, False), (63, True), (64, True), (65, False)):
        cz = GR.coarse_case(257, n)
        one = torch.from_numpy(GR.linspace32(1.0, n, side(n)))
        assert (not torch.equal(GR.coarse_z32(cz, n, True, lin=one), GR.coarse_z32(cz, n, True))) == differs, n


def test_reflect_padding_that_repeats_the_edge_is_rejected():
    """(5, 3, 1), where every tap reflects, and (9, 5, 2), at sigma 0.7 and 1.9: squares of one or two pixels, so the pixel behind the
    edge has the other colour.  Not everywhere: at sigma 0.1 the blur is the identity (the neighbours weigh e^-50), a square of 5 or more
    holds the reflected and the repeated pixel alike but for the outermost tap of nine, and L larger than the image is 0.8 either way"""
    for H, W, L in GR.CH_SHAPES:
        for sigma in GR.CH_SIGMA:
            err = float((GR.chess(H, W, L, sigma, st=ReflectRepeatsEdge()) - GR.chess(H, W, L, sigma)).abs().max())
            if L <= 2 and sigma > 0.5:
                assert err > 100 * GR.ALLOW * GR.CH_F32_ERR, (H, W, L, sigma, err)
            if L > max(H, W) or sigma < 0.5:
                assert err < 1e-12, (H, W, L, sigma, err)


def test_cosine_gradient_with_the_norms_branch_under_the_clamp_is_rejected():
    """degenerate_rows with B >= 2: image 1 has a norm of 2e-9, under the clamp but not zero.  On the zero row (B = 1) the branch
    multiplies e = 0: the same gradient, no wrong kernel there"""
    for B in (2, 3, 4):
        c = GR.tail_case("degenerate_rows", B, 3)
        v = GR.judge_tail(_round32(GR.loss_tail(c, st=NormBranchUnderClamp())), GR.loss_tail(c))[0]
        assert any("d_enc" in f for f in v), (B, v)
    c = GR.tail_case("degenerate_rows", 1, 3)
    assert torch.equal(GR.loss_tail(c, st=NormBranchUnderClamp())["d_enc"], GR.loss_tail(c)["d_enc"])
    c = GR.tail_case("generic", 4, 3)
    assert not GR.judge_tail(_round32(GR.loss_tail(c, st=NormBranchUnderClamp())), GR.loss_tail(c))[0]


def test_out_slots_of_the_loss_tail_hold_every_cosine():
    """the criterion behind the out[3 + b] change: a kernel that reports cos_0 and cos_1 only is rejected at B = 3 and 4"""
    for B in GR.LT_B:
        c = GR.tail_case("generic", B, 3)
        ref = GR.loss_tail(c)
        got = _round32(ref)
        got["out"] = got["out"].clone()
        got["out"][5:] = 0
        assert bool(GR.judge_tail(got, ref)[0]) == (B > 2)
