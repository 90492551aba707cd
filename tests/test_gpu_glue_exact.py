"""The nine kernels of csrc/avc_glue.hip -- avc_shade_loss_fwd / _bwd, avc_resize_norm_fwd / _bwd, avc_gen_rays, avc_chess_background,
avc_coarse_z, avc_loss_tail_fwd / _bwd -- pixel by pixel against the float64 restatement of tests/glue_restatement.py (pinned on the CPU
by tests/test_glue_restatement_cpu.py, which also measures every tolerance used here and shows which wrong kernel each case rejects), at
the sizes where their code takes another path: below / at / past a wavefront and a block, 257 and 513 blocks (the last block's strided
loop over the partials), one-pixel images, both taps on the last index, grids of one row or column, B = 1 .. 4 embeddings.

Called through lib.call with buffers of the test's own: every output is one row longer than the kernel may write and pre-filled with a
sentinel that has to survive there.  Copies and comparisons are bit-equal, sums of quarters are exact in any order, everything else is
within 4 x what the float32 CPU statement of the same lines leaves against float64 (GR.*_F32_ERR); profiles/glue_exact.md has the
measured figures."""
import numpy as np
import pytest
import torch

from tests import glue_restatement as GR

gpu = pytest.mark.gpu
SENT = -777.0


def _L():
    from avatarclip_amd import lib as L
    L.load()
    return L


def D(t):
    return None if t is None else t.contiguous().to("cuda")


def _buf(rows, *inner, dtype=torch.float32):
    """[rows + 1, *inner] of the sentinel: the kernel may write the first `rows`"""
    return torch.full((rows + 1,) + tuple(inner), SENT, dtype=dtype, device="cuda")


def _take(buf, rows=None):
    """the rows the kernel may write, on the CPU; the row past them must still hold the sentinel"""
    torch.cuda.synchronize()
    b = buf.cpu()
    rows = b.shape[0] - 1 if rows is None else rows
    assert (b[rows:] == SENT).all(), "a launch wrote past its last row"
    return b[:rows]


class Figures(dict):
    def take(self, fig, where):
        for k, v in fig.items():
            if v >= self.get(k, (-1.0, None))[0]:
                self[k] = (v, where)

    def show(self, title, allowed):
        for k, (v, where) in sorted(self.items()):
            a = allowed.get(k)
            print("%s %s: %.3g%s at %s" % (title, k, v, "" if not a else " = %.2f of the allowance %.3g" % (v / a, a), where))


# ------------------------------------------------------------------------------------------------------------------------
# avc_shade_loss_fwd / _bwd
# ------------------------------------------------------------------------------------------------------------------------
SHADE_OPTIONS = [(True, False, "image"), (True, True, "const0"), (False, False, "const1"), (True, False, "const1")]      # (nsum, img0_is_extra, background)


def _shade_fwd(c, dev, nsum, img0x, bg_mode, ticket):
    L = _L()
    P = c["P"]
    blocks = L.load().avc_shade_loss_blocks(P)
    assert blocks == (P + GR.BLOCK - 1) // GR.BLOCK
    images, partial, sums = _buf(2 * P, 3), _buf(blocks, 4), _buf(4)
    L.call("avc_shade_loss_fwd", dev["color"], dev["extra"], dev["wsum"], dev["nsum"] if nsum else None, dev["true_rgb"], dev["mask"],
           dev["ray_of_pixel"], dev["bg"] if bg_mode == "image" else None, 1.0 if bg_mode == "const1" else 0.0, dev["light"] if nsum else None,
           P, int(img0x), images, partial, sums, ticket)
    out = _take(images).reshape(2, P, 3), _take(partial), _take(sums)
    assert int(ticket.cpu()) == 0, "the ticket is not left at zero"
    return out


def _dev(c):
    return {k: D(v) if torch.is_tensor(v) else v for k, v in c.items()}


@gpu
@pytest.mark.parametrize("P", GR.SH_P)
def test_shade_loss_forward_pixel_by_pixel(P):
    """1, 256, 257 and 513 blocks; with and without ray_of_pixel (half the pixels unowned, the rays a permutation); the three
    backgrounds; nsum NULL and given; img0_is_extra.  Images per element, copies bit-equal; sums[0], [1], [3] of the exact family
    torch.equal (a block of partials left out cannot hide); the per-block partials add up to the sums; the same launch twice gives the
    same bits; the ticket reads 0 after every launch"""
    figs, failed = Figures(), []
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    for family in GR.SH_FAMILIES:
        for rop in (False, True):
            c = GR.shade_case(family, P, rop)
            dev = _dev(c)
            for nsum, img0x, bg_mode in SHADE_OPTIONS:
                where = (family, rop, nsum, img0x, bg_mode)
                ref = GR.shade_loss(c, nsum, img0x, bg_mode)
                images, partial, sums = _shade_fwd(c, dev, nsum, img0x, bg_mode, ticket)
                fails, fig = GR.judge_shade_fwd(c, images, sums, ref)
                figs.take(fig, where)
                if fails:
                    failed.append((where, fails))
                perr = GR.partial_err(partial, ref["terms"], P)         # the partials are per-block sums of the same terms
                figs.take(dict(partial=perr), where)
                if perr > GR.ALLOW * GR.SH_F32_ERR["partial"]:
                    failed.append((where, "a block's partial sums off by %.3g" % perr))
                again = _shade_fwd(c, dev, nsum, img0x, bg_mode, ticket)
                assert torch.equal(again[2], sums) and torch.equal(again[1], partial) and torch.equal(again[0], images), where
    figs.show("shade_loss_fwd P = %d" % P, dict(images=GR.ALLOW * GR.SH_F32_ERR["images"], sums=GR.ALLOW * GR.SH_F32_ERR["sums"], partial=GR.ALLOW * GR.SH_F32_ERR["partial"]))
    assert not failed, failed


@gpu
def test_shade_loss_forward_one_ticket_for_grids_of_every_size():
    """five launches of 2, 257, 1, 513 and 1 blocks on ONE ticket: each is right, so the word is back at zero after each and does not
    carry the grid size of the launch before"""
    ticket = torch.zeros(1, dtype=torch.int32, device="cuda")
    for P in (257, 65537, 63, 131073, 256):
        c = GR.shade_case("exact", P, True)
        images, partial, sums = _shade_fwd(c, _dev(c), True, False, "image", ticket)
        fails, _ = GR.judge_shade_fwd(c, images, sums, GR.shade_loss(c))
        assert not fails, (P, fails)


def _shade_bwd(c, dev, nsum, img0x, use0, use1, R=None):
    R = c["R"] if R is None else R
    bufs = dict(dcolor=_buf(R, 3), dextra=_buf(R, 3), dwsum=_buf(R))
    if nsum:
        bufs["dnsum"] = _buf(R, 3)
    _L().call("avc_shade_loss_bwd", dev["color"], dev["extra"], dev["wsum"], dev["nsum"] if nsum else None, dev["true_rgb"], dev["mask"],
              dev["ray_of_pixel"], dev["light"] if nsum else None, c["P"], int(img0x), dev["dimg0"] if use0 else None,
              dev["dimg1"] if use1 else None, dev["gs"], bufs["dcolor"], bufs["dextra"], bufs["dwsum"], bufs.get("dnsum"))
    return {k: _take(v) for k, v in bufs.items()}


@gpu
@pytest.mark.parametrize("P", GR.SH_P_BWD)
def test_shade_loss_backward_ray_by_ray(P):
    """dcolor, dextra, dwsum, dnsum per element against torch.autograd of the float64 restatement, on every family: the threshold
    family sits on wsum = 0.5, 1e-3 and 1 - 1e-3, extra x s' = 0 and 1, normals exactly perpendicular, parallel and opposed to the
    light, zero and NaN normals (finite, and autograd's), color == true_rgb.  dimg0 NULL, dimg1 NULL, both given; nsum NULL; img0_is_extra"""
    figs, failed = Figures(), []
    for family in GR.SH_FAMILIES:
        for rop in (False, True):
            c = GR.shade_case(family, P, rop)
            dev = _dev(c)
            for nsum, img0x, use0, use1 in ((True, False, True, True), (True, False, False, True), (True, False, True, False),
                                            (True, True, True, True), (False, False, True, True)):
                where = (family, rop, nsum, img0x, use0, use1)
                ref = GR.shade_loss_grads(c, nsum, img0x, use0, use1)
                assert ref["owns"].all()
                got = _shade_bwd(c, dev, nsum, img0x, use0, use1)
                assert all(torch.isfinite(v).all() for v in got.values()), where
                fails, fig = GR.judge_shade_bwd(c, got, ref)
                figs.take(fig, where)
                if fails:
                    failed.append((where, fails))
    figs.show("shade_loss_bwd P = %d" % P, {k: GR.ALLOW * GR.SH_F32_ERR[k] for k in ("dextra", "dwsum", "dnsum")})
    assert not failed, failed


@gpu
def test_rays_without_a_pixel_keep_the_buffer_and_get_zero_through_the_function():
    """three rays more than pixels own: a direct call leaves their rows as they were (the sentinel), glue.ShadeLossFn returns 0 there"""
    from avatarclip_amd import glue
    c = GR.shade_case("general", 257, True)
    R = c["R"]
    g = torch.Generator().manual_seed(3)
    for k in ("color", "extra", "nsum"):
        c[k] = torch.cat([c[k], torch.rand(3, 3, generator=g)])
    c["wsum"] = torch.cat([c["wsum"], torch.rand(3, generator=g)])
    dev = _dev(c)
    ref = GR.shade_loss_grads(dict(c, R=R + 3))
    assert ref["owns"].tolist() == [True] * R + [False] * 3
    got = _shade_bwd(c, dev, True, False, True, True, R=R + 3)
    for k, v in got.items():
        assert (v[R:] == SENT).all(), k
    fails, _ = GR.judge_shade_bwd(c, got, ref)
    assert not fails, fails
    leaf = {k: dev[k].clone().requires_grad_(True) for k in ("color", "extra", "wsum", "nsum")}
    images, sums = glue.ShadeLossFn.apply(leaf["color"], leaf["extra"], leaf["wsum"], leaf["nsum"], dev["true_rgb"], dev["mask"],
                                          dev["ray_of_pixel"], dev["bg"], 0.0, dev["light"], False)
    ((images[0] * dev["dimg0"]).sum() + (images[1] * dev["dimg1"]).sum() + (sums * dev["gs"]).sum()).backward()
    fn = {"d" + k: v.grad.cpu() for k, v in leaf.items()}
    for k, v in fn.items():
        assert (v[R:] == 0).all(), k
        assert torch.equal(v[:R], got[k][:R]), k
    fails, _ = GR.judge_shade_fwd(c, images.detach().cpu(), sums.detach().cpu(), GR.shade_loss(dict(c, R=R + 3)))
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------------
# avc_resize_norm_fwd / _bwd
# ------------------------------------------------------------------------------------------------------------------------
def _resize_fwd(x):
    from avatarclip_amd import glue
    B, H, W, _ = x.shape
    out = _buf(B * 3 * GR.RES, GR.RES)
    _L().call("avc_resize_norm_fwd", D(x), B, H, W, glue._MEAN, glue._STD, out)
    return _take(out).reshape(B, 3, GR.RES, GR.RES)


def _resize_bwd(dout, H, W):
    from avatarclip_amd import glue
    B = dout.shape[0]
    din = _buf(B * H, W, 3)
    _L().call("avc_resize_norm_bwd", D(dout), B, H, W, glue._MEAN, glue._STD, din)
    return _take(din).reshape(B, H, W, 3)


@gpu
@pytest.mark.parametrize("H,W", GR.RS_SHAPES)
def test_resize_norm_forward_and_its_transpose(H, W):
    """forward per element within 4 x the float32 F.interpolate's own offset at that shape; the backward as the forward's transpose
    (<fwd(x) - fwd(0), w> = <x, bwd(w)> in float64 from the kernels' outputs), its one-hot gradients at the four corners, an edge
    and an interior pixel equal to the forward's weights and zero elsewhere, exact zeros at input pixels no output touches"""
    for B in GR.RS_B:
        case = GR.resize_case(H, W, B)
        fx, f0 = _resize_fwd(case["x"]), _resize_fwd(torch.zeros_like(case["x"]))
        bw, b1 = _resize_bwd(case["w"], H, W), _resize_bwd(GR.onehot_dout(), H, W)
        fails, fig = GR.judge_resize(H, W, fx, f0, bw, b1, case)
        tol = GR.RS_F32_ERR[(H, W)]
        print("resize_norm (%d, %d) B = %d: %s; pixels no output touches: %d" % (
            H, W, B, ", ".join("%s %.3g = %.2f of the allowance" % (k, fig[k], fig[k] / (GR.ALLOW * tol[k])) for k in tol), fig["untouched"]))
        assert not fails, (B, fails)
        if (H, W) == (224, 224):
            mean, std = GR._norm(torch.float64)
            assert (fx.double() - (case["x"].double().permute(0, 3, 1, 2) - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)).abs().max() < 4e-7
    if (H, W) == (1000, 37):
        assert fig["untouched"] >= 1000 * 37 // 2          # (a strong reduction: most input pixels feed no output)


# ------------------------------------------------------------------------------------------------------------------------
# avc_gen_rays
# ------------------------------------------------------------------------------------------------------------------------
def _gen_rays(c):
    Wn, Hn, R = c["Wn"], c["Hn"], c["R"]
    n = Wn * Hn
    bufs = dict(rays_o=_buf(R, 3), rays_d=_buf(R, 3), near=_buf(R), far=_buf(R), true_rgb=_buf(n, 3), mask=_buf(n))
    pr = c["prior"]
    Hp, Wp = (0, 0) if pr is None else pr.shape[:2]
    W, H, focal = GR.CAMERA
    _L().call("avc_gen_rays", D(c["pose"]), D(c["sel"]), D(pr), Hp, Wp, float(W), float(H), float(focal), Wn, Hn, R, bufs["rays_o"], bufs["rays_d"],
              bufs["near"], bufs["far"], bufs["true_rgb"] if pr is not None else None, bufs["mask"] if pr is not None else None)
    out = {k: _take(v) for k, v in bufs.items() if pr is not None or k not in ("true_rgb", "mask")}
    if pr is None:
        torch.cuda.synchronize()
        assert (bufs["true_rgb"] == SENT).all() and (bufs["mask"] == SENT).all()
    return out


@gpu
@pytest.mark.parametrize("Wn,Hn", GR.GR_GRIDS)
def test_gen_rays_ray_by_ray(Wn, Hn):
    """grids of one pixel, one row, one column, odd and non-square; sel NULL, sorted, a permutation, one ray, more rays than pixels;
    prior NULL, smaller, equal, larger, no multiple of the grid; a pose whose rotation has no zero entry.  rays_o, true_rgb and mask
    bit-equal; rays_d, near, far within 4 x the float32 Dataset's own error.  Against the same torch statement run on the GPU (what
    Runner._view_head_torch runs) rays_o and the resampled prior are bit-equal; rays_d, near and far are NOT (torch's norm and sums
    round differently): the distance is printed in units in the last place and held to twice the allowance, both being within one
    allowance of float64"""
    figs, failed = Figures(), []
    worst = {k: [0.0, 0] for k in ("rays_d", "near", "far")}
    ds = GR.dataset("cuda")
    for sel in GR.GR_SEL:
        for prior in GR.GR_PRIOR:
            c = GR.rays_case(Wn, Hn, sel, prior)
            got, ref = _gen_rays(c), GR.gen_rays(c)
            fails, fig = GR.judge_rays(c, got, ref)
            figs.take(fig, (sel, prior))
            if fails:
                failed.append(((sel, prior), fails))
            tor = {k: v.cpu() for k, v in GR.dataset_rays(ds, c).items()}
            assert torch.equal(got["rays_o"], tor["rays_o"])
            if c["prior"] is not None:
                assert torch.equal(got["true_rgb"], tor["true_rgb"]) and torch.equal(got["mask"], tor["mask"])
            for k in worst:
                diff = (got[k].double() - tor[k].double()).abs()
                # units in the last place of the ray's largest component (rays_d: a unit vector) resp. of the value itself
                size = tor[k].abs().max(-1, keepdim=True)[0] if k == "rays_d" else tor[k].abs()
                ulp = torch.exp2(torch.floor(torch.log2(size.double().clamp_min(1e-30))) - 23)
                worst[k] = [max(worst[k][0], float(diff.max())), max(worst[k][1], float((diff / ulp).max()))]
    figs.show("gen_rays (%d, %d)" % (Wn, Hn), {k: GR.ALLOW * v for k, v in GR.GR_F32_ERR.items()})
    print("gen_rays (%d, %d) against the torch statement on the GPU (largest |difference|, in ulps):" % (Wn, Hn),
          {k: "%.3g, %.1f" % tuple(v) for k, v in worst.items()})
    assert not failed, failed
    for k, v in worst.items():
        assert v[0] <= 2 * GR.ALLOW * GR.GR_F32_ERR[k], (k, v)


# ------------------------------------------------------------------------------------------------------------------------
# avc_chess_background, avc_coarse_z
# ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("H,W,L", GR.CH_SHAPES)
def test_chess_background_pixel_by_pixel(H, W, L):
    """the smallest legal image (every tap reflects), squares of one pixel, squares larger than the image (0.8 everywhere)"""
    for sigma in GR.CH_SIGMA:
        taps = torch.from_numpy(np.concatenate([GR.blur_taps(5, sigma, np.float32), GR.blur_taps(9, sigma, np.float32)]))
        out = _buf(H, W)
        _L().call("avc_chess_background", out, H, W, L, D(taps))
        got = _take(out)
        err = float((got.double() - GR.chess(H, W, L, sigma)).abs().max())
        print("chess (%d, %d, %d) sigma %.1f: %.3g = %.2f of the allowance" % (H, W, L, sigma, err, err / (GR.ALLOW * GR.CH_F32_ERR)))
        assert err <= GR.ALLOW * GR.CH_F32_ERR, (sigma, err)
        if L > max(H, W):
            assert float((got.double() - 0.8).abs().max()) <= GR.ALLOW * GR.CH_F32_ERR


@gpu
@pytest.mark.parametrize("R", GR.CZ_R)
def test_coarse_z_equals_the_torch_ops_bit_for_bit(R):
    """n = 1 (linspace's single point), 2, and 63 | 64 | 65 around a power of two -- where n is none, torch's division of the jitter by
    n (a multiplication by the float32 reciprocal) is not the quotient; near = 0, far = 1 returns the kernel's linspace itself"""
    from avatarclip_amd.renderer import coarse_z_torch
    for n in GR.CZ_N:
        z = _buf(R, n)
        _L().call("avc_coarse_z", torch.zeros(R, 1, device="cuda"), torch.ones(R, 1, device="cuda"), None, R, n, z)
        assert torch.equal(_take(z), torch.linspace(0.0, 1.0, n, device="cuda").cpu()[None, :].expand(R, n)), n
    for n in GR.CZ_N:
        c = GR.coarse_case(R, n)
        near, far, jit = D(c["near"]), D(c["far"]), D(c["jitter"])
        for jitter in (False, True):
            z = _buf(R, n)
            _L().call("avc_coarse_z", near, far, jit if jitter else None, R, n, z)
            want = coarse_z_torch(near, far, n, 1.0 if jitter else 0.0, jit)
            got = _take(z)
            assert torch.equal(got, want.cpu()), (n, jitter, int((got != want.cpu()).sum()), float((got - want.cpu()).abs().max()))


# ------------------------------------------------------------------------------------------------------------------------
# avc_loss_tail_fwd / _bwd
# ------------------------------------------------------------------------------------------------------------------------
def _tail(c, B=None, D_=512, bufs=None):
    w = GR.TAIL_W
    B = c["enc"].shape[0] if B is None else B
    T = c["text"].shape[0]
    enc, text, sums, eik = D(c["enc"]), D(c["text"]), D(c["sums"]), D(c["eik"].reshape(1))
    loss, out, saved, d_enc, dd = bufs if bufs is not None else (_buf(1), _buf(8), _buf(4 * B + 1), _buf(c["enc"].shape[0], 512), _buf(8))
    L = _L()
    L.call("avc_loss_tail_fwd", enc, text, B, T, D_, sums, eik, w["igr"], w["mask"], w["clip"], w["P"], loss, out, saved)
    _take(saved)
    g = torch.tensor([w["g"]], device="cuda")
    L.call("avc_loss_tail_bwd", g, enc, text, B, T, D_, sums, saved, w["igr"], w["mask"], w["clip"], w["P"], d_enc, dd)
    return dict(loss=_take(loss)[0], out=_take(out), d_enc=_take(d_enc), dd=_take(dd))


@gpu
@pytest.mark.parametrize("B", GR.LT_B)
def test_loss_tail_every_image_and_every_degenerate_row(B):
    """B = 1 .. 4 (out[3 + b] = cos_b for EVERY b < B), T = 1, 3, 77; a zero embedding row and a row under the 1e-8 clamp; a text mean
    of zero: loss, out[8], d_enc per element, dd[0..4]"""
    figs, failed = Figures(), []
    for T in GR.LT_T:
        for family in GR.LT_FAMILIES:
            c = GR.tail_case(family, B, T)
            ref = GR.loss_tail(c)
            got = _tail(c)
            fails, fig = GR.judge_tail(got, ref)
            figs.take(fig, (family, T))
            if fails:
                failed.append(((family, T), fails))
            assert (got["out"][3:3 + B].double() - ref["cos"]).abs().max() <= GR.ALLOW * GR.LT_F32_ERR["out"], (family, T, got["out"], ref["cos"])
            if family == "generic":
                assert (got["out"][3:3 + B] != 0).all()
    figs.show("loss_tail B = %d" % B, {k: GR.ALLOW * v for k, v in GR.LT_F32_ERR.items()})
    assert not failed, failed


@gpu
def test_loss_tail_refuses_five_images_and_other_widths():
    """argument checks on the host: the error code with its message, and nothing is launched (every buffer keeps the sentinel)"""
    L = _L()
    w = GR.TAIL_W
    c = GR.tail_case("generic", 4, 3)
    enc, text, sums, eik = D(torch.cat([c["enc"], c["enc"][:1]])), D(c["text"]), D(c["sums"]), D(c["eik"].reshape(1))
    g = torch.tensor([w["g"]], device="cuda")
    loss, out, saved, d_enc, dd = _buf(1), _buf(8), _buf(21), _buf(5, 512), _buf(8)
    for B, width in ((5, 512), (4, 511), (0, 512)):
        with pytest.raises(RuntimeError, match="avc_loss_tail_fwd: built for 512-wide embeddings, 1-4 images"):
            L.call("avc_loss_tail_fwd", enc, text, B, 3, width, sums, eik, w["igr"], w["mask"], w["clip"], w["P"], loss, out, saved)
        with pytest.raises(RuntimeError, match="avc_loss_tail_bwd: built for 512-wide embeddings, 1-4 images"):
            L.call("avc_loss_tail_bwd", g, enc, text, B, 3, width, sums, saved, w["igr"], w["mask"], w["clip"], w["P"], d_enc, dd)
    torch.cuda.synchronize()
    for b in (loss, out, saved, d_enc, dd):
        assert (b == SENT).all()
