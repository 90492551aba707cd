"""GPU parity of the CLIP ViT-B/32 image encoder kernels vs the fp32 CPU oracle (seeded weights, see
oracle/clip_vit_oracle.py for the parity status).  Tolerances: bf16 GEMM operands with fp32 accumulate ->
cosine similarity of the embeddings >= 0.9995 and |d cos(emb, text)| <= 1e-3 (north-star: CLIP cosine tolerance);
pixel gradient relative L2 error <= 3e-2."""
import pytest
import torch

from oracle import clip_vit_oracle as C

gpu = pytest.mark.gpu


@gpu
def test_vit_linear_and_attention_kernels():
    from avatarclip_amd import clip_vit as V
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    for (M, N, K, act) in ((50, 768, 768, 0), (100, 3072, 768, 1), (2, 512, 768, 0), (130, 768, 3072, 0)):
        x = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) * K ** -0.5
        b = torch.randn(N, generator=g) * 0.1
        r = torch.randn(M, N, generator=g)
        lin = V._Lin(w, b, dev)
        xd = x.to(dev).requires_grad_(True)
        y = V.LinearFn.apply(xd, lin, act, r.to(dev))
        xb, wb = x.bfloat16().float(), w.bfloat16().float()
        pre = xb @ wb.t() + b
        ref = (C.quick_gelu(pre) if act else pre) + r
        assert torch.allclose(y.detach().cpu(), ref, atol=2e-3, rtol=2e-3), (M, N, K, (y.detach().cpu() - ref).abs().max())
        dy = torch.randn(M, N, generator=g)
        y.backward(dy.to(dev))
        xr = x.clone().requires_grad_(True)
        pre_r = xr @ w.t() + b
        ((C.quick_gelu(pre_r) if act else pre_r) * dy).sum().backward()
        rel = (xd.grad.cpu() - xr.grad).norm() / xr.grad.norm()
        assert rel < 1e-2, (M, N, K, rel)
    # attention on the matrix core: bf16 operands (q/8, k, v, P, dO, dS), fp32 accumulation and softmax.  Two checks: (1) against the
    # SAME arithmetic restated in torch (operands rounded at the same points): atol/rtol 2e-3 -- this pins the index mapping of
    # the kernels; (2) against fp32 attention: relative L2 error <= 1e-2 (forward) / 2e-2 (gradient) -- the cost of bf16 operands.
    qkv = torch.randn(2, 50, 2304, generator=g)
    do = torch.randn(2, 50, 768, generator=g)
    qd = qkv.to(dev).requires_grad_(True)
    out = V.AttentionFn.apply(qd)
    out.backward(do.to(dev))
    sh = lambda t: t.reshape(2, 50, 12, 64).permute(0, 2, 1, 3)
    un = lambda t: t.permute(0, 2, 1, 3).reshape(2, 50, 768)
    bf = lambda t: t.bfloat16().float()
    qr = qkv.clone().requires_grad_(True)
    q, k, v = qr.split(768, dim=-1)
    att = torch.softmax(sh(q) @ sh(k).transpose(-1, -2) / 8.0, dim=-1)
    ref = un(att @ sh(v))
    (ref * do).sum().backward()
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    e_out, e_grad = rel(out.detach().cpu(), ref.detach()), rel(qd.grad.cpu(), qr.grad)
    print("attention vs fp32: forward rel", e_out, "gradient rel", e_grad)
    assert e_out < 1e-2 and e_grad < 2e-2, (e_out, e_grad)
    with torch.no_grad():
        q, k, v = (sh(t) for t in qkv.split(768, dim=-1))
        qs, kb, vb, dob = bf(q * 0.125), bf(k), bf(v), bf(sh(do))
        P = torch.softmax(qs @ kb.transpose(-1, -2), dim=-1)
        o_b = un(bf(P) @ vb)
        dP = dob @ vb.transpose(-1, -2)
        dS = P * (dP - (P * dP).sum(-1, keepdim=True))
        dq, dk, dv = bf(dS * 0.125) @ kb, bf(dS).transpose(-1, -2) @ qs, bf(P).transpose(-1, -2) @ dob
        g_b = torch.cat([un(dq), un(dk), un(dv)], dim=-1)
    assert torch.allclose(out.detach().cpu(), o_b, atol=2e-3, rtol=2e-3), (out.detach().cpu() - o_b).abs().max()
    assert torch.allclose(qd.grad.cpu(), g_b, atol=2e-3, rtol=2e-3), (qd.grad.cpu() - g_b).abs().max()


@gpu
@pytest.mark.parametrize("B", [3, 8, 37])
def test_batched_scoring_pipeline_matches_the_autograd_path_and_the_oracle(B):
    """The packed route above 128 rows (ClipVisionB32._blocks_packed: no-grad calls with 3+ images, LayerNorm / attention / c_fc hand
    packed bf16 operands to the linear behind them) against the per-kernel route (_blocks_per_kernel: fp32 rows + a packing pass per
    linear): the same arithmetic with the same
    rounding points; what differs is the fp32 LayerNorm (own kernel vs torch), whose last-bit differences flip bf16 roundings that
    twelve layers then carry along: cosine >= 0.99999, |d| <= 5e-3 of the norm (measured 2.5e-3 .. 3.0e-3 -- about what either
    pipeline differs from the fp32 oracle by); and against the fp32 CPU oracle with the tolerance of test_encode_image_matches_oracle.  B = 37: 1850 rows = 14.5 row-tile groups (ragged
    last block); B = 3: the smallest batched call (150 rows)."""
    from avatarclip_amd import clip_vit as V
    dev = torch.device("cuda")
    sd = C.random_state_dict(0)
    model = V.ClipVisionB32(sd, dev)
    img = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(B))
    with torch.no_grad():
        e_packed = model.encode_image(img.to(dev)).cpu()
        assert set(model._packed) == {"ln", "attn", "fc"}      # the packed route ran, on the grown-on-demand operands of > 128 rows
        assert torch.equal(e_packed, model._encode_image_eager(img.to(dev), model._blocks_packed).cpu())
        e_rows = model._encode_image_eager(img.to(dev), model._blocks_per_kernel).cpu()
        assert set(model._packed) == {"ln", "attn", "fc"}      # ... and the per-kernel route is another one: no packed operand of its own
        ref = C.encode_image(sd, img[: min(B, 4)])
    cos = torch.cosine_similarity(e_packed, e_rows, dim=-1)
    rel = ((e_packed - e_rows).norm(dim=-1) / e_rows.norm(dim=-1)).max().item()
    print("packed vs row pipeline: min cosine", cos.min().item(), "max relative difference", rel)
    assert cos.min() > 0.99999 and rel < 5e-3
    assert torch.cosine_similarity(e_packed[: ref.shape[0]], ref, dim=-1).min() > 0.9995


@gpu
@pytest.mark.parametrize("B", [1, 2])
def test_training_call_replayed_as_hip_graphs_is_bit_identical_to_eager_launches(B, monkeypatch):
    """ClipVisionB32.encode_image with a gradient to the pixels (the per-iteration call, main.py:512,524): forward and backward replayed
    as HIP graphs must give exactly what the eager launches give -- embeddings and pixel gradients bit for bit, on fresh inputs and
    on repeated replays."""
    from avatarclip_amd import clip_vit as V
    dev = torch.device("cuda")
    model = V.ClipVisionB32(C.random_state_dict(0), dev)
    text = torch.randn(1, 512, generator=torch.Generator().manual_seed(5)).to(dev)
    assert V.TRAIN_GRAPH
    for k in range(3):
        img = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(10 + k)).to(dev)
        out = []
        for graph in (True, False):
            monkeypatch.setattr(V, "TRAIN_GRAPH", graph)
            x = img.clone().requires_grad_(True)
            e = model.encode_image(x)
            (1 - torch.cosine_similarity(e.mean(0), text.mean(0), dim=0)).backward()
            out.append((e.detach().clone(), x.grad.clone()))
        assert B in model._graphed                              # the graphed route ran
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), k


@gpu
@pytest.mark.parametrize("B", [1, 2])
def test_fused_residual_blocks_equal_the_per_kernel_autograd_path(B):
    """BlocksFn (the 12 residual blocks of a per-iteration call as one autograd node with packed bf16 hand-offs, forward and
    backward) against the same arithmetic as one autograd node per kernel (LinearFn / AttentionFn / F.layer_norm): the only
    difference is the LayerNorm statistics' summation order (last-bit fp32 -> an occasional bf16 rounding flip, carried through 12
    blocks of seeded-random weights), so embeddings agree to 4e-3 relative L2 and pixel gradients to 1e-2 (measured 2.1e-3 / 5.7e-3)
    -- and, the check that separates rounding from a defect, the fused path is no further from the fp32 oracle than the per-kernel
    path is (x 1.25); both with and without a gradient."""
    from avatarclip_amd import clip_vit as V
    dev = torch.device("cuda")
    model = V.ClipVisionB32(C.random_state_dict(0), dev)
    text = torch.randn(1, 512, generator=torch.Generator().manual_seed(5)).to(dev)
    img = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(31)).to(dev)
    res = []
    for blocks in (model._blocks_packed, model._blocks_per_kernel):
        x = img.clone().requires_grad_(True)
        e = model._encode_image_eager(x, blocks)
        (1 - torch.cosine_similarity(e.mean(0), text.mean(0), dim=0)).backward()
        with torch.no_grad():
            e0 = model._encode_image_eager(img, blocks)
        res.append((e.detach().clone(), x.grad.clone(), e0))
    x = img.clone().requires_grad_(True)                # the route a call of this size takes when nobody names one: the packed one
    assert torch.equal(model._encode_image_eager(x).detach(), res[0][0])
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    ee, eg, e0 = rel(res[0][0], res[1][0]), rel(res[0][1], res[1][1]), rel(res[0][2], res[1][2])
    print("fused blocks vs per-kernel autograd: embedding", ee, "pixel gradient", eg, "no-grad embedding", e0)
    assert torch.isfinite(res[0][1]).all()
    assert ee < 4e-3 and e0 < 4e-3 and eg < 1e-2, (ee, e0, eg)
    xr = img.cpu().clone().requires_grad_(True)
    ref = C.encode_image(C.random_state_dict(0), xr)
    (1 - torch.cosine_similarity(ref.mean(0), text.cpu().mean(0), dim=0)).backward()
    err = [(rel(r[0].cpu(), ref.detach()), rel(r[1].cpu(), xr.grad)) for r in res]
    print("vs the fp32 oracle (embedding, pixel gradient): fused", err[0], "per-kernel", err[1])
    assert err[0][0] < 1.25 * err[1][0] and err[0][1] < 1.25 * err[1][1], err
    assert torch.equal(res[0][0], res[0][2])        # the no-grad call runs the same launches


@gpu
def test_layernorm_backward_and_packed_epilogues_of_the_training_pipeline():
    """avc_vit_ln_bwd against torch autograd of F.layer_norm (+ residual gradient), its packed output and the packed / QuickGELU'
    epilogues of avc_vit_linear_packed against avc_vit_pack of the fp32 result (bit-exact: the same values rounded once), on both sides
    of its 128-row dispatch: 128 rows = the last row count of the latency kernel, 129 = the first of the GEMM (5 row tiles: a ragged
    group of four), 160 = two whole tiles in a partial group.  Each side of a torch.equal runs the same kernel at that M."""
    from avatarclip_amd import clip_vit as V, lib as L
    lib, dev = L.load(), torch.device("cuda")
    g = torch.Generator().manual_seed(3)
    for M in (50, 100):
        x = torch.randn(M, 768, generator=g).to(dev) * 2 + 0.3
        dy = torch.randn(M, 768, generator=g).to(dev)
        res = torch.randn(M, 768, generator=g).to(dev)
        gamma = (torch.randn(768, generator=g) * 0.2 + 1).to(dev)
        beta = torch.randn(768, generator=g).to(dev)
        xr = x.clone().requires_grad_(True)
        torch.nn.functional.layer_norm(xr, (768,), gamma, beta, 1e-5).backward(dy)
        ref = xr.grad + res
        dx = torch.empty_like(x)
        nb = lib.avc_vit_workspace_bytes(M, 768)
        ps, ps_ref = torch.zeros(nb, dtype=torch.uint8, device=dev), torch.zeros(nb, dtype=torch.uint8, device=dev)
        L.check(lib.avc_vit_ln_bwd(L.ptr(dy), L.ptr(x), L.ptr(gamma), 1e-5, L.ptr(res), L.ptr(dx), L.ptr(ps), M, 768, L.stream()), "ln_bwd")
        assert torch.allclose(dx, ref, atol=2e-5, rtol=2e-5), (dx - ref).abs().max()
        L.check(lib.avc_vit_pack(L.ptr(dx), None, L.ptr(ps_ref), M, 768, L.stream()), "pack")
        used = ((M + 31) // 32) * 48 * 1024
        assert torch.equal(ps[:used], ps_ref[:used])
        # linear: fp32 rows + packed copy; QuickGELU forward (pre + packed activation); QuickGELU' backward epilogue
        w = torch.randn(3072, 768, generator=g) * 768 ** -0.5
        b = (torch.randn(3072, generator=g) * 0.1).to(dev)
        lin = V._Lin(w, b.cpu(), dev)
        L.check(lib.avc_vit_pack(L.ptr(x), None, L.ptr(ps), M, 768, L.stream()), "pack")
        y, pre = torch.empty(M, 3072, device=dev), torch.empty(M, 3072, device=dev)
        nb2 = lib.avc_vit_workspace_bytes(M, 3072)
        py, py_ref = torch.zeros(nb2, dtype=torch.uint8, device=dev), torch.zeros(nb2, dtype=torch.uint8, device=dev)
        L.check(lib.avc_vit_linear_packed(L.ptr(ps), L.ptr(lin.wp), L.ptr(b), None, None, L.ptr(y), L.ptr(pre), L.ptr(py), M, 3072, 768, 1,
                                          L.stream()), "linear_packed")
        y_ref = V.LinearFn.apply(x, lin, 1, None)
        assert torch.equal(y, y_ref)
        L.check(lib.avc_vit_pack(L.ptr(y), None, L.ptr(py_ref), M, 3072, L.stream()), "pack")
        used2 = ((M + 31) // 32) * 192 * 1024
        assert torch.equal(py[:used2], py_ref[:used2])
        # act 2: (x W^T) * QuickGELU'(pre), packed only
        L.check(lib.avc_vit_linear_packed(L.ptr(ps), L.ptr(lin.wp), None, None, L.ptr(pre), None, None, L.ptr(py), M, 3072, 768, 2,
                                          L.stream()), "linear_packed")
        L.check(lib.avc_vit_linear_packed(L.ptr(ps), L.ptr(lin.wp), None, None, None, L.ptr(y), None, None, M, 3072, 768, 0, L.stream()),
                "linear_packed")
        L.check(lib.avc_vit_pack(L.ptr(y), L.ptr(pre), L.ptr(py_ref), M, 3072, L.stream()), "pack")
        assert torch.equal(py[:used2], py_ref[:used2])
    assert lib.avc_vit_linear_packed(L.ptr(ps), L.ptr(lin.wp), None, None, None, None, None, None, 100, 3072, 768, 0, L.stream()) != 0
    # the 128-row dispatch of the merged entry, N = K = 768: fp32 rows == LinearFn on the fp32 operand (identity, QuickGELU, residual),
    # and the packed output == avc_vit_pack of those rows.  Up to 128 rows whole tiles are compared (the latency kernel writes the
    # rows past M as zeros); the GEMM leaves f(bias) in the rows past M, which no valid row ever reads, so there the M valid rows are
    # compared, every element of them.
    def rows(packed, M, N):          # [row tile][k-step][half][row][8] -> [M, N]
        mt = (M + 31) // 32
        t = packed[:mt * (N // 16) * 1024].view(torch.bfloat16).reshape(mt, N // 16, 2, 32, 8)
        return t.permute(0, 3, 1, 2, 4).reshape(mt * 32, N)[:M]
    w = torch.randn(768, 768, generator=g) * 768 ** -0.5
    b = (torch.randn(768, generator=g) * 0.1).to(dev)
    lin = V._Lin(w, b.cpu(), dev)
    for M in (128, 129, 160):
        x = torch.randn(M, 768, generator=g).to(dev)
        res = torch.randn(M, 768, generator=g).to(dev)
        nb = lib.avc_vit_workspace_bytes(M, 768)
        ps, py, py_ref = (torch.zeros(nb, dtype=torch.uint8, device=dev) for _ in range(3))
        L.check(lib.avc_vit_pack(L.ptr(x), None, L.ptr(ps), M, 768, L.stream()), "pack")
        for act, r in ((0, None), (1, None), (0, res)):
            y = torch.empty(M, 768, device=dev)
            L.check(lib.avc_vit_linear_packed(L.ptr(ps), L.ptr(lin.wp), L.ptr(b), L.ptr(r), None, L.ptr(y), None, None, M, 768, 768, act,
                                              L.stream()), "linear_packed")
            assert torch.equal(y, V.LinearFn.apply(x, lin, act, r)), (M, act)
            if r is None:
                L.check(lib.avc_vit_linear_packed(L.ptr(ps), L.ptr(lin.wp), L.ptr(b), None, None, None, None, L.ptr(py), M, 768, 768, act,
                                                  L.stream()), "linear_packed")
                py_ref.zero_()
                L.check(lib.avc_vit_pack(L.ptr(y), None, L.ptr(py_ref), M, 768, L.stream()), "pack")
                assert torch.equal(rows(py, M, 768).view(torch.int16), rows(py_ref, M, 768).view(torch.int16)), (M, act)
                assert torch.equal(rows(py_ref, M, 768).float(), y.bfloat16().float())     # (the helper reads the layout right)
                if M <= 128:
                    used = ((M + 31) // 32) * 48 * 1024
                    assert torch.equal(py[:used], py_ref[:used]), (M, act)
    # host-side refusals above 128 rows (no launch): QuickGELU with a residual; a column count the GEMM does not cover
    assert lib.avc_vit_linear_packed(L.ptr(ps), L.ptr(lin.wp), L.ptr(b), L.ptr(res), None, L.ptr(y), None, None, 129, 768, 768, 1, L.stream()) != 0
    assert lib.avc_vit_linear_packed(L.ptr(ps), L.ptr(lin.wp), L.ptr(b), None, None, L.ptr(y), None, None, 129, 96, 768, 0, L.stream()) != 0
    # attention backward with its result packed for the transposed in-projection == packing of its fp32 result
    for B in (1, 2):
        M = 50 * B
        qkv = torch.randn(B, 50, 2304, generator=g).to(dev)
        do = torch.randn(B, 50, 768, generator=g).to(dev)
        dq = torch.empty_like(qkv)
        nb3 = lib.avc_vit_workspace_bytes(M, 2304)
        pa, pb = torch.zeros(nb3, dtype=torch.uint8, device=dev), torch.zeros(nb3, dtype=torch.uint8, device=dev)
        L.check(lib.avc_vit_attention_bwd(L.ptr(qkv), L.ptr(do), L.ptr(dq), B, 50, 768, 12, L.stream()), "attention_bwd")
        L.check(lib.avc_vit_pack(L.ptr(dq), None, L.ptr(pa), M, 2304, L.stream()), "pack")
        L.check(lib.avc_vit_attention_bwd_packed(L.ptr(qkv), L.ptr(do), L.ptr(pb), B, 50, 768, 12, L.stream()), "attention_bwd_packed")
        used3 = ((M + 31) // 32) * 144 * 1024
        assert torch.equal(pa[:used3], pb[:used3])


@gpu
def test_two_calls_before_one_backward_do_not_share_the_captured_instance(monkeypatch):
    """The reference's own pattern with add_no_texture (main.py:512 then :524: two encode_image calls of one image each, ONE
    loss.backward()): a captured HIP graph has one set of static activations and one static output, so the second call must not go
    through the instance that is still waiting for its backward.  Embeddings and pixel gradients of both calls equal the eager
    launches bit for bit; a later scoring call that needs a larger packing workspace must not free the one the graphs write into;
    after the backward the instance is free again."""
    from avatarclip_amd import clip_vit as V
    dev = torch.device("cuda")
    model = V.ClipVisionB32(C.random_state_dict(0), dev)
    text = torch.randn(1, 512, generator=torch.Generator().manual_seed(5)).to(dev)
    imgs = [torch.randn(1, 3, 224, 224, generator=torch.Generator().manual_seed(20 + k)).to(dev) for k in range(2)]
    res = {}
    for graph in (True, False):
        monkeypatch.setattr(V, "TRAIN_GRAPH", graph)
        for rnd in range(2):
            xs = [im.clone().requires_grad_(True) for im in imgs]
            es = [model.encode_image(x) for x in xs]
            if graph:
                assert model._graph_busy.get(1) is True           # the first call holds the instance, the second ran eagerly
            loss = sum(1 - torch.cosine_similarity(e.mean(0), text.mean(0), dim=0) for e in es)
            loss.backward()
            if graph:
                assert model._graph_busy.get(1) is False
                if rnd == 0:
                    with torch.no_grad():                         # 8 images: the packed scoring pipeline; the eager linears of a
                        model.encode_image(torch.randn(8, 3, 224, 224, device=dev))     # 4-image gradient call grow the workspace
                    big = torch.randn(4, 3, 224, 224, device=dev, requires_grad=True)
                    model.encode_image(big).sum().backward()
            res[(graph, rnd)] = ([e.detach().clone() for e in es], [x.grad.clone() for x in xs])
    for rnd in range(2):
        for k in range(2):
            assert torch.equal(res[(True, rnd)][0][k], res[(False, rnd)][0][k]), (rnd, k)
            assert torch.equal(res[(True, rnd)][1][k], res[(False, rnd)][1][k]), (rnd, k)
    assert not torch.equal(res[(True, 0)][0][0], res[(True, 0)][0][1])
    # a loss held ACROSS release_graphs() and a later replay: its backward would differentiate the newer call's captured
    # activations -- it must raise instead of returning wrong pixel gradients; the newer call's own backward is unaffected
    monkeypatch.setattr(V, "TRAIN_GRAPH", True)
    x_old, x_new = imgs[0].clone().requires_grad_(True), imgs[1].clone().requires_grad_(True)
    held = model.encode_image(x_old).sum()
    model.release_graphs()
    newer = model.encode_image(x_new)
    assert model._graph_gen[1] >= 2
    with pytest.raises(RuntimeError, match="release_graphs"):
        held.backward()
    (1 - torch.cosine_similarity(newer.mean(0), text.mean(0), dim=0)).backward()
    assert torch.equal(x_new.grad, res[(False, 0)][1][1]) and model._graph_busy.get(1) is False


@gpu
def test_encode_image_matches_oracle():
    from avatarclip_amd import clip_vit as V
    dev = torch.device("cuda")
    sd = C.random_state_dict(0)
    model = V.ClipVisionB32(sd, dev)
    g = torch.Generator().manual_seed(1)
    img = torch.randn(2, 3, 224, 224, generator=g)
    text = torch.randn(1, 512, generator=g)
    xd = img.to(dev).requires_grad_(True)
    emb = model.encode_image(xd)
    cos = torch.cosine_similarity(emb.mean(0), text.to(dev).mean(0), dim=0)
    cos.backward()
    xr = img.clone().requires_grad_(True)
    ref = C.encode_image(sd, xr)
    cos_r = torch.cosine_similarity(ref.mean(0), text.mean(0), dim=0)
    cos_r.backward()
    sim = torch.cosine_similarity(emb.detach().cpu(), ref.detach(), dim=-1)
    rel = (xd.grad.cpu() - xr.grad).norm() / xr.grad.norm()
    print("embedding cosine", sim.tolist(), "cos(emb,text)", cos.item(), cos_r.item(), "pixel-grad rel err", rel.item())
    assert sim.min() > 0.9995
    assert abs(cos.item() - cos_r.item()) < 1e-3
    assert rel < 3e-2


@gpu
@pytest.mark.parametrize("variant", ["channels", "ln4", "ln30"])
def test_encode_image_with_outlier_channels_matches_oracle(variant):
    """trained CLIP ViTs carry a handful of residual channels / c_fc rows tens of times above the median, which
    the N(0, sigma) weights of the test above do not.  Same comparison on oracle/clip_vit_oracle.outlier_state_dict:
      channels: 8 residual channels x 30 (class / CLS-position embedding, ln_pre gain: massive CLS-token channels that persist
                through all blocks), 4 c_fc rows x 20 per block -> the tolerances of the seeded test hold unchanged;
      ln4     : additionally ALL 24 block LayerNorm gains x 4 on those channels.  Rounding the linear operands to bf16 ON THE CPU
                moves the pixel gradient of this network by 2.8 % (encode_image_bf16_operands vs fp32; 0.5 % without the gains):
                still a well-conditioned map, so the kernel's gradient is asserted against BOTH statements -- within 6 % of fp32
                (twice what bf16 operands alone do) and within 5 % of the CPU bf16-operand statement;
      ln30    : the gains x 30.  The untrained network is then chaotic in its input -- a SINGLE block with such gains already moves
                the CPU bf16-operand gradient by 64 % against fp32 (all twelve: 430 %) while the embedding moves by 3e-4 -- so no
                statement about the gradient can be tested there and none is made: only the forward quantities the loss uses
                (embedding, cos(emb, text)) are asserted, the gradient numbers are printed.
    The bounds are stated in DESIGN.md section 2 (main.py:259,512)."""
    from avatarclip_amd import clip_vit as V
    dev = torch.device("cuda")
    sd = C.outlier_state_dict(0, ln_blocks=() if variant == "channels" else range(12), ln_gain=4.0 if variant == "ln4" else None)
    model = V.ClipVisionB32(sd, dev)
    g = torch.Generator().manual_seed(1)
    img = torch.randn(2, 3, 224, 224, generator=g)
    text = torch.randn(1, 512, generator=g)

    def leg(fn, x):
        x = x.clone().requires_grad_(True)
        e = fn(x)
        c = torch.cosine_similarity(e.mean(0), text.to(e.device).mean(0), dim=0)
        c.backward()
        return e.detach().float().cpu(), c.item(), x.grad.detach().float().cpu()
    emb, cos, gx = leg(model.encode_image, img.to(dev))
    ref, cos_r, gr = leg(lambda x: C.encode_image(sd, x), img)
    emq, cos_q, gq = leg(lambda x: C.encode_image_bf16_operands(sd, x), img)
    sim = torch.cosine_similarity(emb, ref, dim=-1).min().item()
    rel = ((gx - gr).norm() / gr.norm()).item()
    rel_q = ((gq - gr).norm() / gr.norm()).item()          # what bf16 operands alone do to this network (CPU, fp32 accumulate)
    rel_kq = ((gx - gq).norm() / gq.norm()).item()         # the kernel against that CPU statement
    print("OUTLIER %s  embedding cosine %.6f (cpu bf16-operand restatement %.6f)  |d cos| %.2e (%.2e)  pixel-grad rel err vs fp32 %.3e "
          "(cpu bf16 operands vs fp32 %.3e, kernel vs cpu bf16 operands %.3e)"
          % (variant, sim, torch.cosine_similarity(emq, ref, dim=-1).min().item(), abs(cos - cos_r), abs(cos_q - cos_r), rel, rel_q, rel_kq))
    assert torch.isfinite(emb).all() and torch.isfinite(gx).all()
    if variant == "channels":
        assert sim > 0.9995 and abs(cos - cos_r) < 1e-3 and rel < 3e-2
    elif variant == "ln4":
        assert sim > 0.9995 and abs(cos - cos_r) < 1e-3
        assert rel_q < 4e-2, "the CPU statement itself: this variant is supposed to be well conditioned"
        assert rel < 6e-2 and rel_kq < 5e-2
    else:
        assert sim > 0.999 and abs(cos - cos_r) < 2e-3


def _full_state_dict():
    from oracle import clip_text_oracle as T
    sd = dict(C.random_state_dict(0))
    sd.update(T.random_state_dict(1))
    return sd


def test_checkpoint_file_formats_load_to_the_same_state_dict(tmp_path):
    """clip_vit.load_state_dict (the $AVC_CLIP_WEIGHTS / clip.weights hook): a torch.save()d state dict, a .safetensors file and a
    TorchScript archive (the format of OpenAI's ViT-B-32.pt) all give back the tensors that went in"""
    from safetensors.torch import save_file
    from avatarclip_amd import clip_vit as V
    sd = {k: v for k, v in _full_state_dict().items() if k.startswith("visual.ln_") or k.startswith("ln_final") or k == "logit_scale"
          or k.endswith("resblocks.0.ln_1.weight")}
    assert len(sd) >= 4
    torch.save(sd, tmp_path / "w.pt")
    save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "w.safetensors"))

    class Holder(torch.nn.Module):          # a scripted module whose state dict carries the same names
        def __init__(self):
            super().__init__()
            for i, (k, v) in enumerate(sorted(sd.items())):
                self.register_buffer("b%d" % i, v.clone())

        def forward(self, x):
            return x
    torch.jit.script(Holder()).save(str(tmp_path / "w_script.pt"))
    a = V.load_state_dict(str(tmp_path / "w.pt"))
    b = V.load_state_dict(str(tmp_path / "w.safetensors"))
    c = V.load_state_dict(str(tmp_path / "w_script.pt"))
    assert set(a) == set(b) == set(sd)
    for k in sd:
        assert torch.equal(a[k], sd[k]) and torch.equal(b[k], sd[k])
    assert len(c) == len(sd) and all(torch.equal(c["b%d" % i], v) for i, (k, v) in enumerate(sorted(sd.items())))


@gpu
def test_runner_takes_clip_weights_from_a_checkpoint_file_without_standins(tmp_path, monkeypatch):
    """main.py:258-259 (`clip.load('ViT-B/32')`): with $AVC_CLIP_WEIGHTS pointing at a checkpoint the Runner needs no stand-in for
    the perceptor (allow_standins = False would raise otherwise) and its image embeddings are the oracle's on that state dict"""
    import bench
    from avatarclip_amd.runner import Runner
    sd = _full_state_dict()
    torch.save(sd, tmp_path / "ViT-B-32.pt")
    monkeypatch.setenv("AVC_CLIP_WEIGHTS", str(tmp_path / "ViT-B-32.pt"))
    conf = bench.make_conf(32, 32, small=True)
    conf.put("general.allow_standins", False)
    runner = Runner(None, mode="train_clip", conf=conf, device=torch.device("cuda"))
    g = torch.Generator().manual_seed(3)
    te = {k: torch.nn.functional.normalize(torch.randn(1, 512, generator=g), dim=-1) for k in ("prompt", "face_prompt", "back_prompt")}
    runner.init_clip(text_embeddings=te)              # prompts cached; the perceptor comes from the file
    img = torch.rand(1, 3, 224, 224, generator=g)
    emb = runner.perceptor.encode_image(img.cuda()).float().cpu()
    ref = C.encode_image(sd, img)
    assert torch.cosine_similarity(emb, ref, dim=-1).min() > 0.9995
    # without the file and without permission for stand-ins the set-up must refuse
    monkeypatch.delenv("AVC_CLIP_WEIGHTS")
    runner2 = Runner(None, mode="train_clip", conf=conf, device=torch.device("cuda"))
    with pytest.raises(RuntimeError):
        runner2.init_clip(text_embeddings=te)


@gpu
def test_real_openai_weights_when_supplied(tmp_path):
    """Where the licensed artefacts exist: $AVC_CLIP_WEIGHTS = OpenAI's ViT-B-32.pt (or a state-dict / safetensors copy) and $AVC_CLIP_BPE =
    bpe_simple_vocab_16e6.txt.gz.  HIP encoders vs the fp32 oracle ON THE REAL WEIGHTS (the seeded-weight tests above cannot show the
    dynamic range of trained weights), and the tokenizer against the known ids of CLIP's README example.  Without $AVC_CLIP_WEIGHTS the
    same checks run on a checkpoint file written here -- the offline proxy for trained weights' dynamic range (clip_vit_oracle.
    outlier_state_dict) plus a seeded text tower, loaded through the same file path -- the text tower on fixed token ids."""
    import os
    from oracle import clip_text_oracle as T
    from avatarclip_amd import clip_vit as V
    wpath, bpath = os.environ.get("AVC_CLIP_WEIGHTS"), os.environ.get("AVC_CLIP_BPE")
    real = bool(wpath) and os.path.exists(wpath)
    if not real:
        import warnings
        warnings.warn(UserWarning("$AVC_CLIP_WEIGHTS not set: the HIP towers were checked on the outlier-proxy checkpoint, not on OpenAI's "
                                  "weights (parity on the real weights stays unpinned)"))
        seeded = dict(C.outlier_state_dict(0))
        seeded.update(T.random_state_dict(0))
        wpath = str(tmp_path / "clip_seeded.pt")
        torch.save(seeded, wpath)
    sd = {k: v.float() for k, v in V.load_state_dict(wpath).items()}
    model = V.ClipVisionB32(sd, torch.device("cuda"))
    g = torch.Generator().manual_seed(5)
    img = torch.randn(2, 3, 224, 224, generator=g)
    emb = model.encode_image(img.cuda()).float().cpu()
    ref = C.encode_image(sd, img)
    assert torch.cosine_similarity(emb, ref, dim=-1).min() > 0.999
    if not real:
        tok = torch.zeros(2, 77, dtype=torch.long)
        for i, n in enumerate((5, 12)):                  # <start>, n word ids, <end>, padding
            tok[i, 0], tok[i, n + 1] = 49406, 49407
            tok[i, 1:n + 1] = torch.randint(1, 49406, (n,), generator=g)
        out = model.encode_text(tok).float().cpu()
        assert torch.cosine_similarity(out, T.encode_text(sd, tok), dim=-1).min() > 0.999
        return
    if bpath and os.path.exists(bpath):
        from avatarclip_amd import tokenizer as TK
        tk = TK.SimpleTokenizer(bpath)
        tok = TK.tokenize(["a diagram", "a 3D rendering of the Iron Man in unreal engine"], tk)
        assert tok[0, 0].item() == 49406 and tok[0, 1].item() == 320 and tok[0, 3].item() == 49407 and tok[0, 4:].sum().item() == 0
        out = model.encode_text(tok).float().cpu()
        ref_t = T.encode_text(sd, tok)
        assert torch.cosine_similarity(out, ref_t, dim=-1).min() > 0.999
        # a render prompt and an unrelated one must be told apart by the joint embedding the way CLIP does it: cos in (-1, 1), finite
        cs = torch.cosine_similarity(out[0], out[1], dim=0)
        assert torch.isfinite(cs) and cs < 0.99


@gpu
def test_batched_scoring_path_matches_the_per_pair_path():
    """row f-4 (ShapeGen codebook search / pose retrieval: hundreds of renders per encode_image call): above 128 token rows the
    linears run in the LDS-staged GEMM (csrc/avc_vit_gemm.hip); the embeddings must agree with the M <= 128 latency-kernel path image by
    image, and with the oracle"""
    from avatarclip_amd import clip_vit as V
    sd = C.random_state_dict(0)
    model = V.ClipVisionB32(sd, torch.device("cuda"))
    g = torch.Generator().manual_seed(7)
    img = torch.randn(12, 3, 224, 224, generator=g)          # 12 x 50 = 600 token rows: the batched kernel (> 128 rows)
    assert 12 * V.TOKENS >= V.BIG_M
    big = model.encode_image(img.cuda()).float().cpu()
    small = torch.cat([model.encode_image(img[i:i + 2].cuda()).float().cpu() for i in range(0, 12, 2)])
    ref = C.encode_image(sd, img[:4])
    assert torch.cosine_similarity(big, small, dim=-1).min() > 0.9999
    assert torch.cosine_similarity(big[:4], ref, dim=-1).min() > 0.9995
    # gradient to the pixels through the batched path
    x = img[:12].cuda().requires_grad_(True)
    model.encode_image(x).square().sum().backward()
    assert torch.isfinite(x.grad).all() and x.grad.abs().max() > 0
