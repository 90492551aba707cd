"""CLIP ViT-B/16 on the GPU: the tiled attention kernels (every T in [1, 256] but 50; avc_vit_attn.hip) through the four attention entry
points, and the image tower at 197 tokens (clip_vit.ClipVision on a patch-16 state dict) on each of its routes, against
oracle/clip_vit_oracle.py with its PATCH / TOKENS globals set to 16 / 197 (pinned against transformers at patch 16 in
test_clip_b16_cpu.py).  Bounds are those of the ViT-B/32 tests in test_gpu_clip.py / test_gpu_iteration.py, named at each use.

Measured on an MI355X.  Kernels against fp32 attention (bounds 1e-2 / 2e-2): forward 1.6e-3 (T = 1), 3.2e-3 .. 3.5e-3 (every other T),
gradient 1.6e-3 (T = 1), 3.6e-3 .. 3.9e-3; against the restatement (bound 2e-3): <= 3.6e-4 forward, <= 4.3e-4 gradient.  encode_image
against the oracle: embedding cosine 0.999995, |d cos| 9e-6, pixel gradient 8.4e-3.  Packed against per-kernel route: cosine 0.9999972,
relative difference 2.4e-3 (B = 1 and 3).  The iteration: loss 11.29215 / 11.29150, worst per-tensor gradient error 1.1e-2.
"""
import functools

import pytest
import torch

from oracle import clip_vit_oracle as C

gpu = pytest.mark.gpu


def _b16(monkeypatch):
    monkeypatch.setattr(C, "PATCH", 16)
    monkeypatch.setattr(C, "TOKENS", 197)


# ---------------------------------------------------------------------------------------------------------------- the kernels
@functools.lru_cache(maxsize=None)
def _case(B, heads, T):
    """inputs, the fp32 torch attention and its gradient, and the kernels' arithmetic restated in torch with the operands rounded where
    the header of the tiled kernels says (q / 8, k, v, dO when read; P after normalisation; dS once, dQ's copy after the scaling)"""
    W = 64 * heads
    g = torch.Generator().manual_seed(1000 * B + 10 * heads + T)
    qkv = torch.randn(B, T, 3 * W, generator=g)
    do = torch.randn(B, T, W, generator=g)
    sh = lambda t: t.reshape(B, T, heads, 64).permute(0, 2, 1, 3)
    un = lambda t: t.permute(0, 2, 1, 3).reshape(B, T, W)
    bf = lambda t: t.bfloat16().float()
    qr = qkv.clone().requires_grad_(True)
    q, k, v = qr.split(W, dim=-1)
    ref = un(torch.softmax(sh(q) @ sh(k).transpose(-1, -2) / 8.0, dim=-1) @ sh(v))
    (ref * do).sum().backward()
    with torch.no_grad():
        q, k, v = (sh(t) for t in qkv.split(W, dim=-1))
        qs, kb, vb, dob = bf(q * 0.125), bf(k), bf(v), bf(sh(do))
        P = torch.softmax(qs @ kb.transpose(-1, -2), dim=-1)
        o_b = un(bf(P) @ vb)
        dP = dob @ vb.transpose(-1, -2)
        dS = P * (dP - (P * dP).sum(-1, keepdim=True))
        dq, dk, dv = bf(dS * 0.125) @ kb, bf(dS).transpose(-1, -2) @ qs, bf(P).transpose(-1, -2) @ dob
        g_b = torch.cat([un(dq), un(dk), un(dv)], dim=-1)
    return qkv, do, ref.detach(), qr.grad, o_b, g_b


def _kernels(qkv, do):
    """forward and backward through AttentionFn (fp32 rows) -> out, dqkv on the device"""
    from avatarclip_amd import clip_vit as V
    qd = qkv.cuda().requires_grad_(True)
    out = V.AttentionFn.apply(qd)
    out.backward(do.cuda())
    return out.detach(), qd.grad


GRID = [(2, 2, T) for T in (1, 32, 33, 49, 64, 65, 197, 224, 256)] + [(3, 12, 197)]


@gpu
@pytest.mark.parametrize("B, heads, T", GRID)
def test_tiled_attention_forward_and_backward_at_every_class_of_T(B, heads, T):
    """one key tile (1, 32), a ragged second one (33, 49), two and three (64, 65), ViT-B/16's 197 = 6 x 32 + 5, 224 = 7 tiles, the
    largest T; two query workgroups in the forward from T = 129.  (a) against fp32 attention: relative L2 <= 1e-2 forward, 2e-2 gradient
    (the bounds test_vit_linear_and_attention_kernels holds T = 50 to); (b) against the restated arithmetic: atol = rtol = 2e-3."""
    qkv, do, ref, gref, o_b, g_b = _case(B, heads, T)
    out, grad = _kernels(qkv, do)
    out, grad = out.cpu(), grad.cpu()
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    e_out, e_grad = rel(out, ref), rel(grad, gref)
    print("B %d heads %d T %3d  vs fp32: forward rel %.3e gradient rel %.3e   vs restatement: max |diff| %.3e / %.3e"
          % (B, heads, T, e_out, e_grad, (out - o_b).abs().max().item(), (grad - g_b).abs().max().item()))
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    assert e_out < 1e-2 and e_grad < 2e-2, (e_out, e_grad)
    assert torch.allclose(out, o_b, atol=2e-3, rtol=2e-3), (out - o_b).abs().max()
    assert torch.allclose(grad, g_b, atol=2e-3, rtol=2e-3), (grad - g_b).abs().max()


@gpu
@pytest.mark.parametrize("T", [0, 257])
def test_token_counts_outside_the_range_are_refused_before_anything_is_launched(T):
    from avatarclip_amd import lib as L
    dev = torch.device("cuda")
    B, heads, W = 1, 2, 128
    rows = max(T, 1)
    qkv = torch.randn(B, rows, 3 * W, device=dev)
    do = torch.randn(B, rows, W, device=dev)
    out = torch.full((B, rows, W), -7.0, device=dev)
    dqkv = torch.full((B, rows, 3 * W), -7.0, device=dev)
    packed = torch.full((L.load().avc_vit_workspace_bytes(B * rows, 3 * W),), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for name, args in (("avc_vit_attention_fwd", (qkv, out)), ("avc_vit_attention_fwd_packed", (qkv, packed)),
                       ("avc_vit_attention_bwd", (qkv, do, dqkv)), ("avc_vit_attention_bwd_packed", (qkv, do, packed))):
        with pytest.raises(RuntimeError) as e:
            L.call(name, *args, B, T, W, heads)
        assert "1 <= T <= 256" in str(e.value) and "50 tokens" not in str(e.value), str(e.value)
        assert torch.cuda.current_stream().query()           # nothing was enqueued
    # ... and a head dim other than 64
    with pytest.raises(RuntimeError) as e:
        L.call("avc_vit_attention_fwd", qkv, out, B, 197, W, 4)
    assert "head dim 64" in str(e.value)
    assert torch.cuda.current_stream().query()
    assert (out == -7.0).all() and (dqkv == -7.0).all() and (packed == 0x5A).all()


@gpu
@pytest.mark.parametrize("T", [197, 33])
def test_nothing_outside_the_rows_of_the_call_is_read_or_written(T):
    """qkv / dout as leading views of allocations whose remainder is NaN, the outputs as leading views of sentinel-filled ones: the
    results are finite, the bits of the run on stand-alone tensors, and the sentinel behind the outputs is intact"""
    from avatarclip_amd import lib as L
    B, heads = 2, 2
    W = 64 * heads
    qkv, do = _case(B, heads, T)[:2]
    out_ref, grad_ref = _kernels(qkv, do)
    dev = torch.device("cuda")
    extra = 3 * W * 40 + 24           # 40 more rows and a ragged tail behind the call's rows

    def lead(t, fill):
        big = torch.full((t.numel() + extra,), fill, device=dev)
        view = big[: t.numel()].view(t.shape)
        return big, view
    qb, qv = lead(qkv, float("nan"))
    db, dv = lead(do, float("nan"))
    qv.copy_(qkv)
    dv.copy_(do)
    ob, ov = lead(do, -7.0)
    gb, gv = lead(qkv, -7.0)
    L.call("avc_vit_attention_fwd", qv, ov, B, T, W, heads)
    L.call("avc_vit_attention_bwd", qv, dv, gv, B, T, W, heads)
    assert torch.isfinite(ov).all() and torch.isfinite(gv).all()
    assert torch.equal(ov, out_ref) and torch.equal(gv, grad_ref)
    assert (ob[do.numel():] == -7.0).all() and (gb[qkv.numel():] == -7.0).all()
    assert torch.isnan(qb[qkv.numel():]).all() and torch.isnan(db[do.numel():]).all()


def _unpack(packed_u8, M, K):
    """[Mpad, K] bf16 from a packed operand: element (row, col) = slot col & 7 of lane (row & 31, (col >> 3) & 1) of k-step col >> 4 of
    row tile row >> 5 (the formula in front of put_packed_elem, avc_vit_attn.hip)"""
    flat = packed_u8.view(torch.bfloat16)
    Mpad = 32 * ((M + 31) // 32)
    row = torch.arange(Mpad, device=flat.device).view(-1, 1)
    col = torch.arange(K, device=flat.device).view(1, -1)
    idx = (((row >> 5) * (K >> 4) + (col >> 4)) * 64 + (row & 31) + 32 * ((col >> 3) & 1)) * 8 + (col & 7)
    return flat[idx]


@gpu
@pytest.mark.parametrize("B", [1, 3])
def test_packed_forms_hold_the_row_form_rounded_to_bf16_and_leave_the_lanes_past_the_last_row(B):
    from avatarclip_amd import lib as L
    heads, T = 12, 197
    W, M = 64 * heads, B * T
    qkv, do = _case(3, heads, T)[:2]
    qkv, do = qkv[:B].contiguous(), do[:B].contiguous()
    out, grad = _kernels(qkv, do)
    dev = torch.device("cuda")
    bits = lambda t: t.contiguous().view(torch.int16)
    for name, args, K, rows in (("avc_vit_attention_fwd_packed", (qkv.to(dev),), W, out),
                                ("avc_vit_attention_bwd_packed", (qkv.to(dev), do.to(dev)), 3 * W, grad)):
        packed = torch.full((L.load().avc_vit_workspace_bytes(M, K),), 0x5A, dtype=torch.uint8, device=dev)
        L.call(name, *args, packed, B, T, W, heads)
        un = _unpack(packed, M, K)
        assert M % 32 != 0 and un.shape[0] > M
        assert torch.equal(bits(un[:M]), bits(rows.reshape(M, K).bfloat16())), name
        assert (bits(un[M:]) == 0x5A5A).all(), name               # rows >= B * T of the last row tile keep the caller's fill
        # ... and so does everything behind the last row tile
        assert (packed[un.shape[0] * K * 2:] == 0x5A).all(), name


@gpu
def test_tiled_attention_is_the_same_bits_in_every_run_and_at_every_place_in_a_batch():
    qkv, do = _case(3, 12, 197)[:2]
    out, grad = _kernels(qkv, do)
    out2, grad2 = _kernels(qkv, do)
    assert torch.equal(out, out2) and torch.equal(grad, grad2)
    for b in range(3):
        o1, g1 = _kernels(qkv[b:b + 1].contiguous(), do[b:b + 1].contiguous())
        assert torch.equal(o1[0], out[b]) and torch.equal(g1[0], grad[b]), b


# ---------------------------------------------------------------------------------------------------------------- the tower
_cache = {}


def _sd16():
    """the oracle's seeded ViT-B/16 weights (call under _b16)"""
    assert C.PATCH == 16 and C.TOKENS == 197
    if "sd" not in _cache:
        _cache["sd"] = C.random_state_dict(0)
    return _cache["sd"]


def _scoring_case():
    """three images and their oracle embeddings (call under _b16): shared by the B = 1 and B = 3 cases of the packed route"""
    if "score" not in _cache:
        img = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(3))
        with torch.no_grad():
            _cache["score"] = (img, C.encode_image(_sd16(), img))
    return _cache["score"]


@gpu
def test_encode_image_b16_matches_the_oracle(monkeypatch):
    """test_encode_image_matches_oracle at patch 16 / 197 tokens, with its bounds.  Two images with a gradient are 394 rows: the
    per-kernel route, AttentionFn on the tiled kernels forward and backward."""
    from avatarclip_amd import clip_vit as V
    _b16(monkeypatch)
    dev = torch.device("cuda")
    sd = _sd16()
    model = V.ClipVision(sd, dev)
    assert (model.patch, model.tokens) == (16, 197)
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
    print("B/16 embedding cosine", sim.tolist(), "cos(emb,text)", cos.item(), cos_r.item(), "pixel-grad rel err", rel.item())
    assert sim.min() > 0.9995
    assert abs(cos.item() - cos_r.item()) < 1e-3
    assert rel < 3e-2


@gpu
@pytest.mark.parametrize("B", [1, 3])
def test_b16_scoring_route_matches_the_per_kernel_route_and_the_oracle(B, monkeypatch):
    """test_batched_scoring_pipeline_matches_the_autograd_path_and_the_oracle at 197 tokens: one image is already 197 rows, the smallest
    call on the GEMM route (avc_vit_attention_fwd_packed at T = 197)."""
    from avatarclip_amd import clip_vit as V
    _b16(monkeypatch)
    dev = torch.device("cuda")
    model = V.ClipVision(_sd16(), dev)
    img, ref = _scoring_case()
    img, ref = img[:B], ref[:B]
    with torch.no_grad():
        e_packed = model.encode_image(img.to(dev)).cpu()
        assert set(model._packed) == {"ln", "attn", "fc"}      # the packed route ran, on the grown-on-demand operands of > 128 rows
        assert torch.equal(e_packed, model._encode_image_eager(img.to(dev), model._blocks_packed).cpu())
        e_rows = model._encode_image_eager(img.to(dev), model._blocks_per_kernel).cpu()
        assert set(model._packed) == {"ln", "attn", "fc"}
    cos = torch.cosine_similarity(e_packed, e_rows, dim=-1)
    rel = ((e_packed - e_rows).norm(dim=-1) / e_rows.norm(dim=-1)).max().item()
    print("B/16 B %d packed vs row pipeline: min cosine %.7f max relative difference %.3e" % (B, cos.min().item(), rel))
    assert cos.min() > 0.99999 and rel < 5e-3
    assert torch.cosine_similarity(e_packed, ref, dim=-1).min() > 0.9995


@gpu
@pytest.mark.parametrize("B", [1, 2])
def test_b16_training_call_replayed_as_hip_graphs_is_bit_identical_to_eager_launches(B, monkeypatch):
    """test_training_call_replayed_as_hip_graphs_is_bit_identical_to_eager_launches at 197 tokens: what is captured is the per-kernel
    pass (197 and 394 rows)"""
    from avatarclip_amd import clip_vit as V
    _b16(monkeypatch)
    dev = torch.device("cuda")
    model = V.ClipVision(_sd16(), dev)
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
        assert model._graphed.get(B) not in (None, False)       # the graphed route ran
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), k


@gpu
def test_a_b32_and_a_b16_model_in_one_process_give_what_each_gives_alone(monkeypatch):
    """the linears' workspace, the packed operands, the _train_buf keys and the graph caches are per instance or grow without moving
    what a captured graph points at: interleaved calls of the two towers return the bits of their first, undisturbed calls"""
    from avatarclip_amd import clip_vit as V
    from avatarclip_amd.runner import clip_vit_random_state_dict
    dev = torch.device("cuda")
    text = torch.randn(1, 512, generator=torch.Generator().manual_seed(5)).to(dev)
    imgs = torch.randn(3, 3, 224, 224, generator=torch.Generator().manual_seed(21)).to(dev)

    def run(model):
        with torch.no_grad():
            scored = model.encode_image(imgs).clone()
        x = imgs[:1].clone().requires_grad_(True)               # the per-iteration call: replayed as HIP graphs
        e = model.encode_image(x)
        (1 - torch.cosine_similarity(e.mean(0), text.mean(0), dim=0)).backward()
        assert model._graphed.get(1) not in (None, False)
        return scored, e.detach().clone(), x.grad.clone()

    same = lambda a, b: all(torch.equal(s, t) for s, t in zip(a, b))
    m32 = V.ClipVisionB32(clip_vit_random_state_dict(0), dev)
    r32 = run(m32)                                              # no ViT-B/16 instance exists yet
    m16 = V.ClipVision(clip_vit_random_state_dict(0, patch=16), dev)
    assert (m32.patch, m32.tokens, m16.patch, m16.tokens) == (32, 50, 16, 197)
    r16 = run(m16)
    assert r32[0].shape == r16[0].shape == (3, 512) and not torch.equal(r32[0], r16[0])
    for _ in range(2):
        assert same(run(m32), r32)
        assert same(run(m16), r16)
    del m32
    assert same(run(V.ClipVision(clip_vit_random_state_dict(0, patch=16), dev)), r16)      # a ViT-B/16 instance on its own


@gpu
def test_train_clip_iteration_with_b16_weights_matches_the_independent_oracle_iteration(monkeypatch):
    """One Runner.train_clip_iteration, small nets, 32 x 32 rays x 32 spp, with init_clip(clip_state_dict=
    clip_vit_random_state_dict(0, patch=16)), against oracle.iteration_oracle.train_clip_iteration under the patched constants: the
    parity run of test_train_clip_iteration_matches_independent_oracle_iteration_small_nets with its gates (loss 2e-3, cosine 1e-3,
    per-tensor gradient 2e-2 / 0.999, Adam displacement)."""
    from avatarclip_amd import runner as R
    from tests import test_gpu_iteration as TI
    _b16(monkeypatch)
    made = []
    orig = R.clip_vit_random_state_dict

    def b16_weights(seed):
        made.append(orig(seed, patch=16))
        return made[-1]
    monkeypatch.setattr(R, "clip_vit_random_state_dict", b16_weights)
    TI._run_parity(res=32, spp=32, iters=1, small=True)
    assert len(made) == 1 and tuple(made[0]["visual.conv1.weight"].shape) == (768, 3, 16, 16)
