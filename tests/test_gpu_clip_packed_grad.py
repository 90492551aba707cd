"""The packed pipeline of the CLIP tower (clip_vit.BlocksFn) with a gradient above 128 rows: the two epilogues of the LDS-staged GEMM
it needs there (c_fc forward: fp32 pre-activation + packed QuickGELU; c_proj^T backward: times QuickGELU'(pre), packed), the pipeline
forward and backward at 150 / 250 rows (ViT-B/32, 3 and 5 images) and 197 / 394 rows (ViT-B/16, 1 and 2 images), the operands it takes
(what HIP graphs may capture never moves) and the route a call takes when nobody names one.

The epilogues are compared bit for bit: each side of a torch.equal is the same GEMM main loop at the same M, rounded once.  The pipeline
is held against the per-kernel route with the gates of test_gpu_clip.test_fused_residual_blocks_equal_the_per_kernel_autograd_path
(embeddings 4e-3, pixel gradients 1e-2 relative L2; no further from the fp32 oracle than 1.25 x the per-kernel route's own distance).

Measured on an MI355X over the four geometries: packed vs per-kernel embedding 2.1e-3 .. 2.7e-3, pixel gradient 6.2e-3 .. 6.4e-3;
against the fp32 oracle the packed route 3.2e-3 .. 3.4e-3 / 8.3e-3, the per-kernel route 3.1e-3 .. 3.4e-3 / 8.3e-3 (the table:
profiles/clip_packed_grad.md)."""
import pytest
import torch

from oracle import clip_vit_oracle as C

gpu = pytest.mark.gpu

N_FC, K_FC = 3072, 768


def rows(packed, nrows, N):
    """the first `nrows` rows of a packed operand, [row tile][k-step][half][row][8] -> [nrows, N] bf16"""
    mt = (nrows + 31) // 32
    t = packed[:mt * (N // 16) * 1024].view(torch.bfloat16).reshape(mt, N // 16, 2, 32, 8)
    return t.permute(0, 3, 1, 2, 4).reshape(mt * 32, N)[:nrows]


def bits(t):
    return t.view(torch.int16)


_lin = {}


def _fc():
    """one seeded c_fc-shaped weight [3072, 768] with its bias, packed once"""
    if not _lin:
        from avatarclip_amd import clip_vit as V
        g = torch.Generator().manual_seed(7)
        w = torch.randn(N_FC, K_FC, generator=g) * K_FC ** -0.5
        b = torch.randn(N_FC, generator=g) * 0.1
        _lin["lin"] = V._Lin(w, b, torch.device("cuda"))
    return _lin["lin"]


# ---------------------------------------------------------------------------------------------------------------- A. the epilogues
@gpu
@pytest.mark.parametrize("M", [129, 160, 256, 394])
def test_pre_activation_and_quickgelu_derivative_epilogues_of_the_gemm_bit_for_bit(M):
    """M = 129: a ragged group of four row tiles (the GEMM computes 256 rows); 160: two whole tiles in a partial group; 256: exact
    groups; 394: two ViT-B/16 images.  y_pre and gelu_pre are the first M rows of larger buffers whose rest holds -7 / NaN: the -7 must
    survive, and a NaN row that was read would show in the padding rows of the act-2 output, which must be exactly zero."""
    from avatarclip_amd import lib as L
    lib, dev = L.load(), torch.device("cuda")
    lin = _fc()
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, K_FC, generator=g).to(dev)
    Mg = ((M + 127) // 128) * 128                       # rows the GEMM computes
    ps = torch.zeros(lib.avc_vit_workspace_bytes(M, K_FC), dtype=torch.uint8, device=dev)
    L.check(lib.avc_vit_pack(L.ptr(x), None, L.ptr(ps), M, K_FC, L.stream()), "pack")
    nb = lib.avc_vit_workspace_bytes(M, N_FC)
    assert nb == Mg * N_FC * 2
    st = L.stream()

    # a. act 1, packed output + fp32 pre-activation, against the (y + y_pre) call
    y_ref, pre_ref = torch.empty(M, N_FC, device=dev), torch.empty(M, N_FC, device=dev)
    L.check(lib.avc_vit_linear_packed(L.ptr(ps), L.ptr(lin.wp), L.ptr(lin.b), None, None, L.ptr(y_ref), L.ptr(pre_ref), None, M, N_FC, K_FC,
                                      1, st), "linear_packed y + y_pre")
    pre_big = torch.full((Mg + 32, N_FC), -7.0, device=dev)
    py, py_ref = (torch.zeros(nb, dtype=torch.uint8, device=dev) for _ in range(2))
    L.check(lib.avc_vit_linear_packed(L.ptr(ps), L.ptr(lin.wp), L.ptr(lin.b), None, None, None, L.ptr(pre_big[:M]), L.ptr(py), M, N_FC, K_FC,
                                      1, st), "linear_packed ys_packed + y_pre")
    L.check(lib.avc_vit_pack(L.ptr(y_ref), None, L.ptr(py_ref), M, N_FC, st), "pack")
    assert torch.equal(pre_big[:M], pre_ref)
    assert (pre_big[M:] == -7.0).all()                  # nothing of y_pre at or past row M is written
    assert torch.equal(bits(rows(py, M, N_FC)), bits(rows(py_ref, M, N_FC)))
    assert torch.equal(rows(py_ref, M, N_FC).float(), y_ref.bfloat16().float())        # (the helper reads the layout right)

    # b. act 2: (x W^T) * QuickGELU'(pre), packed, against avc_vit_pack(y0, pre) of the act-0 rows
    gp_big = torch.full((Mg + 32, N_FC), float("nan"), device=dev)
    gp_big[:M] = pre_ref
    y0 = torch.empty(M, N_FC, device=dev)
    L.check(lib.avc_vit_linear_packed(L.ptr(ps), L.ptr(lin.wp), None, None, None, L.ptr(y0), None, None, M, N_FC, K_FC, 0, st), "act 0")
    py2 = torch.full((nb,), 0x3F, dtype=torch.uint8, device=dev)       # (not zero: the padding rows have to be WRITTEN as zeros)
    L.check(lib.avc_vit_linear_packed(L.ptr(ps), L.ptr(lin.wp), None, None, L.ptr(gp_big[:M]), None, None, L.ptr(py2), M, N_FC, K_FC, 2, st),
            "act 2")
    py_ref.zero_()
    L.check(lib.avc_vit_pack(L.ptr(y0), L.ptr(gp_big[:M]), L.ptr(py_ref), M, N_FC, st), "pack with gelu_pre")
    got = rows(py2, Mg, N_FC)
    assert torch.equal(bits(got[:M]), bits(rows(py_ref, M, N_FC)))
    assert (bits(got[M:]) == 0).all()                   # rows M .. the end of the last group: zeros, and no NaN row was read
    assert torch.isnan(gp_big[M:]).all()


@gpu
def test_combinations_the_gemm_does_not_cover_are_still_refused_and_launch_nothing():
    from avatarclip_amd import lib as L
    lib, dev = L.load(), torch.device("cuda")
    lin = _fc()
    M = 129
    ps = torch.zeros(lib.avc_vit_workspace_bytes(M, N_FC), dtype=torch.uint8, device=dev)      # (large enough for either K)
    py = torch.zeros(lib.avc_vit_workspace_bytes(M, N_FC), dtype=torch.uint8, device=dev)
    y, res, pre = (torch.zeros(M, N_FC, device=dev) for _ in range(3))
    torch.cuda.synchronize()
    p = L.ptr
    refused = {
        "an activation with a residual": (p(lin.b), p(res), None, p(y), None, None, M, N_FC, K_FC, 1),
        "act 2 with a residual": (None, p(res), p(pre), None, None, p(py), M, N_FC, K_FC, 2),
        "y together with ys_packed": (p(lin.b), None, None, p(y), None, p(py), M, N_FC, K_FC, 0),
        "y together with ys_packed, act 1": (p(lin.b), None, None, p(y), p(pre), p(py), M, N_FC, K_FC, 1),
        "y together with ys_packed, act 2": (None, None, p(pre), p(y), None, p(py), M, N_FC, K_FC, 2),
        "a residual together with ys_packed": (p(lin.b), p(res), None, None, None, p(py), M, N_FC, K_FC, 0),
        "N % 128 != 0": (p(lin.b), None, None, p(y), None, None, M, 96, K_FC, 0),
        "N % 128 != 0, packed": (p(lin.b), None, None, None, p(pre), p(py), M, 96, K_FC, 1),
        "K % 32 != 0": (p(lin.b), None, None, p(y), None, None, M, N_FC, 784, 0),
        "K % 32 != 0, act 2": (None, None, p(pre), None, None, p(py), M, N_FC, 784, 2),
    }
    for what, args in refused.items():
        assert lib.avc_vit_linear_packed(p(ps), p(lin.wp), *args, L.stream()) != 0, what
        assert "more than 128 rows" in lib.avc_last_error().decode(), what
        assert torch.cuda.current_stream().query(), what          # nothing was enqueued
    assert (y == 0).all() and (py == 0).all() and (pre == 0).all()


# ---------------------------------------------------------------------------------------------------------------- B. the pipeline
GEOMETRIES = [(32, 3), (32, 5), (16, 1), (16, 2)]          # (patch, images): 150, 250, 197 and 394 rows
_cache = {}


def _variant(monkeypatch, patch):
    if patch == 16:
        monkeypatch.setattr(C, "PATCH", 16)
        monkeypatch.setattr(C, "TOKENS", 197)
    assert C.PATCH == patch


def _sd(patch):
    """the oracle's seeded weights of the variant (call under _variant)"""
    assert C.PATCH == patch
    if ("sd", patch) not in _cache:
        _cache["sd", patch] = C.random_state_dict(0)
    return _cache["sd", patch]


def _text(dev):
    return torch.randn(1, 512, generator=torch.Generator().manual_seed(5)).to(dev)


def _loss(e, text):
    return 1 - torch.cosine_similarity(e.mean(0), text.mean(0), dim=0)


def _images(patch, B):
    return torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(31 + patch + B))


def _oracle(patch, B):
    """embedding and pixel gradient of the fp32 CPU oracle, once per geometry (call under _variant)"""
    if ("ref", patch, B) not in _cache:
        xr = _images(patch, B).requires_grad_(True)
        ref = C.encode_image(_sd(patch), xr)
        _loss(ref, _text("cpu")).backward()
        _cache["ref", patch, B] = (ref.detach(), xr.grad.clone())
    return _cache["ref", patch, B]


def _grad_call(model, img, text, blocks="encode_image"):
    x = img.clone().requires_grad_(True)
    e = model.encode_image(x) if blocks == "encode_image" else model._encode_image_eager(x, blocks)
    _loss(e, text).backward()
    return e.detach().clone(), x.grad.clone()


@gpu
@pytest.mark.parametrize("patch, B", GEOMETRIES)
def test_packed_pipeline_with_a_gradient_above_128_rows_against_the_per_kernel_route_and_the_oracle(patch, B, monkeypatch):
    from avatarclip_amd import clip_vit as V
    _variant(monkeypatch, patch)
    dev = torch.device("cuda")
    model = V.ClipVision(_sd(patch), dev)
    assert model.patch == patch and B * model.tokens >= V.BIG_M
    text, img = _text(dev), _images(patch, B).to(dev)
    res = []
    for blocks in (model._blocks_packed, model._blocks_per_kernel):
        e, gx = _grad_call(model, img, text, blocks)
        with torch.no_grad():
            e0 = model._encode_image_eager(img, blocks)
        res.append((e, gx, e0))
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    ee, eg, e0 = rel(res[0][0], res[1][0]), rel(res[0][1], res[1][1]), rel(res[0][2], res[1][2])
    ref, gref = _oracle(patch, B)
    err = [(rel(r[0].cpu(), ref), rel(r[1].cpu(), gref)) for r in res]
    print("ViT-B/%d B %d (%d rows) packed vs per-kernel: embedding %.3e pixel gradient %.3e no-grad embedding %.3e | vs the fp32 oracle "
          "(embedding, pixel gradient): packed %.3e %.3e per-kernel %.3e %.3e" % (patch, B, B * model.tokens, ee, eg, e0, *err[0], *err[1]))
    assert torch.isfinite(res[0][1]).all()
    assert ee < 4e-3 and e0 < 4e-3 and eg < 1e-2, (ee, e0, eg)
    assert err[0][0] < 1.25 * err[1][0] and err[0][1] < 1.25 * err[1][1], err
    assert torch.equal(res[0][0], res[0][2])        # the no-grad call of the same input returns the gradient call's forward


# ---------------------------------------------------------------------------------------------------------------- C. buffers and graphs
@gpu
@pytest.mark.parametrize("graph", [True, False])
def test_b16_gradient_call_keeps_its_operands_when_a_larger_scoring_call_grows_the_others(graph, monkeypatch):
    """What a captured ViT-B/16 pass points at must not move: its operands are the per-shape ("train", ...) buffers, and a scoring call
    of 8 images in between (1576 rows: the grown-on-demand operands and the linears' workspace are re-allocated) changes no bit of the
    next gradient call, replayed or launched eagerly."""
    from avatarclip_amd import clip_vit as V
    _variant(monkeypatch, 16)
    monkeypatch.setattr(V, "TRAIN_GRAPH", graph)
    dev = torch.device("cuda")
    model = V.ClipVision(_sd(16), dev)
    text, img = _text(dev), _images(16, 2).to(dev)
    e1, g1 = _grad_call(model, img, text)
    assert (model._graphed.get(2) not in (None, False)) == graph
    assert model._packed and all(isinstance(k, tuple) and k[0] == "train" for k in model._packed), list(model._packed)
    with torch.no_grad():
        big = model.encode_image(torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(8)).to(dev))
    assert torch.isfinite(big).all() and {"ln", "attn", "fc"} <= set(model._packed)
    e2, g2 = _grad_call(model, img, text)
    assert torch.isfinite(g1).all()
    assert torch.equal(e1, e2) and torch.equal(g1, g2)


@gpu
def test_grown_operands_of_a_larger_gradient_call_do_not_reach_a_smaller_one():
    """ViT-B/32, 5 images then 3: the 3 run on operands the 5 left filled past their rows, and give the bits a fresh model gives.  The
    gradient calls' operands are grown per role -- not one per row count -- under names apart from the scoring route's."""
    from avatarclip_amd import clip_vit as V
    dev = torch.device("cuda")
    sd = _sd(32)
    text = _text(dev)
    img5, img3 = _images(32, 5).to(dev), _images(32, 3).to(dev)
    model = V.ClipVisionB32(sd, dev)
    _grad_call(model, img5, text)
    keys = set(model._packed)
    assert keys and not any(isinstance(k, tuple) for k in keys) and not keys & {"ln", "attn", "fc"}, keys
    e3, g3 = _grad_call(model, img3, text)
    assert set(model._packed) == keys
    f3, h3 = _grad_call(V.ClipVisionB32(sd, dev), img3, text)
    assert torch.isfinite(g3).all()
    assert torch.equal(e3, f3) and torch.equal(g3, h3)


# ---------------------------------------------------------------------------------------------------------------- D. the default route
@gpu
@pytest.mark.parametrize("patch, B", [(16, 2), (32, 5)])
def test_a_gradient_call_above_128_rows_takes_the_packed_route_when_nobody_names_one(patch, B, monkeypatch):
    from avatarclip_amd import clip_vit as V
    _variant(monkeypatch, patch)
    dev = torch.device("cuda")
    model = V.ClipVision(_sd(patch), dev)
    text, img = _text(dev), _images(patch, B).to(dev)
    e, gx = _grad_call(model, img, text, None)
    ep, gp = _grad_call(model, img, text, model._blocks_packed)
    assert torch.equal(e, ep) and torch.equal(gx, gp)
    assert any(k[1] == "dh" if isinstance(k, tuple) else k == "grad_dh" for k in model._packed)     # BlocksFn's backward ran
