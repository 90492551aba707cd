"""tests/clip_kernel_restatement.py against torch, and the input conditions tests/test_gpu_clip_kernels.py rests on, without a GPU."""
import pytest
import torch

from tests import clip_kernel_restatement as R

LATENCY_K = [16, 112, 128, 144, 512, 768, 784, 1536, 1552, 2048, 2304, 2320, 3072, 3088, 4096]


@pytest.mark.parametrize("N", [32, 96])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 129])
def test_pack_rows_and_unpack_rows_round_trip(M, N):
    g = torch.Generator().manual_seed(M * 100 + N)
    x = torch.randn(M, N, generator=g).bfloat16()
    p = R.pack_rows(x)
    mt = R.row_tiles(M)
    assert mt == {1: 1, 31: 1, 32: 1, 33: 2, 129: 8}[M]
    assert p.dtype == torch.uint8 and p.numel() == mt * (N // 16) * 1024
    assert torch.equal(R.bits(R.unpack_rows(p, M, N)), R.bits(x))
    whole = R.unpack_rows(p, mt * 32, N)
    assert (R.bits(whole[M:]) == 0).all()                       # the padding rows of the last tile or group are zero
    assert torch.equal(R.pack_rows(whole), p)
    # element (r, c) by the index rule of include/avc.h
    e = p.view(torch.bfloat16)
    for r, c in ((0, 0), (M - 1, N - 1), (M // 2, 9), (M - 1, 16)):
        at = (((r >> 5) * (N >> 4) + (c >> 4)) * 64 + (r & 31) + 32 * ((c >> 3) & 1)) * 8 + (c & 7)
        assert R.bits(e[at]) == R.bits(x[r, c])


def test_pack_weight_is_the_header_statement_spelled_as_an_index_loop():
    """include/avc.h: W pre-packed bf16 [N/32][K/16][64][8], lane (n, h) holds W[32t+n][16s+8h+j]"""
    from avatarclip_amd import clip_vit as V
    N, K = 64, 32
    w = torch.randn(N, K, generator=torch.Generator().manual_seed(1))
    got = V.pack_weight(w)
    assert got.dtype == torch.bfloat16 and got.shape == (N * K,)
    want = torch.empty(N // 32, K // 16, 64, 8, dtype=torch.bfloat16)
    for t in range(N // 32):
        for s in range(K // 16):
            for n in range(32):
                for h in range(2):
                    for j in range(8):
                        want[t, s, n + 32 * h, j] = w[32 * t + n, 16 * s + 8 * h + j].bfloat16()
    assert torch.equal(R.bits(got), R.bits(want.reshape(-1)))
    assert torch.equal(got.view(torch.uint8), R.pack_rows(w.bfloat16()))      # the A and B operands share one layout


def test_fp64_layernorm_restatements_agree_with_torch():
    x, gamma, beta = (t.double() for t in R.layernorm_inputs(9, 1, constant_row=4))
    g = torch.Generator().manual_seed(2)
    dy, res = torch.randn(9, 768, generator=g).double(), torch.randn(9, 768, generator=g).double()
    xr = x.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xr, (768,), gamma, beta, 1e-5)
    y.backward(dy)
    assert (R.layernorm(x, gamma, beta, 1e-5) - y.detach()).abs().max() < 1e-12
    assert (R.layernorm_bwd(dy, x, gamma, 1e-5) - xr.grad).abs().max() < 1e-10
    assert (R.layernorm_bwd(dy, x, gamma, 1e-5, res) - (xr.grad + res)).abs().max() < 1e-10
    assert torch.equal(R.layernorm(x, gamma, beta, 1e-5)[4], beta)             # the constant row: variance 0, LayerNorm = beta


def test_fp64_quickgelu_derivative_is_the_autograd_derivative():
    p = torch.linspace(-40, 40, 1601, dtype=torch.float64, requires_grad=True)
    R.quickgelu(p).sum().backward()
    assert (R.quickgelu_grad(p.detach()) - p.grad).abs().max() < 1e-13
    assert R.quickgelu_grad(torch.tensor([40.0])).float().item() == 1.0          # (part D, case 1: the factor is 1 in fp32)


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("B, T, heads", [(2, 5, 3), (1, 1, 1), (1, 33, 2)])
def test_fp64_attention_restatement_agrees_with_torch_softmax(B, T, heads, causal):
    qkv = R.attention_inputs(B, T, heads, 3, q_scale=3.0).double()
    W = heads * 64
    q, k, v = (t.reshape(B, T, heads, 64).transpose(1, 2) for t in qkv.split(W, dim=-1))
    sc = q @ k.transpose(-1, -2) / 8
    if causal:
        sc = sc + torch.full((T, T), float("-inf"), dtype=torch.float64).triu(1)
    want = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B, T, W)
    got = R.attention(qkv, heads, causal)
    assert (got - want).abs().max() < 1e-12
    if causal:
        assert torch.equal(got[:, 0], qkv[:, 0, 2 * W:])                         # row 0 under the mask is v[0]


def test_integer_cases_stay_exact_in_fp32():
    """every latency-kernel K at M = 77 and the largest GEMM shapes: operands in range and exact in bf16, results below 2^24, and the
    fp32 matmul of torch (some other order of the sums) returns the int64 reference bit for bit"""
    assert R.X_MAX * R.W_MAX * R.K_MAX + 2 * R.B_MAX < R.EXACT_BELOW
    for M, N, K in [(77, 96, k) for k in LATENCY_K] + [(129, 128, 32), (150, 768, 3072), (197, 768, 2304)]:
        c = R.integer_case(M, N, K)
        for name, lim in (("x", R.X_MAX), ("w", R.W_MAX), ("bias", R.B_MAX), ("res", R.B_MAX)):
            t = c[name]
            assert t.dtype == torch.float32 and t.abs().max() <= lim and torch.equal(t, t.round()), name
            assert torch.equal(t.bfloat16().float(), t), name
        assert c["x"].abs().max() == R.X_MAX and c["w"].abs().max() == R.W_MAX
        for v in c["ref"].values():
            assert v.dtype == torch.int64 and int(v.abs().max()) < R.EXACT_BELOW
        assert torch.equal((c["x"] @ c["w"].t() + c["bias"] + c["res"]).long(), c["ref"]["full"])
        assert torch.equal(c["ref"]["full"].float().long(), c["ref"]["full"])


@pytest.mark.parametrize("K", [768, 3072])
@pytest.mark.parametrize("M", [77, 128, 129, 200])
def test_thinned_cases_keep_half_of_the_pre_activations_out_of_saturation(M, K):
    c = R.thinned_case(M, 128, K)
    assert c["share"] >= 0.5 and c["share"] == R.thinned_share(c["pre"])
    assert c["w"].abs().max() == 1 and c["bias"].abs().max() <= 2 and c["x"].abs().max() <= R.X_MAX
    nz = (c["x"] != 0).float().sum(1).mean().item()
    assert 6 < nz < 9, nz                                                        # about 8 entries per row (7.1 after the zeros drawn)
    assert torch.equal((c["x"] @ c["w"].t() + c["bias"]).long(), c["pre"])
    # the share of outputs on which QuickGELU is neither the identity nor zero to fp32
    y, p = R.quickgelu(c["pre"]), c["pre"].double()
    assert float(((y != p) & (y != 0)).double().mean()) > 0.5


def test_the_half_ulp_bound_holds_for_an_fp32_layernorm_rounded_to_bf16_and_not_at_half_of_it():
    """the bound of the packed LayerNorm output, on the CPU: fp32 F.layer_norm rounded to bf16 stays inside 2^-8 |ref| + the fp32 slack
    on every element, and a 2^-9 bound would be violated -- so the bound is as tight as a correctly rounded result allows"""
    x, gamma, beta = R.layernorm_inputs(160, 0)
    ref = R.layernorm(x, gamma, beta, 1e-5)
    y32 = torch.nn.functional.layer_norm(x, (768,), gamma, beta, 1e-5)
    assert R.slack_excess(y32, ref) <= 1
    got = y32.bfloat16()
    assert R.half_ulp_excess(got, ref) <= 1
    tighter = ((got.double() - ref).abs() / (2.0 ** -9 * ref.abs() + R.FP32_SLACK * (1 + ref.abs()))).max()
    assert tighter > 1


def test_fp32_torch_stays_inside_the_fp32_slack_on_the_gpu_tests_inputs():
    """LayerNorm backward, QuickGELU on integers and attention with scores of +-14 in plain fp32 against the fp64 restatements"""
    x, gamma, beta = R.layernorm_inputs(50, 0)
    g = torch.Generator().manual_seed(50)
    dy, res = torch.randn(50, 768, generator=g), torch.randn(50, 768, generator=g)
    xr = x.clone().requires_grad_(True)
    torch.nn.functional.layer_norm(xr, (768,), gamma, beta, 1e-5).backward(dy)
    assert R.slack_excess(xr.grad + res, R.layernorm_bwd(dy, x, gamma, 1e-5, res)) <= 1
    p = torch.arange(-40, 41, dtype=torch.float32)
    assert R.slack_excess(p * torch.sigmoid(1.702 * p), R.quickgelu(p)) <= 1
    qkv = R.attention_inputs(2, 77, 8, 1, q_scale=3.0)
    q, k, v = (t.reshape(2, 77, 8, 64).transpose(1, 2) for t in qkv.split(512, dim=-1))
    sc = q @ k.transpose(-1, -2) / 8
    assert sc.abs().max() > 10
    out = (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(2, 77, 512)
    assert R.slack_excess(out, R.attention(qkv, 8, 0)) <= 1
