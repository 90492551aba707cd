"""The linears, LayerNorm kernels and text-tower attention of csrc/avc_vit.hip and csrc/avc_vit_gemm.hip through their raw entry
points, element by element against tests/clip_kernel_restatement.py.

A, B, D case 1, every y_pre and every padding row: bit equality against an int64 matmul (integer operands: exact in bf16 and in fp32
sums of any order).  Everything else against fp64 under |got - ref| <= 2e-5 (1 + |ref|), packed bf16 results with half a bf16 ulp,
2^-8 |ref|, on top; every element, no share of exceptions.  Code paths and the maxima measured on an MI355X:
profiles/clip_kernel_pins.md.

Every operand and output buffer has at least the size the entry point documents (avc_vit_workspace_bytes); outputs are leading views of
larger allocations whose remainder holds a sentinel that has to survive."""
import pytest
import torch

from tests import clip_kernel_restatement as R

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
LATENCY_M = [1, 31, 32, 33, 77, 100, 128]
LATENCY_K = [16, 112, 128, 144, 512, 768, 784, 1536, 1552, 2048, 2304, 2320, 3072, 3088, 4096]
LATENCY_CASES = [(77, k) for k in LATENCY_K] + [(m, k) for k in (768, 2304) for m in LATENCY_M if m != 77]
GEMM_SHAPES = [(129, 128, 32), (200, 384, 64), (257, 640, 96), (385, 1152, 160), (150, 768, 768), (150, 3072, 768), (150, 768, 3072),
               (197, 2304, 768), (197, 768, 2304)]


class _Env:
    def __init__(self):
        from avatarclip_amd import clip_vit, lib
        self.L, self.lib, self.dev = lib, lib.load(), torch.device("cuda")
        self.pack_weight = clip_vit.pack_weight

    @property
    def st(self):
        return self.L.stream()

    def dev_(self, t):
        return None if t is None else t.to(self.dev)

    def weight(self, w):
        return self.pack_weight(w).to(self.dev)

    def operand(self, x):
        """pack_rows of x (fp32 values exact in bf16, or bf16) in a zeroed buffer of avc_vit_workspace_bytes"""
        M, K = x.shape
        buf = torch.zeros(self.lib.avc_vit_workspace_bytes(M, K), dtype=torch.uint8, device=self.dev)
        p = R.pack_rows(x.bfloat16())
        assert p.numel() <= buf.numel()
        buf[:p.numel()] = p.to(self.dev)
        return buf

    def workspace(self, M, K):
        return torch.zeros(self.lib.avc_vit_workspace_bytes(M, K), dtype=torch.uint8, device=self.dev)

    def packed_out(self, M, N, byte=0x3F):
        return torch.full((self.lib.avc_vit_workspace_bytes(M, N),), byte, dtype=torch.uint8, device=self.dev)

    def guarded(self, M, N, fill=SENTINEL):
        """([M + 8, N] filled with `fill`, its first M rows)"""
        big = torch.full((M + 8, N), fill, device=self.dev)
        return big, big[:M]

    def linear(self, x, wp, bias, res, y, y_pre, M, N, K, act):
        """avc_vit_linear: fp32 rows in, the packing pre-pass into a workspace"""
        ws = self.workspace(M, K)
        p = self.L.ptr
        self.L.check(self.lib.avc_vit_linear(p(x), p(wp), p(bias), p(res), p(y), p(y_pre), M, N, K, act, p(ws), self.st), "avc_vit_linear")

    def linear_packed(self, xs, wp, bias, res, gelu_pre, y, y_pre, ys, M, N, K, act):
        p = self.L.ptr
        self.L.check(self.lib.avc_vit_linear_packed(p(xs), p(wp), p(bias), p(res), p(gelu_pre), p(y), p(y_pre), p(ys), M, N, K, act, self.st),
                     "avc_vit_linear_packed")


_env = []


def env():
    if not _env:
        _env.append(_Env())
    return _env[0]


def survived(big, M, fill=SENTINEL):
    return bool((big[M:] == fill).all())


def bf16_bits(t):
    """bits of the bf16 rounding (RNE) of an exactly known fp32 / int64 tensor"""
    return R.bits(t.float().bfloat16())


def exact_rows(y, ref_int):
    """an fp32 device result equals an int64 reference bit for bit"""
    return torch.equal(y.cpu(), ref_int.float())


def group_rows(M):
    return R.row_tiles(M) * 32


# ------------------------------------------------------------------------------------------------------- A. the latency kernel, exact
def _latency_exact(M, N, K):
    E = env()
    c = R.integer_case(M, N, K)
    x, b, r, wp = E.dev_(c["x"]), E.dev_(c["bias"]), E.dev_(c["res"]), E.weight(c["w"])
    ref = c["ref"]
    # fp32 rows in (the packing pre-pass), with and without bias and residual
    for bias, res, key in ((None, None, "plain"), (b, None, "bias"), (None, r, "res"), (b, r, "full")):
        big, y = E.guarded(M, N)
        E.linear(x, wp, bias, res, y, None, M, N, K, 0)
        assert exact_rows(y, ref[key]), (key, (y.cpu() - ref[key].float()).abs().max())
        assert survived(big, M), key
    # a packed operand no kernel produced
    xs = E.operand(c["x"])
    big, y = E.guarded(M, N)
    E.linear_packed(xs, wp, None, None, None, y, None, None, M, N, K, 0)
    assert exact_rows(y, ref["plain"]) and survived(big, M)
    # ys_packed only: the bits of bf16(y), the rows past M of the last tile WRITTEN as zeros
    Mt = group_rows(M)
    ys = E.packed_out(M, N)
    E.linear_packed(xs, wp, b, None, None, None, None, ys, M, N, K, 0)
    got = R.unpack_rows(ys, Mt, N).cpu()
    assert torch.equal(R.bits(got[:M]), bf16_bits(ref["bias"]))
    assert (R.bits(got[M:]) == 0).all()
    # y beside ys_packed, bias and residual
    ys = E.packed_out(M, N)
    big, y = E.guarded(M, N)
    E.linear_packed(xs, wp, b, r, None, y, None, ys, M, N, K, 0)
    got = R.unpack_rows(ys, Mt, N).cpu()
    assert exact_rows(y, ref["full"]) and survived(big, M)
    assert torch.equal(R.bits(got[:M]), bf16_bits(ref["full"])) and torch.equal(R.bits(got[:M]), R.bits(y.bfloat16().cpu()))
    assert (R.bits(got[M:]) == 0).all()


@pytest.mark.parametrize("M, K", LATENCY_CASES)
def test_latency_linear_equals_the_integer_matmul_bit_for_bit(M, K):
    """N = 96 (three column tiles).  K picks the instantiation: ceil(K / 16 / 8) k-steps per wavefront, NB = 6, 12, 18 or 24; K = 16:
    seven wavefronts without a k-step; 112 / 144, 784, 1552, 2320: a ragged share (`s < KS` inside a batch); 3088, 4096: a second round
    of the batch loop"""
    _latency_exact(M, 96, K)


@pytest.mark.parametrize("N", [32, 512])
def test_latency_linear_one_and_sixteen_column_tiles(N):
    _latency_exact(77, N, 768)


def test_latency_linear_writes_zero_padding_whatever_the_operand_holds_past_its_rows():
    """the operand a larger call left behind: rows 77 .. 95 of the last tile are not zero.  The valid rows do not see them, and the packed
    output's rows past M are zeros all the same (include/avc.h)"""
    E = env()
    M, N, K = 77, 96, 768
    c = R.integer_case(M, N, K)
    b, wp = E.dev_(c["bias"]), E.weight(c["w"])
    x96 = torch.full((96, K), 3.0)
    x96[:M] = c["x"]
    xs = E.operand(x96)
    ys = E.packed_out(M, N)
    big, y = E.guarded(M, N)
    E.linear_packed(xs, wp, b, None, None, y, None, ys, M, N, K, 0)
    got = R.unpack_rows(ys, 96, N).cpu()
    assert exact_rows(y, c["ref"]["bias"]) and survived(big, M)
    assert torch.equal(R.bits(got[:M]), bf16_bits(c["ref"]["bias"]))
    assert (R.bits(got[M:]) == 0).all()


# ---------------------------------------------------------------------------------------------------------------- B. the GEMM, exact
@pytest.mark.parametrize("M, N, K", GEMM_SHAPES)
def test_gemm_linear_equals_the_integer_matmul_bit_for_bit(M, N, K):
    """K / 32 = 1, 2, 3 ring iterations against 3 ring slots (prologue and tail), 2, 6, 15, 36 blocks (the XCD renumbering with a block
    count that is no multiple of 8), one column block, ragged groups of four row tiles, and the shipped shapes"""
    E = env()
    assert M > 128
    c = R.integer_case(M, N, K)
    x, b, r, wp = E.dev_(c["x"]), E.dev_(c["bias"]), E.dev_(c["res"]), E.weight(c["w"])
    ref = c["ref"]
    xs = E.operand(c["x"])
    for bias, res, key in ((None, None, "plain"), (b, None, "bias"), (None, r, "res"), (b, r, "full")):
        big, y = E.guarded(M, N)
        E.linear(x, wp, bias, res, y, None, M, N, K, 0)                      # fp32 rows: the packing pre-pass in groups of four
        assert exact_rows(y, ref[key]), (key, (y.cpu() - ref[key].float()).abs().max())
        assert survived(big, M), key
        big2, y2 = E.guarded(M, N)
        E.linear_packed(xs, wp, bias, res, None, y2, None, None, M, N, K, 0)    # pack_rows of the same operand: the same y
        assert torch.equal(y2, y) and survived(big2, M), key
    # into ys_packed: the M rows the bits of bf16(y), rows M .. the end of the last group of four tiles f(bias) = bias
    Mg = group_rows(M)
    for bias, key in ((b, "bias"), (None, "plain")):
        ys = E.packed_out(M, N)
        E.linear_packed(xs, wp, bias, None, None, None, None, ys, M, N, K, 0)
        got = R.unpack_rows(ys, Mg, N).cpu()
        assert torch.equal(R.bits(got[:M]), bf16_bits(ref[key])), key
        pad = c["bias"] if bias is not None else torch.zeros(N)
        assert torch.equal(R.bits(got[M:]), bf16_bits(pad).expand(Mg - M, N)), key


# ------------------------------------------------------------------------------------------- C. activation epilogues on both routes
@pytest.mark.parametrize("M", [77, 128, 129, 200])
def test_quickgelu_epilogues_exact_pre_activation_and_fp64_activation(M):
    """(N, K) = (128, 768), thinned operands (at least half of the pre-activations in [-4, 4]).  77, 128: the latency kernel; 129, 200:
    the GEMM.  act 1: y_pre is the integer reference, y and ys_packed the fp64 QuickGELU of it; act 2: the product times
    QuickGELU'(gelu_pre) with gelu_pre the exact pre-activation"""
    E = env()
    N, K = 128, 768
    c = R.thinned_case(M, N, K)
    x, b, wp = E.dev_(c["x"]), E.dev_(c["bias"]), E.weight(c["w"])
    xs = E.operand(c["x"])
    pre, act_ref = c["pre"], R.quickgelu(c["pre"])
    Mg, gemm = group_rows(M), M > 128
    worst, err = {}, {}
    # act 1, fp32 rows out + y_pre, both entry points
    for name in ("linear", "linear_packed"):
        (bigy, y), (bigp, yp) = E.guarded(M, N), E.guarded(M, N)
        if name == "linear":
            E.linear(x, wp, b, None, y, yp, M, N, K, 1)
        else:
            E.linear_packed(xs, wp, b, None, None, y, yp, None, M, N, K, 1)
        assert exact_rows(yp, pre) and survived(bigp, M) and survived(bigy, M), name
        worst["act 1 y"] = max(worst.get("act 1 y", 0), R.slack_excess(y, act_ref))
        err["act 1 y"] = max(err.get("act 1 y", 0), R.max_abs_error(y, act_ref))
    # act 1, packed out + y_pre
    ys = E.packed_out(M, N)
    bigp, yp = E.guarded(M, N)
    E.linear_packed(xs, wp, b, None, None, None, yp, ys, M, N, K, 1)
    got = R.unpack_rows(ys, Mg, N).cpu()
    assert exact_rows(yp, pre) and survived(bigp, M)
    worst["act 1 ys"] = R.half_ulp_excess(got[:M], act_ref)
    if gemm:                    # rows past M: f(bias)
        worst["act 1 ys padding"] = R.half_ulp_excess(got[M:], R.quickgelu(c["bias"]).expand(Mg - M, N))
    else:
        assert (R.bits(got[M:]) == 0).all()
    # act 2: gelu_pre is the leading view of an allocation whose remainder is NaN; without and with a bias
    biggp, gp = E.guarded(M, N, float("nan"))
    gp.copy_(pre.float())
    for bias, prod in ((None, c["prod"]), (b, pre)):
        ref2 = prod.double() * R.quickgelu_grad(pre)
        ys = E.packed_out(M, N)
        if gemm:
            E.linear_packed(xs, wp, bias, None, gp, None, None, ys, M, N, K, 2)
        else:
            bigy, y = E.guarded(M, N)
            E.linear_packed(xs, wp, bias, None, gp, y, None, ys, M, N, K, 2)
            assert survived(bigy, M)
            worst["act 2 y"] = max(worst.get("act 2 y", 0), R.slack_excess(y, ref2))
            err["act 2 y"] = max(err.get("act 2 y", 0), R.max_abs_error(y, ref2))
        got = R.unpack_rows(ys, Mg, N).cpu()
        if not gemm:
            assert torch.equal(R.bits(got[:M]), R.bits(y.bfloat16().cpu()))
        worst["act 2 ys"] = max(worst.get("act 2 ys", 0), R.half_ulp_excess(got[:M], ref2))
        assert (R.bits(got[M:]) == 0).all()                                     # zeros on both routes, with a bias too
    assert torch.isnan(biggp[M:]).all()
    print("M %d: share of pre-activations in [-4, 4] %.2f; error / bound:" % (M, c["share"]),
          ", ".join("%s %.3f" % kv for kv in sorted(worst.items())), "; max |error| of the fp32 rows:",
          ", ".join("%s %.2e" % kv for kv in sorted(err.items())))
    assert all(v <= 1 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------------- D. avc_vit_linear_bwd_gelu
@pytest.mark.parametrize("M", [100, 200])
def test_linear_bwd_gelu_with_a_saturated_pre_activation_is_the_plain_integer_linear(M):
    """pre = +40: sigmoid(68.08) is 1 in fp32 (exp(-68) vanishes against 1), so s + 1.702 p s (1 - s) is exactly 1 and the call returns
    dy W bit for bit -- 100 rows: the latency kernel at K = 3072 (NB 24); 200: the GEMM"""
    E = env()
    N, K = 768, 3072
    c = R.integer_case(M, N, K)
    dy, wtp = E.dev_(c["x"]), E.weight(c["w"])
    pre = torch.full((M, K), 40.0, device=E.dev)
    big, dx = E.guarded(M, N)
    ws = E.workspace(M, K)
    p = E.L.ptr
    E.L.check(E.lib.avc_vit_linear_bwd_gelu(p(dy), p(pre), p(wtp), p(dx), M, N, K, p(ws), E.st), "avc_vit_linear_bwd_gelu")
    assert exact_rows(dx, c["ref"]["plain"]) and survived(big, M)


@pytest.mark.parametrize("M", [77, 200])
def test_pack_with_gelu_pre_is_dy_times_the_fp64_derivative(M):
    """the derivative folded into the packing pass, on its own: no K = 3072 sum behind it"""
    E = env()
    K = 768
    g = torch.Generator().manual_seed(M)
    dy, pre = torch.randn(M, K, generator=g), torch.randn(M, K, generator=g) * 3
    xs = E.packed_out(M, K)
    p = E.L.ptr
    dyd, pred = E.dev_(dy), E.dev_(pre)
    E.L.check(E.lib.avc_vit_pack(p(dyd), p(pred), p(xs), M, K, E.st), "avc_vit_pack")
    Mt = ((M + 31) // 32) * 32
    got = R.unpack_rows(xs, Mt, K).cpu()
    ex = R.half_ulp_excess(got[:M], dy.double() * R.quickgelu_grad(pre))
    print("M %d: avc_vit_pack(dy, pre) error / bound %.3f" % (M, ex))
    assert ex <= 1
    assert (R.bits(got[M:]) == 0).all()
    xs2 = E.packed_out(M, K)
    E.L.check(E.lib.avc_vit_pack(p(dyd), None, p(xs2), M, K, E.st), "avc_vit_pack")
    assert torch.equal(R.bits(R.unpack_rows(xs2, M, K).cpu()), R.bits(dy.bfloat16()))


# --------------------------------------------------------------------------------------------------------------------- E. LayerNorm
@pytest.mark.parametrize("M", [1, 3, 4, 5, 100, 128, 129, 160, 257])
def test_layernorm_forward_packed_against_fp64(M):
    """up to 128 rows one wavefront per row, four rows per workgroup (1, 3, 4, 5: around one workgroup); above the 32-row tile kernel in
    groups of four tiles.  One channel is 40 x the others; the second case has a constant row (variance 0, output beta)"""
    E = env()
    p = E.L.ptr
    rows_kernel = M <= 128
    Mg = group_rows(M) if not rows_kernel else 128
    for const in (None, M // 2):
        x, gamma, beta = R.layernorm_inputs(M, 0, constant_row=const)
        xs = E.workspace(M, 768) if rows_kernel else E.packed_out(M, 768)
        assert xs.numel() == Mg * 768 * 2
        xd, gd, bd = E.dev_(x), E.dev_(gamma), E.dev_(beta)
        E.L.check(E.lib.avc_vit_ln_pack(p(xd), p(gd), p(bd), 1e-5, M, 768, p(xs), E.st), "avc_vit_ln_pack")
        got = R.unpack_rows(xs, Mg, 768).cpu()
        ref = R.layernorm(x, gamma, beta, 1e-5)
        ex = R.half_ulp_excess(got[:M], ref)
        print("M %d%s: LayerNorm packed error / bound %.3f, max |error| %.2e" % (M, "" if const is None else " (constant row)", ex,
                                                                               R.max_abs_error(got[:M], ref)))
        assert ex <= 1
        if const is not None:
            assert torch.equal(ref[const], beta.double()) and R.half_ulp_excess(got[const], beta) <= 1
        if rows_kernel:
            assert (R.bits(got[M:]) == 0).all()                                 # rows past M of a zero-filled buffer stay zero
        else:
            assert torch.equal(R.bits(got[M:]), bf16_bits(beta).expand(Mg - M, 768))    # LayerNorm(0) = beta, bit for bit


@pytest.mark.parametrize("M", [1, 5, 50, 128, 160])
def test_layernorm_backward_against_fp64(M):
    E = env()
    p = E.L.ptr
    x, gamma, _ = R.layernorm_inputs(M, 1)
    g = torch.Generator().manual_seed(40 + M)
    dy, res = torch.randn(M, 768, generator=g), torch.randn(M, 768, generator=g)
    xd, gd, dyd, resd = (E.dev_(t) for t in (x, gamma, dy, res))
    pattern = torch.full((2,), 0xA5, dtype=torch.uint8).view(torch.int16).item()
    Mg = E.lib.avc_vit_workspace_bytes(M, 768) // (768 * 2)
    worst = err = 0.0
    for with_res in (False, True):
        ref = R.layernorm_bwd(dy, x, gamma, 1e-5, res if with_res else None)
        for with_xs in (False, True):
            big, dx = E.guarded(M, 768)
            xs = E.packed_out(M, 768, 0xA5) if with_xs else None
            E.L.check(E.lib.avc_vit_ln_bwd(p(dyd), p(xd), p(gd), 1e-5, p(resd if with_res else None), p(dx), p(xs), M, 768, E.st),
                      "avc_vit_ln_bwd")
            worst = max(worst, R.slack_excess(dx, ref))
            err = max(err, R.max_abs_error(dx, ref))
            assert survived(big, M)
            if with_xs:
                got = R.unpack_rows(xs, Mg, 768).cpu()
                assert torch.equal(R.bits(got[:M]), R.bits(dx.bfloat16().cpu()))
                assert (R.bits(got[M:]) == pattern).all()                       # rows past M are not touched
    print("M %d: LayerNorm backward error / bound %.3f, max |error| %.2e" % (M, worst, err))
    assert worst <= 1


def test_layernorm_entry_points_refuse_another_width_and_launch_nothing():
    E = env()
    p = E.L.ptr
    M, K = 5, 512
    x, dy, dx = (torch.zeros(M, 768, device=E.dev) for _ in range(3))
    gamma, beta = torch.ones(768, device=E.dev), torch.zeros(768, device=E.dev)
    xs = E.workspace(M, 768)
    torch.cuda.synchronize()
    assert E.lib.avc_vit_ln_pack(p(x), p(gamma), p(beta), 1e-5, M, K, p(xs), E.st) != 0
    assert "768" in E.lib.avc_last_error().decode() and torch.cuda.current_stream().query()
    assert E.lib.avc_vit_ln_bwd(p(dy), p(x), p(gamma), 1e-5, None, p(dx), p(xs), M, K, E.st) != 0
    assert "768" in E.lib.avc_last_error().decode() and torch.cuda.current_stream().query()
    assert (xs == 0).all() and (dx == 0).all()


# ---------------------------------------------------------------------------------------------------------------- F. text attention
def _text_attention(B, T, heads, causal, q_scale=1.0):
    E = env()
    p = E.L.ptr
    W = heads * 64
    qkv_cpu = R.attention_inputs(B, T, heads, causal, q_scale)
    n_in, n_out = B * T * 3 * W, B * T * W
    big_in = torch.full((n_in + 4 * 3 * W,), float("nan"), device=E.dev)
    big_in[:n_in] = qkv_cpu.reshape(-1).to(E.dev)
    big_out = torch.full((n_out + 4 * W,), SENTINEL, device=E.dev)
    qkv, out = big_in[:n_in].view(B, T, 3 * W), big_out[:n_out].view(B, T, W)
    E.L.check(E.lib.avc_text_attention_fwd(p(qkv), p(out), B, T, W, heads, causal, E.st), "avc_text_attention_fwd")
    got = out.cpu()
    assert bool((big_out[n_out:] == SENTINEL).all()) and not torch.isnan(got).any()
    if causal:
        assert torch.equal(got[:, 0], qkv_cpu[:, 0, 2 * W:])                    # one key: the softmax weight is exactly 1
    ref = R.attention(qkv_cpu, heads, causal)
    return R.slack_excess(got, ref), R.max_abs_error(got, ref)


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("B, heads", [(2, 8), (1, 1)])
@pytest.mark.parametrize("T", [1, 2, 77, 126, 127, 128])
def test_text_attention_against_fp64(T, B, heads, causal):
    """T = 127, 128: 2 T 65 4 = 66 040 and 66 560 bytes of LDS, more than the 64 KiB a launch gets without hipFuncSetAttribute"""
    ex, err = _text_attention(B, T, heads, causal)
    print("T %d B %d heads %d causal %d: attention error / bound %.3f, max |error| %.2e" % (T, B, heads, causal, ex, err))
    assert ex <= 1


@pytest.mark.parametrize("causal", [0, 1])
def test_text_attention_with_scores_of_fourteen_rescales_its_running_maximum(causal):
    ex, err = _text_attention(2, 128, 8, causal, q_scale=3.0)
    print("T 128 causal %d, q x 3: attention error / bound %.3f, max |error| %.2e" % (causal, ex, err))
    assert ex <= 1


def test_text_attention_refuses_no_token_and_more_than_128_and_launches_nothing():
    E = env()
    p = E.L.ptr
    heads, W = 8, 512
    qkv, out = torch.zeros(1, 129, 3 * W, device=E.dev), torch.full((1, 129, W), SENTINEL, device=E.dev)
    torch.cuda.synchronize()
    for T in (0, 129):
        assert E.lib.avc_text_attention_fwd(p(qkv), p(out), 1, T, W, heads, 1, E.st) != 0, T
        assert "1 <= T <= 128" in E.lib.avc_last_error().decode() and torch.cuda.current_stream().query(), T
    assert (out == SENTINEL).all()
