"""Plain-torch restatements for csrc/avc_vit.hip and csrc/avc_vit_gemm.hip (CPU only; tests/test_gpu_clip_kernels.py holds the kernels
against them, tests/test_clip_kernel_restatement_cpu.py holds this file against torch).

Packed operands.  An [M, K] activation is stored as [row tile][k-step][half][row][8] bf16: element (r, c) is slot c & 7 of lane
(r & 31, (c >> 3) & 1) of k-step c >> 4 of row tile r >> 5, 1 KiB per (tile, k-step).  Up to 128 rows the kernels read ceil(M / 32)
tiles, above that whole groups of four (avc_vit_workspace_bytes).

Integer cases.  x and w are integers in [-4, 4], bias and residual integers in [-64, 64], K <= 4096: every operand is exact in bf16,
every product and every partial sum of a row is an integer of magnitude at most 16 K + 128 < 2^24, so fp32 accumulation is exact IN
ANY ORDER of the sums (the argument of tests/test_gpu_wgrad.py) and a kernel has to return the int64 matmul bit for bit.  bf16 of an
exact integer is one determined rounding (RNE), so packed outputs are compared by bits too.

Thinned cases, for the activation epilogues.  x is non-zero (an integer of [-4, 4]) at rate 8 / K, w is in {-1, 0, 1}, the bias in
[-2, 2]: the pre-activation is still an exact integer, and at least half of them lie in [-4, 4], where QuickGELU is not yet the
identity or zero (asserted by the builder on the reference).

Bounds.  FP32_SLACK: |got - ref| <= 2e-5 (1 + |ref|), the gate tests/test_gpu_clip.py holds avc_vit_ln_bwd to.  A packed bf16 result
of a non-integer value may in addition be half a bf16 ulp away: 2^-8 |ref|."""
import functools

import torch

FP32_SLACK = 2e-5
HALF_ULP_BF16 = 2.0 ** -8
X_MAX, W_MAX, B_MAX, K_MAX = 4, 4, 64, 4096
EXACT_BELOW = 2 ** 24


# ------------------------------------------------------------------------------------------------------------------- packed operands
def row_tiles(M):
    """32-row tiles of a packed operand of M rows: ceil(M / 32) up to 128 rows, whole groups of four above"""
    return (M + 31) // 32 if M <= 128 else ((M + 127) // 128) * 4


def unpack_rows(packed_uint8, nrows, N):
    """the first `nrows` rows of a packed operand, [row tile][k-step][half][row][8] -> [nrows, N] bf16"""
    mt = (nrows + 31) // 32
    t = packed_uint8[:mt * (N // 16) * 1024].view(torch.bfloat16).reshape(mt, N // 16, 2, 32, 8)
    return t.permute(0, 3, 1, 2, 4).reshape(mt * 32, N)[:nrows]


def pack_rows(x_bf16):
    """[M, K] bf16 -> the packed operand as flat uint8, row_tiles(M) tiles, the padding rows zero"""
    assert x_bf16.dtype == torch.bfloat16 and x_bf16.dim() == 2 and x_bf16.shape[1] % 16 == 0
    M, K = x_bf16.shape
    mt = row_tiles(M)
    full = torch.zeros(mt * 32, K, dtype=torch.bfloat16, device=x_bf16.device)
    full[:M] = x_bf16
    p = full.reshape(mt, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous()
    return p.reshape(-1).view(torch.uint8)


def bits(t):
    return t.contiguous().view(torch.int16)


# --------------------------------------------------------------------------------------------------------------------- integer cases
def _randint(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g)


@functools.lru_cache(maxsize=None)
def integer_case(M, N, K, seed=0):
    """x[M,K], w[N,K], bias[N], res[M,N] as fp32 integers and the int64 references: `plain` = x w^T, `bias` = plain + bias, `res` =
    plain + res, `full` = plain + bias + res.  Asserts that every partial sum stays below 2^24.  Cached: treat as read-only."""
    assert K <= K_MAX and K % 16 == 0 and N % 32 == 0
    g = torch.Generator().manual_seed(1000003 * seed + 4099 * M + 31 * N + K)
    x, w = _randint(g, -X_MAX, X_MAX, M, K), _randint(g, -W_MAX, W_MAX, N, K)
    b, r = _randint(g, -B_MAX, B_MAX, N), _randint(g, -B_MAX, B_MAX, M, N)
    plain = x @ w.t()
    assert plain.dtype == torch.int64
    # the largest magnitude any partial sum can reach in any order: sum |x w| over the row, plus bias and residual
    assert X_MAX * W_MAX * K + 2 * B_MAX < EXACT_BELOW
    ref = {"plain": plain, "bias": plain + b, "res": plain + r, "full": plain + b + r}
    assert all(int(v.abs().max()) < EXACT_BELOW for v in ref.values())
    return {"x": x.float(), "w": w.float(), "bias": b.float(), "res": r.float(), "ref": ref, "M": M, "N": N, "K": K}


def thinned_share(pre):
    """share of the pre-activations in [-4, 4]"""
    return float((pre.abs() <= 4).double().mean())


@functools.lru_cache(maxsize=None)
def thinned_case(M, N, K, seed=0):
    """x non-zero at rate 8 / K, w in {-1, 0, 1}, bias in [-2, 2]; `prod` = x w^T and `pre` = prod + bias as int64.  Asserts that at
    least half of the pre-activations lie in [-4, 4].  Cached: treat as read-only."""
    assert K <= K_MAX and K % 16 == 0 and N % 32 == 0
    g = torch.Generator().manual_seed(7000003 * seed + 4099 * M + 31 * N + K)
    keep = torch.rand(M, K, generator=g) < 8.0 / K
    x = _randint(g, -X_MAX, X_MAX, M, K) * keep
    w = _randint(g, -1, 1, N, K)
    b = _randint(g, -2, 2, N)
    prod = x @ w.t()
    pre = prod + b
    assert X_MAX * K + 2 < EXACT_BELOW and int(pre.abs().max()) < EXACT_BELOW
    share = thinned_share(pre)
    assert share >= 0.5, share
    return {"x": x.float(), "w": w.float(), "bias": b.float(), "prod": prod, "pre": pre, "share": share, "M": M, "N": N, "K": K}


# ------------------------------------------------------------------------------------------------------------------ fp64 restatements
def quickgelu(p):
    p = p.double()
    return p * torch.sigmoid(1.702 * p)


def quickgelu_grad(p):
    """d quickgelu / dp = s + 1.702 p s (1 - s), s = sigmoid(1.702 p)"""
    p = p.double()
    s = torch.sigmoid(1.702 * p)
    return s + 1.702 * p * s * (1 - s)


def layernorm(x, gamma, beta, eps):
    """LayerNorm over the last dimension, biased variance, eps inside the square root"""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def layernorm_bwd(dy, x, gamma, eps, residual_grad=None):
    """dx = rstd (g - mean(g) - xhat mean(g xhat)) (+ residual_grad), g = dy gamma, xhat = (x - mean) rstd"""
    dy, x, gamma = dy.double(), x.double(), gamma.double()
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xhat = (x - mean) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(-1, keepdim=True) - xhat * (g * xhat).mean(-1, keepdim=True))
    return dx if residual_grad is None else dx + residual_grad.double()


def attention(qkv, heads, causal):
    """qkv[B,T,3W] (q | k | v, head h at columns 64 h) -> out[B,T,W]: softmax(q k^T / 8 (+ causal mask)) v per head, float64"""
    B, T, W3 = qkv.shape
    W = W3 // 3
    assert W == heads * 64
    q, k, v = (t.reshape(B, T, heads, 64).permute(0, 2, 1, 3) for t in qkv.double().split(W, dim=-1))
    out = torch.empty(B, heads, T, 64, dtype=torch.float64)
    for i in range(T):
        jend = i + 1 if causal else T
        sc = (q[:, :, i:i + 1] * k[:, :, :jend]).sum(-1) * 0.125                 # [B, heads, jend]
        p = torch.exp(sc - sc.max(-1, keepdim=True).values)
        p = p / p.sum(-1, keepdim=True)
        out[:, :, i] = (p.unsqueeze(-1) * v[:, :, :jend]).sum(2)
    return out.permute(0, 2, 1, 3).reshape(B, T, W)


# ---------------------------------------------------------------------------------------------------------------------------- bounds
def max_abs_error(got, ref):
    return float((got.double().cpu() - ref.double().cpu()).abs().max())


def slack_excess(got, ref):
    """max of |got - ref| / (FP32_SLACK (1 + |ref|)): <= 1 passes"""
    got, ref = got.double().cpu(), ref.double().cpu()
    return float(((got - ref).abs() / (FP32_SLACK * (1 + ref.abs()))).max())


def half_ulp_excess(got_bf16, ref):
    """max of |got - ref| / (2^-8 |ref| + FP32_SLACK (1 + |ref|)) for a packed bf16 result: <= 1 passes, every element"""
    got, ref = got_bf16.double().cpu(), ref.double().cpu()
    return float(((got - ref).abs() / (HALF_ULP_BF16 * ref.abs() + FP32_SLACK * (1 + ref.abs()))).max())


# ---------------------------------------------------------------------------------------------------------------------- random inputs
def layernorm_inputs(M, seed=0, constant_row=None):
    """x = randn * 2 + 0.3 with channel 300 multiplied by 40 (the outlier channel of CLIP's residual stream), gamma, beta; with
    `constant_row` that row is the constant 3.0 (variance 0: only eps keeps it finite, LayerNorm gives beta)"""
    g = torch.Generator().manual_seed(911 * seed + M)
    x = torch.randn(M, 768, generator=g) * 2 + 0.3
    x[:, 300] *= 40
    if constant_row is not None:
        x[constant_row] = 3.0
    gamma = torch.randn(768, generator=g) * 0.2 + 1
    beta = torch.randn(768, generator=g)
    return x, gamma, beta


def attention_inputs(B, T, heads, seed=0, q_scale=1.0):
    g = torch.Generator().manual_seed(577 * seed + 131 * T + 7 * B + heads)
    qkv = torch.randn(B, T, 3 * heads * 64, generator=g)
    qkv[..., :heads * 64] *= q_scale
    return qkv
