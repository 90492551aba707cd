"""avc_weight_grad_all / avc_weight_grad_reduce (csrc/avc_wgrad.hip) on their own, through the C ABI, against tests/wgrad_restatement.py.

The kernel is a contraction with fp32 accumulation.  On small-integer panels every product and every partial sum is an integer below
2^24 (asserted on the very same inputs by tests/test_wgrad_cpu.py), so the result does not depend on the order of the sums or on the
rounding of the matrix core's adder and the comparison is bit for bit, through an int32 view, sentinel-filled surroundings included.
On the panels a real backward pass leaves, the bound is the accumulation's own: |err| <= n 2^-23 sum |a| |b| per element for the n
points of a split (products of two bf16 values are exact in fp32; 2^-23 rather than 2^-24 because the adder is not documented to round
to nearest).  Measured figures: profiles/r14_wgrad_tests.md."""
import numpy as np
import pytest
import torch

from avatarclip_amd import packing as PK
from tests import wgrad_restatement as W

gpu = pytest.mark.gpu
SENTINEL = 0x7FA5C3D2          # a NaN pattern no sum of integers produces

E_SHAPE = b"avc_weight_grad_all: 1 <= ta <= 8, 1 <= tb <= 9 (or the 9 x 9 product)"
E_NULL = b"avc_weight_grad_all: fpanels / gpanels == NULL"
E_MANY = b"avc_weight_grad_all: too many pairs"
E_TYPE = b"avc_weight_grad_all: operand types are 0 (F region) or 1 (G region)"
E_TILES = b"avc_weight_grad_all: a pair's tiles lie outside their region"
E_OUT = b"avc_weight_grad_all: a pair's products lie outside out_stride"
E_BIAS = b"avc_weight_grad_all: a pair's bias sums lie outside bias_stride"
E_MULT4 = b"avc_weight_grad_reduce: sizes and strides must be multiples of 4 floats"


def _lib():
    from avatarclip_amd import lib as L
    return L, L.load()


def _region(bits, region_tiles, typ, dev):
    """the region on the device behind BASE_BLOCKS blocks of poison; -> (tensor, pointer to block 0).  The allocation ends with the last
    block."""
    poison = W.to_bits([W.POISON if typ == W.F16 else W.POISON_BF16], typ)[0]
    lead = np.full(W.BASE_BLOCKS * region_tiles * W.TILE_U16, poison, np.uint16)
    t = torch.from_numpy(np.concatenate([lead, bits]).view(np.int16)).to(dev)
    return t, t.data_ptr() + W.BASE_BLOCKS * region_tiles * 2048


def _sentinel(rows, cols, dev):
    return torch.full((rows, cols), SENTINEL, dtype=torch.int32, device=dev)


def _launch(lc, nsplit, dev):
    """two launches on the same inputs into sentinel-filled buffers with two spare rows -> (partial, bias_partial) as int32 on the host"""
    L, lib = _lib()
    ft, fptr = _region(lc.fbits, lc.ftiles, W.F16, dev)
    gt, gptr = _region(lc.gbits, lc.gtiles, W.BF16, dev)
    pairs = np.ascontiguousarray(lc.pairs, np.int32)
    outs = []
    for rep in range(2):
        po, pb = _sentinel(nsplit + 2, lc.out_stride, dev), _sentinel(nsplit + 2, lc.bias_stride, dev)
        L.check(lib.avc_weight_grad_all(fptr, lc.ftiles, gptr, lc.gtiles, len(pairs), pairs.ctypes.data, lc.nblk, po.data_ptr(),
                                        pb.data_ptr(), nsplit, lc.out_stride, lc.bias_stride, L.stream()), "avc_weight_grad_all")
        outs.append((po, pb))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two launches, different bits"
    return outs[0][0].cpu(), outs[0][1].cpu()


def _as_bits(x):
    x = np.asarray(x, np.float64) + 0.0          # (-0 -> +0)
    f = x.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), x)
    return f.view(np.int32)


def _expected(lc, nsplit, convert=True):
    """what the two buffers must hold, sentinel included"""
    eo = np.full((nsplit + 2, lc.out_stride), SENTINEL, np.int32)
    eb = np.full((nsplit + 2, lc.bias_stride), SENTINEL, np.int32)
    bounds = W.splits(lc.nblk, nsplit)
    cache = {}
    for pair in lc.pairs.tolist():
        pa, ta, pb, tb, oo, bo, tya, tyb = pair
        key = (pa, ta, pb, tb, tya, tyb)
        if key not in cache:
            cache[key] = [W.pair_reference(lc.fbits, lc.ftiles, lc.gbits, lc.gtiles, pair, bounds[s], bounds[s + 1], convert=convert)
                          for s in range(nsplit)]
        for s, (out, bias) in enumerate(cache[key]):
            eo[s, oo:oo + ta * tb * 1024] = _as_bits(out)
            if bo >= 0:
                eb[s, bo:bo + 32 * ta] = _as_bits(bias)
    return torch.from_numpy(eo), torch.from_numpy(eb)


def _where(lc, nsplit, got, exp, bias):
    """a readable account of the first mismatch"""
    bad = np.argwhere(got.numpy() != exp.numpy())
    s, j = (int(v) for v in bad[0])
    for k, (pa, ta, pb, tb, oo, bo, tya, tyb) in enumerate(lc.pairs.tolist()):
        lo, n = (bo, 32 * ta) if bias else (oo, ta * tb * 1024)
        if s < nsplit and lo >= 0 and lo <= j < lo + n:
            return "%d mismatches, first: %s of pair %d %r, split %d of %d (blocks %r), element %d: got 0x%08x, expected 0x%08x" % (
                len(bad), "bias" if bias else "product", k, (pa, ta, pb, tb, oo, bo, tya, tyb), s, nsplit, W.splits(lc.nblk, nsplit),
                j - lo, int(got[s, j]) & 0xFFFFFFFF, int(exp[s, j]) & 0xFFFFFFFF)
    return "%d mismatches, first outside every pair's area: row %d, float %d: 0x%08x" % (len(bad), s, j, int(got[s, j]) & 0xFFFFFFFF)


def _check(lc, nsplit, dev):
    po, pb = _launch(lc, nsplit, dev)
    eo, eb = _expected(lc, nsplit)
    assert torch.equal(po, eo), _where(lc, nsplit, po, eo, False)
    assert torch.equal(pb, eb), _where(lc, nsplit, pb, eb, True)
    return po, pb


@gpu
@pytest.mark.parametrize("nblk,nsplit,types,seed", list(W.integer_cases()))
def test_integer_panels_every_shape_bit_for_bit(nblk, nsplit, types, seed):
    """every accepted (ta, tb), with and without bias, up to 24 pairs per launch with shuffled offsets, poison in every tile no pair
    names, both stride choices, a panel pointer some blocks into its buffer; splits of 0 .. 9 blocks (the ring holds 4)"""
    dev = torch.device("cuda")
    n = 0
    for lc in W.integer_launches(nblk, types, seed):
        _check(lc, nsplit, dev)
        n += len(lc.pairs)
    assert n == 2 * len(W.ALL_SHAPES)


@gpu
@pytest.mark.parametrize("nblk,nsplit,types,seed", list(W.rounding_cases()))
def test_f16_operands_are_rounded_to_bf16_before_the_product(nblk, nsplit, types, seed):
    """f16 integers up to 1023 (ties included) against [-4, 4]: one shape per dispatcher body, the f16 operand on either side, the bias
    sums taken after the conversion"""
    dev = torch.device("cuda")
    for lc in W.rounding_launches(nblk, types, seed):
        po, pb = _check(lc, nsplit, dev)
        eo, eb = _expected(lc, nsplit, convert=False)       # the test can tell: without the conversion the figures differ
        assert not torch.equal(po, eo)
        if types[0] == W.F16:
            assert not torch.equal(pb, eb)


@gpu
@pytest.mark.parametrize("small", [True, False])
@pytest.mark.parametrize("nblk,nsplit", W.PRODUCTION_SPLITS)
def test_production_pair_tables_bit_for_bit(small, nblk, nsplit):
    """packing.region_local_pairs of both nets, real FTILES / GTILES, one launch, the whole [gout | gbias]"""
    dev = torch.device("cuda")
    spec = PK.SMALL if small else PK.FULL
    lc = W.production_launch(spec, nblk, 300 + W.PRODUCTION_SPLITS.index((nblk, nsplit)))
    lay = PK.layout_for(spec)
    assert (lc.ftiles, lc.gtiles) == (lay.panel["FTILES"], lay.panel["GTILES"]) and (small or (lc.ftiles, lc.gtiles) == (89, 83))
    po, pb = _check(lc, nsplit, dev)
    # the table tiles [0, gout_size) and [0, gbias_size) without a gap: nothing of either is left unwritten
    assert not (po[:nsplit, :lay.gout_size] == SENTINEL).any() and not (pb[:nsplit, :lay.gbias_size] == SENTINEL).any()


@gpu
@pytest.mark.parametrize("ns", [1, 7, 8, 9, 17])
def test_reduce_sums_integer_partials_exactly(ns):
    """avc_weight_grad_reduce: acc (+)= sum over the splits, exact on integers; the unroll-by-8 tail, accumulate 0 / 1, with and without
    bias sums; rows past ns and floats past the sizes are not read, nothing past gout_size + gbias_size is written"""
    L, lib = _lib()
    dev = torch.device("cuda")
    rng = np.random.default_rng(ns)
    G, B, pad = 4 * (256 * 3 + 5), 4 * 37, 12        # more than one workgroup of 4-float threads, a ragged last one
    po = rng.integers(-2 ** 17, 2 ** 17, size=(ns + 1, G + pad)).astype(np.float32)
    pb = rng.integers(-2 ** 14, 2 ** 14, size=(ns + 1, B + pad)).astype(np.float32)
    po[ns], po[:, G:], pb[ns], pb[:, B:] = np.nan, np.nan, np.nan, np.nan
    prev = rng.integers(-2 ** 17, 2 ** 17, size=G + B).astype(np.float32)
    dpo, dpb = torch.from_numpy(po).to(dev), torch.from_numpy(pb).to(dev)
    for accumulate in (0, 1):
        for gb in (0, B):
            acc = _sentinel(1, G + B + 64, dev).reshape(-1)
            acc[:G + gb] = torch.from_numpy(prev[:G + gb].view(np.int32)).to(dev)
            L.check(lib.avc_weight_grad_reduce(dpo.data_ptr(), dpb.data_ptr() if gb else None, ns, G + pad, B + pad, G, gb,
                                               acc.data_ptr(), accumulate, L.stream()), "avc_weight_grad_reduce")
            torch.cuda.synchronize()
            exp = np.concatenate([po[:ns, :G].astype(np.float64).sum(0), pb[:ns, :gb].astype(np.float64).sum(0)])
            if accumulate:
                exp = exp + prev[:G + gb]
            assert np.abs(exp).max() < 2 ** 24
            want = np.full(G + B + 64, SENTINEL, np.int32)
            want[:G + gb] = _as_bits(exp)
            assert torch.equal(acc.cpu(), torch.from_numpy(want)), (accumulate, gb)
    # sizes and strides that are no multiples of 4 floats are refused on the host
    acc = _sentinel(1, G + B + 64, dev).reshape(-1)
    for args in ((G + pad, B + pad, G - 2, B), (G + pad, B + pad, G, B - 1), (G + pad - 1, B + pad, G, B), (G + pad, B + pad + 2, G, B)):
        assert lib.avc_weight_grad_reduce(dpo.data_ptr(), dpb.data_ptr(), ns, *args, acc.data_ptr(), 0, L.stream()) == 1
        assert lib.avc_last_error() == E_MULT4
    torch.cuda.synchronize()
    assert (acc == SENTINEL).all()


@gpu
def test_bad_arguments_are_refused_on_the_host_and_nothing_is_launched():
    """shapes the dispatcher has no body for, too many pairs, NULL panels (the present error texts) and every way a pair table can
    leave its buffers: types outside {0, 1}, tile ranges outside their region, products or bias sums outside the split's row"""
    L, lib = _lib()
    dev = torch.device("cuda")
    ftiles, gtiles, nblk, nsplit = 20, 12, 2, 2
    ft = torch.zeros(nblk * ftiles * 1024, dtype=torch.int16, device=dev)
    gt = torch.zeros(nblk * gtiles * 1024, dtype=torch.int16, device=dev)
    out_stride, bias_stride = 81 * 1024, 9 * 32
    po, pb = _sentinel(nsplit, out_stride, dev), _sentinel(nsplit, bias_stride, dev)

    def call(pairs, fptr=ft.data_ptr(), gptr=gt.data_ptr(), nblk_=nblk):
        pairs = np.ascontiguousarray(np.array(pairs, dtype=np.int32).reshape(-1, 8))
        return lib.avc_weight_grad_all(fptr, ftiles, gptr, gtiles, len(pairs), pairs.ctypes.data, nblk_, po.data_ptr(), pb.data_ptr(),
                                       nsplit, out_stride, bias_stride, L.stream())

    ok = [2, 4, 1, 5, 0, 0, 0, 1]                   # pa, ta, pb, tb, out_off, bias_off, type_a, type_b
    refused = [
        ([2, 0, 1, 5, 0, 0, 0, 1], E_SHAPE),        # ta = 0
        ([2, 9, 1, 5, 0, 0, 0, 1], E_SHAPE),        # ta = 9 with tb != 9
        ([2, 4, 1, 10, 0, 0, 0, 1], E_SHAPE),       # tb = 10
        ([2, 4, 1, 0, 0, 0, 0, 1], E_SHAPE),        # tb = 0
        ([ok] * 25, E_MANY),
        ([2, 4, 1, 5, 0, 0, 2, 1], E_TYPE),
        ([2, 4, 1, 5, 0, 0, 0, -1], E_TYPE),
        ([-1, 4, 1, 5, 0, 0, 0, 1], E_TILES),       # pa < 0
        ([17, 4, 1, 5, 0, 0, 0, 1], E_TILES),       # pa + ta = 21 > 20 F tiles
        ([2, 4, -2, 5, 0, 0, 0, 1], E_TILES),       # pb < 0
        ([2, 4, 8, 5, 0, 0, 0, 1], E_TILES),        # pb + tb = 13 > 12 G tiles
        ([13, 4, 1, 5, 0, 0, 1, 0], E_TILES),       # A in the G region: 13 + 4 > 12, though it would fit the F region
        ([2, 9, 4, 9, 0, 0, 0, 1], E_TILES),        # the 9 x 9 product: pb + 9 = 13 > 12
        ([2, 4, 1, 5, 61 * 1024 + 4, 0, 0, 1], E_OUT),      # out_off + 20 * 1024 > out_stride
        ([2, 4, 1, 5, -1024, 0, 0, 1], E_OUT),
        ([2, 4, 1, 5, 0, 5 * 32 + 1, 0, 1], E_BIAS),        # bias_off + 4 * 32 > bias_stride
        ([ok, [2, 4, 1, 5, 0, 0, 0, 3]], E_TYPE),           # a bad entry behind a good one
    ]
    for pairs, text in refused:
        assert call(pairs) == 1, pairs
        assert lib.avc_last_error() == text, (pairs, lib.avc_last_error())
    assert call(ok, fptr=None) == 1 and lib.avc_last_error() == E_NULL
    assert call(ok, gptr=None) == 1 and lib.avc_last_error() == E_NULL
    assert call(ok, nblk_=0) == 0                    # nothing to contract: no launch, no store
    torch.cuda.synchronize()
    assert (po == SENTINEL).all() and (pb == SENTINEL).all()
    # the limits themselves are accepted: the last tiles of both regions, products and bias sums that end with the row
    L.check(call([16, 4, 7, 5, 61 * 1024, 5 * 32, 0, 1]), "avc_weight_grad_all")
    torch.cuda.synchronize()
    assert (po[:, 61 * 1024:] == 0).all() and (po[:, :61 * 1024] == SENTINEL).all()      # (zero panels)
    assert (pb[:, 5 * 32:] == 0).all() and (pb[:, :5 * 32] == SENTINEL).all()
    L.check(call([3, 9, 11, 9, 0, -1, 1, 0]), "avc_weight_grad_all")
    torch.cuda.synchronize()
    assert (po == 0).all() and (pb[:, :5 * 32] == SENTINEL).all()


def _engine_pass(eng, pk, R, S, dev):
    """training forward + backward of R x S points in one slab -> (grad, F panels, G panels, partials, bias partials, nblk, ns)"""
    from tests.engine_cases import _inputs
    ro, rd, z, dsdf, dn, drgb = _inputs(R, S, dev)
    _, _, rgbf = eng.points_fwd_train(pk, ro, rd, z, 2 / 32)
    assert eng.plan(R, S) == (R, R)
    grad = eng.points_bwd(pk, ro, rd, z, 2 / 32, dsdf, dn, drgb, rgbf, panels_valid=True).clone()
    torch.cuda.synchronize()
    nblk = (R * S + 31) // 32
    ns = max(1, min(eng.WG_MAX_SPLITS, nblk // eng.WG_BLOCKS_PER_SPLIT, nblk))
    fp = eng._fpanels[:nblk * eng.fwd_tiles * 2048].cpu().numpy().view(np.uint16)
    gp = eng._gpanels[:nblk * eng.grad_tiles * 2048].cpu().numpy().view(np.uint16)
    return grad, fp, gp, eng._partials[:ns].cpu().numpy(), eng._bpartials[:ns].cpu().numpy(), nblk, ns


@gpu
@pytest.mark.parametrize("small", [True, False])
def test_real_panels_with_a_ragged_tail_and_uneven_splits(small, monkeypatch):
    """The kernel on the panels of a real backward pass: 37 rays x 33 samples = 1221 points = 39 blocks, 5 of 32 rows used in the last
    one, 9 uneven splits.  Every pair of the real table, every split, against float64 within the accumulation's own bound.
    The tail contract the engine relies on: for the unused rows of the last block every pair has an operand whose rows are exactly
    zero (csrc/avc_bwd_body.h: vmask and the selections behind it) while the other one is finite, and every operand that feeds a bias
    sum is zero there.  Stale rows -- the same ray set after a larger one has filled the buffers -- change no bit of the gradient."""
    from avatarclip_amd.engine import Engine
    from tests.engine_cases import _nets
    dev = torch.device("cuda")
    monkeypatch.setattr(Engine, "WG_BLOCKS_PER_SPLIT", 4)
    ren = _nets(small, dev)
    eng = ren.engine
    pk = eng.pack(ren.flat_params())
    R, S = 37, 33
    grad, fp, gp, po, pb, nblk, ns = _engine_pass(eng, pk, R, S, dev)
    assert (nblk, ns, R * S - 32 * (nblk - 1)) == (39, 9, 5)
    bounds = W.splits(nblk, ns)
    assert len({b1 - b0 for b0, b1 in zip(bounds, bounds[1:])}) > 1
    ft, gtl = eng.fwd_tiles, eng.grad_tiles
    pairs = PK.region_local_pairs(eng.dl.lay)
    assert np.isfinite(po).all() and np.isfinite(pb).all()
    worst = 0.0
    for pair in pairs.tolist():
        pa, ta, pb_, tb, oo, bo, tya, tyb = pair
        # the tail contract, on the raw tiles
        A, B = W.operands(fp, ft, gp, gtl, pair, nblk - 1, nblk, convert=False)
        assert np.isfinite(A).all() and np.isfinite(B).all()
        assert not A[5:].any() or not B[5:].any(), ("both operands non-zero in the unused rows", pair)
        if bo >= 0:
            assert not A[5:].any(), ("bias operand non-zero in the unused rows", pair)
        for s in range(ns):
            b0, b1 = bounds[s], bounds[s + 1]
            ref, rbias = W.pair_reference(fp, ft, gp, gtl, pair, b0, b1)
            mag, mbias = W.pair_reference(fp, ft, gp, gtl, pair, b0, b1, magnitude=True)
            n = 32 * (b1 - b0)
            checks = [(po[s, oo:oo + ta * tb * 1024], ref, mag)]
            if bo >= 0:
                checks.append((pb[s, bo:bo + 32 * ta], rbias, mbias))
            for got, want, m in checks:
                err, lim = np.abs(got.astype(np.float64) - want), n * 2.0 ** -23 * m
                ratio = float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0
                worst = max(worst, ratio)
                assert (err <= lim).all(), (pair, s, ratio, float(err.max()), int((err > lim).sum()))
    print("weight-gradient kernel on real panels (%s net): worst err / bound = %.4f" % ("small" if small else "full", worst))
    assert worst > 0, "an fp32 accumulation of a few hundred products is not exact on real data: is the comparison looking at the kernel's output?"
    # stale rows: a larger ray set fills the buffers with other data, then the same 37 rays again
    _engine_pass(eng, pk, 64, S, dev)
    grad2, fp2, gp2, po2, pb2, _, _ = _engine_pass(eng, pk, R, S, dev)
    assert np.array_equal(po2.view(np.int32), po.view(np.int32)) and np.array_equal(pb2.view(np.int32), pb.view(np.int32))
    assert torch.equal(grad2.view(torch.int32), grad.view(torch.int32))
