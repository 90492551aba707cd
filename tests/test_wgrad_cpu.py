"""tests/wgrad_restatement.py against plain numpy, and the exactness premise of tests/test_gpu_wgrad.py on the inputs that file
launches (no GPU)."""
import numpy as np
import pytest

from avatarclip_amd import packing as PK
from tests import wgrad_restatement as W


@pytest.mark.parametrize("typ", [W.F16, W.BF16])
def test_tile_round_trip_and_element_order(typ):
    rng = np.random.default_rng(typ)
    a = rng.integers(-256, 257, size=(32, 32)).astype(np.float64)
    t = W.encode_tile(a, typ)
    assert t.dtype == np.uint16 and t.shape == (1024,)
    assert np.array_equal(W.decode_tile(t, typ), a)
    # the rule itself, element by element
    for s in range(2):
        for h in range(2):
            for p in (0, 5, 31):
                for j in range(8):
                    bits = t[((2 * s + h) * 32 + p) * 8 + j:][:1]
                    assert W.from_bits(bits, typ)[0] == a[p, PK.frag_feature(s, h, j)]
    # 1.0 is 0x3C00 as f16 and 0x3F80 as bf16
    one = W.encode_tile(np.ones((32, 32)), typ)
    assert (one == (0x3C00 if typ == W.F16 else 0x3F80)).all()
    # a region: block b, tile t at 16-bit element (b * region_tiles + t) * 1024
    v = rng.integers(-256, 257, size=(3, 5, 32, 32)).astype(np.float64)
    buf = W.panels(5, 3, typ, [(0, v)])
    assert buf.shape == (3 * 5 * 1024,)
    for b, tl in ((0, 0), (1, 4), (2, 2)):
        assert np.array_equal(buf[(b * 5 + tl) * 1024:][:1024], W.encode_tile(v[b, tl], typ))
    got = W.read_panels(buf, 5, typ, 1, 3, 1, 3)
    assert np.array_equal(got, v[1:3, :, :, :][:, 1:4].transpose(0, 2, 1, 3).reshape(64, 96))


def test_rounding_to_bf16_is_nearest_even():
    x = np.array([514, 518, 1023, -514, -518, 256, 257, 258, 259, 3, 0], np.float32)
    assert W.round_to_bf16(x).tolist() == [512, 520, 1024, -512, -520, 256, 256, 258, 260, 3, 0]
    # against torch's conversion on every integer the rounding case uses
    import torch
    v = np.arange(-1023, 1024).astype(np.float32)
    assert np.array_equal(W.round_to_bf16(v), torch.from_numpy(v).to(torch.bfloat16).float().numpy())
    assert W.POISON_BF16 == float(torch.tensor(W.POISON).to(torch.bfloat16)) and np.isfinite(np.float16(W.POISON))


@pytest.mark.parametrize("types", W.TYPE_COMBOS)
def test_pair_reference_is_a_transposed_product(types):
    """pair_reference == einsum of the dense operands for every pair shape, over a sub-range of the blocks"""
    rng = np.random.default_rng(7)
    ftiles, gtiles, nblk = 21, 23, 3
    vals = [rng.integers(-200, 201, size=(nblk, n, 32, 32)).astype(np.float64) for n in (ftiles, gtiles)]
    vals[0] *= 5                                   # f16 integers up to 1000: the conversion matters
    fp, gp = W.panels(ftiles, nblk, W.F16, [(0, vals[0])]), W.panels(gtiles, nblk, W.BF16, [(0, vals[1])])
    for ta, tb in W.ALL_SHAPES:
        pa, pb = 1, 11
        pair = (pa, ta, pb, tb, 0, 0) + types
        out, bias = W.pair_reference(fp, ftiles, gp, gtiles, pair, 1, 3)
        dense = []
        for p0, nt, typ in ((pa, ta, types[0]), (pb, tb, types[1])):
            d = vals[typ][1:3, p0:p0 + nt].transpose(0, 2, 1, 3).reshape(64, 32 * nt)
            dense.append(W.round_to_bf16(d.astype(np.float32)).astype(np.float64) if typ == W.F16 else d)
        M = np.einsum("pi,pk->ik", dense[0], dense[1])
        assert out.shape == (ta * tb * 1024,) and bias.shape == (32 * ta,)
        assert np.array_equal(bias, dense[0].sum(0))
        o4 = out.reshape(ta, tb, 64, 16)
        for lane in (0, 1, 31, 32, 45, 63):
            for r in range(16):
                assert np.array_equal(o4[:, :, lane, r], M.reshape(ta, 32, tb, 32)[:, PK.acc_row(r, lane >> 5), :, lane & 31])
        assert np.array_equal(np.sort(out), np.sort(M.reshape(-1)))      # every product exactly once


def test_split_bounds():
    assert W.splits(37, 5) == [0, 7, 14, 22, 29, 37]
    assert W.splits(3, 5) == [0, 0, 1, 1, 2, 3]
    assert W.splits(64, 7) == [0, 9, 18, 27, 36, 45, 54, 64]
    sizes = set()
    for nblk, nsplit in W.SPLIT_CASES:
        b = W.splits(nblk, nsplit)
        assert b[0] == 0 and b[-1] == nblk and all(x <= y for x, y in zip(b, b[1:]))
        sizes |= {y - x for x, y in zip(b, b[1:])}
    assert sizes >= {0, 1, 2, 3, 4, 5, 7, 8, 9}      # the ring's start-up (depth 4), its first wrap-around and empty splits


def _check_launch(L):
    m_out, m_bias = W.exactness_margin(L)
    assert m_out < 2 ** 24 and m_bias < 2 ** 24
    # the table stays inside its buffers and names no poison tile; output areas are disjoint
    poison_f, poison_g = W.to_bits([W.POISON], W.F16)[0], W.to_bits([W.POISON_BF16], W.BF16)[0]
    outs, biases = [], []
    for pa, ta, pb, tb, oo, bo, tya, tyb in L.pairs.tolist():
        for p0, nt, typ in ((pa, ta, tya), (pb, tb, tyb)):
            rt, buf, poison = (L.gtiles, L.gbits, poison_g) if typ else (L.ftiles, L.fbits, poison_f)
            assert 0 <= p0 and p0 + nt <= rt
            tiles = buf.reshape(L.nblk, rt, 1024)[:, p0:p0 + nt]
            assert not (tiles == poison).any()
        outs.append((oo, oo + ta * tb * 1024))
        assert oo % 4 == 0 and outs[-1][1] <= L.out_stride
        if bo >= 0:
            biases.append((bo, bo + 32 * ta))
            assert biases[-1][1] <= L.bias_stride
    for spans in (outs, biases):
        spans.sort()
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert len(L.pairs) <= W.MAX_PAIRS and L.out_stride % 4 == 0 and L.bias_stride % 4 == 0
    return m_out, m_bias


@pytest.mark.parametrize("only", W.TYPE_COMBOS)
def test_integer_cases_are_exact_in_fp32_and_cover_every_shape(only):
    """max sum |a| |b| < 2^24 and max sum |a| < 2^24 on the generated inputs: every product and partial sum is an integer fp32 holds"""
    worst = 0.0
    for nblk, nsplit, types, seed in W.integer_cases():
        if types != only:
            continue
        seen = set()
        strides = set()
        for L in W.integer_launches(nblk, types, seed):
            m_out, m_bias = _check_launch(L)
            assert m_out <= 2 ** 17 and m_bias <= 2 ** 14      # 2048 points x 64, 2048 x 8
            worst = max(worst, m_out)
            seen |= {(ta, tb, bo >= 0) for _, ta, _, tb, _, bo, _, _ in L.pairs.tolist()}
            strides.add((L.ftiles, L.gtiles))
            assert (L.pairs[:, 6:] == types).all()
            # unused tiles around every operand range hold poison
            for pa, ta, pb, tb, _, _, tya, tyb in L.pairs.tolist():
                for p0, nt, typ in ((pa, ta, tya), (pb, tb, tyb)):
                    rt, buf = (L.gtiles, L.gbits) if typ else (L.ftiles, L.fbits)
                    t = buf.reshape(L.nblk, rt, 1024)
                    poison = t[0, 0, 0]
                    assert (t[:, p0 - 1] == poison).all() and (p0 + nt == rt or (t[:, p0 + nt] == poison).all())
        assert seen == {(ta, tb, b) for ta, tb in W.ALL_SHAPES for b in (False, True)}
        assert strides == set(W.STRIDES)
    assert worst > 2 ** 14       # (and the sums are not trivially small)


def test_rounding_and_production_cases_are_exact_in_fp32():
    for nblk, nsplit, types, seed in W.rounding_cases():
        shapes = set()
        for L in W.rounding_launches(nblk, types, seed):
            m_out, m_bias = _check_launch(L)
            assert m_out <= 2 ** 22 and m_bias <= 2 ** 20
            shapes |= {(ta, tb) for _, ta, _, tb, _, _, _, _ in L.pairs.tolist()}
            assert (L.pairs[:, 5] >= 0).all()
            # the f16 side really needs the rounding: the reference without it differs
            pair = L.pairs[0]
            assert not np.array_equal(W.pair_reference(L.fbits, L.ftiles, L.gbits, L.gtiles, pair, 0, nblk)[0],
                                      W.pair_reference(L.fbits, L.ftiles, L.gbits, L.gtiles, pair, 0, nblk, convert=False)[0])
            f = W.from_bits(L.fbits, W.F16)
            named = f[f != W.POISON]
            assert named.max() > 1000 and named.min() < -1000 and (np.abs(named) % 4 == 2)[np.abs(named) > 512].any()     # ties
        assert shapes == set(W.BODY_SHAPES)
    for spec in (PK.SMALL, PK.FULL):
        for k, (nblk, nsplit) in enumerate(W.PRODUCTION_SPLITS):
            L = W.production_launch(spec, nblk, 300 + k)
            m_out, m_bias = W.exactness_margin(L)          # (the real table shares tiles between pairs: no poison around them)
            assert m_out <= 37 * 32 * 64 < 2 ** 24 and m_bias <= 37 * 32 * 8
