"""avc_weight_grad_all on real-valued panels, bit for bit against digests of the library of the commit before the block loop of
csrc/avc_wgrad.hip was specialised for the shipped shapes.

tests/test_gpu_wgrad.py compares integer panels, which are exact in any order of the sums; these panels are not.  The f16 operands
carry subnormals and values next to 65504, the bf16 operands 64 binades, so a product added to another accumulator, a k-step taken
out of order, a block contracted before its copy has landed or a bias sum added in another order changes bits.  What must hold is
stated in the header of the kernel: every accumulator receives k-step 0, then k-step 1 of each block, blocks ascending, splits
unchanged.  tests/golden/wgrad_bits.json holds the seeds and the SHA-256 digests of `partial` and `bias_partial` (sentinel-filled
spare rows and gaps included), written by

    AVC_LIB_NAME=<library of the earlier commit> python -m tests.test_gpu_wgrad_bits --record tests/golden/wgrad_bits.json

(avatarclip_amd/build.py builds a second library beside the first with AVC_LIB_NAME / AVC_OBJ_SUFFIX).  Block counts 1 .. 5 and 37
against the ring of 4 and its peeled tail of 3; 1, 5 and nblk + 2 splits, the last with splits of 0 and 1 blocks."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

from avatarclip_amd import packing as PK
from tests import wgrad_restatement as W
from tests.test_gpu_wgrad import SENTINEL, _lib, _region, _sentinel

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_bits.json")
SEEDS = {"full": 7101, "small": 7102, "roles": 7103}
NBLKS = (1, 2, 3, 4, 5, 37)
SPLIT_KINDS = ("1", "5", "nblk+2")
# the products in which a wave's role is chosen before the block loop: 7 x 8 (the seventh A tile: waves wa = 0 only) in both operand
# orders, 8 x 9 (the ninth B tile: waves wb = 0 only), 9 x 9 with and without bias (the ninth A tile, the bias sums); F tiles, G tiles
# and (pa, ta, pb, tb, bias, type_a, type_b) on the full nets' strides
ROLE_STRIDES = (89, 83)
ROLE_ENTRIES = ((1, 7, 1, 8, True, 1, 0), (10, 7, 9, 8, False, 0, 1), (18, 9, 18, 9, True, 1, 0), (28, 9, 28, 9, False, 1, 0),
                (38, 8, 38, 9, True, 1, 0), (47, 8, 48, 8, True, 1, 0), (57, 8, 56, 8, False, 0, 1))
ROLE_SPLITS = ((5, 1), (9, 2))              # (nblk, nsplit)


def _f16_bits(rng, n):
    """n f16 patterns: finite, either sign; one in eight subnormal, one in eight in the top binade with the upper mantissa bits set
    (>= 65024), the others with an exponent field drawn evenly from 1 .. 30"""
    kind = rng.integers(0, 8, n)
    expo = np.where(kind == 0, 0, np.where(kind == 1, 30, rng.integers(1, 31, n)))
    mant = np.where(kind == 1, 0x3F0 | rng.integers(0, 16, n), rng.integers(0, 1024, n))
    return (rng.integers(0, 2, n) << 15 | expo << 10 | mant).astype(np.uint16)


def _bf16_bits(rng, n):
    """n bf16 patterns: finite, either sign, exponents 2^-40 .. 2^23, one in sixteen zero"""
    v = rng.integers(0, 2, n) << 15 | rng.integers(127 - 40, 127 + 24, n) << 7 | rng.integers(0, 128, n)
    return np.where(rng.integers(0, 16, n) == 0, 0, v).astype(np.uint16)


class _Case:
    pass


_cases = {}


def _case(name):
    """the 37-block panels and the pair table of `name`, made once; a launch on fewer blocks reads the first ones"""
    if name in _cases:
        return _cases[name]
    c = _Case()
    rng = np.random.default_rng(SEEDS[name])
    if name == "roles":
        c.ftiles, c.gtiles = ROLE_STRIDES
        rows, o, b = [], 0, 0
        for pa, ta, pb, tb, bias, tya, tyb in ROLE_ENTRIES:
            rows.append([pa, ta, pb, tb, o, b if bias else -1, tya, tyb])
            o += ta * tb * 1024 + 256
            b += (32 * ta + 8) if bias else 0
        c.pairs = np.array(rows, np.int32)
        c.out_stride, c.bias_stride = o + 1024, b + 64
    else:
        lay = PK.layout_for(PK.SMALL if name == "small" else PK.FULL)
        c.ftiles, c.gtiles = lay.panel["FTILES"], lay.panel["GTILES"]
        c.pairs = PK.region_local_pairs(lay)
        c.out_stride, c.bias_stride = lay.gout_size + 1024, lay.gbias_size + 64
    nblk = max(NBLKS)
    named = [np.zeros(c.ftiles, bool), np.zeros(c.gtiles, bool)]
    for pa, ta, pb, tb, _, _, tya, tyb in c.pairs:
        named[tya][pa:pa + ta] = True
        named[tyb][pb:pb + tb] = True
    c.bits = []
    for typ, tiles, gen, poison in ((W.F16, c.ftiles, _f16_bits, W.POISON), (W.BF16, c.gtiles, _bf16_bits, W.POISON_BF16)):
        buf = np.full((nblk, tiles, W.TILE_U16), W.to_bits([poison], typ)[0], np.uint16)      # tiles no pair names hold poison
        idx = np.nonzero(named[typ])[0]
        buf[:, idx] = gen(rng, nblk * len(idx) * W.TILE_U16).reshape(nblk, len(idx), W.TILE_U16)
        c.bits.append(buf)
    _cases[name] = c
    return c


def _nsplit(nblk, kind):
    return {"1": 1, "5": 5, "nblk+2": nblk + 2}[kind]


def _run(name, nblk, nsplit):
    """two launches on the first nblk blocks -> (partial, bias_partial) as int32 arrays on the host, the same bits both times"""
    L, lib = _lib()
    dev = torch.device("cuda")
    c = _case(name)
    ft, fptr = _region(c.bits[0][:nblk].reshape(-1), c.ftiles, W.F16, dev)
    gt, gptr = _region(c.bits[1][:nblk].reshape(-1), c.gtiles, W.BF16, dev)
    pairs = np.ascontiguousarray(c.pairs, np.int32)
    outs = []
    for rep in range(2):
        po, pb = _sentinel(nsplit + 2, c.out_stride, dev), _sentinel(nsplit + 2, c.bias_stride, dev)
        L.check(lib.avc_weight_grad_all(fptr, c.ftiles, gptr, c.gtiles, len(pairs), pairs.ctypes.data, nblk, po.data_ptr(),
                                        pb.data_ptr(), nsplit, c.out_stride, c.bias_stride, L.stream()), "avc_weight_grad_all")
        outs.append((po, pb))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two launches, different bits"
    return outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _table_digests(name, nblk, kind):
    po, pb = _run(name, nblk, _nsplit(nblk, kind))
    return [_sha(po), _sha(pb)]


def _role_digests(nblk, nsplit):
    """{"pair k tile i,j": digest over the splits of that output tile, "pair k bias": digest of its bias sums, "all": everything}"""
    po, pb = _run("roles", nblk, nsplit)
    c = _case("roles")
    out = {"all": _sha(po)[:16] + _sha(pb)[:16]}
    for k, (pa, ta, pb_, tb, oo, bo, tya, tyb) in enumerate(c.pairs.tolist()):
        for i in range(ta):
            for j in range(tb):
                lo = oo + (i * tb + j) * 1024
                out["pair %d tile %d,%d" % (k, i, j)] = _sha(po[:nsplit, lo:lo + 1024])[:16]
        if bo >= 0:
            out["pair %d bias" % k] = _sha(pb[:nsplit, bo:bo + 32 * ta])[:16]
    return out


def _golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["seeds"] == SEEDS, "tests/golden/wgrad_bits.json was recorded for other seeds"
    return g


@gpu
@pytest.mark.parametrize("kind", SPLIT_KINDS)
@pytest.mark.parametrize("nblk", NBLKS)
@pytest.mark.parametrize("name", ["full", "small"])
def test_real_valued_panels_of_the_shipped_tables_keep_their_bits(name, nblk, kind):
    """packing.region_local_pairs of both nets, real FTILES / GTILES, poison in every tile no pair names: `partial` and `bias_partial`
    byte for byte what the earlier library wrote"""
    want = _golden()["tables"]["%s nblk=%d nsplit=%s" % (name, nblk, kind)]
    got = _table_digests(name, nblk, kind)
    assert got[0] == want[0], "partial differs from the recorded bits"
    assert got[1] == want[1], "bias_partial differs from the recorded bits"


@gpu
@pytest.mark.parametrize("nblk,nsplit", ROLE_SPLITS)
def test_every_wave_role_keeps_the_bits_of_its_output_tiles(nblk, nsplit):
    """7 x 8 in both operand orders, 8 x 9, 9 x 9 with and without bias, 8 x 8 in both orders: every output tile and every pair's
    bias sums on their own, so that a failure names the tile (and with it the wave and its role)"""
    want = _golden()["roles"]["nblk=%d nsplit=%d" % (nblk, nsplit)]
    got = _role_digests(nblk, nsplit)
    assert sorted(got) == sorted(want)
    bad = [k for k in sorted(got) if got[k] != want[k] and k != "all"]
    assert not bad, "%d of %d differ from the recorded bits: %s" % (len(bad), len(got) - 1, ", ".join(bad[:12]))
    assert got["all"] == want["all"], "bits outside every pair's area differ"


def _record(path):
    g = {"seeds": SEEDS, "tables": {}, "roles": {}}
    for name in ("full", "small"):
        for nblk in NBLKS:
            for kind in SPLIT_KINDS:
                g["tables"]["%s nblk=%d nsplit=%s" % (name, nblk, kind)] = _table_digests(name, nblk, kind)
    for nblk, nsplit in ROLE_SPLITS:
        g["roles"]["nblk=%d nsplit=%d" % (nblk, nsplit)] = _role_digests(nblk, nsplit)
    with open(path, "w") as f:
        json.dump(g, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d + %d cases with %s" % (len(g["tables"]), len(g["roles"]), _lib()[0].lib_path()))


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    _record(sys.argv[2])
