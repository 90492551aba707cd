"""tests/panel_restatement.py without a GPU: the decoders of the operand panels and ReLU masks against the tile statement the
contraction tests already trust (tests/wgrad_restatement.py), and the comparison of tests/test_gpu_panels.py against the mistakes it is
there for -- at the very gates that test applies, on reference tiles carrying noise of the gates' size."""
import functools

import numpy as np
import pytest
import torch

from avatarclip_amd import packing as PK
from tests import panel_restatement as PR
from tests import wave_emulator as E
from tests import wgrad_restatement as W
from tests.test_gpu_panels import GATES, GATE_CAP, RELU_AMBIGUOUS_CAP, SAMPLE_DIST, gate

NETS = [True, False]
NBLK = 2


@functools.lru_cache(maxsize=None)
def _reference(small):
    """two blocks (2 rays x 32 samples) of the seeded net and inputs of the GPU tests -> (spec, layout, reference, inputs of the emulator)"""
    from avatarclip_amd.engine import flatten_dense_torch
    from tests.engine_cases import _inputs, _nets
    cpu = torch.device("cpu")
    ren = _nets(small, cpu)
    spec = PK.SMALL if small else PK.FULL
    flat = flatten_dense_torch(ren.sdf_network, ren.color_network, spec).detach().double().numpy()
    ro, rd, z, dsdf, dn, drgb = (a.numpy() for a in _inputs(NBLK, 32, cpu))
    args = (spec, flat, PR.midpoints(ro, rd, z, SAMPLE_DIST), dsdf.reshape(-1), dn.reshape(-1, 3), drgb.reshape(-1, 6))
    ref = PR.reference_blocks(*args)
    for a in ref.values():
        a.setflags(write=False)
    return spec, PK.layout_for(spec), ref, args


def _region(small, region):
    spec, lay, ref, _ = _reference(small)
    return lay, ref["F" if region == PR.F_REGION else "G"], lay.panel["FTILES" if region == PR.F_REGION else "GTILES"]


def _noisy(small, region, seed=0):
    """the reference through a raw region and back, with noise of 0.9 x gate x rms on every entry of every group"""
    lay, ref, ntiles = _region(small, region)
    rng = np.random.default_rng(seed)
    got = ref.copy()
    for group, t0, nt in PR.groups(lay, region):
        rms = np.sqrt(np.mean(ref[:, t0:t0 + nt] ** 2))
        got[:, t0:t0 + nt] += rng.uniform(-1, 1, size=got[:, t0:t0 + nt].shape) * 0.9 * gate(group) * rms
    return PR.decode(PR.encode(got, region), region, ntiles, NBLK)


def _failing(small, region, got):
    """the groups of a region that miss their gate"""
    lay, ref, _ = _region(small, region)
    out = []
    for group, t0, nt in PR.groups(lay, region):
        res = PR.compare(got[:, t0:t0 + nt], ref[:, t0:t0 + nt], group, PR.UNIT_ROUNDOFF[region])
        if not res.e_max <= gate(group):
            out.append((group, res))
    return out


def test_groups_cover_both_regions_and_the_small_net_has_no_second_colour_layer():
    for spec in (PK.SMALL, PK.FULL):
        lay = PK.layout_for(spec)
        for region, total in ((PR.F_REGION, lay.panel["FTILES"]), (PR.G_REGION, lay.panel["GTILES"])):
            g = PR.groups(lay, region)
            assert g[0][1] == 0 and all(a[1] + a[2] == b[1] for a, b in zip(g, g[1:])) and g[-1][1] + g[-1][2] == total
            assert set(n for n, _, _ in g) <= set(GATES)
        names = [n for n, _, _ in PR.groups(lay, PR.F_REGION) + PR.groups(lay, PR.G_REGION)]
        assert ("R2" in names, "D2" in names) == ((spec.NCMID == 1),) * 2
    assert (PK.layout_for(PK.FULL).panel["FTILES"], PK.layout_for(PK.FULL).panel["GTILES"]) == (89, 83)
    # every gate is 3 x the larger measured figure (to the table's three digits) and below the cap; SDF and DO are derived
    for name, (g, small, full) in GATES.items():
        top = max(v for v in (small, full) if v is not None)
        assert 0 <= g <= GATE_CAP and (abs(g - 3 * top) <= 0.005 * g if top > 0 else name in ("SDF", "DO")), name


@pytest.mark.parametrize("small", NETS)
def test_round_trip_through_a_raw_region(small):
    """encode (16-bit rounding) then decode returns the rounded tiles; fragment space <-> [points, features] is a bijection"""
    for region in (PR.F_REGION, PR.G_REGION):
        lay, ref, ntiles = _region(small, region)
        raw = PR.encode(ref, region)
        assert raw.dtype == np.uint16 and raw.size == NBLK * ntiles * W.TILE_U16
        back = PR.decode(raw, region, ntiles, NBLK)
        assert np.array_equal(back, PR.round16(ref, region))
        err = np.abs(back - ref)
        assert (err <= PR.UNIT_ROUNDOFF[region] * np.abs(ref) + (2.0 ** -25 if region == PR.F_REGION else 0)).all() and err.any()
        assert np.array_equal(PR.to_fragments(PR.to_dense(ref)), ref)


@pytest.mark.parametrize("small", NETS)
def test_decoder_agrees_with_the_operands_of_the_contraction(small):
    """the same raw regions through wgrad_restatement.operands (what the weight-gradient tests multiply) and through decode + to_dense:
    the same [points, features] matrices for every pair of the real table"""
    spec, lay, ref, _ = _reference(small)
    ft, gt = lay.panel["FTILES"], lay.panel["GTILES"]
    fp, gp = PR.encode(ref["F"], PR.F_REGION), PR.encode(ref["G"], PR.G_REGION)
    dense = {PR.F_REGION: PR.to_dense(PR.decode(fp, PR.F_REGION, ft, NBLK)), PR.G_REGION: PR.to_dense(PR.decode(gp, PR.G_REGION, gt, NBLK))}
    for pair in PK.region_local_pairs(lay).tolist():
        pa, ta, pb, tb, _, _, type_a, type_b = pair
        A, B = W.operands(fp, ft, gp, gt, pair, 0, NBLK, convert=False)
        for M, p0, nt, typ in ((A, pa, ta, type_a), (B, pb, tb, type_b)):
            mine = dense[typ][:, p0:p0 + nt].transpose(0, 2, 1, 3).reshape(NBLK * 32, nt * 32)       # [b][t][p][f] -> [b p][t f]
            assert M.shape == mine.shape and np.array_equal(M, mine) and M.any(), pair


@pytest.mark.parametrize("small", NETS)
def test_the_reference_tiles_are_the_emulators_fragments(small):
    """from_product_form undoes panel_store: the fragment pair that goes in comes out, and the product form contracts to the same
    weight gradient (so the reference tiles are the operands tests/test_packing_emulation.py proves against the analytic gradient)"""
    rng = np.random.default_rng(5)
    f0, f1 = rng.standard_normal((64, 8)), rng.standard_normal((64, 8))
    panels = {}
    E.panel_store(panels, 0, f0, f1)
    assert np.allclose(PR.from_product_form(np.stack(panels[0])), np.stack([f0, f1]), rtol=0, atol=1e-14)
    spec, lay, ref, args = _reference(small)
    blob = E.Blob(lay, args[1])
    plain, _ = E.backward_wave(spec, blob, args[2][:32], args[3][:32], args[4][:32], args[5][:32])
    tiles = np.concatenate([ref["F"][0], ref["G"][0]])
    for t in range(lay.panel["TILES"]):
        if t in (lay.panel["H0"], lay.panel["H0"] + 1, lay.panel["SDF"]):      # (the hi + lo splits are the reference's own)
            continue
        # the product form (what the weight-gradient product of the emulator contracts) is the transposed matrix in the same layout
        assert np.array_equal(PR.to_fragments(PR.to_dense(tiles[t]).T), np.stack(plain[t])), t
    # the splits sum to the emulator's value
    P = lay.panel
    d = PR.to_dense(tiles[[P["H0"], P["H0"] + 1, P["SDF"]]])
    pd = PR.to_dense(PR.from_product_form(np.stack([np.stack(plain[t]) for t in (P["H0"], P["H0"] + 1, P["SDF"])])))
    lo = [PK.frag_feature(0, 0, 5 + c) for c in range(3)]
    assert np.array_equal(d[0][:, :3] + d[1][:, lo], pd[0][:, :3]) and d[1][:, lo].any() and not pd[1][:, lo].any()
    assert np.array_equal(d[2][:, 0] + d[2][:, 1], pd[2][:, 0]) and d[2][:, 1].any()
    assert np.array_equal(PR.round16(d[2][:, 0], PR.G_REGION), d[2][:, 0]) and np.array_equal(PR.round16(d[0][:, :3], PR.F_REGION), d[0][:, :3])


@pytest.mark.parametrize("small", NETS)
def test_relu_pattern_of_its_own_changes_nothing(small):
    """backward_wave with relu_pattern = the pattern of its own r1 (/ r2) returns exactly what it returns without the argument"""
    spec, lay, ref, args = _reference(small)
    blob = E.Blob(lay, args[1])
    sl = slice(32, 64)
    plain, out = E.backward_wave(spec, blob, args[2][sl], args[3][sl], args[4][sl], args[5][sl])
    st = E.forward_wave(spec, blob, args[2][sl])[3]
    own = [[f > 0 for f in st["rs"][l]] for l in range(spec.NCMID + 1)]
    again, out2 = E.backward_wave(spec, blob, args[2][sl], args[3][sl], args[4][sl], args[5][sl], relu_pattern=own)
    assert sorted(plain, key=str) == sorted(again, key=str)
    for k in plain:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(again[k])), k
    assert all(np.array_equal(a, b) for a, b in zip(out, out2))
    # ... and the same through reference_blocks with the pattern read off the reference's own r tiles
    groups = dict((n, (t0, nt)) for n, t0, nt in PR.groups(lay, PR.F_REGION))
    pattern = np.stack([ref["F"][:, groups[n][0]:groups[n][0] + groups[n][1]] > 0 for n in ("R1", "R2") if n in groups], 1)
    imposed = PR.reference_blocks(*args, relu_pattern=pattern)
    assert all(np.array_equal(imposed[k], ref[k]) for k in ref)
    # another pattern does change the colour backward (the argument is used), and nothing of the forward
    flipped = PR.reference_blocks(*args, relu_pattern=~pattern)
    assert np.array_equal(flipped["F"], ref["F"]) and not np.array_equal(flipped["G"], ref["G"])


@pytest.mark.parametrize("small", NETS)
def test_masks_round_trip_and_one_flipped_bit_is_seen(small):
    """decode_masks / encode_masks are inverse to each other on the layout of include/avc.h, and the mask check of the GPU test -- every
    bit equals (stored r > 0) -- fails on exactly the entry whose bit was flipped"""
    spec, lay, ref, _ = _reference(small)
    groups = dict((n, (t0, nt)) for n, t0, nt in PR.groups(lay, PR.F_REGION))
    stored = PR.round16(np.stack([ref["F"][:, groups[n][0]:groups[n][0] + groups[n][1]] for n in ("R1", "R2") if n in groups], 1), PR.F_REGION)
    raw = PR.encode_masks(stored > 0, spec)
    assert raw.dtype == np.uint16 and raw.size == NBLK * 2 * spec.HT * 64
    assert np.array_equal(PR.decode_masks(raw, spec), stored > 0) and np.array_equal(PR.decode_masks(raw, spec.net_id, NBLK), stored > 0)
    # the bit of feature row r of a lane's 16 rows, stated once more from the header's words
    blk, layer, t, lane, r_ = 1, spec.NCMID, spec.HT - 1, 37, 11
    word = (blk * 2 + layer) * spec.HT * 64 + t * 64 + lane
    mut = raw.copy()
    mut[word] ^= np.uint16(1 << ((r_ >> 1) + 8 * (r_ & 1)))
    bad = np.argwhere(PR.decode_masks(mut, spec) != (stored > 0))
    assert bad.tolist() == [[blk, layer, t, r_ >> 3, lane, r_ & 7]]
    # share of reference values a 16-bit forward may round to the other side of zero: under the cap on these nets
    for layer, n in enumerate(n for n in ("R1", "R2") if n in groups):
        ref_r = ref["F"][:, groups[n][0]:groups[n][0] + groups[n][1]].reshape(-1)
        share, ndiff, _ = PR.relu_ambiguity(ref_r, ref_r > 0, gate(n))
        assert ndiff == 0 and share < RELU_AMBIGUOUS_CAP, (n, share)


def _largest_change(ref, candidates, mutate):
    """of the candidate places the one at which the mutation moves a value the furthest (a swap of two equal values is no mistake)"""
    best = None
    for c in candidates:
        m = ref.copy()
        mutate(m, c)
        d = np.abs(m - ref).max()
        if best is None or d > best[0]:
            best = (d, c)
    return best[1]


def _swap(a, i, j):
    a[i], a[j] = a[j].copy(), a[i].copy()


MUTATIONS = ("two points", "two slots", "k-steps", "half-waves", "neighbour tile")


@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("small", NETS)
def test_the_comparison_rejects_one_misplaced_value_at_the_gates_in_use(small, mutation):
    """On reference tiles with noise of 0.9 x gate x rms (which pass: the control), ONE of these mistakes in ONE tile of a group makes
    that group miss its gate -- for every group of both regions: two points of a block swapped; two feature slots of a lane swapped; the
    two k-steps swapped; the two half-waves swapped; a tile exchanged with the next tile of its region."""
    for region in (PR.F_REGION, PR.G_REGION):
        lay, ref, ntiles = _region(small, region)
        noisy = _noisy(small, region)
        assert _failing(small, region, noisy) == [], "the control must pass"
        for group, t0, nt in PR.groups(lay, region):
            tiles = [(b, t) for b in range(NBLK) for t in range(t0, t0 + nt)]
            if mutation == "two points":
                cands = [(b, t, p, q) for b, t in tiles for p, q in ((0, 1), (3, 17), (8, 31), (12, 20))]

                def mutate(a, c):
                    b, t, p, q = c
                    for h in (0, 32):
                        _swap(a[b, t, :], (slice(None), p + h), (slice(None), q + h))
            elif mutation == "two slots":
                cands = [(b, t, lane, s0, s1) for b, t in tiles for lane in (0, 5, 33, 63) for s0, s1 in (((0, 0), (0, 1)), ((0, 2), (1, 6)), ((0, 5), (0, 7)))]

                def mutate(a, c):
                    b, t, lane, (e0, j0), (e1, j1) = c
                    a[b, t, e0, lane, j0], a[b, t, e1, lane, j1] = a[b, t, e1, lane, j1], a[b, t, e0, lane, j0]
            elif mutation == "k-steps":
                cands = tiles

                def mutate(a, c):
                    a[c[0], c[1]] = a[c[0], c[1], ::-1].copy()
            elif mutation == "half-waves":
                cands = tiles

                def mutate(a, c):
                    a[c[0], c[1]] = np.concatenate([a[c[0], c[1], :, 32:], a[c[0], c[1], :, :32]], 1)
            else:
                cands = [(b, t) for b, t in tiles if t + 1 < ntiles] or [(b, t - 1) for b, t in tiles]

                def mutate(a, c):
                    _swap(a, (c[0], c[1]), (c[0], c[1] + 1))
            place = _largest_change(ref, cands, mutate)
            got = noisy.copy()
            mutate(got, place)
            failed = _failing(small, region, got)
            assert group in [g for g, _ in failed], (mutation, group, place, [(g, r.e_max) for g, r in failed])
            res = dict(failed)[group]
            assert (res.place[1], t0 + res.place[0]) in ((place[0], place[1]), (place[0], place[1] + 1)), (res.where(), place)


@pytest.mark.parametrize("small", NETS)
def test_a_dropped_column_sum_row_is_seen(small):
    """per-wavefront rows as a launch of 8 wavefronts leaves them (one block each, the others zero) with fp32 rounding: the sum passes,
    the sum without one block's row misses the gate of both parts"""
    spec, lay, ref, _ = _reference(small)
    rows = np.zeros((8, lay.cs_size), np.float32)
    rows[:NBLK] = ref["colsum"].astype(np.float32)
    total, total_abs = ref["colsum"].sum(0), ref["colsum_abs"].sum(0)
    n_hs = spec.ST * 32
    noise = np.random.default_rng(1).uniform(-1, 1, size=lay.cs_size) * (total_abs > 0)
    for part, sl in (("CS_HS", slice(0, n_hs)), ("CS_H0", slice(n_hs, None))):
        noise[sl] *= 0.9 * gate(part) * total_abs[sl][total_abs[sl] > 0].mean()
    for part in ("CS_HS", "CS_H0"):
        ok = PR.compare_colsum(rows.astype(np.float64).sum(0) + noise, total, total_abs, spec)
        assert ok[part][0] <= gate(part), (part, ok)
        for drop in range(NBLK):
            keep = np.arange(8) != drop
            res = PR.compare_colsum(rows[keep].astype(np.float64).sum(0) + noise, total, total_abs, spec)
            assert res[part][0] > gate(part), (part, drop, res)
    # a column no point contributes to must be exactly zero
    pad = np.flatnonzero(total_abs == 0)
    if len(pad):
        bad = rows.astype(np.float64).sum(0)
        bad[pad[0]] = 1e-30
        assert np.isinf(max(v[0] for v in PR.compare_colsum(bad, total, total_abs, spec).values()))
