"""What avc_render_points_fwd_train and avc_render_points_bwd STORE -- every operand tile of both panel regions, every ReLU mask bit,
every column-sum row -- against tests/wave_emulator.py (float64, block by block; tests/panel_restatement.py), point by point.

Metric per group of tiles (the names of packing.Layout.panel): e = max(0, |got - ref| - u |ref|) / rms(ref over the group), u = 2^-11
(F region, f16) resp. 2^-8 (G region, bf16) = the storage rounding, derived.  What is left is the error of the f16 forward chain and of
the bf16 backward chain in front of the store; it was measured once with the gates open (profiles/r16_panel_tests.md) and each gate is
3 x the largest e of its group over both nets' sizes below, the margin of test_render_matches_golden_on_reference_z.  No gate may exceed
GATE_CAP = 0.25: a misplaced value is wrong by about one rms (tests/test_panels_cpu.py applies the mutations at these very gates).
The backward is compared with the kernel's own ReLU pattern imposed on the reference (the pattern itself is checked against the stored
r1 / r2 and against the reference's), so a sign that f16 flips near zero does not count against every tile behind it.
Column sums: |got - ref| <= gate x sum over the points of |term|, the latter averaged over the columns of its part (gbar_hs and
gbar_h0 apart), as e of a tile is in units of its group's rms: one point's gbar_hs is a bf16 dot product of 128 or 256 terms that
cancel, its error follows the size of the terms and not of the result, and relative to its own |term| a single column came out wrong
by 1.18 (one point, a column 200 times below the part's mean, sign flipped) where the part's worst is 0.03 of the mean.
Bit-for-bit invariances (through integer views): run to run, the size of the persistent grid, a slab that starts inside the ray set,
stale buffer contents."""
import functools

import numpy as np
import pytest
import torch

from avatarclip_amd import packing as PK
from tests import panel_restatement as PR

gpu = pytest.mark.gpu
GATE_CAP = 0.25
# group: (gate, largest e measured on the small net, on the full net) -- maxima over SIZES on an MI355X, profiles/r16_panel_tests.md;
# gate = 3 x the larger of the two, with two exceptions that were measured as 0 and are derived instead:
#   SDF  the tile holds d_sdf, an input, split hi + lo exactly as the reference splits it: nothing but the storage rounding, gate 0
#   DO   delta_o = d_rgb c (1 - c) differs from the reference only through the colours c of the f16 forward, by less than the bf16
#        rounding of the value itself on every entry measured; the gate is one more rounding unit of an rms-sized value, 2^-8
GATES = {
    # F region (f16)
    "H1": (0.00444, 1.452e-03, 1.479e-03),
    "HM": (0.0115, 3.602e-03, 3.832e-03),
    "HS": (0.0153, 3.921e-03, 5.093e-03),
    "H0": (1.32e-05, 4.390e-06, 4.390e-06),
    "GA1": (0.0226, 7.511e-03, 6.967e-03),
    "GAM": (0.0435, 1.448e-02, 1.319e-02),
    "GAS": (0.0451, 1.501e-02, 1.124e-02),
    "FEAT": (0.00384, 1.280e-03, 1.052e-03),
    "XN": (0.000881, 1.600e-04, 2.934e-04),
    "R1": (0.00954, 2.511e-03, 3.177e-03),
    "R2": (0.013, None, 4.320e-03),
    # G region (bf16), against the reference with the kernel's own ReLU pattern
    "GBH1": (0.0853, 2.821e-02, 2.843e-02),
    "GBHM": (0.135, 2.861e-02, 4.493e-02),
    "GB0": (0.000956, 3.186e-04, 1.322e-04),
    "AB1": (0.155, 3.744e-02, 5.148e-02),
    "ABM": (0.138, 3.484e-02, 4.589e-02),
    "ABS": (0.0865, 2.883e-02, 1.821e-02),
    "DFEAT": (0.0711, 2.003e-02, 2.369e-02),
    "SDF": (0.0, 0.0, 0.0),
    "D1": (0.0705, 2.085e-02, 2.349e-02),
    "D2": (0.0597, None, 1.988e-02),
    "DO": (2.0 ** -8, 0.0, 0.0),
    # column sums (fp32 sums of the unrounded gbar_hs / gbar_h0), e in units of the part's mean sum over the points of |term|
    "CS_HS": (0.0975, 3.247e-02, 2.522e-02),
    "CS_H0": (0.00167, 5.565e-04, 2.739e-04),
}
assert all(0 <= g[0] <= GATE_CAP for g in GATES.values())
RELU_AMBIGUOUS_CAP = 0.02          # share of a ReLU group whose reference value lies in (0, gate x rms): a property of the reference
SAMPLE_DIST = 2 / 32
# (rays, samples): 1221 points = 39 blocks with 5 valid rows in the last; one point; exactly one block; one row into a second block
SIZES = ((37, 33), (1, 1), (1, 32), (3, 11))
NAN_BITS = 0x7FA5C3D2              # the pattern the column-sum buffer is pre-filled with


def gate(group):
    return GATES[group][0]


@functools.lru_cache(maxsize=None)
def _engine(small):
    """(renderer, engine, packed parameters, flat parameters as float64 on the host) of the seeded net"""
    from tests.engine_cases import _nets
    dev = torch.device("cuda")
    ren = _nets(small, dev)
    eng = ren.engine
    flat = ren.flat_params().detach()
    return ren, eng, eng.pack(flat), flat, flat.double().cpu().numpy()


class Run:
    pass


def _pass(small, R, S, seed=1):
    """training forward + backward of R x S points in one slab -> what the two kernels stored, on the host"""
    from tests.engine_cases import _inputs
    _, eng, pk, _, _ = _engine(small)
    dev = torch.device("cuda")
    r = Run()
    r.inputs = _inputs(R, S, dev, seed)
    ro, rd, z, dsdf, dn, drgb = r.inputs
    r.npts, r.nblk = R * S, (R * S + 31) // 32
    _, _, rgbf = eng.points_fwd_train(pk, ro, rd, z, SAMPLE_DIST)
    assert eng.plan(R, S) == (R, R)
    r.rows = int(eng.lib.avc_bwd_colsum_rows(r.npts, eng.MAX_BWD_WAVES))
    eng._colsum = torch.full((r.rows + 3, eng.dl.lay.cs_size), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    r.grad = eng.points_bwd(pk, ro, rd, z, SAMPLE_DIST, dsdf, dn, drgb, rgbf, panels_valid=True).clone()
    torch.cuda.synchronize()
    r.rgb = rgbf
    r.fp = eng._fpanels[:r.nblk * eng.fwd_tiles * 2048].cpu().numpy().view(np.uint16)
    r.gp = eng._gpanels[:r.nblk * eng.grad_tiles * 2048].cpu().numpy().view(np.uint16)
    r.masks = eng._masks[:r.nblk * eng.mask_u16].cpu().numpy().view(np.uint16)
    r.colsum = eng._colsum.cpu().numpy()
    return r


@functools.lru_cache(maxsize=None)
def _case(small, R, S):
    """one pass with the default grid, decoded, and its reference (computed once, shared by the tests, never written to)"""
    _, eng, _, _, flat = _engine(small)
    spec = eng.spec
    r = _pass(small, R, S)
    r.F = PR.decode(r.fp, PR.F_REGION, eng.fwd_tiles, r.nblk)
    r.G = PR.decode(r.gp, PR.G_REGION, eng.grad_tiles, r.nblk)
    r.pattern = PR.decode_masks(r.masks, spec, r.nblk)
    ro, rd, z, dsdf, dn, drgb = (a.cpu().numpy() for a in r.inputs)
    x = PR.midpoints(ro, rd, z, SAMPLE_DIST)
    r.ref = PR.reference_blocks(spec, flat, x, dsdf.reshape(-1), dn.reshape(-1, 3), drgb.reshape(-1, 6), relu_pattern=r.pattern)
    r.valid = PR.valid_lanes(r.nblk, r.npts)
    for a in (r.F, r.G, r.pattern, r.valid, r.fp, r.gp, r.masks, r.colsum, *r.ref.values()):
        a.setflags(write=False)
    return r


def _valid_entries(r, tiles):
    """[nblk][nt][2][64][8] -> the entries of valid points, 1-D"""
    return tiles[np.broadcast_to(r.valid[:, None, None, :, None], tiles.shape)]


def _compare_region(r, lay, region, name):
    """every group of a region against the reference; -> the largest e.  Prints each figure before it asserts."""
    got, ref = (r.F, r.ref["F"]) if region == PR.F_REGION else (r.G, r.ref["G"])
    worst, failures = 0.0, []
    for group, t0, nt in PR.groups(lay, region):
        res = PR.compare(got[:, t0:t0 + nt], ref[:, t0:t0 + nt], group, PR.UNIT_ROUNDOFF[region], r.valid)
        print("panels %s %-5s e max %.3e mean %.3e (gate %.3e) rms %.3e" % (name, group, res.e_max, res.e_mean, gate(group), res.rms))
        assert res.rms > 0, group
        worst = max(worst, res.e_max)
        if not res.e_max <= gate(group):
            failures.append(res.where())
    assert not failures, "\n".join(failures)
    return worst


def _name(small, R, S):
    return "%s %dx%d" % ("small" if small else "full", R, S)


@gpu
@pytest.mark.parametrize("R,S", SIZES)
@pytest.mark.parametrize("small", [True, False])
def test_forward_panels_match_the_emulator_point_by_point(small, R, S):
    """F region: h_l, the PE values (x split hi + lo), g_a,l, the feature vector, [x, n], r1 (, r2) of every valid point, group by group.
    r1 / r2 are compared as values, relu(r): a sign flipped near zero is an error of the value's own size."""
    r = _case(small, R, S)
    lay = _engine(small)[1].dl.lay
    worst = _compare_region(r, lay, PR.F_REGION, _name(small, R, S))
    assert worst > 0, "f16 tiles of an f16 chain cannot equal float64 to the rounding: is the comparison looking at the kernel's output?"


@gpu
@pytest.mark.parametrize("R,S", SIZES)
@pytest.mark.parametrize("small", [True, False])
def test_relu_masks_are_the_sign_of_the_stored_activations(small, R, S):
    """Every mask bit of a valid point equals (stored r > 0), exactly.  The kernel's pattern differs from the reference's only where the
    reference's relu(r) is below the group's gate, and such values are under 2 % of the group (measured: 0.6 % at most on 39 blocks).
    Stored zeros whose reference is positive and above the smallest f16 subnormal are counted and printed; none may lie above the gate.
    They do occur below it, and as often as the opposite flip -- the f16 chain's error of about 1e-3 rms around a reference next to zero:
    on 39 blocks 9 lost / 10 gained of 156288 (small net, r1), 18 / 18 (full, r1), 18 / 19 (full, r2), the largest reference among them
    7.2e-4, 6.0e-4, 1.8e-3 of the group's rms; at most 1 in the one-block cases."""
    r = _case(small, R, S)
    _, eng, _, _, _ = _engine(small)
    lay = eng.dl.lay
    layers = [g for g in PR.groups(lay, PR.F_REGION) if g[0] in ("R1", "R2")]
    assert len(layers) == r.pattern.shape[1] == eng.spec.NCMID + 1
    for layer, (group, t0, nt) in enumerate(layers):
        stored, on = r.F[:, t0:t0 + nt], r.pattern[:, layer]
        bad = np.argwhere((on != (stored > 0)) & r.valid[:, None, None, :, None])
        assert not len(bad), "%s: %d mask bits differ from (stored value > 0), first at block %d, tile %d, k-step %d, lane %d, slot %d" % (
            (group, len(bad)) + tuple(int(v) for v in bad[0]))
        assert not (_valid_entries(r, stored) < 0).any(), group
        ref_r, stored_v, on_v = (_valid_entries(r, a) for a in (r.ref["F"][:, t0:t0 + nt], stored, on))
        rms = float(np.sqrt(np.mean(ref_r ** 2)))
        lost = int(((stored_v == 0) & (ref_r > PR.SMALLEST_F16)).sum())
        lost_above = int(((stored_v == 0) & (ref_r > max(PR.SMALLEST_F16, gate(group) * rms))).sum())
        share, ndiff, worst = PR.relu_ambiguity(ref_r, on_v, gate(group))
        print("masks %s %s: %d of %d patterns differ from the reference's (largest relu(r_ref) / rms among them %.3e, gate %.3e); stored zeros "
              "with a positive reference %d, above the gate %d; share of the group in (0, gate x rms) %.4f"
              % (_name(small, R, S), group, ndiff, ref_r.size, worst, gate(group), lost, lost_above, share))
        assert lost_above == 0, (group, lost_above)
        assert worst < gate(group), (group, worst)
        assert share < RELU_AMBIGUOUS_CAP, (group, share)


@gpu
@pytest.mark.parametrize("R,S", SIZES)
@pytest.mark.parametrize("small", [True, False])
def test_backward_panels_and_column_sums_match_the_emulator(small, R, S):
    """G region: gbar_h, abar, ybar[1:], d_sdf (hi + lo), delta of every valid point, group by group, against the emulator run with the
    kernel's own ReLU pattern; the column sums of gbar_hs / gbar_h0 summed over the rows of the launch; every row of the launch written,
    none behind them."""
    r = _case(small, R, S)
    _, eng, _, _, _ = _engine(small)
    worst = _compare_region(r, eng.dl.lay, PR.G_REGION, _name(small, R, S))
    assert worst > 0, "bf16 tiles of a bf16 chain cannot equal float64 to the rounding: is the comparison looking at the kernel's output?"
    assert r.rows == 8 * min((r.nblk + 7) // 8, eng.MAX_BWD_WAVES // 8)
    bits = r.colsum.view(np.int32)
    assert not (bits[:r.rows] == NAN_BITS).any(), "a column-sum row of the launch was not written"
    assert (bits[r.rows:] == NAN_BITS).all(), "a row behind the launch's was written"
    _check_colsum(r, eng.spec, _name(small, R, S))


def _check_colsum(r, spec, name, rows=None):
    rows = r.colsum[:r.rows] if rows is None else rows
    assert np.isfinite(rows).all()
    res = PR.compare_colsum(rows.astype(np.float64).sum(0), r.ref["colsum"].sum(0), r.ref["colsum_abs"].sum(0), spec)
    for part, (e, col, got, ref) in res.items():
        print("panels %s %-5s e max %.3e (gate %.3e) at column %d: got %.6g, reference %.6g" % (name, part, e, gate(part), col, got, ref))
        assert e <= gate(part), (part, e, col, got, ref)


def _same_bits(a, b, what):
    a, b = np.asarray(a).view(np.uint16), np.asarray(b).view(np.uint16)
    assert a.shape == b.shape, what
    bad = np.flatnonzero(a != b)
    assert not len(bad), "%s: %d 16-bit words differ, first at %d (tile %d, element %d): 0x%04x != 0x%04x" % (
        what, len(bad), bad[0], bad[0] // 1024, bad[0] % 1024, a[bad[0]], b[bad[0]])


def _same_valid_bits(r, other, eng, what):
    """F, G and masks of the valid points of two passes over the same ray set"""
    v = np.broadcast_to(r.valid[:, None, None, :, None], (r.nblk, 1, 2, 64, 8))
    for name, a, b, tiles in (("F", r.fp, other.fp, eng.fwd_tiles), ("G", r.gp, other.gp, eng.grad_tiles)):
        a, b = (np.asarray(x).reshape(r.nblk, tiles, 2, 64, 8) for x in (a, b))
        m = np.broadcast_to(v, a.shape)
        _same_bits(a * m, b * m, "%s, %s region" % (what, name))
    a, b = (np.asarray(x).reshape(r.nblk, -1, 64) for x in (r.masks, other.masks))
    _same_bits(a * r.valid[:, None, :], b * r.valid[:, None, :], "%s, masks" % what)


@gpu
@pytest.mark.parametrize("small", [True, False])
def test_stored_bits_do_not_depend_on_the_run_the_grid_or_stale_buffers(small, monkeypatch):
    """39 blocks: a second run; MAX_BWD_WAVES = 8 (one workgroup that loops over all blocks), 16 and the default; the same rays after a
    larger ray set has filled the buffers.  No bit of F, G or the masks of a valid point changes; the column sums, whose fp32 summation
    order follows the grid, stay within their bound; the rows of every launch are all written."""
    from avatarclip_amd.engine import Engine
    R, S = SIZES[0]
    r = _case(small, R, S)
    _, eng, _, _, _ = _engine(small)
    name = _name(small, R, S)
    again = _pass(small, R, S)
    _same_bits(again.fp, r.fp, "second run, F region")
    _same_bits(again.gp, r.gp, "second run, G region")
    _same_bits(again.masks, r.masks, "second run, masks")
    assert np.array_equal(again.colsum.view(np.int32), r.colsum.view(np.int32)), "second run, column sums"
    assert torch.equal(again.grad.view(torch.int32), r.grad.view(torch.int32))
    default = Engine.MAX_BWD_WAVES
    for waves in (8, 16):
        monkeypatch.setattr(Engine, "MAX_BWD_WAVES", waves)
        o = _pass(small, R, S)
        monkeypatch.setattr(Engine, "MAX_BWD_WAVES", default)
        assert o.rows == waves < r.rows == 40
        _same_bits(o.fp, r.fp, "MAX_BWD_WAVES = %d, F region" % waves)
        _same_bits(o.gp, r.gp, "MAX_BWD_WAVES = %d, G region" % waves)
        _same_bits(o.masks, r.masks, "MAX_BWD_WAVES = %d, masks" % waves)
        bits = o.colsum.view(np.int32)
        assert not (bits[:o.rows] == NAN_BITS).any() and (bits[o.rows:] == NAN_BITS).all(), waves
        _check_colsum(r, eng.spec, "%s, %d waves" % (name, waves), rows=o.colsum[:o.rows])
    # stale data: 64 rays fill the buffers with other values (and the last block's unused rows with them), then the same 37 again
    _pass(small, 64, S, seed=2)
    o = _pass(small, R, S)
    _same_valid_bits(r, o, eng, "after a larger ray set")
    assert np.array_equal(o.colsum.view(np.int32), r.colsum.view(np.int32)), "after a larger ray set, column sums"


@gpu
@pytest.mark.parametrize("small", [True, False])
def test_a_slab_that_starts_inside_the_ray_set_writes_the_same_blocks(small):
    """avc_render_points_bwd on rays 3..7 of 8 rays x 32 samples (every ray is a block), all pointers advanced as include/avc.h
    describes, into a G region of its own: its blocks 0..4 are blocks 3..7 of the one-slab run, bit for bit, and its column sums are those
    blocks' share."""
    from avatarclip_amd import lib as L
    _, eng, pk, _, _ = _engine(small)
    dev = torch.device("cuda")
    R, S, s0 = 8, 32, 3
    r = _pass(small, R, S)
    ro, rd, z, dsdf, dn, drgb = r.inputs
    npts = (R - s0) * S
    nblk = npts // 32
    rows = int(eng.lib.avc_bwd_colsum_rows(npts, eng.MAX_BWD_WAVES))
    assert (nblk, rows) == (5, 8)
    gpanels = torch.zeros((nblk + 1) * eng.grad_tiles * 2048, dtype=torch.uint8, device=dev)      # + the sink block of the wavefronts past the end
    colsum = torch.full((rows, eng.dl.lay.cs_size), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    # (the F region and the masks of the one-slab run are still in the engine's buffers: 8 blocks and the forward's sink block)
    assert eng._fpanels.numel() >= (R + 1) * eng.fwd_tiles * 2048 and eng._masks.numel() >= (R + 1) * eng.mask_u16
    L.call("avc_render_points_bwd", eng.net, None, ro.data_ptr() + s0 * 3 * 4, rd.data_ptr() + s0 * 3 * 4, z.data_ptr() + s0 * z.stride(0) * 4,
           S, z.stride(0), SAMPLE_DIST, npts, pk.w_bf16, pk.tab, eng.dl.offsets, dsdf.data_ptr() + s0 * S * 4, dn.data_ptr() + s0 * S * 3 * 4,
           drgb.data_ptr() + s0 * S * 6 * 4, r.rgb.data_ptr() + s0 * S * 6 * 4, eng._fpanels.data_ptr() + s0 * eng.fwd_tiles * 2048, gpanels,
           eng._masks.data_ptr() + s0 * eng.mask_u16 * 2, colsum, eng.MAX_BWD_WAVES)
    torch.cuda.synchronize()
    got = gpanels[:nblk * eng.grad_tiles * 2048].cpu().numpy().view(np.uint16)
    _same_bits(got, r.gp.reshape(R, -1)[s0:].reshape(-1), "slab of rays %d..%d, G region" % (s0, R - 1))
    # one wavefront per block, one row per wavefront, in both launches: the rows are the blocks'
    cs = colsum.cpu().numpy().view(np.int32)
    assert not (cs == NAN_BITS).any()
    assert np.array_equal(cs[:nblk], r.colsum.view(np.int32)[s0:R]) and not cs[nblk:].any()
