"""What avc_render_points_fwd_train and avc_render_points_bwd store, point by point (TEST INFRASTRUCTURE ONLY): decoders of the two
operand-panel regions and of the ReLU masks as include/avc.h states them, the float64 reference of every tile and column sum
(tests/wave_emulator.py, block by block) and the comparison that names the first wrong value.

Everything is compared in FRAGMENT SPACE, the layout of a tile in memory: [k-step e][lane = point + 32 half][8 slots], slot (e, h, j)
= feature packing.frag_feature(e, h, j) of the tile's 32.  These are the fragment pairs the emulator hands to its panel_store; what
panel_store RETURNS is the same tile seen by the weight-gradient product (lane = feature + 32 half, slots = points, the transpose),
and the emulator builds its SDF tile directly in that form, so the reference tiles are brought back with from_product_form."""
import numpy as np

from avatarclip_amd import packing as PK
from tests import wave_emulator as E
from tests import wgrad_restatement as W

F_REGION, G_REGION = W.F16, W.BF16                 # region = element type of the ABI: 0 = F (f16 tiles), 1 = G (bf16 tiles)
UNIT_ROUNDOFF = {F_REGION: 2.0 ** -11, G_REGION: 2.0 ** -8}      # round to nearest of an 11- resp. 8-bit significand
F_GROUPS = ("H1", "HM", "HS", "H0", "GA1", "GAM", "GAS", "FEAT", "XN", "R1", "R2")
G_GROUPS = ("GBH1", "GBHM", "GB0", "AB1", "ABM", "ABS", "DFEAT", "SDF", "D1", "D2", "DO")
SMALLEST_F16 = 2.0 ** -24                          # the smallest f16 subnormal

# slot (e, h, j) of a tile <-> feature of the tile (fragment space) = point of the block (product form)
_SLOT = np.array([[[PK.frag_feature(e, h, j) for j in range(8)] for h in range(2)] for e in range(2)])      # [e][h][j]
assert sorted(_SLOT.reshape(-1)) == list(range(32))
assert all(PK.acc_row(8 * e + j, h) == _SLOT[e, h, j] for e in range(2) for h in range(2) for j in range(8))


def groups(lay, region):
    """[(name, first tile local to its region, tiles)] of a region, in region order; a group's size is where the next one starts
    (the small net has no R2 / D2 tiles: those are left out)"""
    P = lay.panel
    names = F_GROUPS if region == F_REGION else G_GROUPS
    base, end = (0, P["FTILES"]) if region == F_REGION else (P["FTILES"], P["TILES"])
    starts = [P[n] for n in names] + [end]
    assert starts[0] == base and starts == sorted(starts), "packing.Layout.panel: the groups of a region follow each other"
    return [(n, starts[i] - base, starts[i + 1] - starts[i]) for i, n in enumerate(names) if starts[i + 1] > starts[i]]


def decode(raw_u16, region, tiles_per_block, nblk):
    """the raw bytes of a region, viewed as uint16 -> float64 [nblk][tile][2 k-steps][64 lanes][8] (F region: f16, G region: bf16)"""
    raw = np.asarray(raw_u16).reshape(-1).view(np.uint16)
    n = nblk * tiles_per_block * W.TILE_U16
    assert raw.size >= n
    return W.from_bits(raw[:n], region).reshape(nblk, tiles_per_block, 2, 64, 8)


def round16(v, region):
    """float64 values rounded to the region's 16-bit type (nearest, ties to even), as float64"""
    v = np.asarray(v, np.float64)
    if region == F_REGION:
        return v.astype(np.float16).astype(np.float64)
    return W.round_to_bf16(v.astype(np.float32)).astype(np.float64)


def encode(tiles, region):
    """[nblk][tile][2][64][8] -> the raw region (uint16), every value rounded to the region's 16-bit type"""
    return W.to_bits(round16(tiles, region), region).reshape(-1)


def decode_masks(raw_u16, net, nblk=None):
    """the ReLU masks (include/avc.h: [layer][tile][lane] x 16 bits per block, bit (r >> 1) + 8 (r & 1) = feature row r of the lane's
    16 rows; rows 0..7 are the slots of the tile's first fragment, 8..15 of its second) -> bool [nblk][layer][tile][2][64][8], the
    > 0 pattern in the shape of the R1 (/ R2) fragments.  Layers the net does not have (the small net's second) are left out."""
    spec = PK.SMALL if net in (1, PK.SMALL) else PK.FULL
    per_block = 2 * spec.HT * 64
    raw = np.asarray(raw_u16).reshape(-1).view(np.uint16)
    nblk = raw.size // per_block if nblk is None else nblk
    m = raw[:nblk * per_block].reshape(nblk, 2, spec.HT, 64).astype(np.uint32)
    bit = np.array([[(r >> 1) + 8 * (r & 1) for r in range(8 * e, 8 * e + 8)] for e in range(2)])            # [e][j]
    out = (m[:, :, :, None, :, None] >> bit[None, None, None, :, None, :]) & 1                                  # [b][layer][t][e][lane][j]
    return out[:, :spec.NCMID + 1].astype(bool)


def encode_masks(pattern, net):
    """the inverse of decode_masks: bool [nblk][layer][tile][2][64][8] -> uint16 [nblk * 2 * HT * 64] (a missing layer: zeros)"""
    spec = PK.SMALL if net in (1, PK.SMALL) else PK.FULL
    pattern = np.asarray(pattern, bool)
    nblk = pattern.shape[0]
    bit = np.array([[(r >> 1) + 8 * (r & 1) for r in range(8 * e, 8 * e + 8)] for e in range(2)])
    m = np.zeros((nblk, 2, spec.HT, 64), np.uint32)
    m[:, :pattern.shape[1]] = (pattern.astype(np.uint32) << bit[None, None, None, :, None, :]).sum(axis=(3, 5))
    return m.astype(np.uint16).reshape(-1)


def from_product_form(k):
    """[..., 2, 64, 8] tiles as wave_emulator.panel_store returns them ((k0, k1): lane = feature + 32 half, slot (e, h, j) = point
    frag_feature(e, h, j)) -> the same tiles in fragment space (lane = point + 32 half, slot (e, h, j) = feature frag_feature(e, h, j))"""
    k = np.asarray(k)
    lead = k.shape[:-3]
    m = np.empty(lead + (32, 32))                                                     # [point][feature]
    m[..., _SLOT.reshape(-1), :] = k.reshape(lead + (2, 2, 32, 8)).swapaxes(-1, -2).reshape(lead + (32, 32))
    return to_fragments(m)


def to_fragments(m):
    """[..., 32 points, 32 features] -> [..., 2, 64, 8]"""
    m = np.asarray(m)
    f = m[..., _SLOT]                                                                 # [.., p, e, h, j]
    return np.ascontiguousarray(np.moveaxis(f, -4, -2)).reshape(m.shape[:-2] + (2, 64, 8))


def to_dense(frags):
    """[..., 2, 64, 8] -> [..., 32 points, 32 features]"""
    frags = np.asarray(frags)
    lead = frags.shape[:-3]
    m = np.empty(lead + (32, 32))
    m[..., _SLOT] = np.moveaxis(frags.reshape(lead + (2, 2, 32, 8)), -2, -4)
    return m


def midpoints(ro, rd, z, sample_dist):
    """the points the kernels evaluate (csrc/avc_mlp.h: fetch_point): ro + rd (z + dist / 2), dist = the next sample's distance, the
    last section's = sample_dist; float64 from the fp32 inputs -> [R * S, 3]"""
    ro, rd, z = (np.asarray(a, np.float32).astype(np.float64) for a in (ro, rd, z))
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((z.shape[0], 1), float(np.float32(sample_dist)))], 1)
    t = z + 0.5 * dist
    return (ro[:, None, :] + rd[:, None, :] * t[:, :, None]).reshape(-1, 3)


def reference_blocks(spec, flat_params, x, d_sdf, d_n, d_rgb, relu_pattern=None):
    """wave_emulator.backward_wave block by block over the points x [N, 3] with cotangents d_sdf [N], d_n [N, 3], d_rgb [N, 6] ->
    {"F": [nblk][FTILES][2][64][8], "G": [nblk][GTILES][2][64][8], "colsum" / "colsum_abs": [nblk][cs_size]} in float64.
    relu_pattern: bool [nblk][layer][tile][2][64][8] (decode_masks) imposed on the colour backward.
    The rows of the last block past N repeat the last point with zero cotangents, as the kernels do (their entries are not compared).
    Two operands are stored SPLIT in two 16-bit slots, which the emulator -- unrounded -- has no reason to do; the reference states
    the split the kernels document, hi = the value rounded to the tile's type, lo = value - hi:
      x (packing.kmap_pe(lo_as_x): PE slots 0..2 = hi, 21..23 = lo of half 0; csrc/avc_common.h pe_to_frags_f16), f16;
      d_sdf (features 0, 1 of the SDF tile, both row 0 of the last layer; csrc/avc_bwd_body.h), bf16."""
    lay = PK.layout_for(spec)
    P = lay.panel
    blob = E.Blob(lay, np.asarray(flat_params, np.float64))
    x, d_sdf, d_n, d_rgb = (np.asarray(a, np.float64) for a in (x, d_sdf, d_n, d_rgb))
    N = x.shape[0]
    nblk = (N + 31) // 32
    pad = 32 * nblk - N
    x = np.concatenate([x, np.repeat(x[-1:], pad, 0)])
    d_sdf, d_n, d_rgb = (np.concatenate([a, np.zeros((pad,) + a.shape[1:])]) for a in (d_sdf.reshape(N), d_n.reshape(N, 3), d_rgb.reshape(N, 6)))
    tiles = np.zeros((nblk, P["TILES"], 2, 64, 8))
    colsum, colsum_abs = np.zeros((nblk, lay.cs_size)), np.zeros((nblk, lay.cs_size))
    for b in range(nblk):
        sl = slice(32 * b, 32 * b + 32)
        pat = None
        if relu_pattern is not None:
            pat = [[relu_pattern[b][l][t][e] for t in range(spec.HT) for e in range(2)] for l in range(spec.NCMID + 1)]
        panels, _ = E.backward_wave(spec, blob, x[sl], d_sdf[sl], d_n[sl], d_rgb[sl], relu_pattern=pat)
        colsum[b], colsum_abs[b] = panels.pop("colsum"), panels.pop("colsum_abs")
        assert sorted(panels) == list(range(P["TILES"])), "every tile of both regions, nothing else"
        for t, (k0, k1) in panels.items():
            tiles[b, t] = from_product_form(np.stack([k0, k1]))
    # the two split operands (half 0 = lanes 0..31)
    h0 = tiles[:, P["H0"]:P["H0"] + 2]
    assert not h0[:, 1, 0, :32, 5:8].any()
    hi = round16(h0[:, 0, 0, :32, 0:3], F_REGION)
    h0[:, 1, 0, :32, 5:8] = h0[:, 0, 0, :32, 0:3] - hi
    h0[:, 0, 0, :32, 0:3] = hi
    sd = tiles[:, P["SDF"]]
    assert not sd[:, 0, :32, 1].any()
    hi = round16(sd[:, 0, :32, 0], G_REGION)
    sd[:, 0, :32, 1] = sd[:, 0, :32, 0] - hi
    sd[:, 0, :32, 0] = hi
    return {"F": tiles[:, :P["FTILES"]], "G": tiles[:, P["FTILES"]:], "colsum": colsum, "colsum_abs": colsum_abs}


def valid_lanes(nblk, npts):
    """bool [nblk][64]: the lanes (point + 32 half) of every block that belong to one of the npts points"""
    pt = 32 * np.arange(nblk)[:, None] + (np.arange(64)[None, :] & 31)
    return pt < npts


class Result:
    """outcome of compare(): e_max / e_mean over the group's valid entries, the reference's rms, the place of the maximum"""
    def __init__(self, group, e_max, e_mean, rms, place, got, ref):
        self.group, self.e_max, self.e_mean, self.rms, self.place, self.got, self.ref = group, e_max, e_mean, rms, place, got, ref

    def where(self):
        t, b, e, lane, j = self.place
        return ("%s: worst e = %.3e (mean %.3e, reference rms %.3e) at tile %d of the group, block %d, k-step %d, lane %d (point %d of the "
                "block, half %d), slot %d = feature %d of the tile: got %.6g, reference %.6g"
                % (self.group, self.e_max, self.e_mean, self.rms, t, b, e, lane, lane & 31, lane >> 5, j, _SLOT[e, lane >> 5, j],
                   self.got, self.ref))


def compare(got, ref, group, unit_roundoff, valid=None):
    """got, ref [nblk][tiles of the group][2][64][8] -> Result with e = max(0, |got - ref| - u |ref|) / rms(ref over the whole group): the
    excess over the storage rounding of the reference value, in units of the group's root mean square; valid: bool [nblk][64], the
    lanes that count (default: all)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and got.shape[2:] == (2, 64, 8), (got.shape, ref.shape)
    nblk, nt = got.shape[:2]
    v = np.ones((nblk, 64), bool) if valid is None else np.asarray(valid, bool)
    v = np.broadcast_to(v[:, None, None, :, None], got.shape)
    assert v.any()
    rms = float(np.sqrt(np.mean(ref[v] ** 2)))
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.maximum(0.0, np.abs(got - ref) - unit_roundoff * np.abs(ref)) / rms
    e = np.where(np.isfinite(e), e, np.inf)            # a NaN / Inf in the kernel's output, or a zero rms, is the worst error there is
    e = np.where(v, e, 0.0)
    k = int(np.argmax(e))
    b, t, ks, lane, j = (int(i) for i in np.unravel_index(k, e.shape))
    return Result(group, float(e.reshape(-1)[k]), float(e[v].mean()), rms, (t, b, ks, lane, j), float(got[b, t, ks, lane, j]),
                  float(ref[b, t, ks, lane, j]))


def compare_colsum(got, ref, ref_abs, spec):
    """the column sums of a launch, got [cs_size] = the sum of the kernel's rows, against the reference's sum over the blocks, for the
    gbar_hs and the gbar_h0 part apart: e = |got - ref| / (sum over the points of |term|, averaged over the part's columns) -> {"CS_HS":
    (e_max, column, got, ref), "CS_H0": ..}.  A column no point contributes to (padding of the layout) must be exactly zero: it counts
    as e = inf if not."""
    got, ref, ref_abs = (np.asarray(a, np.float64).reshape(-1) for a in (got, ref, ref_abs))
    n_hs = spec.ST * 32
    assert got.shape == ref.shape == ref_abs.shape == (n_hs + 48,)
    err = np.abs(got - ref)
    out = {}
    for name, sl in (("CS_HS", slice(0, n_hs)), ("CS_H0", slice(n_hs, n_hs + 48))):
        live = ref_abs[sl] > 0
        assert live.any(), name
        e = np.where(live, err[sl] / ref_abs[sl][live].mean(), np.where(err[sl] > 0, np.inf, 0.0))
        e = np.where(np.isfinite(got[sl]), e, np.inf)
        k = int(np.argmax(e))
        out[name] = (float(e[k]), k, float(got[sl][k]), float(ref[sl][k]))
    return out


def relu_ambiguity(ref_r, kernel_on, gate):
    """ref_r: the reference's R1 or R2 tiles (relu(r) >= 0), kernel_on: the kernel's pattern of the same shape, both restricted to the valid
    entries (1-D) -> (share of entries with 0 < relu(r_ref) below gate x rms -- a property of the reference alone --, number of entries whose
    pattern differs from the reference's, the largest |relu(r_ref)| / rms among those)"""
    ref_r, kernel_on = np.asarray(ref_r, np.float64), np.asarray(kernel_on, bool)
    rms = float(np.sqrt(np.mean(ref_r ** 2)))
    differ = kernel_on != (ref_r > 0)
    share = float(np.mean((ref_r > 0) & (ref_r < gate * rms)))
    return share, int(differ.sum()), float((ref_r[differ] / rms).max()) if differ.any() else 0.0
