"""The fused NeuS kernels at the four scaled-down network shapes (packing.SUPPORTED beyond the two the reference ships: 128-wide with
4 + 2 layers, 256-wide with 3 + 1, 64-wide with either depth), on an MI355X.  Every statement and gate is one the suite already makes
about the two shipped shapes, applied at the new ones:

  rendered values / parameter gradients   tests/test_gpu_kernels.py: test_render_matches_golden_on_reference_z and
                                          test_parameter_gradients_match_golden (SURVEY 8d's gates), against the reference's own render
                                          and autograd (tests/golden/neus_shape_*.npz, scripts/gen_golden_shapes.py)
  SDF kernel at ragged sizes              a point's value does not depend on what shares its launch, bit for bit
  stored panels, masks, column sums       tests/test_gpu_panels.py's metric against tests/wave_emulator.py, point by point
  weight-gradient products                tests/test_gpu_wgrad.py: the production pair table on integer panels, bit for bit
  one whole iteration                     tests/test_gpu_iteration.py's parity statement against oracle/iteration_oracle.py, then a
                                          checkpoint round trip

Panel gates: e per group was measured once with the gates open at (5, 13) and (33, 64) on the four shapes (profiles/net_shapes.md);
each gate is 3 x the largest of those eight figures, the project's margin, and none exceeds GATE_CAP.  SDF = 0 and DO = 2^-8 are
derived (tests/test_gpu_panels.py) and carry over unmeasured."""
import functools

import numpy as np
import pytest
import torch

from avatarclip_amd import packing as PK
from tests import panel_restatement as PR
from tests import wgrad_restatement as W
from tests.helpers import relerr
from tests.net_shapes_common import NEW_SHAPES, SHAPE_IDS, confs, decode_masks, load_shape_case, seeded_renderer

gpu = pytest.mark.gpu
shapes = pytest.mark.parametrize("shape", NEW_SHAPES, ids=SHAPE_IDS)
GATE_CAP = 0.25
# group: (gate, largest e measured over the four shapes and the two sizes); gate = 3 x measured, SDF and DO derived
GATES = {
    # F region (f16)
    "H1": (0.00622, 2.070e-03),
    "HM": (0.0136, 4.515e-03),
    "HS": (0.0164, 5.465e-03),
    "H0": (1.42e-05, 4.724e-06),
    "GA1": (0.0437, 1.454e-02),
    "GAM": (0.0941, 3.137e-02),
    "GAS": (0.0698, 2.326e-02),
    "FEAT": (0.00301, 1.003e-03),
    "XN": (0.00157, 5.201e-04),
    "R1": (0.0084, 2.798e-03),
    "R2": (0.0108, 3.578e-03),
    # G region (bf16), against the reference with the kernel's own ReLU pattern
    "GBH1": (0.0939, 3.127e-02),
    "GBHM": (0.144, 4.786e-02),
    "GB0": (0.00192, 6.373e-04),
    "AB1": (0.184, 6.117e-02),
    "ABM": (0.216, 7.196e-02),
    "ABS": (0.205, 6.833e-02),
    "DFEAT": (0.0927, 3.089e-02),
    "SDF": (0.0, 0.0),
    "D1": (0.0809, 2.695e-02),
    "D2": (0.0612, 2.038e-02),
    "DO": (2.0 ** -8, 0.0),
    # column sums, e in units of the part's mean sum over the points of |term|
    "CS_HS": (0.011, 3.643e-03),
    "CS_H0": (0.000145, 4.822e-05),
}
RELU_AMBIGUOUS_CAP = 0.02          # tests/test_gpu_panels.py
SAMPLE_DIST = 2 / 32
# (rays, samples): 65 points = one full block, one ragged block (1 valid row in the third) and ray boundaries inside the blocks;
# 2112 points = 66 blocks, more than one 8-wave workgroup iteration
PANEL_SIZES = ((5, 13), (33, 64))
NAN_BITS = 0x7FA5C3D2


def gate(group):
    g = GATES[group][0]
    assert g is not None and 0 <= g <= GATE_CAP, group
    return g


# --------------------------------------------------------------------------------------------- rendered values, parameter gradients
def _setup(shape):
    from avatarclip_amd import fields, renderer
    spec = PK.NetSpec(*shape)
    rec, sd_sdf, sd_col, variance = load_shape_case(shape)
    dev = torch.device("cuda")
    sdf_conf, col_conf = confs(spec)
    sdf = fields.SDFNetwork(**sdf_conf)
    col = fields.RenderingNetwork(**col_conf)
    var = fields.SingleVarianceNetwork(0.3)
    sdf.load_state_dict(sd_sdf)
    col.load_state_dict(sd_col)
    var.load_state_dict({"variance": variance})
    sdf, col, var = sdf.to(dev), col.to(dev), var.to(dev)
    ren = renderer.NeuSRenderer(None, sdf, var, col, n_samples=32, n_importance=32, n_outside=0, up_sample_steps=4, perturb=1.0,
                                extra_color=True)
    assert ren.engine.spec == spec and ren.engine.net == spec.net_id == 2 + NEW_SHAPES.index(shape)
    return rec, sdf, col, var, ren, dev


def _render(rec, ren, dev):
    bg = rec["bg"].to(dev) if rec["bg"].numel() else None
    return ren.render(rec["rays_o"].to(dev), rec["rays_d"].to(dev), rec["near"].to(dev), rec["far"].to(dev), background_rgb=bg,
                      cos_anneal_ratio=float(rec["cos_anneal"]), z_vals=rec["z_final"].to(dev))


@gpu
@shapes
def test_render_matches_the_reference_on_its_z(shape):
    """the training forward (grad mode is on) against the reference's own render on identical rays, weights and z: SURVEY 8d's gates"""
    rec, sdf, col, var, ren, dev = _setup(shape)
    out = _render(rec, ren, dev)
    torch.cuda.synchronize()
    for k, tol_max, tol_mean in (("color_fine", 5e-3, 2e-4), ("extra_color_fine", 5e-3, 2e-4), ("weight_sum", 5e-3, 2e-4), ("weights", 1e-2, 1e-4)):
        e = (out[k].detach().cpu() - rec["out_" + k]).abs()
        print(shape, k, "max", e.max().item(), "mean", e.mean().item())
        assert e.max() < tol_max and e.mean() < tol_mean, k
    assert torch.allclose(out["mid_z_vals"].cpu(), rec["out_mid_z_vals"], atol=1e-5)
    assert torch.equal(out["inside_sphere"].cpu(), rec["out_inside_sphere"])
    assert abs(out["gradient_error"].item() - rec["out_gradient_error"].item()) < 5e-3


@gpu
@shapes
def test_parameter_gradients_match_the_reference(shape):
    """loss.backward() through the HIP path against the reference's autograd gradients (double backward of SDFNetwork.gradient included),
    the scalar loss of oracle/gen_golden.py: 1e-2 per tensor with cosine above 0.9995; 2e-2 for tensors below 1e-4 of the whole gradient's
    norm, which may be colour-branch tensors only"""
    from oracle.gen_golden import scalar_loss
    rec, sdf, col, var, ren, dev = _setup(shape)
    out = _render(rec, ren, dev)
    coef = {k[5:]: v.to(dev) for k, v in rec.items() if k.startswith("coef_")}
    loss = scalar_loss(out, coef)
    loss.backward()
    torch.cuda.synchronize()
    print(shape, "loss", loss.item(), "ref", rec["loss"].item())
    assert abs(loss.item() - rec["loss"].item()) < 2e-3 * max(1.0, abs(rec["loss"].item()))
    worst, bad = 0.0, []
    gnorm = float(np.sqrt(sum(float(rec[k].double().pow(2).sum()) for k in rec if k.startswith("grad_"))))
    for pfx, net in (("sdf.", sdf), ("var.", var), ("col.", col)):
        for n_, p in net.named_parameters():
            ref = rec["grad_" + pfx + n_]
            g = p.grad.detach().cpu() if p.grad is not None else torch.zeros_like(ref)
            if ref.abs().max() < 1e-7:
                continue
            re = relerr(g, ref)
            cos = torch.nn.functional.cosine_similarity(g.reshape(1, -1).double(), ref.reshape(1, -1).double()).item()
            tiny = ref.double().norm().item() < 1e-4 * gnorm
            assert not (tiny and pfx != "col."), ("only colour-branch tensors may fall under the tiny-tensor allowance", pfx + n_)
            gate_ = 2e-2 if tiny else 1e-2
            print("  %-22s rel %.3e cos %.5f |ref| %.3e%s" % (pfx + n_, re, cos, ref.norm().item(), "  (tiny: gate 2e-2)" if tiny else ""))
            worst = max(worst, re)
            if not (re < gate_ and cos > 0.9995):
                bad.append((pfx + n_, re, cos))
    print(shape, "worst per-tensor relative gradient error", worst)
    assert not bad, bad


# --------------------------------------------------------------------------------------------- SDF kernel at ragged sizes
@functools.lru_cache(maxsize=None)
def _engine(shape):
    """(renderer, engine, packed parameters, flat parameters as float64 on the host) of the seeded net of tests/engine_cases.py"""
    dev = torch.device("cuda")
    ren = seeded_renderer(PK.NetSpec(*shape), dev)
    eng = ren.engine
    flat = ren.flat_params().detach()
    return ren, eng, eng.pack(flat), flat.double().cpu().numpy()


@gpu
@shapes
def test_sdf_kernel_at_ragged_sizes_equals_the_padded_launch_bit_for_bit(shape):
    """avc_sdf_forward on 1, 31, 33 and 8 x 32 + 5 points (less than a wavefront's block, one past it, a ragged block behind a whole
    8-block row) against the same kernel on the points padded to a multiple of 32: the same bits on the common points"""
    _, eng, pk, _ = _engine(shape)
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(11)
    for n in (1, 31, 33, 8 * 32 + 5):
        pts = (torch.randn(n, 3, generator=g) * 0.4).to(dev)
        pad = (torch.randn((n + 31) // 32 * 32 - n, 3, generator=g) * 0.5).to(dev)
        assert pad.shape[0] > 0
        alone = eng.sdf_pts(pk, pts).cpu().reshape(-1)
        padded = eng.sdf_pts(pk, torch.cat([pts, pad])).cpu().reshape(-1)
        assert alone.shape[0] == n and padded.shape[0] % 32 == 0
        assert torch.equal(alone.view(torch.int32), padded[:n].view(torch.int32)), (n, (alone - padded[:n]).abs().max().item())
        assert torch.isfinite(padded).all() and alone.abs().max() > 0, n


# --------------------------------------------------------------------------------------------- stored panels, masks, column sums
class Run:
    pass


@functools.lru_cache(maxsize=None)
def _case(shape, R, S):
    """training forward + backward of R x S points in one slab: what the two kernels stored, decoded, and the emulator's reference with the
    kernel's own ReLU pattern (computed once, shared by the tests, never written to)"""
    from tests.engine_cases import _inputs
    _, eng, pk, flat = _engine(shape)
    spec = eng.spec
    dev = torch.device("cuda")
    r = Run()
    r.inputs = _inputs(R, S, dev, 1)
    ro, rd, z, dsdf, dn, drgb = r.inputs
    r.npts, r.nblk = R * S, (R * S + 31) // 32
    _, _, rgbf = eng.points_fwd_train(pk, ro, rd, z, SAMPLE_DIST)
    assert eng.plan(R, S) == (R, R)
    r.rows = int(eng.lib.avc_bwd_colsum_rows(r.npts, eng.MAX_BWD_WAVES))
    eng._colsum = torch.full((r.rows + 3, eng.dl.lay.cs_size), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    eng.points_bwd(pk, ro, rd, z, SAMPLE_DIST, dsdf, dn, drgb, rgbf, panels_valid=True)
    torch.cuda.synchronize()
    fp = eng._fpanels[:r.nblk * eng.fwd_tiles * 2048].cpu().numpy().view(np.uint16)
    gp = eng._gpanels[:r.nblk * eng.grad_tiles * 2048].cpu().numpy().view(np.uint16)
    masks = eng._masks[:r.nblk * eng.mask_u16].cpu().numpy().view(np.uint16)
    r.colsum = eng._colsum.cpu().numpy()
    r.F = PR.decode(fp, PR.F_REGION, eng.fwd_tiles, r.nblk)
    r.G = PR.decode(gp, PR.G_REGION, eng.grad_tiles, r.nblk)
    r.pattern = decode_masks(masks, spec, r.nblk)
    ro, rd, z, dsdf, dn, drgb = (a.cpu().numpy() for a in r.inputs)
    x = PR.midpoints(ro, rd, z, SAMPLE_DIST)
    r.ref = PR.reference_blocks(spec, flat, x, dsdf.reshape(-1), dn.reshape(-1, 3), drgb.reshape(-1, 6), relu_pattern=r.pattern)
    r.valid = PR.valid_lanes(r.nblk, r.npts)
    for a in (r.F, r.G, r.pattern, r.valid, r.colsum, *r.ref.values()):
        a.setflags(write=False)
    return r


def measure_panels(shape, R, S):
    """{group: largest e} of both regions and of the two column-sum parts -- what the gates are set from (profiles/net_shapes.md)"""
    r = _case(shape, R, S)
    _, eng, _, _ = _engine(shape)
    out = {}
    for region, got, ref in ((PR.F_REGION, r.F, r.ref["F"]), (PR.G_REGION, r.G, r.ref["G"])):
        for group, t0, nt in PR.groups(eng.dl.lay, region):
            out[group] = PR.compare(got[:, t0:t0 + nt], ref[:, t0:t0 + nt], group, PR.UNIT_ROUNDOFF[region], r.valid)
    cs = PR.compare_colsum(r.colsum[:r.rows].astype(np.float64).sum(0), r.ref["colsum"].sum(0), r.ref["colsum_abs"].sum(0), eng.spec)
    return out, cs


def _name(shape, R, S):
    return "%d_%d_%d %dx%d" % (shape + (R, S))


@gpu
@pytest.mark.parametrize("R,S", PANEL_SIZES)
@shapes
def test_stored_panels_and_column_sums_match_the_emulator_point_by_point(shape, R, S):
    """F region (h_l, PE values, g_a,l, feature, [x, n], r1 (, r2)) and G region (gbar_h, abar, ybar[1:], d_sdf, delta) of every valid
    point, group by group; the column sums of gbar_hs / gbar_h0 over the rows of the launch, every row written and none behind them"""
    r = _case(shape, R, S)
    _, eng, _, _ = _engine(shape)
    res, cs = measure_panels(shape, R, S)
    names = {g for region in (PR.F_REGION, PR.G_REGION) for g, _, _ in PR.groups(eng.dl.lay, region)}
    assert names == set(res) and ("R2" in names) == ("D2" in names) == (eng.spec.NCMID == 1)
    failures = []
    for group, c in res.items():
        print("panels %s %-5s e max %.3e mean %.3e (gate %.3e) rms %.3e" % (_name(shape, R, S), group, c.e_max, c.e_mean, gate(group), c.rms))
        assert c.rms > 0, group
        if not c.e_max <= gate(group):
            failures.append(c.where())
    assert not failures, "\n".join(failures)
    assert max(c.e_max for c in res.values()) > 0, "16-bit tiles of a 16-bit chain cannot equal float64 to the rounding"
    assert r.rows == 8 * min((r.nblk + 7) // 8, eng.MAX_BWD_WAVES // 8)
    bits = r.colsum.view(np.int32)
    assert not (bits[:r.rows] == NAN_BITS).any(), "a column-sum row of the launch was not written"
    assert (bits[r.rows:] == NAN_BITS).all(), "a row behind the launch's was written"
    assert np.isfinite(r.colsum[:r.rows]).all()
    for part, (e, col, got, ref) in cs.items():
        print("panels %s %-5s e max %.3e (gate %.3e) at column %d: got %.6g, reference %.6g" % (_name(shape, R, S), part, e, gate(part), col, got, ref))
        assert e <= gate(part), (part, e, col, got, ref)


@gpu
@pytest.mark.parametrize("R,S", PANEL_SIZES)
@shapes
def test_relu_masks_are_the_sign_of_the_stored_activations(shape, R, S):
    """every mask bit of a valid point equals (stored r > 0), exactly; the kernel's pattern differs from the reference's only where the
    reference's relu(r) is below the group's gate, and such values are under 2 % of the group"""
    r = _case(shape, R, S)
    _, eng, _, _ = _engine(shape)
    layers = [g for g in PR.groups(eng.dl.lay, PR.F_REGION) if g[0] in ("R1", "R2")]
    assert len(layers) == r.pattern.shape[1] == eng.spec.NCMID + 1
    sel = lambda tiles: tiles[np.broadcast_to(r.valid[:, None, None, :, None], tiles.shape)]
    for layer, (group, t0, nt) in enumerate(layers):
        stored, on = r.F[:, t0:t0 + nt], r.pattern[:, layer]
        bad = np.argwhere((on != (stored > 0)) & r.valid[:, None, None, :, None])
        assert not len(bad), "%s: %d mask bits differ from (stored value > 0), first at block %d, tile %d, k-step %d, lane %d, slot %d" % (
            (group, len(bad)) + tuple(int(v) for v in bad[0]))
        assert not (sel(stored) < 0).any(), group
        ref_r, stored_v, on_v = sel(r.ref["F"][:, t0:t0 + nt]), sel(stored), sel(on)
        rms = float(np.sqrt(np.mean(ref_r ** 2)))
        lost_above = int(((stored_v == 0) & (ref_r > max(PR.SMALLEST_F16, gate(group) * rms))).sum())
        share, ndiff, worst = PR.relu_ambiguity(ref_r, on_v, gate(group))
        print("masks %s %s: %d of %d patterns differ from the reference's (largest relu(r_ref) / rms among them %.3e, gate %.3e); stored "
              "zeros above the gate %d; share of the group in (0, gate x rms) %.4f" % (_name(shape, R, S), group, ndiff, ref_r.size, worst,
                                                                                      gate(group), lost_above, share))
        assert lost_above == 0, (group, lost_above)
        assert worst < gate(group), (group, worst)
        assert share < RELU_AMBIGUOUS_CAP, (group, share)


# --------------------------------------------------------------------------------------------- weight-gradient products
@gpu
@pytest.mark.parametrize("shape", [(128, 2, 1), (256, 1, 0), (64, 2, 1)], ids=["128_2_1", "256_1_0", "64_2_1"])
def test_production_pair_table_bit_for_bit(shape):
    """tests/test_gpu_wgrad.py: test_production_pair_tables_bit_for_bit at one new shape of each width: packing.region_local_pairs on
    integer panels, real FTILES / GTILES, the whole [gout | gbias]; 37 blocks in 5 splits leave a ragged last split (7, 7, 8, 7, 8)"""
    from tests.test_gpu_wgrad import SENTINEL, _check
    dev = torch.device("cuda")
    spec = PK.NetSpec(*shape)
    nblk, nsplit = 37, 5
    assert len({b - a for a, b in zip(W.splits(nblk, nsplit), W.splits(nblk, nsplit)[1:])}) > 1
    lc = W.production_launch(spec, nblk, 400 + spec.net_id)
    lay = PK.layout_for(spec)
    assert (lc.ftiles, lc.gtiles) == (lay.panel["FTILES"], lay.panel["GTILES"])
    po, pb = _check(lc, nsplit, dev)
    assert not (po[:nsplit, :lay.gout_size] == SENTINEL).any() and not (pb[:nsplit, :lay.gbias_size] == SENTINEL).any()


# --------------------------------------------------------------------------------------------- one whole iteration
@gpu
def test_train_clip_iterations_of_a_halved_full_size_conf_match_the_oracle_and_resume_from_a_checkpoint(tmp_path, monkeypatch):
    """A full-size conf with d_hidden = 128 (shape 128_2_1), stand-in CLIP, 32 x 32 rays, 32 + 32 samples: two train_clip_iterations
    against oracle/iteration_oracle.py by the statement and gates of tests/test_gpu_iteration.py's first-iteration parity tests.  Then
    the checkpoint round trip: a Runner that loads the saved checkpoint computes the third iteration's loss the running one computes.
    Both run the same kernels on weights the checkpoint stores exactly, so only the order of the atomics-free sums could differ: the
    bound is 1e-5 of the O(1) loss, a hundred fp32 roundings, where a lost Adam state or weight set moves it in the third digit."""
    import bench
    from avatarclip_amd.runner import Runner, clip_vit_random_state_dict, EllipsoidPrior
    from tests import test_gpu_iteration as TI
    made = []

    def halved_conf():
        conf = bench.make_conf(32, 64, small=False)                  # 32 + 32 samples per ray
        for key, v in (("model.sdf_network.d_hidden", 128), ("model.sdf_network.d_out", 129), ("model.rendering_network.d_hidden", 128),
                       ("model.rendering_network.d_feature", 128), ("general.base_exp_dir", str(tmp_path / "exp")),
                       ("train.use_bg_aug", False), ("train.warm_up_end", 0)):
            conf.put(key, v)
        return conf

    def make_runner(device, res, spp, small=True, **over):
        assert (res, spp, small, over) == (32, 64, False, {})
        torch.manual_seed(0)
        made.append(Runner(None, mode="train_clip", conf=halved_conf(), device=device))
        return made[-1]
    monkeypatch.setattr(TI, "_make_runner", make_runner)
    TI._run_parity(res=32, spp=64, iters=2, small=False)
    a = made[0]
    assert a.renderer.engine.spec == PK.NetSpec(128, 2, 1) and a.renderer.engine.net == 2
    assert (a.renderer.n_samples, a.renderer.n_importance) == (32, 32)
    # ---- checkpoint round trip
    dev = torch.device("cuda")
    a.iter_step = 2
    a.save_checkpoint()
    torch.manual_seed(1)                                             # other initial weights: everything must come from the checkpoint
    b = Runner(None, mode="train_clip", conf=halved_conf(), device=dev)
    b.init_clip(clip_state_dict=clip_vit_random_state_dict(0))
    prior = EllipsoidPrior(device="cpu")
    cam = (np.array([0.9, 0.3, 1.1], np.float32), np.array([0.0, 0.02, 0.0], np.float32), 0.7, 1.3, 1)
    pr = prior(cam[0], cam[1])
    b.init_smpl(prior_renderer=lambda eye, at: pr.to(dev))
    a.init_smpl(prior_renderer=lambda eye, at: pr.to(dev))
    b.load_checkpoint("ckpt_000002.pth")
    assert b.iter_step == 2
    for (n, pa), (_, pb) in zip(a.sdf_network.state_dict().items(), b.sdf_network.state_dict().items()):
        assert torch.equal(pa, pb), n
    b.update_learning_rate()
    jit = torch.rand(32 * 32, 1, generator=torch.Generator().manual_seed(102)).to(dev)
    losses = []
    for r in (a, b):
        render = type(r.renderer).render.__get__(r.renderer)      # (the parity leg left its own jitter wrapper on the instance)
        r.renderer.render = lambda *args, _f=render, **kw: _f(*args, jitter=jit, **kw)
        np.random.seed(4323)
        losses.append(r.train_clip_iteration(2, camera=cam).item())
    print("third iteration: running %.7f, resumed from the checkpoint %.7f" % tuple(losses))
    assert np.isfinite(losses).all() and abs(losses[0] - losses[1]) <= 1e-5 * max(1.0, abs(losses[0]))
    for pa, pb in zip(a.params_to_train, b.params_to_train):         # and the Adam step that followed used the same state
        assert torch.allclose(pa, pb, rtol=0, atol=0.2 * a.optimizer.param_groups[0]["lr"])
