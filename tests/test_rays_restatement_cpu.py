"""tests/rays_restatement.py against oracle/neus_oracle.py, the reference's own recorded up-sampling steps and its own claims (no GPU):
the float64 restatement IS the oracle's up_sample / cat_z_vals; the criterion `judge_upsample` accepts the reference's records and the
float32 statement on every case of the GPU table (tests/test_gpu_rays_exact.py) and rejects the wrong samplers; the inputs keep the
margins the GPU tests rely on.  What each deliberately wrong sampler does under the criterion is in profiles/rays_exact.md."""
import pytest
import torch

from oracle import neus_oracle as O
from tests import rays_restatement as RR
from tests.helpers import load_case, relerr


@pytest.mark.parametrize("n,m", RR.UP_SHAPES)
def test_restatement_is_the_oracle_in_float64(n, m):
    """upsample_cdf + invert_cdf in float64 == O.up_sample in float64, sampler_f32 == O.up_sample in float32, merge == O.cat_z_vals:
    all bit for bit, on every input family (duplicate depths included: ties old-first)"""
    for family in RR.UP_FAMILIES:
        for inv_s in RR.UP_INV_S:
            ro, rd, z, sdf = RR.upsample_case(family, 5, n, m, inv_s)
            cdf = RR.upsample_cdf(ro, rd, z, sdf, inv_s)
            assert cdf.dtype == torch.float64 and cdf.shape == (5, n)
            u = RR.u_values(m, torch.float64)[None, :].expand(5, m)
            ref64 = O.up_sample(ro.double(), rd.double(), z.double(), sdf.double(), m, inv_s)
            assert torch.equal(RR.invert_cdf(cdf, z.double(), u), ref64), (family, inv_s)
            ref32 = O.up_sample(ro, rd, z, sdf, m, inv_s)
            assert torch.equal(RR.sampler_f32(ro, rd, z, sdf, m, inv_s), ref32), (family, inv_s)
            for new in (ref32, z[:, :m].contiguous()):                 # (the second: every new depth ties with an old one)
                z_out, slot, pos = RR.merge(z, new)
                z_sorted, index = torch.sort(torch.cat([z, new], -1), dim=-1, stable=True)
                assert torch.equal(z_out, z_sorted) and torch.equal(z_out, O.cat_z_vals(None, ro, rd, z, new, None, last=True)[0])
                assert torch.equal(torch.gather(index, 1, slot), n + torch.arange(m)[None, :].expand(5, m))
                assert torch.equal(torch.gather(index, 1, pos), torch.arange(n)[None, :].expand(5, n))


@pytest.mark.parametrize("name", ["neus_small.npz", "neus_full.npz", "neus_full_128.npz"])
def test_the_references_recorded_steps_pass_the_criterion(name):
    rec = load_case(name)[0]
    for i in range(4):
        z, sdf, new = rec["up%d_z_in" % i].contiguous(), rec["up%d_sdf_in" % i].contiguous(), rec["up%d_new_z" % i]
        j = RR.judge_upsample(rec["rays_o"], rec["rays_d"], z, sdf, 64.0 * 2 ** i, new)
        print(name, i, "worst residual / tol_r %.3f" % j["worst"], "borderline %.4f" % j["borderline"].float().mean().item())
        assert j["ok"].all(), (name, i, int((~j["ok"]).sum()), j["worst"])


@pytest.mark.parametrize("n,m", RR.UP_SHAPES)
def test_criterion_accepts_the_float32_statement_and_rejects_the_wrong_samplers(n, m):
    """Per case of the GPU table: the float32 statement passes, at most 2% of its samples sit in borderline bins (judged on the
    float64 restatement alone), and each wrong sampler fails for at least one sample wherever it is wrong on that input, which is
    decided from float64 alone: some sample moves by more than 2 tol_r in CDF space (RR.mutation_displacement).  The three entries that
    are no wrong samplers are shown to be none: `same` returns the honest samples bit for bit, `sub_ulp` moves u by <= 2^-23."""
    must = {k: 0 for k, v in RR.MUTATIONS.items() if v == "reject"}
    cases = RR.up_cases(n, m)
    for family, R, inv_s in cases:
        ro, rd, z, sdf = RR.upsample_case(family, R, n, m, inv_s)
        if family == "dup":
            assert ((z[:, 1:] == z[:, :-1]).sum(-1) >= 1).all()
        if family == "miss":
            assert (ro[:, None, :] + rd[:, None, :] * z[..., None]).norm(dim=-1).min() > 1.5
        ref = O.up_sample(ro, rd, z, sdf, m, inv_s)
        j = RR.judge_upsample(ro, rd, z, sdf, inv_s, ref, ref_new=ref)
        assert j["ok"].all(), (family, R, inv_s, j["worst"])
        assert j["ref_residual"].max() < 2.5e-3            # (tol_r stays far below the 0.5 / 64 that a wrong u moves a sample by)
        assert j["borderline"].float().mean() <= 0.02, (family, R, inv_s)
        assert not j["thin"].any()                         # tol_r >= 1e-5: step 3 of the criterion judges no sample (module docstring)
        cdf = j["pre"][0]
        for mutation, kind in RR.MUTATIONS.items():
            new = RR.sampler_f32(ro, rd, z, sdf, m, inv_s, mutation)
            if kind == "same":
                assert torch.equal(new, ref), (mutation, family, R, inv_s)
                continue
            v = RR.judge_upsample(ro, rd, z, sdf, inv_s, new, pre=j["pre"])
            if kind == "sub_ulp":
                assert (RR.u_affine(m) - RR.u_values(m)).abs().max() <= 2.0 ** -23 and v["ok"].all(), (mutation, family, R, inv_s)
                continue
            wrong = bool((RR.mutation_displacement(cdf, z, m, mutation) > 2 * j["tol"]).any())
            must[mutation] += wrong
            assert not wrong or not v["ok"].all(), (mutation, family, R, inv_s)
    print((n, m), "cases", len(cases), "of which the sampler is wrong on (and rejected in):", must)
    # the mistakes are mistakes on most inputs: a wrong u wherever there is a neighbour (m >= 2) or an end (always), bar rays that
    # are one zero-width bin; the doubled bin wherever a sample lies behind the middle of the ray and the bin holds mass
    assert must["u_endpoints"] >= len(cases) - 10 and (m == 1 or must["last_u"] >= len(cases) - 10)
    assert (must["last_u"] == 0) == (m == 1) and (m == 1 or must["half_bin_twice"] >= 30)


def test_composite_families_keep_their_margins():
    for S in RR.CO_S:
        for kind in RR.CO_FAMILIES:
            c = RR.composite_case(kind, 5, S, 1000 * S)
            pn = RR.composite_pn(c)
            assert RR.composite_margin(c) >= 1e-4, (kind, S)
            cs = (c["rays_d"].double()[:, None, :] * c["normal"].double()).sum(-1)
            if kind == "thresholds" and S >= 63:          # every ray has mid-points in all three shells
                assert ((pn < 1.0).any(-1) & ((pn > 1.0) & (pn < 1.2)).any(-1) & (pn > 1.2).any(-1)).all(), S
            if kind == "thresholds" and S <= 2:           # too few samples to cross: the rays lie on different sides
                assert len(set((pn[:, 0] < 1.0).tolist())) + len(set((pn[:, 0] < 1.2).tolist())) >= 3, S
            if kind == "branches":
                assert torch.minimum(cs.abs(), (cs - 1).abs()).min() >= 5e-3, S
                if S >= 63:                               # -c/2 + 1/2 and -c each take both signs within every ray
                    assert ((cs > 1).any(-1) & (cs < 1).any(-1) & (cs > 0).any(-1) & (cs < 0).any(-1)).all(), S
            if kind == "zero_normal":
                assert (c["normal"][:, 0] == 0).all() and (pn[:, 0] < 1.2 - 1e-4).all() and (c["normal"][:, 1:].norm(dim=-1) > 0).all()
            if kind == "saturated":                       # float32: every alpha is 0, 1 or the 1e-5 / (1 + 1e-5) of P = Q = 1
                for car in RR.CO_ANNEAL:
                    cf = RR.composite_reference(c, 0, car, dtype=torch.float32)[0]
                    assert ((cf["alpha"] == 1) | (cf["alpha"] < 1.0001e-5)).all() and ((cf["P"] == 0) | (cf["P"] == 1)).all()
                    assert (cf["w"].sum(-1) < 1.0001).all() and (S < 63 or (cf["w"].max(-1)[0] > 0.99).all())   # one sample takes the weight
            else:
                assert RR.composite_clip_margin(c) >= 5e-6, (kind, S)


@pytest.mark.parametrize("S", [1, 2, 65, 256])
def test_zero_normal_gradient_is_torch_autograds(S):
    """oracle.analytic.composite_backward on a zero normal inside |p| < 1.2: finite, and torch.autograd's gradient of the float64
    statement (linalg.norm's backward gives 0 at 0, so the eikonal term contributes nothing there)"""
    for bg_mode, car in ((0, 0.0), (1, 0.3), (2, 1.0)):
        c = RR.composite_case("zero_normal", 5, S, 1000 * S + 1)
        cf, cb, _ = RR.composite_reference(c, bg_mode, car)
        assert all(torch.isfinite(v).all() for v in cb.values())
        d_n = RR.composite_autograd(c, bg_mode, car)
        assert relerr(cb["d_n"], d_n) < 1e-12 and (d_n[:, 0] - cb["d_n"][:, 0]).abs().max() < 1e-14


def test_float32_statement_error_behind_the_composite_tolerances():
    """The tolerances of tests/test_gpu_rays_exact.py for S > 128 and for the saturated family are 4 x RR.CO_F32_ERR; those figures
    are what oracle.analytic's composite_forward / _backward in float32 leave against float64 on the very cases of the GPU table
    (R = 5, every bg_mode and cos_anneal): never more, and the largest within a factor 1.5 of the figure."""
    seen = {}
    for S in RR.CO_S:
        for kind in RR.CO_FAMILIES:
            if S <= 128 and kind != "saturated":
                continue
            for bg_mode in (0, 1, 2):
                for car in RR.CO_ANNEAL:
                    c = RR.composite_case(kind, 5, S, RR.composite_seed(S, bg_mode, car))
                    for k, v in RR.composite_errors(RR.composite_reference(c, bg_mode, car, dtype=torch.float32),
                                                    RR.composite_reference(c, bg_mode, car), kind).items():
                        key = ("saturated" if kind == "saturated" else "S>128", k)
                        seen[key] = max(seen.get(key, 0.0), v)
    for key, v in sorted(seen.items()):
        print(key, "%.3e" % v, "figure %.3e" % RR.CO_F32_ERR[key[0]][key[1]])
    for key, v in sorted(seen.items()):
        assert v <= RR.CO_F32_ERR[key[0]][key[1]] <= max(1.5 * v, 1e-30), key
