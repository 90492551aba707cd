"""The per-ray kernels of csrc/avc_rays.hip -- avc_upsample_step(_lanes), avc_composite_fwd, avc_composite_bwd, avc_colsum -- sample by
sample against the float64 restatement of tests/rays_restatement.py (pinned on the CPU by tests/test_rays_restatement_cpu.py), at
every size at which their host or device code takes another path, R <= 67 rays, a few seconds per test.

Up-sampling: EVERY new depth is judged in CDF space (rays_restatement.judge_upsample; none is left out as by the 1% allowance of
  tests/test_gpu_kernels.py): residual <= tol_r = 1e-5 + n 2^-23 + 4 x the float32 CPU statement's residual on the same ray.  The
  merge is exact: z_out, sdf_out and slot equal the stable-sort restatement bit for bit.  Measured (profiles/rays_exact.md): the
  largest kernel / float32-statement residual ratio per (n, m) and the largest residual / tol_r.
Compositing against oracle.analytic in float64:
  S <= 128, families benign / thresholds / branches: the project's figures -- 2e-5 absolute forward, relative L2 1e-4 (d_sdf,
  d_normal) / 1e-5 (d_rgb), d_inv_s 1e-3 relative.  `inside` and the eikonal count are exact in every family (no mid-point is
  within 1e-4 of the radii 1.0 and 1.2).
  S > 128 and `saturated`: 4 x what oracle.analytic in float32 leaves against float64 on the same cases (rays_restatement.CO_F32_ERR,
  measured by the CPU module):
                  color    extra    weights  cdf      d_sdf    d_normal d_rgb    d_inv_s
    float32 stmt  1.2e-6   1.0e-6   7.5e-7   1.1e-7   7.0e-6   5.5e-7   2.5e-6   2.0e-7     (S > 128)
    allowed       4.8e-6   4.0e-6   3.0e-6   4.4e-7   2.8e-5   2.2e-6   1.0e-5   8.0e-7
    float32 stmt  1.2e-7   1.5e-7   5.6e-8   0                                              (saturated, every S; backward: finite)
    allowed       4.8e-7   6.0e-7   2.2e-7   0
  zero_normal: d_normal finite and torch.autograd's of the float64 statement (the eikonal term gives 0 at n = 0), relative L2 1e-4.
  Rays are independent: R = 1, 2, 3 reproduce the first rows of R = 5 bit for bit, and no launch touches the row past its last ray.
Column sums: small-integer floats whose partial sums stay below 2^24 -- any order is exact, the check is torch.equal.
"""
import pytest
import torch

from tests import rays_restatement as RR

gpu = pytest.mark.gpu
SENT = -777.0


def _L():
    from avatarclip_amd import lib as L
    L.load()
    return L


def D(t):
    return None if t is None else t.contiguous().to("cuda")


def _sentinel(shape, dtype=torch.float32):
    return torch.full(shape, SENT, dtype=dtype, device="cuda")


def _rows(bufs, R):
    """the first R rows of every buffer on the CPU; the row past them must still hold the sentinel"""
    torch.cuda.synchronize()
    out = []
    for b in bufs:
        b = b.cpu()
        assert (b[R:] == SENT).all(), "a launch wrote past its last ray"
        out.append(b[:R])
    return out


# ------------------------------------------------------------------------------------------------------------------------
# up-sampling
# ------------------------------------------------------------------------------------------------------------------------
def _upsample(ro, rd, z, sdf, m, inv_s, lanes):
    R, n = z.shape
    bufs = [_sentinel((R + 1, n + m)), _sentinel((R + 1, n + m)), _sentinel((R + 1, m)), _sentinel((R + 1, m), torch.int32)]
    _L().call("avc_upsample_step_lanes", D(ro), D(rd), D(z), D(sdf), R, n, m, float(inv_s), *bufs, lanes)
    return _rows(bufs, R)


@gpu
@pytest.mark.parametrize("n,m", RR.UP_SHAPES)
def test_upsample_every_sample_in_cdf_space_and_exact_merge(n, m):
    """n + m = 64 | 65 and 128 | 129 and m = 16 | 17 are the edges of the dispatch (16 / 32 lanes per ray / a wavefront); n - 1 > 128
    gives the 64-lane instantiation three and four values per lane in its scans; R = 1, 3, 5 leave wavefronts or lane groups of the last
    block without a ray; both routes (lanes = 0: as dispatched, 64: the 64-lane instantiation) are judged independently."""
    from oracle import neus_oracle as O
    fig = {0: [0.0, 0.0, None], 64: [0.0, 0.0, None]}
    failed = []
    for family, R, inv_s in RR.up_cases(n, m):
        ro, rd, z, sdf = RR.upsample_case(family, R, n, m, inv_s)
        ref = O.up_sample(ro, rd, z, sdf, m, inv_s)
        pre = None
        for lanes in (0, 64):
            z_out, sdf_out, z_new, slot = _upsample(ro, rd, z, sdf, m, inv_s, lanes)
            where = (family, R, inv_s, lanes)
            j = RR.judge_upsample(ro, rd, z, sdf, inv_s, z_new, ref_new=ref, pre=pre)
            pre = j["pre"]
            if j["ratio"] > fig[lanes][0]:
                fig[lanes][0], fig[lanes][2] = j["ratio"], where
            fig[lanes][1] = max(fig[lanes][1], j["worst"])
            if not j["ok"].all():       # (judged after the figures are out)
                failed.append((where, "samples failing", int((~j["ok"]).sum()), "steps 1, 2 ok:", bool(j["step1"].all()), bool(j["step2"].all()),
                               "largest residual / tol_r", j["worst"], "kernel / float32 statement", j["ratio"]))
            # the merge, exactly: the stable sort of cat([z, z_new]) with ties old-first
            want_out, want_slot, pos = RR.merge(z, z_new)
            assert torch.equal(z_out, torch.sort(torch.cat([z, z_new], -1), dim=-1)[0]) and torch.equal(z_out, want_out), where
            assert torch.equal(torch.gather(z_out, 1, slot.long()), z_new), where
            assert torch.equal(slot.long(), want_slot), where
            tie = z[:, :, None] == z_new[:, None, :]                                    # a new depth equal to an old one bit for bit ...
            assert (pos[:, :, None] < slot.long()[:, None, :])[tie].all(), where        # ... sits behind it
            keep = torch.ones_like(z_out, dtype=torch.bool).scatter_(1, slot.long(), False)
            assert torch.equal(sdf_out[keep].reshape(z.shape), sdf) and (torch.gather(sdf_out, 1, slot.long()) == 0).all(), where
    for lanes in (0, 64):
        print("upsample (n, m) = (%d, %d) lanes %2d: largest kernel / float32-statement residual ratio %.3f at %s; largest residual / tol_r %.3f"
              % (n, m, lanes, fig[lanes][0], fig[lanes][2], fig[lanes][1]))
    assert not failed, failed


@gpu
@pytest.mark.parametrize("n,m", [(1, 1), (200, 57), (100, 65)])
def test_upsample_refuses_sizes_outside_its_buffers(n, m):
    """n = 1, n + m = 257 and m = 65: a non-zero return with a message, and nothing is launched"""
    L = _L()
    R = 3
    g = torch.Generator().manual_seed(n)
    ro, rd = torch.zeros(R, 3), torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    z = torch.sort(torch.rand(R, n, generator=g) + 0.5, dim=-1)[0]
    bufs = [_sentinel((R, n + m)), _sentinel((R, n + m)), _sentinel((R, m)), _sentinel((R, m), torch.int32)]
    for lanes in (0, 64):
        with pytest.raises(RuntimeError, match="avc_upsample_step: need 2 <= n"):
            L.call("avc_upsample_step_lanes", D(ro), D(rd), D(z), D(z - 1.0), R, n, m, 64.0, *bufs, lanes)
    torch.cuda.synchronize()
    assert all((b == SENT).all() for b in bufs)


# ------------------------------------------------------------------------------------------------------------------------
# compositing
# ------------------------------------------------------------------------------------------------------------------------
FWD_OUT = ("color", "extra", "w", "P", "mid_z", "inside", "eik", "wstat", "nsum")
BWD_OUT = ("d_sdf", "d_n", "d_rgb6", "d_inv_s_ray")


def _bg(c, R, bg_mode):
    return None if bg_mode == 0 else (c["bg3"] if bg_mode == 1 else c["bg_ray"][:R])


def _composite_fwd(c, R, bg_mode, car, wstat=True, nsum=True):
    """avc_composite_fwd on the first R rays of the case -> dict of FWD_OUT (wstat as [2, R]; None where not asked for)"""
    S = c["z"].shape[1]
    bufs = [_sentinel((R + 1, 3)), _sentinel((R + 1, 3)), _sentinel((R + 1, S)), _sentinel((R + 1, S)), _sentinel((R + 1, S)),
            _sentinel((R + 1, S)), _sentinel((R + 1, 2)), _sentinel((2 * R + 1,)), _sentinel((R + 1, 3))]
    args = list(bufs)
    if not wstat:
        args[7] = None
    if not nsum:
        args[8] = None
    _L().call("avc_composite_fwd", D(c["sdf"][:R]), D(c["normal"][:R]), D(c["rgb"][:R]), D(c["z"][:R]), D(c["rays_o"][:R]),
              D(c["rays_d"][:R]), R, S, D(c["inv_s"]), float(c["sample_dist"]), float(car), D(_bg(c, R, bg_mode)), bg_mode, *args)
    torch.cuda.synchronize()
    if not wstat:
        assert (bufs[7] == SENT).all()
    if not nsum:
        assert (bufs[8] == SENT).all()
    out = dict(zip(FWD_OUT, _rows(bufs[:7], R) + _rows([bufs[7]], 2 * R) + _rows([bufs[8]], R)))
    out["wstat"] = out["wstat"].reshape(2, R) if wstat else None
    if not nsum:
        out["nsum"] = None
    return out


def _composite_bwd(c, R, bg_mode, car, eik_scale, d_w=True, d_n_up=True, d_wsum=True, d_nsum=True):
    """avc_composite_bwd on the first R rays; an upstream gradient is True (the case's), False (NULL) or 0 (explicit zeros)"""
    S = c["z"].shape[1]
    bufs = [_sentinel((R + 1, S)), _sentinel((R + 1, S, 3)), _sentinel((R + 1, S, 6)), _sentinel((R + 1,))]
    up = [None if f is False else D(c[k][:R] if f is True else torch.zeros_like(c[k][:R]))
          for k, f in (("d_w", d_w), ("d_n_up", d_n_up), ("d_wsum", d_wsum), ("d_nsum", d_nsum))]
    _L().call("avc_composite_bwd", D(c["sdf"][:R]), D(c["normal"][:R]), D(c["rgb"][:R]), D(c["z"][:R]), D(c["rays_o"][:R]),
              D(c["rays_d"][:R]), R, S, D(c["inv_s"]), float(c["sample_dist"]), float(car), D(_bg(c, R, bg_mode)), bg_mode,
              D(c["d_color"][:R]), D(c["d_extra"][:R]), *up, D(eik_scale), *bufs)
    return dict(zip(BWD_OUT, _rows(bufs, R)))


@gpu
@pytest.mark.parametrize("S", RR.CO_S)
def test_composite_forward_backward_every_sample(S):
    """S = 1, 2: a lane or two; 63 | 64 | 65 and 128 | 129, 192 | 255 | 256: one to four values per lane in the prefix, suffix and affine
    scans; R = 1, 2, 3: wavefronts of the block without a ray; every bg_mode and cos_anneal 0, 0.3, 1; the five input families."""
    worst, failed = {}, []
    for kind in RR.CO_FAMILIES:
        tol = RR.composite_tolerances(kind, S)
        for bg_mode in (0, 1, 2):
            for car in RR.CO_ANNEAL:
                where = (kind, S, bg_mode, car)
                c = RR.composite_case(kind, 5, S, RR.composite_seed(S, bg_mode, car))
                ref = RR.composite_reference(c, bg_mode, car)
                cf, cb, eik_scale = ref
                f = _composite_fwd(c, 5, bg_mode, car)
                b = _composite_bwd(c, 5, bg_mode, car, eik_scale)
                for k, v in {**f, **b}.items():
                    assert torch.isfinite(v).all(), (where, k)
                pn = RR.composite_pn(c)
                assert torch.equal(f["inside"], (pn < 1.0).float()) and torch.equal(f["eik"][:, 1], (pn < 1.2).float().sum(-1)), where
                assert torch.allclose(f["mid_z"].double(), c["z"].double() + cf["dists"] * 0.5, atol=1e-6), where
                assert torch.allclose(f["eik"][:, 0].double(), (cf["relax"] * (cf["gn"] - 1) ** 2).sum(-1), rtol=1e-5, atol=1e-5), where
                # the per-ray reductions of the weights handed out beside them, as test_composite_forward_backward_fp32 checks them
                assert torch.allclose(f["wstat"][0], f["w"].sum(-1), atol=1e-5) and torch.allclose(f["wstat"][1], f["w"].max(-1)[0], atol=1e-7)
                assert torch.allclose(f["nsum"], (c["normal"] * f["w"][..., None]).sum(1), atol=1e-5), where
                err = RR.composite_errors({**f, **b}, ref, kind)
                for k, v in err.items():
                    key = (kind if kind == "saturated" else "other", k)
                    worst[key] = max(worst.get(key, 0.0), v)
                bad = {k: (v, tol[k]) for k, v in err.items() if not v <= tol[k]}
                if bad:                   # (judged after the figures are out)
                    failed.append((where, "error, allowed:", bad))
                if kind == "zero_normal":
                    d_n = RR.composite_autograd(c, bg_mode, car)
                    assert float((b["d_n"].double() - d_n).norm() / d_n.norm()) < 1e-4 and (b["d_n"][:, 0].double() - d_n[:, 0]).abs().max() < 1e-5, where
                for R in (1, 2, 3):       # rays are independent: fewer of them change no bit of the ones that stay
                    fr, br = _composite_fwd(c, R, bg_mode, car), _composite_bwd(c, R, bg_mode, car, eik_scale)
                    for k in FWD_OUT:
                        assert torch.equal(fr[k], f[k][:, :R] if k == "wstat" else f[k][:R]), (where, R, k)
                    for k in BWD_OUT:
                        assert torch.equal(br[k], b[k][:R]), (where, R, k)
    print("composite S = %d: largest error per output" % S, {"%s %s" % k: "%.2e" % v for k, v in sorted(worst.items())})
    assert not failed, failed


@gpu
@pytest.mark.parametrize("S", [1, 65, 256])
def test_composite_optional_pointers(S):
    """d_weights, d_normal_up, d_wsum, d_nsum as NULL equal explicit zeros bit for bit; wstat / nsum as NULL leave every other output
    as it is; S outside 1..256 is refused and nothing is launched"""
    L = _L()
    c = RR.composite_case("benign", 3, S, 5000 + S)
    eik_scale = torch.tensor([0.01])
    for bg_mode, car in ((0, 0.0), (1, 0.3), (2, 1.0)):
        full = _composite_fwd(c, 3, bg_mode, car)
        for wstat, nsum in ((False, True), (True, False), (False, False)):
            part = _composite_fwd(c, 3, bg_mode, car, wstat=wstat, nsum=nsum)
            for k in FWD_OUT:
                assert part[k] is None or torch.equal(part[k], full[k]), (S, bg_mode, wstat, nsum, k)
        for null in ((False, True, True, True), (True, False, True, True), (True, True, False, True), (True, True, True, False),
                     (False, False, False, False)):
            a = _composite_bwd(c, 3, bg_mode, car, eik_scale, *null)
            z = _composite_bwd(c, 3, bg_mode, car, eik_scale, *[f if f else 0 for f in null])
            for k in BWD_OUT:
                assert torch.isfinite(a[k]).all() and torch.equal(a[k], z[k]), (S, bg_mode, null, k)
    out = _sentinel((3, 3))
    for bad_S in (0, 257):
        with pytest.raises(RuntimeError, match="1 <= S <= 256"):
            L.call("avc_composite_fwd", D(c["sdf"]), D(c["normal"]), D(c["rgb"]), D(c["z"]), D(c["rays_o"]), D(c["rays_d"]), 3, bad_S,
                   D(c["inv_s"]), 0.0625, 0.3, None, 0, out, out, out, out, out, out, out, None, None)
        with pytest.raises(RuntimeError, match="1 <= S <= 256"):
            L.call("avc_composite_bwd", D(c["sdf"]), D(c["normal"]), D(c["rgb"]), D(c["z"]), D(c["rays_o"]), D(c["rays_d"]), 3, bad_S,
                   D(c["inv_s"]), 0.0625, 0.3, None, 0, D(c["d_color"]), D(c["d_extra"]), None, None, None, None, D(eik_scale), out, out, out, out)
    torch.cuda.synchronize()
    assert (out == SENT).all()


# ------------------------------------------------------------------------------------------------------------------------
# column sums
# ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("R", [0, 1, 1023, 1025, 4096, 4097, 262144, 262145])
def test_colsum_exact_at_its_block_edges(R):
    """1024 rows per pass of a workgroup, 4096 rows per workgroup, at most 64 workgroups (R > 262144); the last workgroup to finish adds
    the partial sums and leaves the ticket word zero, so a second call on the same scratch is right as well; out[C:] stays untouched."""
    L = _L()
    lib = L.load()
    g = torch.Generator().manual_seed(R)
    scr = torch.zeros(lib.avc_colsum_scratch_bytes(), dtype=torch.uint8, device="cuda")
    for C, mode in ((1, 0), (2, 0), (3, 0), (4, 0), (2, 1)):
        x = torch.randint(0, 4, (R, C), generator=g).float()                   # every partial sum <= 3 * 262145 < 2^24: exact in any order
        s = x.long().sum(0)
        want = s.float()
        xd = D(x) if R > 0 else None
        for call in range(2):
            out = _sentinel((8,))
            L.call("avc_colsum", xd, R, C, mode, out, scr)
            torch.cuda.synchronize()
            got = out.cpu()
            assert (got[C:] == SENT).all(), (R, C, mode, call)
            if mode == 0:
                assert torch.equal(got[:C], want), (R, C, call, got, want)
            else:                                                              # out[1] = s1 + 1e-5 (float32), out[0] = s0 / out[1]
                den = want[1] + torch.tensor(1e-5, dtype=torch.float32)
                assert got[1] == den and abs(got[0].item() - (want[0] / den).item()) <= 2.0 ** -23 * (want[0] / den).item(), (R, call, got)
                if R == 0:
                    assert got[0] == 0 and got[1] == torch.tensor(1e-5, dtype=torch.float32)
            assert int(scr.view(torch.int32)[-1]) == 0, "the ticket word is left zero"


@gpu
def test_colsum_refuses_what_it_cannot_sum():
    L = _L()
    lib = L.load()
    x, out = torch.ones(16, 5, device="cuda"), _sentinel((8,))
    scr = torch.zeros(lib.avc_colsum_scratch_bytes(), dtype=torch.uint8, device="cuda")
    for C, mode in ((5, 0), (0, 0), (3, 1), (1, 1)):
        with pytest.raises(RuntimeError, match="avc_colsum: 1 <= C <= 4"):
            L.call("avc_colsum", x, 16, C, mode, out, scr)
    torch.cuda.synchronize()
    assert (out == SENT).all() and not scr.any()
