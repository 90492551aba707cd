"""Float64 restatement of the per-ray kernels of csrc/avc_rays.hip and the criterion their up-sampling step is judged by.

TEST INFRASTRUCTURE ONLY (CPU, torch).  tests/test_rays_restatement_cpu.py pins this module against oracle/neus_oracle.py and the
reference's own recorded steps; tests/test_gpu_rays_exact.py judges the kernels with it.

The up-sampling step inverts a piecewise-linear CDF F (z_i -> cdf_i) at m fixed u_j.  Where the pdf is flat the inverse is
ill-conditioned, so a bound on |z_new - z_ref| has to leave some samples out (tests/test_gpu_kernels.py lets 1% be wrong by any
amount).  The forward map is well-conditioned everywhere: |u_j - F(z_new_j)| is small for EVERY sample of a right sampler, whatever
the pdf looks like, and an index or scan bug moves a sample by a bin's worth of CDF.  `judge_upsample` judges every sample that way:

  1. z_new is non-decreasing along the ray and lies in [z_0, z_{n-1}]                                     (float32, exact)
  2. residual = dist(u_j, F(z_new_j)) <= tol_r      (F(z) is the interval [cdf_i, cdf_{i+1}] where z lies in a zero-width bin)
  3. a sample whose bin has den = cdf_{i+1} - cdf_i < 1e-5 - tol_r (the reference's `denom := 1` branch, where step 2 says nothing
     about the position inside the bin) also has |z_new - (Z_b + (u - cdf_b) dZ)| <= tol_r dZ + 2^-22 |z_new|
  4. a bin with |den - 1e-5| <= tol_r is borderline: steps 1 and 2 only

  tol_r (per ray) = 1e-5 + n 2^-23 + 4 x the largest residual the float32 CPU statement (oracle.neus_oracle.up_sample) leaves on
  that ray: the reference's own threshold below which its output is no inversion, an n-term float32 cumulative sum in any order,
  and 4 x for the kernel's summation order and its __expf sigmoid.

Since tol_r >= 1e-5, `den < 1e-5 - tol_r` holds for no bin: step 3 is stated as the criterion was set but judges nothing, and every
bin with den <= 1e-5 + tol_r is a borderline bin.  What that leaves open is the position of a sample inside a bin that holds less
than tol_r of the ray's mass (profiles/rays_exact.md).
"""
import torch

from oracle import neus_oracle as O

UP_SHAPES = [(2, 1), (3, 2), (32, 8), (56, 8), (48, 16), (49, 16), (63, 1), (112, 16), (113, 16), (64, 17), (129, 8), (192, 64),
             (255, 1)]
UP_RAYS = (1, 3, 5, 17, 67)
UP_INV_S = (64.0, 512.0)
UP_FAMILIES = ("sphere_grid", "random", "miss", "const", "dup", "sharp")

CO_S = (1, 2, 63, 64, 65, 128, 129, 192, 255, 256)
CO_RAYS = (1, 2, 3, 5)
CO_ANNEAL = (0.0, 0.3, 1.0)
CO_FAMILIES = ("benign", "thresholds", "branches", "saturated", "zero_normal")
SAMPLE_DIST = 2.0 / 32


# ------------------------------------------------------------------------------------------------------------------------
# up-sampling: inputs
# ------------------------------------------------------------------------------------------------------------------------
def up_cases(n, m):
    """the (family, R, inv_s) of one (n, m) of the GPU table; the sharp surface exists at inv_s = 512 only"""
    return [(f, R, s) for f in UP_FAMILIES for R in UP_RAYS for s in UP_INV_S if not (f == "sharp" and s != 512.0)]


def upsample_case(family, R, n, m, inv_s):
    """float32 (rays_o, rays_d, z, sdf) of one case; the seed is a function of the case alone"""
    g = torch.Generator().manual_seed(1000003 * UP_FAMILIES.index(family) + 7919 * R + 31 * n + m + int(inv_s))
    rd = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    if family == "miss":        # the origin 2.5 away, the direction at right angles to it: no point comes nearer than 2.5 - 0.2
        e = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
        rd = torch.nn.functional.normalize(rd - (rd * e).sum(-1, keepdim=True) * e, dim=-1)
        ro = 2.5 * e + 0.05 * torch.randn(R, 3, generator=g)
    else:
        ro = torch.randn(R, 3, generator=g) * 0.2
    if family in ("sphere_grid", "sharp"):      # a jittered grid: every cell of 2 / n holds one depth
        z = 0.2 + 2.0 * (torch.arange(n)[None, :] + 0.5 + 0.8 * (torch.rand(R, n, generator=g) - 0.5)) / n
    else:                                       # sorted uniform-random depths: tiny gaps
        z = torch.sort(torch.rand(R, n, generator=g) * 2 + 0.2, dim=-1)[0]
    if family == "dup":                         # exact duplicates: one pair per ray, two where there is room
        k = torch.randint(0, n - 1, (R,), generator=g)
        z[torch.arange(R), k + 1] = z[torch.arange(R), k]
        if n >= 8:
            k2 = (k + n // 2) % (n - 1)
            z[torch.arange(R), k2 + 1] = z[torch.arange(R), k2]
        z = torch.sort(z, dim=-1)[0]
    z = z.float().contiguous()
    rad = (ro[:, None, :] + rd[:, None, :] * z[..., None]).norm(dim=-1)
    if family == "const":
        sdf = torch.full((R, n), 0.1)
    elif family == "sharp":
        sdf = rad - 0.6
    else:
        sdf = rad - 0.6 + 0.02 * torch.randn(R, n, generator=g)
    return ro.float().contiguous(), rd.float().contiguous(), z, sdf.float().contiguous()


# ------------------------------------------------------------------------------------------------------------------------
# up-sampling: the reference's cdf, its inversion, the merge
# ------------------------------------------------------------------------------------------------------------------------
def upsample_cdf(rays_o, rays_d, z, sdf, inv_s):
    """the reference's cdf [R, n] (renderer.py:133-158 + sample_pdf's first four lines) in float64 from float32 inputs"""
    ro, rd, z, sdf = rays_o.double(), rays_d.double(), z.double(), sdf.double()
    R, n = z.shape
    radius = torch.linalg.norm(ro[:, None, :] + rd[:, None, :] * z[..., :, None], ord=2, dim=-1)
    inside = (radius[:, :-1] < 1.0) | (radius[:, 1:] < 1.0)
    dz = z[:, 1:] - z[:, :-1]
    mid = (sdf[:, :-1] + sdf[:, 1:]) * 0.5
    cos = (sdf[:, 1:] - sdf[:, :-1]) / (dz + 1e-5)
    prev = torch.cat([torch.zeros(R, 1, dtype=z.dtype), cos[:, :-1]], -1)
    cos = torch.minimum(prev, cos).clip(-1e3, 0.0) * inside
    pc = torch.sigmoid((mid - cos * dz * 0.5) * inv_s)
    nc = torch.sigmoid((mid + cos * dz * 0.5) * inv_s)
    alpha = (pc - nc + 1e-5) / (pc + 1e-5)
    w = alpha * torch.cumprod(torch.cat([torch.ones(R, 1, dtype=z.dtype), 1.0 - alpha + 1e-7], -1), -1)[:, :-1]
    w = w + 1e-5
    pdf = w / torch.sum(w, -1, keepdim=True)
    return torch.cat([torch.zeros(R, 1, dtype=z.dtype), torch.cumsum(pdf, -1)], -1)


def u_values(m, dtype=torch.float32):
    return torch.linspace(0.5 / m, 1.0 - 0.5 / m, steps=m, dtype=dtype)


def invert_cdf(cdf, z, u, right=True):
    """sample_pdf's inversion (renderer.py:52-68) of `cdf` over the bins `z` at `u` [R, m], in the dtype of its arguments"""
    n = cdf.shape[-1]
    inds = torch.searchsorted(cdf.contiguous(), u.contiguous(), right=right)
    below, above = torch.clamp(inds - 1, min=0), torch.clamp(inds, max=n - 1)
    cb, ca = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    zb, za = torch.gather(z, 1, below), torch.gather(z, 1, above)
    den = ca - cb
    den = torch.where(den < 1e-5, torch.ones_like(den), den)
    return zb + (u - cb) / den * (za - zb)


def merge(z, z_new):
    """cat_z_vals' stable sort of cat([z, z_new]) restated by counting: an old sample moves up by the new ones below it, a new one
    by the old ones at or below it (ties: old first).  -> z_out [R, n + m], slot [R, m] of the new samples, pos [R, n] of the old"""
    R, n = z.shape
    m = z_new.shape[1]
    pos = torch.arange(n)[None, :] + (z_new[:, None, :] < z[:, :, None]).sum(-1)
    slot = torch.arange(m)[None, :] + (z[:, None, :] <= z_new[:, :, None]).sum(-1)
    z_out = torch.empty(R, n + m, dtype=z.dtype)
    z_out.scatter_(1, pos, z)
    z_out.scatter_(1, slot, z_new)
    return z_out, slot, pos


def cdf_residual(cdf, z, z_new, m):
    """per new sample: the distance from u_j (the float32 linspace value) to F(z_new_j), F the piecewise-linear map z_i -> cdf_i
    and, where z_new_j lies in zero-width bins, the interval of their cdf values; the containing bin b (of the bins whose closed
    depth range holds z_new_j, the one nearest to u_j in cdf), its den = cdf_{b+1} - cdf_b and width dZ.
    -> dict(residual, den, dz, bin, u), all [R, m], float64 / int64"""
    cdf, z, zn = cdf.double(), z.double().contiguous(), z_new.double().contiguous()
    R, n = z.shape
    u = u_values(m).double()[None, :].expand(R, m)
    lo = torch.searchsorted(z, zn, right=False)           # first old depth >= z_new
    hi = torch.searchsorted(z, zn, right=True)            # first old depth >  z_new
    i0 = torch.clamp(lo - 1, 0, n - 2)                    # bins i with z_i <= z_new <= z_{i+1}: lo - 1 .. hi - 1
    i1 = torch.maximum(torch.clamp(hi - 1, 0, n - 2), i0)

    def image(i, upper):
        za, zb = torch.gather(z, 1, i), torch.gather(z, 1, i + 1)
        ca, cb = torch.gather(cdf, 1, i), torch.gather(cdf, 1, i + 1)
        wide = zb > za
        frac = torch.where(wide, (zn - za) / torch.where(wide, zb - za, torch.ones_like(za)), torch.full_like(za, float(upper)))
        return ca + frac.clip(0.0, 1.0) * (cb - ca)
    f_lo, f_hi = image(i0, False), image(i1, True)
    residual = torch.maximum(torch.maximum(f_lo - u, u - f_hi), torch.zeros_like(u))
    b = torch.minimum(torch.maximum(torch.searchsorted(cdf.contiguous(), u.contiguous(), right=True) - 1, i0), i1)
    cb = torch.gather(cdf, 1, b)
    zb = torch.gather(z, 1, b)
    return dict(residual=residual, den=torch.gather(cdf, 1, b + 1) - cb, dz=torch.gather(z, 1, b + 1) - zb, bin=b, u=u,
                cdf_b=cb, z_b=zb)


def judge_upsample(rays_o, rays_d, z, sdf, inv_s, z_new, ref_new=None, pre=None):
    """The criterion of the module docstring on z_new [R, m] (float32).  `ref_new`: the float32 CPU statement's samples of the same
    inputs (computed here when not given); `pre`: the `pre` of an earlier verdict on the same inputs, which spares computing the cdf
    and the statement's residual again.  -> dict: ok [R, m] (every sample is judged), the masks and figures behind it, `worst` = the
    largest residual / tol_r, `ratio` = the case's largest residual / the float32 statement's largest residual."""
    R, n = z.shape
    m = z_new.shape[1]
    if pre is None:
        if ref_new is None:
            ref_new = O.up_sample(rays_o, rays_d, z, sdf, m, float(inv_s))
        cdf = upsample_cdf(rays_o, rays_d, z, sdf, inv_s)
        ref_res = cdf_residual(cdf, z, ref_new, m)["residual"].max(-1)[0]
        pre = (cdf, ref_res)
    cdf, ref_res = pre
    tol = (1e-5 + n * 2.0 ** -23 + 4.0 * ref_res)[:, None]
    r = cdf_residual(cdf, z, z_new, m)
    zn = z_new.float()
    mono = torch.ones(R, m, dtype=torch.bool)
    mono[:, 1:] = zn[:, 1:] >= zn[:, :-1]
    step1 = mono & (zn >= z[:, :1]) & (zn <= z[:, -1:]) & torch.isfinite(zn)
    step2 = r["residual"] <= tol
    thin = r["den"] < 1e-5 - tol
    borderline = (r["den"] - 1e-5).abs() <= tol
    znd = zn.double()
    step3 = (znd - (r["z_b"] + (r["u"] - r["cdf_b"]) * r["dz"])).abs() <= tol * r["dz"] + 2.0 ** -22 * znd.abs()
    ok = step1 & step2 & (~thin | step3)
    return dict(ok=ok, step1=step1, step2=step2, thin=thin, borderline=borderline, residual=r["residual"], tol=tol, den=r["den"],
                ref_residual=ref_res, pre=pre, worst=float((r["residual"] / tol).max()),
                ratio=float(r["residual"].max() / ref_res.max().clamp_min(1e-30)))


# ------------------------------------------------------------------------------------------------------------------------
# up-sampling: the float32 statement with one thing wrong at a time
# ------------------------------------------------------------------------------------------------------------------------
# name -> what test_rays_restatement_cpu.py asserts of it (profiles/rays_exact.md gives the reasons):
#   "reject"      a wrong sampler: at least one sample of every case it applies to fails the criterion
#   "same"        no wrong sampler: its samples equal the honest statement's bit for bit on every case
#   "sub_ulp"     moves u by at most one float32 ulp, 170 times below the criterion's floor of 1e-5: accepted
MUTATIONS = {"last_u": "reject", "u_endpoints": "reject", "half_bin_twice": "reject", "u_affine": "sub_ulp",
             "searchsorted_left": "same", "prev_cos_first": "same"}


def sampler_f32(rays_o, rays_d, z, sdf, m, inv_s, mutation=None):
    """oracle.neus_oracle.up_sample in float32 (bit for bit with mutation=None), with one deliberate mistake:
      last_u             u of the last sample replaced by its neighbour's (m >= 2)
      u_endpoints        u = linspace(0, 1, m): the half-step offsets at both ends forgotten
      half_bin_twice     the pdf of bin (n - 1) // 2 added twice to the cdf from there on (a chunk boundary counted twice in a scan)
      u_affine           u = start + step i for every i (torch.linspace counts down from `end` in its upper half)
      searchsorted_left  searchsorted(right=False)
      prev_cos_first     the first section's prev_cos taken as cos[0] instead of 0"""
    R, n = z.shape
    f32 = torch.float32
    radius = torch.linalg.norm(rays_o[:, None, :] + rays_d[:, None, :] * z[..., :, None], ord=2, dim=-1)
    inside = (radius[:, :-1] < 1.0) | (radius[:, 1:] < 1.0)
    prev_sdf, next_sdf, prev_z, next_z = sdf[:, :-1], sdf[:, 1:], z[:, :-1], z[:, 1:]
    mid = (prev_sdf + next_sdf) * 0.5
    cos = (next_sdf - prev_sdf) / (next_z - prev_z + 1e-5)
    first = cos[:, :1] if mutation == "prev_cos_first" else torch.zeros(R, 1, dtype=f32)
    cos = torch.minimum(torch.cat([first, cos[:, :-1]], -1), cos).clip(-1e3, 0.0) * inside
    dist = next_z - prev_z
    pc = torch.sigmoid((mid - cos * dist * 0.5) * inv_s)
    nc = torch.sigmoid((mid + cos * dist * 0.5) * inv_s)
    alpha = (pc - nc + 1e-5) / (pc + 1e-5)
    w = alpha * torch.cumprod(torch.cat([torch.ones(R, 1, dtype=f32), 1.0 - alpha + 1e-7], -1), -1)[:, :-1]
    w = w + 1e-5
    pdf = w / torch.sum(w, -1, keepdim=True)
    cdf = torch.cat([torch.zeros(R, 1, dtype=f32), torch.cumsum(pdf, -1)], -1)
    cdf, u = apply_mutation(cdf, pdf, u_values(m), mutation)
    u = u[None, :].expand(R, m).contiguous()
    return invert_cdf(cdf, z, u, right=mutation != "searchsorted_left")


def apply_mutation(cdf, pdf, u, mutation):
    """the mistakes of `sampler_f32` that act on the cdf [R, n] or on u [m], in the dtype of the arguments"""
    n, m = cdf.shape[1], u.shape[0]
    if mutation == "half_bin_twice":
        k = (n - 1) // 2
        cdf = cdf.clone()
        cdf[:, k + 1:] += pdf[:, k:k + 1]
    if mutation == "last_u" and m >= 2:
        u = u.clone()
        u[-1] = u[-2]
    elif mutation == "u_endpoints":
        u = torch.linspace(0.0, 1.0, steps=m, dtype=u.dtype)
    elif mutation == "u_affine":
        u = u_affine(m).to(u.dtype)
    return cdf, u


def mutation_displacement(cdf, z, m, mutation):
    """How far the mistake moves a sample in CDF space, from float64 alone: the float64 cdf (and u) with the mistake, inverted in
    float64, rounded to float32 and measured against the cdf without it.  [R, m].  A case in which some sample moves by more than
    twice its ray's tol_r is one the criterion has to reject; where nothing moves (one sample and no neighbour, a ray whose samples
    all fall into one zero-width bin, a doubled bin behind the last sample) the sampler is not wrong on those inputs."""
    R = z.shape[0]
    pdf = cdf[:, 1:] - cdf[:, :-1]
    cdf_m, u = apply_mutation(cdf, pdf, u_values(m).double(), mutation)
    zn = invert_cdf(cdf_m, z.double(), u[None, :].expand(R, m).contiguous()).float()
    return cdf_residual(cdf, z, zn, m)["residual"]


def u_affine(m):
    start, end = torch.tensor(0.5 / m, dtype=torch.float32), torch.tensor(1.0 - 0.5 / m, dtype=torch.float32)
    step = (end - start) / max(m - 1, 1)
    return start + step * torch.arange(m, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------------------------------
# compositing: inputs
# ------------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / v.norm(dim=-1, keepdim=True)


def composite_pn(c):
    """|p| at the section mid-points in float64 from the float32 inputs (what decides `inside` and the eikonal count)"""
    z = c["z"].double()
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], c["sample_dist"])], -1)
    mid = z + dists * 0.5
    return (c["rays_o"].double()[:, None, :] + c["rays_d"].double()[:, None, :] * mid[..., None]).norm(dim=-1)


def composite_case(kind, R, S, seed):
    """float32 inputs of avc_composite_fwd / _bwd: dict(sdf [R,S], normal [R,S,3], rgb [R,S,6], z [R,S], rays_o, rays_d [R,3],
    inv_s [1], sample_dist) and the upstream gradients d_color, d_extra [R,3], d_w [R,S], d_n_up [R,S,3], d_wsum [R], d_nsum [R,3].
      benign       as test_composite_forward_backward_fp32
      thresholds   rays from near the centre whose mid-points run from |p| = 0.55 to 1.65; every mid-point is at least 1e-4 away from
                   the radii 1.0 and 1.2
      branches     normals facing and opposing the ray: c = d . n spread over [-1.8, 1.8], at least 0.01 from the kinks at 0 and 1
      saturated    inv_s = 1e6, 0.2 <= |sdf| <= 1 with random signs, gaps <= 0.2 (|e - sdf| <= 0.1): every sigmoid is 0 or 1 in float32
      zero_normal  benign rays from near the centre; sample 0 of every ray lies inside |p| < 1.2 and has n = 0 exactly
    Every family is redrawn until no mid-point is within 1e-4 of the radii 1.0 and 1.2 and (saturated apart) no a_raw within 5e-6 of
    the kink of its clip at 0: on either the float32 kernel and the float64 statement may take different branches."""
    assert kind in CO_FAMILIES
    for attempt in range(200):
        g = torch.Generator().manual_seed(seed + 7907 * attempt)
        z = torch.sort(torch.rand(R, S, generator=g) * 2 + 0.5, dim=-1)[0]
        sdf = torch.randn(R, S, generator=g) * 0.05
        n = _unit(torch.randn(R, S, 3, generator=g)) * (1 + 0.2 * torch.randn(R, S, 1, generator=g))
        rgb = torch.rand(R, S, 6, generator=g)
        ro = torch.randn(R, 3, generator=g) * 0.3
        rd = _unit(torch.randn(R, 3, generator=g))
        inv_s = torch.tensor([40.0])
        if kind == "thresholds":
            ro = torch.randn(R, 3, generator=g) * 0.02
            z = torch.sort(torch.rand(R, S, generator=g) * 1.1 + 0.55, dim=-1)[0]
        elif kind == "branches":
            c = torch.rand(R, S, 1, generator=g) * 3.6 - 1.8
            c = torch.where((c.abs() < 0.01) | ((c - 1).abs() < 0.01), c + 0.05, c)
            p = torch.randn(R, S, 3, generator=g)
            p = p - (p * rd[:, None, :]).sum(-1, keepdim=True) * rd[:, None, :]
            n = c * rd[:, None, :] + 0.3 * p
        elif kind == "saturated":
            inv_s = torch.tensor([1e6])
            span = min(2.0, 0.1 * S)
            z = 0.5 + span * (torch.arange(S)[None, :] + torch.rand(R, S, generator=g)) / S
            sdf = (0.2 + 0.8 * torch.rand(R, S, generator=g)) * (torch.randint(0, 2, (R, S), generator=g) * 2 - 1)
            n = _unit(torch.randn(R, S, 3, generator=g))
        elif kind == "zero_normal":
            ro = torch.randn(R, 3, generator=g) * 0.05
            z[:, 0] = 0.3 + 0.2 * torch.rand(R, generator=g)
            if S > 1:
                z[:, 1] = torch.minimum(z[:, 1], z[:, 0] + 0.3)      # keeps sample 0's mid-point inside 1.2
            n[:, 0, :] = 0.0
        c = dict(kind=kind, sdf=sdf, normal=n, rgb=rgb, z=z, rays_o=ro, rays_d=rd, inv_s=inv_s, sample_dist=SAMPLE_DIST)
        c.update(d_color=torch.randn(R, 3, generator=g), d_extra=torch.randn(R, 3, generator=g), d_w=torch.randn(R, S, generator=g),
                 d_n_up=torch.randn(R, S, 3, generator=g) * 0.1, d_wsum=torch.randn(R, generator=g),
                 d_nsum=torch.randn(R, 3, generator=g) * 0.1, bg3=torch.rand(3, generator=g), bg_ray=torch.rand(R, generator=g))
        c = {k: (v.float().contiguous() if torch.is_tensor(v) else v) for k, v in c.items()}
        if composite_margin(c) >= 1e-4 and (kind == "saturated" or composite_clip_margin(c) >= 5e-6):
            return c
    raise AssertionError("no draw of %s R=%d S=%d keeps its mid-points off the radii and its alphas off the clip" % (kind, R, S))


def composite_margin(c):
    """the smallest distance of a mid-point's |p| from the radii 1.0 and 1.2"""
    pn = composite_pn(c)
    return float(torch.minimum((pn - 1.0).abs(), (pn - 1.2).abs()).min())


def composite_clip_margin(c):
    """the smallest |a_raw| over the three cos_anneal values of the table: alpha = clip(a_raw, 0, 1) has its lower kink there (a_raw
    = 1 - Q / (P + 1e-5) reaches the upper one only at Q = 0), and a sample within float32 rounding of it takes either gradient"""
    sdf, n, z, rd = c["sdf"].double(), c["normal"].double(), c["z"].double(), c["rays_d"].double()
    dists = torch.cat([z[:, 1:] - z[:, :-1], torch.full_like(z[:, :1], c["sample_dist"])], -1)
    cs = (rd[:, None, :] * n).sum(-1)
    worst = float("inf")
    for car in CO_ANNEAL:
        ic = -(torch.relu(-cs * 0.5 + 0.5) * (1 - car) + torch.relu(-cs) * car)
        P = torch.sigmoid((sdf - ic * dists * 0.5) * c["inv_s"].double())
        Q = torch.sigmoid((sdf + ic * dists * 0.5) * c["inv_s"].double())
        worst = min(worst, float(((P - Q + 1e-5) / (P + 1e-5)).abs().min()))
    return worst


def composite_reference(c, bg_mode, cos_anneal, dtype=torch.float64, d_eik=0.7):
    """oracle.analytic's composite_forward / composite_backward on the case in `dtype`, with the gradients of the fused reductions
    (sum_i w_i, sum_i w_i n_i) folded in as test_composite_forward_backward_fp32 does.  -> (cf, cb, eik_scale float32 [1])"""
    from oracle import analytic as A
    T = lambda t: t.to(dtype)
    R, S = c["z"].shape
    bg = None if bg_mode == 0 else (c["bg3"].reshape(1, 3) if bg_mode == 1 else c["bg_ray"].reshape(R, 1))
    pn = composite_pn(c)
    cf = A.composite_forward(T(c["sdf"]), T(c["normal"]), T(c["rgb"]), T(c["z"]), T(c["rays_d"]), T(pn), T(c["inv_s"]),
                             c["sample_dist"], cos_anneal, None if bg is None else T(bg))
    d_w_tot = T(c["d_w"]) + T(c["d_wsum"])[:, None] + (T(c["normal"]) * T(c["d_nsum"])[:, None, :]).sum(-1)
    d_n_tot = T(c["d_n_up"]) + cf["w"][..., None] * T(c["d_nsum"])[:, None, :]
    bgb = None if bg is None else (T(bg) if bg_mode == 1 else T(bg).expand(R, 3))
    cb = A.composite_backward(cf, T(c["sdf"]), T(c["normal"]), T(c["rgb"]), T(c["rays_d"]), T(c["inv_s"]), cos_anneal, bgb,
                              T(c["d_color"]), T(c["d_extra"]), d_w_tot, d_n_tot, torch.tensor(d_eik, dtype=dtype))
    eik_scale = (torch.tensor(d_eik, dtype=torch.float64) / cf["eik_den"].double()).float().reshape(1)
    return cf, cb, eik_scale


def composite_autograd(c, bg_mode, car, d_eik=0.7):
    """d loss / d normal by torch.autograd through oracle.analytic.composite_forward in float64, loss = the upstream gradients of
    RR.composite_case against the outputs they belong to"""
    from oracle import analytic as A
    D = lambda k: c[k].double()
    R, S = c["z"].shape
    n = D("normal").clone().requires_grad_(True)
    bg = None if bg_mode == 0 else (D("bg3").reshape(1, 3) if bg_mode == 1 else D("bg_ray").reshape(R, 1))
    cf = A.composite_forward(D("sdf"), n, D("rgb"), D("z"), D("rays_d"), composite_pn(c), D("inv_s"), c["sample_dist"], car, bg)
    w = cf["w"]
    loss = (cf["color"] * D("d_color")).sum() + (cf["extra"] * D("d_extra")).sum() + (w * D("d_w")).sum() + (n * D("d_n_up")).sum() \
        + (w.sum(-1) * D("d_wsum")).sum() + ((w[..., None] * n).sum(1) * D("d_nsum")).sum() + d_eik * cf["eik"]
    return torch.autograd.grad(loss, n)[0]


def composite_seed(S, bg_mode, cos_anneal):
    return 1000 * S + 17 * bg_mode + int(10 * cos_anneal)


def composite_values(ref):
    """the compared outputs of a composite_reference(...) as one dict"""
    cf, cb = ref[0], ref[1]
    return dict(color=cf["color"], extra=cf["extra"], w=cf["w"], P=cf["P"], d_sdf=cb["d_sdf"], d_n=cb["d_n"], d_rgb6=cb["d_rgb6"],
                d_inv_s_ray=cb["d_inv_s_ray"])


# what is compared per family: the backward of `saturated` is checked for finiteness only (its gradients are 0 or cancel to rounding
# noise), and `zero_normal` is about d_normal: with c = 0 and cos_anneal = 1 its P = Q, where d_sdf is a difference of equal terms
CO_KEYS = {"saturated": ("color", "extra", "w", "P"), "zero_normal": ("color", "extra", "w", "P", "d_n", "d_rgb6")}
CO_ALL = ("color", "extra", "w", "P", "d_sdf", "d_n", "d_rgb6", "d_inv_s")


def composite_errors(got, ref, kind):
    """forward outputs: largest absolute error; d_sdf, d_n, d_rgb6: relative L2; d_inv_s: error of the sum over the rays relative to
    max(1, |sum|) -- the measures of test_composite_forward_backward_fp32.  `got` / `ref`: composite_reference tuples or value dicts"""
    got, ref = (composite_values(x) if isinstance(x, tuple) else x for x in (got, ref))
    out = {}
    for k in CO_KEYS.get(kind, CO_ALL):
        if k in ("color", "extra", "w", "P"):
            out[k] = float((got[k].double() - ref[k].double()).abs().max())
        elif k == "d_inv_s":
            a, b = float(got["d_inv_s_ray"].double().sum()), float(ref["d_inv_s_ray"].double().sum())
            out[k] = abs(a - b) / max(1.0, abs(b))
        else:
            out[k] = float((got[k].double() - ref[k].double()).norm() / (ref[k].double().norm() + 1e-30))
    return out


# The project's figures for pure-float32 compositing (tests/test_gpu_kernels.py), kept for S <= 128 ...
CO_TOL = dict(color=2e-5, extra=2e-5, w=2e-5, P=2e-5, d_sdf=1e-4, d_n=1e-4, d_rgb6=1e-5, d_inv_s=1e-3)
# ... and what oracle.analytic in float32 leaves against float64 on the cases of the GPU table with S > 128 (all families but
# `saturated`) and on `saturated` (every S): measured by test_float32_statement_error_behind_the_composite_tolerances, which keeps
# these figures honest; the GPU tests allow 4 x them.
CO_F32_ERR = {"S>128": dict(color=1.2e-6, extra=1.0e-6, w=7.5e-7, P=1.1e-7, d_sdf=7.0e-6, d_n=5.5e-7, d_rgb6=2.5e-6, d_inv_s=2.0e-7),
              "saturated": dict(color=1.2e-7, extra=1.5e-7, w=5.6e-8, P=0.0)}


def composite_tolerances(kind, S):
    if kind == "saturated":
        return {k: 4 * v for k, v in CO_F32_ERR["saturated"].items()}
    if S > 128:
        return {k: 4 * v for k, v in CO_F32_ERR["S>128"].items()}
    return dict(CO_TOL)
