"""Float64 restatement of the nine kernels of csrc/avc_glue.hip, their input families and the criteria they are judged by.

TEST INFRASTRUCTURE ONLY (CPU, torch / numpy).  tests/test_glue_restatement_cpu.py pins this module against tests/golden/glue.npz, the
product's torch statements (Runner.shade_and_scatter / assemble_loss, chess_background, Dataset, coarse_z_torch, clip_preprocess) and
torch.cosine_similarity, measures the figures below and shows that the criteria reject wrong kernels; tests/test_gpu_glue_exact.py
judges the kernels with it.  Written from the reference lines the kernels cite (main.py:387-534, dataset.py:252-293,331-342,
renderer.py:311-322); it shares no code with the kernels.

ARITHMETIC IN FLOAT64, DECISIONS IN FLOAT32.  Every product, sum and quotient is float64 on the float32 inputs.  Every decision -- a
threshold (`wsum < 0.5`, the clamps to [0, 1], isnan, the BCE clip ends, `e == 0`, the 1e-8 clamp of a norm), a tap index of the
bilinear resize, the nearest-neighbour source index, the side of torch.linspace's two-sided formula -- is taken on the float32 value
the kernel sees and is a method of `Statement`, so that a case never differs from the kernel by a branch and a wrong kernel is one
overridden method (the mutants of the CPU module).  No case has a decision on a COMPUTED quantity within rounding of its threshold
(`shade_margin`); the on-threshold cases put an input value, or a quantity that is exact in both precisions, on the threshold.

TOLERANCES.  `*_F32_ERR` hold what the float32 CPU statement of the same lines leaves against the float64 restatement per family
(measured by the CPU module, which keeps them honest); a kernel is allowed 4 x that: it may order its operations differently from
torch but has no reason to be worse than a few roundings more.  Copies and comparisons are bit-equal; sums of small-integer multiples
of 1/16 are exact in any order.
"""
import numpy as np
import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
RES = 224
BLOCK = 256                                    # pixels per block of avc_shade_loss_fwd
EPS7 = float(np.float32(1e-7))
CLIP_LO = np.float32(1e-3)
CLIP_HI = np.float32(1.0 - 1e-3)               # (= 1.f - 1e-3f in float32 as well: asserted by the CPU module)
ALLOW = 4.0

# ------------------------------------------------------------------------------------------------------------------------
# the tables of the GPU module
# ------------------------------------------------------------------------------------------------------------------------
SH_P = (1, 63, 64, 65, 255, 256, 257, 65536, 65537, 131073)
SH_P_BWD = (1, 64, 65, 257, 65537)             # below a wavefront, at its edge, past it, a second block, 257 blocks
SH_FAMILIES = ("general", "threshold", "exact")
SH_BG = ("image", "const0", "const1")
RS_SHAPES = ((1, 1), (2, 3), (3, 2), (7, 5), (97, 97), (223, 225), (224, 100), (100, 224), (224, 224), (300, 224), (449, 448), (1000, 37))
RS_B = (1, 3)
GR_GRIDS = ((1, 1), (1, 7), (7, 1), (5, 9), (56, 56), (64, 80))       # (Wn, Hn)
GR_SEL = ("none", "sorted", "perm", "one", "repeat")         # repeat: R = Wn Hn + 5 rays, some pixels twice
GR_PRIOR = ("none", "smaller", "equal", "larger", "odd")
CH_SHAPES = ((5, 3, 1), (5, 3, 9), (9, 5, 2), (64, 80, 5), (190, 190, 13), (224, 224, 300))
CH_SIGMA = (0.1, 0.7, 1.9)
CZ_R, CZ_N = (1, 255, 257), (1, 2, 63, 64, 65)
LT_B, LT_T = (1, 2, 3, 4), (1, 3, 77)
LT_FAMILIES = ("generic", "degenerate_rows", "text_mean_zero")
CAMERA = (256.0, 256.0, 0.5 * 256.0 / np.tan(0.5 * np.pi / 3))        # W, H, focal of the dataset's pinhole camera

# What the float32 CPU statement leaves against the float64 restatement, per family: measured by tests/test_glue_restatement_cpu.py,
# which asserts measured <= stored <= 2 x measured (+ half an ulp); stored = 1.3 x measured, and no less than 2^-24 = 6e-8: a float32
# statement that comes out below ONE rounding of the format does so by the luck of its values.  The GPU module allows ALLOW x these.
# images: absolute; sums: relative (every term is >= 0); partial: `partial_err`; gradients: `rel_err` with the scales of judge_shade_bwd.
SH_F32_ERR = dict(images=2.4e-7, sums=2.1e-7, bce_exact=2.8e-7, partial=2.9e-7, dextra=1.6e-7, dwsum=8.5e-8, dnsum=1.4e-6)
# (H, W) -> fwd: largest |F.interpolate + Normalize in float32 - restatement| (the float32 source coordinate: grows with the input
# size); onehot: the same for autograd's gradient of one output pixel; transpose: `transpose_gap` of F.interpolate and its autograd,
# the largest of six draws
RS_F32_ERR = {
    (1, 1): dict(fwd=6.5e-07, onehot=4.7e-07, transpose=2.4e-08),
    (2, 3): dict(fwd=7.6e-07, onehot=1.6e-07, transpose=2.0e-08),
    (3, 2): dict(fwd=8.6e-07, onehot=2.4e-07, transpose=1.2e-08),
    (7, 5): dict(fwd=1.2e-06, onehot=4.2e-07, transpose=5.1e-09),
    (97, 97): dict(fwd=3.8e-05, onehot=5.5e-06, transpose=4.1e-10),
    (223, 225): dict(fwd=8.5e-05, onehot=5.5e-05, transpose=4.2e-10),
    (224, 100): dict(fwd=2.2e-05, onehot=8.2e-06, transpose=2.8e-10),
    (100, 224): dict(fwd=2.2e-05, onehot=5.1e-06, transpose=3.5e-10),
    (224, 224): dict(fwd=3.0e-07, onehot=1.6e-07, transpose=2.6e-10),
    (300, 224): dict(fwd=8.6e-05, onehot=2.1e-05, transpose=3.3e-10),
    (449, 448): dict(fwd=1.6e-04, onehot=8.5e-05, transpose=3.4e-10),
    (1000, 37): dict(fwd=2.6e-04, onehot=1.3e-04, transpose=4.5e-10),
}
GR_F32_ERR = dict(rays_d=1.8e-7, near=6.3e-7, far=6.8e-7)        # absolute; |rays_d| = 1, near / far about 1 and 3
CH_F32_ERR = 2.3e-7                                             # absolute, values in [0.2, 0.8]
LT_F32_ERR = dict(loss=1.3e-7, out=6.3e-7, d_enc=1.5e-7, dd=6e-8)   # loss: relative; out: absolute (out[0] is the loss, about 4); d_enc, dd: rel_err


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (k if isinstance(k, int) else sum(ord(c) * (i + 1) for i, c in enumerate(str(k))))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def rel_err(got, ref, scale=None):
    """largest |got - ref| / (|ref| + scale): an element is held to its own size and to `scale`, the natural size of its row (a gradient
    that cancels to nothing is not held to the nothing).  scale None: the largest |ref| of the row; an element whose |ref| + scale is 0
    has to be 0 exactly"""
    got, ref = got.double(), ref.double()
    if ref.numel() == 0:
        return 0.0
    if not torch.isfinite(got).all():
        return float("inf")
    a = ref.abs()
    if scale is None:
        scale = a.reshape(a.shape[0], -1).max(-1)[0].reshape([-1] + [1] * (a.dim() - 1)) if a.dim() > 1 else a
    d = (got - ref).abs()
    return float(torch.where(d == 0, torch.zeros_like(d), d / (a + scale)).max())


def _hook_abs(e, sign):
    """|e| whose derivative is `sign` (a constant tensor of -1, 0, +1)"""
    return e * sign


class Statement:
    """the decisions of the nine kernels, each on the float32 value the kernel sees"""

    # --- shading and the loss terms (main.py:426-497)
    def is_background(self, ws32):                       # main.py:444
        return ws32 < 0.5

    def outside_unit(self, x32):                         # clamp(min=0, max=1): -> (below, above); the gradient passes elsewhere, ends included
        return x32 < 0, x32 > 1

    def outside_clip(self, ws32):                        # clip(1e-3, 1 - 1e-3): ends included as well
        return ws32 < CLIP_LO, ws32 > CLIP_HI

    def l1_sign(self, e32):                              # d |e| / d e, 0 at e == 0
        return torch.sign(e32)

    def summed_pixels(self, P):                          # the pixels whose terms reach sums[4]: all of them
        return slice(0, P)

    # --- bilinear resize to 224 (F.interpolate, align_corners=False)
    def taps(self, n_in, dtype=F64):
        """-> i0, i1 [224] (from the float32 source coordinate), w0, w1 [224] (`dtype` arithmetic)"""
        o = torch.arange(RES)
        s32 = np.float32(n_in) / np.float32(RES)
        src32 = torch.clamp(torch.tensor(s32) * (o.float() + 0.5) - 0.5, min=0.0)
        i0 = torch.clamp(src32.long(), max=n_in - 1)
        i1 = i0 + (i0 < n_in - 1).long()
        if dtype == F64:
            src = torch.clamp((n_in / RES) * (o.double() + 0.5) - 0.5, min=0.0)
        else:
            src = src32
        w1 = src - i0.to(dtype)
        return i0, i1, 1.0 - w1, w1

    def resize_matrix(self, n_in, dtype=F64):
        """A [224, n_in]: out = A in along one axis"""
        i0, i1, w0, w1 = self.taps(n_in, dtype)
        A = torch.zeros(RES, n_in, dtype=dtype)
        A[torch.arange(RES), i0] += w0
        A[torch.arange(RES), i1] += w1
        return A

    def resize_matrix_bwd(self, n_in, dtype=F64):
        """what the backward transposes: the same matrix"""
        return self.resize_matrix(n_in, dtype)

    # --- the head of a view (dataset.py:252-293, main.py:376-380)
    def linspace_side(self, n):                          # torch.linspace: start + i step below the middle, end - (n - 1 - i) step above
        return torch.arange(n) < n // 2

    def nearest_index(self, n_out, n_in):                # F.interpolate(mode='nearest'): floor(dst * (in / out)) in float32
        s32 = np.float32(n_in) / np.float32(n_out)
        return torch.clamp(torch.floor(torch.arange(n_out).float() * torch.tensor(s32)).long(), max=n_in - 1)

    # --- GaussianBlur's reflect padding
    def reflect(self, i, n):
        return torch.where(i < 0, -i, torch.where(i >= n, 2 * n - 2 - i, i))

    # --- cosine: x / max(|x|, 1e-8); the norm's derivative counts only where the clamp is inactive
    def clamp_norm(self, nr):
        """max(|x|, 1e-8) of a norm `nr` (float64, differentiable), decided on its float32 value"""
        return torch.where(nr.detach().float() > 1e-8, nr, torch.full_like(nr, 1e-8))


HONEST = Statement()


# ------------------------------------------------------------------------------------------------------------------------
# avc_shade_loss_fwd / _bwd
# ------------------------------------------------------------------------------------------------------------------------
def unit_light32(light_dir, ambience):
    """main.py:434-441 on the host: the light direction normalised like `rand_light_d / (norm + 1e-7)` in float32, + the ambience"""
    l = np.asarray(light_dir, np.float32)
    l = l / (np.sqrt((l * l).sum(dtype=np.float32)).astype(np.float32) + np.float32(1e-7))
    return torch.tensor([l[0], l[1], l[2], np.float32(ambience)], dtype=F32)


def axis_light(ambience=0.25):
    """unit light along +x with an ambience that is exact in float32: (n^ . l^) is exact for small-integer normals"""
    return torch.tensor([1.0, 0.0, 0.0, ambience], dtype=F32)


def shade_case(family, P, rop, seed=0):
    """float32 inputs of avc_shade_loss_fwd / _bwd.  rop: with ray_of_pixel (about half the pixels unowned, the ray order a
    permutation of the owned pixels) or without (ray p = pixel p).
      general    random values with every computed threshold quantity at least 1e-4 off its threshold
      threshold  rows cycle through the on-threshold constructions: wsum of 0.5, float32(1e-3), float32(1 - 1e-3) and values on either
                 side; extra of 0 and 1 on background rows (s' = 1); normals perpendicular, parallel and opposed to the axis-aligned
                 light, zero and NaN; color == true_rgb; mask 0 and 1
      exact      0 / 1 mask, color - true_rgb in multiples of 1/4: sums[0], [1], [3] are exact in any order"""
    assert family in SH_FAMILIES
    g = _gen("shade", family, P, int(rop), seed)
    if rop:
        owned = torch.rand(P, generator=g) < 0.5
        owned[-1] = True                                   # (the last pixel, alone in the last block at P = 65537, is somebody's)
        R = int(owned.sum())
        ray_of_pixel = torch.full((P,), -1, dtype=torch.int32)
        ray_of_pixel[owned] = torch.randperm(R, generator=g).to(torch.int32)
    else:
        R, ray_of_pixel = P, None
    pix_of_ray = torch.arange(P) if ray_of_pixel is None else torch.argsort(torch.where(ray_of_pixel < 0, 2 ** 30, ray_of_pixel.long()))[:R]
    color = torch.rand(R, 3, generator=g)
    extra = torch.rand(R, 3, generator=g) * 1.3 - 0.1
    wsum = torch.rand(R, generator=g) * 1.1 - 0.05
    nsum = torch.randn(R, 3, generator=g) * 0.5
    true_rgb = torch.rand(P, 3, generator=g)
    mask = (torch.rand(P, generator=g) < 0.6).float()
    bg = torch.rand(P, generator=g)
    light = torch.randn(3, generator=g)
    light = torch.cat([light / light.norm(), torch.tensor([0.13])]).float()
    if family == "general":
        for t in (0.5, float(CLIP_LO), float(CLIP_HI)):    # wsum off its three thresholds
            wsum = torch.where((wsum - t).abs() < 1e-3, wsum + 3e-3, wsum)
    elif family == "exact":
        true_rgb = torch.randint(0, 5, (P, 3), generator=g).float() / 4
        color = true_rgb[pix_of_ray] + torch.randint(-2, 3, (R, 3), generator=g).float() / 4
        mask[-1] = 1.0
        color[-1 if ray_of_pixel is None else int(ray_of_pixel[-1])] = true_rgb[-1] + 0.5
    elif family == "threshold":
        light = axis_light()
        i = torch.arange(R)
        wtab = torch.tensor([0.5, float(CLIP_LO), float(CLIP_HI), 0.25, 0.75, 0.0, 1.0, -0.05, 1.05, 0.4375], dtype=F32)
        wsum = wtab[i % 10]
        ntab = torch.tensor([[0, 3, 0], [2, 0, 0], [-3, 0, 0], [0, 0, 0], [float("nan"), 1, 0], [0, 1, -2], [1, 2, 2], [-1, 2, 0]], dtype=F32)
        nsum = ntab[i % 7] if R >= 7 else ntab[i % 8]      # (period 7 leaves the last row out: 7 and 10 are coprime)
        etab = i % 3                                        # extra: 0 / 1 / as drawn
        extra = torch.where((etab == 0)[:, None], torch.zeros_like(extra), torch.where((etab == 1)[:, None], torch.ones_like(extra), extra))
        same = (i % 4 == 0)
        color = torch.where(same[:, None], true_rgb[pix_of_ray], color)
    c = dict(family=family, P=P, R=R, color=color, extra=extra, wsum=wsum, nsum=nsum, true_rgb=true_rgb, mask=mask, ray_of_pixel=ray_of_pixel,
             bg=bg, light=light)
    c.update(dimg0=torch.randn(P, 3, generator=g), dimg1=torch.randn(P, 3, generator=g),
             gs=torch.tensor([0.75, 0.0, 0.5 / max(P, 1), 0.0]) if family != "general" else torch.cat([torch.rand(1, generator=g) + 0.5, torch.zeros(1), torch.rand(1, generator=g) / P, torch.zeros(1)]))
    c = {k: (v.float().contiguous() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in c.items()}
    if family == "general":                               # computed threshold quantities: nudge the rows that come near
        for attempt in range(8):
            bad = shade_margin(c, per_ray=True) < 1e-4
            if not bad.any():
                break
            c["nsum"] = torch.where(bad[:, None], c["nsum"] + 0.05, c["nsum"])
            c["extra"] = torch.where(bad[:, None], c["extra"] * 0.97 + 0.011, c["extra"])
        assert shade_margin(c) >= 1e-4
    return c


def shade_margin(c, per_ray=False):
    """the smallest distance of a COMPUTED threshold quantity -- n^ . l^ and extra * s', both clamped to [0, 1] -- from 0 and 1, over
    the rays where it is not exactly on the threshold by construction (an exact 0 or 1 in float64 from the float32 inputs)"""
    N, l = c["nsum"].double(), c["light"].double()
    rho = N.norm(dim=-1)
    dot = ((N / (rho + EPS7)[:, None]) * l[:3]).sum(-1)
    d = torch.where(torch.isnan(dot), torch.ones_like(dot), dot.clamp(0, 1))
    s = l[3] + (1 - l[3]) * d
    sp = torch.where(c["wsum"] < 0.5, torch.ones_like(s), s)
    t = c["extra"].double() * sp[:, None]

    def dist(x):
        m = torch.minimum(x.abs(), (x - 1).abs())
        m = torch.where(torch.isnan(m), torch.ones_like(m), m)
        on = (x == 0) | (x == 1) | ((x.float() == 1) & (x > 1 - 1e-7))      # (2 / (2 + 1e-7) is 1 in float32 and inside [0, 1] in both)
        return torch.where(on, torch.ones_like(m), m)
    m = torch.minimum(dist(dot), dist(t).min(-1)[0])
    return m if per_ray else float(m.min()) if m.numel() else 1.0


def shade_loss(c, nsum=True, img0_is_extra=False, bg_mode="image", st=HONEST, dtype=F64, leaves=None):
    """main.py:426-497 on one case -> dict(images [2,P,3], sums [4], copies [2,P,3] bool: the elements that are copies of a float32
    input and have to come out bit-equal, terms [P,4]).  `leaves`: dict of color / extra / wsum / nsum tensors to differentiate."""
    P, rop = c["P"], c["ray_of_pixel"]
    get = lambda k: (leaves[k] if leaves is not None and k in leaves else c[k].to(dtype))
    owned = torch.ones(P, dtype=torch.bool) if rop is None else rop >= 0
    r = torch.arange(P) if rop is None else rop.long().clamp_min(0)
    color, E, ws = get("color")[r], get("extra")[r], get("wsum")[r]
    ws32 = c["wsum"][r]
    light = c["light"].to(dtype)
    if nsum:
        N = get("nsum")[r]
        nan_row = torch.isnan(c["nsum"][r]).any(-1)
        N = torch.where(nan_row[:, None], torch.ones_like(N), N)          # (keeps NaN out of the graph: the row's shading is the constant 1)
        rho = torch.norm(N, dim=-1, keepdim=True)
        dot = ((N / (rho + EPS7)) * light[:3]).sum(-1)
        dot32 = dot.detach().float()
        lo, hi = st.outside_unit(dot32)
        d = torch.where(nan_row, torch.ones_like(dot), torch.where(lo, torch.zeros_like(dot), torch.where(hi, torch.ones_like(dot), dot)))
        s = light[3] + (1 - light[3]) * d
        bgm = st.is_background(ws32)
        sp = torch.where(bgm, torch.ones_like(s), s)
        rsh = torch.where(bgm[:, None], E, s[:, None].expand(P, 3))
        t = E * sp[:, None]
        lo, hi = st.outside_unit(t.detach().float())
        tex = torch.where(lo, torch.zeros_like(t), torch.where(hi, torch.ones_like(t), t))
        rsh_copy = bgm[:, None].expand(P, 3)
    else:
        tex = rsh = E
        rsh_copy = torch.ones(P, 3, dtype=torch.bool)
    img0 = E if (img0_is_extra or not nsum) else tex
    bgv = (c["bg"].to(dtype) if bg_mode == "image" else torch.full((P,), 0.0 if bg_mode == "const0" else 1.0, dtype=dtype))[:, None].expand(P, 3)
    images = torch.stack([torch.where(owned[:, None], img0, bgv), torch.where(owned[:, None], rsh, bgv)])
    copies = torch.stack([~owned[:, None] | torch.full((P, 3), bool(img0_is_extra or not nsum)), ~owned[:, None] | rsh_copy])
    m = c["mask"].to(dtype)
    C = torch.where(owned[:, None], color, torch.zeros_like(color))
    wsp = torch.where(owned, ws, torch.zeros_like(ws))
    ws32 = torch.where(owned, ws32, torch.zeros_like(ws32))
    diff = C - c["true_rgb"].to(dtype)
    e = diff * m[:, None]
    l1 = _hook_abs(e, st.l1_sign(e.detach().float()).to(dtype)).sum(-1)
    lo, hi = st.outside_clip(ws32)
    x = torch.where(lo, torch.full_like(wsp, float(CLIP_LO)), torch.where(hi, torch.full_like(wsp, float(CLIP_HI)), wsp))
    bce = -(m * torch.log(x) + (1 - m) * torch.log(1 - x))
    terms = torch.stack([l1, m, bce, (diff * diff * m[:, None]).sum(-1)], -1)
    return dict(images=images, copies=copies, terms=terms, sums=terms[st.summed_pixels(P)].sum(0), owned=owned)


def shade_loss_grads(c, nsum=True, img0_is_extra=False, use0=True, use1=True, st=HONEST, dtype=F64):
    """torch.autograd of `shade_loss` under the upstream gradients of the case (dimg0 / dimg1 on the images, gs on the sums) ->
    dict(dcolor, dextra, dwsum, dnsum [R,...]) and `owns` [R] bool: the rays that own a pixel (the others keep what the buffer held)"""
    names = ("color", "extra", "wsum") + (("nsum",) if nsum else ())
    leaves = {}
    for k in names:
        v = c[k].to(dtype)
        leaves[k] = torch.where(torch.isnan(v), torch.zeros_like(v), v).requires_grad_(True)
    out = shade_loss(c, nsum, img0_is_extra, "image", st, dtype, leaves)
    loss = (out["sums"] * c["gs"].to(dtype)).sum()
    if use0:
        loss = loss + (out["images"][0] * c["dimg0"].to(dtype)).sum()
    if use1:
        loss = loss + (out["images"][1] * c["dimg1"].to(dtype)).sum()
    gr = torch.autograd.grad(loss, [leaves[k] for k in names], allow_unused=True)
    res = {"d" + k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(names, gr)}
    owns = torch.ones(c["R"], dtype=torch.bool)
    if c["ray_of_pixel"] is not None:
        owns = torch.zeros(c["R"], dtype=torch.bool)
        owns[c["ray_of_pixel"][c["ray_of_pixel"] >= 0].long()] = True
    res["owns"] = owns
    return res


def judge_shade_fwd(c, got_images, got_sums, ref, exact=None):
    """-> list of failures (empty: accepted) and the figures.  got_*: float32.  Copies bit-equal; every other image element within
    ALLOW x SH_F32_ERR['images']; sums[0], [1], [3] torch.equal in the exact family, else each sum within ALLOW x SH_F32_ERR['sums']
    of its float64 value, relative (every term is non-negative); the BCE sum likewise"""
    exact = c["family"] == "exact" if exact is None else exact
    fails, fig = [], {}
    ri = ref["images"].detach()
    cp = ref["copies"]
    if not torch.equal(got_images[cp], ri.float()[cp]):
        fails.append("a copied image element is not bit-equal")
    fig["images"] = float((got_images.double() - ri)[~cp].abs().max()) if (~cp).any() else 0.0
    if not torch.isfinite(got_images).all() or fig["images"] > ALLOW * SH_F32_ERR["images"]:
        fails.append("images off by %.3g" % fig["images"])
    rs = ref["sums"].detach()
    rel = ((got_sums.double() - rs).abs() / rs.abs().clamp_min(1e-30))
    rel = torch.where(got_sums.double() == rs, torch.zeros_like(rel), rel)
    fig["sums"] = float(rel.max())
    if exact:
        if not torch.equal(got_sums[[0, 1, 3]], rs.float()[[0, 1, 3]]):
            fails.append("exact sums differ: %s vs %s" % (got_sums[[0, 1, 3]].tolist(), rs[[0, 1, 3]].tolist()))
        if float(rel[2]) > ALLOW * SH_F32_ERR["bce_exact"]:
            fails.append("BCE sum off by %.3g relative" % float(rel[2]))
    elif fig["sums"] > ALLOW * SH_F32_ERR["sums"]:
        fails.append("sums off by %.3g relative" % fig["sums"])
    return fails, fig


def block_sums(terms, P):
    """[P, 4] -> [blocks, 4] in the dtype of `terms`"""
    blocks = (P + BLOCK - 1) // BLOCK
    return torch.cat([terms, torch.zeros(blocks * BLOCK - P, 4, dtype=terms.dtype)]).reshape(blocks, BLOCK, 4).sum(1)


def partial_err(partial, terms, P):
    """the per-block partial sums [blocks, 4] (block b = pixels 256 b .. 256 b + 255) against the float64 terms [P, 4]: largest
    |partial - sum| / (|sum| + the number of pixels in the block).  Relative to the sum for a full block; a block of one pixel is held
    to the absolute rounding of a term of order 1 (a BCE term -log(0.999) = 1e-3 carries the 6e-8 of its float32 argument, not of its
    own size): SH_F32_ERR['partial'] is the float32 statement's figure under this measure"""
    blocks = (P + BLOCK - 1) // BLOCK
    t = terms.detach().double()
    pad = torch.cat([t, torch.zeros(blocks * BLOCK - P, 4, dtype=F64)]).reshape(blocks, BLOCK, 4).sum(1)
    npix = torch.full((blocks, 1), float(BLOCK), dtype=F64)
    npix[-1] = P - (blocks - 1) * BLOCK
    d = (partial.double() - pad).abs()
    return float(torch.where(d == 0, torch.zeros_like(d), d / (pad.abs() + npix)).max())


def judge_shade_bwd(c, got, ref):
    """got / ref: dicts of dcolor, dextra, dwsum (, dnsum) [R,...]; only the rays that own a pixel are judged (ref['owns']).  dcolor
    bit-equal (gs[0] x a 0 / 1 mask x a sign is exact); the others finite and within ALLOW x SH_F32_ERR[name] under `rel_err` with the
    scales 1 (dextra: the upstream gradients are of order 1), gs[2] (dwsum) and 1 / (|N| + 1e-7) (dnsum: the size of d n^ / d N)"""
    fails, fig = [], {}
    o = ref["owns"]
    if not torch.equal(got["dcolor"][o], ref["dcolor"].float()[o]):
        fails.append("dcolor is not bit-equal")
    rho = c["nsum"].double().norm(dim=-1, keepdim=True)
    scale = dict(dextra=1.0, dwsum=float(c["gs"][2]), dnsum=torch.where(torch.isnan(rho), torch.ones_like(rho), 1.0 / (rho + EPS7))[o])
    for k in ("dextra", "dwsum", "dnsum"):
        if k in ref:
            fig[k] = rel_err(got[k][o], ref[k][o], scale[k])
            if not fig[k] <= ALLOW * SH_F32_ERR[k]:
                fails.append("%s off by %.3g" % (k, fig[k]))
    return fails, fig


# ------------------------------------------------------------------------------------------------------------------------
# avc_resize_norm_fwd / _bwd
# ------------------------------------------------------------------------------------------------------------------------
def resize_case(H, W, B):
    g = _gen("resize", H, W, B)
    return dict(x=torch.rand(B, H, W, 3, generator=g), w=torch.randn(B, 3, RES, RES, generator=g))


def _norm(dtype):
    return torch.tensor(CLIP_MEAN, dtype=F32).to(dtype), torch.tensor(CLIP_STD, dtype=F32).to(dtype)


def resize_norm(x, st=HONEST, dtype=F64):
    """[B,H,W,3] -> [B,3,224,224] = (bilinear resize - mean) / std (main.py:510-511); 224 x 224 is a copy before the normalisation"""
    B, H, W, _ = x.shape
    mean, std = _norm(dtype)
    v = x.to(dtype).permute(0, 3, 1, 2)
    if (H, W) != (RES, RES):
        v = st.resize_matrix(H, dtype) @ v @ st.resize_matrix(W, dtype).t()
    return (v - mean.view(1, 3, 1, 1)) / std.view(1, 3, 1, 1)


def resize_norm_bwd(dout, H, W, st=HONEST, dtype=F64):
    """the transpose: [B,3,224,224] -> [B,H,W,3]"""
    _, std = _norm(dtype)
    v = dout.to(dtype) / std.view(1, 3, 1, 1)
    if (H, W) != (RES, RES):
        v = st.resize_matrix_bwd(H, dtype).t() @ v @ st.resize_matrix_bwd(W, dtype)
    return v.permute(0, 2, 3, 1).contiguous()


ONEHOT_PIXELS = ((0, 0), (0, RES - 1), (RES - 1, 0), (RES - 1, RES - 1), (0, 100), (111, 57))     # four corners, an edge, an interior (oy, ox)


def onehot_dout():
    """[6, 3, 224, 224]: image k is 1 at ONEHOT_PIXELS[k] in channel k % 3"""
    d = torch.zeros(len(ONEHOT_PIXELS), 3, RES, RES)
    for k, (oy, ox) in enumerate(ONEHOT_PIXELS):
        d[k, k % 3, oy, ox] = 1.0
    return d


def transpose_gap(fx, f0, w, x, bw):
    """|<fwd(x) - fwd(0), w> - <x, bwd(w)>| / (|fwd(x) - fwd(0)| |w|), both products accumulated in float64 from float32 results"""
    lin = fx.double() - f0.double()
    a, b = (lin * w.double()).sum(), (x.double() * bw.double()).sum()
    return float((a - b).abs() / (lin.norm() * w.double().norm()).clamp_min(1e-300))


def judge_resize(H, W, fx, f0, bw, b1, case, st_ref=HONEST):
    """fx = fwd(x), f0 = fwd(0), bw = bwd(w), b1 = bwd(onehot_dout()) of a float32 implementation -> (failures, figures)"""
    tol = {k: ALLOW * v for k, v in RS_F32_ERR[(H, W)].items()}
    fails, fig = [], {}
    fig["fwd"] = float((fx.double() - resize_norm(case["x"], st_ref)).abs().max())
    if not fig["fwd"] <= tol["fwd"]:
        fails.append("forward off by %.3g" % fig["fwd"])
    fig["transpose"] = transpose_gap(fx, f0, case["w"], case["x"], bw)
    if not fig["transpose"] <= tol["transpose"]:
        fails.append("backward is not the forward's transpose: %.3g" % fig["transpose"])
    want = resize_norm_bwd(onehot_dout(), H, W, st_ref)
    fig["onehot"] = float((b1.double() - want).abs().max())
    if not fig["onehot"] <= tol["onehot"]:
        fails.append("one-hot gradient off the forward's weights by %.3g" % fig["onehot"])
    if not (b1[want == 0] == 0).all():
        fails.append("one-hot gradient reaches a pixel outside the stencil")
    untouched = resize_norm_bwd(torch.ones(1, 3, RES, RES), H, W, st_ref)[0] == 0
    if not (bw[:, untouched] == 0).all():
        fails.append("a pixel no output touches has a gradient")
    fig["untouched"] = int(untouched.sum()) // 3
    return fails, fig


# ------------------------------------------------------------------------------------------------------------------------
# avc_gen_rays
# ------------------------------------------------------------------------------------------------------------------------
def linspace32(end, n, side=None):
    """torch.linspace(0, end, n) in float32 as numpy float32 operations; side [n] bool: True = start + i step"""
    if n == 1:
        return np.zeros(1, np.float32)
    side = HONEST.linspace_side(n).numpy() if side is None else np.asarray(side)
    i = np.arange(n)
    step = np.float32(end) / np.float32(n - 1)
    return np.where(side, step * i.astype(np.float32), np.float32(end) - step * (n - 1 - i).astype(np.float32)).astype(np.float32)


def linspace64(end, n, st=HONEST):
    if n == 1:
        return torch.zeros(1, dtype=F64)
    i = torch.arange(n, dtype=F64)
    step = float(end) / (n - 1)
    return torch.where(st.linspace_side(n), step * i, float(end) - step * (n - 1 - i))


def rays_case(Wn, Hn, sel, prior):
    g = _gen("rays", Wn, Hn, sel, prior)
    # a camera 2 away from the centre looking at it, rolled about its axis: a rotation with no zero entry
    eye = torch.tensor([1.1, 0.7, 1.5], dtype=F64)
    eye = 2.0 * eye / eye.norm()
    zc = eye / eye.norm()
    up = torch.tensor([0.2, 1.0, -0.1], dtype=F64)
    xc = torch.linalg.cross(up, zc)
    xc = xc / xc.norm()
    yc = torch.linalg.cross(zc, xc)
    pose = torch.eye(4, dtype=F64)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = xc, yc, zc, eye
    n = Wn * Hn
    if sel == "none":
        idx = None
    elif sel == "sorted":
        idx = torch.sort(torch.randperm(n, generator=g)[:max(1, n // 2)])[0]
    elif sel == "perm":
        idx = torch.randperm(n, generator=g)
    elif sel == "one":
        idx = torch.randint(0, n, (1,), generator=g)
    else:
        idx = torch.randint(0, n, (n + 5,), generator=g)
    shape = dict(none=None, smaller=(max(1, Hn // 2), max(1, Wn // 2)), equal=(Hn, Wn), larger=(2 * Hn, 3 * Wn), odd=(Hn + 3, 2 * Wn + 1))[prior]
    pr = None
    if shape is not None:
        pr = torch.rand(shape[0], shape[1], 3, generator=g)
        pr = torch.where(torch.rand(shape[0], shape[1], 1, generator=g) < 0.4, torch.zeros_like(pr), pr)
    return dict(Wn=Wn, Hn=Hn, pose=pose.float().contiguous(), sel=idx, prior=pr, R=n if idx is None else int(idx.numel()))


def gen_rays(c, st=HONEST, dtype=F64, camera=CAMERA):
    """dataset.py:277-293 on the Wn x Hn grid (or its listed pixels), :331-342 and main.py:376-380 -> dict of rays_o, rays_d [R,3],
    near, far [R], and (with a prior) true_rgb [Hn Wn, 3], mask [Hn Wn]"""
    W, H, focal = camera
    Wn, Hn = c["Wn"], c["Hn"]
    p = torch.arange(Wn * Hn) if c["sel"] is None else c["sel"]
    iy, ix = p // Wn, p % Wn
    if dtype == F64:
        px, py = linspace64(W - 1, Wn, st)[ix], linspace64(H - 1, Hn, st)[iy]
        focal = float(np.float32(focal))
    else:
        px = torch.from_numpy(linspace32(W - 1, Wn, st.linspace_side(Wn).numpy()))[ix]
        py = torch.from_numpy(linspace32(H - 1, Hn, st.linspace_side(Hn).numpy()))[iy]
        focal = np.float32(focal)
    cam = torch.stack([(px - 0.5 * W) / focal, -(py - 0.5 * H) / focal, -torch.ones_like(px)], -1)
    v = cam / cam.norm(dim=-1, keepdim=True)
    pose = c["pose"].to(dtype)
    d = (v[:, None, :] * pose[:3, :3]).sum(-1)
    o = pose[:3, 3].expand(d.shape)
    a = (d * d).sum(-1)
    b = 2.0 * (o * d).sum(-1)
    mid = 0.5 * (-b) / a
    out = dict(rays_o=o, rays_d=d, near=torch.where(mid.float() - 1 < 0, torch.zeros_like(mid), mid - 1), far=mid + 1)
    if c["prior"] is not None:
        Hp, Wp = c["prior"].shape[:2]
        t = c["prior"][st.nearest_index(Hn, Hp)][:, st.nearest_index(Wn, Wp)].reshape(-1, 3)
        out.update(true_rgb=t, mask=(t[:, 0] != 0).float())
    return out


def dataset(device="cpu"):
    """the product's Dataset with the camera of the table and nothing loaded: its ray methods are the torch statement"""
    from avatarclip_amd.dataset import SMPL_Dataset
    ds = object.__new__(SMPL_Dataset)
    ds.W, ds.H, ds.focal, ds.device = int(CAMERA[0]), int(CAMERA[1]), CAMERA[2], torch.device(device)
    return ds


def dataset_rays(ds, c):
    """dataset.py:252-293 on the Wn x Hn grid as Dataset.gen_rays_silhouettes states it + near_far_from_sphere + main.py:376-380, on
    the dataset's device in float32: what Runner._view_head_torch runs"""
    device = ds.device
    tx = torch.linspace(0, ds.W - 1, c["Wn"], device=device)
    ty = torch.linspace(0, ds.H - 1, c["Hn"], device=device)
    px, py = torch.meshgrid(tx, ty, indexing="ij")
    o, v = ds._dirs(px.t(), py.t(), c["pose"].to(device))
    o, v = o.reshape(-1, 3), v.reshape(-1, 3)
    if c["sel"] is not None:
        o, v = o.index_select(0, c["sel"].to(device)), v.index_select(0, c["sel"].to(device))
    near, far = ds.near_far_from_sphere(o, v)
    out = dict(rays_o=o.contiguous(), rays_d=v.contiguous(), near=near.reshape(-1), far=far.reshape(-1))
    if c["prior"] is not None:
        t = F.interpolate(c["prior"].to(device).permute(2, 0, 1).unsqueeze(0), size=(c["Hn"], c["Wn"])).squeeze(0).permute(1, 2, 0).reshape(-1, 3)
        out.update(true_rgb=t.contiguous(), mask=(t != 0).float()[:, 0].contiguous())
    return out


def ulps(a, b):
    """largest distance of two float32 tensors in units in the last place (of the larger magnitude's binade)"""
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    ia, ib = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia), torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int((ia - ib).abs().max()) if a.numel() else 0


def judge_rays(c, got, ref):
    fails, fig = [], {}
    if not torch.equal(got["rays_o"], c["pose"][:3, 3].expand(c["R"], 3)):
        fails.append("rays_o is not the pose column")
    for k in ("true_rgb", "mask"):
        if k in ref and not torch.equal(got[k], ref[k]):
            fails.append("%s is not bit-equal" % k)
    for k in ("rays_d", "near", "far"):
        fig[k] = float((got[k].double() - ref[k].double()).abs().max())
        if not fig[k] <= ALLOW * GR_F32_ERR[k]:
            fails.append("%s off by %.3g" % (k, fig[k]))
    return fails, fig


# ------------------------------------------------------------------------------------------------------------------------
# avc_chess_background
# ------------------------------------------------------------------------------------------------------------------------
def blur_taps(k, sigma, dtype=np.float64):
    """torchvision's GaussianBlur kernel of k taps"""
    r = np.arange(k, dtype=dtype) - dtype((k - 1) / 2)
    w = np.exp(dtype(-0.5) * (r / dtype(sigma)) ** 2).astype(dtype)
    return (w / w.sum(dtype=dtype)).astype(dtype)


def chess(H, W, L, sigma, st=HONEST, taps=None):
    """main.py:398-405 in float64 -> [H, W]; taps = (kx[5], ky[9]) to blur with (default: the float64 Gaussian of `sigma`)"""
    kx, ky = (blur_taps(5, sigma), blur_taps(9, sigma)) if taps is None else taps
    y, x = torch.arange(H), torch.arange(W)
    out = torch.zeros(H, W, dtype=F64)
    for a in range(9):
        yy = st.reflect(y + a - 4, H)
        for b in range(5):
            xx = st.reflect(x + b - 2, W)
            board = torch.where(((yy[:, None] // L + xx[None, :] // L) % 2) == 0, torch.tensor(0.8, dtype=F64), torch.tensor(0.2, dtype=F64))
            out += float(ky[a]) * float(kx[b]) * board
    return out


# ------------------------------------------------------------------------------------------------------------------------
# avc_coarse_z
# ------------------------------------------------------------------------------------------------------------------------
def coarse_case(R, n):
    g = _gen("coarse", R, n)
    near = torch.rand(R, 1, generator=g) + 0.5
    return dict(near=near, far=near + 1.5 + torch.rand(R, 1, generator=g), jitter=torch.rand(R, 1, generator=g))


def coarse_z32(c, n, jitter, lin=None):
    """renderer.py:311-322 in float32, one rounding per torch op; lin: the linspace(0, 1, n) to use (default torch's)"""
    lin = torch.linspace(0.0, 1.0, n) if lin is None else lin
    z = c["near"] + (c["far"] - c["near"]) * lin[None, :]
    if jitter:
        z = z + (c["jitter"] - 0.5) * 2.0 / n
    return z


# ------------------------------------------------------------------------------------------------------------------------
# avc_loss_tail_fwd / _bwd
# ------------------------------------------------------------------------------------------------------------------------
TAIL_W = dict(igr=0.1, mask=0.3, clip=1.7, P=224.0 * 224.0, g=1.9)


def tail_case(family, B, T):
    """generic: random embeddings; degenerate_rows: image 0 is a zero row and image 1 (B >= 2) a row of norm 2e-9, below the 1e-8
    clamp but not zero; text_mean_zero: the text rows cancel in pairs, exactly and in the order they are added"""
    assert family in LT_FAMILIES
    g = _gen("tail", family, B, T)
    enc = torch.randn(B, 512, generator=g)
    text = F.normalize(torch.randn(T, 512, generator=g), dim=-1)
    if family == "degenerate_rows":
        enc[0] = 0.0
        if B >= 2:
            enc[1] = enc[1] * 1e-10
    if family == "text_mean_zero":
        text[1::2] = -text[0:T - 1:2]
        if T % 2:
            text[T - 1] = 0.0
    return dict(enc=enc.contiguous(), text=text.contiguous(), sums=torch.tensor([812.5, 30211.0, 9120.25, 77.0]), eik=torch.tensor(0.0371))


def loss_tail(c, st=HONEST, dtype=F64):
    """main.py:491-534 from the embeddings on, cos = <e / max(|e|, 1e-8), t / max(|t|, 1e-8)> -> dict(loss, out [8], d_enc [B,512],
    dd [8]) with the gradients of g x loss; c["P"]: the pixel count the BCE sum is divided by (default TAIL_W's)"""
    w = TAIL_W
    enc, sums, eik = (c[k].detach().to(dtype).clone().requires_grad_(True) for k in ("enc", "sums", "eik"))
    P = c.get("P", w["P"])
    B = enc.shape[0]

    def unit(x):
        nr = torch.norm(x, dim=-1, keepdim=True)
        return x / st.clamp_norm(nr)
    th = unit(c["text"].to(dtype).mean(0, keepdim=True))
    cos = (unit(enc) * th).sum(-1)
    colour, maskl = sums[0] / (sums[1] + 1e-5), sums[2] / P
    loss = colour + eik * w["igr"] + maskl * w["mask"]
    for b in range(B):
        loss = loss + (1.0 - cos[b]) * w["clip"]
    d_enc, d_sums, d_eik = torch.autograd.grad(loss * w["g"], [enc, sums, eik])
    out = torch.zeros(8, dtype=dtype)
    out[0], out[1], out[2] = loss.detach(), colour.detach(), maskl.detach()
    out[3:3 + B] = cos.detach()
    dd = torch.zeros(8, dtype=dtype)
    dd[0], dd[2], dd[4] = d_sums[0], d_sums[2], d_eik          # ([1], the mask count, and [3], the psnr's error, are constants of the iteration)
    return dict(loss=loss.detach(), out=out, d_enc=d_enc, dd=dd, cos=cos.detach())


def judge_tail(got, ref):
    fails, fig = [], {}
    fig["loss"] = abs(float(got["loss"]) - float(ref["loss"])) / abs(float(ref["loss"]))
    fig["out"] = float((got["out"].double() - ref["out"].double()).abs().max())
    fig["d_enc"] = rel_err(got["d_enc"], ref["d_enc"])
    fig["dd"] = rel_err(got["dd"][:5], ref["dd"][:5])
    for k, v in fig.items():
        if not v <= ALLOW * LT_F32_ERR[k]:
            fails.append("%s off by %.3g" % (k, v))
    B = ref["d_enc"].shape[0]
    if not (got["out"][3 + B:] == 0).all() or not (got["dd"][5:] == 0).all() or float(got["dd"][1]) != 0 or float(got["dd"][3]) != 0:
        fails.append("an unused slot of out[] / dd[] is not zero")
    return fails, fig
