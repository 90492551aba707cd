"""CPU restatement of neural_renderer's rasteriser backward (TEST INFRASTRUCTURE ONLY): the approximate gradient of Kato, Ushiku and Harada,
"Neural 3D Mesh Renderer" (CVPR 2018) section 3.3, restated from the paper and the published kernel, in numpy float32 following the rules of
DESIGN.md section 8 operation by operation (csrc/avc_raster_grad.hip is tested against it).  Unpinned against neural_renderer itself.

  n = 2 S; I = the face-index map (y up, -1 = background); c = light[I] (0 on background); G(x, y) = grad_image[(n-1-y) div 2, x div 2] / 4.
  For every front-facing face, edge (a, b, o) and axis (0: u = x, w = y; 1: u = y, w = x), every integer scan line u0 the edge spans:
  crossing w_x, w_in = floor / ceil(w_x), w_out = w_in + dir; out run (if I(w_in) = f) from w_out to the border, Delta = (c(w) - c(w_in)) G(w);
  in run from w_in to the opposite side (pixels of f), Delta = (c(w) - c(w_out)) G(w); where Delta > 0 the w-components of a and b get
  -= Delta / d, d = the displacement that moves the edge through pixel w (in NDC, pushed away from zero by eps).

The walk is written once (`walk`), with Delta as a hook: `pseudo_grad` is the walk with the grey term above, tests/nr_texture_restatement.py
hands it the three-channel term of the textured body.  tests/golden/nr_walk.npz pins its sums (tests/test_texture_cpu.py).
"""
import numpy as np

f32 = np.float32


def pixel_coords(ndc, n):
    """P = 0.5 (ndc n + n - 1), as face_setup computes it"""
    nd = np.asarray(ndc, f32)
    return f32(0.5) * (nd[..., :2] * f32(n) + f32(n) - f32(1))


def is_back(tri):
    """the forward's back-face rule on a face's three NDC vertices [3, >=2]"""
    x0, y0, x1, y1, x2, y2 = tri[0, 0], tri[0, 1], tri[1, 0], tri[1, 1], tri[2, 0], tri[2, 1]
    return (y2 - y0) * (x1 - x0) < (y1 - y0) * (x2 - x0)


def signed_area(p):
    """twice the signed area of a face's pixel coordinates p [3,2]: the denominator of its barycentrics"""
    return p[2, 0] * (p[0, 1] - p[1, 1]) + p[0, 0] * (p[1, 1] - p[2, 1]) + p[1, 0] * (p[2, 1] - p[0, 1])


def face_weights(p, zs, xi, yi):
    """face_weights of csrc/avc_raster.h at pixels (xi, yi) (float32, any broadcastable shapes) for a face's pixel coordinates p [3,2] and
    vertex depths zs [3]: the clamped barycentrics [3,...], their sum (>= 1e-10) and the depth zp"""
    den = signed_area(p)
    with np.errstate(divide="ignore", invalid="ignore"):
        w0 = np.clip(((p[1, 1] - p[2, 1]) * xi + (p[2, 0] - p[1, 0]) * yi + (p[1, 0] * p[2, 1] - p[2, 0] * p[1, 1])) / den, 0, 1)
        w1 = np.clip(((p[2, 1] - p[0, 1]) * xi + (p[0, 0] - p[2, 0]) * yi + (p[2, 0] * p[0, 1] - p[0, 0] * p[2, 1])) / den, 0, 1)
        w2 = np.clip(((p[0, 1] - p[1, 1]) * xi + (p[1, 0] - p[0, 0]) * yi + (p[0, 0] * p[1, 1] - p[1, 0] * p[0, 1])) / den, 0, 1)
        ws = np.maximum(w0 + w1 + w2, f32(1e-10))
        zp = f32(1) / ((w0 / zs[0] + w1 / zs[1] + w2 / zs[2]) / ws)
    return np.stack([w0, w1, w2]).astype(f32), ws.astype(f32), zp.astype(f32)


def rasterize_index(ndc, faces, n, near=0.1, far=100.0):
    """the forward rasteriser (oracle/nr_oracle.rasterize) returning the face-index map [n, n], y up, -1 = background"""
    nd = np.asarray(ndc, f32)
    fidx = np.full((n, n), -1, np.int64)
    zbuf = np.full((n, n), np.inf, f32)
    nf = f32(n)
    near, far = f32(near), f32(far)
    for k, face in enumerate(np.asarray(faces)):
        t = nd[face]
        if is_back(t):
            continue
        xs, ys, zs = t[:, 0], t[:, 1], t[:, 2]
        p = f32(0.5) * (t[:, :2] * nf + nf - f32(1))
        if signed_area(p) == 0 or not np.isfinite(p).all():
            continue
        lo_x = max(int(np.floor(p[:, 0].min())) - 1, 0); hi_x = min(int(np.ceil(p[:, 0].max())) + 1, n - 1)
        lo_y = max(int(np.floor(p[:, 1].min())) - 1, 0); hi_y = min(int(np.ceil(p[:, 1].max())) + 1, n - 1)
        if lo_x > hi_x or lo_y > hi_y:
            continue
        xi = np.arange(lo_x, hi_x + 1, dtype=f32)[None, :]
        yi = np.arange(lo_y, hi_y + 1, dtype=f32)[:, None]
        xp = (f32(2) * xi + f32(1) - nf) / nf
        yp = (f32(2) * yi + f32(1) - nf) / nf
        out = ((yp - ys[0]) * (xs[1] - xs[0]) < (xp - xs[0]) * (ys[1] - ys[0])) | \
              ((yp - ys[1]) * (xs[2] - xs[1]) < (xp - xs[1]) * (ys[2] - ys[1])) | \
              ((yp - ys[2]) * (xs[0] - xs[2]) < (xp - xs[2]) * (ys[0] - ys[2]))
        _, _, zp = face_weights(p, zs, xi, yi)
        ok = (~out) & (zp > near) & (zp < far)
        sz = zbuf[lo_y:hi_y + 1, lo_x:hi_x + 1]
        si = fidx[lo_y:hi_y + 1, lo_x:hi_x + 1]
        win = ok & (zp < sz)
        sz[win] = zp[win]
        si[win] = k
    return fidx


def G_map(grad_image):
    """G at the super-sampled pixels, [n, n] y up: the 2 x 2 average's backward with the row flip undone"""
    g = np.asarray(grad_image, f32)[::-1]
    return np.repeat(np.repeat(g, 2, 0), 2, 1) * f32(0.25)


def pooled_image(fidx, light):
    """the forward's pooled grey image from the face-index map: light[I] (0 on background), row flip, 2 x 2 average"""
    lt = np.asarray(light, f32)
    c = np.where(fidx >= 0, lt[np.maximum(fidx, 0)], f32(0))[::-1]
    n = c.shape[0]
    S = n // 2
    c4 = c.reshape(S, 2, S, 2)
    return ((c4[:, 0, :, 0] + c4[:, 0, :, 1]) + c4[:, 1, :, 0] + c4[:, 1, :, 1]) / f32(4)


def _expand(starts, lengths):
    """(index of the run, position k in the run) for runs of the given lengths"""
    lengths = np.maximum(lengths, 0)
    rep = np.repeat(np.arange(len(lengths)), lengths)
    k = np.arange(rep.size) - np.repeat(np.cumsum(lengths) - lengths, lengths)
    return rep, k


def walk(ndc, faces, fidx, delta_fn, eps=1e-4, count=None, abs_sum=None):
    """the rules' scan-line walk with the colour term as a hook: delta_fn((rows, cols) of the run's pixels, (rows, cols) of their reference
    pixel: w_in for an out run, w_out for an in run) -> Delta float32.  -> grad_ndc [V, 3] (float64 sums of float32 terms; z = 0).
    count: optional dict, gets 'out' and 'in' = the number of run pixels visited.  abs_sum: optional float64 array [V, 3], gets the sum of
    |term| over the terms of every vertex component (a scale for the rounding of any order of summation)."""
    nd = np.asarray(ndc, f32)
    faces = np.asarray(faces)
    fidx = np.asarray(fidx)
    n = fidx.shape[0]
    nf, eps = f32(n), f32(eps)
    P = pixel_coords(nd, n)
    grad = np.zeros((nd.shape[0], 3), np.float64)
    visits = {"out": 0, "in": 0}
    for f, face in enumerate(faces):
        if is_back(nd[face]):
            continue
        p = P[face]
        if not np.isfinite(p).all():
            continue
        for e in range(3):
            a, b, o = e, (e + 1) % 3, (e + 2) % 3
            for axis in (0, 1):
                ui, wi_ = (0, 1) if axis == 0 else (1, 0)
                comp = 1 if axis == 0 else 0
                ua, wa, ub, wb, uo, wo = p[a, ui], p[a, wi_], p[b, ui], p[b, wi_], p[o, ui], p[o, wi_]
                dir_ = (-1 if ua < ub else 1) if axis == 0 else (1 if ua < ub else -1)
                lo = max(np.ceil(min(ua, ub)), f32(0))
                hi = min(max(ua, ub), f32(n - 1))
                if not (lo <= n - 1) or not (hi > -1):
                    continue
                u0 = np.arange(int(lo), int(hi) + 1)
                if u0.size == 0:
                    continue
                fu = u0.astype(f32)
                with np.errstate(divide="ignore", invalid="ignore"):
                    wx = (wb - wa) / (ub - ua) * (fu - ua) + wa
                    w_in = np.floor(wx) if dir_ > 0 else np.ceil(wx)
                    w_out = w_in + f32(dir_)
                    ok = (w_in >= 0) & (w_in < nf) & (w_out >= 0) & (w_out < nf)
                if not ok.any():
                    continue
                u0, fu, wx, w_in, w_out = u0[ok], fu[ok], wx[ok], w_in[ok], w_out[ok]
                i_in, i_out = w_in.astype(np.int64), w_out.astype(np.int64)
                at = (lambda u, w: (w, u)) if axis == 0 else (lambda u, w: (u, w))     # (row y, column x) of scan-line position w

                def update(r, w, delta):
                    dw = w.astype(f32) - wx[r]
                    fr = fu[r]
                    with np.errstate(divide="ignore", invalid="ignore"):
                        for vert, m, d in ((a, ub != fr, (ub - ua) / (ub - fr) * dw * f32(2) / nf),
                                           (b, ua != fr, (ub - ua) / (fr - ua) * dw * f32(2) / nf)):
                            d = np.where(d > 0, d + eps, d - eps).astype(f32)
                            term = (delta / d).astype(f32)
                            grad[face[vert], comp] -= term[m].astype(np.float64).sum()
                            if abs_sum is not None:
                                abs_sum[face[vert], comp] += np.abs(term[m]).astype(np.float64).sum()

                # out runs
                sel = np.nonzero(fidx[at(u0, i_in)] == f)[0]
                if sel.size:
                    lens = (n - i_out[sel]) if dir_ > 0 else (i_out[sel] + 1)
                    rr, k = _expand(sel, lens)
                    r = sel[rr]
                    w = i_out[r] + dir_ * k
                    delta = delta_fn(at(u0[r], w), at(u0[r], i_in[r]))
                    visits["out"] += w.size
                    pos = delta > 0
                    if pos.any():
                        update(r[pos], w[pos], delta[pos])
                # in runs
                with np.errstate(divide="ignore", invalid="ignore"):
                    two = (fu - ua) * (fu - uo) < 0
                    wx2 = np.where(two, (wo - wa) / (uo - ua) * (fu - ua) + wa, (wb - wo) / (ub - uo) * (fu - uo) + wo).astype(f32)
                    lim = np.ceil(wx2) if dir_ > 0 else np.floor(wx2)
                r_lo = np.maximum(np.fmin(w_in, lim), f32(0)).astype(np.int64)
                r_hi = np.minimum(np.fmax(w_in, lim), f32(n - 1)).astype(np.int64)
                rr, k = _expand(np.arange(u0.size), r_hi - r_lo + 1)
                w = r_lo[rr] + k
                visits["in"] += w.size
                mine = fidx[at(u0[rr], w)] == f
                rr, w = rr[mine], w[mine]
                delta = delta_fn(at(u0[rr], w), at(u0[rr], i_out[rr]))
                pos = delta > 0
                if pos.any():
                    update(rr[pos], w[pos], delta[pos])
    if count is not None:
        count.update(visits)
    return grad


def grey_delta(fidx, light, G):
    """the grey colour term as a hook for walk(): (c(w) - c(w_ref)) G(w), c = light[I] (0 on background)"""
    lt = np.asarray(light, f32)
    c_map = np.where(fidx >= 0, lt[np.maximum(fidx, 0)], f32(0))
    return lambda px, ref: (c_map[px] - c_map[ref]) * G[px]


def pseudo_grad(ndc, faces, light, fidx, G, eps=1e-4, count=None, abs_sum=None):
    """the rules on a super-sampled pixel gradient G [n, n] (y up) -> grad_ndc [V, 3]: the walk with the grey colour term"""
    fidx = np.asarray(fidx)
    return walk(ndc, faces, fidx, grey_delta(fidx, light, np.asarray(G, f32)), eps, count, abs_sum)


def light_grad(fidx, G, F):
    """grad_light[f] = sum of G over the pixels whose face index is f"""
    m = fidx >= 0
    return np.bincount(fidx[m], weights=np.asarray(G, np.float64)[m], minlength=F)


def backward(ndc, faces, light, fidx, grad_image, eps=1e-4, count=None, abs_sum=None):
    """grad_image [S, S] -> (grad_ndc [V, 3], grad_light [F])"""
    G = G_map(grad_image)
    return pseudo_grad(ndc, faces, light, fidx, G, eps, count, abs_sum), light_grad(np.asarray(fidx), G, len(faces))
