"""A numpy restatement of the preview renderer's rules WITH the frustum clipper (TEST INFRASTRUCTURE ONLY; csrc/avc_preview_clip.h states
the rules, csrc/avc_preview_clip.hip implements them).  Written from the rules, not from the kernel: one face at a time, the clipper in
Python floats (IEEE doubles, one correctly rounded operation each, no fused multiply-add), coverage and depth through
tests/preview_restatement.py's own project / orient / face_weights / resolve.  A face whose three corners are valid is handled exactly as
preview_restatement handles it; every other face with finite corners is clipped against near, far, left, right, bottom, top, snapped and
drawn as a fan under its ORIGINAL face index."""
import math

import numpy as np

from tests import preview_restatement as PR

EXTRA = 256                     # the side planes and the clamp of generated corners sit one raster pixel outside the guard band
MAX_POLY = 9
INT64_MAX = np.iinfo(np.int64).max


def camera_points(v, cam):
    """float64 [V,3]: the camera-space points exactly as the projection computes them"""
    v = np.asarray(v, np.float32).astype(np.float64)
    cam = np.asarray(cam, np.float32).astype(np.float64)
    d = v - cam[None, :3]
    with np.errstate(all="ignore"):
        return np.stack([(d[:, 0] * cam[3 + 3 * j] + d[:, 1] * cam[4 + 3 * j]) + d[:, 2] * cam[5 + 3 * j] for j in range(3)], 1)


def _distance(plane, u, e, near, far):
    s = e * u[2]
    if plane == 0:
        return u[2] - near
    if plane == 1:
        return far - u[2]
    if plane == 2:
        return s + u[0]
    if plane == 3:
        return s - u[0]
    if plane == 4:
        return s + u[1]
    return s - u[1]


def clip_polygon(corners, width, near, far, R):
    """corners: three (c_x, c_y, c_z) -> the clipped polygon, a list of ([c_x, c_y, c_z, b_0, b_1, b_2], corner) with corner = 0..2 for a
    vertex that is still an original corner and -1 for an intersection; [] when fewer than 3 vertices are left"""
    kp = 1.0 + (65536.0 + 256.0) / (128.0 * float(R))
    e = kp * width
    poly = [([float(c[0]), float(c[1]), float(c[2])] + [1.0 if k == i else 0.0 for k in range(3)], i) for i, c in enumerate(corners)]
    for plane in range(6):
        out = []
        m = len(poly)
        for i in range(m):
            (A, ta), (B, _) = poly[i], poly[(i + 1) % m]
            da, db = _distance(plane, A, e, near, far), _distance(plane, B, e, near, far)
            ina, inb = bool(da >= 0.0), bool(db >= 0.0)                     # NaN: outside
            if ina and len(out) < MAX_POLY:
                out.append((list(A), ta))
            if ina != inb and len(out) < MAX_POLY:
                (P, dp), (Q, dq) = ((A, da), (B, db)) if ina else ((B, db), (A, da))     # always from the inside end to the outside end
                t = dp / (dp - dq)
                u = [P[k] + t * (Q[k] - P[k]) for k in range(6)]
                if plane == 0:
                    u[2] = near
                if plane == 1:
                    u[2] = far
                out.append((u, -1))
        poly = out
        if len(poly) < 3:
            return []
    return poly


def snap(u, width, near, far, R):
    """(X, Y, Z, 1 / c_z as float32) of a generated corner: the projection's formulas, clamped instead of refused"""
    s = u[2] * width
    half = float(R) * 0.5
    lo, hi = -float(PR.GUARD + EXTRA), 256.0 * R + float(PR.GUARD + EXTRA)
    X = math.floor((u[0] / s + 1.0) * half * 256.0 + 0.5)
    Y = math.floor((1.0 - u[1] / s) * half * 256.0 + 0.5)
    Z = math.floor(((u[2] - near) * far) / (u[2] * (far - near)) * float(PR.ZMAX) + 0.5)
    return int(min(max(X, lo), hi)), int(min(max(Y, lo), hi)), int(min(max(Z, 0.0), float(PR.ZMAX))), np.float32(1.0 / u[2])


def clipped_face(f, tri, v32, cpts, X, Y, Z, iw, width, near, far, R):
    """None: the face never meets the clipper (untouched or dropped by its indices / a non-finite corner); else the fan's corners
    (Xl, Yl, Zl int64 [m], iwl float32 [m], bary float32 [m,3]), m = 0 when nothing is left"""
    idx = [int(i) for i in tri]
    if min(idx) < 0 or max(idx) >= len(X):
        return None
    if min(Z[i] for i in idx) >= 0:
        return None
    if not np.isfinite(v32[idx]).all():
        return None
    poly = clip_polygon([cpts[i] for i in idx], width, near, far, R)
    Xl, Yl, Zl, iwl, bary = [], [], [], [], []
    for u, corner in poly:
        if corner >= 0 and Z[idx[corner]] >= 0:
            i = idx[corner]
            x, y, z, w = int(X[i]), int(Y[i]), int(Z[i]), iw[i]
        else:
            x, y, z, w = snap(u, width, near, far, R)
        Xl.append(x), Yl.append(y), Zl.append(z), iwl.append(w), bary.append([np.float32(b) for b in u[3:]])
    return (np.asarray(Xl, np.int64), np.asarray(Yl, np.int64), np.asarray(Zl, np.int64), np.asarray(iwl, np.float32),
            np.asarray(bary, np.float32).reshape(-1, 3))


def _piece(Xa, Ya, Za, corners, f, R):
    """one triangle of snapped corners under face index f: (idx, xs, ys, w, cov, key) as preview_restatement.rasterize forms them, or None"""
    o = PR.orient(Xa, Ya, Za, corners)
    if o is None:
        return None
    idx, area2 = o
    fw = PR.face_weights(Xa, Ya, idx, R)
    if fw is None:
        return None
    xs, ys, w, cov = fw
    if not cov.any():
        return None
    assert area2 * PR.ZMAX < 1 << 63
    num = w[0] * int(Za[idx[0]]) + w[1] * int(Za[idx[1]]) + w[2] * int(Za[idx[2]])
    return idx, xs, ys, w, cov, (np.floor_divide(num, area2) << 32) | f


def _fan_keys(fan, f, R):
    """for each drawn sub-triangle j = (p_0, p_j+1, p_j+2) of a fan: (j, idx, xs, ys, w, cov, key)"""
    for j in range(len(fan[0]) - 2):
        piece = _piece(fan[0], fan[1], fan[2], (0, j + 1, j + 2), f, R)
        if piece is not None:
            yield (j,) + piece


def rasterize(v, cam, width, near, far, tris, R, order=None, clip=True):
    """(key [R,R] int64 (EMPTY: background), fans {face: its fan}, X, Y, Z, iw): preview_restatement.rasterize with the clipped faces'
    fans joining the same minimum"""
    width, near, far = (float(np.float32(x)) for x in (width, near, far))
    v32 = np.asarray(v, np.float32)
    tris = np.asarray(tris)
    with np.errstate(all="ignore"):
        X, Y, Z, iw = PR.project(v32, cam, width, near, far, R)
    cpts = camera_points(v32, cam)
    key = np.full((R, R), INT64_MAX, np.int64)
    fans = {}
    for f in (range(len(tris)) if order is None else order):
        fan = clipped_face(f, tris[f], v32, cpts, X, Y, Z, iw, width, near, far, R) if clip else None
        if fan is None:
            piece = _piece(X, Y, Z, tris[f], f, R)                            # untouched (or dropped): as preview_restatement.rasterize
            pieces = [] if piece is None else [(0,) + piece]
        else:
            fans[f] = fan
            pieces = _fan_keys(fan, f, R)
        for _, _, xs, ys, _, cov, k in pieces:
            sub = key[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
            sub[cov] = np.minimum(sub[cov], k[cov])
    return np.where(key == INT64_MAX, PR.EMPTY, key), fans, X, Y, Z, iw


def shade_raster(key, fans, X, Y, Z, iw, v, tris, colors, light, ambient, background, grey=200.0):
    """float64 [R,R,3]: preview_restatement.shade_raster for the untouched winners, the clipped winners by the fan rule: the lowest
    sub-triangle that covers the pixel at the winning depth, l_i = w_i iw_i, L_k = (l_0 b_0k + l_1 b_1k) + l_2 b_2k over the carried
    barycentrics, colour = ((L_0 c_0 + L_1 c_1) + L_2 c_2) / ((L_0 + L_1) + L_2) over the ORIGINAL corners, the original face's shade"""
    R = key.shape[0]
    ids = PR.face_ids(key)
    plain = np.where(np.isin(ids, list(fans)), PR.EMPTY, key) if fans else key
    out = PR.shade_raster(plain, X, Y, Z, iw, v, tris, colors, light, ambient, background, grey)
    v64 = np.asarray(v, np.float32).astype(np.float64)
    light = np.asarray(light, np.float32).astype(np.float64)
    for f, fan in fans.items():
        if not (ids == f).any():
            continue
        done = np.zeros((R, R), bool)
        i0, i1, i2 = (int(i) for i in tris[f])
        n = np.cross(v64[i1] - v64[i0], v64[i2] - v64[i0])
        nn = np.linalg.norm(n) * np.linalg.norm(light)
        s = float(np.float32(ambient))
        if nn > 0:
            s = s + (1.0 - s) * min(abs(float(n @ light)) / nn, 1.0)
        for j, idx, xs, ys, w, cov, k in _fan_keys(fan, f, R):
            sub_key, sub_done = key[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1], done[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
            take = cov & (sub_key == k) & ~sub_done
            if not take.any():
                continue
            sub_done |= take
            lam = [w[i][take].astype(np.float64) * float(fan[3][idx[i]]) for i in range(3)]
            L = [(lam[0] * float(fan[4][idx[0], c]) + lam[1] * float(fan[4][idx[1], c])) + lam[2] * float(fan[4][idx[2], c]) for c in range(3)]
            den = (L[0] + L[1]) + L[2]
            yy, xx = np.nonzero(take)
            for ch in range(3):
                col = float(grey) if colors is None else \
                    ((L[0] * float(colors[i0, ch]) + L[1] * float(colors[i1, ch])) + L[2] * float(colors[i2, ch])) / den
                out[yy + ys[0], xx + xs[0], ch] = col * s
        assert done[ids == f].all()
    return out


def render(v, tris, colors, cam, width, near, far, light, ambient, background, S, ss, grey=200.0, clip=True):
    """one frame: (image uint8 [S,S,3], face ids int32 [S*ss, S*ss]); clip=False is preview_restatement.render"""
    R = S * ss
    key, fans, X, Y, Z, iw = rasterize(v, cam, width, near, far, tris, R, clip=clip)
    img, _ = PR.resolve(shade_raster(key, fans, X, Y, Z, iw, v, np.asarray(tris), colors, light, ambient, background, grey), ss)
    return img, PR.face_ids(key)

