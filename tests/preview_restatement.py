"""A numpy restatement of the preview renderer's rules (TEST INFRASTRUCTURE ONLY; include/avc.h states the rules, csrc/avc_preview.hip
implements them): projection and snapping in float64 one rounded operation at a time, coverage and depth in int64 / Python integers with
the top-left fill rule, the (depth << 32 | face) key, perspective-correct colours and flat two-sided shading in float64.  Written from
the rules, not from the kernel; one frame at a time, one face at a time."""
import numpy as np

SUBPIXEL = 256
GUARD = 1 << 16
ZMAX = (1 << 24) - 1
MAX_RASTER = 2048
EMPTY = -1


def project(v, cam, width, near, far, R):
    """v [V,3] float32, cam [12] float32 (eye, x, y, z axis) -> X, Y, Z int64 [V] (Z = -1: invalid) and 1 / c_z as float32 [V]"""
    v = np.asarray(v, np.float32).astype(np.float64)
    cam = np.asarray(cam, np.float32).astype(np.float64)
    width, near, far = (float(np.float32(x)) for x in (width, near, far))
    d = v - cam[None, :3]
    c = [(d[:, 0] * cam[3 + 3 * j] + d[:, 1] * cam[4 + 3 * j]) + d[:, 2] * cam[5 + 3 * j] for j in range(3)]
    with np.errstate(all="ignore"):
        s = c[2] * width
        half = float(R) * 0.5
        X = np.floor((c[0] / s + 1.0) * half * 256.0 + 0.5)
        Y = np.floor((1.0 - c[1] / s) * half * 256.0 + 0.5)
        Z = np.floor(((c[2] - near) * far) / (c[2] * (far - near)) * float(ZMAX) + 0.5)
        hi = 256.0 * R + GUARD
        ok = (c[2] > near) & (c[2] <= far) & (X >= -GUARD) & (X <= hi) & (Y >= -GUARD) & (Y <= hi)
        iw = (1.0 / c[2]).astype(np.float32)
    Z = np.clip(Z, 0, ZMAX)
    X, Y, Z = (np.where(ok, a, 0).astype(np.int64) for a in (X, Y, Z))
    return X, Y, np.where(ok, Z, -1), iw


def orient(X, Y, Z, tri):
    """the oriented corner indices (i0, i1, i2) and area2 > 0, or None for a dropped face (invalid corner, zero area)"""
    i0, i1, i2 = (int(t) for t in tri)
    if min(i0, i1, i2) < 0 or max(i0, i1, i2) >= len(X) or min(Z[i0], Z[i1], Z[i2]) < 0:
        return None
    area2 = (int(X[i1]) - int(X[i0])) * (int(Y[i2]) - int(Y[i0])) - (int(Y[i1]) - int(Y[i0])) * (int(X[i2]) - int(X[i0]))
    if area2 == 0:
        return None
    if area2 < 0:
        i1, i2, area2 = i2, i1, -area2
    return (i0, i1, i2), area2


def _top_left(ax, ay, bx, by):
    return by < ay or (by == ay and bx > ax)


def face_weights(X, Y, idx, R):
    """(xs, ys, w [3, h, w] int64, covered [h, w]) over the pixels whose centres lie in the face's box (clamped to the raster); None when
    there is none.  Python-integer corner values, int64 arrays: |every product| < 2^39 (checked)."""
    x = [int(X[i]) for i in idx]
    y = [int(Y[i]) for i in idx]
    xa, xb = max(0, -((128 - min(x)) // SUBPIXEL)), min(R - 1, (max(x) - 128) // SUBPIXEL)       # ceil((lo - 128) / 256), floor((hi - 128) / 256)
    ya, yb = max(0, -((128 - min(y)) // SUBPIXEL)), min(R - 1, (max(y) - 128) // SUBPIXEL)
    if xb < xa or yb < ya:
        return None
    xs, ys = np.arange(xa, xb + 1, dtype=np.int64), np.arange(ya, yb + 1, dtype=np.int64)
    px, py = (SUBPIXEL * xs + 128)[None, :], (SUBPIXEL * ys + 128)[:, None]
    w, cov = [], np.ones((len(ys), len(xs)), bool)
    for a, b in ((1, 2), (2, 0), (0, 1)):
        dx, dy = x[b] - x[a], y[b] - y[a]
        assert abs(dx) < 1 << 20 and abs(dy) < 1 << 20
        e = dx * (py - y[a]) - dy * (px - x[a])
        assert int(np.abs(e).max()) < 1 << 40
        cov &= (e >= 0) if _top_left(x[a], y[a], x[b], y[b]) else (e > 0)
        w.append(e)
    return xs, ys, np.stack(w), cov


def rasterize(X, Y, Z, tris, R, order=None):
    """key [R,R] int64 = min over the faces covering the pixel of (depth << 32 | face), EMPTY where none does; `order`: the sequence in
    which the faces are visited (the result must not depend on it)"""
    assert 0 < R <= MAX_RASTER
    key = np.full((R, R), np.iinfo(np.int64).max, np.int64)
    for f in (range(len(tris)) if order is None else order):
        o = orient(X, Y, Z, tris[f])
        if o is None:
            continue
        idx, area2 = o
        fw = face_weights(X, Y, idx, R)
        if fw is None:
            continue
        xs, ys, w, cov = fw
        if not cov.any():
            continue
        assert area2 * ZMAX < 1 << 63
        num = w[0] * int(Z[idx[0]]) + w[1] * int(Z[idx[1]]) + w[2] * int(Z[idx[2]])
        depth = np.floor_divide(num, area2)                        # at covered pixels every w >= 0: 0 <= num <= area2 * ZMAX < 2^63
        k = (depth << 32) | f
        sub = key[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
        sub[cov] = np.minimum(sub[cov], k[cov])
    return np.where(key == np.iinfo(np.int64).max, EMPTY, key)


def face_ids(key):
    return np.where(key == EMPTY, -1, key & 0xFFFFFFFF).astype(np.int32)


def coverage_count(X, Y, Z, tris, R):
    """how many faces cover each pixel [R,R]"""
    n = np.zeros((R, R), np.int32)
    for f in range(len(tris)):
        o = orient(X, Y, Z, tris[f])
        fw = None if o is None else face_weights(X, Y, o[0], R)
        if fw is not None:
            xs, ys, _, cov = fw
            n[ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] += cov
    return n


def shade_raster(key, X, Y, Z, iw, v, tris, colors, light, ambient, background, grey=200.0):
    """float64 [R,R,3] in 0..255: the shaded colour of every raster pixel before the box average"""
    R = key.shape[0]
    v = np.asarray(v, np.float32).astype(np.float64)
    light = np.asarray(light, np.float32).astype(np.float64)
    out = np.empty((R, R, 3), np.float64)
    out[:] = np.asarray(background, np.float64)
    ids = face_ids(key)
    for f in np.unique(ids[ids >= 0]):
        idx, area2 = orient(X, Y, Z, tris[f])
        yy, xx = np.nonzero(ids == f)
        px, py = SUBPIXEL * xx + 128, SUBPIXEL * yy + 128
        x, y = [int(X[i]) for i in idx], [int(Y[i]) for i in idx]
        w = [((x[b] - x[a]) * (py - y[a]) - (y[b] - y[a]) * (px - x[a])).astype(np.float64) for a, b in ((1, 2), (2, 0), (0, 1))]
        lam = [w[k] * float(iw[idx[k]]) for k in range(3)]
        den = lam[0] + lam[1] + lam[2]
        n = np.cross(v[idx[1]] - v[idx[0]], v[idx[2]] - v[idx[0]])
        nn = np.linalg.norm(n) * np.linalg.norm(light)
        s = float(np.float32(ambient))
        if nn > 0:
            s = s + (1.0 - s) * min(abs(float(n @ light)) / nn, 1.0)
        for ch in range(3):
            col = float(grey) if colors is None else sum(lam[k] * float(colors[idx[k], ch]) for k in range(3)) / den
            out[yy, xx, ch] = col * s
    return out


def resolve(raster, ss):
    """[S*ss, S*ss, 3] float64 -> uint8 [S,S,3]: ss x ss box average, floor(x + 0.5), clamped; and the distance of every averaged value
    from the nearest rounding boundary (a value that close to k + 0.5 may round either way in float32)"""
    R = raster.shape[0]
    S = R // ss
    avg = raster.reshape(S, ss, S, ss, 3).mean(axis=(1, 3))
    return np.clip(np.floor(avg + 0.5), 0, 255).astype(np.uint8), avg


def render(v, tris, colors, cam, width, near, far, light, ambient, background, S, ss, grey=200.0):
    """one frame: (image uint8 [S,S,3], face ids int32 [S*ss, S*ss])"""
    R = S * ss
    X, Y, Z, iw = project(v, cam, width, near, far, R)
    key = rasterize(X, Y, Z, np.asarray(tris), R)
    img, _ = resolve(shade_raster(key, X, Y, Z, iw, v, np.asarray(tris), colors, light, ambient, background, grey), ss)
    return img, face_ids(key)
