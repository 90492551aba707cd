"""A numpy fp64 restatement of the texture bake (TEST INFRASTRUCTURE ONLY; csrc/avc_bake.h states the rules, csrc/avc_bake.hip and
avatarclip_amd/bake.py implement them): the atlas layout, the closest point of a triangle (Ericson 5.1.5) brute force over ALL triangles
with the stated operation order and tie rule, the bake, and the preview's bilinear fetch.  Written from the rules; numpy evaluates every
product and sum below as one rounded IEEE operation, which is what the kernel does under `fp contract(off)`."""
import math

import numpy as np


# ---------------------------------------------------------------------------------------------------------------- the atlas
def cells(F, size):
    G = math.isqrt((F + 1) // 2 - 1) + 1
    assert (G - 1) ** 2 < (F + 1) // 2 <= G * G
    return G, size // G


def corners_local(P, upper):
    """the three corners of a chart as local texel indices (a, b), a to the right, b UP"""
    return [(P - 2, P - 2), (3, P - 2), (P - 2, 3)] if upper else [(1, 1), (P - 3, 1), (1, P - 3)]


def layout(F, size):
    """(uv float32 [F,3,2], owner int32 [size,size], corner texels int [F,3,2] as (column, row from the top)), one triangle at a time"""
    G, P = cells(F, size)
    assert P >= 6
    owner = np.full((size, size), -1, np.int32)
    corner = np.zeros((F, 3, 2), np.int64)
    for f in range(F):
        c, upper = f // 2, f % 2 == 1
        col, row = c % G, c // G
        for a in range(P):
            for b in range(P):
                if (a + b >= P) if upper else (a + b <= P - 1):
                    assert owner[row * P + P - 1 - b, col * P + a] == -1
                    owner[row * P + P - 1 - b, col * P + a] = f
        for k, (a, b) in enumerate(corners_local(P, upper)):
            corner[f, k] = (col * P + a, row * P + P - 1 - b)
    uv = ((corner.astype(np.float64) + 0.5) / float(size)).astype(np.float32)
    return uv, owner, corner


def texel_barycentrics(i, j, F, size):
    """(triangle, (b0, b1, b2) fp64) of texel column i, row j, or None for a free one"""
    G, P = cells(F, size)
    col, row = i // P, j // P
    if col >= G or row >= G:
        return None
    a, b = i % P, P - 1 - j % P
    upper = a + b > P - 1
    f = 2 * (row * G + col) + int(upper)
    if f >= F:
        return None
    if upper:
        b1, b2 = np.float64(P - 2 - a) / np.float64(P - 5), np.float64(P - 2 - b) / np.float64(P - 5)
    else:
        b1, b2 = np.float64(a - 1) / np.float64(P - 4), np.float64(b - 1) / np.float64(P - 4)
    return f, ((np.float64(1.0) - b1) - b2, b1, b2)


# ---------------------------------------------------------------------------------------------------------------- the closest point
def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def degenerate(a, b, c):
    ab, ac = b - a, c - a
    n0 = ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1]
    n1 = ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2]
    n2 = ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]
    return (n0 == 0) & (n1 == 0) & (n2 == 0)


def closest_on_triangles(p, a, b, c):
    """p [..., 3] fp64 against a, b, c [..., 3] fp64 (broadcast) -> (bary [..., 3], d2 [...]): every triangle's closest point to p, the
    rules in order, the first that holds"""
    with np.errstate(all="ignore"):
        p, a, b, c = np.broadcast_arrays(p, a, b, c)
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        one, zero = np.ones_like(d1), np.zeros_like(d1)
        s_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        g = 1.0 / ((va + vb) + vc)
        s_f, w_f = vb * g, vc * g
        rules = [((d1 <= 0) & (d2 <= 0), (one, zero, zero)),
                 ((d3 >= 0) & (d4 <= d3), (zero, one, zero)),
                 ((vc <= 0) & (d1 >= 0) & (d3 <= 0), (1.0 - s_ab, s_ab, zero)),
                 ((d6 >= 0) & (d5 <= d6), (zero, zero, one)),
                 ((vb <= 0) & (d2 >= 0) & (d6 <= 0), (1.0 - w_ac, zero, w_ac)),
                 ((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), (zero, 1.0 - w_bc, w_bc)),
                 (np.ones(d1.shape, bool), ((1.0 - s_f) - w_f, s_f, w_f))]
        conds = [r[0] for r in rules]
        bary = np.stack([np.select(conds, [r[1][k] for r in rules]) for k in range(3)], -1)          # np.select: the first condition that holds
        q = (bary[..., 0:1] * a + bary[..., 1:2] * b) + bary[..., 2:3] * c
        e = p - q
        return bary, _dot(e, e)


def closest_on_mesh(points, vertices, triangles, return_all=False):
    """brute force: (tri int32 [Q], bary fp64 [Q,3], d2 fp64 [Q]); the smaller d2 wins, equal d2 the lower index (np.argmin's first);
    degenerate triangles are never candidates.  return_all: also the [Q,F] matrix of squared distances (inf for a degenerate one)."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    t = np.asarray(triangles).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    dead = degenerate(a, b, c)
    if dead.all():
        raise ValueError("every triangle is degenerate")
    pts = np.asarray(points, np.float64)
    tri, bary, d2 = np.zeros(len(pts), np.int32), np.zeros((len(pts), 3)), np.zeros(len(pts))
    every = np.zeros((len(pts), len(t))) if return_all else None
    step = max(1, (1 << 18) // len(t))                        # a block of queries against all triangles: [step, F] arrays
    for q0 in range(0, len(pts), step):
        bc, dd = closest_on_triangles(pts[q0:q0 + step, None, :], a[None], b[None], c[None])
        dd = np.where(dead[None] | np.isnan(dd), np.inf, dd)
        k = np.argmin(dd, axis=1)
        rows = np.arange(len(k))
        tri[q0:q0 + step], bary[q0:q0 + step], d2[q0:q0 + step] = k, bc[rows, k], dd[rows, k]
        if return_all:
            every[q0:q0 + step] = dd
    return (tri, bary, d2, every) if return_all else (tri, bary, d2)


# ---------------------------------------------------------------------------------------------------------------- the bake
def texel_points(simple_v, simple_t, size):
    """(texel (j, i) list [Q,2], owning triangle [Q], fp64 points [Q,3]) over the owned texels in row-major order"""
    sv = np.asarray(simple_v, np.float32).astype(np.float64)
    st = np.asarray(simple_t).reshape(-1, 3)
    where, own, pts = [], [], []
    for j in range(size):
        for i in range(size):
            tb = texel_barycentrics(i, j, len(st), size)
            if tb is None:
                continue
            f, (b0, b1, b2) = tb
            where.append((j, i))
            own.append(f)
            pts.append((b0 * sv[st[f, 0]] + b1 * sv[st[f, 1]]) + b2 * sv[st[f, 2]])
    return np.asarray(where), np.asarray(own), np.asarray(pts, np.float64)


def mix_colors(tri, bary, dense_t, colors):
    c = np.asarray(colors)[:, :3].astype(np.float64)
    t = np.asarray(dense_t).reshape(-1, 3)[tri]
    x = (bary[:, 0:1] * c[t[:, 0]] + bary[:, 1:2] * c[t[:, 1]]) + bary[:, 2:3] * c[t[:, 2]]
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def bake(simple_v, simple_t, dense_v, dense_t, colors, size):
    """(uv, image uint8 [size,size,3], the texel list, tri, bary) -- free texels 128"""
    uv, owner, _ = layout(len(np.asarray(simple_t).reshape(-1, 3)), size)
    where, own, pts = texel_points(simple_v, simple_t, size)
    assert np.array_equal(own, owner[where[:, 0], where[:, 1]]) and len(own) == int((owner >= 0).sum())
    tri, bary, _ = closest_on_mesh(pts, dense_v, dense_t)
    image = np.full((size, size, 3), 128, np.uint8)
    image[where[:, 0], where[:, 1]] = mix_colors(tri, bary, dense_t, colors)
    return uv, image, where, tri, bary


# ---------------------------------------------------------------------------------------------------------------- the bilinear fetch
def bilinear_taps(u, v, T):
    """the four texels (x0, x1, y0, y1 clamped to [0, T - 1]) and the fractions (fx, fy) of a fetch at (u, v), in float64"""
    x, y = u * T - 0.5, v * T - 0.5
    xf, yf = np.floor(x), np.floor(y)
    cl = lambda a: np.clip(a, 0, T - 1).astype(np.int64)
    return cl(xf), cl(xf + 1), cl(yf), cl(yf + 1), x - xf, y - yf


def bilinear(texels, u, v):
    """texels uint8 [T,T,3], u, v arrays -> float64 [..., 3]: top = c00 (1 - fx) + c10 fx, bottom likewise, top (1 - fy) + bottom fy"""
    tex = np.asarray(texels).astype(np.float64)
    x0, x1, y0, y1, fx, fy = bilinear_taps(np.asarray(u, np.float64), np.asarray(v, np.float64), tex.shape[0])
    fx, fy = fx[..., None], fy[..., None]
    top = tex[y0, x0] * (1.0 - fx) + tex[y0, x1] * fx
    bottom = tex[y1, x0] * (1.0 - fx) + tex[y1, x1] * fx
    return top * (1.0 - fy) + bottom * fy
