"""Seeded inputs of the texture bake's tests (TEST INFRASTRUCTURE ONLY), shared by tests/test_bake_cpu.py (which checks
with the restatement alone that they hold what the GPU tests rely on) and tests/test_gpu_bake.py: a numpy-built UV sphere, its
spoilt variant for the closest-point routine (a huge triangle, a zero-area one, a duplicate), the query set, and the bake case (a finer sphere
simplified at divisor 8, baked at size 128) with its restated reference, recorded in tests/golden/bake_sphere.npz."""
import functools
import os

import numpy as np

from tests import bake_restatement as BR
from tests import rig_standins as RS

NU, NV = 32, 16                       # segments around and from pole to pole: 2 + 15 * 32 vertices, 960 triangles
BAKE_SIZE, BAKE_DIVISOR = 128, 8
PALETTE = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [255, 0, 255], [0, 255, 255], [0, 0, 0], [255, 255, 255]], np.uint8)
AMBIGUOUS = 1e-9                      # of the squared bounding-box diagonal: closer than this, two dense triangles tie for a texel


def uv_sphere(nu=NU, nv=NV):
    """(vertices float32 [2 + (nv - 1) nu, 3], triangles int32 [2 nu (nv - 1), 3]) of the unit sphere, outward winding"""
    v = [(0.0, 1.0, 0.0)]
    for j in range(1, nv):
        th = np.pi * j / nv
        for i in range(nu):
            ph = 2.0 * np.pi * i / nu
            v.append((np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)))
    v.append((0.0, -1.0, 0.0))
    ring = lambda j, i: 1 + (j - 1) * nu + i % nu
    t = []
    for i in range(nu):
        t.append((0, ring(1, i + 1), ring(1, i)))
    for j in range(1, nv - 1):
        for i in range(nu):
            a, b, c, d = ring(j, i), ring(j, i + 1), ring(j + 1, i + 1), ring(j + 1, i)
            t += [(a, b, c), (a, c, d)]
    for i in range(nu):
        t.append((len(v) - 1, ring(nv - 1, i), ring(nv - 1, i + 1)))
    return np.asarray(v, np.float32), np.asarray(t, np.int32)


def smooth_colors(v):
    """uint8 [N,4]: a colour that varies over the sphere, so that a wrong triangle or wrong barycentrics show"""
    c = np.clip(np.rint((np.asarray(v, np.float64) * 0.5 + 0.5) * 255.0), 0, 255)
    return np.concatenate([c, np.full((len(c), 1), 255.0)], 1).astype(np.uint8)


HUGE, FLAT, COPIED = 100, 500, 333       # the triangles replaced by a huge one and by a zero-area one; the one appended again at the end


def spoilt_sphere(huge=True):
    """the sphere with triangle HUGE replaced by one that spans the bounding box (three added vertices; r_max becomes larger than the
    sphere, so no query can stop early: it must only cost time), triangle FLAT by a zero-area one (two distinct corners and their exact
    midpoint), and triangle COPIED appended once more as the last triangle (every query nearest to it ties: the lower index wins)"""
    v, t = uv_sphere()
    v = np.concatenate([v, np.array([[-1, -1, -1], [1, -1, 1], [-1, 1, 1]], np.float32)])
    t = t.copy()
    if huge:
        t[HUGE] = (len(v) - 3, len(v) - 2, len(v) - 1)
    a, b = v[t[FLAT, 0]].astype(np.float64), v[t[FLAT, 1]].astype(np.float64)
    a, b = np.round(a * 256) / 256, np.round(b * 256) / 256            # (few mantissa bits: the midpoint and the cross product are exact)
    v = np.concatenate([v, np.stack([a, b, (a + b) * 0.5]).astype(np.float32)])
    t[FLAT] = (len(v) - 3, len(v) - 2, len(v) - 1)
    t = np.concatenate([t, t[COPIED:COPIED + 1]])
    return v, t


def queries(v, t, seed=0):
    """float64 [1003, 3] (no multiple of 64): 400 points on the surface, 400 inside, 202 about 10 bounding-box diameters outside the
    grid, one exactly at a shared vertex"""
    rs = np.random.RandomState(seed)
    vv = np.asarray(v, np.float32).astype(np.float64)
    f = np.concatenate([rs.randint(0, len(t), 396), [COPIED] * 4])
    w = rs.dirichlet((1.0, 1.0, 1.0), len(f))
    surface = (w[:, 0:1] * vv[t[f, 0]] + w[:, 1:2] * vv[t[f, 1]]) + w[:, 2:3] * vv[t[f, 2]]
    inside = rs.standard_normal((400, 3))
    inside = inside / np.linalg.norm(inside, axis=1, keepdims=True) * (0.9 * rs.uniform(0, 1, (400, 1)) ** (1.0 / 3.0))
    diam = float(np.linalg.norm(vv.max(0) - vv.min(0)))
    outside = rs.standard_normal((202, 3))
    outside = outside / np.linalg.norm(outside, axis=1, keepdims=True) * (10.0 * diam * rs.uniform(0.9, 1.1, (202, 1)))
    q = np.concatenate([surface, inside, outside, vv[t[700, 1]][None]])
    assert q.shape == (1003, 3)
    return np.ascontiguousarray(q)


# ---------------------------------------------------------------------------------------------------------------- the bake case
# The end-to-end case: a 64 x 32 sphere (3 968 triangles) simplified at divisor 8 (576 triangles: 17 x 17 cells of 7 texels at size 128).
# At that chart size three texels in five are gutter, extrapolated up to a third of a leg beyond the simplified triangle, i.e. OUTSIDE the
# dense polyhedron, where the closest point lies on a dense edge or vertex and the triangles around it tie.  With a random palette colour
# per dense triangle 18 % of the texels are ambiguous at 64 x 32 (27 % at 32 x 16, 14 % at 96 x 48); painting the eight octants of a
# tilted frame -- still one flat colour per dense triangle, all eight colours used -- leaves the ties that matter only along the three
# great circles between the patches, and the finer sphere narrows the wedge over each boundary edge: 4.5 % at 32 x 16, 1.5 % at 64 x 32.
# The brute-force restatement of this case takes some 20 s, so its results are RECORDED in tests/golden/bake_sphere.npz
# (scripts/gen_golden_bake.py) together with the sphere's float32 vertices (sin and cos may differ in the last bit between C libraries;
# everything after them is IEEE arithmetic); tests/test_bake_cpu.py recomputes the record, tests/test_gpu_bake.py reads it.
BAKE_NU, BAKE_NV = 64, 32
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bake_sphere.npz")
TILT = np.array([[0.36, 0.48, 0.80], [0.80, -0.60, 0.0], [0.48, 0.64, -0.60]])        # the normals of the three planes between the patches


def octant_palette(v, t):
    """the palette index of every triangle: the octant of its centroid in the tilted frame"""
    h = np.asarray(v, np.float32).astype(np.float64)[t].mean(1) @ TILT.T
    return ((h[:, 0] > 0) + 2 * (h[:, 1] > 0) + 4 * (h[:, 2] > 0)).astype(np.int64)


def split_per_triangle(v, t):
    """(vertices [3F,3], triangles [F,3] = arange, colours uint8 [3F,3], palette index [F]): every dense triangle on its own three
    vertices, painted one flat colour of PALETTE; the geometry, and so every closest point, is the shared-vertex mesh's"""
    pick = octant_palette(v, t)
    return (np.ascontiguousarray(v[t.reshape(-1)]), np.arange(3 * len(t), dtype=np.int32).reshape(-1, 3), np.repeat(PALETTE[pick], 3, axis=0), pick)


@functools.lru_cache(maxsize=None)
def bake_inputs(recorded=True):
    """dense (v, t, c) -- v the recorded vertices, or with recorded=False this machine's uv_sphere --, simple (v, t) = the restated vertex
    clustering at BAKE_DIVISOR, uv / owner = the restated layout at BAKE_SIZE, where [Q,2] = the owned texels as (row, column) with their
    fp64 points, flat = split_per_triangle.  Quick; read-only."""
    v, t = uv_sphere(BAKE_NU, BAKE_NV)
    if recorded:
        v = np.load(GOLD)["v"]
    c = smooth_colors(v)
    sv, st, _, _ = RS.restated_simplify(v, t, c, BAKE_DIVISOR)
    uv, owner, _ = BR.layout(len(st), BAKE_SIZE)
    where, own, pts = BR.texel_points(sv, st, BAKE_SIZE)
    assert np.array_equal(own, owner[where[:, 0], where[:, 1]]) and len(own) == int((owner >= 0).sum())
    out = dict(dense=(v, t, c), simple=(sv, st), uv=uv, owner=owner, where=where, points=pts, flat=split_per_triangle(v, t))
    for x in (v, t, c, sv, st, uv, owner, where, pts) + out["flat"]:
        x.setflags(write=False)
    return out


def bake_reference(inputs):
    """The restated bake of bake_inputs, brute force (some 20 s): tri [Q] = the closest dense triangle of every owned texel, image = the
    bake of the smooth colours, flat_image = the bake of the palette, ambiguous [Q] = texels whose nearest dense triangle of ANOTHER
    colour lies within AMBIGUOUS (of the squared bounding-box diagonal) of the nearest one."""
    v, t, c = inputs["dense"]
    where = inputs["where"]
    tri, bary, d2, every = BR.closest_on_mesh(inputs["points"], v, t, return_all=True)
    fv, ft, fc, pick = inputs["flat"]
    image = np.full((BAKE_SIZE, BAKE_SIZE, 3), 128, np.uint8)
    image[where[:, 0], where[:, 1]] = BR.mix_colors(tri, bary, t, c)
    flat_image = np.full((BAKE_SIZE, BAKE_SIZE, 3), 128, np.uint8)
    flat_image[where[:, 0], where[:, 1]] = BR.mix_colors(tri, bary, ft, fc)
    other = np.where(pick[None, :] != pick[tri][:, None], every, np.inf).min(1)
    vv = v.astype(np.float64)
    diag2 = float(((vv.max(0) - vv.min(0)) ** 2).sum())
    return dict(tri=tri, image=image, flat_image=flat_image, ambiguous=(other - d2) < AMBIGUOUS * diag2, min_bary=float(bary.min()))


@functools.lru_cache(maxsize=None)
def bake_record():
    """what scripts/gen_golden_bake.py recorded of bake_reference(bake_inputs()): v, tri, image, flat_image, ambiguous (read-only)"""
    z = np.load(GOLD)
    out = {k: z[k] for k in ("v", "tri", "image", "flat_image", "ambiguous")}
    for x in out.values():
        x.setflags(write=False)
    return out
