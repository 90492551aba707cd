"""Seeded scenes of the preview renderer's tests (TEST INFRASTRUCTURE ONLY), shared by tests/test_preview_cpu.py (which checks that they
hold what the GPU tests rely on: background, overlaps, ties) and tests/test_gpu_preview.py.  A scene is a dict: v [V,3] float32, t [F,3]
int32, c [V,3] uint8, eye, at (the camera looks down -z from (0, 0, 3) at a [-1.1, 1.1]^2 window of the plane z = 0), fov, near, far."""
import math

import numpy as np

EYE, AT = np.array([0.0, 0.0, 3.0]), np.array([0.0, 0.0, 0.0])
FOV = 2.0 * math.degrees(math.atan(1.1 / 3.0))
NEAR, FAR = 1.5, 4.5


def _scene(v, t, seed):
    v = np.asarray(v, np.float32)
    c = np.random.RandomState(seed + 1000).randint(0, 256, (len(v), 3)).astype(np.uint8)
    return dict(v=v, t=np.asarray(t, np.int32), c=c, eye=EYE.copy(), at=AT.copy(), fov=FOV, near=NEAR, far=FAR)


def random_triangles(seed=0, n_own=190, n_shared=100, n_copies=10):
    """n_own + n_shared + n_copies = 300 triangles: small ones with their own vertices at random depths (they cross each other), then
    ones that share an edge with an earlier triangle, then exact copies of earlier triangles (every pixel a depth tie: the lower index
    wins), every other copy with the winding reversed"""
    rs = np.random.RandomState(seed)
    ctr = np.concatenate([rs.uniform(-0.95, 0.95, (n_own, 1, 2)), rs.uniform(-0.6, 0.6, (n_own, 1, 1))], 2)
    off = np.concatenate([rs.uniform(-0.22, 0.22, (n_own, 3, 2)), rs.uniform(-0.5, 0.5, (n_own, 3, 1))], 2)
    v = list((ctr + off).reshape(-1, 3))
    t = [[3 * i, 3 * i + 1, 3 * i + 2] for i in range(n_own)]
    for _ in range(n_shared):
        a, b, _c = t[rs.randint(len(t))]
        mid = (v[a] + v[b]) * 0.5
        v.append(mid + np.concatenate([rs.uniform(-0.25, 0.25, 2), rs.uniform(-0.4, 0.4, 1)]))
        t.append([b, a, len(v) - 1])
    for k in range(n_copies):
        a, b, c = t[rs.randint(n_own + n_shared)]
        t.append([a, b, c] if k % 2 == 0 else [a, c, b])
    return _scene(np.stack(v), t, seed)


def sheet(seed=1, n=9):
    """an n x n grid of vertices jittered in the plane z = 0 (the border pushed outside the view), 2 (n - 1)^2 triangles with alternating
    diagonals and alternating windings: covers the whole view, every interior edge shared by exactly two triangles"""
    rs = np.random.RandomState(seed)
    g = np.linspace(-1.3, 1.3, n)
    x, y = np.meshgrid(g, g, indexing="xy")
    jit = rs.uniform(-0.1, 0.1, (n, n, 2))
    jit[0, :], jit[-1, :], jit[:, 0], jit[:, -1] = 0, 0, 0, 0
    v = np.stack([x + jit[..., 0], y + jit[..., 1], np.zeros_like(x)], -1).reshape(-1, 3)
    t = []
    for j in range(n - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i, j * n + i + 1, (j + 1) * n + i + 1, (j + 1) * n + i
            tri = [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
            if (i + 2 * j) % 3 == 0:
                tri = [[p, r, q] for p, q, r in tri]
            t += tri
    return _scene(v, t, seed)


def big_behind_small(seed=2, n_small=50):
    """face 0: one triangle that covers the whole view at z = -0.5, then n_small small triangles in front of it"""
    rs = np.random.RandomState(seed)
    v = [np.array([-3.6, -1.4, -0.5]), np.array([3.6, -1.4, -0.5]), np.array([0.0, 3.7, -0.5])]      # (inside the guard band at 256^2)
    t = [[0, 1, 2]]
    for i in range(n_small):
        ctr = np.concatenate([rs.uniform(-0.9, 0.9, 2), rs.uniform(0.0, 0.5, 1)])
        for _ in range(3):
            v.append(ctr + np.concatenate([rs.uniform(-0.15, 0.15, 2), rs.uniform(-0.1, 0.1, 1)]))
        t.append([3 + 3 * i, 4 + 3 * i, 5 + 3 * i])
    return _scene(np.stack(v), t, seed)


def icosphere(subdivisions=2):
    """(vertices [162,3], triangles [320,3], colours [162,4]) for 2 subdivisions of the icosahedron"""
    p = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    t = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nt = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                x = v[a] + v[b]
                v.append(x / np.linalg.norm(x))
                mid[k] = len(v) - 1
            return mid[k]

        for a, b, c in t:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        t = nt
    v = np.stack(v).astype(np.float32) * np.float32(0.5)
    c = np.concatenate([np.clip((v + 0.5) * 255, 0, 255), np.full((len(v), 1), 255)], 1).astype(np.uint8)
    return v, np.asarray(t, np.int32), c


# a two-bone strip: 6 vertices along y, joint 0 at the origin, joint 1 at (0, 1, 0); the lower pair follows joint 0, the upper pair joint 1,
# the middle pair both halves.  The track turns joint 1 by 0, 90 and 180 degrees about z.
STRIP_V = np.array([[-0.1, 0, 0], [0.1, 0, 0], [-0.1, 1, 0], [0.1, 1, 0], [-0.1, 2, 0], [0.1, 2, 0]], np.float32)
STRIP_T = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4], [3, 5, 4]], np.int32)
STRIP_C = np.array([[255, 0, 0, 255], [255, 0, 0, 255], [0, 255, 0, 255], [0, 255, 0, 255], [0, 0, 255, 255], [0, 0, 255, 255]], np.uint8)
STRIP_JOINTS = np.array([[[0, 0, 0, 0]] * 2 + [[0, 1, 0, 0]] * 2 + [[1, 0, 0, 0]] * 2], np.uint8)
STRIP_WEIGHTS = np.array([[[1, 0, 0, 0]] * 2 + [[0.5, 0.5, 0, 0]] * 2 + [[1, 0, 0, 0]] * 2], np.float32)
STRIP_JOINT_POS = np.array([[0, 0, 0], [0, 1, 0]], np.float64)
STRIP_ANGLES = (0.0, 90.0, 180.0)


def write_strip_glb(path, animated=True):
    from avatarclip_amd import rig
    times = rot = None
    if animated:
        times = np.arange(len(STRIP_ANGLES), dtype=np.float32) / np.float32(30)
        rot = np.zeros((len(STRIP_ANGLES), 2, 4), np.float32)
        rot[:, 0, 3] = 1
        for k, a in enumerate(STRIP_ANGLES):
            rot[k, 1] = (0, 0, math.sin(math.radians(a) / 2), math.cos(math.radians(a) / 2))
    return rig.write_glb(path, STRIP_V, STRIP_T, STRIP_C, STRIP_JOINTS, STRIP_WEIGHTS, STRIP_JOINT_POS, parents=(-1, 0), names=("root", "tip"),
                         times=times, rotations=rot, name="strip")


def strip_expected():
    """the hand-computed positions [3,6,3]: a rotation of joint 1 by angle a about z through (0, 1, 0) moves p to (0, 1, 0) + Rz(a)(p - (0, 1, 0));
    the middle pair lies at y = 1, blends half of that with half of staying"""
    out = np.zeros((len(STRIP_ANGLES), 6, 3))
    for k, a in enumerate(STRIP_ANGLES):
        c, s = round(math.cos(math.radians(a)), 12), round(math.sin(math.radians(a)), 12)
        for i, p in enumerate(STRIP_V.astype(np.float64)):
            d = p - np.array([0.0, 1.0, 0.0])
            moved = np.array([0.0, 1.0, 0.0]) + np.array([c * d[0] - s * d[1], s * d[0] + c * d[1], d[2]])
            w1 = (0.0, 0.0, 0.5, 0.5, 1.0, 1.0)[i]
            out[k, i] = (1 - w1) * p + w1 * moved
    return out
