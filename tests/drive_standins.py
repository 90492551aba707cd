"""Seeded inputs of the drive step (TEST INFRASTRUCTURE ONLY), shared by scripts/gen_golden_drive.py (which runs the reference's own drive.py
functions on them) and tests/test_drive_cpu.py / tests/test_gpu_drive.py: an SMPL-shaped template (24 joints on SMPL's kinematic tree, ~700
vertices, non-zero pose blend shapes, duplicated vertices so that nearest-point ties are exact) and an "avatar" mesh -- marching cubes of an
analytic body-like SDF (oracle/mcubes_oracle.py) with colours, two detached blobs and an isolated vertex.  Their content is arbitrary; what
the fixture pins is the arithmetic around them."""
import numpy as np
import torch

# SMPL's kinematic tree (kintree_table[0] of the published model)
SMPL_PARENTS = [-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21]
K_TEMPLATE = 700
DUPLICATES = [(70, 690), (649, 12), (193, 194), (111, 500), (333, 699), (16, 450)]   # (source, copy): the copy is identical in every array


def template_arrays(seed=0, K=K_TEMPLATE):
    rs = np.random.RandomState(seed)
    # points of an upright body-ish cloud (SMPL units: metres, y up)
    v = np.stack([rs.uniform(-0.35, 0.35, K), rs.uniform(-1.1, 0.6, K), rs.uniform(-0.15, 0.15, K)], 1).astype(np.float32)
    w = rs.uniform(0, 1, (K, 24)).astype(np.float32) ** 6
    w /= w.sum(1, keepdims=True)
    jreg = rs.uniform(0, 1, (24, K)).astype(np.float32) ** 8
    jreg /= jreg.sum(1, keepdims=True)
    posedirs = (rs.randn(23 * 9, K, 3) * 0.01).astype(np.float32)
    for a, b in DUPLICATES:
        v[b], w[b], posedirs[:, b] = v[a], w[a], posedirs[:, a]
    return dict(v_template=torch.from_numpy(v), posedirs=torch.from_numpy(posedirs.reshape(23 * 9, K * 3)), J_regressor=torch.from_numpy(jreg),
                parents=torch.tensor(SMPL_PARENTS, dtype=torch.int64), lbs_weights=torch.from_numpy(w))


def _capsule(p, a, b, r):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    ab = b - a
    t = np.clip(((p - a) @ ab) / (ab @ ab), 0, 1)
    return np.linalg.norm(p - (a + t[..., None] * ab), axis=-1) - r


def body_sdf(p):
    """a standing figure in the NeuS frame the mesh comes out of (y up, z towards the viewer before drive.py's rotation) + two detached blobs"""
    parts = [
        _capsule(p, (0, -0.05, 0), (0, 0.35, 0), 0.17),           # torso
        np.linalg.norm(p - np.array([0, 0.58, 0], np.float32), axis=-1) - 0.12,   # head
        _capsule(p, (0, 0.38, 0), (0, 0.5, 0), 0.05),             # neck
        _capsule(p, (-0.15, 0.33, 0), (-0.55, 0.1, 0), 0.05),     # arms (A pose)
        _capsule(p, (0.15, 0.33, 0), (0.55, 0.1, 0), 0.05),
        _capsule(p, (-0.09, -0.1, 0), (-0.14, -0.85, 0), 0.07),   # legs
        _capsule(p, (0.09, -0.1, 0), (0.14, -0.85, 0), 0.07),
        np.linalg.norm(p - np.array([0.7, 0.7, 0.3], np.float32), axis=-1) - 0.1,    # blobs
        np.linalg.norm(p - np.array([-0.7, -0.6, -0.4], np.float32), axis=-1) - 0.08,
    ]
    return np.min(np.stack(parts), 0)


def avatar_mesh(res=48):
    """(vertices [N,3] float32 in [-1,1]^3, triangles [F,3] int32, colours [N,4] uint8): vertex 0 is an isolated vertex (an island of its own
    with the smallest index), then the marching-cubes vertices of body_sdf in the oracle's order"""
    from oracle import mcubes_oracle
    g = np.linspace(-1, 1, res, dtype=np.float32)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1)
    v, t = mcubes_oracle.marching_cubes(-body_sdf(p), 0.0)
    v = (v / (res - 1.0) * 2.0 - 1.0).astype(np.float32)
    v = np.concatenate([np.array([[0.9, -0.9, 0.9]], np.float32), v])
    t = (t + 1).astype(np.int32)
    c = np.concatenate([np.clip((v + 1) * 127.5, 0, 255), np.full((len(v), 1), 255)], 1).astype(np.uint8)
    return v, t, c


def tie_mesh():
    """two islands of four vertices and one of three: the two equal ones tie, the one found first (smallest vertex index) is kept; their
    vertices interleave so that order and re-indexing show"""
    v = np.arange(33, dtype=np.float32).reshape(11, 3) * 0.1
    t = np.array([[1, 3, 5], [3, 5, 7], [0, 2, 4], [2, 4, 6], [8, 9, 10]], np.int32)
    c = np.stack([np.arange(11), np.arange(11) * 2, np.arange(11) * 3, np.full(11, 255)], 1).astype(np.uint8)
    return v, t, c


def motion(T=8, seed=3):
    return (np.random.RandomState(seed).randn(T, 72) * 0.3).astype(np.float32)
