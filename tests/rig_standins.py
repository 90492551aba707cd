"""Seeded inputs and restatements of the rig step (TEST INFRASTRUCTURE ONLY), shared by scripts/gen_golden_rig.py and tests/test_rig_cpu.py /
tests/test_gpu_rig.py.  The template, the avatar mesh and the motion are tests/drive_standins.py's; added here: a 4-sparse variant of the
template's blend weights (the published SMPL has at most 4 non-zero weights per vertex, the seeded stand-in 24), a small hand-made mesh
that meets every rule of the vertex clustering, and `restated_simplify`, the clustering in plain numpy fp64."""
import numpy as np
import torch

from tests import drive_standins as S


def sparse_template_arrays(seed=0, keep=4):
    """drive_standins.template_arrays with only the `keep` largest blend weights of every vertex, renormalised (float32)"""
    a = S.template_arrays(seed)
    w = a["lbs_weights"].numpy().copy()
    drop = np.argsort(-w, axis=1, kind="stable")[:, keep:]
    np.put_along_axis(w, drop, 0.0, axis=1)
    w = (w / w.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)
    a["lbs_weights"] = torch.from_numpy(w)
    return a


# The hand-made mesh: bounding box (0,0,0)-(4,2,1) at voxel_divisor 4 gives voxel_size 1 and origin (-0.5,-0.5,-0.5), so the cell of a
# coordinate x is floor(x + 0.5), every value below exact in binary.
#   vertex  position           cell      output          what it is there for
#   0       (0, 0, 0)          (0,0,0)   0  (A)
#   1       (2, 0, 0)          (2,0,0)   1  (B)
#   2       (0, 2, 0)          (0,2,0)   2  (C)
#   3       (0.25, 0, 0)       (0,0,0)   0  (A)          merges with vertex 0
#   4       (2.25, 0.25, 0)    (2,0,0)   1  (B)          merges with vertex 1
#   5       (4, 2, 1)          (4,2,1)   3  (D)          the far corner: index voxel_divisor on the longest axis
#   6       (0.5, 0, 0)        (1,0,0)   4  (E)          exactly on the boundary between cells 0 and 1 of x: (0.5 + 0.5) / 1 = 1
#   7       (3, 1, 0)          (3,1,0)   5  (F)          in no triangle: still an output vertex
#   8       (0, 1.75, 0.25)    (0,2,0)   2  (C)          merges with vertex 2
#   9       (2, 2, 1)          (2,2,1)   6  (G)
HAND_DIVISOR = 4
HAND_VERTICES = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [0.25, 0, 0], [2.25, 0.25, 0], [4, 2, 1], [0.5, 0, 0], [3, 1, 0], [0, 1.75, 0.25],
                          [2, 2, 1]], np.float32)
HAND_TRIANGLES = np.array([
    [0, 1, 2],   # (A,B,C) -> (0,1,2)
    [4, 8, 3],   # (B,C,A) -> rotated (0,1,2): an exact duplicate of the first, removed
    [3, 2, 1],   # (A,C,B) -> (0,2,1): the opposite orientation, kept
    [0, 3, 1],   # (A,A,B): collapses to an edge, dropped
    [5, 1, 2],   # (D,B,C) = (3,1,2) -> rotated (1,2,3)
    [6, 0, 1],   # (E,A,B) = (4,0,1) -> rotated (0,1,4)
    [9, 5, 4],   # (G,D,B) = (6,3,1) -> rotated (1,6,3)
    [1, 0, 2],   # (B,A,C) = (1,0,2) -> rotated (0,2,1): a duplicate of the third, removed
], np.int32)
HAND_COLORS = np.array([[10, 20, 30, 255], [0, 255, 128, 255], [7, 7, 7, 255], [11, 21, 33, 255], [1, 254, 127, 255], [255, 255, 255, 255],
                        [0, 0, 0, 255], [90, 80, 70, 255], [8, 9, 200, 255], [1, 2, 3, 255]], np.uint8)


def hand_mesh():
    return HAND_VERTICES.copy(), HAND_TRIANGLES.copy(), HAND_COLORS.copy()


def restated_simplify(vertices, triangles, colors, voxel_divisor=256):
    """open3d's simplify_vertex_clustering (contraction Average) at voxel_size = max extent / voxel_divisor, from its published algorithm:
    cell = floor((v - origin) / voxel_size) in fp64 with origin = min_bound - voxel_size / 2; one output vertex per occupied cell in the
    order the cells are first met; position / colour = the fp64 mean (np.bincount adds in input order), rounded to float32; a triangle is
    mapped, dropped if two corners coincide, rotated smallest index first, exact duplicates removed, the first occurrences kept in input
    order.  Returns (vertices [M,3] float32, triangles int32, colors [M,3] float32, vmap [N])."""
    v = np.asarray(vertices, np.float32).astype(np.float64)
    mn, mx = v.min(0), v.max(0)
    voxel = (mx - mn).max() / voxel_divisor
    origin = mn - voxel * 0.5
    cell = np.floor((v - origin) / voxel).astype(np.int64)
    assert cell.min() >= 0 and cell.max() <= voxel_divisor + 1
    key = (cell[:, 0] * (voxel_divisor + 2) + cell[:, 1]) * (voxel_divisor + 2) + cell[:, 2]
    _, first, inverse = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    vmap = rank[inverse.reshape(-1)]
    M = len(first)
    n = np.bincount(vmap, minlength=M).astype(np.float64)
    pos = np.stack([np.bincount(vmap, weights=v[:, k], minlength=M) / n for k in range(3)], 1).astype(np.float32)
    col = None
    if colors is not None:
        c = np.asarray(colors)[:, :3].astype(np.float64) / 255.0
        col = np.stack([np.bincount(vmap, weights=c[:, k], minlength=M) / n for k in range(3)], 1).astype(np.float32)
    t = vmap[np.asarray(triangles, np.int64).reshape(-1, 3)]
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
    if len(t):
        shift = np.argmin(t, 1)
        t = np.stack([t[np.arange(len(t)), (shift + k) % 3] for k in range(3)], 1)
        _, keep = np.unique(t, axis=0, return_index=True)
        t = t[np.sort(keep)]
    return pos, t.astype(np.int32).reshape(-1, 3), col, vmap.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- reading a .glb back
def dense_weights(joints, weights, num_joints=24):
    """JOINTS_n / WEIGHTS_n sets [S,M,4] -> the dense [M, num_joints] matrix (float32: every joint appears at most once per vertex with a
    non-zero weight, so nothing is rounded)"""
    joints, weights = np.asarray(joints), np.asarray(weights, np.float32)
    M = joints.shape[1]
    W = np.zeros((M, num_joints), np.float32)
    for s in range(joints.shape[0]):
        for k in range(4):
            nz = weights[s, :, k] != 0
            assert not (W[np.flatnonzero(nz), joints[s, nz, k]] != 0).any(), "a joint listed twice for one vertex"
            W[np.flatnonzero(nz), joints[s, nz, k]] = weights[s, nz, k]
    return W


def glb_sets(g):
    """(joints [S,M,4], weights [S,M,4]) of what rig.read_glb returned"""
    n = sum(1 for k in g["attributes"] if k.startswith("JOINTS_"))
    return np.stack([g["attributes"]["JOINTS_%d" % s] for s in range(n)]), np.stack([g["attributes"]["WEIGHTS_%d" % s] for s in range(n)])


def _quat_matrix(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def glb_frames(g):
    """The file-side skin evaluator: glTF 2.0's skinning equations in fp64 from nothing but what rig.read_glb returns -- node
    translations and the tree, the animation's quaternions (the rest rotations without one), inverseBindMatrices, JOINTS_n / WEIGHTS_n and
    POSITION.  vertex = sum_j w_j (G_j IBM_j) (p, 1) with G_j = G_parent(j) T(translation_j) R(rotation_j).  Returns [T, M, 3] float64, one
    frame per animation key (one frame in the rest pose without an animation)."""
    nodes, skin = g["nodes"], g["skin"]
    tracks = {ch["node"]: ch["values"] for ch in g["animation"] if ch["path"] == "rotation"}
    T = max([len(v) for v in tracks.values()] + [1])
    W = dense_weights(*glb_sets(g), num_joints=len(skin["joints"])).astype(np.float64)
    p = np.concatenate([g["attributes"]["POSITION"].astype(np.float64), np.ones((W.shape[0], 1))], 1)
    ibm = skin["inverse_bind_matrices"].astype(np.float64)
    out = np.zeros((T, W.shape[0], 3))
    for t in range(T):
        world = {}

        def global_of(i):
            if i not in world:
                local = np.eye(4)
                local[:3, :3] = _quat_matrix(tracks[i][t] if i in tracks else nodes[i]["rotation"])
                local[:3, 3] = nodes[i]["translation"]
                world[i] = local if nodes[i]["parent"] is None else global_of(nodes[i]["parent"]) @ local
            return world[i]

        mats = np.stack([global_of(n) @ ibm[j] for j, n in enumerate(skin["joints"])])          # [J, 4, 4]
        blended = np.einsum("mj,jrc->mrc", W, mats)
        out[t] = np.einsum("mrc,mc->mr", blended, p)[:, :3]
    return out
