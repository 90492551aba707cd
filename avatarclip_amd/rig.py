"""Export a rigged avatar: Avatar2FBX/export_fbx.py:49-109 (with utils/ply_utils.py) on the device, written as binary glTF 2.0.

    python -m avatarclip_amd.rig --mesh X.ply --smpl SMPL.npz|pkl --pose_npy stand_pose.npy --out_dir D
                                 [--name NAME] [--motion motion.npy] [--fps 60] [--voxel_divisor 256] [--no_simplify]
                                 [--cleanup] [--max_influences K] [--scale 1.0] [--keep_root] [--bake_texture SIZE] [--preview]

writes D/<name>.glb (mesh, vertex colours, the 24-joint SMPL skeleton under Mixamo's bone names, the skin, and with --motion one rotation
track per joint) and D/<name>_rig.npz (the reference's `smpl_object`, export_fbx.py:102-109, under its own keys and shapes, plus `nearest`
and `parents`: what fbx_utils.CreateScene takes, for whoever owns Autodesk's FBX SDK -- the FBX container is the one part not built here).
The steps and their reference lines:
  simplify_mesh      vertex clustering, contraction Average     ply_utils.py:16-19   csrc/avc_rig.hip (restated from open3d's published
                                                                                    algorithm: UNPINNED against open3d itself)
  rotate, nearest template vertex, blend-weight gather         export_fbx.py:55-73  drive.rotate_vertices / drive.find_nearest_ind, avc_skin_pack
  inv_lbs            T-pose vertices                            :84                  drive.inv_lbs
  T-pose joints      J_regressor @ v_template (betas = 0)       :85-86
  skeleton           joint = parent + translation, no rotation  fbx_utils.py:140-243 (its align_vectors block only feeds commented-out lines)
  skin               one cluster per joint                      fbx_utils.py:246-274 -> JOINTS_n / WEIGHTS_n, inverseBindMatrices = translate(-joint)
  animation          the reference's TODO (fbx_utils.py:320)    drive.read_pose_my -> avc_rot_to_quat; this port's extension
Choices this port makes where the reference leaves one open: the triangle order of the simplified mesh (open3d's comes out of a hash set)
is the order of each surviving triangle's first occurrence in the input; the file carries ALL non-zero weights of a vertex, in as many
JOINTS_n / WEIGHTS_n sets as the fullest vertex needs, unless --max_influences cuts them.  The mesh is stored in SMPL's T-pose frame (y
up) and the tracks carry drive's root rotation (pi/2, 0, 0), which turns the PLAYED avatar into Blender's frame (z up, as drive's .pc2):
this project's own renderer (avatarclip_amd.preview) shows the rest pose upright with --up y and a played track upright with --up z, so
a viewer that takes glTF's y-up convention at its word would show the motion lying down unless --keep_root is given.  --preview renders
the file into D/<name>_preview.gif with the up axis that fits what was written.  No third-party viewer has been tried.
--bake_texture SIZE (this port's extension, avatarclip_amd/bake.py) separates colour resolution from triangle count: the colours of the
mesh BEFORE the clustering are baked into a SIZE x SIZE base-colour texture on the mesh after it, and the .glb carries TEXCOORD_0, one
material and the PNG (also written as D/<name>_texture.png) instead of COLOR_0, with one vertex per triangle corner."""
import argparse
import json
import os
import struct

import numpy as np
import torch

from . import drive
from . import lib as L
from . import mesh as _mesh
from . import smpl_lbs

MAX_VOXEL_DIVISOR = 1022                  # AVC_RIG_MAX_DIVISOR: 10-bit cell indices in [0, divisor + 1]
MAX_KEYED_VERTICES = 1 << 21              # AVC_RIG_MAX_KEYED_VERTICES: three output indices in one 63-bit triangle key
NUM_JOINTS = 24
# SMPL's kinematic tree (kintree_table[0]; fbx_utils.Child2Father) and Mixamo's bone names in SMPL's joint order
SMPL_PARENTS = (-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21)
JOINT_NAMES = tuple("mixamorig:" + n for n in (
    "Hips", "LeftUpLeg", "RightUpLeg", "Spine", "LeftLeg", "RightLeg", "Spine1", "LeftFoot", "RightFoot", "Spine2", "LeftToeBase",
    "RightToeBase", "Neck", "LeftShoulder", "RightShoulder", "Head", "LeftArm", "RightArm", "LeftForeArm", "RightForeArm", "LeftHand",
    "RightHand", "LeftHandMiddle1", "RightHandMiddle1"))


# ---------------------------------------------------------------------------------------------------------------- simplification
def voxel_grid(min_bound, max_bound, voxel_divisor):
    """(voxel_size, origin [3]) in fp64: voxel_size = max(max_bound - min_bound) / voxel_divisor (ply_utils.py:17), origin = min_bound -
    voxel_size * 0.5 (open3d's simplify_vertex_clustering)"""
    mn, mx = np.asarray(min_bound, np.float64), np.asarray(max_bound, np.float64)
    voxel = float(np.max(mx - mn)) / voxel_divisor
    return voxel, mn - voxel * 0.5


def simplify_mesh(vertices, triangles, colors=None, voxel_divisor=256, return_map=False):
    """ply_utils.py:16-19, open3d's vertex clustering with contraction Average (csrc/avc_rig.hip; the rules in DESIGN section 8, row f-6).
    vertices [N,3] float32, triangles [F,3], colors [N,3|4] uint8 or None (arrays or device tensors).  Returns device tensors (vertices
    [M,3] float32, triangles [F',3] int32, colors [M,3] float32 in [0, 1] or None), and with return_map the output index of every input
    vertex (int32 [N]).  One output vertex per occupied cell in the order the cells are first met; triangles in the order of their first
    occurrence.  More than 2^21 output vertices raise ValueError (the duplicate search packs three indices into 63 bits)."""
    if not 1 <= int(voxel_divisor) <= MAX_VOXEL_DIVISOR:
        raise ValueError("voxel_divisor must lie in [1, %d] (10-bit cell indices), got %s" % (MAX_VOXEL_DIVISOR, voxel_divisor))
    device = vertices.device if torch.is_tensor(vertices) and vertices.is_cuda else torch.device("cuda")
    v = vertices if torch.is_tensor(vertices) else torch.as_tensor(np.asarray(vertices))
    if v.dim() != 2 or v.shape[1] != 3 or v.shape[0] == 0:
        raise ValueError("vertices must be [N, 3] with N > 0, got %s" % (tuple(v.shape),))
    v = v.to(device=device, dtype=torch.float32).contiguous()
    t = drive._i32(triangles, device).reshape(-1, 3)
    N, F = v.shape[0], t.shape[0]
    c = None
    if colors is not None:
        c = torch.as_tensor(np.asarray(colors) if not torch.is_tensor(colors) else colors)
        if c.dim() != 2 or c.shape[0] != N or c.shape[1] not in (3, 4) or c.dtype != torch.uint8:
            raise ValueError("colors must be [N, 3] or [N, 4] uint8, got %s %s" % (tuple(c.shape), c.dtype))
        c = c.to(device).contiguous()
    if F and (int(t.min()) < 0 or int(t.max()) >= N):
        raise ValueError("a triangle names a vertex outside [0, %d)" % N)
    if not bool(torch.isfinite(v).all()):
        raise ValueError("simplify_mesh: a vertex is not finite")
    mn, mx = torch.aminmax(v, dim=0)
    voxel, origin = voxel_grid(mn.cpu().numpy(), mx.cpu().numpy(), int(voxel_divisor))
    if not voxel > 0.0:
        raise ValueError("simplify_mesh: the mesh has no extent")
    s = L.stream()
    keyed = torch.empty(N, device=device, dtype=torch.int64)
    L.call("avc_rig_cell_keys", v, N, float(origin[0]), float(origin[1]), float(origin[2]), voxel, int(voxel_divisor), keyed, stream=s)
    keyed = torch.sort(keyed).values                       # distinct words: a cell is a run, its vertices ascending
    first = torch.empty(N, device=device, dtype=torch.int32)
    L.call("avc_rig_cluster_heads", keyed, N, first, stream=s)
    finc = torch.cumsum(first, 0, dtype=torch.int32)
    M = int(finc[-1].item())
    rank = finc - first                                    # exclusive scan: the cell's rank by its first vertex
    v_out = torch.empty(M, 3, device=device, dtype=torch.float32)
    c_out = torch.empty(M, 3, device=device, dtype=torch.float32) if c is not None else None
    vmap = torch.empty(N, device=device, dtype=torch.int32)
    L.call("avc_rig_cluster_average", keyed, N, v, c, c.shape[1] if c is not None else 0, rank, M, v_out, c_out, vmap, stream=s)
    del keyed, first, finc, rank
    t_out = torch.empty(0, 3, device=device, dtype=torch.int32)
    if F:
        if M > MAX_KEYED_VERTICES:
            raise ValueError("simplify_mesh: %d output vertices; the duplicate-triangle search handles at most 2^21 = %d (use a smaller "
                             "voxel_divisor)" % (M, MAX_KEYED_VERTICES))
        tri = torch.empty(F, 3, device=device, dtype=torch.int32)
        key = torch.empty(F, device=device, dtype=torch.int64)
        L.call("avc_rig_tri_keys", t, F, N, vmap, M, tri, key, stream=s)
        skey, order = torch.sort(key, stable=True)         # stable: among equal keys the first input occurrence leads
        tflag = torch.empty(F, device=device, dtype=torch.int32)
        L.call("avc_rig_tri_unique", skey, order.contiguous(), F, tflag, stream=s)
        tinc = torch.cumsum(tflag, 0, dtype=torch.int32)
        n_t = int(tinc[-1].item())
        tid = tinc - tflag
        t_out = torch.empty(n_t, 3, device=device, dtype=torch.int32)
        if n_t:
            L.call("avc_rig_tri_compact", tri, F, tflag, tid, n_t, t_out, stream=s)
    return (v_out, t_out, c_out, vmap) if return_map else (v_out, t_out, c_out)


def unit_colors(colors):
    """uint8 colours -> what open3d holds and export_fbx.py:55 casts: c / 255 in fp64, as float32 [N,3]"""
    return (np.asarray(colors)[:, :3].astype(np.float64) / 255.0).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- skin, tracks
def skin_pack(lbs_weights, nearest, max_influences=0):
    """export_fbx.py:73,88 and the influence lists of the file (avc_skin_sort_template / avc_skin_pack): lbs_weights [K,24] float32, nearest
    int32 [M] -> (joints uint8 [S,M,4], weights float32 [S,M,4], blend_weights float32 [24,M]).  Every vertex's non-zero weights sorted by
    weight descending then joint ascending, S = ceil(n / 4) sets for the fullest vertex's n; unused slots joint 0, weight 0.
    max_influences > 0 keeps that many and renormalises them in float32 (blend_weights stays the reference's dense matrix)."""
    w = lbs_weights.to(torch.float32).contiguous()
    K, M = w.shape[0], nearest.shape[0]
    if w.dim() != 2 or w.shape[1] != NUM_JOINTS or nearest.dtype != torch.int32 or M == 0:
        raise ValueError("skin_pack takes lbs_weights [K, 24] and nearest int32 [M > 0]")
    if int(nearest.min()) < 0 or int(nearest.max()) >= K:
        raise ValueError("skin_pack: a template index outside [0, %d)" % K)
    if max_influences < 0:
        raise ValueError("max_influences must be >= 0")
    dev, s = w.device, L.stream()
    tj = torch.empty(K, NUM_JOINTS, device=dev, dtype=torch.uint8)
    tw = torch.empty(K, NUM_JOINTS, device=dev, dtype=torch.float32)
    count = torch.empty(K, device=dev, dtype=torch.int32)
    L.call("avc_skin_sort_template", w, K, int(max_influences), tj, tw, count, stream=s)
    sets = (int(count[nearest.long()].max().item()) + 3) // 4
    joints = torch.empty(sets, M, 4, device=dev, dtype=torch.uint8)
    weights = torch.empty(sets, M, 4, device=dev, dtype=torch.float32)
    blend = torch.empty(NUM_JOINTS, M, device=dev, dtype=torch.float32)
    L.call("avc_skin_pack", w, tj, tw, K, nearest.contiguous(), M, sets, joints if sets else None, weights if sets else None, blend, stream=s)
    return joints, weights, blend


def rot_to_quat(rot_mats):
    """[..., 3, 3] float32 device rotation matrices -> [..., 4] unit quaternions (x, y, z, w), w >= 0 (avc_rot_to_quat, Shepperd's method)"""
    if rot_mats.shape[-2:] != (3, 3):
        raise ValueError("rot_to_quat takes [..., 3, 3]")
    r = rot_mats.to(torch.float32).contiguous()
    q = torch.empty(r.shape[:-2] + (4,), device=r.device, dtype=torch.float32)
    n = q.numel() // 4
    if n:
        L.call("avc_rot_to_quat", r, n, q)
    return q


def motion_rotations(motion, keep_root=False):
    """drive.read_pose_my's rotations [T,24,3,3] (root = (pi/2, 0, 0), what drive plays); keep_root: the root of the motion itself ([T,72+]
    layouts; the 69 / 63 layouts carry none: identity)"""
    rot = drive.read_pose_my(motion)
    if keep_root:
        poses = np.load(motion) if isinstance(motion, (str, os.PathLike)) else np.asarray(motion)
        poses = np.array(poses, dtype=np.float32)
        poses = poses[None] if poses.ndim == 1 else poses
        root = poses[:, :3] if poses.shape[1] >= 72 else np.zeros((poses.shape[0], 3), np.float32)
        rot[:, 0] = smpl_lbs.batch_rodrigues(torch.from_numpy(np.ascontiguousarray(root)))
    return rot


# ---------------------------------------------------------------------------------------------------------------- binary glTF
GLB_MAGIC, GLB_JSON, GLB_BIN = 0x46546C67, 0x4E4F534A, 0x004E4942
_CTYPE = {5120: np.int8, 5121: np.uint8, 5122: np.int16, 5123: np.uint16, 5125: np.uint32, 5126: np.float32}
_CODE = {np.dtype(v): k for k, v in _CTYPE.items()}
_NCOMP = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}
ARRAY_BUFFER, ELEMENT_ARRAY_BUFFER = 34962, 34963


class _Bin:
    """the BIN chunk being assembled: every bufferView starts on a 4-byte boundary"""

    def __init__(self):
        self.blob, self.views, self.accessors = bytearray(), [], []

    def add(self, array, kind, target=None, normalized=False, minmax=False):
        a = np.ascontiguousarray(array)
        a = a.astype(a.dtype.newbyteorder("<"), copy=False)
        self.blob += b"\0" * (-len(self.blob) % 4)
        view = {"buffer": 0, "byteOffset": len(self.blob), "byteLength": a.nbytes}
        if target is not None:
            view["target"] = target
        self.blob += a.tobytes()
        self.views.append(view)
        acc = {"bufferView": len(self.views) - 1, "componentType": _CODE[np.dtype(a.dtype.name)], "count": int(a.shape[0]), "type": kind}
        if normalized:
            acc["normalized"] = True
        if minmax:
            flat = a.reshape(a.shape[0], -1)
            acc["min"], acc["max"] = [float(x) for x in flat.min(0)], [float(x) for x in flat.max(0)]
        self.accessors.append(acc)
        return len(self.accessors) - 1

    def add_bytes(self, data):
        """a bufferView of its own without target or accessor (an image): its index"""
        self.blob += b"\0" * (-len(self.blob) % 4)
        self.views.append({"buffer": 0, "byteOffset": len(self.blob), "byteLength": len(data)})
        self.blob += bytes(data)
        return len(self.views) - 1


LINEAR, CLAMP_TO_EDGE = 9729, 33071


def encode_png(image):
    """uint8 [T,T,3] -> the bytes of an RGB PNG (PIL)"""
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(image), "RGB").save(buf, format="PNG")
    return buf.getvalue()


def decode_png(data):
    """the bytes of a PNG -> uint8 [H,W,C] (PIL); ValueError when they are no PNG"""
    import io
    from PIL import Image
    try:
        im = Image.open(io.BytesIO(bytes(data)))
        if im.format != "PNG":
            raise ValueError("the image is %s, not PNG" % im.format)
        a = np.asarray(im)
    except ValueError:
        raise
    except Exception as e:
        raise ValueError("the image does not decode: %s" % e) from None
    return a if a.ndim == 3 else a[:, :, None]


def write_glb(path, positions, triangles, colors, joints, weights, joint_positions, parents=SMPL_PARENTS, names=JOINT_NAMES, times=None,
              rotations=None, name="avatar", uv=None, texture=None):
    """One skinned mesh on a joint tree as binary glTF 2.0 (numpy + json + struct).  positions [M,3] float32; triangles [F,3] (uint32
    indices); colors [M,4] uint8 or None (COLOR_0, normalised); joints [S,M,4] uint8 and weights [S,M,4] float32 (JOINTS_n / WEIGHTS_n);
    joint_positions [J,3] in the positions' units; parents [J] (-1: the root).  Joint nodes 0..J-1 carry translation = joint - parent's
    joint (the root its joint) and no rest rotation; node J holds the mesh and is a sibling of the root (fbx_utils.CreateScene);
    inverseBindMatrices = translate(-joint), column-major.  times [T] float32 seconds and rotations [T,J,4] (x, y, z, w): one LINEAR
    rotation channel per joint.  uv [M,2] float32 with texture uint8 [T,T,3] (both or neither): TEXCOORD_0 and one material whose
    pbrMetallicRoughness.baseColorTexture is that image, stored as PNG in a bufferView of its own, sampled LINEAR with CLAMP_TO_EDGE."""
    positions = np.asarray(positions, np.float32)
    triangles = np.asarray(triangles)
    joints, weights = np.asarray(joints), np.asarray(weights, np.float32)
    jp = np.asarray(joint_positions, np.float64)
    parents = [int(p) for p in parents]
    M, J = positions.shape[0], jp.shape[0]
    if positions.ndim != 2 or positions.shape[1] != 3 or M == 0:
        raise ValueError("write_glb: positions must be [M > 0, 3]")
    if triangles.ndim != 2 or triangles.shape[1] != 3 or (triangles.size and (triangles.min() < 0 or triangles.max() >= M)):
        raise ValueError("write_glb: triangles must be [F, 3] with indices in [0, M)")
    if joints.dtype != np.uint8 or joints.ndim != 3 or joints.shape[1:] != (M, 4) or weights.shape != joints.shape or joints.shape[0] == 0:
        raise ValueError("write_glb: joints uint8 [S > 0, M, 4] and weights float32 [S, M, 4]")
    if int(joints.max()) >= J or len(parents) != J or len(names) != J or jp.shape != (J, 3):
        raise ValueError("write_glb: joint_positions [J,3], parents [J], names [J], joint indices below J")
    roots = [i for i, p in enumerate(parents) if p < 0]
    if len(roots) != 1 or any(not (p < i) for i, p in enumerate(parents)):
        raise ValueError("write_glb: one root, every parent before its child")
    if colors is not None and (np.asarray(colors).dtype != np.uint8 or np.asarray(colors).shape != (M, 4)):
        raise ValueError("write_glb: colors must be uint8 [M, 4]")
    if (uv is None) != (texture is None):
        raise ValueError("write_glb: uv and texture go together")
    if uv is not None:
        uv, texture = np.asarray(uv), np.asarray(texture)
        if uv.dtype != np.float32 or uv.shape != (M, 2):
            raise ValueError("write_glb: uv must be float32 [M, 2]")
        if texture.dtype != np.uint8 or texture.ndim != 3 or texture.shape[0] != texture.shape[1] or texture.shape[2] != 3 or texture.shape[0] == 0:
            raise ValueError("write_glb: texture must be uint8 [T, T, 3]")
    b = _Bin()
    attributes = {"POSITION": b.add(positions, "VEC3", ARRAY_BUFFER, minmax=True)}
    if colors is not None:
        attributes["COLOR_0"] = b.add(np.asarray(colors), "VEC4", ARRAY_BUFFER, normalized=True)
    if uv is not None:
        attributes["TEXCOORD_0"] = b.add(uv, "VEC2", ARRAY_BUFFER)
    for s in range(joints.shape[0]):
        attributes["JOINTS_%d" % s] = b.add(joints[s], "VEC4", ARRAY_BUFFER)
        attributes["WEIGHTS_%d" % s] = b.add(weights[s], "VEC4", ARRAY_BUFFER)
    indices = b.add(triangles.astype(np.uint32).reshape(-1), "SCALAR", ELEMENT_ARRAY_BUFFER)
    ibm = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (J, 1))
    ibm[:, 12:15] = -jp.astype(np.float32)                                   # column-major: the translation is the fourth column
    ibm_acc = b.add(ibm, "MAT4")
    nodes = []
    for i in range(J):
        rel = jp[i] - (jp[parents[i]] if parents[i] >= 0 else 0.0)
        node = {"name": str(names[i]), "translation": [float(x) for x in rel]}
        kids = [k for k in range(J) if parents[k] == i]
        if kids:
            node["children"] = kids
        nodes.append(node)
    nodes.append({"name": str(name), "mesh": 0, "skin": 0})
    doc = {"asset": {"version": "2.0", "generator": "avatarclip_amd.rig"}, "scene": 0, "scenes": [{"nodes": [J, roots[0]]}], "nodes": nodes,
           "meshes": [{"name": str(name), "primitives": [{"attributes": attributes, "indices": indices, "mode": 4}]}],
           "skins": [{"inverseBindMatrices": ibm_acc, "joints": list(range(J)), "skeleton": roots[0]}]}
    if uv is not None:
        doc["meshes"][0]["primitives"][0]["material"] = 0
        doc["materials"] = [{"name": str(name), "pbrMetallicRoughness": {"baseColorTexture": {"index": 0}, "metallicFactor": 0.0, "roughnessFactor": 1.0}}]
        doc["textures"] = [{"sampler": 0, "source": 0}]
        doc["samplers"] = [{"magFilter": LINEAR, "minFilter": LINEAR, "wrapS": CLAMP_TO_EDGE, "wrapT": CLAMP_TO_EDGE}]
        doc["images"] = [{"bufferView": b.add_bytes(encode_png(texture)), "mimeType": "image/png"}]
    if rotations is not None:
        rotations, times = np.asarray(rotations, np.float32), np.asarray(times, np.float32)
        if rotations.ndim != 3 or rotations.shape[1:] != (J, 4) or times.shape != (rotations.shape[0],) or times.shape[0] == 0:
            raise ValueError("write_glb: rotations [T > 0, J, 4] and times [T]")
        t_acc = b.add(times, "SCALAR", minmax=True)
        samplers, channels = [], []
        for i in range(J):
            samplers.append({"input": t_acc, "output": b.add(rotations[:, i], "VEC4"), "interpolation": "LINEAR"})
            channels.append({"sampler": i, "target": {"node": i, "path": "rotation"}})
        doc["animations"] = [{"name": "motion", "samplers": samplers, "channels": channels}]
    doc["accessors"], doc["bufferViews"] = b.accessors, b.views
    blob = bytes(b.blob) + b"\0" * (-len(b.blob) % 4)
    doc["buffers"] = [{"byteLength": len(blob)}]
    text = json.dumps(doc, separators=(",", ":")).encode("utf-8")
    text += b" " * (-len(text) % 4)
    with open(path, "wb") as f:
        f.write(struct.pack("<III", GLB_MAGIC, 2, 12 + 8 + len(text) + 8 + len(blob)))
        f.write(struct.pack("<II", len(text), GLB_JSON))
        f.write(text)
        f.write(struct.pack("<II", len(blob), GLB_BIN))
        f.write(blob)
    return path


def _need(ok, what):
    if not ok:
        raise ValueError("read_glb: " + what)


def read_glb(path):
    """A strict reader of what write_glb writes (tests, tools): the container's header, chunk lengths, padding and alignment are checked as
    the glTF 2.0 specification states them (ValueError otherwise).  Returns a dict: `json` (the document), `accessors` (every accessor
    as numpy: [count] or [count, components], MAT4 as [count, 4, 4] in FILE order, i.e. column-major), `nodes` (name, children,
    translation and rotation as float64, mesh, skin, parent), `scene_nodes`, `attributes` (name -> array) and `indices` of the one mesh
    primitive, `skin` (joints, skeleton, inverse_bind_matrices [J,4,4] as mathematical matrices), `animation` (a list of node, path,
    interpolation, times, values), `uv` (TEXCOORD_0, float32 [M,2]) and `image` (the base-colour texture decoded, uint8 [T,T,3]) of a
    textured file, both None otherwise."""
    with open(path, "rb") as f:
        data = f.read()
    _need(len(data) >= 20, "shorter than a header and a chunk header")
    magic, version, length = struct.unpack_from("<III", data, 0)
    _need(magic == GLB_MAGIC, "magic is not 'glTF'")
    _need(version == 2, "container version %d, not 2" % version)
    _need(length == len(data), "header length %d, file length %d" % (length, len(data)))
    jlen, jtype = struct.unpack_from("<II", data, 12)
    _need(jtype == GLB_JSON, "the first chunk is not JSON")
    _need(jlen % 4 == 0 and 20 + jlen <= len(data), "JSON chunk length %d is not a multiple of 4 inside the file" % jlen)
    text = data[20:20 + jlen]
    _need(text.rstrip(b" ") == text.rstrip(), "the JSON chunk is padded with something other than spaces")
    doc = json.loads(text.decode("utf-8"))
    blob = b""
    pos = 20 + jlen
    if pos < len(data):
        _need(pos + 8 <= len(data), "truncated chunk header")
        blen, btype = struct.unpack_from("<II", data, pos)
        _need(btype == GLB_BIN, "the second chunk is not BIN")
        _need(blen % 4 == 0 and pos + 8 + blen == len(data), "BIN chunk length %d does not end the file on a 4-byte boundary" % blen)
        blob = data[pos + 8:]
    _need(doc.get("asset", {}).get("version") == "2.0", "asset.version is not 2.0")
    buffers = doc.get("buffers", [])
    _need(len(buffers) == 1 and "uri" not in buffers[0], "exactly one buffer, the BIN chunk")
    blen = buffers[0]["byteLength"]
    _need(blen <= len(blob) < blen + 4 and not any(blob[blen:]), "buffer.byteLength against the BIN chunk (zero padding of at most 3 bytes)")
    views = doc.get("bufferViews", [])
    for v in views:
        _need(v["buffer"] == 0 and v.get("byteOffset", 0) % 4 == 0, "a bufferView is not 4-byte aligned")
        _need(v.get("byteOffset", 0) + v["byteLength"] <= blen, "a bufferView leaves the buffer")
        _need("byteStride" not in v, "strided bufferViews are not written here")
    spans = sorted((v.get("byteOffset", 0), v["byteLength"]) for v in views)
    for (o0, l0), (o1, _) in zip(spans, spans[1:]):
        _need(o0 + l0 <= o1 and not any(blob[o0 + l0:o1]), "bufferViews overlap or the gap between them is not zero")
    accessors = []
    for a in doc.get("accessors", []):
        v = views[a["bufferView"]]
        dt, nc = np.dtype(_CTYPE[a["componentType"]]).newbyteorder("<"), _NCOMP[a["type"]]
        off = v.get("byteOffset", 0) + a.get("byteOffset", 0)
        _need(off % dt.itemsize == 0 and (nc == 1 or (dt.itemsize * nc) % 4 == 0), "accessor alignment")
        _need(a.get("byteOffset", 0) + a["count"] * nc * dt.itemsize <= v["byteLength"], "an accessor leaves its bufferView")
        arr = np.frombuffer(blob, dtype=dt, count=a["count"] * nc, offset=off).astype(dt.newbyteorder("="))
        arr = arr.reshape(a["count"], 4, 4) if nc == 16 else (arr.reshape(a["count"], nc) if nc > 1 else arr)
        if "min" in a:
            flat = arr.reshape(a["count"], -1)
            _need(np.array_equal(flat.min(0), np.asarray(a["min"], flat.dtype)) and np.array_equal(flat.max(0), np.asarray(a["max"], flat.dtype)),
                  "accessor min / max do not match the data")
        accessors.append(arr)
    nodes = []
    for n in doc.get("nodes", []):
        nodes.append({"name": n.get("name"), "children": list(n.get("children", [])), "translation": np.asarray(n.get("translation", [0, 0, 0]), np.float64),
                      "rotation": np.asarray(n.get("rotation", [0, 0, 0, 1]), np.float64), "mesh": n.get("mesh"), "skin": n.get("skin"), "parent": None})
    for i, n in enumerate(nodes):
        for k in n["children"]:
            _need(0 <= k < len(nodes) and nodes[k]["parent"] is None and k != i, "the node tree is not a tree")
            nodes[k]["parent"] = i
    out = {"json": doc, "accessors": accessors, "nodes": nodes, "scene_nodes": list(doc["scenes"][doc.get("scene", 0)]["nodes"])}
    _need(all(nodes[i]["parent"] is None for i in out["scene_nodes"]), "a scene node has a parent")
    meshes = doc.get("meshes", [])
    _need(len(meshes) == 1 and len(meshes[0]["primitives"]) == 1, "one mesh with one primitive")
    prim = meshes[0]["primitives"][0]
    _need(prim.get("mode", 4) == 4, "the primitive is not a triangle list")
    out["attributes"] = {k: accessors[i] for k, i in prim["attributes"].items()}
    nv = doc["accessors"][prim["attributes"]["POSITION"]]
    _need("min" in nv and "max" in nv and nv["type"] == "VEC3" and nv["componentType"] == 5126, "POSITION is float32 VEC3 with min / max")
    _need(all(doc["accessors"][i]["count"] == nv["count"] for i in prim["attributes"].values()), "attribute counts differ")
    _need(all(views[doc["accessors"][i]["bufferView"]].get("target") == ARRAY_BUFFER for i in prim["attributes"].values()), "attribute bufferView targets")
    ia = doc["accessors"][prim["indices"]]
    _need(ia["type"] == "SCALAR" and ia["componentType"] == 5125 and ia["count"] % 3 == 0 and views[ia["bufferView"]].get("target") == ELEMENT_ARRAY_BUFFER,
          "indices are uint32 scalars, three per triangle, in an ELEMENT_ARRAY_BUFFER view")
    out["indices"] = accessors[prim["indices"]]
    _need(out["indices"].size == 0 or int(out["indices"].max()) < nv["count"], "an index names no vertex")
    for k, i in prim["attributes"].items():
        a = doc["accessors"][i]
        if k.startswith("JOINTS_"):
            _need(a["componentType"] == 5121 and a["type"] == "VEC4" and ("WEIGHTS_" + k[7:]) in prim["attributes"], "JOINTS_n is uint8 VEC4 with its WEIGHTS_n")
        if k.startswith("WEIGHTS_"):
            _need(a["componentType"] == 5126 and a["type"] == "VEC4", "WEIGHTS_n is float32 VEC4")
        if k == "COLOR_0":
            _need(a["componentType"] == 5121 and a["type"] == "VEC4" and a.get("normalized") is True, "COLOR_0 is normalised uint8 VEC4")
        if k == "TEXCOORD_0":
            _need(a["componentType"] == 5126 and a["type"] == "VEC2" and not a.get("normalized"), "TEXCOORD_0 is float32 VEC2")
    out["uv"], out["image"] = out["attributes"].get("TEXCOORD_0"), None
    materials, textures, samplers, images = (doc.get(k, []) for k in ("materials", "textures", "samplers", "images"))
    if "material" in prim or materials or textures or samplers or images:
        _need(len(materials) == 1 and prim.get("material") == 0, "one material, the primitive's")
        pbr = materials[0].get("pbrMetallicRoughness", {})
        _need(pbr.get("metallicFactor") == 0 and pbr.get("roughnessFactor") == 1, "the material is metallicFactor 0, roughnessFactor 1")
        ti = pbr.get("baseColorTexture", {}).get("index")
        _need(isinstance(ti, int) and 0 <= ti < len(textures) and pbr["baseColorTexture"].get("texCoord", 0) == 0, "baseColorTexture names no texture on TEXCOORD_0")
        si, ii = textures[ti].get("sampler"), textures[ti].get("source")
        _need(isinstance(si, int) and 0 <= si < len(samplers), "the texture names no sampler")
        _need(isinstance(ii, int) and 0 <= ii < len(images), "the texture names no image")
        sm = samplers[si]
        _need(sm.get("magFilter") == LINEAR and sm.get("minFilter") == LINEAR and sm.get("wrapS") == CLAMP_TO_EDGE and sm.get("wrapT") == CLAMP_TO_EDGE,
              "the sampler is LINEAR / LINEAR, CLAMP_TO_EDGE both ways")
        im = images[ii]
        _need(im.get("mimeType") == "image/png" and "uri" not in im, "the image is a PNG in the buffer")
        vi = im.get("bufferView")
        _need(isinstance(vi, int) and 0 <= vi < len(views) and "target" not in views[vi], "the image names no bufferView without a target")
        _need(all(a.get("bufferView") != vi for a in doc.get("accessors", [])), "an accessor reads the image's bufferView")
        o = views[vi].get("byteOffset", 0)
        try:
            image = decode_png(blob[o:o + views[vi]["byteLength"]])
        except ValueError as e:
            _need(False, str(e))
        _need(image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3 and image.shape[0] == image.shape[1], "the PNG decodes to uint8 [T, T, 3]")
        _need(out["uv"] is not None, "a textured primitive without TEXCOORD_0")
        out["image"] = np.ascontiguousarray(image)
    else:
        _need(out["uv"] is None, "TEXCOORD_0 without a material")
    skins = doc.get("skins", [])
    _need(len(skins) <= 1, "at most one skin")
    if skins:
        sk = skins[0]
        m = accessors[sk["inverseBindMatrices"]]
        _need(m.shape == (len(sk["joints"]), 4, 4) and m.dtype == np.float32, "inverseBindMatrices: one float32 MAT4 per joint")
        _need(all(int(out["attributes"][k].max()) < len(sk["joints"]) for k in out["attributes"] if k.startswith("JOINTS_")), "a joint index outside the skin")
        out["skin"] = {"joints": list(sk["joints"]), "skeleton": sk.get("skeleton"), "inverse_bind_matrices": m.transpose(0, 2, 1).copy()}
    out["animation"] = []
    for an in doc.get("animations", []):
        for ch in an["channels"]:
            sm = an["samplers"][ch["sampler"]]
            ta = doc["accessors"][sm["input"]]
            _need(ta["type"] == "SCALAR" and ta["componentType"] == 5126 and "min" in ta and "max" in ta, "animation times are float32 scalars with min / max")
            times, values = accessors[sm["input"]], accessors[sm["output"]]
            _need(len(times) == len(values) and (len(times) < 2 or bool(np.all(np.diff(times) > 0))), "animation times ascend, one value each")
            out["animation"].append({"node": ch["target"]["node"], "path": ch["target"]["path"], "interpolation": sm.get("interpolation", "LINEAR"),
                                     "times": times, "values": values})
    return out


def colors_to_u8(colors):
    """float colours in [0, 1] -> uint8 RGBA, round-half-even (np.rint), alpha 255"""
    c = np.rint(np.asarray(colors, np.float32).astype(np.float64) * 255.0).clip(0, 255).astype(np.uint8)
    return np.concatenate([c[:, :3], np.full((len(c), 1), 255, np.uint8)], 1)


# ---------------------------------------------------------------------------------------------------------------- the whole step
def build_rig(mesh, smpl, pose_npy, out_dir, name="avatar", motion=None, fps=60.0, voxel_divisor=256, simplify=True, cleanup=False,
              max_influences=0, scale=1.0, keep_root=False, device=None, bake_texture=0):
    """export_fbx.py:49-109.  mesh: a PLY path (Runner.validate_mesh's) or (vertices, triangles, colors uint8 or None); smpl: a path (.npz /
    official .pkl) or the arrays; pose_npy: stand_pose.npy; motion: None, a .npy path or an array (drive.read_pose_my's layouts).
    Writes out_dir/<name>.glb and out_dir/<name>_rig.npz; returns both paths.
    bake_texture = SIZE > 0 (this port's extension, avatarclip_amd.bake): the colours of the mesh as it is BEFORE the clustering (after
    cleanup) are baked into a SIZE x SIZE atlas on the mesh as it is after it.  The .glb then holds one vertex per triangle corner
    (position and skin gathered from the shared vertex), TEXCOORD_0 and the texture instead of COLOR_0; out_dir/<name>_texture.png is the
    same image, and the .npz gains `uv` [F',3,2] while its other keys stay what they are without the option (shared vertices)."""
    bake_texture = int(bake_texture)
    if bake_texture < 0:
        raise ValueError("bake_texture is a texture size, 0 for none, got %d" % bake_texture)
    device = torch.device(device) if device is not None else torch.device("cuda")
    v, t, c = _mesh.read_ply(str(mesh)) if isinstance(mesh, (str, os.PathLike)) else mesh
    a = smpl_lbs.load_smpl_arrays(smpl, device=str(device)) if isinstance(smpl, (str, os.PathLike)) else \
        {k: (x.to(device) if torch.is_tensor(x) and k != "parents" else x) for k, x in smpl.items()}
    if a["lbs_weights"].shape[1] != NUM_JOINTS or [int(p) for p in a["parents"]][1:] != list(SMPL_PARENTS[1:]):
        raise ValueError("rig: the model is not on SMPL's 24-joint tree")
    if cleanup:                                               # this port's extension: the largest island only (drive.cleanup_mesh)
        v, t, c = drive.cleanup_mesh(v, t, c)
    dense = (v, t, c)
    if bake_texture and c is None:
        raise ValueError("rig: --bake_texture needs a mesh with colours")
    if simplify:
        v, t, colors = simplify_mesh(v, t, c, voxel_divisor)
        colors = None if colors is None else colors.cpu().numpy()
    else:
        c = c.cpu().numpy() if torch.is_tensor(c) else c
        colors = None if c is None else unit_colors(c)
    v = v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v, np.float32)
    triangles = (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).astype(np.int32)
    uv = image = None
    if bake_texture:
        from . import bake as _bake
        uv, image = _bake.bake_texture(v, triangles, dense[0], dense[1], dense[2], bake_texture)
    del dense
    rot_vertices = torch.from_numpy(drive.rotate_vertices(v)).to(device)                      # export_fbx.py:56-62
    template, pose_rot = drive.load_template_smpl(a, pose_npy)
    nearest = drive.find_nearest_ind(rot_vertices, template)                                 # :71
    joints_n, weights_n, blend = skin_pack(a["lbs_weights"], nearest, max_influences)        # :72-73, :88
    tpose = drive.inv_lbs(a, rot_vertices, nearest, pose_rot)                                # :84
    tpose_joints = torch.einsum("bik,ji->bjk", a["v_template"][None], a["J_regressor"])[0]    # :85-86 (betas = 0)
    tpose, tpose_joints = tpose.cpu().numpy(), tpose_joints.cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    npz = os.path.join(out_dir, "%s_rig.npz" % name)
    np.savez(npz, vertices=tpose * 100, triangles=triangles, joints=tpose_joints * 100, blend_weights=blend.cpu().numpy(),
             colors=colors if colors is not None else np.zeros((0, 3), np.float32), name=np.array(str(name)), nearest=nearest.cpu().numpy(),
             parents=np.asarray(SMPL_PARENTS, np.int32), **({} if uv is None else {"uv": uv}))
    times = quats = None
    if motion is not None:
        rot = motion_rotations(motion, keep_root).to(device)
        quats = rot_to_quat(rot).cpu().numpy()
        times = (np.arange(rot.shape[0], dtype=np.float64) / float(fps)).astype(np.float32)
    glb = os.path.join(out_dir, "%s.glb" % name)
    if uv is not None:                                        # one vertex per corner: a chart's UVs belong to one triangle alone
        corner = triangles.reshape(-1).astype(np.int64)
        with open(os.path.join(out_dir, "%s_texture.png" % name), "wb") as f:
            f.write(encode_png(image))
        write_glb(glb, (tpose * np.float32(scale))[corner], np.arange(corner.shape[0], dtype=np.int32).reshape(-1, 3), None,
                  np.ascontiguousarray(joints_n.cpu().numpy()[:, corner]), np.ascontiguousarray(weights_n.cpu().numpy()[:, corner]),
                  tpose_joints * np.float32(scale), times=times, rotations=quats, name=name, uv=uv.reshape(-1, 2), texture=image)
        return glb, npz
    write_glb(glb, tpose * np.float32(scale), triangles, None if colors is None else colors_to_u8(colors), joints_n.cpu().numpy(),
              weights_n.cpu().numpy(), tpose_joints * np.float32(scale), times=times, rotations=quats, name=name)
    return glb, npz


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mesh", required=True, help="the avatar's PLY (Runner.validate_mesh)")
    ap.add_argument("--smpl", required=True, help="SMPL model arrays: .npz or the official .pkl")
    ap.add_argument("--pose_npy", required=True, help="stand_pose.npy: the pose the avatar was generated in")
    ap.add_argument("--out_dir", required=True)
    ap.add_argument("--name", default=None, help="base name of the outputs (default: the mesh file's)")
    ap.add_argument("--motion", default=None, help="motion .npy ([T,72], [T,69], [T,63] or one pose): adds one rotation track per joint")
    ap.add_argument("--fps", type=float, default=60.0, help="frame rate of the tracks (drive's point cache: 60)")
    ap.add_argument("--voxel_divisor", type=int, default=256, help="cells along the longest side of the bounding box (the reference: 256)")
    ap.add_argument("--no_simplify", action="store_true", help="skip the vertex clustering")
    ap.add_argument("--cleanup", action="store_true", help="keep the largest island only (drive.cleanup_mesh) before anything else")
    ap.add_argument("--max_influences", type=int, default=0, help="keep the K largest weights per vertex and renormalise (0: all)")
    ap.add_argument("--scale", type=float, default=1.0, help="unit of the .glb: 1.0 = metres (glTF's), 100 = the reference's centimetres")
    ap.add_argument("--keep_root", action="store_true", help="keep the motion's own root rotation instead of drive's (pi/2, 0, 0)")
    ap.add_argument("--bake_texture", type=int, default=0, metavar="SIZE",
                    help="bake the colours of the mesh before the clustering into a SIZE x SIZE texture on the mesh after it (0: vertex colours)")
    ap.add_argument("--preview", action="store_true", help="also render the .glb into <out_dir>/<name>_preview.gif (avatarclip_amd.preview)")
    args = ap.parse_args(argv)
    name = args.name or os.path.splitext(os.path.basename(args.mesh))[0]
    glb, npz = build_rig(args.mesh, args.smpl, args.pose_npy, args.out_dir, name=name, motion=args.motion, fps=args.fps,
                         voxel_divisor=args.voxel_divisor, simplify=not args.no_simplify, cleanup=args.cleanup,
                         max_influences=args.max_influences, scale=args.scale, keep_root=args.keep_root, bake_texture=args.bake_texture)
    print(glb)
    print(npz)
    if args.preview:
        from . import preview
        # the rest pose is y up; drive's root rotation (pi/2, 0, 0) in the tracks turns the played avatar into Blender's frame, z up
        up = "z" if args.motion is not None and not args.keep_root else "y"
        print(preview.preview(os.path.join(args.out_dir, "%s_preview.gif" % name), glb=glb, up=up)[0])


if __name__ == "__main__":
    main()
