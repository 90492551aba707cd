"""The host side of the rig step (avatarclip_amd/rig.py) without a GPU: the clustering rules on a hand-made mesh, the binary glTF container
written and read back, a skin evaluator that plays the file and must land on drive's skinning, and the joint tables against the
reference's (tests/golden/rig.npz, scripts/gen_golden_rig.py)."""
import json
import os
import struct

import numpy as np
import pytest
import torch

from tests import drive_standins as S
from tests import rig_standins as RS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rig.npz")


def test_restated_simplify_on_the_hand_made_mesh():
    v, t, c, vmap = RS.restated_simplify(*RS.hand_mesh(), RS.HAND_DIVISOR)
    assert v.dtype == np.float32 and t.dtype == np.int32 and c.dtype == np.float32
    assert vmap.tolist() == [0, 1, 2, 0, 1, 3, 4, 5, 2, 6]
    assert v.tolist() == [[0.125, 0, 0], [2.125, 0.125, 0], [0, 1.875, 0.125], [4, 2, 1], [0.5, 0, 0], [3, 1, 0], [2, 2, 1]]
    assert t.tolist() == [[0, 1, 2], [0, 2, 1], [1, 2, 3], [0, 1, 4], [1, 6, 3]]
    f = np.float32
    expect = [[f((10 / 255 + 11 / 255) / 2), f((20 / 255 + 21 / 255) / 2), f((30 / 255 + 33 / 255) / 2)],
              [f((0 / 255 + 1 / 255) / 2), f((255 / 255 + 254 / 255) / 2), f((128 / 255 + 127 / 255) / 2)],
              [f((7 / 255 + 8 / 255) / 2), f((7 / 255 + 9 / 255) / 2), f((7 / 255 + 200 / 255) / 2)],
              [f(1), f(1), f(1)], [f(0), f(0), f(0)], [f(90 / 255), f(80 / 255), f(70 / 255)], [f(1 / 255), f(2 / 255), f(3 / 255)]]
    assert c.tolist() == [[float(x) for x in row] for row in expect]


def test_voxel_grid_and_argument_checks():
    from avatarclip_amd import rig
    voxel, origin = rig.voxel_grid(np.float32([0, 0, 0]), np.float32([4, 2, 1]), 4)
    assert voxel == 1.0 and origin.tolist() == [-0.5, -0.5, -0.5] and origin.dtype == np.float64
    with pytest.raises(ValueError, match="1022"):
        rig.simplify_mesh(RS.HAND_VERTICES, RS.HAND_TRIANGLES, RS.HAND_COLORS, voxel_divisor=1023)
    assert rig.colors_to_u8(np.float32([[0.4 / 255, 1.6 / 255, 2.4 / 255], [1, 0, 254.6 / 255]])).tolist() == [[0, 2, 2, 255], [255, 0, 255, 255]]
    assert rig.unit_colors(np.uint8([[255, 0, 51, 255]])).tolist() == [[1.0, 0.0, float(np.float32(0.2))]]


def _numpy_sets(W):
    """influence lists of a dense [M,24] matrix: weight descending, joint ascending, 4 per set"""
    M = W.shape[0]
    n = int((W != 0).sum(1).max())
    sets = (n + 3) // 4
    order = np.lexsort((np.broadcast_to(np.arange(24), W.shape), -W.astype(np.float64)), axis=1)[:, :sets * 4]
    w = np.take_along_axis(W, order, 1)
    j = np.where(w != 0, order, 0).astype(np.uint8)
    return np.ascontiguousarray(j.reshape(M, sets, 4).transpose(1, 0, 2)), np.ascontiguousarray(w.reshape(M, sets, 4).transpose(1, 0, 2))


def _fixture_rig(sparse):
    """tests/golden/rig.npz's T-pose mesh with the skin of the dense or the 4-sparse template, and the stand-in motion as quaternions"""
    from scipy.spatial.transform import Rotation

    from avatarclip_amd import drive
    g = dict(np.load(GOLD))
    a = RS.sparse_template_arrays() if sparse else S.template_arrays()
    nearest = torch.from_numpy(g["nearest"])
    W = a["lbs_weights"].numpy()[g["nearest"]]
    tpose = (g["vertices"] / 100).astype(np.float32)
    joints = torch.einsum("bik,ji->bjk", a["v_template"][None], a["J_regressor"])[0].numpy()
    rot = drive.read_pose_my(S.motion())
    q = Rotation.from_matrix(rot.reshape(-1, 3, 3).double().numpy()).as_quat().reshape(-1, 24, 4)
    q = (q * np.where(q[..., 3:] < 0, -1.0, 1.0)).astype(np.float32)
    return g, a, nearest, W, tpose, joints, rot, q


def test_glb_round_trip_and_container_layout(tmp_path):
    from avatarclip_amd import rig
    g, a, nearest, W, tpose, joints, rot, q = _fixture_rig(sparse=False)
    js, ws = _numpy_sets(W)
    assert js.shape[0] == 6
    colors = rig.colors_to_u8(g["colors"])
    times = (np.arange(len(q)) / 60.0).astype(np.float32)
    path = rig.write_glb(str(tmp_path / "a.glb"), tpose, g["triangles"], colors, js, ws, joints, times=times, rotations=q, name="fixture")
    data = open(path, "rb").read()
    # ---- the container, by the glTF 2.0 specification's binary layout
    magic, version, length = struct.unpack_from("<4sII", data, 0)
    assert magic == b"glTF" and version == 2 and length == len(data) and length % 4 == 0
    jlen, jtype = struct.unpack_from("<I4s", data, 12)
    assert jtype == b"JSON" and jlen % 4 == 0
    text = data[20:20 + jlen]
    doc = json.loads(text)
    assert text[:1] == b"{" and text.rstrip(b" ")[-1:] == b"}" and set(text[len(text.rstrip(b" ")):]) <= {0x20}
    blen, btype = struct.unpack_from("<I4s", data, 20 + jlen)
    assert btype == b"BIN\0" and blen % 4 == 0 and 20 + jlen + 8 + blen == len(data)
    assert len(doc["buffers"]) == 1 and blen - 3 <= doc["buffers"][0]["byteLength"] <= blen
    assert all(v["byteOffset"] % 4 == 0 and v["byteOffset"] + v["byteLength"] <= blen for v in doc["bufferViews"])
    assert doc["asset"]["version"] == "2.0" and doc["scenes"][0]["nodes"] == [24, 0] and doc["skins"][0]["skeleton"] == 0
    pos = doc["accessors"][doc["meshes"][0]["primitives"][0]["attributes"]["POSITION"]]
    assert pos["min"] == tpose.min(0).tolist() and pos["max"] == tpose.max(0).tolist()
    # ---- every array, exactly
    r = rig.read_glb(path)
    at = r["attributes"]
    assert np.array_equal(at["POSITION"], tpose) and at["POSITION"].dtype == np.float32
    assert np.array_equal(at["COLOR_0"], colors) and at["COLOR_0"].dtype == np.uint8
    assert np.array_equal(r["indices"], g["triangles"].reshape(-1)) and r["indices"].dtype == np.uint32
    rj, rw = RS.glb_sets(r)
    assert np.array_equal(rj, js) and np.array_equal(rw, ws) and rj.dtype == np.uint8 and rw.dtype == np.float32
    ibm = r["skin"]["inverse_bind_matrices"]
    assert np.array_equal(ibm[:, :3, 3], -joints) and np.array_equal(ibm[:, :3, :3], np.broadcast_to(np.eye(3, dtype=np.float32), (24, 3, 3)))
    assert np.array_equal(ibm[:, 3], np.broadcast_to(np.float32([0, 0, 0, 1]), (24, 4)))
    assert [n["name"] for n in r["nodes"]] == list(rig.JOINT_NAMES) + ["fixture"]
    assert [(-1 if n["parent"] is None else n["parent"]) for n in r["nodes"][:24]] == list(rig.SMPL_PARENTS)
    assert r["nodes"][24]["parent"] is None and r["nodes"][24]["mesh"] == 0 and r["nodes"][24]["skin"] == 0
    j64 = joints.astype(np.float64)
    for i, n in enumerate(r["nodes"][:24]):
        p = rig.SMPL_PARENTS[i]
        assert np.array_equal(n["translation"], j64[i] - (j64[p] if p >= 0 else 0)) and n["rotation"].tolist() == [0, 0, 0, 1]
    assert len(r["animation"]) == 24
    for i, ch in enumerate(r["animation"]):
        assert ch["node"] == i and ch["path"] == "rotation" and ch["interpolation"] == "LINEAR"
        assert np.array_equal(ch["times"], times) and np.array_equal(ch["values"], q[:, i])
    # ---- the strict reader refuses a damaged container
    for bad in (data[:-1], data[:8] + struct.pack("<I", len(data) + 4) + data[12:], data[:4] + struct.pack("<I", 1) + data[8:],
                data[:20 + jlen - 1] + b"\0" + data[20 + jlen:]):
        (tmp_path / "bad.glb").write_bytes(bad)
        with pytest.raises(ValueError):
            rig.read_glb(str(tmp_path / "bad.glb"))


@pytest.mark.parametrize("sparse", [False, True])
def test_file_side_evaluator_reproduces_drive_skinning(tmp_path, sparse):
    """the .glb played back in fp64 against drive's skinning, T = (W A)[nearest] applied to the T-pose vertices, on the CPU in torch"""
    from avatarclip_amd import drive, rig
    g, a, nearest, W, tpose, joints, rot, q = _fixture_rig(sparse)
    js, ws = _numpy_sets(W)
    assert js.shape[0] == (1 if sparse else 6) and np.array_equal(RS.dense_weights(js, ws), W)
    path = rig.write_glb(str(tmp_path / "a.glb"), tpose, g["triangles"], None, js, ws, joints, times=np.arange(len(q), dtype=np.float32) / 60, rotations=q)
    frames = RS.glb_frames(rig.read_glb(path))
    T = drive.template_transforms(a, rot)[:, nearest]                                    # [T, M, 4, 4]
    homo = torch.cat([torch.from_numpy(tpose), torch.ones(len(tpose), 1)], 1)
    ref = torch.matmul(T, homo[None, :, :, None])[:, :, :3, 0].numpy()
    err = np.abs(frames - ref).max()
    print("worst |file playback - drive skinning| = %.3e m" % err)
    assert frames.shape == ref.shape == (8, len(tpose), 3) and err < 1e-5
    # without an animation the file rests in the T pose
    rest = rig.write_glb(str(tmp_path / "rest.glb"), tpose, g["triangles"], None, js, ws, joints)
    assert np.abs(RS.glb_frames(rig.read_glb(rest))[0] - tpose).max() < 1e-6


def test_joint_tables_are_the_references():
    from avatarclip_amd import rig
    g = np.load(GOLD)
    assert list(rig.JOINT_NAMES) == [str(n) for n in g["joint_names"]]
    assert list(rig.SMPL_PARENTS) == g["parents"].tolist() == S.SMPL_PARENTS
    assert g["blend_weights"].shape == (24, g["vertices"].shape[0]) and g["joints"].shape == (24, 3)
