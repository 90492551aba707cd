"""tests/golden/rig.npz by RUNNING THE REFERENCE'S OWN Avatar2FBX/utils/ply_utils.py functions (build container only: needs the reference
checkout).      python scripts/gen_golden_rig.py                                         TEST INFRASTRUCTURE ONLY.

ply_utils.py imports open3d and smplx at module level (both absent here), so it cannot be imported; its functions batch_rodrigues,
load_template_smpl, find_nearest_ind, inv_lbs, blend_shapes, vertices2joints, batch_rigid_transform and transform_mat are extracted with
`ast` (oracle/gen_golden_animate.extract) and run unmodified on the CPU.  The body of export_fbx.py is a script under `__main__`, so its
lines 55-88 are restated here around those functions, statement by statement.  Stand-ins for the absent packages:
  * the simplified mesh: open3d's simplify_vertex_clustering is not available, so the input of lines 55-88 is
    tests/rig_standins.restated_simplify of the seeded avatar mesh (UNPINNED against open3d itself);
  * SMPLLayer (scripts/gen_golden_drive.py's): smplx's forward through avatarclip_amd.smpl_lbs.lbs, with the attributes inv_lbs reads.
Also recorded, as data: the reference's shipped Avatar2FBX/poses/stand_pose.npy and the literal tables Child2Father / Num2Joints of
utils/fbx_utils.py (read with ast.literal_eval; that module imports the FBX SDK)."""
import ast
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from gen_golden_drive import SMPLLayer  # noqa: E402
from oracle import gen_golden_animate as G  # noqa: E402
from oracle import ref_loader  # noqa: E402
from tests import drive_standins as S  # noqa: E402
from tests import rig_standins as RS  # noqa: E402

A2F = os.path.join(ref_loader.REF_ROOT, "Avatar2FBX")
PLY_UTILS = os.path.join(A2F, "utils", "ply_utils.py")
FBX_UTILS = os.path.join(A2F, "utils", "fbx_utils.py")
STAND_POSE = os.path.join(A2F, "poses", "stand_pose.npy")
FUNCS = ("batch_rodrigues", "load_template_smpl", "find_nearest_ind", "inv_lbs", "blend_shapes", "vertices2joints", "batch_rigid_transform",
         "transform_mat")
MESH_RES, MESH_DIVISOR = 48, 24


def literal_tables(path, names):
    out = {}
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and getattr(node.targets[0], "id", None) in names:
            out[node.targets[0].id] = ast.literal_eval(node.value)
    return out


def main():
    ns = {"torch": torch, "np": np, "F": F, "Tensor": torch.Tensor}
    G.extract(PLY_UTILS, ns, functions=FUNCS)
    rec = {}
    v, t, c = S.avatar_mesh(MESH_RES)
    sv, st, sc, _ = RS.restated_simplify(v, t, c, MESH_DIVISOR)
    rec.update(simp_v=sv, simp_t=st, simp_c=sc, mesh_res=np.int32(MESH_RES), voxel_divisor=np.int32(MESH_DIVISOR))
    # ---- export_fbx.py:55-88 (ply_mesh.vertices = sv as open3d's float64, vertex_colors = sc)
    colors = np.asarray(sc.astype(np.float64)).astype(np.float32)
    ori_vertices = np.asarray(sv.astype(np.float64)).astype(np.float32)
    rot_vertices = np.matmul(ori_vertices, np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], dtype=np.float32))
    triangles = np.asarray(st)
    smpl_model = SMPLLayer(S.template_arrays())
    template_object, pose_rot, beta = ns["load_template_smpl"](smpl_model, STAND_POSE)
    nearest_ind = ns["find_nearest_ind"](rot_vertices, template_object)
    smpl_blend_weights = smpl_model.lbs_weights
    mesh_blend_weights = torch.gather(smpl_blend_weights, 0, torch.from_numpy(nearest_ind).unsqueeze(-1).repeat(1, smpl_blend_weights.shape[-1]))
    tpose_vertices = ns["inv_lbs"](smpl_model, rot_vertices, mesh_blend_weights, pose_rot, beta)
    v_shaped = smpl_model.v_template + ns["blend_shapes"](beta, smpl_model.shapedirs)
    tpose_joints = ns["vertices2joints"](smpl_model.J_regressor, v_shaped).squeeze().cpu().numpy()
    mesh_blend_weights = mesh_blend_weights.permute(1, 0).cpu().numpy()
    # ---- smpl_object (:102-109)
    rec.update(stand_pose=np.load(STAND_POSE).astype(np.float32), template_v=template_object["vertices"][0].numpy(), nearest=nearest_ind.astype(np.int64),
               vertices=(tpose_vertices * 100).numpy(), triangles=triangles, joints=tpose_joints * 100, blend_weights=mesh_blend_weights, colors=colors)
    tabs = literal_tables(FBX_UTILS, ("Child2Father", "Num2Joints"))
    rec["parents"] = np.array([-1] + [tabs["Child2Father"][i] for i in range(1, 24)], np.int32)
    rec["joint_names"] = np.array([tabs["Num2Joints"][i] for i in range(24)])
    path = os.path.join(G.GOLD, "rig.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), {k: getattr(x, "shape", x) for k, x in rec.items()})
    print("mesh", v.shape[0], "->", sv.shape[0], "vertices;", t.shape[0], "->", st.shape[0], "triangles")


if __name__ == "__main__":
    main()
