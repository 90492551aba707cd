"""tests/golden/drive.npz by RUNNING THE REFERENCE'S OWN drive.py functions (build container only: needs the reference checkout).
    python scripts/gen_golden_drive.py                                                   TEST INFRASTRUCTURE ONLY.

AvatarGen/AppearanceGen/drive.py imports open3d and smplx at module level (both absent here), so it cannot be imported; its functions
batch_rodrigues, vertices2joints, blend_shapes, batch_rigid_transform, transform_mat, cleanup_mesh, load_template_smpl, find_nearest_ind,
inv_lbs, lbs, read_pose_my and write_pc2 are extracted with `ast` (oracle/gen_golden_animate.extract) and run unmodified, in
generate_animation's order (:317-361), on the CPU.  Two stand-ins replace the absent packages:
  * O3DMesh: the open3d TriangleMesh that cleanup_mesh touches -- `vertices` (float64), compute_adjacency_list / adjacency_list (the set of
    triangle-edge neighbours of every vertex) and remove_vertices_by_index (the surviving vertices, their colours and the triangles whose three
    corners survive, in their original order, indices remapped);
  * SMPLLayer: smplx's SMPLLayer forward (betas, body_pose / global_orient as rotation matrices -> vertices) through avatarclip_amd.smpl_lbs.lbs,
    with the model attributes inv_lbs / lbs read (v_template, shapedirs = 0, J_regressor, parents, lbs_weights).
So this row is UNPINNED against open3d / smplx themselves.  Inputs: tests/drive_standins.py (seeded) and the reference's shipped
stand_pose.npy (72 floats, recorded as data)."""
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from avatarclip_amd import smpl_lbs  # noqa: E402
from oracle import gen_golden_animate as G  # noqa: E402
from oracle import ref_loader  # noqa: E402
from tests import drive_standins as S  # noqa: E402

DRIVE = os.path.join(ref_loader.REF_AG, "drive.py")
STAND_POSE = os.path.join(ref_loader.REF_ROOT, "AvatarGen", "ShapeGen", "output", "stand_pose.npy")
FUNCS = ("batch_rodrigues", "vertices2joints", "blend_shapes", "batch_rigid_transform", "transform_mat", "cleanup_mesh", "load_template_smpl",
         "find_nearest_ind", "inv_lbs", "lbs", "read_pose_my", "write_pc2")


class O3DMesh:
    def __init__(self, vertices, triangles, colors):
        self.vertices = np.asarray(vertices, np.float64)
        self.triangles = np.asarray(triangles, np.int64)
        self.vertex_colors = np.asarray(colors)

    def compute_adjacency_list(self):
        adj = [set() for _ in range(len(self.vertices))]
        for a, b, c in self.triangles:
            adj[a].update((b, c))
            adj[b].update((a, c))
            adj[c].update((a, b))
        self.adjacency_list = adj

    def remove_vertices_by_index(self, idx):
        keep = np.ones(len(self.vertices), bool)
        keep[np.asarray(idx, np.int64)] = False
        remap = np.cumsum(keep) - 1
        self.vertices, self.vertex_colors = self.vertices[keep], self.vertex_colors[keep]
        self.triangles = remap[self.triangles[keep[self.triangles].all(1)]]


class SMPLLayer:
    def __init__(self, arrays):
        self.v_template, self.posedirs, self.J_regressor = arrays["v_template"], arrays["posedirs"], arrays["J_regressor"]
        self.parents, self.lbs_weights = arrays["parents"], arrays["lbs_weights"]
        self.shapedirs = torch.zeros(self.v_template.shape[0], 3, 10)

    def __call__(self, betas, body_pose, global_orient):
        full = torch.cat([global_orient.reshape(-1, 1, 3, 3), body_pose.reshape(-1, 23, 3, 3)], dim=1)
        v, _ = smpl_lbs.lbs(self.v_template[None], full, self.posedirs, self.J_regressor, self.parents, self.lbs_weights)
        return {"vertices": v}


def main():
    ns = {"torch": torch, "np": np, "F": F, "Tensor": torch.Tensor, "struct": __import__("struct"), "tqdm": lambda it: it}
    G.extract(DRIVE, ns, functions=FUNCS)
    rec = {}
    # ---- the islands: the avatar (drive.py:317-325) and the equal-size case
    v, t, c = S.avatar_mesh()
    rec.update(in_v=v, in_t=t, in_c=c)
    mesh = O3DMesh(v, t, c)
    mesh.vertices = np.matmul(np.asarray(mesh.vertices), np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], dtype=np.float32))
    mesh = ns["cleanup_mesh"](mesh)
    rec.update(clean_v=np.asarray(mesh.vertices).astype(np.float32), clean_t=mesh.triangles.astype(np.int32), clean_c=mesh.vertex_colors)
    tv, tt, tc = S.tie_mesh()
    tie = ns["cleanup_mesh"](O3DMesh(tv, tt, tc))
    rec.update(tie_in_v=tv, tie_in_t=tt, tie_in_c=tc, tie_v=tie.vertices.astype(np.float32), tie_t=tie.triangles.astype(np.int32), tie_c=tie.vertex_colors)
    # ---- template, nearest vertex, unposing (:334-341)
    arrays = S.template_arrays()
    smpl_model = SMPLLayer(arrays)
    template_object, pose_rot, beta = ns["load_template_smpl"](smpl_model, STAND_POSE)
    nearest_ind = ns["find_nearest_ind"](np.asarray(mesh.vertices), template_object)
    smpl_blend_weights = smpl_model.lbs_weights
    mesh_blend_weights = torch.gather(smpl_blend_weights, 0, torch.from_numpy(nearest_ind).unsqueeze(-1).repeat(1, smpl_blend_weights.shape[-1]))
    tpose_vertices = ns["inv_lbs"](smpl_model, np.asarray(mesh.vertices), mesh_blend_weights, pose_rot, beta)
    rec.update(stand_pose=np.load(STAND_POSE).astype(np.float32), template_v=template_object["vertices"][0].numpy(), nearest=nearest_ind.astype(np.int64),
               tpose=tpose_vertices.numpy())
    # the per-template transforms of inv_lbs' statements (:243-248) with the template's own weights, and their inverses
    J = ns["vertices2joints"](smpl_model.J_regressor, smpl_model.v_template + ns["blend_shapes"](beta, smpl_model.shapedirs))
    _, A = ns["batch_rigid_transform"](pose_rot, J, smpl_model.parents)
    T = torch.matmul(smpl_blend_weights.unsqueeze(0), A.view(1, 24, 16)).view(1, -1, 4, 4)
    rec.update(stand_A=A[0].numpy(), stand_T_inv=torch.inverse(T)[0].numpy())
    # ---- the motion, re-posing, the point cache (:350-361)
    mo = S.motion()
    rec["motion"] = mo
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "action.npy"), mo)
        pose_list = ns["read_pose_my"](os.path.join(d, "action.npy"))
        frame_A = [ns["batch_rigid_transform"](p, J, smpl_model.parents)[1][0].numpy() for p in pose_list]
        vertices_list = [ns["lbs"](smpl_model, tpose_vertices, mesh_blend_weights, p, beta) for p in pose_list]
        ns["write_pc2"](os.path.join(d, "motion.pc2"), vertices_list)
        with open(os.path.join(d, "motion.pc2"), "rb") as f:
            pc2 = f.read()
    rec.update(frame_rot=torch.cat(pose_list).numpy(), frame_A=np.stack(frame_A), pc2=np.frombuffer(pc2, np.uint8).copy())
    path = os.path.join(G.GOLD, "drive.npz")
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), {k: getattr(x, "shape", x) for k, x in rec.items()})
    n = len(rec["nearest"])
    ties = sum(1 for a, b in S.DUPLICATES if (rec["nearest"] == a).any() or (rec["nearest"] == b).any())
    print("mesh", v.shape[0], "->", n, "vertices; template pairs with an exact tie in use:", ties)


if __name__ == "__main__":
    main()
