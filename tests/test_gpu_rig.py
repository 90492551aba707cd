"""The rig step on the device (csrc/avc_rig.hip through avatarclip_amd/rig.py): the vertex clustering bit for bit against its numpy
restatement (tests/rig_standins.restated_simplify), the skin against the reference's own functions (tests/golden/rig.npz,
scripts/gen_golden_rig.py), the packed influences, the .glb played back against drive, production sizes, and the chain from
Runner.validate_mesh's PLY."""
import os

import numpy as np
import pytest
import torch

from tests import drive_standins as S
from tests import rig_standins as RS

gpu = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rig.npz")
DEV = "cuda"


def _arrays(sparse=False, dev=DEV):
    a = RS.sparse_template_arrays() if sparse else S.template_arrays()
    return {k: (v.to(dev) if k != "parents" else v) for k, v in a.items()}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_simplify(v, t, c, divisor):
    from avatarclip_amd import rig
    rv, rt, rc, rmap = RS.restated_simplify(v, t, c, divisor)
    gv, gt, gc, gmap = rig.simplify_mesh(v, t, c, divisor, return_map=True)
    assert gv.dtype == torch.float32 and gt.dtype == torch.int32 and gc.dtype == torch.float32
    assert np.array_equal(gmap.cpu().numpy(), rmap)                                 # the cells in first-occurrence order
    assert _same_bits(gv.cpu().numpy(), rv) and _same_bits(gc.cpu().numpy(), rc) and _same_bits(gt.cpu().numpy(), rt)
    again = rig.simplify_mesh(v, t, c, divisor, return_map=True)
    assert all(torch.equal(x, y) for x, y in zip((gv, gt, gc, gmap), again))
    return rv, rt


@gpu
def test_simplify_hand_made_mesh_bit_for_bit():
    from avatarclip_amd import rig
    rv, rt = _check_simplify(*RS.hand_mesh(), RS.HAND_DIVISOR)
    assert rv.shape == (7, 3) and rt.tolist() == [[0, 1, 2], [0, 2, 1], [1, 2, 3], [0, 1, 4], [1, 6, 3]]
    v, t, c = RS.hand_mesh()
    gv, gt, gc = rig.simplify_mesh(v, np.zeros((0, 3), np.int32), None, RS.HAND_DIVISOR)       # no triangles, no colours
    assert _same_bits(gv.cpu().numpy(), rv) and gt.shape == (0, 3) and gc is None
    gv, gt, gc = rig.simplify_mesh(v, t, c[:, :3].copy(), RS.HAND_DIVISOR)                      # RGB without alpha
    assert _same_bits(gt.cpu().numpy(), rt)
    with pytest.raises(ValueError):
        rig.simplify_mesh(v, np.array([[0, 1, 10]], np.int32), c, RS.HAND_DIVISOR)
    with pytest.raises(ValueError, match="1022"):
        rig.simplify_mesh(v, t, c, 1023)


@gpu
@pytest.mark.parametrize("res,divisor,n_in,n_out,f_in,f_out", [(48, 24, 1585, 455, 3156, 900), (96, 32, 6243, 865, 12472, 1720)])
def test_simplify_avatar_mesh_bit_for_bit(res, divisor, n_in, n_out, f_in, f_out):
    v, t, c = S.avatar_mesh(res)
    rv, rt = _check_simplify(v, t, c, divisor)
    assert (len(v), len(rv), len(t), len(rt)) == (n_in, n_out, f_in, f_out)
    assert len(rv) < len(v) // 2 and len(rt) < len(t)                               # it really merges and really drops


@gpu
def test_skin_matches_the_reference_functions():
    """export_fbx.py:55-88 on the fixture's simplified mesh: nearest and blend_weights exact, T-pose vertices and joints within the drive
    fixture's 1e-5 m (x 100: the reference's centimetres); the worst error is printed."""
    from avatarclip_amd import drive, rig
    g = np.load(GOLD)
    a = _arrays()
    rot_vertices = torch.from_numpy(drive.rotate_vertices(g["simp_v"])).to(DEV)
    template, pose_rot = drive.load_template_smpl(a, g["stand_pose"])
    e_t = np.abs(template.cpu().numpy() - g["template_v"]).max()
    print("worst |template - reference| = %.3e m" % e_t)          # evaluated on the host CPU: to rounding, not to the bit, across machines
    assert e_t < 1e-5
    nearest = drive.find_nearest_ind(rot_vertices, torch.from_numpy(g["template_v"]).to(DEV))   # as tests/test_gpu_drive.py: the recorded template
    assert np.array_equal(nearest.cpu().numpy(), g["nearest"])
    _, _, blend = rig.skin_pack(a["lbs_weights"], nearest)
    assert blend.shape == (24, len(g["simp_v"])) and _same_bits(blend.cpu().numpy(), g["blend_weights"])
    tpose = drive.inv_lbs(a, rot_vertices, nearest, pose_rot).cpu().numpy() * 100
    joints = torch.einsum("bik,ji->bjk", a["v_template"][None], a["J_regressor"])[0].cpu().numpy() * 100
    e_v, e_j = np.abs(tpose - g["vertices"]).max(), np.abs(joints - g["joints"]).max()
    print("worst |T-pose vertex - reference| = %.3e cm, worst |T-pose joint - reference| = %.3e cm" % (e_v, e_j))
    assert e_v < 1e-5 * 100 and e_j < 1e-5 * 100


def _sorted_as_specified(joints, weights):
    """per vertex: weights descending, equal weights by joint ascending, zeros (joint 0) at the end"""
    j = joints.transpose(1, 0, 2).reshape(joints.shape[1], -1).astype(np.int64)
    w = weights.transpose(1, 0, 2).reshape(weights.shape[1], -1)
    ok = (w[:, :-1] > w[:, 1:]) | ((w[:, :-1] == w[:, 1:]) & ((j[:, :-1] < j[:, 1:]) | (w[:, 1:] == 0)))
    return bool(ok.all()) and bool((j[w == 0] == 0).all())


@gpu
@pytest.mark.parametrize("sparse,sets", [(False, 6), (True, 1)])
def test_skin_packing(sparse, sets):
    from avatarclip_amd import rig
    g = np.load(GOLD)
    a = _arrays(sparse)
    nearest = torch.from_numpy(g["nearest"]).to(DEV).to(torch.int32)
    W = a["lbs_weights"].cpu().numpy()[g["nearest"]]
    joints, weights, blend = rig.skin_pack(a["lbs_weights"], nearest)
    j, w = joints.cpu().numpy(), weights.cpu().numpy()
    assert j.shape == w.shape == (sets, len(W), 4) and j.dtype == np.uint8 and w.dtype == np.float32
    assert _same_bits(RS.dense_weights(j, w), W) and _same_bits(blend.cpu().numpy(), np.ascontiguousarray(W.T))
    assert _sorted_as_specified(j, w)
    # --max_influences 4: the four largest, renormalised in float32
    j4, w4, blend4 = rig.skin_pack(a["lbs_weights"], nearest, max_influences=4)
    j4, w4 = j4.cpu().numpy(), w4.cpu().numpy()
    assert j4.shape == (1, len(W), 4) and np.array_equal(j4[0], j[0]) and _sorted_as_specified(j4, w4)
    rows = w4[0].astype(np.float64).sum(1)
    print("max_influences 4: worst |row sum - 1| = %.3e" % np.abs(rows - 1).max())
    assert np.abs(rows - 1).max() <= 4 * np.finfo(np.float32).eps
    s = w[0][:, 0] + w[0][:, 1] + w[0][:, 2] + w[0][:, 3]                            # float32, left to right: the kernel's sum
    assert _same_bits(w4[0], w[0] / s[:, None]) and _same_bits(blend4.cpu().numpy(), np.ascontiguousarray(W.T))
    # equal weights: the lower joint first; a vertex with one influence
    tie = torch.zeros(3, 24, device=DEV)
    tie[0, [20, 3, 11]] = torch.tensor([0.25, 0.5, 0.25], device=DEV)
    tie[1, 7] = 1.0
    tie[2, [0, 23]] = 0.5
    jt, wt, _ = rig.skin_pack(tie, torch.tensor([2, 0, 1, 0], device=DEV, dtype=torch.int32))
    assert jt.cpu().tolist() == [[[0, 23, 0, 0], [3, 11, 20, 0], [7, 0, 0, 0], [3, 11, 20, 0]]]
    assert wt.cpu().tolist() == [[[0.5, 0.5, 0, 0], [0.5, 0.25, 0.25, 0], [1, 0, 0, 0], [0.5, 0.25, 0.25, 0]]]
    with pytest.raises(ValueError):
        rig.skin_pack(tie, torch.tensor([3], device=DEV, dtype=torch.int32))


def _write_inputs(d, sparse=False):
    from avatarclip_amd import mesh
    g = np.load(GOLD)
    v, t, c = S.avatar_mesh(int(g["mesh_res"]))
    mesh.write_ply(os.path.join(d, "avatar.ply"), v, t, c)
    np.save(os.path.join(d, "action.npy"), S.motion())
    np.save(os.path.join(d, "stand_pose.npy"), g["stand_pose"])
    a = RS.sparse_template_arrays() if sparse else S.template_arrays()
    np.savez(os.path.join(d, "smpl.npz"), v_template=a["v_template"].numpy(), posedirs=a["posedirs"].numpy(), J_regressor=a["J_regressor"].numpy(),
             parents=a["parents"].numpy(), lbs_weights=a["lbs_weights"].numpy(), faces=np.zeros((1, 3), np.int32))
    return g


@gpu
@pytest.mark.parametrize("sparse", [False, True])
def test_cli_playback_equals_drive(tmp_path, sparse):
    """python -m avatarclip_amd.rig --motion on the fixture; the file played back by the fp64 evaluator against drive.lbs on the device"""
    from avatarclip_amd import drive, rig
    d = str(tmp_path)
    g = _write_inputs(d, sparse)
    rig.main(["--mesh", os.path.join(d, "avatar.ply"), "--smpl", os.path.join(d, "smpl.npz"), "--pose_npy", os.path.join(d, "stand_pose.npy"),
              "--out_dir", os.path.join(d, "out"), "--name", "fixture", "--motion", os.path.join(d, "action.npy"),
              "--voxel_divisor", str(int(g["voxel_divisor"]))])
    r = rig.read_glb(os.path.join(d, "out", "fixture.glb"))
    z = np.load(os.path.join(d, "out", "fixture_rig.npz"))
    M = len(g["simp_v"])
    assert z["vertices"].shape == (M, 3) and z["blend_weights"].shape == (24, M) and z["joints"].shape == (24, 3) and str(z["name"]) == "fixture"
    assert np.array_equal(z["triangles"], g["triangles"]) and _same_bits(z["colors"], g["colors"])
    assert z["parents"].tolist() == list(rig.SMPL_PARENTS)
    # the skin of the file = the library's own steps on this machine (the template is evaluated on the host CPU, so it is the golden's
    # to rounding only: parity with the reference's recorded template is test_skin_matches_the_reference_functions' job)
    a = _arrays(sparse)
    template, pose_rot = drive.load_template_smpl(a, g["stand_pose"])
    rot_vertices = torch.from_numpy(drive.rotate_vertices(g["simp_v"])).to(DEV)
    expect = drive.find_nearest_ind(rot_vertices, template)
    assert np.array_equal(z["nearest"], expect.cpu().numpy())
    assert _same_bits(z["blend_weights"], np.ascontiguousarray(a["lbs_weights"].cpu().numpy()[z["nearest"]].T))
    assert _same_bits(z["vertices"], drive.inv_lbs(a, rot_vertices, expect, pose_rot).cpu().numpy() * 100)
    assert np.array_equal(r["attributes"]["POSITION"] * np.float32(100), z["vertices"]) and np.array_equal(r["indices"].reshape(-1, 3), g["triangles"])
    assert np.array_equal(r["attributes"]["COLOR_0"], rig.colors_to_u8(g["colors"]))
    assert sum(k.startswith("JOINTS_") for k in r["attributes"]) == (1 if sparse else 6)
    assert _same_bits(RS.dense_weights(*RS.glb_sets(r)), np.ascontiguousarray(z["blend_weights"].T))
    assert [n["name"] for n in r["nodes"][:24]] == list(rig.JOINT_NAMES)
    q = np.stack([ch["values"] for ch in r["animation"]], 1)                         # [T, 24, 4]
    assert q.shape == (8, 24, 4) and np.abs(np.linalg.norm(q.astype(np.float64), axis=-1) - 1).max() < 1e-6 and (q[..., 3] >= 0).all()
    assert np.array_equal(r["animation"][0]["times"], (np.arange(8) / 60.0).astype(np.float32))
    tpose = torch.from_numpy(r["attributes"]["POSITION"]).to(DEV)
    nearest = torch.from_numpy(z["nearest"]).to(DEV)
    ref = drive.lbs(a, tpose, nearest, drive.read_pose_my(os.path.join(d, "action.npy")).to(DEV)).cpu().numpy()
    err = np.abs(RS.glb_frames(r) - ref).max()
    print("worst |file playback - drive.lbs| = %.3e m" % err)
    assert err < 1e-5


@gpu
def test_rot_to_quat_branches_and_switches(tmp_path):
    from scipy.spatial.transform import Rotation

    from avatarclip_amd import rig
    # rotations by nearly pi about each axis and about a diagonal, tiny rotations, the identity: every branch of Shepperd's method
    rv = np.array([[3.1, 0, 0], [0, 3.1, 0], [0, 0, 3.1], [1.8, 1.8, 1.8], [1e-4, 0, 0], [0, 0, 0], [-2, 1, 0.5], [np.pi, 0, 0]])
    rv = np.concatenate([rv, np.random.RandomState(0).randn(500, 3) * 2])
    R = Rotation.from_rotvec(rv).as_matrix()
    q = rig.rot_to_quat(torch.from_numpy(R).float().to(DEV)).cpu().numpy().astype(np.float64)
    assert np.abs(np.linalg.norm(q, axis=1) - 1).max() < 1e-6 and (q[:, 3] >= 0).all()
    err = np.abs(Rotation.from_quat(q).as_matrix() - R).max()
    print("worst |R(q) - R| = %.3e" % err)
    assert err < 5e-7
    assert rig.rot_to_quat(torch.zeros(0, 24, 3, 3, device=DEV)).shape == (0, 24, 4)
    # --keep_root, --no_simplify, --scale, --cleanup, --max_influences
    d = str(tmp_path)
    g = _write_inputs(d)
    common = ["--mesh", os.path.join(d, "avatar.ply"), "--smpl", os.path.join(d, "smpl.npz"), "--pose_npy", os.path.join(d, "stand_pose.npy"),
              "--out_dir", os.path.join(d, "out"), "--motion", os.path.join(d, "action.npy")]
    rig.main(common + ["--name", "k", "--keep_root", "--no_simplify", "--scale", "100", "--max_influences", "4", "--fps", "30"])
    r = rig.read_glb(os.path.join(d, "out", "k.glb"))
    v, t, c = S.avatar_mesh(int(g["mesh_res"]))
    assert r["attributes"]["POSITION"].shape == v.shape and np.array_equal(r["indices"].reshape(-1, 3), t) and np.array_equal(r["attributes"]["COLOR_0"], c)
    assert sum(k.startswith("JOINTS_") for k in r["attributes"]) == 1 and np.array_equal(r["animation"][0]["times"], (np.arange(8) / 30.0).astype(np.float32))
    root = Rotation.from_quat(r["animation"][0]["values"].astype(np.float64)).as_matrix()
    assert np.abs(root - Rotation.from_rotvec(S.motion()[:, :3].astype(np.float64)).as_matrix()).max() < 1e-6
    z = np.load(os.path.join(d, "out", "k_rig.npz"))
    assert np.array_equal(r["attributes"]["POSITION"], z["vertices"]) and np.allclose(r["nodes"][0]["translation"], z["joints"][0])
    rig.main(common + ["--name", "c", "--cleanup", "--voxel_divisor", "24"])
    rc = rig.read_glb(os.path.join(d, "out", "c.glb"))
    from avatarclip_amd import drive
    cv, ct, cc = drive.cleanup_mesh(v, t, c)                                          # the blobs and the lone vertex are gone
    ev, et, _, _ = RS.restated_simplify(cv.cpu().numpy(), ct.cpu().numpy(), cc.cpu().numpy(), 24)
    assert len(cv) < len(v) and rc["attributes"]["POSITION"].shape == ev.shape and np.array_equal(rc["indices"].reshape(-1, 3), et)


def _device_body_sdf(n):
    """drive_standins.body_sdf on an n^3 grid over [-1, 1]^3, evaluated on the device"""
    ax = torch.linspace(-1, 1, n, device=DEV)
    p = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1)

    def capsule(a, b, r):
        a, b = torch.tensor(a, device=DEV, dtype=torch.float32), torch.tensor(b, device=DEV, dtype=torch.float32)
        ab = b - a
        t = (((p - a) * ab).sum(-1) / (ab * ab).sum()).clamp(0, 1)
        return (p - (a + t[..., None] * ab)).norm(dim=-1) - r

    def sphere(c, r):
        return (p - torch.tensor(c, device=DEV, dtype=torch.float32)).norm(dim=-1) - r

    d = capsule((0, -0.05, 0), (0, 0.35, 0), 0.17)
    for part in (lambda: sphere((0, 0.58, 0), 0.12), lambda: capsule((0, 0.38, 0), (0, 0.5, 0), 0.05),
                 lambda: capsule((-0.15, 0.33, 0), (-0.55, 0.1, 0), 0.05), lambda: capsule((0.15, 0.33, 0), (0.55, 0.1, 0), 0.05),
                 lambda: capsule((-0.09, -0.1, 0), (-0.14, -0.85, 0), 0.07), lambda: capsule((0.09, -0.1, 0), (0.14, -0.85, 0), 0.07),
                 lambda: sphere((0.7, 0.7, 0.3), 0.1), lambda: sphere((-0.7, -0.6, -0.4), 0.08)):
        d = torch.minimum(d, part())
    return d


@gpu
@pytest.mark.parametrize("n", [256, 512])
def test_simplify_at_production_size(n):
    """marching cubes of body_sdf on an n^3 grid (avc_mcubes), clustered at the reference's divisor 256, against the restatement"""
    from avatarclip_amd import mesh, rig
    v, t = mesh.marching_cubes(-_device_body_sdf(n), 0.0)
    v = v / (n - 1.0) * 2.0 - 1.0
    c = torch.cat([((v + 1) * 127.5).clamp(0, 255), torch.full((len(v), 1), 255.0, device=DEV)], 1).to(torch.uint8)
    gv, gt, gc, gmap = rig.simplify_mesh(v, t, c, 256, return_map=True)
    torch.cuda.synchronize()
    rv, rt, rc, rmap = RS.restated_simplify(v.cpu().numpy(), t.cpu().numpy(), c.cpu().numpy(), 256)
    print("grid %d^3: %d -> %d vertices, %d -> %d triangles" % (n, len(v), len(gv), len(t), len(gt)))
    assert len(gv) == len(rv) and np.array_equal(gmap.cpu().numpy(), rmap)           # vertex count, first-occurrence order
    assert _same_bits(gt.cpu().numpy(), rt) and _same_bits(gv.cpu().numpy(), rv) and _same_bits(gc.cpu().numpy(), rc)
    if n >= 512:
        assert len(gv) < len(v) // 2 and len(gt) < len(t)
    # invariants
    tt = gt.long()
    assert int(tt.min()) >= 0 and int(tt.max()) < len(gv)
    assert not ((tt[:, 0] == tt[:, 1]) | (tt[:, 1] == tt[:, 2]) | (tt[:, 0] == tt[:, 2])).any()
    assert bool((tt[:, 0] < tt[:, 1]).all() and (tt[:, 0] < tt[:, 2]).all())          # smallest index first
    assert len(torch.unique(tt, dim=0)) == len(tt)
    idx = gmap.long()[:, None].expand(-1, 3)
    lo = torch.full_like(gv, float("inf")).scatter_reduce(0, idx, v, "amin")
    hi = torch.full_like(gv, float("-inf")).scatter_reduce(0, idx, v, "amax")
    assert bool(torch.isfinite(lo).all()) and bool(((lo <= gv) & (gv <= hi)).all())   # every output vertex lies among its cell's inputs
    assert float(gc.min()) >= 0.0 and float(gc.max()) <= 1.0


@gpu
def test_validate_mesh_then_animate_then_rig(tmp_path):
    """Runner.validate_mesh(resolution=40) -> animate.run (as tests/test_gpu_drive.py chains them) -> rig: a .glb the strict reader accepts"""
    import bench
    from avatarclip_amd import animate as A
    from avatarclip_amd import mesh, rig
    from avatarclip_amd.conf import ConfigFactory
    from avatarclip_amd.runner import Runner
    from oracle.animate_standins import StandInVPoser, text_feature_of
    conf = bench.make_conf(64, 64, small=True)
    conf.put("general.base_exp_dir", str(tmp_path / "gen"))
    torch.manual_seed(0)
    ply = Runner(None, mode="validate_mesh", conf=conf, device=torch.device(DEV)).validate_mesh(world_space=True, resolution=40, threshold=0.0)
    z = np.load(os.path.join(os.path.dirname(GOLD), "animate.npz"))
    ctx = A.AnimateContext(None, text_feature_of, None, StandInVPoser(0), device="cpu")
    aconf = ConfigFactory.parse_string("general { base_exp_dir = %s\n mode = motion\n text = a rendered 3d man is arguing }\n"
                                       "pose_generator { type = VPoserCodebook }\nmotion_generator { type = MotionInterpolation }" % (tmp_path / "anim"))
    A.run(aconf, ctx, pose_assets=dict(codebook=torch.from_numpy(z["cb_codebook"]), codebook_embedding=torch.from_numpy(z["cb_embedding"])))
    _write_inputs(str(tmp_path))
    glb, npz = rig.build_rig(ply, str(tmp_path / "smpl.npz"), str(tmp_path / "stand_pose.npy"), str(tmp_path / "out"), name="General",
                             motion=str(tmp_path / "anim" / "motion.npy"), voxel_divisor=16)
    r = rig.read_glb(glb)
    pos = r["attributes"]["POSITION"]
    n_in = mesh.read_ply(ply)[0].shape[0]
    acc = r["json"]["accessors"][r["json"]["meshes"][0]["primitives"][0]["attributes"]["POSITION"]]
    assert 0 < len(pos) < n_in and np.isfinite(pos).all()
    assert (np.asarray(acc["min"]) <= pos).all() and (pos <= np.asarray(acc["max"])).all() and acc["min"] == pos.min(0).tolist()
    assert len(r["animation"]) == 24 and all(len(ch["times"]) == 60 for ch in r["animation"])
    assert np.load(npz)["blend_weights"].shape == (24, len(pos))
