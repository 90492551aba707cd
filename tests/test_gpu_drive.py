"""The drive step on the device (csrc/avc_drive.hip through avatarclip_amd/drive.py): the nearest template vertex, the largest island and the
skinning gather against tests/golden/drive.npz (the reference's own drive.py functions, scripts/gen_golden_drive.py) and, at production size,
against restatements -- fp64 torch ops one per kernel for the nearest point, scipy's connected components for the islands."""
import os

import numpy as np
import pytest
import torch

from tests import drive_standins as S

gpu = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drive.npz")
DEV = "cuda"


def _gold():
    return dict(np.load(GOLD))


def _arrays(dev=DEV):
    return {k: (v.to(dev) if k != "parents" else v) for k, v in S.template_arrays().items()}


def _nearest_restated(q, t, chunk=8192):
    """find_nearest_ind in fp64 torch on the device: t - q, squares, (dx^2 + dy^2) + dz^2 as separate kernels (nothing fused), argmin = first
    minimum"""
    t64 = t.double()
    out = []
    for i in range(0, q.shape[0], chunk):
        q64 = q[i:i + chunk].double()
        dx = t64[None, :, 0] - q64[:, None, 0]
        dy = t64[None, :, 1] - q64[:, None, 1]
        dz = t64[None, :, 2] - q64[:, None, 2]
        s = torch.mul(dx, dx)
        s = torch.add(s, torch.mul(dy, dy))
        s = torch.add(s, torch.mul(dz, dz))
        out.append(torch.argmin(s, dim=1))
    return torch.cat(out)


@gpu
def test_nearest_point_is_the_reference_bit_for_bit():
    from avatarclip_amd import drive
    g = _gold()
    idx = drive.find_nearest_ind(torch.from_numpy(g["clean_v"]).to(DEV), torch.from_numpy(g["template_v"]).to(DEV))
    assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), g["nearest"])
    # the fixture's exact ties: a duplicated template vertex is never chosen over its first copy
    for a, b in S.DUPLICATES:
        assert not (g["nearest"] == max(a, b)).any()
    assert drive.find_nearest_ind(torch.zeros(0, 3, device=DEV), torch.zeros(5, 3, device=DEV)).shape == (0,)


@gpu
@pytest.mark.parametrize("M", [600_000, 2_600_000])
def test_nearest_point_at_production_size(M):
    from avatarclip_amd import drive
    g = torch.Generator().manual_seed(M)
    K = 6890
    t = torch.rand(K, 3, generator=g) * torch.tensor([0.8, 0.4, 1.8]) - torch.tensor([0.4, 0.2, 1.1])
    t[K // 2:K // 2 + 300] = t[100:400]                          # duplicated template points: exact ties
    t[7:20] = t[6000:6013]                                       # (the copy before the original, too)
    q = torch.rand(M, 3, generator=g) * torch.tensor([1.0, 0.6, 2.0]) - torch.tensor([0.5, 0.3, 1.2])
    q[:5000] = t[torch.randint(0, K, (5000,), generator=g)]     # queries ON template points (distance 0, ties where duplicated)
    q, t = q.to(DEV), t.to(DEV)
    got = drive.find_nearest_ind(q, t).long()
    ref = _nearest_restated(q, t)
    assert torch.equal(got, ref), int((got != ref).sum())
    assert not torch.isin(got, torch.arange(K // 2, K // 2 + 300, device=DEV)).any()
    assert not torch.isin(got, torch.arange(6000, 6013, device=DEV)).any()


def _canonical(labels):
    """component labels -> the smallest vertex index of each component"""
    labels = np.asarray(labels)
    first = np.full(labels.max() + 1, np.iinfo(np.int64).max)
    np.minimum.at(first, labels, np.arange(len(labels)))
    return first[labels]


@gpu
def test_cleanup_mesh_is_the_reference_on_the_fixture():
    from avatarclip_amd import drive
    g = _gold()
    v, t, c = drive.cleanup_mesh(torch.from_numpy(drive.rotate_vertices(g["in_v"])).to(DEV), g["in_t"], g["in_c"])
    assert np.array_equal(v.cpu().numpy(), g["clean_v"]) and np.array_equal(t.cpu().numpy(), g["clean_t"]) and np.array_equal(c.cpu().numpy(), g["clean_c"])
    v, t, c = drive.cleanup_mesh(g["tie_in_v"], g["tie_in_t"], g["tie_in_c"])
    assert np.array_equal(v.cpu().numpy(), g["tie_v"]) and np.array_equal(t.cpu().numpy(), g["tie_t"]) and np.array_equal(c.cpu().numpy(), g["tie_c"])


@gpu
def test_components_of_a_many_island_marching_cubes_mesh_match_scipy():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    from avatarclip_amd import drive, mesh
    n = 256
    g = torch.Generator().manual_seed(5)
    centres = torch.rand(400, 3, generator=g) * (n - 1)
    radii = torch.rand(400, generator=g) * 6 + 1.5
    ax = torch.arange(n, dtype=torch.float32, device=DEV)
    u = torch.full((n, n, n), -1e9, device=DEV)
    for c, r in zip(centres.to(DEV), radii.to(DEV)):
        d = ((ax[:, None, None] - c[0]) ** 2 + (ax[None, :, None] - c[1]) ** 2 + (ax[None, None, :] - c[2]) ** 2).sqrt()
        u = torch.maximum(u, r - d)
    v, t = mesh.marching_cubes(u, 0.0)
    nv = v.shape[0]
    label = drive.mesh_components(t, nv).cpu().numpy()
    tt = t.cpu().numpy().astype(np.int64)
    rows = np.concatenate([tt[:, 0], tt[:, 1], tt[:, 2]])
    cols = np.concatenate([tt[:, 1], tt[:, 2], tt[:, 0]])
    ncomp, lab = connected_components(coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(nv, nv)), directed=False)
    print("vertices", nv, "triangles", len(tt), "islands", ncomp)
    assert ncomp > 50 and np.array_equal(label, _canonical(lab))
    again = drive.mesh_components(t, nv).cpu().numpy()
    assert np.array_equal(label, again)
    v1, t1, _ = drive.cleanup_mesh(v, t)
    v2, t2, _ = drive.cleanup_mesh(v, t)
    assert torch.equal(v1, v2) and torch.equal(t1, t2)
    sizes = np.bincount(label, minlength=nv)
    keep = int(np.flatnonzero(sizes == sizes.max())[0])
    assert np.array_equal(v1.cpu().numpy(), v.cpu().numpy()[label == keep])


@gpu
def test_components_of_a_long_randomly_numbered_path():
    from avatarclip_amd import drive
    n = 1_000_000
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    tris = torch.stack([perm[:-1], perm[1:], perm[1:]], 1).to(torch.int32)      # degenerate triangles: one edge each, a path of length n - 1
    extra = 4                                                                    # + four isolated vertices
    label = drive.mesh_components(tris.to(DEV), n + extra).cpu()
    assert torch.equal(label[:n], torch.zeros(n, dtype=torch.int32)) and label[n:].tolist() == list(range(n, n + extra))
    v, t, _ = drive.cleanup_mesh(torch.rand(n + extra, 3, device=DEV), tris.to(DEV))
    assert v.shape == (n, 3) and torch.equal(t.cpu(), tris)


@gpu
def test_equal_islands_go_to_the_smallest_label():
    from avatarclip_amd import drive
    # five islands of three vertices each, the one holding vertex 0 listed last; vertex 15 joins it in the first case
    tris = np.array([[14, 9, 3], [2, 11, 5], [12, 6, 13], [10, 4, 8], [7, 0, 1]], np.int32)
    tris = np.concatenate([tris, [[7, 0, 15]]])       # island {0, 1, 7, 15} is the only 4-vertex one
    v = np.arange(16 * 3, dtype=np.float32).reshape(16, 3)
    vo, to, _ = drive.cleanup_mesh(v, tris)
    assert np.array_equal(vo.cpu().numpy(), v[[0, 1, 7, 15]])
    vo, to, _ = drive.cleanup_mesh(v, tris[:5])        # all five of size 3: the one with vertex 0
    assert np.array_equal(vo.cpu().numpy(), v[[0, 1, 7]]) and to.cpu().tolist() == [[2, 0, 1]]
    vo, to, _ = drive.cleanup_mesh(v, np.zeros((0, 3), np.int32))   # no triangles: every vertex alone, vertex 0 kept
    assert vo.shape == (1, 3) and to.shape == (0, 3)
    with pytest.raises(ValueError):
        drive.cleanup_mesh(v, np.array([[0, 1, 16]], np.int32))


@gpu
def test_skinning_matches_the_reference_and_batches_bit_for_bit():
    from avatarclip_amd import drive
    g = _gold()
    a = _arrays()
    v = torch.from_numpy(g["clean_v"]).to(DEV)
    nearest = torch.from_numpy(g["nearest"]).to(DEV).to(torch.int32)
    _, pose_rot = drive.load_template_smpl(a, g["stand_pose"])
    tpose = drive.inv_lbs(a, v, nearest, pose_rot)
    e_t = (tpose.cpu() - torch.from_numpy(g["tpose"])).abs().max().item()
    rot = torch.from_numpy(g["frame_rot"]).to(DEV)
    frames = drive.lbs(a, tpose, nearest, rot)
    ref = np.frombuffer(g["pc2"][32:].tobytes(), "<f4").reshape(8, -1, 3)
    e_f = np.abs(frames.cpu().numpy() - ref).max()
    print("worst |T-pose - reference| = %.3e, worst |frame - reference| = %.3e (metres)" % (e_t, e_f))
    assert e_t < 1e-5 and e_f < 1e-5
    xf = drive.rows3(drive.template_transforms(a, rot))
    for t in range(8):
        assert torch.equal(drive.skin_apply(xf[t:t + 1], nearest, tpose)[0], frames[t])
    # odd M: the tail lanes of the 4-vertex groups
    for m in (1, 2, 3, 5, 1413):
        assert torch.equal(drive.skin_apply(xf, nearest[:m], tpose[:m]), frames[:, :m])
    from avatarclip_amd import lib as L
    assert drive.skin_apply(xf[:0], nearest, tpose).shape == (0, v.shape[0], 3)
    assert drive.skin_apply(xf, nearest[:0], tpose[:0]).shape == (8, 0, 3)
    assert L.load().avc_skin_apply(None, None, None, 0, 700, 8, None, None) == 0
    assert L.load().avc_skin_apply(None, None, None, 5, 0, 8, None, None) != 0
    bad = nearest.clone()
    bad[7] = 700
    with pytest.raises(ValueError):
        drive.skin_apply(xf, bad, tpose)
    bad[7] = -1
    with pytest.raises(ValueError):
        drive.skin_apply(xf, bad, tpose)


def _write_inputs(d, g):
    from avatarclip_amd import mesh
    mesh.write_ply(os.path.join(d, "avatar.ply"), g["in_v"], g["in_t"], g["in_c"])
    np.save(os.path.join(d, "action.npy"), g["motion"])
    np.save(os.path.join(d, "stand_pose.npy"), g["stand_pose"])
    a = S.template_arrays()
    np.savez(os.path.join(d, "smpl.npz"), v_template=a["v_template"].numpy(), posedirs=a["posedirs"].numpy(), J_regressor=a["J_regressor"].numpy(),
             parents=a["parents"].numpy(), lbs_weights=a["lbs_weights"].numpy(), faces=np.zeros((1, 3), np.int32))


@gpu
def test_cli_reproduces_the_reference_outputs(tmp_path):
    from avatarclip_amd import drive, mesh
    g = _gold()
    d = str(tmp_path)
    _write_inputs(d, g)
    drive.main(["--mesh", os.path.join(d, "avatar.ply"), "--motion", os.path.join(d, "action.npy"), "--smpl", os.path.join(d, "smpl.npz"),
                "--pose_npy", os.path.join(d, "stand_pose.npy"), "--out_dir", os.path.join(d, "out"), "--name", "General"])
    v, t, c = mesh.read_ply(os.path.join(d, "out", "General_cleaned_apose.ply"))
    assert np.array_equal(v, g["clean_v"]) and np.array_equal(t, g["clean_t"]) and np.array_equal(c, g["clean_c"])
    with open(os.path.join(d, "out", "action.pc2"), "rb") as f:
        got = f.read()
    ref = g["pc2"].tobytes()
    assert len(got) == len(ref) and got[:32] == ref[:32]
    err = np.abs(np.frombuffer(got[32:], "<f4") - np.frombuffer(ref[32:], "<f4")).max()
    print("CLI: worst |frame - reference| = %.3e" % err)
    assert err < 1e-5


@gpu
def test_validate_mesh_then_animate_then_drive(tmp_path):
    """Runner.validate_mesh(resolution=40) -> animate.run (codebook retrieval + interpolation on stand-in blobs, as tests/test_animate.py)
    -> drive: a .pc2 with the cleaned mesh's vertex count and the motion's 60 frames"""
    import bench
    from avatarclip_amd import animate as A
    from avatarclip_amd import drive, mesh
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
    g = _gold()
    _write_inputs(str(tmp_path), g)
    ply_out, pc2 = drive.generate_animation(ply, str(tmp_path / "anim" / "motion.npy"), str(tmp_path / "smpl.npz"), str(tmp_path / "stand_pose.npy"),
                                            str(tmp_path / "out"))
    v, _, c = mesh.read_ply(ply_out)
    head, frames = drive.read_pc2(pc2)
    assert os.path.basename(pc2) == "motion.pc2" and c is not None
    assert head[0] == b"POINTCACHE2\0" and head[1:] == (1, v.shape[0], 0.0, 60.0, 60) and frames.shape == (60, v.shape[0], 3)
    assert 0 < v.shape[0] <= mesh.read_ply(ply)[0].shape[0] and np.isfinite(frames).all()
