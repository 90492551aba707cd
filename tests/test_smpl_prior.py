"""the SMPL prior (posed mesh -> silhouette / grey render) without smplx / neural_renderer.
  CPU: linear blend skinning against an independent numpy restatement on a synthetic skeleton; the neural_renderer
       restatement's conventions against the reference-produced renders (framing / orientation / grey range -- the shipped
       renders show a posed body, so this is NOT a pin of the rasteriser, see oracle/nr_oracle.py);
  GPU: the HIP rasteriser (avc_rasterize_faces behind smpl_prior.MeshPrior) against the restatement on the SMPL template."""
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "smpl_views.npz")


def test_lbs_matches_numpy_restatement_on_a_synthetic_skeleton():
    from avatarclip_amd import smpl_lbs
    from oracle import lbs_oracle as LO
    rng = np.random.RandomState(0)
    V, J = 200, 6
    parents = np.array([-1, 0, 1, 1, 3, 0])
    v = rng.randn(V, 3) * 0.3
    Jreg = np.abs(rng.rand(J, V)); Jreg /= Jreg.sum(1, keepdims=True)
    W = np.abs(rng.rand(V, J)) ** 3; W /= W.sum(1, keepdims=True)
    posedirs = rng.randn((J - 1) * 9, V * 3) * 0.01
    pose = rng.randn(J, 3) * 0.6
    rot = np.stack([LO.rodrigues(p) for p in pose])
    ref_v, ref_j = LO.lbs(v, rot, posedirs, Jreg, parents, W)
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    rot_t = smpl_lbs.batch_rodrigues(t(pose))
    assert np.abs(rot_t.numpy() - rot).max() < 1e-9
    out_v, out_j = smpl_lbs.lbs(t(v)[None], rot_t[None], t(posedirs), t(Jreg), torch.from_numpy(parents), t(W))
    assert np.abs(out_v[0].numpy() - ref_v).max() < 1e-9 and np.abs(out_j[0].numpy() - ref_j).max() < 1e-9
    # the T pose of main.py:307-309 (root turned by pi/2 about x) followed by rot_mat is a pure translation of the template
    pose0 = np.zeros((J, 3)); pose0[0, 0] = np.pi / 2
    r0 = smpl_lbs.batch_rodrigues(t(pose0))
    v0, _ = smpl_lbs.lbs(t(v)[None], r0[None], t(posedirs) * 0, t(Jreg), torch.from_numpy(parents), t(W))
    from oracle.nr_oracle import ROT_MAT
    d = v0[0].numpy() @ ROT_MAT - v
    assert np.abs(d - d[0]).max() < 1e-7      # (the 1e-8 epsilon inside batch_rodrigues)


def test_renderer_restatement_conventions_against_reference_renders():
    from oracle import nr_oracle as NR
    z = np.load(GOLD)
    V, Fc = z["mesh_v"].astype(np.float64), z["mesh_f"]
    ims, poses = z["tpose_images"], z["tpose_poses"]
    assert sorted(np.unique(ims))[1] in (31, 32) and ims.max() >= 240      # 1/4 coverage x ambient 0.5 ... ambient + directional
    t = np.array([0.0, 0.288, 0.211])     # pelvis offset of the posed body (fitted on the legs; the SMPL joint regressor is not available)
    for k in (3, 57):                     # camera in front of / behind the body, elevation 0
        eye = poses[k][:3, 3]
        img = NR.render(V + t, Fc, eye, -eye / np.linalg.norm(eye))
        a, b = img > 0, ims[k] > 0
        ra, rb = np.nonzero(a.any(1))[0], np.nonzero(b.any(1))[0]
        assert abs(ra.min() - rb.min()) <= 12 and abs(ra.max() - rb.max()) <= 12         # head top / feet rows: same framing, upright
        ca, cb = np.nonzero(a.any(0))[0], np.nonzero(b.any(0))[0]
        assert abs(0.5 * (ca.min() + ca.max()) - 0.5 * (cb.min() + cb.max())) <= 4       # centred alike
        band = slice(int(0.5 * (cb.min() + cb.max())) - 10, int(0.5 * (cb.min() + cb.max())) + 11)   # torso / head column band
        inter, union = (a[:, band] & b[:, band]).sum(), (a[:, band] | b[:, band]).sum()
        assert inter / union > 0.75     # pose-independent part only roughly (different arm / leg pose, fitted pelvis offset)
        both = a & b
        assert abs(float(img[both].mean() * 255) - float(ims[k][both].mean())) < 25     # same light model (grey level of the body)


def _prior_by_torch_ops(prior, eye, at):
    """MeshPrior.__call__ stated with torch ops around the face-list rasteriser: look + perspective, the reference's patch (behind the camera
    -> 0), the gather to faces [F,9], avc_rasterize_faces at 2 S, avg_pool2d, the x flip and the three equal channels"""
    from avatarclip_amd import h2d, lib as L
    from avatarclip_amd.smpl_prior import camera_frame
    dev = prior.v_world.device
    eye, at = np.asarray(eye, np.float64), np.asarray(at, np.float64)
    cam = h2d.upload(camera_frame(eye, (at - eye) / np.linalg.norm(at - eye)), dev)
    v = (prior.v_world - cam[:3]) @ cam[3:].reshape(3, 3).t()
    ndc = torch.stack([v[:, 0] / v[:, 2] / prior.width, v[:, 1] / v[:, 2] / prior.width, v[:, 2]], dim=1)   # perspective.py
    ndc = torch.where(v[:, 2:3] <= 0, torch.zeros_like(ndc), ndc)     # ... with the reference's patch (README.md:126-134)
    fz = ndc[prior.faces2].reshape(-1, 9).contiguous()
    S2 = 2 * prior.image_size                                    # anti_aliasing=True
    img = torch.empty(S2, S2, device=dev, dtype=torch.float32)
    lib = L.load()
    zbuf = torch.full((lib.avc_rasterize_scratch_bytes(fz.shape[0], S2),), 255, dtype=torch.uint8, device=dev)
    L.check(lib.avc_rasterize_faces(L.ptr(fz), L.ptr(prior.light2), fz.shape[0], S2, prior.near, prior.far, L.ptr(img), L.ptr(zbuf), L.stream()),
            "avc_rasterize_faces")
    grey = torch.nn.functional.avg_pool2d(img[None, None], kernel_size=2, stride=2)[0, 0]
    return grey.flip(1)[..., None].repeat(1, 1, 3)


@gpu
def test_hip_rasteriser_matches_restatement():
    import time
    from avatarclip_amd.smpl_prior import MeshPrior
    from oracle import nr_oracle as NR
    z = np.load(GOLD)
    V, Fc = z["mesh_v"], z["mesh_f"]
    prior = MeshPrior(V, Fc, device="cuda")
    cams = [(np.array([0.2, 0.3, 1.6]), np.array([0.0, -0.1, 0.05])), (np.array([-1.3, -0.4, -0.9]), np.array([0.05, 0.1, 0.0])),
            (np.array([0.05, 1.5, 0.6]), np.array([0.0, 0.2, 0.0])),
            # close-ups: faces whose boxes hold thousands of sub-pixels (the tile-parallel pass of the rasteriser), the second one
            # from so near that part of the body is beside / behind the camera
            (np.array([0.05, 0.35, 0.55]), np.array([0.0, 0.3, 0.0])), (np.array([0.1, 0.0, 0.22]), np.array([0.0, 0.1, 0.0]))]
    for eye, at in cams:
        # the four-launch form (projection + pooling inside the library) against the torch ops around avc_rasterize_faces: same image up to
        # the few sub-pixels whose edge test sits within an ulp of the projection's rounding
        unf = _prior_by_torch_ops(prior, eye, at).cpu().numpy()
        out = prior(eye, at).cpu().numpy()
        nd = (np.abs(out[..., 0] - unf[..., 0]) > 1e-6).sum()
        assert nd <= 24 and np.abs(out - unf).max() <= 0.51, (nd, np.abs(out - unf).max())     # (13 of 65 536 pixels on the nearest close-up, 0 on the far views)
        assert np.array_equal(prior.render_grey(eye, (at - eye) / np.linalg.norm(at - eye)).cpu().numpy()[:, ::-1], out[..., 0])
        ref = NR.render_one_batch(V.astype(np.float64), Fc, eye, at).astype(np.float32)
        assert out.shape == (256, 256, 3) and np.array_equal(out[..., 0], out[..., 1])
        mism = ((out[..., 0] > 0) != (ref[..., 0] > 0)).sum()
        inter, union = ((out[..., 0] > 0) & (ref[..., 0] > 0)).sum(), ((out[..., 0] > 0) | (ref[..., 0] > 0)).sum()
        d = np.abs(out - ref)
        print("eye", eye, "coverage", (ref[..., 0] > 0).mean(), "mask mismatches", mism, "IoU", inter / union, "max |d|", d.max(), "mean |d|", d.mean())
        assert inter / union > 0.999 and d.mean() < 1e-4 and (d > 0.26).sum() <= 4    # a flipped edge sub-sample moves a pixel by <= 1/4
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(20):
        prior(cams[0][0], cams[0][1])
    torch.cuda.synchronize()
    print("MeshPrior render: %.3f ms per 256x256 view (13776 faces, 2x super-sampling)" % ((time.time() - t0) / 20 * 1e3))
    # as the Runner's prior: mask / colour target of train_clip
    import bench
    from avatarclip_amd.runner import Runner
    conf = bench.make_conf(64, 32, small=True)
    r = Runner(None, mode="train_clip", conf=conf, device=torch.device("cuda"))
    r.init_clip()
    r.init_smpl(prior)
    loss = r.train_clip_iteration(1)
    assert torch.isfinite(loss)


def test_shapegen_camera_list_equals_the_shipped_datasets():
    """ShapeGen/render.py:17-29,48-56: the 108 camera-to-world matrices of `render_for_nerf`, against the transforms_train.json files
    the reference ships (packed in tests/golden/smpl_views.npz): the stand-pose set exactly, the T-pose set with its camera
    distance of 2.0 (same rotations)."""
    from avatarclip_amd import shapegen_render as SR
    z = np.load(GOLD)
    T = np.stack([t for _, t in SR.nerf_cameras()])
    assert T.shape == (108, 4, 4) and np.abs(T - z["stand_poses"]).max() < 1e-12
    assert abs(float(z["stand_camera_angle_x"]) - SR.CAMERA_ANGLE_X) < 1e-15
    T2 = np.stack([t for _, t in SR.nerf_cameras(camera_distance=2.0)])
    assert np.abs(T2 - z["tpose_poses"]).max() < 1e-12
    eye0 = SR.get_points_from_angles(2.2, -60, 0)
    assert np.allclose(eye0, [0.0, 2.2 * np.sin(np.deg2rad(-60)), -2.2 * np.cos(np.deg2rad(-60))])


@gpu
def test_shapegen_dataset_writer_feeds_runner_train(tmp_path):
    """row f-4 / BASELINE config 5's ShapeGen -> AppearanceGen link: the HIP rasteriser writes the 108-view dataset of
    ShapeGen/render.py for the SMPL template (T pose after rot_mat, pelvis offset fitted as in the CPU test above); its views agree
    with the shipped neural_renderer renders of data/zero_beta_tpose_render in framing, silhouette (torso band) and grey level, and
    Runner.train (main.py:180-256) trains on the written folder."""
    import json
    from PIL import Image
    import bench
    from avatarclip_amd import shapegen_render as SR
    from avatarclip_amd.runner import Runner
    z = np.load(GOLD)
    V, Fc = z["mesh_v"].astype(np.float64), z["mesh_f"]
    t = np.array([0.0, 0.288, 0.211])
    out = str(tmp_path / "render")
    # render_for_nerf multiplies the (posed) vertices by rot_mat (render.py:39-43); the T-posed body of the shipped set is the
    # template + t AFTER that rotation, so the writer gets the template turned the other way
    from avatarclip_amd.smpl_prior import ROT_MAT
    u8, transforms = SR.write_nerf_dataset(out, ((V + t) @ np.asarray(ROT_MAT).T).astype(np.float32), Fc, camera_distance=2.0)
    meta = json.load(open(os.path.join(out, "transforms_train.json")))
    assert len(meta["frames"]) == 108 and abs(meta["camera_angle_x"] - np.pi / 3) < 1e-12
    assert np.abs(np.asarray([f["transform_matrix"] for f in meta["frames"]]) - z["tpose_poses"]).max() < 1e-9
    im0 = np.asarray(Image.open(os.path.join(out, "img", "0003.png")))
    assert im0.shape == (256, 256, 3) and (im0[..., 0] == im0[..., 1]).all() and np.array_equal(im0[..., 0], u8[3])
    ims = z["tpose_images"]
    for k, tol_rows, tol_iou, tol_c in ((3, 12, 0.75, 6), (57, 12, 0.75, 6), (27, 20, 0.3, 20), (87, 20, 0.3, 20)):
        # elevation 0: azimuth 0 (front), 180 (back), 80 and 280 (the sides: the pelvis offset t was fitted on the front view, its depth
        # component is off by ~0.1, which moves the side views sideways by ~13 pixels: they only pin orientation and framing)
        a, b = u8[k] > 0, ims[k] > 0
        ra, rb = np.nonzero(a.any(1))[0], np.nonzero(b.any(1))[0]
        assert abs(ra.min() - rb.min()) <= tol_rows and abs(ra.max() - rb.max()) <= tol_rows, k
        cb = np.nonzero(b.any(0))[0]
        ca = np.nonzero(a.any(0))[0]
        assert abs(0.5 * (ca.min() + ca.max()) - 0.5 * (cb.min() + cb.max())) <= tol_c, k
        mid = int(0.5 * (cb.min() + cb.max()))
        band = slice(mid - 10, mid + 11)
        iou = (a[:, band] & b[:, band]).sum() / max((a[:, band] | b[:, band]).sum(), 1)
        both = a & b
        print("view", k, "torso-band IoU %.3f" % iou, "grey", float(u8[k][both].mean()), float(ims[k][both].mean()))
        assert iou > tol_iou and abs(float(u8[k][both].mean()) - float(ims[k][both].mean())) < 25, k
    # AppearanceGen's NeuS-init stage on the written folder
    conf = bench.make_conf(256, 32, small=True)
    conf.put("general.base_exp_dir", str(tmp_path / "exp"))
    conf.put("dataset.data_dir", out)
    conf.put("train.batch_size", 1024)
    conf.put("train.warm_up_end", 0)
    conf.put("train.end_iter", 30)
    conf.put("model.rendering_network.extra_color", False)
    conf.put("model.neus_renderer.extra_color", False)
    r = Runner(None, mode="train", conf=conf, device=torch.device("cuda"))
    assert r.dataset.n_images == 108
    losses = []
    image_perm = r.get_image_perm()
    r.update_learning_rate()
    for _ in range(30):
        batch = r.dataset.gen_random_rays_at(image_perm[r.iter_step % len(image_perm)], r.batch_size)
        losses.append(r.train_iteration(batch).item())
        r.update_learning_rate()
    assert np.isfinite(losses).all() and np.mean(losses[-5:]) < np.mean(losses[:5])
