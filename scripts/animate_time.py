"""Device time of one iteration of AvatarAnimate's CLIP-guided optimisers with the renderer gradient (AnimateContext(renderer_gradient=True)):
PoseOptimizer (5 views, one batched render + ViT forward / backward of 5 images) and MotionOptimizer with its CLIP term (2 frames at azimuth 150,
the graph-replayed B = 2 ViT path), on the real template mesh (tests/golden/smpl_views.npz: 13 776 faces, 27 552 with fill_back), S = 256 on a
512^2 super-sampled grid, seeded stand-in CLIP weights and SMPL-shaped arrays (tests/test_animate.py's).  Device events around K iterations
after warm-up; run it under `rocprofv3 --kernel-trace --stats -- python scripts/animate_time.py` for the per-kernel split.

    python scripts/animate_time.py [--iters K] [--posing torch|hip]     GPU (the posing: smpl_lbs.lbs, or smpl_lbs.pose_hip_grad on HIP)
    python scripts/animate_time.py --posing_alone [--posing torch|hip]  GPU: posed_vertices forward + backward on their own, bs = 1 and 2
    python scripts/animate_time.py --count_visits         CPU: pixels the restated backward visits for one view (tests/nr_grad_restatement.py)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _ctx(dev, posing="torch"):
    from avatarclip_amd import animate as A
    from avatarclip_amd import clip_vit as V
    from oracle import clip_vit_oracle as C
    from oracle.animate_standins import StandInVPoser, text_feature_of
    from tests.test_animate import _synthetic_smpl
    perceptor = V.ClipVisionB32(C.random_state_dict(0), dev) if dev.type == "cuda" else None
    return A.AnimateContext(perceptor, text_feature_of, _synthetic_smpl(dev), StandInVPoser(0).to(dev), device=dev, renderer_gradient=True, posing=posing)


def _time(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.time()
    s.record()
    fn(iters)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters, (time.time() - t0) * 1e3 / iters


def main_gpu(iters, posing="torch"):
    from avatarclip_amd import animate as A
    from tests.test_animate import _gold
    dev = torch.device("cuda")
    ctx = _ctx(dev, posing)
    tf = ctx.get_text_feature("a rendered 3d man is arguing")
    out = {"posing": posing, "faces": int(len(ctx.smpl["faces"])), "image_size": ctx.image_size}
    pose = A.PoseOptimizer(ctx, num_iteration=3)
    np.random.seed(0)
    torch.manual_seed(0)
    pose.get_pose(tf)                                               # warm-up: code objects, allocator, the eager ViT's shapes

    def run_pose(k):
        pose.num_iteration = k
        pose.get_pose(tf)
    out["pose_optimizer_ms_per_iteration"], out["pose_optimizer_host_ms"] = _time(run_pose, iters)
    mo = A.MotionOptimizer(ctx, num_iteration=3, clip_coef=0.001)        # the reference's defaults: 60 frames, width 256, 4 layers
    poses = _gold()["mi_poses"][:, :63].to(dev)
    mo.get_motion("a rendered 3d man is arguing", poses)               # warm-up incl. the B = 2 graph capture

    def run_motion(k):
        mo.num_iteration = k
        mo.get_motion("a rendered 3d man is arguing", poses)
    out["motion_optimizer_ms_per_iteration"], out["motion_optimizer_host_ms"] = _time(run_motion, iters)
    out["iters"] = iters
    print(json.dumps(out))


def main_posing_alone(iters, posing):
    """AnimateContext.posed_vertices and its backward on their own, at the batch sizes of the two optimisers: a pose leaf on the device,
    a fixed upstream gradient, device events and the host clock around `iters` forward + backward pairs after three warm-up pairs"""
    dev = torch.device("cuda")
    ctx = _ctx(dev, posing)
    out = {"posing": posing, "vertices": int(ctx.smpl["v_template"].shape[0]), "iters": iters}
    for bs in (1, 2):
        pose = (torch.randn(bs, 63, generator=torch.Generator().manual_seed(bs)) * 0.3).to(dev).requires_grad_(True)
        g = torch.randn(bs, out["vertices"], 3, generator=torch.Generator().manual_seed(7)).to(dev)

        def run(k):
            for _ in range(k):
                pose.grad = None
                ctx.posed_vertices(pose).backward(g)
        run(3)
        out["bs%d_device_ms" % bs], out["bs%d_host_ms" % bs] = _time(run, iters)
    print(json.dumps(out))


def count_visits():
    """the restatement on one PoseOptimizer view (T pose, azimuth 150, elevation 0) with a dense random upstream gradient"""
    from avatarclip_amd import mesh_render as M
    from avatarclip_amd.shapegen_render import get_points_from_angles
    from tests import nr_grad_restatement as R
    ctx = _ctx(torch.device("cpu"))
    v = ctx.posed_vertices(torch.zeros(1, 63))[0] @ torch.tensor(M.ROT_MAT)
    eye = get_points_from_angles(2.0, 0.0, 150).astype(np.float32)
    cam = torch.from_numpy(M.camera_frame(eye, (-eye / np.linalg.norm(eye)).astype(np.float32)))[None]
    ndc = M.project(v[None], cam, float(np.tan(np.deg2rad(30.0))))[0].numpy()
    f = np.asarray(ctx.smpl["faces"], np.int64)
    f2 = np.concatenate([f, f[:, ::-1]])
    S = ctx.image_size
    t0 = time.time()
    fidx = R.rasterize_index(ndc, f2, 2 * S)
    light = M.face_light(v, torch.from_numpy(f)).numpy()
    g = np.random.RandomState(0).randn(S, S).astype(np.float32)
    count = {}
    R.pseudo_grad(ndc, f2, light, fidx, R.G_map(g), count=count)
    front = sum(not R.is_back(ndc[t]) for t in f2)
    print(json.dumps({"image": 2 * S, "faces": len(f2), "front_facing": int(front), "covered_pixels": int((fidx >= 0).sum()),
                      "out_run_visits": count["out"], "in_run_visits": count["in"], "cpu_seconds": round(time.time() - t0, 1)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--count_visits", action="store_true")
    ap.add_argument("--posing", choices=("torch", "hip"), default="torch", help="AnimateContext's posing: smpl_lbs.lbs or smpl_lbs.pose_hip_grad")
    ap.add_argument("--posing_alone", action="store_true", help="time posed_vertices forward + backward on their own instead of the optimisers")
    a = ap.parse_args()
    count_visits() if a.count_visits else (main_posing_alone(a.iters, a.posing) if a.posing_alone else main_gpu(a.iters, a.posing))
