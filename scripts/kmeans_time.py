"""Time k-means on the device (profiles/codebook.md):

  * milliseconds per Lloyd iteration (assign + sort + update + the changed count) at N = 2^21, K = 4096, D = 32, and of the two launches alone;
  * the same iteration as a chunked torch.cdist + argmin + index_add_ on the same device -- the baseline, not the code under test;
  * the seconds of a full pose-build at K = 4096 with the seeded stand-ins (tests/drive_standins' SMPL-shaped arrays, StandInVPoser,
    runner.clip_vit_random_state_dict), image_size 64.

    python scripts/kmeans_time.py [--n 2097152] [--k 4096] [--d 32] [--iters 5] [--pose_build] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _ms(fn, iters):
    fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def torch_iteration(x, c, prev, chunk=1 << 16):
    """the baseline: nearest centre by torch.cdist in chunks of points, means by index_add_ (float atomics: not reproducible bit for bit)"""
    a = torch.empty(x.shape[0], device=x.device, dtype=torch.int64)
    for i in range(0, x.shape[0], chunk):
        a[i:i + chunk] = torch.cdist(x[i:i + chunk], c).argmin(1)
    changed = int((a != prev).sum().item())
    s = torch.zeros_like(c).index_add_(0, a, x)
    n = torch.zeros(c.shape[0], device=x.device).index_add_(0, a, torch.ones(x.shape[0], device=x.device))
    return torch.where(n[:, None] > 0, s / n[:, None].clamp(min=1), c), a, changed


def main(argv=None):
    from avatarclip_amd import kmeans as KM
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 21)
    ap.add_argument("--k", type=int, default=4096)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--pose_build", action="store_true")
    ap.add_argument("--pose_build_k", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    x = torch.randn(args.n, args.d, generator=torch.Generator().manual_seed(0)).to(dev)
    c0 = KM.initial_centres(x, args.k, 0)
    res = {"N": args.n, "K": args.k, "D": args.d, "device": torch.cuda.get_device_name(0)}

    a, _ = KM.assign(x, c0)
    prev = torch.full_like(a, -1)

    def hip_iteration():
        c = c0.clone()
        a, d = KM.assign(x, c)
        d.sum(dtype=torch.float64)
        int((a != prev).sum().item())
        KM.update(x, a, c)

    res["assign_ms"] = _ms(lambda: KM.assign(x, c0), args.iters)
    res["update_with_sort_ms"] = _ms(lambda: KM.update(x, a, c0.clone()), args.iters)
    res["hip_iteration_ms"] = _ms(hip_iteration, args.iters)
    prev64 = prev.to(torch.int64)
    res["torch_iteration_ms"] = _ms(lambda: torch_iteration(x, c0, prev64), args.iters)
    # distances = N K (D subtractions + D fused multiply-adds): 3 D flop each
    res["assign_tflops"] = 3.0 * args.d * args.n * args.k / (res["assign_ms"] * 1e-3) / 1e12
    ct, at, _ = torch_iteration(x, c0, prev64)
    res["assignments_differing_from_torch"] = int((at.to(torch.int32) != a).sum())
    if args.pose_build:
        import tempfile
        from avatarclip_amd import codebook as CB
        from avatarclip_amd.runner import clip_vit_random_state_dict
        from oracle.animate_standins import StandInVPoser
        from tests import drive_standins as S
        z = np.load(os.path.join(ROOT, "tests", "golden", "smpl_views.npz"))
        v_template, faces = z["mesh_v"].astype(np.float32), z["mesh_f"].astype(np.int32)
        arr = S.template_arrays(K=len(v_template))
        with tempfile.TemporaryDirectory() as d:
            p = lambda n: os.path.join(d, n)
            np.savez(p("smpl.npz"), v_template=v_template, posedirs=arr["posedirs"].numpy(), J_regressor=arr["J_regressor"].numpy(),
                     parents=arr["parents"].numpy(), lbs_weights=arr["lbs_weights"].numpy(), faces=faces)
            n_poses = 16 * args.pose_build_k
            np.save(p("poses.npy"), (np.random.RandomState(0).randn(n_poses, 63) * 0.3).astype(np.float32))
            torch.save(clip_vit_random_state_dict(0), p("clip.pth"))
            torch.cuda.synchronize()
            t0 = time.time()
            CB.main(["pose-build", "--poses", p("poses.npy"), "--smpl", p("smpl.npz"), "--vposer", "unused", "--clip_weights", p("clip.pth"), "--k",
                     str(args.pose_build_k), "--image_size", "64", "--out", p("pose.pth")], vposer=StandInVPoser(0))
            torch.cuda.synchronize()
            res["pose_build_seconds"] = time.time() - t0
            side = CB.read_sidecar(p("pose.pth"))
            res["pose_build"] = {"K": side["K"], "n_poses": side["n_poses"], "kmeans_iterations": side["kmeans_iterations"], "image_size": 64}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
