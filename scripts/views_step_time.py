"""Time one optimisation step of train.views_per_iter = V views on ONE MI355X against V one-view iterations (the key absent: the
iteration as it was before the key existed -- tests/test_views_per_iter.py pins that path bit for bit), at the same size, in the same
process, the two alternating (profiles/views_per_iter.md).  Two sizes: the full frame at 224^2 x 64 spp, and the reference's default
silhouette mode at max_ray_num = 112 * 112.  Full-size networks.  Expected from the code: the V-view step is the V iterations less
V - 1 Adam steps and zero_grad calls.   python scripts/views_step_time.py [--views 8] [--rounds 5] [--steps 6] [--out result.json]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench


def window(runner, steps, first_iter):
    """`steps` train_clip iterations between two device synchronisations -> (seconds, views rendered, next iter_i)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(first_iter, first_iter + steps):
        runner.train_clip_iteration(i)
        runner.update_learning_rate()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, steps * runner.views_per_iter, first_iter + steps


def compare(name, res, spp, overrides, mesh_prior, V, rounds, steps, dev):
    one = bench.build_runner(res, spp, False, dev, overrides, mesh_prior=mesh_prior)
    many = bench.build_runner(res, spp, False, dev, dict(overrides, **{"train.views_per_iter": V}), mesh_prior=mesh_prior)
    assert one.views_per_iter == 1 and many.views_per_iter == V
    it_one = it_many = 0
    _, _, it_one = window(one, 2 * V, it_one)          # warm-up of every shape and of the CLIP graphs, both runners
    _, _, it_many = window(many, 2, it_many)
    ms_one, ms_many = [], []
    for _ in range(rounds):                              # alternating windows of the same number of views
        t, n, it_one = window(one, steps * V, it_one)
        ms_one.append(1e3 * t / n * V)
        t, n, it_many = window(many, steps, it_many)
        ms_many.append(1e3 * t / n * V)
    med = lambda v: sorted(v)[len(v) // 2]
    out = dict(config=name, views=V, rounds=rounds, views_per_window=steps * V,
               ms_V_one_view_iterations=med(ms_one), ms_one_V_view_step=med(ms_many), ratio=med(ms_many) / med(ms_one),
               all_ms_V_one_view_iterations=ms_one, all_ms_one_V_view_step=ms_many,
               rays_per_step=int(many.last_stats["rays"]))
    del one, many
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6, help="V-view steps per timed window (the one-view window runs V times as many iterations)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("views_step_time.py measures on an MI355X: no GPU here, nothing measured")
    dev = torch.device("cuda", 0)
    results = [
        compare("full frame 224^2 x 64 spp", 224, 64, {}, True, a.views, a.rounds, a.steps, dev),
        compare("silhouette mode, max_ray_num = 112 * 112, 512^2 dataset, 64 spp", 512, 64,
                {"train.use_silhouettes": True, "train.max_ray_num": 112 * 112, "train.use_bg_aug": True}, False, a.views, a.rounds, a.steps, dev),
    ]
    line = json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, results=results))
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
