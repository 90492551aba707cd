"""train.shard_view: time the one-view optimisation step on ONE rank and with the view's rays cut over N ranks,
one MI355X each, collectives over RCCL -- for whoever has a node; nothing here has been measured on more than one device
(profiles/shard_view.md).  Full-size networks, full frame.  Expected from the code, a derivation and not a measurement:
step(N) = (per-ray work of step(1)) / N + the CLIP stretch + the collectives.

    python scripts/shard_step_time.py --gpus 8 [--res 512] [--spp 64] [--steps 10] [--warmup 3] [--out result.json]
    python scripts/shard_step_time.py --plan [--res 512] [--spp 64]     one device: the operand-panel footprint per rank for N = 1, 2, 4, 8
"""
import argparse
import json
import os
import socket
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, res, spp, steps, warmup, out_path):
    """one rank: `warmup` untimed and `steps` timed sharded steps between barriers; rank 0 writes {ms_per_step, rays, loss}"""
    from avatarclip_amd import parallel
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
        os.environ.pop("AVC_DIST_BACKEND", None)
        parallel.init_from_env(backend="nccl", timeout=600)
    dev = torch.device("cuda", rank)
    torch.cuda.set_device(dev)
    runner = bench.build_runner(res, spp, False, dev, {"train.shard_view": True})
    assert runner.shard_view and runner.views_per_iter == 1 and (runner._shard_group is not None) == (world > 1)
    for i in range(warmup):
        runner.train_clip_iteration(i)
        runner.update_learning_rate()
    parallel.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(warmup, warmup + steps):
        runner.train_clip_iteration(i)
        runner.update_learning_rate()
    torch.cuda.synchronize()
    ms = parallel.max_over_ranks(1e3 * (time.perf_counter() - t0) / steps, dev)
    if rank == 0:
        part = getattr(runner.last_view, "part", None)
        with open(out_path, "w") as f:
            json.dump(dict(world=world, ms_per_step=ms, rays=int(runner.last_stats["rays"]), loss=float(runner.last_stats["loss"]),
                           rays_on_rank_0=int(part.rays_o.shape[0]) if part is not None else int(runner.last_stats["rays"])), f)
    parallel.barrier()
    if world > 1:
        torch.distributed.destroy_process_group()


def time_world(world, res, spp, steps, warmup):
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "rank0.json")
        mp.spawn(_rank, args=(world, _free_port(), res, spp, steps, warmup, path), nprocs=world, join=True)
        with open(path) as f:
            return json.load(f)


def panel_plan(res, spp, worlds=(1, 2, 4, 8)):
    """Engine.plan for the rays of one rank of N: -> per N the rays, rays per chunk and per slab, and the bytes of the F region (+ masks)
    of a chunk and of the G region of a slab"""
    dev = torch.device("cuda", 0)
    eng = bench.build_runner(res, spp, False, dev, None, mesh_prior=False).renderer.engine
    blk_f, blk_g = eng.fwd_tiles * 2048 + eng.mask_u16 * 2, eng.grad_tiles * 2048
    nb = lambda rays: (rays * spp + 31) // 32 + 1
    rows = []
    for n in worlds:
        R = -(-res * res // n)
        chunk, slab = eng.plan(R, spp)
        rows.append(dict(world=n, rays_per_rank=R, rays_per_chunk=chunk, rays_per_slab=slab, forward_runs=1 if chunk >= R else 2,
                         f_region_gib=nb(chunk) * blk_f / 2 ** 30, g_region_gib=nb(slab) * blk_g / 2 ** 30,
                         f_panels_of_all_rays_gib=nb(R) * blk_f / 2 ** 30))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=None)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plan", default=False, action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shard_step_time.py measures on MI355X devices: no GPU here, nothing measured")
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, res=a.res, spp=a.spp)
    if a.plan:
        out["panel_plan"] = panel_plan(a.res, a.spp)
    else:
        n = a.gpus if a.gpus is not None else torch.cuda.device_count()
        if n < 2 or torch.cuda.device_count() < n:
            raise SystemExit("shard_step_time.py: %d rank(s) asked for, %d device(s) here -- RCCL takes one device per rank, and the "
                             "comparison needs at least two" % (n, torch.cuda.device_count()))
        one, many = time_world(1, a.res, a.spp, a.steps, a.warmup), time_world(n, a.res, a.spp, a.steps, a.warmup)
        out.update(one_rank=one, n_ranks=many, speed_up=one["ms_per_step"] / many["ms_per_step"])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
