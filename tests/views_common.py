"""Shared pieces of the train.views_per_iter tests: V camera views per optimisation step over W ranks, rank r
rendering the views r, r + W, ...  The Runner under test is the one tests/dp_common.build_runner builds (small nets, train.seed = 0;
on the CPU the oracle renderer and perceptor), with conf keys put on top; the reference is dp_common.single_process_accumulation's
recipe -- the views one after the other, streams seeded B + j, gradients averaged -- restated here so that it also records the cameras
and takes the extra conf keys."""
import os
import random

import numpy as np
import torch

from tests import dp_common


def build_runner(device, res, spp, use_oracle_kernels, extra=None):
    """dp_common.build_runner with `extra` conf keys (e.g. {"train.views_per_iter": 4}) put on bench.make_conf's conf"""
    import bench
    make = bench.make_conf

    def make_with_extra(*a, **k):
        conf = make(*a, **k)
        for key, v in (extra or {}).items():
            conf.put(key, v)
        return conf
    bench.make_conf = make_with_extra
    try:
        return dp_common.build_runner(device, res, spp, use_oracle_kernels)
    finally:
        bench.make_conf = make


def _device(device_kind):
    return torch.device("cuda", 0) if device_kind == "cuda" else torch.device("cpu")


def accumulate_views(device_kind, n_views, res, spp, base_seed=0, iter_i=0, extra=None):
    """dp_common.single_process_accumulation, view by view: -> dict(w0, grads = the mean of the single-view gradients, losses, eyes,
    ats, rays).  View 0 draws from the stream the constructor leaves, view j > 0 from streams freshly seeded with base_seed + j."""
    device = _device(device_kind)
    r = build_runner(device, res, spp, device_kind != "cuda", extra)
    assert r.views_per_iter == 1, "the reference renders one view per clip_loss: pass no views_per_iter here"
    w0 = [p.detach().cpu().clone() for p in r.params_to_train]
    acc, losses, eyes, ats, rays = None, [], [], [], []
    for j in range(n_views):
        if j > 0:
            s = base_seed + j
            np.random.seed(s); random.seed(s); torch.manual_seed(s)
            if device_kind == "cuda":
                torch.cuda.manual_seed(s)
        loss, _ = r.clip_loss(iter_i)
        r.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        g = [torch.zeros_like(p).cpu() if p.grad is None else p.grad.detach().cpu().clone() for p in r.params_to_train]
        acc = g if acc is None else [a + b for a, b in zip(acc, g)]
        losses.append(float(loss.detach()))
        eyes.append(np.asarray(r.last_view.eye).copy()); ats.append(np.asarray(r.last_view.at).copy())
        rays.append(int(r.last_view.rays_o.shape[0]))
    return dict(w0=w0, grads=[a / n_views for a in acc], losses=losses, eyes=eyes, ats=ats, rays=rays)


def _snapshot(r, loss):
    bucket = r.grad_bucket
    return dict(eyes=[np.asarray(v.eye).copy() for v in r.last_views], ats=[np.asarray(v.at).copy() for v in r.last_views],
                rays=[int(v.rays_o.shape[0]) for v in r.last_views], rays_stat=int(r.last_stats["rays"]),
                losses=[float(l) for l in r.last_view_losses], loss=float(loss), iter_step=r.iter_step,
                last_view_is_last=r.last_view is r.last_views[-1],
                grads=[p.grad.detach().cpu().clone() for p in r.params_to_train],
                params=[p.detach().cpu().clone() for p in r.params_to_train],
                bucket_is_grad=bucket is not None and all(p.grad.data_ptr() == g.data_ptr() for p, g in zip(r.params_to_train, bucket.views)))


def run_steps(r, steps, iter_i=0):
    """`steps` optimisation steps of one Runner -> one snapshot per step (all steps with the same iter_i: the cameras then differ by the
    streams alone)"""
    out = []
    for _ in range(steps):
        loss = r.train_clip_iteration(iter_i)
        out.append(_snapshot(r, loss))
        r.update_learning_rate()
    return out


def single_process(device_kind, n_views, res, spp, steps=1, iter_i=0, extra=None):
    """one process, no process group, views_per_iter = n_views (None: the key is absent) -> (w0, snapshots, runner)"""
    keys = dict(extra or {})
    if n_views is not None:
        keys["train.views_per_iter"] = n_views
    r = build_runner(_device(device_kind), res, spp, device_kind != "cuda", keys)
    w0 = [p.detach().cpu().clone() for p in r.params_to_train]
    return w0, run_steps(r, steps, iter_i), r


def worker(rank, world, port, out_dir, device_kind, res, spp, n_views, steps, extra=None):
    """rank `rank` of `world` over gloo (every rank on device 0 when device_kind == "cuda"; the hardware-queue setting is the
    machine's): `steps` steps of views_per_iter = n_views, dist.all_reduce counted per step -> <out_dir>/rank<k>.pt"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      AVC_DIST_BACKEND="gloo")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    from avatarclip_amd import parallel
    parallel.init_from_env(backend="gloo")
    r = build_runner(_device(device_kind), res, spp, device_kind != "cuda", dict(extra or {}, **{"train.views_per_iter": n_views}))
    assert r.world == world and r.rank == rank and r.views_per_iter == n_views and r.grad_bucket is not None
    w0 = [p.detach().cpu().clone() for p in r.params_to_train]
    calls = []
    all_reduce = dist.all_reduce

    def counted(t, *a, **k):
        calls.append((t.data_ptr(), t.numel()))
        return all_reduce(t, *a, **k)
    dist.all_reduce = counted
    snaps, per_step = [], []
    try:
        for _ in range(steps):
            del calls[:]
            loss = r.train_clip_iteration(0)
            per_step.append(list(calls))
            snaps.append(_snapshot(r, loss))
            r.update_learning_rate()
    finally:
        dist.all_reduce = all_reduce
    flat = r.grad_bucket.flat
    torch.save(dict(w0=w0, steps=snaps, data_seed=r.data_seed, base_seed=r.base_seed,
                    all_reduces=[len(c) for c in per_step],
                    all_reduce_on_flat=all(c == [(flat.data_ptr(), flat.numel())] for c in per_step)),
               os.path.join(out_dir, "rank%d.pt" % rank))
    parallel.barrier()
    dist.destroy_process_group()


def spawn_ranks(world, out_dir, device_kind, res, spp, n_views, steps, timeout, extra=None):
    """start the `world` ranks and join them under `timeout` seconds (a rank that has not ended by then is killed and the test fails)
    -> the per-rank results"""
    import time
    import torch.multiprocessing as mp
    ctx = mp.spawn(worker, args=(world, dp_common.free_port(), out_dir, device_kind, res, spp, n_views, steps, extra), nprocs=world, join=False)
    deadline = time.monotonic() + timeout
    try:
        while not ctx.join(timeout=max(0.0, min(5.0, deadline - time.monotonic()))):
            if time.monotonic() >= deadline:
                raise TimeoutError("the %d ranks did not end within %d s" % (world, timeout))
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    return [torch.load(os.path.join(out_dir, "rank%d.pt" % k), weights_only=False) for k in range(world)]


def assert_grads_close(want, got, rel):
    """the data-parallel tests' formula: per tensor ||g1 - g2|| <= rel * (||g1|| + 1e-3 * gn), gn = the norm of all of them together"""
    gn = torch.cat([g.reshape(-1) for g in want]).norm()
    assert len(want) == len(got)
    for i, (g1, g2) in enumerate(zip(want, got)):
        err, bound = (g1 - g2).norm(), rel * (g1.norm() + 1e-3 * gn)
        assert err <= bound, (i, float(err), float(bound))
