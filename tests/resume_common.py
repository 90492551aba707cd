"""Shared pieces of the resume tests (tests/test_resume_cpu.py, tests/test_gpu_resume.py): small `train` and `train_clip` Runners on either
device (bench.make_conf's small nets, seeded; on the CPU the oracle renderer and perceptor, as tests/dp_common.build_runner), a
four-image dataset in the reference's on-disk layout, and an instrumented run that records every step's host-side draws and can be
interrupted BETWEEN two steps by an exception raised from a wrapped Runner._after_step -- never a signal, never a killed process."""
import json
import os

import numpy as np
import torch

from tests import dp_common

RES, SPP, N_IMAGES = 16, 32, 4
TRAIN_STEPS, CLIP_STEPS = 12, 8
# the appearance stage as the issue sets it: silhouette rays, face prompt, untextured pass, background augmentation, two views per step
# on one rank, and validation on the checkpoint's steps (so that its draws lie between the checkpoint and the record).  train.seed = 3: the
# chess-board background takes squares of H // k pixels, k drawn from 10..19, which is 0 pixels on these 16 x 16 views for k >= 17
# (main.py:398 divides by it); seed 3 draws no such k in any run of these tests, bench.make_conf's seed 0 does in the second step.
CLIP_KEYS = {"train.seed": 3, "train.use_silhouettes": True, "train.use_face_prompt": True, "train.add_no_texture": True, "train.use_bg_aug": True,
             "train.views_per_iter": 2, "train.end_iter": CLIP_STEPS, "train.save_freq": 3, "train.val_freq": 3, "train.warm_up_end": 0}
TRAIN_KEYS = {"train.end_iter": TRAIN_STEPS, "train.batch_size": 128, "train.warm_up_end": 0}


class Interrupted(Exception):
    """the interruption: raised after a step's _after_step has returned"""


def device_of(kind):
    return torch.device("cuda", 0) if kind == "cuda" else torch.device("cpu")


def write_dataset(data_dir, res=RES, n=N_IMAGES):
    """n views of a disk in transforms_train.json + img/*.png (the layout of the reference's rendered SMPL views)"""
    from PIL import Image
    from oracle import neus_oracle as O
    os.makedirs(os.path.join(data_dir, "img"), exist_ok=True)
    yy, xx = np.mgrid[0:res, 0:res]
    disk = ((xx - res / 2 + 0.5) ** 2 + (yy - res / 2 + 0.5) ** 2) < (0.3 * res) ** 2
    frames = []
    for k in range(n):
        ang = 2 * np.pi * k / n
        pose = O.lookat(np.array([1.5 * np.sin(ang), 0.2, 1.5 * np.cos(ang)]), np.zeros(3), np.array([0., 1, 0]))
        img = np.zeros((res, res, 3), np.uint8)
        img[disk] = (200, 150 + 20 * k, 100)
        Image.fromarray(img).save(os.path.join(data_dir, "img", "%04d.png" % k))
        frames.append({"file_path": "img/%04d" % k, "transform_matrix": np.asarray(pose).tolist()})
    with open(os.path.join(data_dir, "transforms_train.json"), "w") as fp:
        json.dump({"camera_angle_x": float(np.pi / 3), "frames": frames}, fp)
    return data_dir


def make_conf(exp_dir, data_dir, keys):
    import bench
    conf = bench.make_conf(RES, SPP, small=True)
    conf.put("general.base_exp_dir", str(exp_dir))
    conf.put("general.log_scalars", False)
    conf.put("dataset.data_dir", str(data_dir))
    for k, v in keys.items():
        conf.put(k, v)
    return conf


def _oracle_kernels(r):
    """the CPU stand-ins of dp_common.build_runner: the oracle's render (its jitter from torch's host stream, renderer.py:318) and a
    perceptor around the oracle's ViT.  render() is also what validate_image calls under no_grad: the oracle takes its normals by autograd."""
    from oracle import neus_oracle as O

    def oracle_render(rays_o, rays_d, near, far, perturb_overwrite=-1, background_rgb=None, cos_anneal_ratio=0.0):
        jitter = torch.rand(rays_o.shape[0], 1)
        with torch.enable_grad():
            return O.render(dict(r.sdf_network.named_parameters()), dict(r.color_network.named_parameters()), r.deviation_network.variance,
                            rays_o, rays_d, near, far, SPP // 2, SPP // 2, 4, jitter, background_rgb, cos_anneal_ratio)
    r.renderer.render = oracle_render


def build(kind, mode, exp_dir, data_dir, keys=None, **runner_kw):
    """a Runner of `mode` on device `kind`, ready for train() / train_clip().  `runner_kw`: resume=, resume_tag=, is_continue=, ..."""
    from avatarclip_amd.runner import Runner, EllipsoidPrior, clip_vit_random_state_dict
    device = device_of(kind)
    conf = make_conf(exp_dir, data_dir, dict(TRAIN_KEYS if mode == "train" else CLIP_KEYS, **(keys or {})))
    r = Runner(None, mode=mode, conf=conf, device=device, **runner_kw)
    if kind != "cuda":
        _oracle_kernels(r)
    if mode == "train_clip":
        clip_sd = clip_vit_random_state_dict(0)
        if kind != "cuda":
            from oracle import clip_vit_oracle as C

            class OraclePerceptor:
                def encode_image(self, x):
                    return C.encode_image(clip_sd, x)
            r.init_clip(perceptor=OraclePerceptor())
        else:
            r.init_clip(clip_state_dict=clip_sd)
        r.init_smpl(EllipsoidPrior(device=device))
    return r


def instrument(r, stop_after=None):
    """-> log: one entry per step, appended as the step ends: its number, the learning rate it ran at, and the host-side draws -- train:
    the image index and the drawn [B,10] batch; train_clip: per view eye / at, the background choice and the ray count.  `stop_after`:
    raise Interrupted once that step (iter_step after it) is complete, checkpoint and record written."""
    log, choices, batches = [], [], []
    after, background, rays_at = r._after_step, r.draw_background, r.dataset.gen_random_rays_at

    def draw_background(view, choice_i=None):
        out = background(view, choice_i)
        choices.append(int(out[0]))
        return out

    def gen_random_rays_at(img_idx, batch_size):
        data = rays_at(img_idx, batch_size)
        batches.append((int(img_idx), data.detach().cpu().clone()))
        return data

    def after_step(loss, clip_stage):
        entry = dict(step=int(r.iter_step), lr=float(r.optimizer.param_groups[0]["lr"]))
        if clip_stage:
            entry.update(eyes=[np.asarray(v.eye).copy() for v in r.last_views], ats=[np.asarray(v.at).copy() for v in r.last_views],
                         rays=[int(v.rays_o.shape[0]) for v in r.last_views], choices=list(choices))
        else:
            entry.update(image=batches[-1][0], batch=batches[-1][1])
        del choices[:], batches[:]
        log.append(entry)
        after(loss, clip_stage)
        if stop_after is not None and r.iter_step == stop_after:
            raise Interrupted(stop_after)
    r.draw_background, r.dataset.gen_random_rays_at, r._after_step = draw_background, gen_random_rays_at, after_step
    return log


def run(r, stop_after=None):
    """train() / train_clip() of an instrumented Runner -> (log, parameters after the last step it ran, on the host)"""
    log = instrument(r, stop_after)
    try:
        r.train() if r.mode == "train" else r.train_clip()
        assert stop_after is None, "the run ended before step %r" % (stop_after,)
    except Interrupted:
        pass
    return log, [p.detach().cpu().clone() for p in r.params_to_train]


def same_draws(a, b):
    """two log entries of the same step hold exactly the same host-side draws"""
    if a["step"] != b["step"] or a["lr"] != b["lr"]:
        return False
    if "image" in a:
        return a["image"] == b["image"] and torch.equal(a["batch"], b["batch"])
    return (a["rays"] == b["rays"] and a["choices"] == b["choices"] and len(a["eyes"]) == len(b["eyes"])
            and all(np.array_equal(x, y) for x, y in zip(a["eyes"] + a["ats"], b["eyes"] + b["ats"])))


def max_abs_diff(pa, pb):
    return max(float((x.double() - y.double()).abs().max()) for x, y in zip(pa, pb))


def interrupted_and_resumed(kind, mode, root, data_dir, stop_after, keys=None, tag=None):
    """a run into <root>/exp stopped after `stop_after`, continued by a fresh Runner(resume=True) -> (log of both parts, final parameters,
    the resumed Runner)"""
    exp = os.path.join(str(root), "exp")
    first, _ = run(build(kind, mode, exp, data_dir, keys, resume_tag=tag), stop_after)
    assert [e["step"] for e in first] == list(range(1, stop_after + 1))
    r = build(kind, mode, exp, data_dir, keys, resume=True, resume_tag=tag)
    rest, params = run(r)
    return first + rest, params, r


# ---------------------------------------------------------------------------------------------------------------- two ranks over gloo
RANK_STEPS, RANK_STOP = 4, 2
RANK_KEYS = {"train.end_iter": RANK_STEPS, "train.save_freq": 2, "train.val_freq": 2}


def worker(rank, world, port, out_dir, kind, data_dir):
    """rank `rank` of `world` (every rank on device 0 when kind == "cuda", the machine's hardware-queue setting): the uninterrupted run,
    the run stopped after RANK_STOP, and its continuation by a fresh Runner(resume=True), one after the other -> <out_dir>/rank<k>.pt"""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      AVC_DIST_BACKEND="gloo")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch.distributed as dist
    from avatarclip_amd import parallel
    parallel.init_from_env(backend="gloo")
    full, p_full = run(build(kind, "train_clip", os.path.join(out_dir, "exp_full"), data_dir, RANK_KEYS))
    exp = os.path.join(out_dir, "exp")
    first, _ = run(build(kind, "train_clip", exp, data_dir, RANK_KEYS), RANK_STOP)
    parallel.barrier()                      # rank 0's checkpoint and every rank's record are in place
    r = build(kind, "train_clip", exp, data_dir, RANK_KEYS, resume=True)
    assert r.world == world and r.rank == rank
    resumed_from, data_seed = r.resumed_from, r.data_seed
    rest, p_rest = run(r)
    torch.save(dict(full=full, first=first, rest=rest, p_full=p_full, p_rest=p_rest, resumed_from=resumed_from, data_seed=data_seed),
               os.path.join(out_dir, "rank%d.pt" % rank))
    parallel.barrier()
    dist.destroy_process_group()


def spawn_ranks(world, out_dir, kind, data_dir, timeout):
    """tests/views_common.spawn_ranks with this module's worker: the ranks are joined under `timeout` seconds, a rank still alive then is
    killed and the test fails"""
    import time
    import torch.multiprocessing as mp
    ctx = mp.spawn(worker, args=(world, dp_common.free_port(), out_dir, kind, data_dir), nprocs=world, join=False)
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
