"""Runner(resume=True) on the HIP path (the CPU half, and the tests of the record and of the rule, are tests/test_resume_cpu.py): the same
interrupted `train` and `train_clip` runs at the same sizes -- 16 x 16 views, 32 samples per ray, small nets; train_clip in silhouette
mode, where the view is built on the side stream and the CLIP passes are replayed as graphs, with two views per step and validation on the
checkpoint's steps.  An interruption is an exception raised between two steps, in this process; the run is continued by a fresh Runner
with a perceptor, a side stream and graphs of its own.

What is asserted.  The host-side draws of every step (image index and pixel batch; cameras, background choices, ray counts; learning
rates) equal the uninterrupted run's exactly.  The final parameters are compared with PARAM_BOUND = 4 x the run-to-run spread of two
uninterrupted runs of one seed in two fresh processes, measured on the commit before this feature at these sizes
(profiles/resume.md): that spread is 0 in both modes, so the comparison is torch.equal."""
import os

import numpy as np
import pytest
import torch

from tests import resume_common as RC

gpu = pytest.mark.gpu
pytestmark = gpu
SPAWN_TIMEOUT = 300
PARAM_BOUND = {"train": 0.0, "train_clip": 0.0, "pipeline": 0.0}      # 4 x the measured spread (profiles/resume.md)


def _assert_params(kind, want, got):
    diff = RC.max_abs_diff(want, got)
    print("%s: largest absolute parameter difference to the uninterrupted run %.3e (bound %.3e)" % (kind, diff, PARAM_BOUND[kind]))
    if PARAM_BOUND[kind] == 0.0:
        assert all(torch.equal(x, y) for x, y in zip(want, got)), diff
    else:
        assert diff <= PARAM_BOUND[kind], (diff, PARAM_BOUND[kind])


def _assert_same_run(kind, a, log, params):
    assert [e["step"] for e in log] == [e["step"] for e in a["log"]]
    for want, got in zip(a["log"], log):
        assert RC.same_draws(want, got), ("step %d" % want["step"], want, got)
    _assert_params(kind, a["params"], params)


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    return RC.write_dataset(str(tmp_path_factory.mktemp("views")))


def _uninterrupted(mode, root, data_dir, keys=None):
    log, params = RC.run(RC.build("cuda", mode, os.path.join(str(root), "exp"), data_dir, keys))
    return dict(log=log, params=params)


@pytest.fixture(scope="module")
def train_a(tmp_path_factory, data_dir):
    return _uninterrupted("train", tmp_path_factory.mktemp("train_a"), data_dir, {"train.save_freq": 3})


@pytest.fixture(scope="module")
def clip_a(tmp_path_factory, data_dir):
    return _uninterrupted("train_clip", tmp_path_factory.mktemp("clip_a"), data_dir)


@pytest.mark.parametrize("stop_after,save_freq", [(6, 3), (8, 4)], ids=["mid_epoch", "epoch_boundary"])
def test_train_resumes_draw_for_draw_on_the_hip_path(train_a, tmp_path, data_dir, stop_after, save_freq):
    log, params, r = RC.interrupted_and_resumed("cuda", "train", tmp_path, data_dir, stop_after, {"train.save_freq": save_freq})
    assert r.resumed_from == stop_after and r.iter_step == RC.TRAIN_STEPS
    assert len(train_a["log"]) == RC.TRAIN_STEPS and all(sorted(e["image"] for e in train_a["log"][k:k + 4]) == [0, 1, 2, 3] for k in (0, 4, 8))
    _assert_same_run("train", train_a, log, params)
    rec = torch.load(os.path.join(str(tmp_path), "exp", "resume", "ckpt_%06d.rank0.pt" % stop_after), map_location="cpu", weights_only=True)
    assert rec["streams"]["torch_device"] is not None and rec["streams"]["torch_device"].dtype == torch.uint8      # the device generator is in the record


@pytest.mark.parametrize("stop_after", [3, 6])
def test_train_clip_resumes_draw_for_draw_on_the_hip_path(clip_a, tmp_path, data_dir, stop_after):
    """silhouette mode: ray sets of a data-dependent size, the view built on the side stream, the CLIP passes replayed as graphs; the
    gaussian background and the jitter come from the device generator, whose state the record holds"""
    log, params, r = RC.interrupted_and_resumed("cuda", "train_clip", tmp_path, data_dir, stop_after)
    assert r.resumed_from == stop_after and r.iter_step == RC.CLIP_STEPS and r.use_silhouettes and r._side_stream is not None
    a = clip_a["log"]
    assert len(a) == RC.CLIP_STEPS and all(len(e["eyes"]) == 2 and 0 < min(e["rays"]) and max(e["rays"]) <= RC.RES * RC.RES for e in a)
    assert len({c for e in a for c in e["choices"]}) > 1, "one background choice in the whole run: the augmentation is not in play"
    assert any(f.startswith("%08d_" % stop_after) for f in os.listdir(os.path.join(str(tmp_path), "exp", "validations_fine")))
    _assert_same_run("train_clip", clip_a, log, params)


def test_two_gloo_ranks_on_one_device_each_restore_their_own_streams(tmp_path, data_dir):
    """two processes on device 0 (gloo collectives: RCCL refuses duplicate devices), each with the machine's hardware-queue setting, as
    tests/test_gpu_views_per_iter.py starts them: per rank the uninterrupted run, the interrupted one and its continuation"""
    a, b = RC.spawn_ranks(2, str(tmp_path), "cuda", data_dir, SPAWN_TIMEOUT)
    assert (a["data_seed"], b["data_seed"]) == (3, 4) and a["resumed_from"] == b["resumed_from"] == RC.RANK_STOP
    for rank, res in ((0, a), (1, b)):
        log = res["first"] + res["rest"]
        assert [e["step"] for e in log] == [1, 2, 3, 4] == [e["step"] for e in res["full"]]
        for want, got in zip(res["full"], log):
            assert RC.same_draws(want, got), (rank, want, got)
        _assert_params("train_clip", res["p_full"], res["p_rest"])
    for ea, eb in zip(a["full"], b["full"]):
        assert not np.array_equal(ea["eyes"][0], eb["eyes"][0])
    assert all(torch.equal(x, y) for x, y in zip(a["p_rest"], b["p_rest"]))


def test_the_pipeline_continues_inside_the_appearance_stage(tmp_path):
    """the toy chain of tests/test_gpu_pipeline.py with 4 appearance steps and a checkpoint after each: the stage is interrupted after
    its second step, the pipeline is run again and continues it at step 2; every later stage runs, and the stage's final checkpoint is
    the one an uninterrupted pipeline writes into a second directory"""
    import dataclasses
    from avatarclip_amd import pipeline as P
    from avatarclip_amd.runner import Runner
    from tests import test_gpu_pipeline as TP
    os.makedirs(str(tmp_path / "assets"))
    fields, _ = TP._write_assets(str(tmp_path / "assets"))
    for k, v in (("train.end_iter", 4), ("train.save_freq", 1)):
        fields["appearance_conf"].put(k, v)
    spec = P.PipelineSpec(out_dir=str(tmp_path / "out"), **fields)
    quiet = lambda *a: None
    after = Runner._after_step
    armed = [True]

    def after_step(self, loss, clip_stage):
        after(self, loss, clip_stage)
        if armed[0] and clip_stage and self.iter_step == 2:
            raise RC.Interrupted(2)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(Runner, "_after_step", after_step)
        with pytest.raises(RC.Interrupted):
            P.run(spec, log=quiet)
        m = P.load_manifest(spec.out_dir)["stages"]
        assert m["appearance"]["status"] == "failed" and m["init"]["status"] == "done" and "mesh" not in m
        assert sorted(os.listdir(os.path.join(spec.out_dir, "exp_clip", "checkpoints"))) == ["ckpt_000001.pth", "ckpt_000002.pth"]
        armed[0] = False
        second = P.run(spec, log=quiet)
    later = P.STAGES[P.STAGES.index("appearance"):]
    assert second["stages"] == {st: ("ran" if st in later else "skipped") for st in P.STAGES}
    m = second["manifest"]["stages"]
    assert m["appearance"]["resumed_from"] == 2 and m["appearance"]["status"] == "done" and "resumed_from" not in m["mesh"]
    assert os.path.basename(m["appearance"]["outputs"]["checkpoint"]["path"]) == "ckpt_000004.pth"
    whole = P.run(dataclasses.replace(spec, out_dir=str(tmp_path / "out_whole"), until_stage="appearance"), log=quiet)
    assert "resumed_from" not in whole["manifest"]["stages"]["appearance"]
    load = lambda d: torch.load(os.path.join(d, "exp_clip", "checkpoints", "ckpt_000004.pth"), map_location="cpu", weights_only=True)
    got, want = load(spec.out_dir), load(str(tmp_path / "out_whole"))
    assert got["iter_step"] == want["iter_step"] == 4
    nets = ("sdf_network_fine", "variance_network_fine", "color_network_fine")
    assert all(sorted(got[n]) == sorted(want[n]) for n in nets)
    _assert_params("pipeline", [want[n][k] for n in nets for k in sorted(want[n])], [got[n][k] for n in nets for k in sorted(got[n])])
    adam = lambda c: [c["optimizer"]["state"][i][k] for i in sorted(c["optimizer"]["state"]) for k in ("exp_avg", "exp_avg_sq")]
    _assert_params("pipeline", adam(want), adam(got))
