"""Runner(resume=True): an interrupted `train` or `train_clip` run goes on exactly where it stopped -- networks, Adam state and iter_step
from the checkpoint, the data streams, the per-view streams, the image permutation and the iteration counter from the resume records
beside it.  On the CPU, with the oracle renderer and perceptor (tests/resume_common.py): what is under test is the record, the rule that
picks it and the order of the draws.  An interruption is an exception raised between two steps.  Reference: the uninterrupted run A of
the same seed; the parameters are compared with torch.equal after two uninterrupted runs have been shown to agree that far."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from tests import resume_common as RC
from tests.test_pipeline_cpu import _spec, calls     # noqa: F401  (the recording stage stubs of the pipeline's own CPU tests)

SPAWN_TIMEOUT = 300
FIVE_KEYS = {"sdf_network_fine", "variance_network_fine", "color_network_fine", "optimizer", "iter_step"}


@pytest.fixture(scope="module")
def data_dir(tmp_path_factory):
    return RC.write_dataset(str(tmp_path_factory.mktemp("views")))


@pytest.fixture(scope="module", autouse=True)
def one_thread_count():
    """(reductions split over a varying number of threads are the one thing that could make two CPU runs of one seed differ)"""
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 4))
    yield
    torch.set_num_threads(n)


def _uninterrupted(mode, root, data_dir, keys=None):
    log, params = RC.run(RC.build("cpu", mode, os.path.join(str(root), "exp"), data_dir, keys))
    return dict(log=log, params=params)


def _assert_same_run(a, log, params):
    assert [e["step"] for e in log] == [e["step"] for e in a["log"]]
    for want, got in zip(a["log"], log):
        assert RC.same_draws(want, got), ("step %d" % want["step"], want, got)
    assert all(torch.equal(x, y) for x, y in zip(a["params"], params)), RC.max_abs_diff(a["params"], params)


# ---------------------------------------------------------------------------------------------------------------- mode train
@pytest.fixture(scope="module")
def train_a(tmp_path_factory, data_dir):
    return _uninterrupted("train", tmp_path_factory.mktemp("train_a"), data_dir, {"train.save_freq": 3})


def test_two_uninterrupted_train_runs_agree_bit_for_bit(train_a, tmp_path, data_dir):
    again = _uninterrupted("train", tmp_path, data_dir, {"train.save_freq": 4})       # (the checkpoint interval moves nothing either)
    _assert_same_run(train_a, again["log"], again["params"])
    images = [e["image"] for e in train_a["log"]]
    assert len(images) == RC.TRAIN_STEPS and all(sorted(images[k:k + 4]) == [0, 1, 2, 3] for k in (0, 4, 8))      # three epochs of a permutation
    assert images[0:4] != images[4:8] or images[4:8] != images[8:12]


@pytest.mark.parametrize("stop_after,save_freq", [(6, 3), (8, 4)], ids=["mid_epoch", "epoch_boundary"])
def test_train_resumes_draw_for_draw(train_a, tmp_path, data_dir, stop_after, save_freq):
    """step 6 of 4-image epochs: the permutation of the second epoch is restored and no start-of-run draw is made; step 8: the record
    precedes the reshuffle for the third epoch, which the resumed run makes from the restored streams"""
    log, params, r = RC.interrupted_and_resumed("cpu", "train", tmp_path, data_dir, stop_after, {"train.save_freq": save_freq})
    assert r.resumed_from == stop_after and r.iter_step == RC.TRAIN_STEPS
    _assert_same_run(train_a, log, params)


# ---------------------------------------------------------------------------------------------------------------- mode train_clip
@pytest.fixture(scope="module")
def clip_a(tmp_path_factory, data_dir):
    return _uninterrupted("train_clip", tmp_path_factory.mktemp("clip_a"), data_dir)


def test_two_uninterrupted_train_clip_runs_agree_bit_for_bit(clip_a, tmp_path, data_dir):
    again = _uninterrupted("train_clip", tmp_path, data_dir)
    _assert_same_run(clip_a, again["log"], again["params"])
    log = clip_a["log"]
    assert len(log) == RC.CLIP_STEPS and all(len(e["eyes"]) == 2 and len(e["choices"]) == 2 and min(e["rays"]) > 0 for e in log)
    # the face camera of iter_i % 4 == 0 looks at the head from 0.4 away, every other one at the body from further off
    face = [bool(np.allclose(e["ats"][0], [0, 0.65, 0.3])) for e in log]
    assert face == [i % 4 == 0 for i in range(RC.CLIP_STEPS)]


@pytest.mark.parametrize("stop_after", [3, 6])
def test_train_clip_resumes_draw_for_draw(clip_a, tmp_path, data_dir, stop_after):
    """val_freq = save_freq = 3: the validation camera and the jitter of its render are drawn AFTER the checkpoint of steps 3 and 6 is
    written, from the streams the next step continues; two views per step: the second view's own streams are in the record too"""
    log, params, r = RC.interrupted_and_resumed("cpu", "train_clip", tmp_path, data_dir, stop_after)
    assert r.resumed_from == stop_after and r.iter_step == RC.CLIP_STEPS
    assert any(f.startswith("%08d_" % stop_after) for f in os.listdir(os.path.join(str(tmp_path), "exp", "validations_fine")))      # validation ran there
    _assert_same_run(clip_a, log, params)


def test_is_continue_alone_is_another_run(clip_a, tmp_path, data_dir):
    """the same interruption continued the reference's way: weights, Adam state and iter_step load, but iter_i counts from 0 again and the
    streams are those of a new process -- other cameras from step 4 on.  (This is the defect; `resume=` is what removes it.)"""
    exp = os.path.join(str(tmp_path), "exp")
    first, _ = RC.run(RC.build("cpu", "train_clip", exp, data_dir), 3)
    r = RC.build("cpu", "train_clip", exp, data_dir, is_continue=True)
    assert r.iter_step == 3 and r.resumed_from is None
    rest, _ = RC.run(r)
    assert [e["step"] for e in rest] == [4, 5, 6, 7, 8]
    for want, got in zip(clip_a["log"][:3], first):
        assert RC.same_draws(want, got)
    for want, got in zip(clip_a["log"][3:], rest):
        assert want["lr"] == got["lr"]
        assert not any(np.array_equal(x, y) for x, y in zip(want["eyes"], got["eyes"])), want["step"]


# ---------------------------------------------------------------------------------------------------------------- the record and the rule
@pytest.fixture(scope="module")
def stopped(tmp_path_factory, data_dir):
    """a train run of 12 steps with a checkpoint every 3, stopped after step 9, tag "T" -> its experiment directory"""
    exp = os.path.join(str(tmp_path_factory.mktemp("stopped")), "exp")
    RC.run(RC.build("cpu", "train", exp, data_dir, {"train.save_freq": 3}, resume_tag="T"), 9)
    return exp


def _copy(exp, tmp_path):
    import shutil
    return shutil.copytree(exp, os.path.join(str(tmp_path), "exp"))


def _resume(exp, data_dir, mode="train", keys=None, tag="T", **kw):
    return RC.build("cpu", mode, exp, data_dir, dict({"train.save_freq": 3}, **(keys or {})), resume=True, resume_tag=tag, **kw)


def test_what_is_on_disk(stopped):
    assert sorted(os.listdir(os.path.join(stopped, "checkpoints"))) == ["ckpt_%06d.pth" % s for s in (3, 6, 9)]
    records = sorted(os.listdir(os.path.join(stopped, "resume")))
    assert records == ["ckpt_%06d.rank0.pt" % s for s in (3, 6, 9)] and not any(n.endswith("pth") for n in records)
    blob = torch.load(os.path.join(stopped, "checkpoints", "ckpt_000009.pth"), map_location="cpu", weights_only=True)
    assert set(blob) == FIVE_KEYS and blob["iter_step"] == 9
    rec = torch.load(os.path.join(stopped, "resume", records[-1]), map_location="cpu", weights_only=True)      # no allow-list, no opt-in
    assert rec["iter_step"] == 9 and rec["mode"] == "train" and rec["world"] == 1 and rec["views_per_iter"] == 1 and rec["shard_view"] is False
    assert rec["resume_tag"] == "T" and rec["iter_i"] is None and rec["view_streams"] == [] and (rec["base_seed"], rec["data_seed"]) == (0, 0)
    assert sorted(rec["image_perm"].tolist()) == [0, 1, 2, 3]
    assert set(rec["streams"]) == {"numpy_name", "numpy_keys", "numpy_pos", "numpy_has_gauss", "numpy_cached_gaussian", "random_version",
                                   "random_internal", "random_gauss_next", "torch_host", "torch_device"}
    assert os.path.getsize(os.path.join(stopped, "resume", records[-1])) < 64 * 1024


def test_stream_states_round_trip_bit_for_bit():
    import random
    from avatarclip_amd.runner import pack_rng_state, unpack_rng_state
    np.random.seed(5); random.seed(6); torch.manual_seed(7)
    np.random.normal(); random.gauss(0, 1)                      # (both generators then hold a cached second gaussian)
    state = (np.random.get_state(), random.getstate(), torch.get_rng_state(), None)
    want = (np.random.normal(size=3), [random.gauss(0, 1), random.random()], torch.rand(3))
    np.random.seed(0); random.seed(0); torch.manual_seed(0)
    back = unpack_rng_state(pack_rng_state(state))
    np.random.set_state(back[0]); random.setstate(back[1]); torch.set_rng_state(back[2])
    got = (np.random.normal(size=3), [random.gauss(0, 1), random.random()], torch.rand(3))
    assert np.array_equal(want[0], got[0]) and want[1] == got[1] and torch.equal(want[2], got[2]) and back[3] is None


def test_the_newest_checkpoint_without_its_record_falls_back_to_the_last_complete_pair(stopped, tmp_path, data_dir):
    exp = _copy(stopped, tmp_path)
    os.remove(os.path.join(exp, "resume", "ckpt_000009.rank0.pt"))      # what a kill between the checkpoint and the record leaves
    r = _resume(exp, data_dir)
    assert r.resumed_from == 6 and r.iter_step == 6
    os.remove(os.path.join(exp, "checkpoints", "ckpt_000006.pth"))      # a record without its checkpoint is no pair either
    assert _resume(exp, data_dir).resumed_from == 3


def test_no_pair_starts_at_step_0(tmp_path, data_dir, stopped):
    r = _resume(os.path.join(str(tmp_path), "fresh"), data_dir)
    assert r.resumed_from is None and r.iter_step == 0 and r._resume_record is None
    exp = _copy(stopped, tmp_path)
    import shutil
    shutil.rmtree(os.path.join(exp, "resume"))
    r = _resume(exp, data_dir)
    assert r.resumed_from is None and r.iter_step == 0


def test_another_tag_is_not_continued(stopped, data_dir):
    for tag in ("U", None):
        r = _resume(stopped, data_dir, tag=tag)
        assert r.resumed_from is None and r.iter_step == 0
    assert _resume(stopped, data_dir, tag="T").resumed_from == 9
    assert RC.build("cpu", "train", stopped, data_dir, is_continue=True).iter_step == 9      # is_continue reads no record and no tag


def test_a_record_of_another_kind_of_run_is_refused_with_both_values(stopped, tmp_path, data_dir, monkeypatch):
    from avatarclip_amd import parallel
    with pytest.raises(ValueError) as e:                     # mode
        _resume(stopped, data_dir, mode="train_clip", keys={"train.views_per_iter": 1})
    assert "mode" in str(e.value) and "'train'" in str(e.value) and "'train_clip'" in str(e.value)
    exp = os.path.join(str(tmp_path), "exp")
    RC.run(RC.build("cpu", "train_clip", exp, data_dir, resume_tag="T"), 3)
    with pytest.raises(ValueError) as e:                     # views per step: 2 in the record, 4 asked for
        _resume(exp, data_dir, mode="train_clip", keys={"train.views_per_iter": 4})
    assert "views_per_iter = 2" in str(e.value) and "views_per_iter = 4" in str(e.value)
    monkeypatch.setattr(parallel, "rank_world", lambda: (0, 2))
    with pytest.raises(ValueError) as e:                     # world size: 1 in the record, 2 now
        _resume(exp, data_dir, mode="train_clip")
    assert "world = 1" in str(e.value) and "world = 2" in str(e.value)


def test_a_failing_save_leaves_nothing_under_the_final_name(tmp_path, data_dir, monkeypatch):
    r = RC.build("cpu", "train", os.path.join(str(tmp_path), "exp"), data_dir)
    r.iter_step = 5
    save = torch.save

    def dies_half_way(obj, path, *a, **k):
        with open(path, "wb") as fh:
            fh.write(b"half a checkpoint")
        raise OSError("No space left on device")
    monkeypatch.setattr(torch, "save", dies_half_way)
    with pytest.raises(OSError):
        r.save_checkpoint()
    with pytest.raises(OSError):
        r.save_resume_record()
    assert os.listdir(os.path.join(r.base_exp_dir, "checkpoints")) == [] and os.listdir(os.path.join(r.base_exp_dir, "resume")) == []
    monkeypatch.setattr(torch, "save", save)
    r.save_checkpoint()
    assert os.listdir(os.path.join(r.base_exp_dir, "checkpoints")) == ["ckpt_000005.pth"]


def test_the_command_line_hands_resume_to_the_runner(monkeypatch):
    import sys
    from avatarclip_amd import main as M
    seen = {}

    class Stop(Exception):
        pass

    def runner(*a, **k):
        seen.update(k)
        raise Stop
    monkeypatch.setattr(M, "Runner", runner)
    monkeypatch.setattr(M.parallel, "init_from_env", lambda: (0, 1, 0))
    monkeypatch.setattr(M.torch.cuda, "set_device", lambda d: None)
    for argv, want in ((["--resume", "--resume_tag", "job-7"], (True, "job-7")), ([], (False, None))):
        monkeypatch.setattr(sys, "argv", ["main", "--mode", "train_clip", "--conf", "x.conf"] + argv)
        with pytest.raises(Stop):
            M.main()
        assert (seen["resume"], seen["resume_tag"]) == want


# ---------------------------------------------------------------------------------------------------------------- two ranks
def test_two_gloo_ranks_each_restore_their_own_streams(tmp_path, data_dir):
    a, b = RC.spawn_ranks(2, str(tmp_path), "cpu", data_dir, SPAWN_TIMEOUT)
    assert (a["data_seed"], b["data_seed"]) == (3, 4) and a["resumed_from"] == b["resumed_from"] == RC.RANK_STOP
    assert sorted(os.listdir(os.path.join(str(tmp_path), "exp", "resume"))) == ["ckpt_%06d.rank%d.pt" % (s, k) for s in (2, 4) for k in (0, 1)]
    for rank, res in ((0, a), (1, b)):
        log = res["first"] + res["rest"]
        assert [e["step"] for e in log] == [1, 2, 3, 4] == [e["step"] for e in res["full"]]
        for want, got in zip(res["full"], log):
            assert RC.same_draws(want, got), (rank, want, got)
        assert all(torch.equal(x, y) for x, y in zip(res["p_full"], res["p_rest"])), rank
    for ea, eb in zip(a["full"], b["full"]):      # the two ranks render different views
        assert not np.array_equal(ea["eyes"][0], eb["eyes"][0])
    assert all(torch.equal(x, y) for x, y in zip(a["p_rest"], b["p_rest"]))


# ---------------------------------------------------------------------------------------------------------------- the pipeline's rule
def _decisions(calls_fixture, monkeypatch):
    """the recording stubs, extended to note what `run` decided for the stage: (continue inside?, the tag the Runner would get)"""
    from avatarclip_amd import pipeline as P
    seen = {}
    for st in P.RESUMABLE:
        stub = getattr(P, "stage_" + st)

        def fn(run, st=st, stub=stub):
            seen[st] = (st in run.resume, run.fingerprints.get(st))
            return stub(run)
        monkeypatch.setattr(P, "stage_" + st, fn)
    return seen


def _leave(spec, stage, status):
    from avatarclip_amd import pipeline as P
    m = P.load_manifest(spec.out_dir)
    m["stages"][stage] = {"status": status, "fingerprint": m["stages"][stage]["fingerprint"]}
    P.write_manifest(spec.out_dir, m)


@pytest.mark.parametrize("status", ["failed", "running"])
def test_pipeline_continues_an_unfinished_stage_of_the_same_fingerprint(tmp_path, calls, monkeypatch, status):
    from avatarclip_amd import pipeline as P
    spec = _spec(tmp_path)
    seen = _decisions(calls, monkeypatch)
    P.run(spec, log=lambda *a: None)
    fps = P.fingerprints(spec)
    assert seen == {"init": (False, fps["init"]), "appearance": (False, fps["appearance"])}      # a first run tags its records, continues nothing
    _leave(spec, "appearance", status)
    seen.clear(); del calls[:]
    out = P.run(spec, log=lambda *a: None)
    assert calls == ["appearance"] and seen == {"appearance": (True, fps["appearance"])}
    assert out["manifest"]["stages"]["appearance"]["status"] == "done" and "resumed_from" not in out["manifest"]["stages"]["appearance"]
    # a changed prompt: another fingerprint, nothing of the old run is continued
    _leave(spec, "appearance", status)
    seen.clear(); del calls[:]
    changed = dataclasses.replace(spec, prompt="a 3D rendering of a witch in unreal engine")
    P.run(changed, log=lambda *a: None)
    assert calls[0] == "appearance" and seen == {"appearance": (False, P.fingerprints(changed)["appearance"])}
    assert P.fingerprints(changed)["appearance"] != fps["appearance"]
    # force / restart_stages: a fresh start under the same fingerprint
    for how in (dict(force=True, from_stage="appearance", until_stage="appearance"), dict(restart_stages=True)):
        P.run(spec, log=lambda *a: None)
        _leave(spec, "appearance", status)
        seen.clear(); del calls[:]
        P.run(dataclasses.replace(spec, **how), log=lambda *a: None)
        assert calls[0] == "appearance" and seen == {"appearance": (False, fps["appearance"])}, how
    assert P.fingerprints(dataclasses.replace(spec, restart_stages=True)) == fps
    # a finished stage is skipped as before; an unfinished stage that is no optimisation loop has nothing to continue
    P.run(spec, log=lambda *a: None)
    seen.clear(); del calls[:]
    assert P.run(spec, log=lambda *a: None)["stages"] == {st: "skipped" for st in P.STAGES} and calls == [] and seen == {}
    assert not P.continue_stage(spec, "mesh", {"status": "failed", "fingerprint": fps["mesh"]}, fps["mesh"])
    assert "--restart_stages" in {s for a in P.build_parser()._actions for s in a.option_strings}


def test_a_resumed_stage_records_the_step_it_continued_from(tmp_path, calls, monkeypatch):
    from avatarclip_amd import pipeline as P
    spec = _spec(tmp_path)
    P.run(spec, log=lambda *a: None)
    _leave(spec, "init", "failed")
    stub = P.stage_init

    def resumed(run):
        run.resumed_from["init"] = 17 if "init" in run.resume else None
        return stub(run)
    monkeypatch.setattr(P, "stage_init", resumed)
    out = P.run(spec, log=lambda *a: None)
    assert out["manifest"]["stages"]["init"]["resumed_from"] == 17 and out["stages"]["init"] == "ran"
    with open(os.path.join(spec.out_dir, P.MANIFEST)) as fh:
        assert json.load(fh)["stages"]["init"]["resumed_from"] == 17
