"""train.views_per_iter = V: one optimisation step renders V camera views over the W ranks -- rank r the views
r, r + W, ... one after the other -- and takes ONE Adam step on (1/V) * sum_j grad L_j.  A view's data streams (numpy, random, torch on
the host and on the device) belong to the VIEW, seeded B + j, so (W = 1, V = 4) and (W = 2, V = 4) are the same optimisation.  On the
CPU, with the oracle renderer and perceptor: the distributed and stream logic is what is under test.  Reference: the single-view
gradients taken one after the other and averaged (tests/dp_common.single_process_accumulation's recipe, views_common.accumulate_views).
Bounds: those of tests/test_parallel_runner_gloo.py (fp32 re-association of the accumulation only).
The background augmentation is off here (it is on in tests/test_gpu_views_per_iter.py): its chess board takes squares of H // k pixels,
k in 10..19, which is 0 at the 8 x 8 view of these tests -- views 2 and 3 of seed 0 draw that background.  Camera, light, ambience and
jitter still come from the view's numpy and torch streams."""
import random

import numpy as np
import pytest
import torch

from tests import views_common as VC

RES, SPP, V = 8, 8, 4
EXTRA = {"train.use_bg_aug": False}
SPAWN_TIMEOUT = 300


@pytest.fixture(scope="module")
def reference():
    return VC.accumulate_views("cpu", V, RES, SPP, extra=EXTRA)


@pytest.fixture(scope="module")
def one_process():
    w0, steps, r = VC.single_process("cpu", V, RES, SPP, extra=EXTRA)
    return dict(w0=w0, step=steps[0], views_per_iter=r.views_per_iter, world=r.world)


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    return VC.spawn_ranks(2, str(tmp_path_factory.mktemp("w2v4")), "cpu", RES, SPP, V, 2, SPAWN_TIMEOUT, extra=EXTRA)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_one_process_renders_four_views_per_step(reference, one_process):
    ref, s = reference, one_process["step"]
    assert one_process["views_per_iter"] == V and one_process["world"] == 1
    assert _same(ref["w0"], one_process["w0"])
    assert len(s["eyes"]) == V and s["last_view_is_last"]
    for a in range(V):
        for b in range(a + 1, V):
            assert not np.array_equal(s["eyes"][a], s["eyes"][b]), "views %d and %d drew the same camera" % (a, b)
    for j in range(V):
        assert np.array_equal(s["eyes"][j], ref["eyes"][j]) and np.array_equal(s["ats"][j], ref["ats"][j]), j
        assert abs(s["losses"][j] - ref["losses"][j]) < 1e-6, (j, s["losses"], ref["losses"])
    assert abs(s["loss"] - np.mean(ref["losses"])) < 1e-6
    assert s["rays_stat"] == sum(s["rays"]) == V * RES * RES
    VC.assert_grads_close(ref["grads"], s["grads"], 1e-5)
    assert s["iter_step"] == 1
    assert any(not torch.equal(w, p) for w, p in zip(one_process["w0"], s["params"])), "the step moved no parameter"


def test_two_gloo_ranks_render_two_views_each(reference, one_process, two_ranks):
    a, b = two_ranks
    sa, sb = a["steps"][0], b["steps"][0]
    assert a["base_seed"] == b["base_seed"] == 0 and (a["data_seed"], b["data_seed"]) == (0, 1)
    assert _same(a["w0"], b["w0"]) and _same(a["w0"], one_process["w0"])
    one = one_process["step"]
    for rank, s in ((0, sa), (1, sb)):      # rank r renders the views r and r + 2, in that order
        assert len(s["eyes"]) == 2 and s["last_view_is_last"]
        for k, j in enumerate((rank, rank + 2)):
            assert np.array_equal(s["eyes"][k], one["eyes"][j]) and np.array_equal(s["ats"][k], one["ats"][j]), (rank, j)
            assert abs(s["losses"][k] - reference["losses"][j]) < 1e-6, (rank, j)
        assert abs(s["loss"] - np.mean(s["losses"])) < 1e-6
        assert s["iter_step"] == 1 and s["bucket_is_grad"]
    assert _same(sa["grads"], sb["grads"]) and _same(sa["params"], sb["params"])
    VC.assert_grads_close(reference["grads"], sa["grads"], 1e-5)
    VC.assert_grads_close(one["grads"], sa["grads"], 1e-5)
    for r in (a, b):
        assert r["all_reduces"] == [1, 1] and r["all_reduce_on_flat"], r["all_reduces"]


def test_a_views_streams_continue_from_step_to_step(two_ranks, tmp_path):
    """views 0 and 1 over two steps: the same cameras whether view 1 is the second view of the only process (W = 1, V = 2), the view of
    rank 1 (W = 2, V = 2) or the first of rank 1's two views (W = 2, V = 4).  Cameras only: after the first Adam step the parameters
    of the three configurations differ by re-association, amplified by Adam's normalisation -- the cameras depend on the streams alone."""
    _, w1v2, _ = VC.single_process("cpu", 2, RES, SPP, steps=2, extra=EXTRA)
    w2v2 = VC.spawn_ranks(2, str(tmp_path), "cpu", RES, SPP, 2, 2, SPAWN_TIMEOUT, extra=EXTRA)
    w2v4 = two_ranks
    for step in range(2):
        for j in (0, 1):
            want = (w1v2[step]["eyes"][j], w1v2[step]["ats"][j])
            for name, ranks in (("W=2,V=2", w2v2), ("W=2,V=4", w2v4)):
                s = ranks[j]["steps"][step]
                assert np.array_equal(s["eyes"][0], want[0]) and np.array_equal(s["ats"][0], want[1]), (name, step, j)
    assert not np.array_equal(w1v2[0]["eyes"][0], w1v2[1]["eyes"][0]), "view 0 drew the same camera in both steps"
    assert not np.array_equal(w1v2[0]["eyes"][1], w1v2[1]["eyes"][1]), "view 1 drew the same camera in both steps"


def test_the_default_is_one_view_per_rank_and_untouched():
    def run(n_views):
        w0, steps, r = VC.single_process("cpu", n_views, RES, SPP, extra=EXTRA)
        states = (np.random.get_state(), random.getstate(), torch.get_rng_state())
        return r, steps[0], states
    r0, s0, st0 = run(None)
    assert r0.views_per_iter == r0.world == 1 and r0.grad_bucket is None and r0._view_rngs == []
    r1, s1, st1 = run(1)
    assert r1.views_per_iter == 1
    assert _same(s0["grads"], s1["grads"]) and _same(s0["params"], s1["params"])
    assert np.array_equal(s0["eyes"][0], s1["eyes"][0]) and s0["loss"] == s1["loss"]
    assert len(s0["eyes"]) == 1 and s0["rays_stat"] == RES * RES
    assert st0[0][0] == st1[0][0] and np.array_equal(st0[0][1], st1[0][1]) and st0[0][2:] == st1[0][2:]
    assert st0[1] == st1[1]
    assert torch.equal(st0[2], st1[2])


def _conf(**train_keys):
    import bench
    conf = bench.make_conf(RES, SPP, small=True)
    for k, v in train_keys.items():
        conf.put("train." + k, v)
    return conf


@pytest.mark.parametrize("world,views", [(1, 0), (2, 3), (2, 1), (1, -2)])
def test_views_per_iter_must_be_a_positive_multiple_of_the_world_size(world, views, monkeypatch):
    from avatarclip_amd import parallel
    from avatarclip_amd.runner import Runner
    monkeypatch.setattr(parallel, "rank_world", lambda: (0, world))
    with pytest.raises(ValueError) as e:
        Runner(None, mode="train_clip", conf=_conf(views_per_iter=views), device=torch.device("cpu"))
    assert str(views) in str(e.value) and str(world) in str(e.value)
    with pytest.raises(ValueError):     # the constructor's argument (main.py's --views_per_iter) overrides the conf and is checked alike
        Runner(None, mode="train_clip", conf=_conf(views_per_iter=world), device=torch.device("cpu"), views_per_iter=views)


def test_mode_train_refuses_views_per_iter():
    from avatarclip_amd.runner import Runner
    with pytest.raises(ValueError) as e:
        Runner(None, mode="train", conf=_conf(views_per_iter=2), device=torch.device("cpu"))
    assert "2" in str(e.value) and "train" in str(e.value)


def test_the_command_line_flag_overrides_the_conf(monkeypatch):
    """python -m avatarclip_amd.main --views_per_iter V hands V to the Runner, which prefers it to train.views_per_iter"""
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
    monkeypatch.setattr(sys, "argv", ["main", "--mode", "train_clip", "--conf", "x.conf", "--views_per_iter", "8"])
    with pytest.raises(Stop):
        M.main()
    assert seen["views_per_iter"] == 8
    from avatarclip_amd.runner import Runner
    r = Runner(None, mode="train_clip", conf=_conf(views_per_iter=2), device=torch.device("cpu"), views_per_iter=4)
    assert r.views_per_iter == 4 and len(r._view_rngs) == 3
