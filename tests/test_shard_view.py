"""train.shard_view: the rays of ONE view cut over the W ranks by pixel range, so that the one-view optimisation of
the reference confs runs on W devices as the same optimisation.  On the CPU, over gloo, with the oracle renderer and perceptor: the
distributed logic is what is under test -- shared data streams, the cut, the three global quantities (eikonal sums, loss sums, CLIP
images) and their autograd rules, the SUM of the bucket.  The yardstick of every case is the same step by ONE process without the key
(tests/shard_common.yardstick); the bounds are those of tests/test_parallel_runner_gloo.py, because the difference is of the same kind:
fp32 re-association of sums only (loss 1e-6, gradients 1e-5 * (|g| + 1e-3 |G|))."""
import numpy as np
import pytest
import torch

from tests import shard_common as SC

SPP = 8
LOSS_TOL, GRAD_REL = 1e-6, 1e-5
# an odd grid side: P = 23 * 23 = 529 is a multiple of neither 2 nor 3 (and the chess-board background has squares of 23 // k >= 1 pixels)
FULL_RES = 23
# silhouette mode: rays inside the dilated silhouette of the ellipsoid prior on a grid of at most 24 x 24; one image into CLIP
SIL_RES = 24
SIL = {"train.use_silhouettes": True, "train.max_ray_num": 200, "train.add_no_texture": False}
# fewer rays than ranks (no background augmentation: a grid this small has no room for a chess board)
TINY = {"train.use_silhouettes": True, "train.max_ray_num": 3, "train.use_bg_aug": False}


@pytest.fixture(scope="module")
def full_frame_yardstick():
    return SC.yardstick("cpu", None, FULL_RES, SPP)


@pytest.fixture(scope="module")
def silhouette_yardstick():
    return SC.yardstick("cpu", None, SIL_RES, SPP, SIL)


@pytest.mark.parametrize("world", [2, 3])
def test_full_frame_cut_over_the_ranks_is_the_single_process_step(world, full_frame_yardstick, tmp_path):
    ranks = SC.spawn_ranks(world, str(tmp_path), "cpu", FULL_RES, SPP)
    assert all(b["views_per_iter"] == 1 for b in ranks), "views_per_iter defaults to 1 with train.shard_view"
    assert (FULL_RES * FULL_RES) % world != 0
    SC.check_cuts(ranks, silhouette=False)
    SC.check_against_yardstick(ranks, full_frame_yardstick, LOSS_TOL, GRAD_REL)
    assert any(not torch.equal(w, p) for w, p in zip(ranks[0]["w0"], ranks[0]["step"]["params"])), "the step moved no parameter"


@pytest.mark.parametrize("world", [2, 4])
def test_silhouette_rays_cut_at_their_quantiles(world, silhouette_yardstick, tmp_path):
    ranks = SC.spawn_ranks(world, str(tmp_path), "cpu", SIL_RES, SPP, SIL)
    R, P = ranks[0]["step"]["rays"][0], ranks[0]["H"][0] * ranks[0]["W"][0]
    assert world <= R < P, "the silhouette selects a part of the grid"
    SC.check_cuts(ranks, silhouette=True)
    SC.check_against_yardstick(ranks, silhouette_yardstick, LOSS_TOL, GRAD_REL)


def test_a_rank_without_rays_joins_every_collective(tmp_path):
    world = 4
    ref = SC.yardstick("cpu", None, SIL_RES, SPP, TINY)
    R = ref["step"]["rays"][0]
    assert 1 <= R < world, "the case needs fewer rays than ranks, got %d" % R
    ranks = SC.spawn_ranks(world, str(tmp_path), "cpu", SIL_RES, SPP, TINY)
    SC.check_cuts(ranks, silhouette=True)
    idle = [b for b in ranks if b["rays_rendered"][0] == 0]
    assert len(idle) == world - R and all(b["my_pixels"][0][0] == b["my_pixels"][0][1] for b in idle), "a rank without rays owns no pixel"
    SC.check_against_yardstick(ranks, ref, LOSS_TOL, GRAD_REL)


def test_two_views_per_step_each_cut_over_the_ranks(tmp_path):
    """add_no_texture (two images into CLIP) and views_per_iter = 2: both views are cut over both ranks, one after the other; the step is
    the one process's that renders the same two views, and the mean is over 2 (not over the ranks)"""
    extra = {"train.add_no_texture": True}
    ref = SC.yardstick("cpu", 2, FULL_RES, SPP, extra)
    ranks = SC.spawn_ranks(2, str(tmp_path), "cpu", FULL_RES, SPP, dict(extra, **{"train.views_per_iter": 2}))
    assert all(b["views_per_iter"] == 2 and len(b["step"]["eyes"]) == 2 for b in ranks)
    assert not np.array_equal(ranks[0]["step"]["eyes"][0], ranks[0]["step"]["eyes"][1])
    SC.check_cuts(ranks, silhouette=False)
    SC.check_against_yardstick(ranks, ref, LOSS_TOL, GRAD_REL)
    assert abs(ranks[0]["step"]["loss"] - np.mean(ref["step"]["losses"])) < LOSS_TOL


def _conf(**train_keys):
    import bench
    conf = bench.make_conf(8, SPP, small=True)
    for k, v in train_keys.items():
        conf.put("train." + k, v)
    return conf


def test_one_rank_with_the_key_is_the_step_without_it():
    """world 1: nothing to cut, no process group needed, the same bits"""
    from tests import views_common as VC
    _, off, r_off = VC.single_process("cpu", None, 8, SPP, extra={"train.use_bg_aug": False})
    _, on, r_on = VC.single_process("cpu", None, 8, SPP, extra={"train.use_bg_aug": False, "train.shard_view": True})
    assert not r_off.shard_view and r_on.shard_view and r_on._shard_group is None and r_on.grad_bucket is None
    assert not torch.distributed.is_initialized()
    assert r_on.views_per_iter == 1
    assert off[0]["loss"] == on[0]["loss"] and np.array_equal(off[0]["eyes"][0], on[0]["eyes"][0])
    assert SC._same(off[0]["grads"], on[0]["grads"]) and SC._same(off[0]["params"], on[0]["params"])


def test_the_key_allows_any_view_count_on_any_world(monkeypatch):
    from avatarclip_amd import parallel
    from avatarclip_amd.runner import Runner
    monkeypatch.setattr(parallel, "rank_world", lambda: (1, 2))
    r = Runner(None, mode="train_clip", conf=_conf(shard_view=True), device=torch.device("cpu"))
    assert r.views_per_iter == 1 and r._view_rngs == []
    r = Runner(None, mode="train_clip", conf=_conf(shard_view=True, views_per_iter=3), device=torch.device("cpu"))
    assert r.views_per_iter == 3 and len(r._view_rngs) == 2      # the views 1 and 2, on every rank
    assert r.data_seed == r.base_seed == 0, "rank 1 draws from the streams of rank 0: one set for the job"
    with pytest.raises(ValueError):
        Runner(None, mode="train_clip", conf=_conf(shard_view=True, views_per_iter=0), device=torch.device("cpu"))
    with pytest.raises(ValueError):      # without the key a single view on two ranks stays refused
        Runner(None, mode="train_clip", conf=_conf(views_per_iter=1), device=torch.device("cpu"))
    # the argument overrides the conf, both ways
    assert Runner(None, mode="train_clip", conf=_conf(), device=torch.device("cpu"), shard_view=True).shard_view
    assert not Runner(None, mode="train_clip", conf=_conf(shard_view=True, views_per_iter=2), device=torch.device("cpu"), shard_view=False).shard_view


def test_validation_on_rank_0_leaves_the_shared_streams_alone():
    """rank 0 alone validates, and validation draws (its camera from numpy, its jitter from torch): with a view cut over the ranks those
    draws must not move rank 0's data streams away from the other ranks'.  Without the cut they move them, as they always did."""
    import random
    from avatarclip_amd.runner import Runner
    r = Runner(None, mode="train_clip", conf=_conf(shard_view=True), device=torch.device("cpu"))
    drawn = []

    def validate(*a, **k):
        drawn.append((np.random.randint(1 << 30), random.random(), float(torch.rand(1))))
    r.validate_image = r.validate_mesh = validate
    r.val_freq = r.val_mesh_freq = 1
    state = lambda: (np.random.get_state()[1].copy(), np.random.get_state()[2], random.getstate(), torch.get_rng_state())
    same = lambda a, b: np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and torch.equal(a[3], b[3])
    before = state()
    r._shard_group = object()       # as on more than one rank
    r._validation_hooks(clip_stage=True)
    assert len(drawn) == 2 and same(before, state())
    r._shard_group = None
    r._validation_hooks(clip_stage=True)
    assert len(drawn) == 4 and not same(before, state())


def test_mode_train_refuses_the_key():
    from avatarclip_amd.runner import Runner
    with pytest.raises(ValueError) as e:
        Runner(None, mode="train", conf=_conf(shard_view=True), device=torch.device("cpu"))
    assert "shard_view" in str(e.value) and "train_clip" in str(e.value)
    with pytest.raises(ValueError):
        Runner(None, mode="train", conf=_conf(), device=torch.device("cpu"), shard_view=True)


def test_the_command_line_flag_reaches_the_runner(monkeypatch):
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
    monkeypatch.setattr(sys, "argv", ["main", "--mode", "train_clip", "--conf", "x.conf", "--shard_view"])
    with pytest.raises(Stop):
        M.main()
    assert seen["shard_view"] is True
    seen.clear()
    monkeypatch.setattr(sys, "argv", ["main", "--mode", "train_clip", "--conf", "x.conf"])
    with pytest.raises(Stop):
        M.main()
    assert seen["shard_view"] is None, "without the flag the conf decides"


def test_the_cut_of_a_view():
    """parallel.shard_ranges on its own: equal full-frame ranges; ray quantiles; ranks without rays own no pixel"""
    from avatarclip_amd import parallel
    q, p = parallel.shard_ranges(3, 49)
    assert q == p == [0, 16, 32, 49]
    sel = torch.tensor([3, 4, 9, 10, 11, 20, 30])
    q, p = parallel.shard_ranges(2, 36, sel)
    assert q == [0, 3, 7] and p == [0, 10, 36]
    q, p = parallel.shard_ranges(4, 36, sel[:2])
    assert q == [0, 0, 1, 1, 2] and p == [0, 0, 4, 4, 36]
    q, p = parallel.shard_ranges(4, 36, sel[:1])
    assert q == [0, 0, 0, 0, 1] and p == [0, 0, 0, 0, 36]


def test_the_collectives_without_a_group_are_the_identity():
    from avatarclip_amd import parallel
    x = torch.arange(6.0).reshape(1, 2, 3).requires_grad_(True)
    assert parallel.allreduce_sum(x) is x and parallel.PixelGather()(x, [0, 2], 0) is x
    assert parallel.shard_group() is None
