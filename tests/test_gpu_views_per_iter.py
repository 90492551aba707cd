"""train.views_per_iter on the HIP path (the CPU half is tests/test_views_per_iter.py): V views per optimisation
step are the existing kernels run V / W times on a rank, one view's forward and backward before the next view is built.  Reference:
tests/dp_common.single_process_accumulation -- the single-view gradients one after the other, streams seeded B + j, averaged.  Bounds:
those of tests/test_gpu_parallel.py (per tensor 1e-4 * (||g|| + 1e-3 * ||all g||), per-view losses within 1e-5).  32 x 32 views, 32 samples
per ray, small nets, background augmentation on."""
import numpy as np
import pytest
import torch

from tests import views_common as VC
from tests.dp_common import single_process_accumulation

gpu = pytest.mark.gpu

RES, SPP, V = 32, 32, 4
SPAWN_TIMEOUT = 300


@pytest.fixture(scope="module")
def reference():
    w0, grads, losses = single_process_accumulation("cuda", V, RES, SPP, list(range(V)))     # train.seed = 0: B + j = j
    return dict(w0=w0, grads=grads, losses=losses)


@pytest.fixture(scope="module")
def one_process():
    w0, steps, r = VC.single_process("cuda", V, RES, SPP)
    return dict(w0=w0, step=steps[0], views_per_iter=r.views_per_iter)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@gpu
def test_one_process_renders_four_views_per_step_on_the_hip_path(reference, one_process):
    ref, s = reference, one_process["step"]
    assert one_process["views_per_iter"] == V and _same(ref["w0"], one_process["w0"])
    assert len(s["eyes"]) == V and s["last_view_is_last"] and s["bucket_is_grad"]
    eyes = np.stack(s["eyes"])
    assert (np.abs(eyes[:, None] - eyes[None]).max(-1) + np.eye(V)).min() > 1e-3, "two views drew the same camera"
    for j in range(V):
        assert abs(s["losses"][j] - ref["losses"][j]) < 1e-5, (j, s["losses"], ref["losses"])
    assert abs(s["loss"] - np.mean(ref["losses"])) < 1e-5
    assert s["rays_stat"] == sum(s["rays"]) == V * RES * RES
    VC.assert_grads_close(ref["grads"], s["grads"], 1e-4)
    assert s["iter_step"] == 1
    assert any(not torch.equal(w, p) for w, p in zip(one_process["w0"], s["params"])), "the step moved no parameter"


@gpu
def test_two_gloo_ranks_on_one_device_render_two_views_each(reference, one_process, tmp_path):
    """two processes on device 0 (gloo collectives: RCCL refuses duplicate devices), each with the machine's hardware-queue setting --
    two processes at the default four queues are inside what parallel.check_queue_oversubscription allows"""
    a, b = VC.spawn_ranks(2, str(tmp_path), "cuda", RES, SPP, V, 1, SPAWN_TIMEOUT)
    sa, sb = a["steps"][0], b["steps"][0]
    assert (a["data_seed"], b["data_seed"]) == (0, 1)
    assert _same(a["w0"], b["w0"]) and _same(a["w0"], reference["w0"])
    one = one_process["step"]
    for rank, s in ((0, sa), (1, sb)):      # rank r renders the views r and r + 2, in that order
        assert len(s["eyes"]) == 2 and s["last_view_is_last"]
        for k, j in enumerate((rank, rank + 2)):
            assert np.array_equal(s["eyes"][k], one["eyes"][j]) and np.array_equal(s["ats"][k], one["ats"][j]), (rank, j)
            assert abs(s["losses"][k] - reference["losses"][j]) < 1e-5, (rank, j, s["losses"], reference["losses"])
        assert s["iter_step"] == 1 and s["bucket_is_grad"]
    assert _same(sa["grads"], sb["grads"]) and _same(sa["params"], sb["params"])
    VC.assert_grads_close(reference["grads"], sa["grads"], 1e-4)
    for r in (a, b):
        assert r["all_reduces"] == [1] and r["all_reduce_on_flat"], r["all_reduces"]


@gpu
def test_two_silhouette_views_per_step():
    """the reference's default sampling mode: ray sets of a data-dependent size, the view built on the side stream, the CLIP passes
    replayed as graphs.  Two views in one step -- a graph instance or a view's panels held across views would show here.  iter_i = 1:
    body cameras (the face camera of iter_i % 4 == 0 sits 0.4 from the head, where the silhouette fills the frame)."""
    extra = {"train.use_silhouettes": True, "train.max_ray_num": 1024}
    ref = VC.accumulate_views("cuda", 2, RES, SPP, iter_i=1, extra=extra)
    w0, steps, r = VC.single_process("cuda", 2, RES, SPP, iter_i=1, extra=extra)
    s = steps[0]
    assert r.use_silhouettes and r._side_stream is not None and _same(ref["w0"], w0)
    assert s["rays"] == ref["rays"] and all(0 < n <= 1024 for n in s["rays"]) and s["rays"][0] != s["rays"][1], (s["rays"], ref["rays"])
    assert s["rays_stat"] == sum(s["rays"])
    for j in range(2):
        assert np.array_equal(s["eyes"][j], ref["eyes"][j]) and np.array_equal(s["ats"][j], ref["ats"][j]), j
        assert abs(s["losses"][j] - ref["losses"][j]) < 1e-5, (j, s["losses"], ref["losses"])
    VC.assert_grads_close(ref["grads"], s["grads"], 1e-4)
    assert s["iter_step"] == 1 and all(torch.isfinite(p).all() for p in s["params"])
