"""train.shard_view on the HIP path (the CPU half is tests/test_shard_view.py): two ranks (gloo collectives, both on
device 0 -- the development layout of tests/test_gpu_parallel.py) cut ONE view's rays by pixel range and take the step that ONE process
takes without the key (tests/shard_common.yardstick: today's path, same train.seed).

What is asserted, per case:
  * the images gathered for CLIP are torch.equal to the single process's: every kernel before them is per point or per ray, and its
    result does not depend on which other rays share the launch (tests/test_gpu_kernels.py asserts padding invariance,
    Runner._render_chunks relies on chunk invariance) -- an exact statement, not a tolerance;
  * loss within 1e-5 and gradients within 1e-4 * (|g| + 1e-3 |G|) of the yardstick: the gates of
    tests/test_gpu_parallel.py::test_ranks_on_the_hip_path_equal_single_gpu_accumulation, for the same kind of difference (the order in
    which partial sums of the weight gradient, the eikonal term and the loss sums are added);
  * the cut, the cameras, the bucket and the collectives as on the CPU (shard_common.check_cuts / check_against_yardstick).
The measured differences are printed (profiles/shard_view.md records them)."""
import pytest
import torch

from tests import shard_common as SC

gpu = pytest.mark.gpu
LOSS_TOL, GRAD_REL = 1e-5, 1e-4

CASES = {
    # an odd grid side: 529 rays, 264 + 265; one image into CLIP
    "full_frame": (23, 16, {"train.add_no_texture": False}, False),
    # rays inside the dilated silhouette of the ellipsoid prior on a grid of at most 32 x 32, scattered into the image by a rank-local ray_of_pixel
    "silhouette": (32, 16, {"train.use_silhouettes": True, "train.max_ray_num": 400, "train.add_no_texture": False}, True),
    # two images into CLIP (texture under the random light, and the untextured shading)
    "add_no_texture": (32, 32, {"train.add_no_texture": True}, False),
}


def _n_devices():
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


def _check(ranks, ref, silhouette):
    SC.check_cuts(ranks, silhouette)
    for k, b in enumerate(ranks):
        assert len(b["images"]) == len(ref["images"]) == 1
        for got, want in zip(b["images"], ref["images"]):
            assert got.shape == want.shape, (k, got.shape, want.shape)
            differ = int((got != want).sum())
            print("rank %d: %d of %d image values differ from the single process's (max |difference| %.3g)"
                  % (k, differ, want.numel(), float((got - want).abs().max())))
            assert torch.equal(got, want), "rank %d: the gathered CLIP images are not the single process's" % k
    SC.check_against_yardstick(ranks, ref, LOSS_TOL, GRAD_REL)


@gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_two_ranks_cut_one_view_and_take_the_single_process_step(case, tmp_path):
    res, spp, extra, silhouette = CASES[case]
    ranks = SC.spawn_ranks(2, str(tmp_path), "cuda", res, spp, extra)
    ref = SC.yardstick("cuda", None, res, spp, extra)
    R, P = ref["step"]["rays"][0], ref["H"][0] * ref["W"][0]
    assert (R < P) if silhouette else (R == P == res * res)
    assert ref["images"][0].shape == (2 if extra["train.add_no_texture"] else 1, P, 3)
    _check(ranks, ref, silhouette)


@gpu
@pytest.mark.skipif(_n_devices() < 2, reason="RCCL refuses two ranks on one device: needs a node with >= 2 MI355X (runs by itself on one)")
def test_rccl_ranks_one_device_each_cut_one_view(tmp_path):
    """the product's layout: world = min(4, devices) ranks, one MI355X each, the collectives over RCCL -- the assertions of the gloo
    cases, so that the first multi-GPU node produces the evidence without a code change"""
    world = min(4, _n_devices())
    res, spp, extra, silhouette = CASES["add_no_texture"]
    ranks = SC.spawn_ranks(world, str(tmp_path), "cuda", res, spp, extra, backend="nccl")
    assert [b["device"] for b in ranks] == ["cuda:%d" % k for k in range(world)] and all(b["backend"] == "nccl" for b in ranks)
    ref = SC.yardstick("cuda", None, res, spp, extra)
    _check(ranks, ref, silhouette)
    print("RCCL world %d: one view cut over the ranks == the single-process step" % world)
