"""AvatarAnimate's CLIP-guided optimisers on the MI355X with AnimateContext(renderer_gradient=True): renders through the HIP rasteriser with
neural_renderer's approximate backward (avatarclip_amd.mesh_render), embeddings through the HIP ViT, seeded stand-in assets (tests/test_animate.py's
synthetic SMPL arrays, StandInVPoser, random CLIP weights)."""
import os
import warnings

import numpy as np
import pytest
import torch

from oracle.animate_standins import StandInVPoser, text_feature_of
from tests.test_animate import CONF, _gold, _synthetic_smpl

gpu = pytest.mark.gpu


def _ctx(text_fn=text_feature_of):
    from avatarclip_amd import animate as A
    from avatarclip_amd import clip_vit as V
    from oracle import clip_vit_oracle as C
    dev = torch.device("cuda")
    return A.AnimateContext(V.ClipVisionB32(C.random_state_dict(0), dev), text_fn, _synthetic_smpl(dev), StandInVPoser(0).to(dev), device=dev,
                            renderer_gradient=True)


def _score(ctx, tf, pose, seed=0):
    np.random.seed(seed)                   # the same camera draws for every pose compared
    with torch.no_grad():
        return float(torch.nn.functional.cosine_similarity(ctx.get_pose_feature(pose.reshape(1, -1)), tf.reshape(1, -1)).reshape(-1)[0])


@gpu
def test_pose_optimisers_raise_the_clip_score_of_a_rendered_target():
    from avatarclip_amd import animate as A
    ctx = _ctx()
    target = _gold()["mi_poses"][1][:63].cuda()
    np.random.seed(1)
    with torch.no_grad():
        tf = ctx.get_pose_feature(target)[0]                 # the "text" is the embedding of the target pose's renders
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for cls, dim in ((A.PoseOptimizer, 63), (A.VPoserOptimizer, 32)):
            gen = cls(ctx, num_iteration=20, optim_cfg={"lr": 0.03}, topk=1)
            torch.manual_seed(5)
            start = torch.randn(dim)                         # the draw get_pose makes first
            start_pose = start.cuda() if dim == 63 else ctx.vp.decode(start.cuda()[None])["pose_body"].reshape(-1)
            torch.manual_seed(5)
            np.random.seed(2)
            pose = gen.get_pose(tf)
            assert pose.shape == (69,) and torch.isfinite(pose).all()
            before, after = _score(ctx, tf, start_pose), _score(ctx, tf, pose[:63])
            print(cls.__name__, "cosine to the target's embedding", before, "->", after)
            # (random CLIP weights put every render's embedding close to one common direction: the cosines are all near 1, what moves is the gap)
            assert after > before and (1 - after) < 0.95 * (1 - before)
    assert not [w for w in caught if "still waiting for the backward" in str(w.message)]


@gpu
def test_motion_optimizer_clip_term_runs_and_changes_the_motion():
    from avatarclip_amd import animate as A
    ctx = _ctx()
    poses = _gold()["mi_poses"][:, :63].cuda()
    out = {}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for coef in (0.0, 0.001):
            torch.manual_seed(21)
            mo = A.MotionOptimizer(ctx, num_frame=60, latent_dim=64, num_layers=2, num_heads=4, num_iteration=4, clip_coef=coef, delta_coef=0.01)
            torch.manual_seed(22)
            np.random.seed(3)
            out[coef] = mo.get_motion("a rendered 3d man is arguing", poses)
    assert not [w for w in caught if "still waiting for the backward" in str(w.message)]
    assert out[0.001].shape == (60, 69) and torch.isfinite(out[0.001]).all()
    assert (out[0.001] - out[0.0]).abs().max() > 0


@gpu
def test_the_base_conf_layout_runs_with_the_renderer_gradient(tmp_path):
    """confs/base.conf: VPoserCodebook candidates, then MotionOptimizer with its defaults (clip_coef = 0.001), a short optimisation"""
    from avatarclip_amd import animate as A
    from avatarclip_amd.conf import ConfigFactory
    ctx = _ctx()
    g = _gold()
    conf = ConfigFactory.parse_string(CONF.format(out=str(tmp_path / "base"), mode="motion", pose="VPoserCodebook", motion="MotionOptimizer",
                                                  extra="    num_iteration = 2\n    latent_dim = 64\n    num_layers = 2"))
    np.random.seed(0)
    poses, motion = A.run(conf, ctx, pose_assets=dict(codebook=g["cb_codebook"], codebook_embedding=g["cb_embedding"]))
    assert poses.shape == (5, 63) and motion.shape == (60, 69) and torch.isfinite(motion).all()
    assert sorted(os.listdir(str(tmp_path / "base"))) == ["candidate_%d.npy" % i for i in range(5)] + ["motion.npy"]
