"""AvatarAnimate's CLIP-guided optimisers (avatarclip_amd.animate with AnimateContext(renderer_gradient=True)) against tests/golden/animate_clip.npz,
which scripts/gen_golden_animate_clip.py produced by RUNNING THE REFERENCE'S OWN PoseOptimizer / VPoserOptimizer / MotionOptimizer methods (extracted
with `ast`), on CPU with the same differentiable stand-ins on both sides (tests/animate_clip_standins.py, oracle/animate_standins.py): the random draw
order (torch and numpy), the loss composition and the returned poses / motion are pinned; the renderer and CLIP behind the stand-ins are not."""
import os

import numpy as np
import pytest
import torch

from oracle.animate_standins import StandInVPoser, text_feature_of
from tests import animate_clip_standins as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TEXT = "a rendered 3d man is arguing"


def _gold():
    z = np.load(os.path.join(GOLD, "animate_clip.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind == "f" and z[k].ndim else z[k]) for k in z.files}


def _ctx(renderer_gradient=True):
    from avatarclip_amd import animate as A
    return A.AnimateContext(S.Perceptor(0), text_feature_of, S.smpl_arrays(0), StandInVPoser(0), render_fn=S.render, device="cpu",
                            renderer_gradient=renderer_gradient)


@pytest.mark.parametrize("name", ["PoseOptimizer", "VPoserOptimizer"])
def test_pose_optimisers_match_the_reference_methods(name):
    from avatarclip_amd import animate as A
    g = _gold()
    gen = A.build_pose_generator({"type": name, "optim_cfg": {"lr": 0.05}, "num_iteration": 4, "topk": 3}, _ctx())
    torch.manual_seed(int(g[name + "_seed"]))
    np.random.seed(int(g[name + "_seed"]))
    poses = gen.get_topk_poses(TEXT)
    assert poses.shape == (3, 69) and torch.allclose(poses, g[name + "_poses"], atol=1e-5), (poses - g[name + "_poses"]).abs().max()
    assert np.random.rand() == float(g[name + "_after_draw"])          # the same number of elevation draws, in the same places


def test_motion_optimizer_clip_term_matches_the_reference_method():
    from avatarclip_amd import animate as A
    g = _gold()
    cand = torch.from_numpy(np.load(os.path.join(GOLD, "animate.npz"))["mi_poses"])
    torch.manual_seed(int(g["motion_seed"]))
    mo = A.MotionOptimizer(_ctx(), num_frame=12, latent_dim=64, num_layers=2, num_heads=4, num_iteration=4, clip_coef=0.5, delta_coef=0.01,
                           clip_num_part=5)
    torch.manual_seed(int(g["motion_init_seed"]))
    np.random.seed(int(g["motion_init_seed"]))
    motion = mo.get_motion(TEXT, cand)
    assert motion.shape == (12, 69) and torch.allclose(motion, g["motion"], atol=1e-5), (motion - g["motion"]).abs().max()
    assert np.random.rand() == float(g["motion_after_draw"])


def test_the_switch_is_off_by_default_and_named_in_the_refusal():
    from avatarclip_amd import animate as A
    ctx = _ctx(renderer_gradient=False)
    assert ctx.render_fn is S.render and not ctx.renderer_gradient
    for make in (lambda: A.PoseOptimizer(ctx), lambda: A.VPoserOptimizer(ctx), lambda: A.MotionOptimizer(ctx, clip_coef=0.001)):
        with pytest.raises(NotImplementedError, match="renderer_gradient=True"):
            make()
    assert A.AnimateContext(None, text_feature_of, S.smpl_arrays(0), None, device="cpu").render_fn.__name__ == "_render_hip"
    assert A.AnimateContext(None, text_feature_of, S.smpl_arrays(0), None, device="cpu", renderer_gradient=True).render_fn.__name__ == "_render_hip_grad"


def test_cli_flag_sets_the_switch(monkeypatch):
    from avatarclip_amd import animate as A
    seen = {}

    class Stop(Exception):
        pass

    def fake_ctx(*a, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(A, "AnimateContext", fake_ctx)
    import sys
    import types
    # the CLI's third-party imports, stubbed: only the argument handling is under test
    hbp = types.ModuleType("human_body_prior")
    models, tools = types.ModuleType("human_body_prior.models"), types.ModuleType("human_body_prior.tools")
    vm, ml = types.ModuleType("human_body_prior.models.vposer_model"), types.ModuleType("human_body_prior.tools.model_loader")
    vm.VPoser = object

    class Blob:
        def to(self, device):
            return self

        def eval(self):
            return self

    ml.load_model = lambda *a, **k: (Blob(), None)
    for name, mod in (("human_body_prior", hbp), ("human_body_prior.models", models), ("human_body_prior.tools", tools),
                      ("human_body_prior.models.vposer_model", vm), ("human_body_prior.tools.model_loader", ml)):
        monkeypatch.setitem(sys.modules, name, mod)
    from avatarclip_amd import clip_vit, smpl_lbs, tokenizer
    monkeypatch.setattr(clip_vit, "load_state_dict", lambda p: {})
    monkeypatch.setattr(clip_vit, "ClipVisionB32", lambda *a, **k: None)
    monkeypatch.setattr(tokenizer, "SimpleTokenizer", lambda p: None)
    monkeypatch.setattr(smpl_lbs, "load_smpl_arrays", lambda p, d: None)
    args = ["--clip_weights", "w", "--bpe", "b", "--smpl", "s", "--vposer", "v"]
    for extra, want in (([], False), (["--renderer_gradient"], True)):
        seen.clear()
        with pytest.raises(Stop):
            A.main(args + extra)
        assert seen["renderer_gradient"] is want
