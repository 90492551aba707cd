"""tests/golden/animate_clip.npz by RUNNING THE REFERENCE'S OWN CLIP-guided optimisers (build container only: needs the reference checkout).
    python scripts/gen_golden_animate_clip.py                                    TEST INFRASTRUCTURE ONLY.

The way oracle/gen_golden_animate.py does it (its `extract` / `bind` helpers, reused): the reference's methods, unmodified, extracted with `ast` and
bound to a stand-in `self` -- BasePoseGenerator.get_pose_feature / calculate_pose_score / sort_poses_by_score, PoseOptimizer.get_pose /
get_topk_poses, VPoserOptimizer.get_pose / get_topk_poses (pose_generation.py), BaseMotionGenerator.get_pose_feature and MotionOptimizer's
network construction, decode and get_motion with clip_coef > 0 (motion_generation.py).  What they call outside themselves is a stand-in from
tests/animate_clip_standins.py (SMPL, render_one_batch, the image encoder) or oracle/animate_standins.py (VPoser, the text feature), the same
objects tests/test_animate_clip_cpu.py hands to avatarclip_amd.animate.  Pinned: random draw order, loss composition, return values."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from oracle import gen_golden_animate as G  # noqa: E402
from oracle.animate_standins import StandInVPoser, text_feature_of  # noqa: E402
from tests import animate_clip_standins as S  # noqa: E402

TEXT = "a rendered 3d man is arguing"
POSE_SEED, VPOSER_SEED, MOTION_SEED, MOTION_INIT_SEED = 31, 32, 41, 42


def _self(**kw):
    s = G.Self()
    s.smpl, s.clip, s.vp = S.SMPLStandIn(S.smpl_arrays(0)), S.Perceptor(0), StandInVPoser(0)
    s.get_text_feature = lambda text: text_feature_of(text)
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def main():
    U = G.load_utils()
    ns = G.namespace(U)
    ns["render_one_batch"] = S.render_one_batch
    P = os.path.join(G.AA, "pose_generation.py")
    M = os.path.join(G.AA, "motion_generation.py")
    base = [("BasePoseGenerator", n, None) for n in ("get_pose_feature", "calculate_pose_score", "sort_poses_by_score")]
    fp = G.extract(P, ns, functions=("pose_padding",), methods=base + [(c, n, None) for c in ("PoseOptimizer", "VPoserOptimizer")
                                                                       for n in ("get_pose", "get_topk_poses")])
    fm = G.extract(M, ns, classes=("SinusoidalPositionalEncoding", "MotionXTransformerEncoder", "MotionXTransformerDecoder"), functions=("pose_padding",),
                   methods=[("BaseMotionGenerator", "get_pose_feature", None), ("MotionOptimizer", "__init__", G.NET_ONLY),
                            ("MotionOptimizer", "decode", None), ("MotionOptimizer", "get_motion", None)])
    rec = {}
    for cname, seed in (("PoseOptimizer", POSE_SEED), ("VPoserOptimizer", VPOSER_SEED)):
        gen = _self(optim_name="Adam", optim_cfg={"lr": 0.05}, num_iteration=4, topk=3)
        G.bind(gen, fp, "BasePoseGenerator", "get_pose_feature", "calculate_pose_score", "sort_poses_by_score")
        G.bind(gen, fp, cname, "get_pose", "get_topk_poses")
        torch.manual_seed(seed)
        np.random.seed(seed)
        poses = gen.get_topk_poses(TEXT)
        rec[cname + "_poses"] = poses
        rec[cname + "_seed"] = np.int64(seed)
        rec[cname + "_after_draw"] = np.float64(np.random.rand())           # where numpy's generator stands afterwards: the draw count
    torch.manual_seed(MOTION_SEED)
    mo = _self(num_frame=12)
    fm[("MotionOptimizer", "__init__")](mo, latent_dim=64, num_layers=2, num_heads=4, ckpt_path=None, optim_name="Adam", optim_cfg={"lr": 0.01},
                                        num_iteration=4, recon_coef=(1, 0.8, 0.6, 0.4, 0.2), clip_coef=0.5, delta_coef=0.01, clip_num_part=5)
    mo.eval()
    mo.get_pose_feature = fm[("BaseMotionGenerator", "get_pose_feature")].__get__(mo)
    G.bind(mo, fm, "MotionOptimizer", "decode", "get_motion")
    cand = torch.from_numpy(np.load(os.path.join(G.GOLD, "animate.npz"))["mi_poses"])
    torch.manual_seed(MOTION_INIT_SEED)
    np.random.seed(MOTION_INIT_SEED)
    rec["motion"] = mo.get_motion(TEXT, cand[:, :63].contiguous())
    rec["motion_after_draw"] = np.float64(np.random.rand())
    rec.update(motion_seed=np.int64(MOTION_SEED), motion_init_seed=np.int64(MOTION_INIT_SEED))
    out = {k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in rec.items()}
    path = os.path.join(G.GOLD, "animate_clip.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), {k: getattr(v, "shape", v) for k, v in out.items()})


if __name__ == "__main__":
    main()
