"""AvatarAnimate's candidate-pose and motion generators (reference: AvatarAnimate/models/pose_generation.py,
motion_generation.py, builder.py, main.py) on this repository's kernels: every render goes through the HIP rasteriser (`mesh_render.render_batch`:
one batched call for the white body and the textured one alike, camera_mode 'look_at'), every CLIP embedding through the HIP ViT / text towers
(`clip_vit.ClipVisionB32`, batched scoring path), SMPL posing through `smpl_lbs`.  The reference's third-party blobs are INPUTS, not part of the tree: the VPoser body prior (`human_body_prior`), the pose
codebook / conditional RealNVP / motion-VAE checkpoints, the SMPL model, the UV texture.  `AnimateContext` takes them as objects / state dicts with
the reference's names, so the reference's files load unmodified where somebody holds them; the tests drive everything with seeded stand-ins and pin
the arithmetic to the reference's OWN classes and methods (`oracle/gen_golden_animate.py` extracts them with `ast`).

What is built                                                                  reference
  AnimateContext.get_text_feature / get_pose_feature / calculate_pose_score     pose_generation.py:56-99, motion_generation.py:64-97
  VPoserCodebook   (codebook retrieval + duplicate suppression: the default)    pose_generation.py:288-329
  VPoserRealNVP    (conditional flow: decode / encode / sample / get_pose)      pose_generation.py:176-286
  MotionInterpolation (linear walk through VPoser's latent space)               motion_generation.py:100-137
  MotionOptimizer  (transformer motion-VAE decoder + reconstruction / delta     motion_generation.py:140-358
                    losses + the CLIP term when clip_coef > 0, see below)
  PoseOptimizer    (SMPL body pose optimised against the CLIP score)            pose_generation.py:102-135
  VPoserOptimizer  (VPoser latent optimised against the CLIP score)             pose_generation.py:138-173
  build_pose_generator / build_motion_generator / main (conf-driven CLI)        builder.py, main.py

The renderer gradient is OPT-IN: PoseOptimizer, VPoserOptimizer and MotionOptimizer's CLIP term (clip_coef > 0, the reference's default, so its
confs/base.conf) differentiate the CLIP score with respect to the POSE through the rasteriser, which takes neural_renderer's backward pass -- the
approximate gradient of Kato, Ushiku and Harada (CVPR 2018), restated and unpinned (mesh_render.py, csrc/avc_raster_grad.hip).
`AnimateContext(renderer_gradient=True)` (CLI: --renderer_gradient) makes the default render differentiable and lets them run; without it they
raise NotImplementedError as before, and a user-supplied `render_fn` combined with the switch is taken to be differentiable.

The posing on HIP is OPT-IN as well: `AnimateContext(posing="hip")` (CLI: --hip_posing) poses every body, scored or optimised, with
`smpl_lbs.pose_hip_grad` (two launches forward, three backward: csrc/avc_smpl.hip, csrc/avc_smpl_grad.hip) instead of `smpl_lbs.lbs` and
autograd.  The two agree to fp32 rounding, not bit for bit; the pinned scores of tests/golden/animate*.npz belong to the default, "torch".
"""
import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import clip_score

DEFAULT_ANGLES = (120, 150, 180, 210, 240)          # pose_generation.py:76-77
CAMERA_DISTANCE = 2.0                               # models/render.py:13


def pose_padding(pose):
    """63 body-pose values -> SMPL's 69 (the two hand joints stay at rest); 69 pass through  (pose_generation.py:19-24)"""
    if pose.shape[-1] == 69:
        return pose
    if pose.shape[-1] != 63:
        raise ValueError("a body pose has 63 or 69 values, got %d" % pose.shape[-1])
    return torch.cat([pose, pose.new_zeros(pose.shape[:-1] + (6,))], dim=-1)


# ----------------------------------------------------------------------------------------------------------------- rotations (models/utils.py)
def axis_angle_to_matrix(aa):
    """Rodrigues through the unit quaternion, as models/utils.py:143-221 composes it (angle -> 0 handled by the series of sin(x/2)/x)"""
    ang = aa.norm(dim=-1, keepdim=True)
    half = 0.5 * ang
    small = ang.abs() < 1e-6
    k = torch.where(small, 0.5 - ang * ang / 48.0, torch.sin(half) / torch.where(small, torch.ones_like(ang), ang))
    w, xyz = torch.cos(half), aa * k
    x, y, z = xyz.unbind(-1)
    w = w.squeeze(-1)
    s = 2.0 / (w * w + x * x + y * y + z * z)
    rows = [1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w),
            s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w),
            s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]
    return torch.stack(rows, -1).reshape(aa.shape[:-1] + (3, 3))


def matrix_to_rotation_6d(m):
    return m[..., :2, :].reshape(m.shape[:-2] + (6,))


def rotation_6d_to_matrix(d6):
    """Gram-Schmidt on the two stored rows (Zhou et al.; models/utils.py:125-141)"""
    b1 = F.normalize(d6[..., :3], dim=-1)
    a2 = d6[..., 3:]
    b2 = F.normalize(a2 - (b1 * a2).sum(-1, keepdim=True) * b1, dim=-1)
    return torch.stack([b1, b2, torch.linalg.cross(b1, b2, dim=-1)], dim=-2)


def matrix_to_axis_angle(m):
    """rotation matrix -> quaternion (the best-conditioned of the four candidates) -> axis-angle: the route of MotionOptimizer.decode
    (motion_generation.py:299-302 through models/utils.py:23-123)"""
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.reshape(m.shape[:-2] + (9,)).unbind(-1)
    q2 = torch.stack([1 + m00 + m11 + m22, 1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22], -1)
    pos = q2 > 0                                            # sqrt(max(0, x)) with a ZERO subgradient at x <= 0 (utils.py:11-20): the optimiser differentiates through this
    q_abs = torch.where(pos, torch.sqrt(torch.where(pos, q2, torch.ones_like(q2))), torch.zeros_like(q2))
    cand = torch.stack([torch.stack([q2[..., 0].clamp(min=0), m21 - m12, m02 - m20, m10 - m01], -1),
                        torch.stack([m21 - m12, q2[..., 1].clamp(min=0), m10 + m01, m02 + m20], -1),
                        torch.stack([m02 - m20, m10 + m01, q2[..., 2].clamp(min=0), m12 + m21], -1),
                        torch.stack([m10 - m01, m20 + m02, m21 + m12, q2[..., 3].clamp(min=0)], -1)], -2)
    cand = cand / (2.0 * q_abs.clamp(min=0.1))[..., None]
    best = q_abs.argmax(-1)
    quat = torch.gather(cand, -2, best[..., None, None].expand(best.shape + (1, 4))).squeeze(-2)
    n = quat[..., 1:].norm(dim=-1, keepdim=True)
    half = torch.atan2(n, quat[..., :1])
    ang = 2 * half
    small = ang.abs() < 1e-6
    k = torch.where(small, 0.5 - ang * ang / 48.0, torch.sin(half) / torch.where(small, torch.ones_like(ang), ang))
    return quat[..., 1:] / k


# ----------------------------------------------------------------------------------------------------------------- shared context
class AnimateContext:
    """What BasePoseGenerator / BaseMotionGenerator build in their constructors (pose_generation.py:31-49), handed in instead:

      perceptor     clip_vit.ClipVisionB32 (HIP) -- or anything with encode_image([B,3,224,224]) -> [B,512]
      text_feature  callable(text) -> [512] (ClipVisionB32.encode_text on the tokenised prompt, a cached embedding, ...)
      smpl          smpl_lbs.load_smpl_arrays(...) dict (v_template, posedirs, J_regressor, parents, lbs_weights, faces)
      vposer        VPoser-like object: decode(z[B,32]) -> {'pose_body': [B,21,3]}, encode(pose[B,63]).mean -> [B,32]
      render_fn     callable(vertices[bs,V,3] tensor, faces, angles) -> images [len(angles) * bs, 3, H, W] in [0,1], camera-major
                    (None: the HIP rasteriser below -- a white body, or the textured one when `texture` is given)
      texture       None (default): the body is white.  The path of a textured .obj (the reference's data/smpl_uv.obj; texture.load_obj_texture,
                    texture_size 8) or its cubes [F,8,8,8,3]: the default render_fn shows that body (mesh_render.render_rgb_batch), with or
                    without renderer_gradient.  A precomputed codebook matches it only if it was made with the same texture.
      renderer_gradient False (default): render_fn's images carry no gradient and the generators that need one refuse to run; True: the default
                    render_fn is the differentiable HIP path (mesh_render.render_grey_batch), a given render_fn is taken to be differentiable
      posing        "torch" (default): posed_vertices is smpl_lbs.lbs, differentiated by autograd -- the arithmetic the pinned scores were
                    taken with; "hip": smpl_lbs.pose_hip_grad, the same vertices to fp32 rounding (not bit for bit) and their gradient to the
                    pose from csrc/avc_smpl_grad.hip
    """
    POSINGS = ("torch", "hip")

    def __init__(self, perceptor, text_feature, smpl, vposer, render_fn=None, device=None, image_size=256, renderer_gradient=False, posing="torch",
                 texture=None):
        if posing not in self.POSINGS:
            raise ValueError("AnimateContext: posing is \"torch\" (smpl_lbs.lbs) or \"hip\" (smpl_lbs.pose_hip_grad), got %r" % (posing,))
        self.posing = posing
        self.perceptor, self.text_feature, self.smpl, self.vp = perceptor, text_feature, smpl, vposer
        self.device = torch.device(device) if device is not None else smpl["v_template"].device
        self.image_size = image_size
        self.renderer_gradient = bool(renderer_gradient)
        self.texture = None
        if texture is not None:
            from .texture import as_cubes
            self.texture = as_cubes(texture, self.device)
        default = self._render_hip_grad if self.renderer_gradient else self._render_hip
        self.render_fn = render_fn if render_fn is not None else default

    def get_text_feature(self, text):
        with torch.no_grad():
            return self.text_feature(text).reshape(-1).float().to(self.device)

    def posed_vertices(self, pose):
        """SMPL vertices of body poses [bs, 63 | 69] with the root turned by pi/2 about x (pose_generation.py:70-75); posing="hip": the same
        [bs,24,3] axis-angle through smpl_lbs.pose_hip_grad (equal to fp32 rounding, not bit for bit)"""
        from . import smpl_lbs
        pose = pose_padding(pose.reshape(-1, pose.shape[-1]).float().to(self.device))
        bs = pose.shape[0]
        root = pose.new_zeros(bs, 1, 3)
        root[:, 0, 0] = math.pi / 2
        full = torch.cat([root, pose.reshape(bs, 23, 3)], dim=1)
        if self.posing == "hip":
            return smpl_lbs.pose_hip_grad(self.smpl, full)
        rot = smpl_lbs.batch_rodrigues(full.reshape(-1, 3)).reshape(bs, 24, 3, 3)
        s = self.smpl
        v, _ = smpl_lbs.lbs(s["v_template"][None].expand(bs, -1, -1), rot, s["posedirs"], s["J_regressor"], s["parents"], s["lbs_weights"])
        return v

    @torch.no_grad()
    def _render_hip(self, vertices, faces, angles):
        """_render_hip_grad without a gradient: the default render of the pose and motion scorers"""
        return self._render_hip_grad(vertices.to(self.device), faces, angles)

    def _render_hip_grad(self, vertices, faces, angles):
        """models/render.py:10-39 on the HIP rasteriser: camera_mode 'look_at' at distance 2, azimuth = the angle, elevation drawn per angle
        from numpy's global generator (np.random.randn() * 0.3 degrees: the reference's draw, in its order).  White body under
        neural_renderer's light, or (AnimateContext(texture=...); models/render.py:6-35) the cubes of data/smpl_uv.obj on the same cameras.
        The len(angles) x bs renders camera-major in one call of mesh_render.render_batch (one batched forward-with-save, neural_renderer's
        approximate backward to the vertices) -> [len(angles) * bs, 3, S, S] either way."""
        from .mesh_render import render_batch
        from .shapegen_render import get_points_from_angles
        eyes = [get_points_from_angles(CAMERA_DISTANCE, np.random.randn() * 0.3, a) for a in angles]     # draw order: once per angle, before the batch loop
        bs = vertices.shape[0]
        eye_all = [e.astype(np.float32) for e in eyes for _ in range(bs)]
        dir_all = [(-e / np.linalg.norm(e)).astype(np.float32) for e in eyes for _ in range(bs)]
        texture = getattr(self, "texture", None)                 # tests/test_gpu_raster_grad.py calls this unbound, on a namespace with image_size alone
        return render_batch(vertices, faces, eye_all, dir_all, texture, image_size=self.image_size)

    def release_graphs(self):
        """Runner.train_clip_iteration's call at the top of every generator iteration: a graph-replayed encode_image that never reached backward
        does not hold its instance"""
        release = getattr(self.perceptor, "release_graphs", None)
        if release is not None:
            release()

    def get_pose_feature(self, pose, angles=None):
        """mean CLIP embedding of the posed body over the cameras -> [bs, 512]  (pose_generation.py:63-89)"""
        angles = DEFAULT_ANGLES if angles is None else tuple(angles)
        v = self.posed_vertices(pose)
        images = self.render_fn(v, self.smpl["faces"], angles)
        return clip_score.pose_feature(self.perceptor, images.to(self.device), len(angles))

    def calculate_pose_score(self, text, pose):
        return float(clip_score.pose_score(self.get_text_feature(text), self.get_pose_feature(pose)).reshape(-1)[0])

    def sort_poses_by_score(self, text, poses):
        """best first; every pose is scored ONCE (the reference's list.sort key renders each pose once as well)"""
        scores = [self.calculate_pose_score(text, p) for p in poses]
        return [poses[i] for i in sorted(range(len(poses)), key=lambda i: -scores[i])]


_NO_RENDERER_GRADIENT = ("%s optimises the CLIP score with respect to the pose THROUGH the rasteriser: it needs neural_renderer's backward pass (a hand-designed "
                         "pseudo-gradient), which this context does not enable (DESIGN.md section 8).  Build the context with "
                         "AnimateContext(..., renderer_gradient=True) (CLI: --renderer_gradient) to run it on the restated approximate gradient.  Available "
                         "without it: VPoserCodebook, VPoserRealNVP, MotionInterpolation, MotionOptimizer with clip_coef = 0 (the reference's "
                         "motion_ablation/baseline conf)")


def _needs_renderer_gradient(ctx, what):
    if not getattr(ctx, "renderer_gradient", False):
        raise NotImplementedError(_NO_RENDERER_GRADIENT % what)


class _ClipPoseOptimizer:
    """the loop PoseOptimizer / VPoserOptimizer share (pose_generation.py:115-128, :151-166): a parameter drawn on the host with torch.randn, the
    optimiser getattr(torch.optim, optim_name)(**optim_cfg), num_iteration steps of 1 - cos(mean CLIP embedding over the 5 cameras, text)"""
    DIM = 63

    def __init__(self, ctx, optim_name="Adam", optim_cfg=None, num_iteration=500, topk=5, name=None, smpl_path=None, vposer_path=None):
        self.ctx, self.name, self.topk = ctx, name or type(self).__name__, int(topk)
        self.optim_name, self.optim_cfg, self.num_iteration = optim_name, dict(optim_cfg or {"lr": 0.01}), int(num_iteration)

    def _pose_of(self, param):
        raise NotImplementedError

    def _result(self, param, last_pose):
        raise NotImplementedError

    def get_pose(self, text_feature):
        param = nn.Parameter(torch.randn(self.DIM))                       # drawn on the host, as the reference does
        opt = getattr(torch.optim, self.optim_name)([param], **self.optim_cfg)
        new_pose = None
        for _ in range(self.num_iteration):
            self.ctx.release_graphs()
            new_pose = self._pose_of(param)
            clip_feature = self.ctx.get_pose_feature(new_pose).squeeze(0)
            loss = (1 - F.cosine_similarity(clip_feature, text_feature, dim=-1)).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
        return self._result(param, new_pose)

    def get_topk_poses(self, text):
        tf = self.ctx.get_text_feature(text)
        poses = self.ctx.sort_poses_by_score(text, [self.get_pose(tf) for _ in range(self.topk)])
        return torch.stack(poses, dim=0)


class PoseOptimizer(_ClipPoseOptimizer):
    """pose_generation.py:102-135: the 63 body-pose values themselves are optimised; returns the parameter after its last step"""

    def __init__(self, ctx=None, **conf):
        _needs_renderer_gradient(ctx, "PoseOptimizer (pose_generation.py:102-135)")
        super().__init__(ctx, **conf)

    def _pose_of(self, param):
        return param.to(self.ctx.device)

    def _result(self, param, last_pose):
        return pose_padding(param.data).to(self.ctx.device)


class VPoserOptimizer(_ClipPoseOptimizer):
    """pose_generation.py:138-173: VPoser's 32-d latent is optimised; returns the pose decoded in the last iteration, before its step"""
    DIM = 32

    def __init__(self, ctx=None, **conf):
        _needs_renderer_gradient(ctx, "VPoserOptimizer (pose_generation.py:138-173)")
        super().__init__(ctx, **conf)

    def _pose_of(self, param):
        return self.ctx.vp.decode(param.to(self.ctx.device).unsqueeze(0))["pose_body"].contiguous().view(-1)

    def _result(self, param, last_pose):
        return pose_padding(last_pose.detach())


# ----------------------------------------------------------------------------------------------------------------- candidate poses
class VPoserCodebook:
    """pose_generation.py:288-329: the `pre_topk` codebook entries whose stored CLIP embedding is closest to the text, decoded by VPoser,
    near-duplicates (mean |difference| <= filter_threshold to an already kept pose) dropped, the first `topk` kept.  `codebook` [N,32] latent
    codes, `codebook_embedding` [N,512] (the reference's data/codebook.pth: pass its path as `codebook_path`, or the two tensors)."""

    def __init__(self, ctx, codebook=None, codebook_embedding=None, codebook_path="data/codebook.pth", topk=5, pre_topk=40, filter_threshold=0.07,
                 name="VPoserCodebook", smpl_path=None, vposer_path=None):       # (smpl_path / vposer_path: the reference's base-class keys; the assets are in `ctx`)
        self.ctx, self.name, self.topk, self.pre_topk, self.filter_threshold = ctx, name, int(topk), int(pre_topk), float(filter_threshold)
        if codebook is None:
            data = torch.load(codebook_path, map_location="cpu", weights_only=True)
            codebook, codebook_embedding = data["codebook"], data["codebook_embedding"]
        self.codebook = codebook.float().to(ctx.device)
        self.codebook_embedding = codebook_embedding.float().to(ctx.device)

    @staticmethod
    def suppress_duplicated_poses(poses, threshold):
        """greedy, in score order: keep a pose iff its mean absolute distance to EVERY kept pose exceeds the threshold"""
        kept = [0]
        for i in range(1, poses.shape[0]):
            d = (poses[i][None] - poses[kept]).abs().mean(-1)
            if float(min(d.min(), torch.tensor(10.0, device=d.device))) > threshold:
                kept.append(i)
        return poses[kept]

    @torch.no_grad()
    def get_topk_poses(self, text):
        tf = self.ctx.get_text_feature(text)
        score = F.cosine_similarity(self.codebook_embedding, tf[None]).reshape(-1)
        idx = torch.topk(score, self.pre_topk).indices
        poses = self.ctx.vp.decode(self.codebook[idx])["pose_body"].reshape(self.pre_topk, -1)
        return self.suppress_duplicated_poses(poses, self.filter_threshold)[: self.topk]


class VPoserRealNVP(nn.Module):
    """pose_generation.py:176-286: a conditional RealNVP over VPoser's 32-d latent, conditioned on the CLIP text feature; `num_batch` rounds of
    `num_sample` draws, each scored by rendering the decoded pose, the best kept; `topk` such poses, sorted.  Parameter names are the reference's
    (`s.{i}.{0,2,4}`, `t.{i}.{0,2,4}`, buffer `mask`), so data/pose_realnvp.pth's `state_dict` loads as it is."""

    def __init__(self, ctx, dim=32, hdim=256, num_block=8, num_sample=10, num_batch=50, ckpt_path=None, state_dict=None, topk=5, name="VPoserRealNVP",
                 smpl_path=None, vposer_path=None):
        super().__init__()
        self.ctx, self.name, self.topk = ctx, name, int(topk)
        self.dim, self.num_block, self.num_sample, self.num_batch = dim, num_block, num_sample, num_batch
        mask = (torch.randn(num_block, 1, dim) > 0).float()
        self.register_buffer("mask", mask)
        mlp = lambda last: nn.Sequential(nn.Linear(dim + 512, hdim), nn.LeakyReLU(), nn.Linear(hdim, hdim), nn.LeakyReLU(), nn.Linear(hdim, dim), *last)
        self.s, self.t = nn.ModuleList(), nn.ModuleList()
        for _ in range(num_block):            # (s_i then t_i, block by block: the reference's construction order, so that a seed reproduces its initialisation)
            self.s.append(mlp([nn.Tanh()]))
            self.t.append(mlp([]))
        if state_dict is None and ckpt_path is not None:
            state_dict = torch.load(ckpt_path, map_location="cpu", weights_only=True)["state_dict"]
        if state_dict is not None:
            self.load_state_dict(state_dict, strict=False)
        self.to(ctx.device).eval()

    def _coupling(self, x_kept, features, i):
        h = torch.cat([x_kept, features], dim=-1)
        free = 1 - self.mask[i]
        return self.s[i](h) * free, self.t[i](h) * free, free

    def decode(self, z, features):
        x = z
        for i in range(self.num_block):
            kept = x * self.mask[i]
            s, t, free = self._coupling(kept, features, i)
            x = kept + free * (x * torch.exp(s) + t)
        return x

    def encode(self, x, features):
        """inverse flow + log-determinant (training only in the reference)"""
        z, log_det = x, x.new_zeros(x.shape[0])
        for i in reversed(range(self.num_block)):
            kept = z * self.mask[i]
            s, t, free = self._coupling(kept, features, i)
            z = free * (z - t) * torch.exp(-s) + kept
            log_det = log_det - s.sum(dim=1)
        return z, log_det

    def sample(self, bs, features):
        z = torch.randn(bs, self.dim, device=self.mask.device)        # N(0, I): distributions.MultivariateNormal(0, I).sample of the reference
        return self.decode(z, features.reshape(1, -1).expand(bs, -1))

    @torch.no_grad()
    def get_pose(self, text_feature):
        tf = text_feature.reshape(1, -1)
        best, best_score = None, 0.0
        for _ in range(self.num_batch):
            poses = self.ctx.vp.decode(self.sample(self.num_sample, tf))["pose_body"].reshape(self.num_sample, -1)
            score = F.cosine_similarity(self.ctx.get_pose_feature(poses), tf)
            i = int(score.argmax())
            if float(score[i]) > best_score:
                best, best_score = poses[i], float(score[i])
        return best

    def get_topk_poses(self, text):
        tf = self.ctx.get_text_feature(text)
        poses = self.ctx.sort_poses_by_score(text, [self.get_pose(tf) for _ in range(self.topk)])
        return torch.stack(poses, dim=0)


# ----------------------------------------------------------------------------------------------------------------- motions
class MotionInterpolation:
    """motion_generation.py:100-137: the candidate poses encoded by VPoser, placed at the anchor frames, the latent code walked linearly between
    consecutive anchors, every frame decoded -> [num_frame, 69]"""

    def __init__(self, ctx, num_frame=60, anchor_position=(0, 14, 29, 44, 59), name="MotionInterpolation", smpl_path=None, vposer_path=None):
        self.ctx, self.name, self.num_frame, self.anchor_position = ctx, name, int(num_frame), tuple(int(a) for a in anchor_position)
        if self.anchor_position[0] != 0 or self.anchor_position[-1] != self.num_frame - 1:
            raise ValueError("the anchors start at frame 0 and end at the last frame")

    @torch.no_grad()
    def get_motion(self, text, poses):
        codes = self.ctx.vp.encode(poses[:, :63]).mean                        # [n_anchor, 32]
        z = codes.new_zeros(self.num_frame, codes.shape[-1])
        z[0] = codes[0]
        for k in range(1, len(self.anchor_position)):
            a, b = self.anchor_position[k - 1], self.anchor_position[k]
            step = (codes[k] - codes[k - 1]) / (b - a)
            for j in range(a, b):                                             # (accumulated step by step: the reference's fp32 summation order)
                z[j + 1] = z[j] + step
        return pose_padding(self.ctx.vp.decode(z)["pose_body"].reshape(self.num_frame, 63))


class SinusoidalPositionalEncoding(nn.Module):
    """buffer `pe` [max_len, 1, d] (motion_generation.py:140-157); the decoder uses its first `seq_len` rows as the queries"""

    def __init__(self, d_model, dropout=0.1, max_len=5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        pos = torch.arange(max_len, dtype=torch.float32)[:, None]
        freq = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
        pe = torch.zeros(max_len, d_model)
        pe[:, 0::2], pe[:, 1::2] = torch.sin(pos * freq), torch.cos(pos * freq)
        self.register_buffer("pe", pe[:, None, :])

    def forward(self, x):
        return self.dropout(x + self.pe[: x.shape[0]])


class MotionXTransformerEncoder(nn.Module):
    """ACTOR-style motion encoder (motion_generation.py:160-200); kept for checkpoint compatibility -- get_motion only decodes"""

    def __init__(self, seq_len=16, latent_dim=256, output_dim=256, num_heads=4, ff_size=1024, num_layers=8, activation="gelu", dropout=0.1):
        super().__init__()
        self.input_feats, self.seq_len, self.latent_dim = 55 * 6, seq_len, latent_dim
        self.skelEmbedding = nn.Linear(self.input_feats, latent_dim)
        self.pos_encoder = SinusoidalPositionalEncoding(latent_dim)
        self.query = nn.Parameter(torch.randn(1, latent_dim))
        layer = nn.TransformerEncoderLayer(d_model=latent_dim, nhead=num_heads, dim_feedforward=ff_size, dropout=dropout, activation=activation)
        self.seqTransEncoder = nn.TransformerEncoder(layer, num_layers=num_layers)
        self.final = nn.Linear(latent_dim, output_dim)

    def forward(self, motion):
        B, T = motion.shape[:2]
        tok = torch.cat([self.query.reshape(1, 1, -1).expand(B, 1, -1), self.skelEmbedding(motion.reshape(B, T, -1))], dim=1)
        return self.final(self.seqTransEncoder(self.pos_encoder(tok.permute(1, 0, 2).contiguous()))[0])


class MotionXTransformerDecoder(nn.Module):
    """latent [B, input_dim] -> 6-d rotations [B, seq_len, 55, 6] (motion_generation.py:203-246): the positional encodings of the frames are the
    queries, the latent code is the single memory token"""

    def __init__(self, seq_len=16, input_dim=256, latent_dim=256, num_heads=4, ff_size=1024, num_layers=8, activation="gelu", dropout=0.1):
        super().__init__()
        self.linear = nn.Linear(input_dim, latent_dim) if input_dim != latent_dim else nn.Identity()
        self.input_feats, self.seq_len, self.latent_dim = 55 * 6, seq_len, latent_dim
        self.pos_encoder = SinusoidalPositionalEncoding(latent_dim)
        layer = nn.TransformerDecoderLayer(d_model=latent_dim, nhead=num_heads, dim_feedforward=ff_size, dropout=dropout, activation=activation)
        self.seqTransDecoder = nn.TransformerDecoder(layer, num_layers=num_layers)
        self.final = nn.Linear(latent_dim, self.input_feats)

    def forward(self, latent):
        B, T = latent.shape[0], self.seq_len
        memory = self.linear(latent).reshape(1, B, -1)
        queries = self.pos_encoder.pe[:T].reshape(T, 1, -1).expand(T, B, -1)
        out = self.final(self.seqTransDecoder(tgt=queries, memory=memory))
        return out.permute(1, 0, 2).reshape(B, T, 55, 6)


class MotionOptimizer(nn.Module):
    """motion_generation.py:249-358: a latent code of the pretrained motion VAE optimised (Adam, 5 000 iterations) so that the decoded motion
    passes through the candidate poses IN ORDER (for candidate j the best-matching frame's 6-d rotation error, weighted recon_coef[j]) while the
    frame-to-frame change is REWARDED (- delta_coef x mse).  clip_coef > 0 adds clip_coef x the CLIP term of every clip_num_part-th frame
    (random phase) rendered at azimuth 150 through the rasteriser, which needs AnimateContext(renderer_gradient=True) (module docstring).  Decoder / encoder parameter names are the reference's: data/motion_vae.pth's `state_dict` loads as it is."""

    def __init__(self, ctx, num_frame=60, latent_dim=256, num_layers=4, num_heads=4, ckpt_path=None, state_dict=None, optim_name="Adam", optim_cfg=None,
                 num_iteration=5000, recon_coef=(1, 0.8, 0.6, 0.4, 0.2), clip_coef=0.001, delta_coef=0.01, clip_num_part=30, name="MotionOptimizer",
                 smpl_path=None, vposer_path=None):
        super().__init__()
        if float(clip_coef) > 0:
            _needs_renderer_gradient(ctx, "MotionOptimizer with clip_coef = %g (motion_generation.py:333-345)" % clip_coef)
        self.clip_coef, self.clip_num_part = float(clip_coef), int(clip_num_part)
        self.ctx, self.name, self.num_frame, self.latent_dim = ctx, name, int(num_frame), int(latent_dim)
        kw = dict(seq_len=self.num_frame, latent_dim=latent_dim, num_heads=num_heads, ff_size=latent_dim * 4, num_layers=num_layers)
        self.encoder = MotionXTransformerEncoder(output_dim=latent_dim, **kw)
        self.decoder = MotionXTransformerDecoder(input_dim=latent_dim, **kw)
        if state_dict is None and ckpt_path is not None:
            state_dict = torch.load(ckpt_path, map_location="cpu", weights_only=True)["state_dict"]
        if state_dict is not None:
            self.load_state_dict(state_dict, strict=False)
        self.optim_name, self.optim_cfg, self.num_iteration = optim_name, dict(optim_cfg or {"lr": 0.01}), int(num_iteration)
        self.recon_coef, self.delta_coef = tuple(float(c) for c in recon_coef), float(delta_coef)
        if self.num_iteration < 1:
            raise ValueError("num_iteration must be at least 1")
        self.to(ctx.device).eval()

    def decode(self, latent_code):
        """latent -> [num_frame, 63] axis-angle body pose (joints 1..21 of the 55 the VAE was trained on)"""
        rot6d = self.decoder(latent_code.reshape(-1, self.latent_dim)).reshape(-1, 6)
        aa = matrix_to_axis_angle(rotation_6d_to_matrix(rot6d)).reshape(-1, 165)
        return aa[:, 3:66].contiguous()

    def losses(self, motion, poses):
        """(reconstruction, delta) of a decoded motion [T,63] against candidate poses [k,63]"""
        r6 = lambda p: matrix_to_rotation_6d(axis_angle_to_matrix(p.reshape(p.shape[:-1] + (21, 3))))
        err = ((r6(motion)[None] - r6(poses)[:, None]) ** 2).mean(-1).mean(-1)          # [k, T]
        recon = (err.min(dim=1).values * torch.as_tensor(self.recon_coef[: poses.shape[0]], device=err.device, dtype=err.dtype)).sum()
        delta = F.mse_loss(motion[:-1], motion[1:])
        return recon, delta

    def clip_loss(self, motion, text_feature):
        """motion_generation.py:333-344: frames st_idx, st_idx + clip_num_part, ... (st_idx drawn from numpy's generator BEFORE the render's
        elevation draw) rendered at azimuth 150, 1 - cos against the text, weighted by their position in time"""
        self.ctx.release_graphs()
        st_idx = np.random.randint(self.clip_num_part)
        part_poses = motion[st_idx::self.clip_num_part].contiguous()
        feats = self.ctx.get_pose_feature(part_poses, (150,))
        return clip_score.motion_clip_loss(feats, text_feature, st_idx, self.clip_num_part, self.num_frame)

    def get_motion(self, text, poses):
        poses = poses[..., :63].contiguous().to(self.ctx.device)
        latent = nn.Parameter(torch.randn(self.latent_dim))               # drawn on the host, as the reference does
        opt = getattr(torch.optim, self.optim_name)([latent], **self.optim_cfg)
        motion = None
        text_feature = self.ctx.get_text_feature(text) if self.clip_coef > 0 else None
        for _ in range(self.num_iteration):
            motion = self.decode(latent.to(self.ctx.device))
            recon, delta = self.losses(motion, poses)
            if self.clip_coef > 0:
                loss = recon + self.clip_coef * self.clip_loss(motion, text_feature)
            else:
                loss = recon
            loss = loss - (delta * self.delta_coef if self.delta_coef > 0 else 0.0)
            opt.zero_grad()
            loss.backward()
            opt.step()
        return pose_padding(motion.detach()).to(self.ctx.device)


# ----------------------------------------------------------------------------------------------------------------- builder.py / main.py
POSE_GENERATORS = {"PoseOptimizer": PoseOptimizer, "VPoserOptimizer": VPoserOptimizer, "VPoserRealNVP": VPoserRealNVP, "VPoserCodebook": VPoserCodebook}
MOTION_GENERATORS = {"MotionInterpolation": MotionInterpolation, "MotionOptimizer": MotionOptimizer}


def build_pose_generator(conf, ctx, **assets):
    conf = dict(conf)
    name = conf.pop("type")
    return POSE_GENERATORS[name](ctx, name=name, **conf, **assets)


def build_motion_generator(conf, ctx, **assets):
    conf = dict(conf)
    name = conf.pop("type")
    return MOTION_GENERATORS[name](ctx, name=name, **conf, **assets)


def _write_previews(ctx, out_dir, poses, motion, size):
    """candidate_<i>.png (the front view of every candidate, all under ONE camera framed over all of them, so the pictures compare) and
    motion.gif (the fixed front camera, preview's default fps): the SMPL body of ctx.smpl posed by smpl_lbs.pose_hip, rendered by the preview
    rasteriser.  Draws nothing from any random generator and leaves its inputs alone."""
    from . import preview as P
    from . import smpl_lbs
    for name, p in (("candidate", poses), ("motion", motion)):
        if p is None or p.shape[0] == 0:
            continue
        body = torch.from_numpy(P.body_pose(p.detach().cpu().numpy()))
        v = smpl_lbs.pose_hip(ctx.smpl, body)
        eyes, ats, near, far = P.frame_cameras(v, 1, up="y")
        images = P.render_frames(v, ctx.smpl["faces"], None, eyes, ats, up="y", image_size=size, near=near, far=far)
        if name == "motion":
            P.save_frames(images, os.path.join(out_dir, "motion.gif"))
        else:
            for i in range(images.shape[0]):
                P.save_frames(images[i:i + 1], os.path.join(out_dir, "candidate_%d.png" % i))


def run(conf, ctx, pose_assets=None, motion_assets=None, preview=False, preview_size=512, pose_ctx=None):
    """main.py:14-41: candidate poses (saved as candidate_<i>.npy), then -- unless general.mode == 'pose' -- the motion (motion.npy).  The
    reference also writes pyrender pictures of them (candidate_<i>.jpg, motion.mp4; visualize.py render_pose / render_motion): with
    `preview` this writes candidate_<i>.png and motion.gif of `preview_size` pixels from the HIP posing kernel and the preview rasteriser
    (preview.py: its own camera framing and shading, not pyrender's; no .jpg / .mp4 encoder here).  Off by default; the returned tensors
    are the same either way.  `pose_ctx`: a second AnimateContext for the pose generator alone (pipeline.py: a pose codebook of ViT-B/32
    embeddings searched beside a ViT-B/16 main tower); None: `ctx`."""
    out_dir = conf.get_string("general.base_exp_dir")
    os.makedirs(out_dir, exist_ok=True)
    text = conf.get_string("general.text")
    poses = build_pose_generator(dict(conf["pose_generator"]), ctx if pose_ctx is None else pose_ctx, **(pose_assets or {})).get_topk_poses(text)
    for i in range(poses.shape[0]):
        np.save(os.path.join(out_dir, "candidate_%d.npy" % i), poses[i].detach().cpu().numpy())
    if conf.get_string("general.mode") == "pose":
        if preview:
            _write_previews(ctx, out_dir, poses, None, int(preview_size))
        return poses, None
    motion = build_motion_generator(dict(conf["motion_generator"]), ctx, **(motion_assets or {})).get_motion(text, poses=poses)
    np.save(os.path.join(out_dir, "motion.npy"), motion.detach().cpu().numpy())
    if preview:
        _write_previews(ctx, out_dir, poses, motion, int(preview_size))
    return poses, motion


def main(argv=None):
    """python -m avatarclip_amd.animate [--renderer_gradient] [--hip_posing] [--smpl_uv smpl_uv.obj] [--preview] --conf confs/base.conf --clip_weights ViT-B-32.pt --bpe bpe_simple_vocab_16e6.txt.gz --smpl SMPL_NEUTRAL.pkl
    --vposer data/vposer [--codebook data/codebook.pth] [--realnvp data/pose_realnvp.pth] [--motion_vae data/motion_vae.pth]
    (AvatarAnimate/main.py with the assets its constructors load named on the command line; VPoser itself comes from the `human_body_prior` package)"""
    import argparse
    from . import clip_vit, smpl_lbs, tokenizer
    from .conf import ConfigFactory
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--conf", default="./confs/base.conf")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--renderer_gradient", action="store_true",
                    help="differentiate the renders (neural_renderer's approximate backward, restated): PoseOptimizer, VPoserOptimizer and "
                         "MotionOptimizer with clip_coef > 0 (the reference's confs/base.conf) need it")
    ap.add_argument("--hip_posing", action="store_true",
                    help="pose the body with smpl_lbs.pose_hip_grad (HIP, forward and backward) instead of smpl_lbs.lbs: equal to fp32 rounding, "
                         "not bit for bit")
    ap.add_argument("--smpl_uv", default=None,
                    help="the textured body (data/smpl_uv.obj with its .mtl and image): every render that is scored or optimised shows it instead "
                         "of a white body, as AvatarAnimate/models/render.py:6-35 does; a precomputed codebook matches only if it was made with the "
                         "same texture")
    ap.add_argument("--preview", action="store_true", help="also write candidate_<i>.png and, in motion mode, motion.gif: the SMPL body in those poses")
    ap.add_argument("--preview_size", type=int, default=512)
    for name in ("clip_weights", "bpe", "smpl", "vposer"):
        ap.add_argument("--" + name, required=True)
    for name in ("codebook", "realnvp", "motion_vae"):
        ap.add_argument("--" + name, default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda", args.gpu)
    try:
        from human_body_prior.models.vposer_model import VPoser
        from human_body_prior.tools.model_loader import load_model
    except ImportError as e:
        raise SystemExit("the VPoser body prior comes from the `human_body_prior` package (pose_generation.py:15-16), which is not installed: %s" % e)
    vp, _ = load_model(args.vposer, model_code=VPoser, remove_words_in_model_weights="vp_model.", disable_grad=True)
    perceptor = clip_vit.ClipVisionB32({k: v.float() for k, v in clip_vit.load_state_dict(args.clip_weights).items()}, dev)
    tk = tokenizer.SimpleTokenizer(args.bpe)
    text_feature = lambda text: perceptor.encode_text(tokenizer.tokenize([text], tk))[0]
    ctx = AnimateContext(perceptor, text_feature, smpl_lbs.load_smpl_arrays(args.smpl, dev), vp.to(dev).eval(), device=dev,
                         renderer_gradient=args.renderer_gradient, posing="hip" if args.hip_posing else "torch", texture=args.smpl_uv)
    with open(args.conf) as fh:
        conf = ConfigFactory.parse_string(fh.read())
    pose_assets = {"codebook_path": args.codebook} if args.codebook else ({"ckpt_path": args.realnvp} if args.realnvp else {})
    run(conf, ctx, pose_assets=pose_assets, motion_assets={"ckpt_path": args.motion_vae} if args.motion_vae else {}, preview=args.preview,
        preview_size=args.preview_size)


if __name__ == "__main__":
    main()

