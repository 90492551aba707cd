"""Runner: the reference's optimisation driver with the same constructor, conf keys, modes and checkpoint
format (AvatarGen/AppearanceGen/main.py:30-632), running its per-iteration hot path on the gfx950 kernels.

Differences that are deliberate and documented:
  * view-sharded data parallelism (not in the reference, which is single-GPU): when torch.distributed is
    initialised every rank draws its own camera and ONE flat-bucket all-reduce (RCCL over xGMI) averages the
    gradients before the identical Adam step; `train.views_per_iter = V` sets the number of views per step
    independently of the number of ranks (rank r of W renders the views r, r + W, ... one after the other);
    `train.shard_view = true` instead cuts the rays of each view over the ranks by pixel range: every rank draws the same view and
    renders 1/W of it, which is the reference's one-view optimisation on W devices (_clip_loss_sharded);
  * the SMPL silhouette prior (smplx + neural_renderer, main.py:290-335,360) is rendered by the HIP rasteriser of
    smpl_prior.py from a posed mesh (`general.smpl_mesh`, an .obj, or `init_smpl(prior_renderer=...)`); the licensed SMPL
    pickles stay an input.  Seeded CLIP weights, seeded text embeddings, the procedural ellipsoid prior and a missing
    `train.pretrain` are STAND-INS for benchmarks and tests: they must be asked for (`allow_standins=True` /
    `general.allow_standins = True`), otherwise the Runner raises instead of training on meaningless inputs;
  * tensorboard logging is optional (absent offline) and scalar logging does not force a device sync every step;
  * `resume=True` continues an interrupted train / train_clip run draw for draw from a resume record written beside every checkpoint
    (the reference's `is_continue` loads the weights and starts the data streams and the iteration counter over; it is kept as it is);
    checkpoints and records are written under a temporary name and moved into place.
"""
import importlib
import logging
import os
import random
import types
from shutil import copyfile

import numpy as np
import torch
import torch.nn.functional as F

from .conf import ConfigFactory
from .dataset import SMPL_Dataset
from .fields import RenderingNetwork, SDFNetwork, SingleVarianceNetwork
from .renderer import NeuSRenderer
from .utils import lookat, random_at, random_eye, random_eye_normal, sphere_coord
from . import parallel
from . import h2d


class EllipsoidPrior:
    """Procedural stand-in for `render_one_batch(self.v, self.f, eye, at)` (models/utils.py:108-125): a Lambert-shaded
    ellipsoid 'body' rendered at 256x256 with the dataset's 60-degree camera.  Only used when no SMPL prior renderer is
    supplied (licensed SMPL files and neural_renderer are not available offline)."""

    def __init__(self, radii=(0.28, 0.85, 0.2), res=256, fov=np.pi / 3, device="cuda"):
        self.radii = torch.tensor(radii, dtype=torch.float32, device=device)
        self.res, self.focal, self.device = res, 0.5 * res / np.tan(0.5 * fov), device

    def __call__(self, eye, at):
        pose = torch.from_numpy(lookat(np.asarray(eye, np.float64), np.asarray(at, np.float64), np.array([0., 1, 0]))).float().to(self.device)
        t = torch.linspace(0, self.res - 1, self.res, device=self.device)
        px, py = torch.meshgrid(t, t, indexing="ij")
        px, py = px.t(), py.t()
        p = torch.stack([(px - 0.5 * self.res) / self.focal, -(py - 0.5 * self.res) / self.focal, -torch.ones_like(px)], -1)
        d = p / p.norm(dim=-1, keepdim=True)
        d = torch.sum(d[..., None, :] * pose[:3, :3], -1)
        o = pose[:3, 3]
        od, dd = o / self.radii, d / self.radii
        a, b, c = (dd * dd).sum(-1), 2 * (od * dd).sum(-1), (od * od).sum() - 1
        disc = b * b - 4 * a * c
        hit = disc > 0
        tt = (-b - torch.sqrt(disc.clamp(min=0))) / (2 * a)
        n = (o + d * tt[..., None]) / self.radii ** 2
        n = n / n.norm(dim=-1, keepdim=True).clamp(min=1e-6)
        shade = (0.35 + 0.65 * (-(n * d).sum(-1)).clamp(0, 1)) * hit
        return shade[..., None].repeat(1, 1, 3)


class ScalarLog:
    """main.py:102 (`SummaryWriter(log_dir=os.path.join(base_exp_dir, 'logs'))`) without tensorboard (absent offline): the same
    `add_scalar(tag, value, step)` calls, written as JSON lines to <base_exp_dir>/logs/scalars.jsonl.  The values stay device
    tensors until `flush()` (one host transfer per report interval, not one per scalar and step)."""

    def __init__(self, log_dir):
        os.makedirs(log_dir, exist_ok=True)
        self.path = os.path.join(log_dir, "scalars.jsonl")
        self.pending = []

    def add_scalar(self, tag, value, step):
        self.pending.append((tag, value.detach() if torch.is_tensor(value) else value, int(step)))

    def flush(self):
        if not self.pending:
            return
        import json
        with open(self.path, "a") as fh:
            for tag, v, step in self.pending:
                fh.write(json.dumps({"tag": tag, "value": float(v), "step": step}) + "\n")
        self.pending = []


class Runner:
    def __init__(self, conf_path, mode="train", case="CASE_NAME", is_continue=False, is_colab=False, conf=None,
                 device=None, data_root=None, allow_standins=None, views_per_iter=None, shard_view=None, resume=False, resume_tag=None):
        """`resume`: continue the run that was interrupted in this base_exp_dir -- the newest checkpoint whose resume records
        (<base_exp_dir>/resume/, one per rank, written beside every checkpoint) are complete and carry `resume_tag`: networks, Adam state
        and iter_step as `is_continue` loads them, and at the top of train() / train_clip() the data streams, the per-view streams, the
        image permutation and the iteration counter, so that the run goes on draw for draw.  Without such a checkpoint the run starts
        at step 0.  `resume_tag`: an opaque string written into this run's records; a record with another tag is never continued."""
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("avatarclip_amd.Runner needs an MI355X (torch.cuda) -- the hot path has no CPU fallback")
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        self.conf_path = conf_path
        if is_colab or conf is not None:
            self.conf = conf
        else:
            with open(self.conf_path) as f:
                self.conf = ConfigFactory.parse_string(f.read())
        self.rank, self.world = parallel.rank_world()
        # train.views_per_iter: camera views per optimisation step over ALL ranks (default: one per rank).  The argument overrides the conf.
        V = self.conf.get_int("train.views_per_iter", default=None) if views_per_iter is None else views_per_iter
        # train.shard_view: the rays of ONE view are cut over the ranks by pixel range instead of every rank
        # rendering views of its own.  All ranks then build the same views from the same data streams: for the views, the job is one
        # process (_view_rank of _view_world), and views_per_iter defaults to 1.  The argument overrides the conf.
        self.shard_view = bool(self.conf.get_bool("train.shard_view", default=False) if shard_view is None else shard_view)
        if self.shard_view and mode == "train":
            raise ValueError("train.shard_view with mode 'train': that mode draws pixels of stored images, not camera views; "
                             "the key applies to mode 'train_clip' only")
        self._view_rank, self._view_world = (0, 1) if self.shard_view else (self.rank, self.world)
        self._shard_group = parallel.shard_group() if self.shard_view else None     # None: one rank, nothing to cut
        self._gather_pixels = parallel.PixelGather()
        if self.shard_view:
            self.views_per_iter = 1 if V is None else int(V)
            if self.views_per_iter <= 0:
                raise ValueError("train.views_per_iter = %d must be positive (train.shard_view: each view is cut over all %d ranks)"
                                 % (self.views_per_iter, self.world))
        else:
            self.views_per_iter = self.world if V is None else int(V)
        if self.views_per_iter <= 0 or self.views_per_iter % self._view_world != 0:
            raise ValueError("train.views_per_iter = %d must be a positive multiple of the world size %d (rank r renders the views r, r + %d, ...)"
                             % (self.views_per_iter, self.world, self.world))
        if mode == "train" and self.views_per_iter != self.world:
            raise ValueError("train.views_per_iter = %d with world size %d: mode 'train' draws pixels of stored images, not camera views; "
                             "the key applies to mode 'train_clip' only" % (self.views_per_iter, self.world))
        self.allow_standins = bool(self.conf.get_bool("general.allow_standins", default=False)
                                   if allow_standins is None else allow_standins)
        self.base_exp_dir = self.conf["general.base_exp_dir"]
        os.makedirs(self.base_exp_dir, exist_ok=True)
        ds_conf = self.conf.get("dataset", default=None)
        if data_root is not None and ds_conf is not None and "data_dir" in ds_conf:
            ds_conf.put("data_dir", os.path.join(data_root, ds_conf["data_dir"]))
        self.dataset = SMPL_Dataset(ds_conf, device=self.device, load_images=(mode == "train"),
                                    H=self.conf.get_int("dataset.H", default=None) if ds_conf is not None else None,
                                    W=self.conf.get_int("dataset.W", default=None) if ds_conf is not None else None)
        self.iter_step = 0
        c = self.conf
        # Training parameters (main.py:50-62)
        self.end_iter = c.get_int("train.end_iter")
        self.save_freq = c.get_int("train.save_freq")
        self.report_freq = c.get_int("train.report_freq")
        self.val_freq = c.get_int("train.val_freq")
        self.val_mesh_freq = c.get_int("train.val_mesh_freq")
        self.batch_size = c.get_int("train.batch_size")
        self.validate_resolution_level = c.get_int("train.validate_resolution_level")
        self.learning_rate = c.get_float("train.learning_rate")
        self.learning_rate_alpha = c.get_float("train.learning_rate_alpha")
        self.use_white_bkgd = c.get_bool("train.use_white_bkgd")
        self.warm_up_end = c.get_float("train.warm_up_end", default=0.0)
        self.anneal_end = c.get_float("train.anneal_end", default=0.0)
        self.max_ray_num = c.get_int("train.max_ray_num", default=112 * 112)
        self.igr_weight = c.get_float("train.igr_weight")
        self.mask_weight = c.get_float("train.mask_weight")
        # optional keys with the reference's defaults (main.py:67-127)
        self.clip_weight = c.get_float("train.clip_weight", default=None)
        self.extra_color = c.get_bool("model.rendering_network.extra_color", default=False)
        self.add_no_texture = c.get_bool("train.add_no_texture", default=False)
        self.texture_cast_light = c.get_bool("train.texture_cast_light", default=False)
        self.use_face_prompt = c.get_bool("train.use_face_prompt", default=False)
        self.use_back_prompt = c.get_bool("train.use_back_prompt", default=False)
        self.use_silhouettes = c.get_bool("train.use_silhouettes", default=False)
        self.head_height = c.get_float("train.head_height", default=0.65)
        self.use_bg_aug = c.get_bool("train.use_bg_aug", default=True)
        self.full_frame_resolution_level = c.get_float("train.full_frame_resolution_level", default=2.25)  # main.py:371
        seed = c.get_int("train.seed", default=None)
        self.seed = seed
        if seed is not None:
            torch.manual_seed(seed); torch.cuda.manual_seed_all(seed); random.seed(seed); np.random.seed(seed)
        self.smpl_model_path = c.get_string("general.smpl_model_path", default="../../smpl_models")
        self.pose_type = c.get_string("general.pose_type", default="stand_pose")
        assert self.pose_type in ["stand_pose", "t_pose"]
        self.is_continue = is_continue
        self.mode = mode
        self.writer = None

        # Networks (main.py:133-151); every rank builds identical weights (same torch seed / same checkpoint)
        self.nerf_outside = None
        self.sdf_network = SDFNetwork(**self.conf["model.sdf_network"]).to(self.device)
        self.deviation_network = SingleVarianceNetwork(**self.conf["model.variance_network"]).to(self.device)
        self.color_network = RenderingNetwork(**self.conf["model.rendering_network"]).to(self.device)
        params_to_train = list(self.sdf_network.parameters()) + list(self.deviation_network.parameters()) + \
            list(self.color_network.parameters())
        self.params_to_train = params_to_train
        several = self.views_per_iter != self._view_world     # more than one view per rank and step
        if parallel.is_on():
            parallel.broadcast_params(params_to_train)
        if parallel.is_on() or several:
            self.seed_data_rngs()
        self._view_rngs = self._fresh_view_rngs() if several else []
        self.last_views, self.last_view_losses = [], []      # this rank's views of the last step in render order, and their losses
        self.grad_bucket = parallel.GradBucket(params_to_train) if parallel.is_on() or several else None
        # main.py:145; fused = the same update in ONE launch for all 28 tensors instead of a dozen multi-tensor launches
        self.optimizer = torch.optim.Adam(params_to_train, lr=self.learning_rate, fused=(self.device.type == "cuda"))
        self.renderer = NeuSRenderer(self.nerf_outside, self.sdf_network, self.deviation_network, self.color_network,
                                     **self.conf["model.neus_renderer"])
        pretrain_pth = c.get_string("train.pretrain", default=None)
        if pretrain_pth is not None:
            if os.path.exists(pretrain_pth):
                logging.info("Load pretrain: {}".format(pretrain_pth))
                self.load_pretrain(pretrain_pth)
            elif self.allow_standins:
                logging.warning("pretrain %s not found -- starting from the geometric initialisation (stand-in)", pretrain_pth)
            else:
                raise FileNotFoundError("train.pretrain = %s does not exist (the reference fails here too, main.py:153-155); "
                                        "set general.allow_standins = True to start from the geometric initialisation"
                                        % pretrain_pth)
        latest_model_name = None
        self.resume_tag = "" if resume_tag is None else str(resume_tag)
        self.resumed_from = None          # the step a resume=True run continued from (None: it started where any other run starts)
        self._resume_record = None        # this rank's record of that step until train() / train_clip() has put it in place
        self._image_perm = self._next_iter_i = None      # train()'s permutation / train_clip()'s counter, for the record
        if resume:
            step = self._find_resume_step()
            if step is None:
                logging.info("resume: no checkpoint with complete resume records tagged %r under %s -- starting from step 0",
                             self.resume_tag, self.base_exp_dir)
            else:
                latest_model_name = "ckpt_{:0>6d}.pth".format(step)
                self._resume_record = self._read_resume_record(step, self.rank)
                self.resumed_from = step
        elif is_continue:
            model_list = [m for m in os.listdir(os.path.join(self.base_exp_dir, "checkpoints"))
                          if m[-3:] == "pth" and int(m[5:-4]) <= self.end_iter]
            model_list.sort()
            latest_model_name = model_list[-1]
        if latest_model_name is not None:
            logging.info("Find checkpoint: {}".format(latest_model_name))
            self.load_checkpoint(latest_model_name)
        if self.mode[:5] == "train" and self.rank == 0 and conf_path is not None and os.path.exists(str(conf_path)):
            self.file_backup()
        self.perceptor = None
        self.prior_renderer = None
        self.overlap_view = True      # silhouette mode on the GPU: build the iteration's view on a second HIP stream (_take_view)
        self._side_stream = None      # that stream (make_view_on_side_stream), made on first use

    def seed_data_rngs(self):
        """View-sharded data parallelism: the weights are identical on every rank (broadcast), the DATA must not be.  The
        reference seeds numpy / random / torch once (main.py:104-116); with that alone every rank would draw the same
        cameras, backgrounds, lights, image permutations, pixels and z-jitter and the all-reduce would average N identical
        gradients.  Rank r > 0 re-seeds its data RNGs with seed + r (rank 0 keeps the single-GPU stream); without
        train.seed a base seed is drawn on rank 0 and broadcast (without a process group: drawn here).  With train.views_per_iter = V
        the streams belong to the VIEWS: view j of a step draws from the streams seeded base + j, whichever rank renders it; the
        process's own streams are those of its first view, j = rank (_fresh_view_rngs makes the others).  With train.shard_view every
        rank builds every view, so every rank is rank 0 here: one set of streams, those of a single process."""
        base = self.seed
        if base is None:
            t = torch.tensor([int(np.random.randint(0, 2 ** 31 - 1))], dtype=torch.int64, device=self.device)
            parallel.broadcast_tensor(t)
            base = int(t.item())
        self.base_seed = base
        self.data_seed = base + self._view_rank
        if self._view_rank > 0 or self.seed is None:
            np.random.seed(self.data_seed); random.seed(self.data_seed)
            torch.manual_seed(self.data_seed)
            if self.device.type == "cuda":
                torch.cuda.manual_seed(self.data_seed)

    def _data_rng_state(self):
        """the four data streams of a view (numpy, random, torch on the host, torch on this device).  Host work only: the device
        generator's state is a seed and an offset kept on the host, so neither direction waits for the GPU."""
        return (np.random.get_state(), random.getstate(), torch.get_rng_state(),
                torch.cuda.get_rng_state(self.device) if self.device.type == "cuda" else None)

    def _set_data_rng_state(self, state):
        np.random.set_state(state[0]); random.setstate(state[1]); torch.set_rng_state(state[2])
        if state[3] is not None:
            torch.cuda.set_rng_state(state[3], self.device)

    def _fresh_view_rngs(self):
        """stream sets of this rank's views after its first, j = rank + k * world (k >= 1): freshly seeded with base + j by the calls
        seed_data_rngs makes, taken as states, the process's own streams put back"""
        mine = self._data_rng_state()
        out = []
        for j in range(self._view_rank + self._view_world, self.views_per_iter, self._view_world):
            np.random.seed(self.base_seed + j); random.seed(self.base_seed + j)
            torch.manual_seed(self.base_seed + j)
            if self.device.type == "cuda":
                torch.cuda.manual_seed(self.base_seed + j)
            out.append(self._data_rng_state())
        self._set_data_rng_state(mine)
        return out

    def _validation_hooks(self, clip_stage):
        """main.py:247-251 / 556-561: periodic images and meshes (rank 0)."""
        if self.rank != 0:
            return
        # train.shard_view: the ranks cut the SAME view, so their data streams must stay in step; what rank 0 alone draws here (the
        # validation camera, the jitter of its render) is taken from a copy of the streams and the streams are put back
        held = self._data_rng_state() if self._shard_group is not None else None
        try:
            if self.val_freq > 0 and self.iter_step % self.val_freq == 0:
                if clip_stage:
                    self.validate_image(idx=58 if self.dataset.n_images > 58 else -1, save=True)
                else:
                    self.validate_image(save=True)
            if self.val_mesh_freq > 0 and self.iter_step % self.val_mesh_freq == 0:
                self.validate_mesh()
        finally:
            if held is not None:
                self._set_data_rng_state(held)

    def _after_step(self, loss, clip_stage):
        """main.py:240-253 / 549-563: report, checkpoint, validation, next learning rate"""
        if self.iter_step % self.report_freq == 0 and self.rank == 0:
            if clip_stage:
                print(self.base_exp_dir)
            print("iter:{:8>d} loss = {} lr={}".format(self.iter_step, loss.item(), self.optimizer.param_groups[0]["lr"]))
        saving = self.iter_step % self.save_freq == 0
        if saving and self.rank == 0:
            self.save_checkpoint()
        self._validation_hooks(clip_stage)
        self.update_learning_rate()
        if saving:      # here and not beside save_checkpoint: the hooks above draw from the data streams, and no view is in flight
            self.save_resume_record()

    def _zero_grad(self):
        self.optimizer.zero_grad(set_to_none=self.grad_bucket is None)

    def _reduce_and_step(self, views=None):
        """one RCCL all-reduce of the flat gradient bucket (K17) and the mean over the step's views, the Adam step"""
        if self.grad_bucket is not None:
            self.grad_bucket.allreduce_mean(views)
        self.optimizer.step()
        self.iter_step += 1

    def _optimizer_step(self, loss):
        """main.py:226-230 / 536-540: backward, the all-reduce, the Adam step"""
        self._zero_grad()
        loss.backward()
        self._reduce_and_step()

    def _white_background(self):
        return torch.ones([1, 3], device=self.device)

    def _loss_mask(self, mask):
        """main.py:196-199 / 407-410"""
        return (mask > 0.5).float() if self.mask_weight > 0.0 else torch.ones_like(mask)

    # ------------------------------------------------------------------ NeuS-init stage (main.py:180-256)
    def train(self):
        self._open_writer()
        self.update_learning_rate()
        res_step = self.end_iter - self.iter_step
        record = self._restore_resume_record()
        if record is not None and record["image_perm"] is not None:
            # the interrupted epoch's permutation, without the start-of-run draw; a record taken at an epoch's last step precedes the
            # reshuffle the uninterrupted run made right after it: that draw is made here, from the restored streams
            self._image_perm = record["image_perm"]
            if self.iter_step % len(self._image_perm) == 0:
                self._image_perm = self.get_image_perm()
        else:
            self._image_perm = self.get_image_perm()
        for _ in range(res_step):
            image_perm = self._image_perm
            data = self.dataset.gen_random_rays_at(image_perm[self.iter_step % len(image_perm)], self.batch_size)
            self._after_step(self.train_iteration(data), clip_stage=False)
            if self.iter_step % len(image_perm) == 0:
                self._image_perm = self.get_image_perm()
        if self.writer is not None:
            self.writer.flush()

    def train_iteration(self, data):
        rays_o, rays_d, true_rgb, mask = data[:, :3], data[:, 3:6], data[:, 6:9], data[:, 9:10]
        near, far = self.dataset.near_far_from_sphere(rays_o, rays_d)
        background_rgb = self._white_background() if self.use_white_bkgd else None
        mask = self._loss_mask(mask)
        mask_sum = mask.sum() + 1e-5
        render_out = self.renderer.render(rays_o, rays_d, near, far, background_rgb=background_rgb,
                                          cos_anneal_ratio=self.get_cos_anneal_ratio())
        color_error = (render_out["color_fine"] - true_rgb) * mask
        color_fine_loss = F.l1_loss(color_error, torch.zeros_like(color_error), reduction="sum") / mask_sum
        mask_loss = F.binary_cross_entropy(render_out["weight_sum"].clip(1e-3, 1.0 - 1e-3), mask)
        loss = color_fine_loss + render_out["gradient_error"] * self.igr_weight + mask_loss * self.mask_weight
        self._optimizer_step(loss)
        if self.writer is not None:   # main.py:216,230-238
            with torch.no_grad():
                psnr = 20.0 * torch.log10(1.0 / (((render_out["color_fine"] - true_rgb) ** 2 * mask).sum() / (mask_sum * 3.0)).sqrt())
                for tag, v in (("Loss/loss", loss), ("Loss/color_loss", color_fine_loss), ("Loss/eikonal_loss", render_out["gradient_error"]),
                               ("Statistics/s_val", render_out["s_val"][:1].mean()),
                               ("Statistics/cdf", (render_out["cdf_fine"][:, :1] * mask).sum() / mask_sum),
                               ("Statistics/weight_max", (render_out["weight_max"] * mask).sum() / mask_sum), ("Statistics/psnr", psnr)):
                    self.writer.add_scalar(tag, v, self.iter_step)
            if self.iter_step % self.report_freq == 0:
                self.writer.flush()
        return loss.detach()

    # ------------------------------------------------------------------ CLIP stage set-up (main.py:258-335)
    def _standin(self, what):
        if not self.allow_standins:
            raise RuntimeError("%s is missing and stand-ins are not allowed for this run (pass allow_standins=True or set "
                               "general.allow_standins = True for benchmarks / tests)" % what)
        logging.warning("%s is missing: using the seeded / procedural stand-in", what)

    def init_clip(self, perceptor=None, text_embeddings=None, clip_state_dict=None, tokenizer=None):
        """`tokenizer`: an already built tokenizer.SimpleTokenizer for the prompts of the conf (pipeline.py shares one over its stages);
        None: built here from clip.bpe_path / $AVC_CLIP_BPE when the perceptor carries a text tower"""
        from . import clip_vit
        if perceptor is None:
            if clip_state_dict is None:
                path = self.conf.get_string("clip.weights", default=None) or os.environ.get("AVC_CLIP_WEIGHTS")
                if path is not None and os.path.exists(path):
                    clip_state_dict = clip_vit.load_state_dict(path)
                else:
                    self._standin("the CLIP ViT-B/32 or ViT-B/16 state dict (clip.weights / $AVC_CLIP_WEIGHTS)")
                    clip_state_dict = clip_vit_random_state_dict(0)
            perceptor = clip_vit.ClipVisionB32(clip_state_dict, self.device)
        self.perceptor = perceptor
        self.clip_preprocess = clip_vit.clip_preprocess
        te = text_embeddings or {}

        if tokenizer is None and getattr(perceptor, "_text_sd", None) is not None:
            try:
                from .tokenizer import SimpleTokenizer
                tokenizer = SimpleTokenizer(self.conf.get_string("clip.bpe_path", default=None))
            except FileNotFoundError as e:
                logging.warning("%s", e)

        def emb(key, seed):
            if key in te:
                return te[key].to(self.device).float().reshape(1, -1)
            text = self.conf.get_string("clip." + key, default=None)
            if tokenizer is not None and text is not None:
                # main.py:272-288: clip.tokenize + perceptor.encode_text, detached
                from .tokenizer import tokenize
                print("%s: %s" % (key, text))
                return self.perceptor.encode_text(tokenize([text], tokenizer)).detach()
            self._standin("the text embedding of clip.%s (needs the full CLIP weights + the BPE table, or text_embeddings=)" % key)
            g = torch.Generator().manual_seed(seed)
            v = torch.randn(1, 512, generator=g)
            return (v / v.norm()).to(self.device)
        self.encoded_text = emb("prompt", 11)
        if self.use_face_prompt:
            self.encoded_face_text = emb("face_prompt", 12)
        if self.use_back_prompt:
            self.encoded_back_text = emb("back_prompt", 13)

    def init_smpl(self, prior_renderer=None):
        """main.py:290-335: the posed SMPL body whose renders supervise colour and mask.  `prior_renderer(eye, at)` returns
        the [256,256,3] render of `render_one_batch` (models/utils.py:108-125).  Sources, in order: the argument; the conf
        key `general.smpl_prior = module:callable` (called with this Runner); `general.smpl_mesh = <posed mesh .obj>`
        rendered by the HIP rasteriser (smpl_prior.MeshPrior); else the procedural ellipsoid -- a stand-in."""
        if prior_renderer is None:
            spec = self.conf.get_string("general.smpl_prior", default=None)
            mesh_path = self.conf.get_string("general.smpl_mesh", default=None)
            if spec is not None:
                mod, fn = spec.split(":")
                prior_renderer = getattr(importlib.import_module(mod), fn)(self)
            elif mesh_path is not None:
                from . import smpl_prior
                prior_renderer = smpl_prior.MeshPrior.from_obj(mesh_path, device=self.device)
            else:
                self._standin("the SMPL prior (general.smpl_mesh / general.smpl_prior / init_smpl(prior_renderer=...))")
                prior_renderer = EllipsoidPrior(device=self.device)
        self.prior_renderer = prior_renderer

    # ------------------------------------------------------------------ CLIP-guided loop (main.py:337-566)
    def _open_writer(self):
        """main.py:102: the scalar log of a training run (rank 0; `general.log_scalars = False` turns it off)"""
        if self.writer is None and self.rank == 0 and self.conf.get_bool("general.log_scalars", default=True):
            self.writer = ScalarLog(os.path.join(self.base_exp_dir, "logs"))

    def train_clip(self):
        self._open_writer()
        self.update_learning_rate()
        res_step = self.end_iter - self.iter_step
        record = self._restore_resume_record()
        # (a resumed run counts on from the interrupted run's iter_i: the face camera, the prompt choice and the stop below stay in phase)
        first = 0 if record is None or record["iter_i"] is None else int(record["iter_i"])
        for iter_i in range(first, first + res_step):
            if iter_i == 30010:  # main.py:346-347
                break
            self._next_iter_i = iter_i + 1
            self._after_step(self.train_clip_iteration(iter_i), clip_stage=True)
        if self.writer is not None:
            self.writer.flush()

    def sample_camera(self, iter_i):
        """main.py:348-359 (host numpy RNG, same draw order)."""
        if self.use_face_prompt and iter_i % 4 == 0:
            eye, theta, phi, is_front = random_eye(is_front=1, distance=0.4, theta_std=np.pi / 12)
            at = np.array([0, self.head_height, 0.3]).astype(np.float32)
        else:
            eye, theta, phi, is_front = random_eye_normal()
            at = random_at().astype(np.float32)
        eye = eye.astype(np.float32) + at
        return eye, at, theta, phi, is_front

    # The iteration is split into the stages of main.py so that each stage can be driven with injected inputs by the parity
    # tests (tests/test_glue_golden.py runs the glue on fixtures produced by the reference's own lines):
    #   make_view (main.py:348-385) -> draw_background (:387-415) -> renderer.render (:417-420)
    #   -> shade_and_scatter (:422-487) -> assemble_loss (:489-534) -> backward / all-reduce / Adam (:536-538)
    # On the GPU the view's rays, the chess-board background and shading + loss come out of one launch each; on the CPU the torch
    # statements of the same reference lines run (and serve tests/test_gpu_glue.py as the parity references).  The device alone chooses.
    def _view_head_fused(self, pose, prior):
        """rays + near / far + the prior resampled to the ray grid in one launch (dataset.rays_fused) instead of ~45"""
        dilated_mask = sel_idx = None
        if self.use_silhouettes:
            grid = self.dataset.silhouette_grid(self.max_ray_num, prior[..., 0])
            if grid is None:
                raise RuntimeError("the prior render of this view is empty: no silhouette to sample rays in (dataset.py:262-263)")
            W, dilated_mask, sel_idx = grid
            H = W
        else:
            W, H = int(self.dataset.W // self.full_frame_resolution_level), int(self.dataset.H // self.full_frame_resolution_level)
        rays_o, rays_d, near, far, true_rgb, mask = self.dataset.rays_fused(pose, W, H, sel_idx, prior.reshape(prior.shape[0], prior.shape[1], 3))
        return H, W, rays_o, rays_d, near, far, true_rgb, mask, dilated_mask, sel_idx

    def _view_head_torch(self, pose, prior):
        """main.py:360-380 as torch statements: the parity reference of the fused head, and the CPU path"""
        dilated_mask = sel_idx = None
        if self.use_silhouettes:
            self.dataset.last_sel_idx = None
            rays_o, rays_d, W, dilated_mask = self.dataset.gen_rays_silhouettes(pose, self.max_ray_num, (prior != 0).float()[..., 0])
            sel_idx = self.dataset.last_sel_idx
            H = W
            rays_o, rays_d = rays_o.float(), rays_d.float()
        else:
            rays_o, rays_d = self.dataset.gen_rays_pose(pose, self.full_frame_resolution_level)
            H, W = rays_o.shape[0], rays_o.shape[1]
            rays_o, rays_d = rays_o.reshape(H * W, 3).float(), rays_d.reshape(H * W, 3).float()
        Hp, Wp = prior.shape[0], prior.shape[1]
        true_rgb = F.interpolate(prior.reshape(Hp, Wp, 3).permute(2, 0, 1).unsqueeze(0), size=(H, W)) \
            .squeeze(0).permute(1, 2, 0).reshape(-1, 3)                                        # main.py:376-377 (nearest)
        mask = (true_rgb != 0).float()[..., :1]
        near, far = self.dataset.near_far_from_sphere(rays_o, rays_d)
        return H, W, rays_o, rays_d, near, far, true_rgb, mask, dilated_mask, sel_idx

    def make_view(self, iter_i, camera=None, head=None):
        """`head`: _view_head_fused or _view_head_torch (default: by device)"""
        dev = self.device
        eye, at, theta, phi, is_front = camera if camera is not None else self.sample_camera(iter_i)
        pose = h2d.upload(lookat(eye, at, np.array([0, 1, 0])), dev)
        prior = torch.as_tensor(self.prior_renderer(eye, at), dtype=torch.float32, device=dev)
        if head is None:
            head = self._view_head_fused if dev.type == "cuda" else self._view_head_torch
        H, W, rays_o, rays_d, near, far, true_rgb, mask, dilated_mask, sel_idx = head(pose, prior)
        ray_of_pixel = None
        if sel_idx is not None and dev.type == "cuda":     # pixel -> ray (or -1): what the fused glue scatters with (glue.ShadeLossFn)
            ray_of_pixel = torch.full((H * W,), -1, dtype=torch.int32, device=dev)
            ray_of_pixel[sel_idx] = torch.arange(sel_idx.numel(), dtype=torch.int32, device=dev)
        view = types.SimpleNamespace(eye=eye, at=at, theta=theta, phi=phi, is_front=is_front, pose=pose, H=H, W=W,
                                     rays_o=rays_o, rays_d=rays_d, near=near, far=far, true_rgb=true_rgb, mask=mask,
                                     dilated_mask=dilated_mask, sel_idx=sel_idx, ray_of_pixel=ray_of_pixel, mask_binary=True)
        if self._shard_group is not None:      # (here, so that the silhouette mode's cut positions come to the host with the view's other round trips)
            view.ray_cuts, view.pixel_cuts = parallel.shard_ranges(self.world, H * W, sel_idx)
        return view

    def shard_of_view(self, view, rank=None):
        """train.shard_view: rank `rank`'s part of `view` -- the rays [q0, q1) and the row-major pixels [p0, p1) of parallel.shard_ranges --
        as a view of its own whose tensors are slices.  Its pixel grid is the range itself, H = p1 - p0 rows of W = 1 pixel, with
        sel_idx / ray_of_pixel / dilated_mask local to it, so that the per-pixel statements (shade_and_scatter, glue.ShadeLossFn)
        apply unchanged; `full_hw` and `pixel_cuts` say where the range lies in the image that CLIP sees."""
        r = self.rank if rank is None else rank
        (q0, q1), (p0, p1) = view.ray_cuts[r:r + 2], view.pixel_cuts[r:r + 2]
        n = p1 - p0
        sel_idx = ray_of_pixel = dilated_mask = None
        if view.sel_idx is not None:
            sel_idx = view.sel_idx[q0:q1] - p0
            dilated_mask = view.dilated_mask.reshape(-1)[p0:p1].reshape(n, 1)
            if view.ray_of_pixel is not None:
                ray_of_pixel = torch.full((n,), -1, dtype=torch.int32, device=self.device)
                ray_of_pixel[sel_idx] = torch.arange(q1 - q0, dtype=torch.int32, device=self.device)
        return types.SimpleNamespace(eye=view.eye, at=view.at, theta=view.theta, phi=view.phi, is_front=view.is_front, pose=view.pose, H=n, W=1,
                                     rays_o=view.rays_o[q0:q1], rays_d=view.rays_d[q0:q1], near=view.near[q0:q1], far=view.far[q0:q1],
                                     true_rgb=view.true_rgb[p0:p1], mask=view.mask[p0:p1], dilated_mask=dilated_mask, sel_idx=sel_idx,
                                     ray_of_pixel=ray_of_pixel, mask_binary=view.mask_binary, rays=(q0, q1), pixels=(p0, p1),
                                     full_hw=(view.H, view.W), pixel_cuts=view.pixel_cuts, rank=r)

    def _take_view(self, iter_i, camera=None):
        """the view of this iteration: in silhouette mode on the GPU it is built on the side stream (overlap_view = False: on one stream)"""
        if self.use_silhouettes and self.device.type == "cuda" and self.overlap_view:
            return self.make_view_on_side_stream(iter_i, camera)
        return self.make_view(iter_i, camera)

    def make_view_on_side_stream(self, iter_i, camera=None):
        """make_view for the silhouette mode, enqueued on a second HIP stream.  The ray set of that mode has a data-dependent size, so
        make_view has to bring two numbers to the host (dataset.gen_rays_silhouettes); on the main stream each of those round trips
        waits for EVERYTHING enqueued before it -- the previous iteration's backward pass -- and the host, which would otherwise run
        an iteration ahead of the GPU, falls into lock-step with it.  The view depends on nothing the optimiser writes: on its own
        stream its round trips wait for its own few small kernels only.  Host order -- and with it every numpy / torch random draw --
        is unchanged; the main stream waits for the view's event before its first use, and every tensor of the view is registered
        with the main stream so the caching allocator does not hand its memory back to the side stream while main-stream kernels
        still read it.  (In full-frame mode there is nothing to gain: no round trips, and small kernels do not become resident beside
        the persistent MLP kernels -- profiles/r03_side_stream.txt.)"""
        main = torch.cuda.current_stream(self.device)
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(device=self.device)
            self._side_stream.wait_stream(main)       # first use: whatever initialisation is still in flight on the main stream
        with torch.cuda.device(self.device), torch.cuda.stream(self._side_stream):
            view = self.make_view(iter_i, camera)
            ready = torch.cuda.Event()
            ready.record(self._side_stream)
        main.wait_event(ready)
        for t in vars(view).values():
            if torch.is_tensor(t) and t.is_cuda:
                t.record_stream(main)
        return view

    def draw_background(self, view, choice_i=None):
        """main.py:387-415 -> (choice_i, background_rgb [1,3] | [H*W,1] | None, what render() gets)."""
        dev, H, W = self.device, view.H, view.W
        background_rgb = None
        if choice_i is None:
            choice_i = np.random.choice(4) if self.use_bg_aug else 3
        if choice_i == 0:
            background_rgb = self._white_background()
        elif choice_i == 1:
            # (= torch.normal(zeros + 0.5, zeros + 0.2), main.py:393-394, draw for draw -- without the host-side check of the std TENSOR
            # that form makes, a stream synchronisation; test_gpu_iteration compares the two on the device)
            gaussian = torch.randn([H, W, 1], device=dev) * 0.2 + 0.5
            background_rgb = torch.clamp(gaussian, min=0, max=1).reshape(-1, 1)
        elif choice_i == 2:
            chess_length = H // np.random.choice(np.arange(10, 20))
            sigma = torch.empty(1).uniform_(0.1, 2.0).item()   # torchvision GaussianBlur.get_params: torch CPU RNG
            background_rgb = (chess_background_fused if dev.type == "cuda" else chess_background)(H, W, chess_length, sigma, dev)
        if self.use_silhouettes and choice_i in (1, 2):
            idx = getattr(view, "sel_idx", None)      # (gather by index: boolean-mask indexing would synchronise the stream for the count)
            masked_background_rgb = background_rgb.reshape(-1, 1).index_select(0, idx) if idx is not None else \
                background_rgb.reshape(H, W, 1)[view.dilated_mask].reshape(-1, 1)
        else:
            masked_background_rgb = background_rgb
        return choice_i, background_rgb, masked_background_rgb

    def _draw_light(self, view):
        """main.py:433, :440 -> (light_dir[3], ambience): a random light around the camera and a random ambience, the numpy draws in the
        reference's order (theta offset, phi offset, ambience).  The reference makes the third draw a few device statements after the
        first two; no other host draw lies between them, so drawing the three together leaves the sequence camera -> background ->
        light -> ambience of an iteration unchanged."""
        light_dir = sphere_coord(view.theta + np.random.uniform(-np.pi / 4, np.pi / 4), view.phi + np.random.uniform(-np.pi / 4, np.pi / 4))
        return light_dir, np.random.uniform(0, 0.2)

    def _weighted_normals(self, render_out):
        """main.py:427-429: sum of the sample normals under the compositing weights; renderer.RenderOut carries the same sum out of the compositing kernel"""
        normals = getattr(render_out, "weighted_normals", None)
        if normals is None:
            normals = (render_out["gradients"] * render_out["weights"][:, :, None]).sum(dim=1)
        return normals

    def _prompt_for(self, iter_i, view):
        """main.py:499-507: the face prompt on the face camera's iterations, the back prompt behind the body, else the prompt"""
        if self.use_face_prompt and iter_i % 4 == 0:
            return self.encoded_face_text
        if self.use_back_prompt and view.is_front == 0:
            return self.encoded_back_text
        return self.encoded_text

    def shade_and_scatter(self, render_out, view, choice_i, background_rgb, light=None):
        """main.py:422-487: Lambert shading from the rendered normals (random light around the camera, random ambience),
        then -- in silhouette mode -- the masked rays are scattered back into full images over the augmentation background.
        `light` = (light_dir[3], ambience) injects the numpy draws (tests)."""
        dev, H, W = self.device, view.H, view.W
        color_fine = render_out["color_fine"]
        extra_color_fine = render_out["extra_color_fine"]
        texture_shading = rand_shading_rgb = None
        if self.add_no_texture or self.texture_cast_light:
            light_dir, ambience = self._draw_light(view) if light is None else (np.asarray(light[0]), float(light[1]))
            normals = self._weighted_normals(render_out)
            normals = normals / (torch.norm(normals, dim=-1, keepdim=True) + 1e-7)
            rand_light_d = torch.zeros_like(normals) + h2d.upload(np.asarray(light_dir), dev)
            rand_light_d = rand_light_d / (torch.norm(rand_light_d, dim=-1, keepdim=True) + 1e-7)
            rand_diffuse_shading = (normals * rand_light_d).sum(-1, keepdim=True).clamp(min=0, max=1)
            rand_diffuse_shading = torch.where(torch.isnan(rand_diffuse_shading), torch.ones_like(rand_diffuse_shading), rand_diffuse_shading)
            rand_shading = ambience + (1 - ambience) * rand_diffuse_shading
            ws = render_out["weight_sum"].reshape(-1)
            bgm = (ws < 0.5)[:, None]
            rand_shading_rgb = torch.where(bgm, extra_color_fine, rand_shading.repeat(1, 3))
            rand_shading = torch.where(bgm, torch.ones_like(rand_shading), rand_shading)
            texture_shading = (extra_color_fine * rand_shading).clamp(min=0, max=1)
        weight_sum = render_out["weight_sum"]
        if self.use_silhouettes:  # scatter the masked rays back to full images (main.py:461-487)
            dilated_mask = view.dilated_mask
            background = torch.zeros([H, W, 3], device=dev)
            if choice_i == 0:
                background[:] = 1
            if choice_i in (1, 2):   # (= background[~dilated_mask] = bg[~dilated_mask], without the count a boolean index needs)
                background = torch.where(dilated_mask[..., None], background, background_rgb.reshape(H, W, 1).expand(H, W, 3))
            idx = getattr(view, "sel_idx", None)

            def scatter(vals, base):
                if idx is not None:      # row-major positions of the mask's pixels (dataset.gen_rays_silhouettes): no synchronisation
                    return base.reshape(-1, vals.shape[-1]).index_copy(0, idx, vals)
                full = base.clone()
                full[dilated_mask] = vals
                return full.reshape(-1, vals.shape[-1])
            if self.add_no_texture or self.texture_cast_light:
                texture_shading = scatter(texture_shading, background)
                rand_shading_rgb = scatter(rand_shading_rgb, background)
            extra_color_fine = scatter(extra_color_fine, background)
            color_fine = scatter(color_fine, torch.zeros([H, W, 3], device=dev))
            weight_sum = scatter(weight_sum, torch.zeros([H, W, 1], device=dev))
        return dict(color_fine=color_fine, extra_color_fine=extra_color_fine, weight_sum=weight_sum,
                    texture_shading=texture_shading, rand_shading_rgb=rand_shading_rgb)

    def assemble_loss(self, render_out, comp, view, iter_i):
        """main.py:489-534.  train.shard_view (`view` = this rank's pixel range, shard_of_view): the sums of the colour and mask terms
        over the range are added up over the ranks -- the BCE mean written as its sum over the P pixels of the whole view -- and the
        images are gathered, so that every rank computes the view's loss; `render_out` may be None on a rank without rays."""
        H, W = view.H, view.W
        group = self._shard_group if hasattr(view, "full_hw") else None
        mask = self._loss_mask(view.mask)
        if group is None:
            mask_sum = mask.sum() + 1e-5
            color_error = (comp["color_fine"] - view.true_rgb) * mask
            color_fine_loss = F.l1_loss(color_error, torch.zeros_like(color_error), reduction="sum") / mask_sum
            psnr = None
            if self.writer is not None:   # main.py:493 (a logged statistic only: not computed when nothing records it)
                with torch.no_grad():
                    psnr = 20.0 * torch.log10(1.0 / (((comp["color_fine"] - view.true_rgb) ** 2 * mask).sum() / (mask_sum * 3.0)).sqrt())
            eikonal_loss = render_out["gradient_error"]
            mask_loss = F.binary_cross_entropy(comp["weight_sum"].clip(1e-3, 1.0 - 1e-3), mask)
        else:
            H, W = view.full_hw
            color_error = (comp["color_fine"] - view.true_rgb) * mask
            sums = parallel.allreduce_sum(torch.stack([
                F.l1_loss(color_error, torch.zeros_like(color_error), reduction="sum"), mask.sum(),
                F.binary_cross_entropy(comp["weight_sum"].clip(1e-3, 1.0 - 1e-3), mask, reduction="sum"),
                ((comp["color_fine"] - view.true_rgb) ** 2 * mask).sum().detach()]), group)
            mask_sum = sums[1] + 1e-5
            color_fine_loss, mask_loss = sums[0] / mask_sum, sums[2] / (H * W)
            psnr = None
            if self.writer is not None:
                with torch.no_grad():
                    psnr = 20.0 * torch.log10(1.0 / (sums[3] / (mask_sum * 3.0)).sqrt())
            eikonal_loss = view.eikonal
            B = 2 if self.add_no_texture else 1
            names = ["texture_shading" if self.texture_cast_light else "extra_color_fine"] + (["rand_shading_rgb"] if B == 2 else [])
            images = self._gather_pixels(torch.stack([comp[k] for k in names]), view.pixel_cuts, view.rank, group)
            comp = dict(comp, **{k: images[i] for i, k in enumerate(names)})
        text = self._prompt_for(iter_i, view)
        img = comp["texture_shading"] if self.texture_cast_light else comp["extra_color_fine"]
        if self.add_no_texture:
            # main.py:512 and :524 encode the two images in two calls; the encoder treats batch entries independently, so
            # one B=2 pass gives the same two embeddings with every frozen ViT weight streamed once instead of twice
            enc_both = self.perceptor.encode_image(torch.cat([self.clip_preprocess(img.reshape(H, W, 3)),
                                                              self.clip_preprocess(comp["rand_shading_rgb"].reshape(H, W, 3))], dim=0))
            enc, enc2 = enc_both[0:1], enc_both[1:2]
        else:
            enc = self.perceptor.encode_image(self.clip_preprocess(img.reshape(H, W, 3)))
        cosine = torch.cosine_similarity(torch.mean(enc, dim=0), torch.mean(text, dim=0), dim=0)
        loss = color_fine_loss + eikonal_loss * self.igr_weight + mask_loss * self.mask_weight + (1.0 - cosine) * self.clip_weight
        cosine_shading = None
        if self.add_no_texture:
            cosine_shading = torch.cosine_similarity(torch.mean(enc2, dim=0), torch.mean(text, dim=0), dim=0)
            loss = loss + (1.0 - cosine_shading) * self.clip_weight
        return loss, dict(color=color_fine_loss, eikonal=eikonal_loss, mask=mask_loss, cosine=cosine, cosine_shading=cosine_shading,
                          psnr=psnr, s_val=render_out["s_val"][:1].mean() if render_out is not None else self._s_val())

    def fused_shade_loss(self, render_out, view, choice_i, background_rgb, iter_i, light=None):
        """shade_and_scatter + assemble_loss (main.py:422-534) through the two fused kernels of glue.py: same host draws in the same
        order (light direction, ambience), same images into CLIP, same loss terms -- ~150 small launches fewer per iteration
        (tests/test_gpu_glue.py: values and gradients against the torch statement)."""
        from . import glue
        dev, H, W = self.device, view.H, view.W
        # train.shard_view: `view` is this rank's pixel range of the image (shard_of_view) -- shading, scatter and the per-pixel loss
        # terms run on the range; the four sums and the images become the whole view's before the loss tail and CLIP see them.  A rank
        # without pixels (render_out None) makes the same host draws and joins the same collectives with nothing.
        group = self._shard_group if hasattr(view, "full_hw") else None
        if group is not None:
            H, W = view.full_hw
        P = H * W
        shading = self.add_no_texture or self.texture_cast_light
        light4 = nsum = None
        if shading:
            light_dir, ambience = self._draw_light(view) if light is None else (np.asarray(light[0]), float(light[1]))
            light4 = h2d.upload(glue.unit_light(light_dir, ambience), dev)
            nsum = self._weighted_normals(render_out) if render_out is not None else None
        bg, bg_const, rop = None, 0.0, None
        if self.use_silhouettes:
            rop = view.ray_of_pixel
            if choice_i == 0:
                bg_const = 1.0
            elif choice_i in (1, 2):
                bg = background_rgb.reshape(-1)
        # main.py:489: (mask > 0.5).float() is the identity on the 0 / 1 masks make_view produces
        mask = view.mask if self.mask_weight > 0.0 and getattr(view, "mask_binary", False) else self._loss_mask(view.mask)
        B = 2 if self.add_no_texture else 1
        if render_out is None:
            images, sums = torch.zeros(2, 0, 3, device=dev), torch.zeros(4, device=dev)
            eikonal_loss, s_val = view.eikonal, self._s_val()
        else:
            images, sums = glue.ShadeLossFn.apply(
                render_out["color_fine"], render_out["extra_color_fine"], render_out["weight_sum"].reshape(-1), nsum, view.true_rgb,
                mask.reshape(-1), rop, bg, bg_const, light4, not self.texture_cast_light)
            eikonal_loss, s_val = render_out["gradient_error"], render_out["s_val"][0, 0]
        if group is not None:
            sums = parallel.allreduce_sum(sums, group)
            images = self._gather_pixels(images[:B], view.pixel_cuts, view.rank, group)
        psnr = None
        if self.writer is not None:   # main.py:493 (a logged statistic only)
            with torch.no_grad():
                psnr = 20.0 * torch.log10(1.0 / (sums[3] / ((sums[1] + 1e-5) * 3.0)).sqrt())
        text = self._prompt_for(iter_i, view)
        enc_both = self.perceptor.encode_image(glue.ResizeNormFn.apply(images[:B].reshape(B, H, W, 3)))
        # main.py:491-534 from here on (colour / mask normalisation, the cosines, the weighted sum) in one launch: glue.LossTailFn
        loss, st = glue.LossTailFn.apply(enc_both, text, sums, eikonal_loss, self.igr_weight, self.mask_weight, self.clip_weight, P)
        return loss, dict(color=st[1], eikonal=eikonal_loss, mask=st[2], cosine=st[3], cosine_shading=st[4] if self.add_no_texture else None,
                          psnr=psnr, s_val=s_val), images

    def clip_loss(self, iter_i, camera=None):
        """main.py:348-534: one view from camera to scalar loss (differentiable)."""
        if self._shard_group is not None:
            return self._clip_loss_sharded(iter_i, camera)
        view = self._take_view(iter_i, camera)
        choice_i, background_rgb, masked_background_rgb = self.draw_background(view)
        render_out = self.renderer.render(view.rays_o, view.rays_d, view.near, view.far, background_rgb=masked_background_rgb,
                                          cos_anneal_ratio=self.get_cos_anneal_ratio())
        # (the fused scatter goes by ray_of_pixel: a silhouette view without it takes the torch statement)
        if self.device.type == "cuda" and not (self.use_silhouettes and getattr(view, "ray_of_pixel", None) is None):
            loss, parts, _ = self.fused_shade_loss(render_out, view, choice_i, background_rgb, iter_i)
        else:
            comp = self.shade_and_scatter(render_out, view, choice_i, background_rgb)
            loss, parts = self.assemble_loss(render_out, comp, view, iter_i)
        self.last_view = view
        return loss, parts

    def _s_val(self):
        """the statistic render() reports as s_val (renderer.py:288), for a rank that rendered nothing"""
        with torch.no_grad():
            return 1.0 / torch.exp(self.deviation_network.variance.detach() * 10.0).clip(1e-6, 1e6)

    def _eikonal_sums_torch(self, render_out, view):
        """renderer.py:283-285 before the quotient, from what render() returns: [sum of (|grad| - 1)^2, count] over the samples within
        radius 1.2 -- the torch statement of avc_colsum mode 0 on the compositing kernel's eik [R,2]"""
        pts = view.rays_o[:, None, :] + view.rays_d[:, None, :] * render_out["mid_z_vals"][..., :, None]
        relax = (torch.linalg.norm(pts, ord=2, dim=-1) < 1.2).float().detach()
        err = (torch.linalg.norm(render_out["gradients"], ord=2, dim=-1) - 1.0) ** 2
        return torch.stack([(relax * err).sum(), relax.sum()])

    def _clip_loss_sharded(self, iter_i, camera=None):
        """clip_loss with train.shard_view on more than one rank.  Every rank builds the WHOLE view and makes all
        of its draws -- camera, prior, silhouette selection, background, the z-jitter of all R rays, light -- from streams that are the
        same on every rank, so the view is the one a single process would render.  The rank then renders the rays of its pixel range
        alone (shard_of_view) and shades, scatters and sums over that range; the eikonal sums, the loss sums and the images are made
        the view's by the collectives of parallel.py, and every rank computes the view's loss.  Its backward pass reaches this rank's
        rays only: the bucket's SUM over the ranks is the gradient of the view.  A rank whose range is empty (fewer rays than ranks)
        renders nothing and joins every collective with zeros."""
        dev, group = self.device, self._shard_group
        view = self._take_view(iter_i, camera)
        choice_i, background_rgb, masked_background_rgb = self.draw_background(view)
        R = view.rays_o.shape[0]
        if R == 0:
            raise RuntimeError("train.shard_view: the view has no rays to cut over the ranks")
        jitter = torch.rand([R, 1], device=dev) if self.renderer.perturb > 0 else None      # renderer.py:318, for all R rays as render() draws it
        part = self.shard_of_view(view)
        (q0, q1), (p0, p1) = part.rays, part.pixels
        cut = lambda t, a, b: t if t is None or t.shape[-1] == 3 else t[a:b]      # [1,3] colours are the same for every ray / pixel
        fused = dev.type == "cuda"
        render_out = None
        if q1 > q0:
            kw = dict(group=group) if fused else {}
            render_out = self.renderer.render(part.rays_o, part.rays_d, part.near, part.far, background_rgb=cut(masked_background_rgb, q0, q1),
                                              cos_anneal_ratio=self.get_cos_anneal_ratio(), jitter=cut(jitter, q0, q1), **kw)
        if fused and render_out is not None:
            part.eikonal = render_out["gradient_error"]
        else:      # the torch statement of the same reduction (and, on either device, the rank without rays)
            sums = self._eikonal_sums_torch(render_out, part) if render_out is not None else torch.zeros(2, device=dev)
            s = parallel.allreduce_sum(sums, group)
            part.eikonal = s[0] / (s[1] + 1e-5)
        background_part = cut(background_rgb, p0, p1)
        if fused:
            loss, parts, _ = self.fused_shade_loss(render_out, part, choice_i, background_part, iter_i)
        else:
            if render_out is not None:
                comp = self.shade_and_scatter(render_out, part, choice_i, background_part)
            else:
                if self.add_no_texture or self.texture_cast_light:
                    self._draw_light(view)
                z3 = torch.zeros(0, 3, device=dev)
                comp = dict(color_fine=z3, extra_color_fine=z3, weight_sum=torch.zeros(0, 1, device=dev), texture_shading=z3, rand_shading_rgb=z3)
            loss, parts = self.assemble_loss(render_out, comp, part, iter_i)
        view.part = part
        self.last_view = view
        return loss, parts

    def train_clip_iteration(self, iter_i, camera=None):
        """One optimisation step: this rank's views_per_iter / world views (global index j = rank, rank + world, ...; all with the same
        iter_i, so the face camera and face prompt hold for the whole step), one after the other -- the operand panels belong to one
        ray set, so a view's forward AND backward are enqueued before the next view is built and no autograd graph outlives its
        view -- then one all-reduce, the mean over all views_per_iter views, one Adam step.  Every view after the rank's first draws
        from its own streams (_fresh_view_rngs), swapped in around its clip_loss and kept for the next step; the rank's first view
        draws from the process's streams, which are back in place when the step returns.  `camera`: one camera for the one view of a
        rank, or a list of one camera per view."""
        n = self.views_per_iter // self._view_world      # (train.shard_view: all views_per_iter views, each cut over all ranks)
        if camera is not None and n > 1 and len(camera) != n:
            raise ValueError("%d views per rank and step: `camera` must be a list of %d cameras" % (n, n))
        release = getattr(self.perceptor, "release_graphs", None)
        losses, parts_of, views, mine = [], [], [], None
        try:
            for k in range(n):
                if release is not None:
                    release()     # a graph-replayed encode_image of an earlier view that never reached backward (exception, probe call) does not hold its instance
                if k > 0:         # (host work only: generator states are host data, nothing here waits for the GPU)
                    if mine is None:
                        mine = self._data_rng_state()
                    self._set_data_rng_state(self._view_rngs[k - 1])
                try:
                    loss, parts = self.clip_loss(iter_i, camera if camera is None or n == 1 else camera[k])
                finally:
                    if k > 0:
                        self._view_rngs[k - 1] = self._data_rng_state()
                if k == 0:
                    self._zero_grad()
                if loss.requires_grad:    # (not on a rank that owns no ray of a sharded view: its part of the gradient is zero)
                    loss.backward()       # (draws nothing: the next view's streams replace this view's directly)
                losses.append(loss.detach())
                # (one view: the statistics as they always were kept; several: detached, no autograd graph outlives its view)
                parts_of.append(parts if n == 1 else {key: None if v is None else v.detach() for key, v in parts.items()})
                views.append(self.last_view)
                del loss, parts
        finally:
            if mine is not None:      # an exception included: the process's streams are never left swapped out
                self._set_data_rng_state(mine)
        # (train.shard_view: the ranks' gradients are PARTS of each view's gradient -- SUM over the ranks, mean over the views alone)
        self._reduce_and_step(None if n == 1 and not self.shard_view else self.views_per_iter)
        self.last_views, self.last_view_losses = views, losses
        if n == 1:
            loss, p = losses[0], parts_of[0]
            parts = dict(color=p["color"].detach(), eikonal=p["eikonal"].detach(), cosine=p["cosine"].detach(), s_val=p["s_val"], psnr=p["psnr"])
        else:                         # the means over this rank's views: one stack and one reduction for all of them
            keys = [key for key in ("color", "eikonal", "cosine", "s_val", "psnr") if parts_of[0][key] is not None]
            m = torch.stack([v.reshape(()) for l, p in zip(losses, parts_of) for v in [l] + [p[key] for key in keys]]).reshape(n, -1).mean(0)
            loss, parts = m[0], dict({"psnr": None}, **{key: m[1 + i] for i, key in enumerate(keys)})
        self.last_stats = dict(loss=loss, color=parts["color"], eikonal=parts["eikonal"], cosine=parts["cosine"],
                               rays=sum(v.rays_o.shape[0] for v in views), s_val=parts["s_val"], psnr=parts["psnr"])
        if self.writer is not None:   # main.py:542-547
            for tag, v in (("Loss/loss", loss), ("Loss/color_loss", parts["color"]), ("Loss/eikonal_loss", parts["eikonal"]),
                           ("Loss/cosine", parts["cosine"]), ("Statistics/s_val", parts["s_val"]), ("Statistics/psnr", parts["psnr"])):
                self.writer.add_scalar(tag, v, self.iter_step)
            if self.iter_step % self.report_freq == 0:
                self.writer.flush()
        return loss

    # ------------------------------------------------------------------ schedule / checkpoints (main.py:568-632)
    def get_image_perm(self):
        return torch.randperm(max(self.dataset.n_images, 1))

    def get_cos_anneal_ratio(self):
        if self.anneal_end == 0.0:
            return 1.0
        return np.min([1.0, self.iter_step / self.anneal_end])

    def update_learning_rate(self):
        if self.iter_step < self.warm_up_end:
            learning_factor = self.iter_step / self.warm_up_end
        else:
            alpha = self.learning_rate_alpha
            progress = (self.iter_step - self.warm_up_end) / (self.end_iter - self.warm_up_end)
            learning_factor = (np.cos(np.pi * progress) + 1.0) * 0.5 * (1 - alpha) + alpha
        for g in self.optimizer.param_groups:
            g["lr"] = float(self.learning_rate * learning_factor)   # (a Python float: a numpy scalar here would make the checkpoint more than tensors and plain containers)

    def file_backup(self):
        dir_lis = self.conf.get("general.recording", default=[])
        os.makedirs(os.path.join(self.base_exp_dir, "recording"), exist_ok=True)
        for dir_name in dir_lis:
            if not os.path.isdir(dir_name):
                continue
            cur_dir = os.path.join(self.base_exp_dir, "recording", dir_name)
            os.makedirs(cur_dir, exist_ok=True)
            for f_name in os.listdir(dir_name):
                if f_name[-3:] == ".py":
                    copyfile(os.path.join(dir_name, f_name), os.path.join(cur_dir, f_name))
        copyfile(self.conf_path, os.path.join(self.base_exp_dir, "recording", "config.conf"))

    def _torch_load(self, path, map_location=None):
        """checkpoints of this stage hold tensors, the optimizer's plain containers and an int: the tensors-only unpickler reads
        them without executing code from the file.  A file it rejects is loaded with the full unpickler -- which executes code from
        the file, as the reference's plain torch.load does -- only with the same explicit opt-in as the other loaders
        (AVC_ALLOW_UNSAFE_PICKLE=1: clip_vit.load_state_dict, smpl_lbs.load_smpl_arrays); I/O errors are not retried."""
        import pickle
        try:
            # (numpy scalars -- the learning rate the reference's update_learning_rate leaves in the optimizer's param groups -- are
            # data, not code: allow-listed for the tensors-only unpickler)
            safe = [np.dtype, type(np.dtype(np.float64)), type(np.dtype(np.float32)), type(np.dtype(np.int64))]
            try:
                from numpy._core.multiarray import scalar as np_scalar       # numpy 2
            except ImportError:
                from numpy.core.multiarray import scalar as np_scalar        # numpy 1
            # (files written under numpy 1 -- the reference's shipped checkpoint -- name it by its old module path)
            safe += [np_scalar, (np_scalar, "numpy.core.multiarray.scalar"), (np_scalar, "numpy._core.multiarray.scalar")]
            with torch.serialization.safe_globals(safe):
                return torch.load(path, map_location=self.device if map_location is None else map_location, weights_only=True)
        except pickle.UnpicklingError as e:
            if os.environ.get("AVC_ALLOW_UNSAFE_PICKLE") != "1":
                raise RuntimeError("%s is not a tensors-only checkpoint (%s); loading it would execute pickled code (set "
                                   "AVC_ALLOW_UNSAFE_PICKLE=1 to allow that)" % (path, str(e)[:200])) from e
            logging.warning("%s is not a tensors-only checkpoint: loading it with the full unpickler (AVC_ALLOW_UNSAFE_PICKLE=1)", path)
            return torch.load(path, map_location=self.device if map_location is None else map_location, weights_only=False)

    def load_checkpoint(self, checkpoint_name):
        checkpoint = self._torch_load(os.path.join(self.base_exp_dir, "checkpoints", checkpoint_name))
        self.sdf_network.load_state_dict(checkpoint["sdf_network_fine"])
        self.deviation_network.load_state_dict(checkpoint["variance_network_fine"])
        self.color_network.load_state_dict(checkpoint["color_network_fine"])
        self.optimizer.load_state_dict(checkpoint["optimizer"])
        self.iter_step = checkpoint["iter_step"]

    def load_pretrain(self, checkpoint_name):
        checkpoint = self._torch_load(checkpoint_name)
        self.sdf_network.load_state_dict(checkpoint["sdf_network_fine"])
        self.deviation_network.load_state_dict(checkpoint["variance_network_fine"])
        self.color_network.load_state_dict(checkpoint["color_network_fine"], strict=False)   # main.py:617

    def save_checkpoint(self):
        checkpoint = {
            "sdf_network_fine": self.sdf_network.state_dict(),
            "variance_network_fine": self.deviation_network.state_dict(),
            "color_network_fine": self.color_network.state_dict(),
            "optimizer": self.optimizer.state_dict(),
            "iter_step": self.iter_step,
        }
        os.makedirs(os.path.join(self.base_exp_dir, "checkpoints"), exist_ok=True)
        _save_atomically(checkpoint, os.path.join(self.base_exp_dir, "checkpoints", "ckpt_{:0>6d}.pth".format(self.iter_step)))

    # ------------------------------------------------------------------ resume records
    # <base_exp_dir>/resume/ckpt_<step>.rank<r>.pt beside checkpoints/ckpt_<step>.pth: what the checkpoint (the reference's format, left
    # as it is) does not hold of a run -- where its data streams stand.  Tensors, ints, floats, strings and None only (_torch_load reads it
    # with the tensors-only unpickler).  Not in checkpoints/, and not named *pth: the is_continue listing parses every such name there.
    def _resume_record_path(self, step, rank):
        return os.path.join(self.base_exp_dir, "resume", "ckpt_{:0>6d}.rank{:d}.pt".format(step, rank))

    def save_resume_record(self):
        """this rank's record of the current step.  Called at the end of _after_step, after the checkpoint is in place: a complete set of
        records means a complete checkpoint."""
        record = {
            "iter_step": int(self.iter_step), "mode": str(self.mode), "world": int(self.world), "rank": int(self.rank),
            "views_per_iter": int(self.views_per_iter), "shard_view": bool(self.shard_view), "resume_tag": self.resume_tag,
            "base_seed": getattr(self, "base_seed", self.seed), "data_seed": getattr(self, "data_seed", self.seed),
            "streams": pack_rng_state(self._data_rng_state()), "view_streams": [pack_rng_state(s) for s in self._view_rngs],
            "iter_i": None if self._next_iter_i is None else int(self._next_iter_i),
            "image_perm": None if self._image_perm is None else self._image_perm.detach().cpu().clone(),
        }
        path = self._resume_record_path(self.iter_step, self.rank)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        _save_atomically(record, path)

    def _read_resume_record(self, step, rank):
        """the record of (step, rank), its tensors on the host (generator states are host data); None when there is none"""
        path = self._resume_record_path(step, rank)
        return self._torch_load(path, map_location="cpu") if os.path.isfile(path) else None

    def _find_resume_step(self):
        """resume=True: the newest step <= end_iter whose checkpoint and whose records of all ranks exist and carry this run's tag, or
        None.  Rank 0 looks, every rank gets its answer.  A record written by another kind of run (world size, views per step, view
        sharding, mode) is refused with both values named: its streams are not those of this run's views."""
        found = -1
        if self.rank == 0:
            ckpt_dir = os.path.join(self.base_exp_dir, "checkpoints")
            names = os.listdir(ckpt_dir) if os.path.isdir(ckpt_dir) else []
            steps = sorted((int(m[5:-4]) for m in names if m[:5] == "ckpt_" and m[-4:] == ".pth" and m[5:-4].isdigit()), reverse=True)
            for step in steps:
                if step > self.end_iter:
                    continue
                records = [self._read_resume_record(step, 0)]
                if records[0] is not None and records[0]["world"] == self.world:      # (another world size: refused below)
                    records += [self._read_resume_record(step, k) for k in range(1, self.world)]
                if all(r is not None and r["resume_tag"] == self.resume_tag and r["iter_step"] == step for r in records):
                    found = step
                    break
        if parallel.is_on():
            t = torch.tensor([found], dtype=torch.int64, device=self.device)
            parallel.broadcast_tensor(t)
            found = int(t.item())
        if found < 0:
            return None
        record = self._read_resume_record(found, 0)
        for key, mine in (("world", self.world), ("views_per_iter", self.views_per_iter), ("shard_view", self.shard_view), ("mode", self.mode)):
            if record[key] != mine:
                raise ValueError("resume: the records of step %d under %s were written by a run with %s = %r, this run has %s = %r; "
                                 "its data streams cannot be continued (restart the run without resume)"
                                 % (found, self.base_exp_dir, key, record[key], key, mine))
        return found

    def _restore_resume_record(self):
        """at the top of train() / train_clip(): put the streams of the interrupted run in place -- after init_clip, init_smpl and the
        dataset have drawn whatever they draw while they are built -- and hand the record on (None: not a resumed run)"""
        record, self._resume_record = self._resume_record, None
        if record is None:
            return None
        self._set_data_rng_state(unpack_rng_state(record["streams"]))
        self._view_rngs = [unpack_rng_state(s) for s in record["view_streams"]]
        logging.info("resume: continuing %s at step %d", self.base_exp_dir, record["iter_step"])
        return record

    def _render_chunks(self, rays_o, rays_d, keys, chunk=None, **render_kw):
        """render() over chunks of rays without keeping a graph (main.py:752-783 and its siblings); returns dict of cats."""
        chunk = chunk or self.batch_size * 16     # the kernels want >= a few thousand rays per launch; the result is chunk-invariant
        outs = {k: [] for k in keys}
        bg = self._white_background() if self.use_white_bkgd else None
        for o, d in zip(rays_o.split(chunk), rays_d.split(chunk)):
            near, far = self.dataset.near_far_from_sphere(o, d)
            with torch.no_grad():
                out = self.renderer.render(o.contiguous(), d.contiguous(), near, far, background_rgb=render_kw.get("background_rgb", bg),
                                           cos_anneal_ratio=self.get_cos_anneal_ratio(),
                                           perturb_overwrite=render_kw.get("perturb_overwrite", -1))
            for k in keys:
                if k == "normals":   # main.py:773-778
                    n = out["gradients"] * out["weights"][:, :, None]
                    if render_kw.get("inside_only", True) and out.get("inside_sphere") is not None:
                        n = n * out["inside_sphere"][..., None]
                    outs[k].append(n.sum(dim=1))
                else:
                    outs[k].append(out[k].detach())
        return {k: torch.cat(v, 0) for k, v in outs.items()}

    def validate_image(self, idx=-1, resolution_level=-1, pose=None, save=False, perturb_overwrite=-1):
        """main.py:741-820.  Returns the [H,W,3] image (extra_color when the colour net has the CLIP head); with save=True
        also writes validations_fine/, validations_extra_fine/ and normals/ PNGs under base_exp_dir with the reference's
        file names and channel conventions (cv.imwrite takes BGR: the colour and normal images are written un-converted,
        i.e. channel-swapped on disk, the extra-colour image is converted first -- reproduced literally)."""
        if resolution_level < 0:
            resolution_level = self.validate_resolution_level
        if pose is None:
            if idx < 0:
                idx = np.random.randint(self.dataset.n_images)
            pose = self.dataset.poses[idx]
        print("Validate: iter: {}, camera: {}".format(self.iter_step, idx))
        rays_o, rays_d = self.dataset.gen_rays_pose(pose, resolution_level)
        H, W, _ = rays_o.shape
        keys = ["color_fine", "normals"] + (["extra_color_fine"] if self.extra_color else [])
        res = self._render_chunks(rays_o.reshape(-1, 3).float(), rays_d.reshape(-1, 3).float(), keys, perturb_overwrite=perturb_overwrite)
        img_fine = (res["color_fine"].reshape(H, W, 3) * 255).clip(0, 255)
        extra = (res["extra_color_fine"].reshape(H, W, 3) * 255).clip(0, 255) if self.extra_color else None
        rot = torch.linalg.inv(torch.as_tensor(pose)[:3, :3].to(self.device).float())
        normal_img = (torch.matmul(rot[None], res["normals"][:, :, None]).reshape(H, W, 3) * 128 + 128).clip(0, 255)
        self.last_validation = dict(color=img_fine, extra=extra, normal=normal_img)
        if save:
            from PIL import Image
            tag = "{:0>8d}_{}_{}.png".format(self.iter_step, 0, idx)
            u8 = lambda t: np.ascontiguousarray(t.detach().cpu().numpy().astype(np.uint8))
            for sub in ("validations_fine", "validations_extra_fine", "normals"):
                os.makedirs(os.path.join(self.base_exp_dir, sub), exist_ok=True)
            fine = u8(img_fine)
            if idx >= 0 and self.dataset.images_lis:
                fine = np.concatenate([fine, self.dataset.image_at(idx, resolution_level=resolution_level)])
            Image.fromarray(np.ascontiguousarray(fine[..., ::-1])).save(os.path.join(self.base_exp_dir, "validations_fine", tag))
            if extra is not None:
                Image.fromarray(u8(extra)).save(os.path.join(self.base_exp_dir, "validations_extra_fine", tag))
            Image.fromarray(np.ascontiguousarray(u8(normal_img)[..., ::-1])).save(os.path.join(self.base_exp_dir, "normals", tag))
        return ((extra if extra is not None else img_fine) / 255.0).clamp(0, 1)

    def render_novel_image(self, idx_0, idx_1, ratio, resolution_level):
        """main.py:822-848: the view interpolated between cameras idx_0 and idx_1 -> uint8 [H,W,3] (x256 like the reference)."""
        rays_o, rays_d = self.dataset.gen_rays_between(idx_0, idx_1, ratio, resolution_level=resolution_level)
        H, W, _ = rays_o.shape
        res = self._render_chunks(rays_o.reshape(-1, 3).float(), rays_d.reshape(-1, 3).float(), ["color_fine"])
        return (res["color_fine"].reshape(H, W, 3).cpu().numpy() * 256).clip(0, 255).astype(np.uint8)

    def interpolate_view(self, img_idx_0, img_idx_1, n_frames=60, resolution_level=4):
        """main.py:921-944: 60 frames forth and back between two cameras.  cv2.VideoWriter is not available offline: the
        frames are written as an animated GIF (30 fps) plus numbered PNGs under base_exp_dir/render/."""
        from PIL import Image
        images = [self.render_novel_image(img_idx_0, img_idx_1, np.sin(((i / n_frames) - 0.5) * np.pi) * 0.5 + 0.5,
                                          resolution_level=resolution_level) for i in range(n_frames)]
        images = images + images[::-1]
        video_dir = os.path.join(self.base_exp_dir, "render")
        os.makedirs(video_dir, exist_ok=True)
        stem = os.path.join(video_dir, "{:0>8d}_{}_{}".format(self.iter_step, img_idx_0, img_idx_1))
        frames = [Image.fromarray(im) for im in images]
        frames[0].save(stem + ".gif", save_all=True, append_images=frames[1:], duration=33, loop=0)
        return stem + ".gif"

    def render_geometry_cast_light(self, light=None):
        """main.py:634-739: 512x512 close-up of the head, textured colour under one random Lambert light (ambience 0, black
        background) -> base_exp_dir/cast_light_texture_head_black.png."""
        phi, theta, camera_distance = 0, 0, 0.5
        eye = np.array([camera_distance * np.sin(theta) * np.cos(phi), camera_distance * np.sin(theta) * np.sin(phi),
                        camera_distance * np.cos(theta)])
        at = np.array([0, self.head_height, 0.3])
        eye = eye + at
        pose = torch.from_numpy(lookat(eye, at, np.array([0, 1, 0]))).float()
        rays_o, rays_d = self.dataset.gen_rays_pose(pose, 0.5)
        H, W = rays_o.shape[0], rays_o.shape[1]
        if light is None:
            light = sphere_coord(theta + np.random.uniform(-np.pi / 4, np.pi / 4), phi + np.random.uniform(-np.pi / 4, np.pi / 4))
        np.random.choice(np.arange(10, 20))      # main.py:676 draws the chess length although choice_i is fixed to 3
        res = self._render_chunks(rays_o.reshape(-1, 3).float(), rays_d.reshape(-1, 3).float(),
                                  ["extra_color_fine" if self.extra_color else "color_fine", "normals", "weight_sum"],
                                  background_rgb=None, inside_only=False)
        extra = res["extra_color_fine" if self.extra_color else "color_fine"]
        normals = res["normals"] / (torch.norm(res["normals"], dim=-1, keepdim=True) + 1e-7)
        ld = torch.from_numpy(np.asarray(light)).float().to(self.device)
        ld = (torch.zeros_like(normals) + ld)
        ld = ld / (torch.norm(ld, dim=-1, keepdim=True) + 1e-7)
        shading = (normals * ld).sum(-1, keepdim=True).clamp(min=0, max=1)
        shading = torch.where(torch.isnan(shading), torch.ones_like(shading), shading)
        shading = torch.where((res["weight_sum"].reshape(-1) < 0.5)[:, None], torch.ones_like(shading), shading)
        img = (extra * shading).clamp(0, 1).reshape(H, W, 3)
        from PIL import Image
        path = os.path.join(self.base_exp_dir, "cast_light_texture_head_black.png")
        Image.fromarray((255 * np.clip(img.cpu().numpy(), 0, 1)).astype(np.uint8)).save(path)   # to8b
        return path

    def validate_mesh(self, world_space=False, resolution=256, threshold=0.0):
        """main.py:850-919: marching cubes of -sdf over the dataset bounding box, vertex colours picked from six axis views
        (per vertex the view whose rendered depth is closest to the true camera-vertex distance), PLY export.
        (`world_space` is accepted and unused, as in the reference.)"""
        from . import mesh
        bound_min = torch.tensor(self.dataset.object_bbox_min, dtype=torch.float32)
        bound_max = torch.tensor(self.dataset.object_bbox_max, dtype=torch.float32)
        vertices, triangles = self.renderer.extract_geometry(bound_min, bound_max, resolution=resolution, threshold=threshold)
        os.makedirs(os.path.join(self.base_exp_dir, "meshes"), exist_ok=True)
        pt = torch.from_numpy(vertices).to(self.device).reshape(-1, 3).float()
        rgb_final, diff_final = None, None
        chunk = self.batch_size * 64      # rays per render call: no gradient is kept, only the panel-free forward runs
        for eye in ([0, 0, 2], [0, 0, -2], [0, 2, 0], [0, -2, 0], [2, 0, 0], [-2, 0, 0]):
            ro_all = torch.tensor(eye, dtype=torch.float32, device=self.device).reshape(1, 3).repeat(pt.shape[0], 1)
            rd_all = pt - ro_all
            dist = torch.norm(rd_all, dim=-1)
            rd_all = rd_all / dist.reshape(-1, 1)
            rgbs, diffs = [], []
            for ro, rd, di in zip(ro_all.split(chunk), rd_all.split(chunk), dist.split(chunk)):
                near, far = self.dataset.near_far_from_sphere(ro, rd)
                bg = self._white_background() if self.use_white_bkgd else None
                with torch.no_grad():
                    out = self.renderer.render(ro.contiguous(), rd.contiguous(), near, far,
                                               cos_anneal_ratio=self.get_cos_anneal_ratio(), background_rgb=bg)
                rgbs.append(out["extra_color_fine"] if self.extra_color else out["color_fine"])
                depth = (out["mid_z_vals"] * out["weights"]).sum(dim=1)
                diffs.append((depth - di).abs())
            rgb, diff = torch.cat(rgbs, 0), torch.cat(diffs, 0)
            if rgb_final is None:
                rgb_final, diff_final = rgb.clone(), diff.clone()
            else:
                ind = diff_final > diff
                rgb_final[ind] = rgb[ind]
                diff_final[ind] = diff[ind]
        colors = (255 * np.clip(rgb_final.cpu().numpy(), 0, 1)).astype(np.uint8) if rgb_final is not None else None
        path = os.path.join(self.base_exp_dir, "meshes", "{:0>8d}.ply".format(self.iter_step))
        mesh.write_ply(path, vertices, triangles, colors)
        logging.info("mesh: %d vertices, %d triangles -> %s", vertices.shape[0], triangles.shape[0], path)
        return path


def _save_atomically(obj, path):
    """torch.save under a temporary name beside `path`, then os.replace: a reader never finds a truncated file under the final name
    (the temporary name does not end in pth either: the is_continue listing parses every such name in checkpoints/)"""
    tmp = "%s.tmp.%d" % (path, os.getpid())
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise


def pack_rng_state(state):
    """Runner._data_rng_state() as tensors, ints, floats, strings and None (what the tensors-only unpickler reads back)"""
    (np_name, np_keys, np_pos, np_has_gauss, np_cached), (py_version, py_internal, py_gauss_next), host, device = state
    return {"numpy_name": str(np_name), "numpy_keys": torch.from_numpy(np.asarray(np_keys).astype(np.int64)), "numpy_pos": int(np_pos),
            "numpy_has_gauss": int(np_has_gauss), "numpy_cached_gaussian": float(np_cached),
            "random_version": int(py_version), "random_internal": torch.tensor(py_internal, dtype=torch.int64),
            "random_gauss_next": None if py_gauss_next is None else float(py_gauss_next),
            "torch_host": host.detach().cpu().clone(), "torch_device": None if device is None else device.detach().cpu().clone()}


def unpack_rng_state(d):
    """the inverse of pack_rng_state, bit for bit"""
    return ((d["numpy_name"], d["numpy_keys"].numpy().astype(np.uint32), d["numpy_pos"], d["numpy_has_gauss"], d["numpy_cached_gaussian"]),
            (d["random_version"], tuple(int(v) for v in d["random_internal"].tolist()), d["random_gauss_next"]),
            d["torch_host"].to(torch.uint8), None if d["torch_device"] is None else d["torch_device"].to(torch.uint8))


def clip_vit_random_state_dict(seed, patch=32):
    """Seeded ViT-B/32 (patch=16: ViT-B/16, 197 positional rows) weights with OpenAI's init scales and key names (used only when no
    real weights are given)."""
    if patch not in (32, 16):
        raise ValueError("clip_vit_random_state_dict: patch 32 (ViT-B/32) or 16 (ViT-B/16), got %r" % (patch,))
    g = torch.Generator().manual_seed(seed)
    W, L, P, T, E = 768, 12, patch, (224 // patch) ** 2 + 1, 512
    rn = lambda *s, std=1.0: torch.randn(*s, generator=g) * std
    sd = {"visual.conv1.weight": rn(W, 3, P, P, std=0.02), "visual.class_embedding": rn(W, std=W ** -0.5),
          "visual.positional_embedding": rn(T, W, std=W ** -0.5), "visual.proj": rn(W, E, std=W ** -0.5)}
    for n in ("ln_pre", "ln_post"):
        sd["visual.%s.weight" % n], sd["visual.%s.bias" % n] = torch.ones(W), torch.zeros(W)
    for i in range(L):
        p = "visual.transformer.resblocks.%d." % i
        sd[p + "attn.in_proj_weight"], sd[p + "attn.in_proj_bias"] = rn(3 * W, W, std=W ** -0.5), torch.zeros(3 * W)
        sd[p + "attn.out_proj.weight"], sd[p + "attn.out_proj.bias"] = rn(W, W, std=W ** -0.5 * (2 * L) ** -0.5), torch.zeros(W)
        for n in ("ln_1", "ln_2"):
            sd[p + n + ".weight"], sd[p + n + ".bias"] = torch.ones(W), torch.zeros(W)
        sd[p + "mlp.c_fc.weight"], sd[p + "mlp.c_fc.bias"] = rn(4 * W, W, std=(2 * W) ** -0.5), torch.zeros(4 * W)
        sd[p + "mlp.c_proj.weight"], sd[p + "mlp.c_proj.bias"] = rn(W, 4 * W, std=W ** -0.5 * (2 * L) ** -0.5), torch.zeros(W)
    return sd


def chess_background(H, W, chess_length, sigma, device):
    """main.py:398-405: 0.2 / 0.8 chess board of `chess_length`-pixel squares, GaussianBlur(kernel (5,9), sigma) -> [H*W,1]."""
    chess_board = torch.zeros([H, W, 1], device=device) + 0.2
    ii = torch.arange(H, device=device)[:, None] // chess_length
    jj = torch.arange(W, device=device)[None, :] // chess_length
    chess_board[((ii + jj) % 2 == 0)] = 0.8
    return _gaussian_blur(chess_board.permute(2, 0, 1).unsqueeze(0), (5, 9), float(sigma)).squeeze(0).permute(1, 2, 0).reshape(-1, 1)


def chess_background_fused(H, W, chess_length, sigma, device):
    """chess_background in one launch (csrc/avc_glue.hip: avc_chess_background; the 14 blur taps are computed on the host)"""
    from . import lib as L
    def k1d(k):
        r = np.arange(k, dtype=np.float32) - np.float32((k - 1) / 2)
        w = np.exp(np.float32(-0.5) * (r / np.float32(sigma)) ** 2).astype(np.float32)
        return w / w.sum(dtype=np.float32)
    taps = h2d.upload(np.concatenate([k1d(5), k1d(9)]), device)
    out = torch.empty(H * W, 1, device=device, dtype=torch.float32)
    L.call("avc_chess_background", out, H, W, int(chess_length), taps)
    return out


def _gaussian_blur(x, ksize, sigma):
    """separable gaussian blur of [1,C,H,W] with reflect padding (torchvision.transforms.GaussianBlur semantics)."""
    def k1d(k):      # (on the host: the taps are nine numbers, and a .tolist() of a device tensor would synchronise the stream)
        r = torch.arange(k, dtype=x.dtype) - (k - 1) / 2
        w = torch.exp(-0.5 * (r / sigma) ** 2)
        return w / w.sum()
    kx, ky = k1d(ksize[0]).tolist(), k1d(ksize[1]).tolist()
    H, W = x.shape[-2:]
    x = F.pad(x, (ksize[0] // 2, ksize[0] // 2, ksize[1] // 2, ksize[1] // 2), mode="reflect")
    # 5 + 9 shifted multiply-adds instead of F.conv2d: MIOpen answers a [1,1,H,W] depthwise convolution with its naive
    # kernel (1.4 ms per call in the profile, 2 % of a step)
    x = sum(w * x[..., :, k:k + W] for k, w in enumerate(kx))
    x = sum(w * x[..., k:k + H, :] for k, w in enumerate(ky))
    return x
