"""Prompt -> animated, rigged avatar as ONE resumable run: the nine stages of this package chained through their files.

    python -m avatarclip_amd.pipeline --out_dir D --target_txt "a 3d rendering of a strong man in unreal engine" \\
        --prompt "a 3D rendering of the Iron Man in unreal engine" --motion_text "a rendered 3d man is arguing" \\
        --init_conf INIT.conf --appearance_conf APPEARANCE.conf --animate_conf ANIMATE.conf \\
        --clip_weights ViT-B-32.pt --bpe bpe_simple_vocab_16e6.txt.gz --smpl SMPL_NEUTRAL.npz --pose_npy stand_pose.npy \\
        --template_obj zero_beta_smpl.obj --AE_path_fname model_VAE_16.pth --codebook_fname shape_codebook.pth \\
        --vposer data/vposer --codebook data/codebook.pth --motion_vae data/motion_vae.pth --renderer_gradient
        [--from STAGE] [--until STAGE] [--force] [--restart_stages]

  stage       calls                                                            writes under out_dir/
  shape       shapegen.create_load_AE, load_codebook, shape_gen, writeOBJ      shape/coarse_shape.obj, shape/shape.json
  dataset     shapegen_render.pose_shape, write_nerf_dataset                   shape/posed.obj, render/img/*.png, render/transforms_train.json
  init        Runner(mode="train").train                                       exp_init/checkpoints/ckpt_*.pth
  appearance  Runner(mode="train_clip"): init_clip, init_smpl, train_clip      exp_clip/checkpoints/ckpt_*.pth
  mesh        Runner(mode="validate_mesh", is_continue).validate_mesh          exp_clip/meshes/*.ply
  motion      animate.AnimateContext, animate.run                              anim/candidate_<i>.npy, anim/motion.npy
  drive       drive.generate_animation                                         drive/<name>_cleaned_apose.ply, drive/motion.pc2
  rig         rig.build_rig(..., motion=anim/motion.npy)                       rig/<name>.glb, rig/<name>_rig.npz (--bake_texture SIZE: a baked
                                                                               base-colour texture, also rig/<name>_texture.png)
  preview     preview.preview, once per kind of result                         preview/{mesh,drive,rig,motion}.gif

Every stage is a call into the module that implements it; none of their arithmetic is restated here.  What this module adds:
  * ONE CLIP tower (clip_vit.ClipVision) and ONE tokenizer, built on first use and handed to shape_gen, Runner.init_clip and
    AnimateContext.  The shipped codebooks hold ViT-B/32 embeddings (README, "ViT-B/32 or ViT-B/16"): with a ViT-B/16 main
    checkpoint give the ViT-B/32 one as `retrieval_clip_weights`; it then serves `shape` and a VPoserCodebook pose generator.
    A codebook written by `avatarclip_amd.codebook` carries a sidecar `<file>.json`: when it names the main tower's variant the
    warning about a ViT-B/16 tower is not raised, and one naming another variant or another texture is a line of `check`.
  * `check`: every asset of every selected stage, both generator types of the AvatarAnimate conf and the renderer gradient of a
    CLIP-guided generator are verified BEFORE the first stage; all problems come in one ValueError.
  * out_dir/pipeline.json: per stage its status, wall seconds, outputs (size, sha256) and a fingerprint = sha256 over the stage's
    own settings, the sha256 of every asset file it reads and the fingerprints of the stages it consumes.  A stage is skipped
    exactly when its recorded fingerprint equals the current one and every recorded output still exists with the recorded size.
    The file is rewritten atomically after every stage, so a killed run resumes after its last finished stage.
  * the two long stages continue INSIDE the stage: `init` and `appearance` tag the Runner's resume records (runner.py, beside every
    checkpoint) with the stage's fingerprint, and a stage whose previous record is `running` or `failed` with the current fingerprint
    is started with Runner(resume=True): it goes on from its newest complete checkpoint, draw for draw, and its `done` record says
    `resumed_from: <step>`.  Checkpoints of another prompt or conf carry another tag and are never continued; `--force` and
    `--restart_stages` start the stage at step 0.

`run(spec)` takes a PipelineSpec or a dict of its fields.  Single process: train.views_per_iter / train.shard_view stay with
`avatarclip_amd.main`."""
import argparse
import copy
import dataclasses
import hashlib
import importlib.util
import json
import os
import sys
import time
import warnings
from typing import Any, Optional

from .conf import ConfigFactory, ConfigTree

STAGES = ("shape", "dataset", "init", "appearance", "mesh", "motion", "drive", "rig", "preview")
# the stages whose OUTPUT FILES a stage reads (`motion` needs no avatar: AvatarAnimate runs on the SMPL body alone)
CONSUMES = {"shape": (), "dataset": ("shape",), "init": ("dataset",), "appearance": ("dataset", "init"), "mesh": ("appearance",), "motion": (),
            "drive": ("mesh", "motion"), "rig": ("mesh", "motion"), "preview": ("mesh", "motion", "drive", "rig")}
MANIFEST, MANIFEST_VERSION = "pipeline.json", 1
SHAPE_LATENT_DIM = 16                                   # ShapeGen/main.py: model_VAE_16.pth
CLIP_GUIDED_POSE = ("PoseOptimizer", "VPoserOptimizer")  # animate.py: optimise the CLIP score through the rasteriser
RENDERING_POSE = CLIP_GUIDED_POSE + ("VPoserRealNVP",)   # embed renders of their own: need the image tower
_OUT = "$OUT"                                           # out_dir inside a fingerprint: moving the directory re-runs nothing
_B16_WARNED = False


@dataclasses.dataclass
class PipelineSpec:
    """One field per command-line flag (`--<field>`; from_stage / until_stage are `--from` / `--until`).  The confs are paths or parsed
    conf.ConfigFactory trees; `vposer` is human_body_prior's model directory or a VPoser-like object (decode / encode, animate.py).
    A prompt left at None stays what its conf says (clip.prompt, clip.face_prompt, clip.back_prompt, general.text)."""
    out_dir: str = None
    # ---- prompts
    target_txt: str = "a 3d rendering of a strong man in unreal engine"
    neutral_txt: str = "a 3d rendering of a person in unreal engine"
    prompt: Optional[str] = None
    face_prompt: Optional[str] = None
    back_prompt: Optional[str] = None
    motion_text: Optional[str] = None
    # ---- confs: NeuS init (Runner.train), appearance (Runner.train_clip, validate_mesh), AvatarAnimate
    init_conf: Any = None
    appearance_conf: Any = None
    animate_conf: Any = None
    # ---- assets
    clip_weights: Optional[str] = None
    bpe: Optional[str] = None
    retrieval_clip_weights: Optional[str] = None
    smpl: Optional[str] = None
    pose_npy: Optional[str] = None
    template_obj: Optional[str] = None
    AE_path_fname: Optional[str] = None
    codebook_fname: Optional[str] = None
    vposer: Any = None
    codebook: Optional[str] = None
    realnvp: Optional[str] = None
    motion_vae: Optional[str] = None
    smpl_uv: Optional[str] = None            # the textured body (.obj + .mtl + image) the scoring renders of shape and motion show; None: white
    # ---- knobs of the stage functions
    pose_type: str = "stand_pose"
    image_size: int = 256
    mesh_resolution: int = 512
    mcube_threshold: float = 0.0
    voxel_divisor: int = 256
    bake_texture: int = 0                    # rig: bake the mesh's colours into a texture of this size on the simplified mesh (0: vertex colours)
    preview_size: int = 512
    preview_views: int = 36
    renderer_gradient: bool = False
    posing: str = "torch"
    name: str = "avatar"
    gpu: int = 0
    # ---- range
    from_stage: Optional[str] = None
    until_stage: Optional[str] = None
    force: bool = False
    restart_stages: bool = False             # init / appearance: start an interrupted stage at step 0 instead of continuing it (in no fingerprint)
    # ---- the only test-facing fields: prompt embeddings where no BPE table / text tower exists.  text_embeddings: {"neutral_txt",
    # "target_txt", "prompt", "face_prompt", "back_prompt"} -> [1, 512]; text_feature: callable(text) -> [512] (AnimateContext's)
    text_embeddings: Any = None
    text_feature: Any = None


HOOKS = ("text_embeddings", "text_feature")
_FLAGS = {"from_stage": "from", "until_stage": "until"}


def as_spec(spec):
    if isinstance(spec, PipelineSpec):
        return spec
    known = {f.name for f in dataclasses.fields(PipelineSpec)}
    unknown = sorted(set(spec) - known)
    if unknown:
        raise ValueError("pipeline: unknown spec field(s): %s" % ", ".join(unknown))
    return PipelineSpec(**spec)


# ---------------------------------------------------------------------------------------------------------------- confs
def _load_conf(c):
    """a private copy of a conf given as a path or as a parsed tree"""
    if isinstance(c, ConfigTree):
        return copy.deepcopy(c)
    return ConfigFactory.parse_file(c)


def effective_conf(spec, which, out_dir, pretrain=None):
    """The conf a stage really runs: `which` in ("init", "appearance", "animate") with this run's directories and prompts put in."""
    conf = _load_conf(getattr(spec, which + "_conf"))
    j = lambda *p: "/".join((out_dir,) + p) if out_dir == _OUT else os.path.join(out_dir, *p)
    if which == "init":
        conf.put("general.base_exp_dir", j("exp_init"))
        conf.put("dataset.data_dir", j("render"))
    elif which == "appearance":
        conf.put("general.base_exp_dir", j("exp_clip"))
        conf.put("general.smpl_mesh", j("shape", "posed.obj"))
        conf.put("train.pretrain", pretrain if pretrain is not None else j("exp_init", "checkpoints", "<init>"))
        for key in ("prompt", "face_prompt", "back_prompt"):
            if getattr(spec, key) is not None:
                conf.put("clip." + key, getattr(spec, key))
    elif which == "animate":
        conf.put("general.base_exp_dir", j("anim"))
        if spec.motion_text is not None:
            conf.put("general.text", spec.motion_text)
    else:
        raise ValueError("no conf %r" % (which,))
    return conf


def _conf_text(spec, which):
    return json.dumps(effective_conf(spec, which, _OUT), sort_keys=True, default=str)


def _generator_types(conf):
    pose, motion = conf.get("pose_generator", default=None), conf.get("motion_generator", default=None)
    return (None if pose is None else pose.get("type", default=None)), (None if motion is None else motion.get("type", default=None))


def _motion_clip_coef(conf):
    return float(conf.get("motion_generator").get("clip_coef", default=0.001))       # animate.MotionOptimizer's default


def _animate_needs(spec, conf):
    """(image tower, text tower of the main checkpoint, text tower of the retrieval checkpoint) that the two generators of the conf use"""
    pose, motion = _generator_types(conf)
    clip_motion = motion == "MotionOptimizer" and _motion_clip_coef(conf) > 0
    image = pose in RENDERING_POSE or clip_motion
    if spec.text_feature is not None:
        return image, False, False
    retrieval = pose == "VPoserCodebook" and spec.retrieval_clip_weights is not None
    main_text = clip_motion or (pose is not None and not retrieval)
    return image, main_text, retrieval


# ---------------------------------------------------------------------------------------------------------------- assets
def _hooked(spec, *keys):
    te = spec.text_embeddings or {}
    return all(k in te for k in keys)


def _appearance_prompt_keys(spec):
    conf = _load_conf(spec.appearance_conf)
    keys = ["prompt"]
    keys += [k for k, switch in (("face_prompt", "train.use_face_prompt"), ("back_prompt", "train.use_back_prompt")) if conf.get_bool(switch, default=False)]
    return keys


def required_assets(spec, stage):
    """[(spec field, path)] of the asset FILES `stage` reads (a None path: the field is not set).  Raises what reading a conf raises."""
    s = spec
    if stage == "shape":
        a = [("template_obj", s.template_obj), ("AE_path_fname", s.AE_path_fname), ("codebook_fname", s.codebook_fname)]
        a.append(("retrieval_clip_weights", s.retrieval_clip_weights) if s.retrieval_clip_weights is not None else ("clip_weights", s.clip_weights))
        return a + ([] if _hooked(s, "neutral_txt", "target_txt") else [("bpe", s.bpe)])
    if stage == "dataset":
        return [("smpl", s.smpl)] + ([("pose_npy", s.pose_npy)] if s.pose_type == "stand_pose" else [])
    if stage == "appearance":
        return [("clip_weights", s.clip_weights)] + ([] if _hooked(s, *_appearance_prompt_keys(s)) else [("bpe", s.bpe)])
    if stage == "motion":
        conf = _load_conf(s.animate_conf)
        pose, motion = _generator_types(conf)
        a = [("smpl", s.smpl)] + ([("vposer", s.vposer)] if s.vposer is None or isinstance(s.vposer, (str, os.PathLike)) else [])
        a += {"VPoserCodebook": [("codebook", s.codebook)], "VPoserRealNVP": [("realnvp", s.realnvp)]}.get(pose, [])
        a += [("motion_vae", s.motion_vae)] if motion == "MotionOptimizer" else []
        image, main_text, retrieval = _animate_needs(s, conf)
        a += [("clip_weights", s.clip_weights)] if image or main_text else []
        a += [("retrieval_clip_weights", s.retrieval_clip_weights)] if retrieval else []
        return a + ([("bpe", s.bpe)] if main_text or retrieval else [])
    if stage in ("drive", "rig"):
        return [("smpl", s.smpl), ("pose_npy", s.pose_npy)]
    if stage == "preview":
        return [("smpl", s.smpl)]
    return []


def texture_fingerprint(path):
    """what --smpl_uv adds to the settings of the stages that render the body: nothing when it is not given (the fingerprints of runs
    without a texture do not move), else the digest of the loaded cubes -- which covers the .obj, its .mtl and the image"""
    if path is None:
        return {}
    from .texture import load_obj_texture
    return {"smpl_uv": _digest_object(load_obj_texture(path)[2])}


def check_texture(path):
    """the pre-flight of --smpl_uv: the .obj, its .mtl and its image load"""
    if path is None:
        return
    from .texture import load_obj_texture
    try:
        load_obj_texture(path)
    except (ValueError, OSError) as e:
        raise SystemExit("--smpl_uv = %s cannot be loaded: %s" % (path, e))


def _sidecar_names(codebook, tower):
    """a codebook file whose sidecar (codebook.py: <file>.json) says that `tower`'s variant made its embeddings"""
    from . import codebook as CB
    side = CB.read_sidecar(codebook) if codebook is not None else None
    return side is not None and side.get("tower") == CB.variant_name(tower)


def check_codebooks(spec, stages):
    """the pre-flight of the codebooks that carry a sidecar: one line per codebook made by another tower variant or with another texture than
    the stage will search it with.  A codebook without a sidecar adds nothing (and no checkpoint is read for it)."""
    from . import clip_vit
    from . import codebook as CB
    from .texture import load_obj_texture
    books = [(st, path) for st, path in (("shape", spec.codebook_fname), ("motion", spec.codebook)) if st in stages and path is not None]
    books = [(st, path) for st, path in books if CB.read_sidecar(path) is not None]
    if not books:
        return []
    weights = spec.retrieval_clip_weights if spec.retrieval_clip_weights is not None else spec.clip_weights
    if weights is None or not os.path.exists(weights):
        return []                                           # (reported as a missing asset)
    try:
        variant = clip_vit.vision_variant(clip_vit.load_state_dict(weights))
    except Exception as e:
        return ["%s cannot be read to compare its tower with the codebooks' sidecars: %s" % (weights, e)]
    try:
        cubes = None if spec.smpl_uv is None else load_obj_texture(spec.smpl_uv)[2]
    except (ValueError, OSError):
        return []                                           # (reported by check_texture)
    return ["%s (stage %s)" % (p, st) for st, path in books for p in CB.check_provenance(path, variant, cubes)]


_CONF_OF = {"init": ("init",), "appearance": ("appearance",), "mesh": ("appearance",), "motion": ("animate",)}


def selected_stages(spec):
    lo = STAGES.index(spec.from_stage) if spec.from_stage is not None else 0
    hi = STAGES.index(spec.until_stage) if spec.until_stage is not None else len(STAGES) - 1
    return STAGES[lo:hi + 1]


def check(spec, manifest=None):
    """Everything that can be known before the first stage runs; returns the list of problems (empty: go)."""
    spec = as_spec(spec)
    problems = []
    flag = lambda f: "--" + _FLAGS.get(f, f)
    for f in ("from_stage", "until_stage"):
        if getattr(spec, f) is not None and getattr(spec, f) not in STAGES:
            problems.append("%s %r is not a stage (%s)" % (flag(f), getattr(spec, f), ", ".join(STAGES)))
    if problems:
        return problems
    sel = selected_stages(spec)
    if not sel:
        return ["--from %s comes after --until %s" % (spec.from_stage, spec.until_stage)]
    if not spec.out_dir:
        problems.append("--out_dir is not set")
    if spec.pose_type not in ("stand_pose", "t_pose"):
        problems.append("--pose_type is stand_pose or t_pose, got %r" % (spec.pose_type,))
    if spec.posing not in ("torch", "hip"):
        problems.append("--posing is torch or hip, got %r" % (spec.posing,))
    if spec.smpl_uv is not None and any(st in sel for st in ("shape", "motion")):
        try:
            check_texture(spec.smpl_uv)
        except SystemExit as e:
            problems.append(str(e))
    confs_ok = {}
    for which in sorted({w for st in sel for w in _CONF_OF.get(st, ())}):
        c = getattr(spec, which + "_conf")
        users = ", ".join(st for st in sel if which in _CONF_OF.get(st, ()))
        if c is None:
            problems.append("%s is not set (stage %s)" % (flag(which + "_conf"), users))
        elif not isinstance(c, ConfigTree) and not os.path.isfile(c):
            problems.append("%s = %s does not exist (stage %s)" % (flag(which + "_conf"), c, users))
        else:
            try:
                confs_ok[which] = _load_conf(c)
            except Exception as e:
                problems.append("%s = %s cannot be parsed: %s" % (flag(which + "_conf"), c, e))
    seen = set()
    for st in sel:
        if any(w not in confs_ok for w in _CONF_OF.get(st, ())):
            continue
        for f, path in required_assets(spec, st):
            if (f, st) in seen:
                continue
            seen.add((f, st))
            if path is None:
                problems.append("%s is not set (stage %s)" % (flag(f), st))
            elif not os.path.exists(path):
                problems.append("%s = %s does not exist (stage %s)" % (flag(f), path, st))
    pose_book = ("motion" in sel and "animate" in confs_ok and _generator_types(confs_ok["animate"])[0] == "VPoserCodebook"
                 and spec.text_feature is None)            # (a hooked text feature: no tower of this run meets the pose codebook)
    problems += check_codebooks(spec, [st for st in sel if st == "shape" or (st == "motion" and pose_book)])
    if "motion" in sel and "animate" in confs_ok:
        from . import animate as A
        conf = confs_ok["animate"]
        pose, motion = _generator_types(conf)
        if pose not in A.POSE_GENERATORS:
            problems.append("pose_generator.type = %r of the AvatarAnimate conf is none of %s" % (pose, ", ".join(A.POSE_GENERATORS)))
        if motion not in A.MOTION_GENERATORS:
            problems.append("motion_generator.type = %r of the AvatarAnimate conf is none of %s" % (motion, ", ".join(A.MOTION_GENERATORS)))
        if not spec.renderer_gradient:
            if pose in CLIP_GUIDED_POSE:
                problems.append("pose_generator %s optimises the CLIP score through the rasteriser: it needs --renderer_gradient" % pose)
            if motion == "MotionOptimizer" and _motion_clip_coef(conf) > 0:
                problems.append("motion_generator MotionOptimizer with clip_coef = %g needs --renderer_gradient (or clip_coef = 0)" % _motion_clip_coef(conf))
        if conf.get_string("general.mode", default="motion") == "pose" and any(st in sel for st in ("drive", "rig", "preview")):
            problems.append("general.mode = pose of the AvatarAnimate conf writes no motion.npy, which the stages drive, rig and preview read")
        if spec.motion_text is None and conf.get("general.text", default=None) is None:
            problems.append("no motion text: --motion_text is not set and the AvatarAnimate conf has no general.text")
        if isinstance(spec.vposer, (str, os.PathLike)) and importlib.util.find_spec("human_body_prior") is None:
            problems.append("--vposer = %s is read by the `human_body_prior` package, which is not installed" % spec.vposer)
    done = {} if manifest is None else manifest.get("stages", {})
    for st in sel:
        for up in CONSUMES[st]:
            if up not in sel and done.get(up, {}).get("status") != "done":
                problems.append("stage %s reads the outputs of stage %s, which is outside the range and has not finished in %s" % (st, up, MANIFEST))
    return problems


# ---------------------------------------------------------------------------------------------------------------- fingerprints
def _sha256_file(path, cache):
    """sha256 of a file, or of a directory's files (relative name + content, sorted: VPoser's model directory)"""
    if path is None or not os.path.exists(path):
        return "missing"
    key = os.path.abspath(path)
    if key not in cache:
        h = hashlib.sha256()
        if os.path.isdir(path):
            names = sorted(os.path.relpath(os.path.join(d, f), path) for d, _, fs in os.walk(path) for f in fs)
        else:
            names = [None]
        for n in names:
            if n is not None:
                h.update(n.encode() + b"\0")
            with open(path if n is None else os.path.join(path, n), "rb") as fh:
                for block in iter(lambda: fh.read(1 << 22), b""):
                    h.update(block)
        cache[key] = h.hexdigest()
    return cache[key]


def _digest_object(x):
    """a tensor / array by its bytes, a module by its state dict, anything else by its type's name"""
    h = hashlib.sha256()
    if hasattr(x, "state_dict"):
        for k, v in sorted(x.state_dict().items()):
            h.update(k.encode() + b"\0" + _digest_object(v).encode())
    elif hasattr(x, "detach"):
        a = x.detach().cpu().contiguous().numpy()
        h.update(str((a.dtype, a.shape)).encode() + a.tobytes())
    elif hasattr(x, "tobytes"):
        h.update(x.tobytes())
    else:
        h.update(("%s.%s" % (type(x).__module__, type(x).__qualname__)).encode())
    return h.hexdigest()


def _hook_digests(spec, keys):
    te = spec.text_embeddings or {}
    return {k: _digest_object(te[k]) for k in keys if k in te}


def stage_settings(spec, stage):
    """what `stage` reads besides files: prompts, knobs, the effective conf text"""
    s = spec
    if stage == "shape":
        return dict({"neutral_txt": s.neutral_txt, "target_txt": s.target_txt, "latent_dim": SHAPE_LATENT_DIM,
                     "text_embeddings": _hook_digests(s, ("neutral_txt", "target_txt"))}, **texture_fingerprint(s.smpl_uv))
    if stage == "dataset":
        return {"pose_type": s.pose_type, "image_size": int(s.image_size)}
    if stage == "init":
        return {"conf": _conf_text(s, "init")}
    if stage == "appearance":
        return {"conf": _conf_text(s, "appearance"), "text_embeddings": _hook_digests(s, ("prompt", "face_prompt", "back_prompt"))}
    if stage == "mesh":
        return {"resolution": int(s.mesh_resolution), "threshold": float(s.mcube_threshold)}
    if stage == "motion":
        conf = effective_conf(s, "animate", _OUT)
        out = {"conf": json.dumps(conf, sort_keys=True, default=str), "renderer_gradient": bool(s.renderer_gradient), "posing": s.posing}
        if s.text_feature is not None:
            out["text_feature"] = _digest_object(s.text_feature(conf.get_string("general.text")))
        if s.vposer is not None and not isinstance(s.vposer, (str, os.PathLike)):
            out["vposer"] = _digest_object(s.vposer)
        out.update(texture_fingerprint(s.smpl_uv))
        return out
    if stage == "drive":
        return {"name": s.name}
    if stage == "rig":
        out = {"name": s.name, "voxel_divisor": int(s.voxel_divisor)}
        if int(s.bake_texture):                                 # (only when asked for: manifests from before the option keep their fingerprints)
            out["bake_texture"] = int(s.bake_texture)
        return out
    if stage == "preview":
        return {"size": int(s.preview_size), "views": int(s.preview_views)}
    raise ValueError("no stage %r" % (stage,))


def fingerprints(spec):
    """{stage: sha256 hex} for ALL stages, in order (a stage's fingerprint holds those of the stages it consumes).  A stage whose conf
    or assets are not given gets a fingerprint all the same ("missing"): `check` is what refuses to run it."""
    spec = as_spec(spec)
    cache, out = {}, {}
    for st in STAGES:
        try:
            settings = stage_settings(spec, st)
            assets = {f: _sha256_file(p, cache) for f, p in required_assets(spec, st)}
        except Exception as e:               # a conf that is not there: only a stage outside the range gets this far
            settings, assets = {"unavailable": type(e).__name__}, {}
        doc = {"version": MANIFEST_VERSION, "stage": st, "settings": settings, "assets": assets, "consumes": {u: out[u] for u in CONSUMES[st]}}
        out[st] = hashlib.sha256(json.dumps(doc, sort_keys=True).encode()).hexdigest()
    return out


# ---------------------------------------------------------------------------------------------------------------- manifest
def load_manifest(out_dir):
    path = os.path.join(out_dir, MANIFEST)
    if os.path.isfile(path):
        with open(path) as fh:
            m = json.load(fh)
        if m.get("version") == MANIFEST_VERSION and isinstance(m.get("stages"), dict):
            return m
    return {"version": MANIFEST_VERSION, "stages": {}}


def write_manifest(out_dir, manifest):
    """atomically: a temporary file beside it, then os.replace"""
    path = os.path.join(out_dir, MANIFEST)
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        json.dump(manifest, fh, indent=1, sort_keys=True)
        fh.flush()
        os.fsync(fh.fileno())
    os.replace(tmp, path)


def _describe(out_dir, path):
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for block in iter(lambda: fh.read(1 << 22), b""):
            h.update(block)
    return {"path": os.path.relpath(path, out_dir), "size": os.path.getsize(path), "sha256": h.hexdigest()}


def up_to_date(record, fingerprint, out_dir):
    """the skip rule: finished, the same fingerprint, every recorded output there with the recorded size (contents are NOT re-hashed)"""
    if not record or record.get("status") != "done" or record.get("fingerprint") != fingerprint:
        return False
    for o in record.get("outputs", {}).values():
        p = os.path.join(out_dir, o["path"])
        if not os.path.isfile(p) or os.path.getsize(p) != o["size"]:
            return False
    return True


# ---------------------------------------------------------------------------------------------------------------- what the stages share
class Run:
    """One run's shared state: the device, the ONE tower (and the retrieval tower when a second checkpoint is given), the ONE tokenizer,
    and the recorded outputs of the finished stages"""

    def __init__(self, spec, manifest):
        self.spec, self.manifest, self.out_dir = spec, manifest, spec.out_dir
        self._device = self._tokenizer = self._vposer = None
        self._towers = {}
        # set by `run` before a stage is called: every stage's fingerprint (the tag of the Runner's resume records), the stages to continue
        # inside (continue_stage); set by the stage: the step its Runner continued from
        self.fingerprints, self.resume, self.resumed_from = {}, set(), {}

    @property
    def device(self):
        if self._device is None:
            import torch
            if not torch.cuda.is_available():
                raise RuntimeError("avatarclip_amd.pipeline needs an MI355X (torch.cuda): its stages have no CPU fallback")
            torch.cuda.set_device(int(self.spec.gpu))
            self._device = torch.device("cuda", int(self.spec.gpu))
        return self._device

    def dir(self, *parts):
        d = os.path.join(self.out_dir, *parts)
        os.makedirs(d, exist_ok=True)
        return d

    def output(self, stage, key):
        """the file a finished stage recorded under `key`"""
        rec = self.manifest["stages"].get(stage, {})
        if rec.get("status") != "done" or key not in rec.get("outputs", {}):
            raise RuntimeError("pipeline: stage %s has no finished output %r in %s" % (stage, key, MANIFEST))
        return os.path.join(self.out_dir, rec["outputs"][key]["path"])

    def conf(self, which):
        pretrain = self.output("init", "checkpoint") if which == "appearance" else None
        return effective_conf(self.spec, which, self.out_dir, pretrain)

    def conf_path(self, which):
        c = getattr(self.spec, which + "_conf")
        return None if isinstance(c, ConfigTree) else c

    def tokenizer(self):
        if self._tokenizer is None:
            from .tokenizer import SimpleTokenizer
            self._tokenizer = SimpleTokenizer(self.spec.bpe)
        return self._tokenizer

    def tower(self, retrieval=False, codebook=None):
        """the main tower; retrieval=True: the tower that searches the codebooks -- the second checkpoint's when one is given.  `codebook`:
        the file the stage is about to search; when its sidecar (codebook.py) names the main tower's variant there is nothing to warn about"""
        global _B16_WARNED
        from . import clip_vit
        key = "retrieval" if retrieval and self.spec.retrieval_clip_weights is not None else "main"
        if key not in self._towers:
            sd = clip_vit.load_state_dict(self.spec.retrieval_clip_weights if key == "retrieval" else self.spec.clip_weights)
            self._towers[key] = clip_vit.ClipVision(sd, self.device)
        t = self._towers[key]
        if retrieval and key == "main" and t.patch == 16 and not _B16_WARNED and not _sidecar_names(codebook, t):
            _B16_WARNED = True
            warnings.warn("the main CLIP checkpoint is ViT-B/16 and no --retrieval_clip_weights is given: the shipped shape and pose codebooks hold "
                          "ViT-B/32 embeddings and are searched with the wrong tower (README, paragraph \"ViT-B/32 or ViT-B/16\")")
        return t

    def encode_text(self, tower, text):
        """[1, 512] of a prompt: the tower's text tower on the ONE tokenizer (shapegen.main's and Runner.init_clip's two calls)"""
        from .tokenizer import tokenize
        return tower.encode_text(tokenize([text], self.tokenizer()).to(self.device)).float()

    def text_embedding(self, key, text, tower):
        te = self.spec.text_embeddings or {}
        if key in te:
            return te[key].to(self.device).float().reshape(1, -1)
        return self.encode_text(tower, text)

    def vposer(self):
        if self._vposer is None:
            vp = self.spec.vposer
            if isinstance(vp, (str, os.PathLike)):              # animate.main's loader
                from human_body_prior.models.vposer_model import VPoser
                from human_body_prior.tools.model_loader import load_model
                vp, _ = load_model(str(vp), model_code=VPoser, remove_words_in_model_weights="vp_model.", disable_grad=True)
            self._vposer = vp.to(self.device).eval() if hasattr(vp, "to") else vp
        return self._vposer


def _final_checkpoint(runner):
    """the checkpoint of the runner's last step; written here when train.save_freq does not divide train.end_iter"""
    path = os.path.join(runner.base_exp_dir, "checkpoints", "ckpt_{:0>6d}.pth".format(runner.iter_step))
    if not os.path.isfile(path):
        runner.save_checkpoint()
    return path


# ---------------------------------------------------------------------------------------------------------------- the stages
# Each takes the Run and returns {key: path} of what it wrote.  `run` looks them up by name when it calls them.
def stage_shape(run):
    from . import shapegen as SG
    from .smpl_prior import read_obj
    s, dev = run.spec, run.device
    v_template, faces = read_obj(s.template_obj)
    model_AE = SG.create_load_AE(v_template.size, SHAPE_LATENT_DIM, v_template, s.AE_path_fname, dev)
    codebook, clip_codebook = SG.load_codebook(s.codebook_fname, dev)
    tower = run.tower(retrieval=True, codebook=s.codebook_fname)
    nembed = run.text_embedding("neutral_txt", SG.parse_prompt(s.neutral_txt)[0], tower)
    tembed = run.text_embedding("target_txt", SG.parse_prompt(s.target_txt)[0], tower)
    render_fn = SG.textured_render_fn(faces, s.smpl_uv, dev) if s.smpl_uv is not None else None
    v, _, best, cos = SG.shape_gen(model_AE, faces, tower, codebook, clip_codebook, nembed, tembed, render_fn=render_fn)
    obj, doc = os.path.join(run.dir("shape"), "coarse_shape.obj"), os.path.join(run.dir("shape"), "shape.json")
    SG.writeOBJ(obj, v, faces)
    cos = [float(c) for c in cos.reshape(-1).cpu()]
    with open(doc, "w") as fh:
        json.dump({"code": int(best), "cosine": cos[int(best)], "cosines": cos, "target_txt": s.target_txt, "neutral_txt": s.neutral_txt}, fh, indent=1)
    return {"obj": obj, "json": doc}


def stage_dataset(run):
    from . import shapegen as SG
    from . import shapegen_render as SR
    from .smpl_prior import read_obj
    s = run.spec
    v, _ = read_obj(run.output("shape", "obj"))
    v, f = SR.pose_shape(v, s.smpl, s.pose_type, s.pose_npy, run.device)
    posed = os.path.join(run.dir("shape"), "posed.obj")
    SG.writeOBJ(posed, v, f)
    data_dir = run.dir("render")
    _, transforms = SR.write_nerf_dataset(data_dir, v, f, device=run.device, image_size=int(s.image_size))
    out = {"posed_obj": posed, "transforms": os.path.join(data_dir, "transforms_train.json")}
    out.update({"img_%04d" % i: os.path.join(data_dir, "img", "%s.png" % str(i).zfill(4)) for i in range(len(transforms))})
    return out


def stage_init(run):
    from .runner import Runner
    r = Runner(run.conf_path("init"), mode="train", conf=run.conf("init"), device=run.device, resume="init" in run.resume,
               resume_tag=run.fingerprints.get("init"))
    run.resumed_from["init"] = r.resumed_from
    r.train()
    return {"checkpoint": _final_checkpoint(r)}


def stage_appearance(run):
    from .runner import Runner
    s = run.spec
    r = Runner(run.conf_path("appearance"), mode="train_clip", conf=run.conf("appearance"), device=run.device, resume="appearance" in run.resume,
               resume_tag=run.fingerprints.get("appearance"))
    run.resumed_from["appearance"] = r.resumed_from
    keys = [k for k in ("prompt", "face_prompt", "back_prompt") if k in (s.text_embeddings or {})]
    r.init_clip(perceptor=run.tower(), text_embeddings={k: s.text_embeddings[k] for k in keys} or None,
                tokenizer=run.tokenizer() if s.bpe is not None else None)
    r.init_smpl()
    r.train_clip()
    return {"checkpoint": _final_checkpoint(r)}


def stage_mesh(run):
    from .runner import Runner
    s = run.spec
    r = Runner(run.conf_path("appearance"), mode="validate_mesh", is_continue=True, conf=run.conf("appearance"), device=run.device)
    return {"ply": r.validate_mesh(world_space=True, resolution=int(s.mesh_resolution), threshold=float(s.mcube_threshold))}


def stage_motion(run):
    from . import animate as A
    from . import smpl_lbs
    s, dev = run.spec, run.device
    conf = run.conf("animate")
    pose, motion = _generator_types(conf)
    image, main_text, retrieval = _animate_needs(s, conf)
    smpl, vp = smpl_lbs.load_smpl_arrays(s.smpl, dev), run.vposer()
    kw = dict(device=dev, renderer_gradient=bool(s.renderer_gradient), posing=s.posing, texture=s.smpl_uv)
    feature_of = lambda tower: s.text_feature if s.text_feature is not None else (lambda text: run.encode_text(tower, text)[0])
    main = run.tower() if image or main_text else None
    ctx = A.AnimateContext(main, feature_of(main), smpl, vp, **kw)
    pose_ctx = None
    if retrieval:                      # the pose codebook's ViT-B/32 embeddings against the ViT-B/32 text tower
        second = run.tower(retrieval=True)
        pose_ctx = A.AnimateContext(second, feature_of(second), smpl, vp, **kw)
    elif pose == "VPoserCodebook" and main is not None:
        run.tower(retrieval=True, codebook=s.codebook)      # (the main tower again: warns once when it is a ViT-B/16 that did not make the codebook)
    pose_assets = {"VPoserCodebook": {"codebook_path": s.codebook}, "VPoserRealNVP": {"ckpt_path": s.realnvp}}.get(pose, {})
    motion_assets = {"ckpt_path": s.motion_vae} if motion == "MotionOptimizer" else {}
    poses, _ = A.run(conf, ctx, pose_assets=pose_assets, motion_assets=motion_assets, pose_ctx=pose_ctx)
    d = conf.get_string("general.base_exp_dir")
    out = {"candidate_%d" % i: os.path.join(d, "candidate_%d.npy" % i) for i in range(poses.shape[0])}
    if conf.get_string("general.mode") != "pose":
        out["motion"] = os.path.join(d, "motion.npy")
    return out


def stage_drive(run):
    from . import drive
    s = run.spec
    ply, pc2 = drive.generate_animation(run.output("mesh", "ply"), run.output("motion", "motion"), s.smpl, s.pose_npy, run.dir("drive"), name=s.name,
                                        device=run.device)
    return {"ply": ply, "pc2": pc2}


def stage_rig(run):
    from . import rig
    s = run.spec
    glb, npz = rig.build_rig(run.output("mesh", "ply"), s.smpl, s.pose_npy, run.dir("rig"), name=s.name, motion=run.output("motion", "motion"),
                             voxel_divisor=int(s.voxel_divisor), device=run.device, bake_texture=int(s.bake_texture))
    out = {"glb": glb, "npz": npz}
    if int(s.bake_texture):
        out["texture"] = os.path.join(run.dir("rig"), "%s_texture.png" % s.name)
    return out


def stage_preview(run):
    from . import preview as P
    s, d = run.spec, run.dir("preview")
    run.device                                                           # (preview renders on the current device)
    kw = dict(views=int(s.preview_views), size=int(s.preview_size))
    out = {}
    out["mesh"] = P.preview(os.path.join(d, "mesh.gif"), mesh=run.output("mesh", "ply"), **kw)[0]
    out["drive"] = P.preview(os.path.join(d, "drive.gif"), mesh=run.output("drive", "ply"), pc2=run.output("drive", "pc2"), **kw)[0]
    out["rig"] = P.preview(os.path.join(d, "rig.gif"), glb=run.output("rig", "glb"), up="z", **kw)[0]      # the tracks carry drive's root rotation
    out["motion"] = P.preview(os.path.join(d, "motion.gif"), smpl=s.smpl, poses=run.output("motion", "motion"), **kw)[0]
    return out


# ---------------------------------------------------------------------------------------------------------------- the run
def _sync():
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()


RESUMABLE = ("init", "appearance")       # the stages that are a Runner's optimisation loop


def continue_stage(spec, stage, record, fingerprint):
    """the rule: a resumable stage is continued inside exactly when its previous run did not finish (`running`: killed, `failed`: an
    exception) under the fingerprint it has now, and the caller did not ask for a fresh start"""
    return (stage in RESUMABLE and not spec.force and not spec.restart_stages and bool(record)
            and record.get("status") in ("running", "failed") and record.get("fingerprint") == fingerprint)


def run(spec, log=print):
    """Check everything, then run the selected stages that are not up to date.  Returns {"out_dir", "stages": {stage: "ran" | "skipped" |
    "not selected"}, "manifest": the manifest as written}."""
    spec = as_spec(spec)
    manifest = load_manifest(spec.out_dir) if spec.out_dir else None
    problems = check(spec, manifest)
    if problems:
        raise ValueError("pipeline: %d problem(s) before the first stage:\n%s" % (len(problems), "\n".join("  - " + p for p in problems)))
    selected = selected_stages(spec)
    fps = fingerprints(spec)
    os.makedirs(spec.out_dir, exist_ok=True)
    shared = Run(spec, manifest)
    shared.fingerprints = dict(fps)
    report = {}
    for st in STAGES:
        if st not in selected:
            report[st] = "not selected"
            continue
        if not spec.force and up_to_date(manifest["stages"].get(st), fps[st], spec.out_dir):
            report[st] = "skipped"
            log("[pipeline] %-10s up to date" % st)
            continue
        if continue_stage(spec, st, manifest["stages"].get(st), fps[st]):
            shared.resume.add(st)
        manifest["stages"][st] = {"status": "running", "fingerprint": fps[st]}
        write_manifest(spec.out_dir, manifest)
        t0 = time.perf_counter()
        try:
            outputs = globals()["stage_" + st](shared)
            _sync()
            record = {"status": "done", "fingerprint": fps[st], "seconds": round(time.perf_counter() - t0, 3),
                      "outputs": {k: _describe(spec.out_dir, p) for k, p in sorted(outputs.items())}}
            if shared.resumed_from.get(st) is not None:
                record["resumed_from"] = int(shared.resumed_from[st])
        except BaseException as e:
            manifest["stages"][st] = {"status": "failed", "fingerprint": fps[st], "seconds": round(time.perf_counter() - t0, 3), "error": repr(e)[:2000]}
            write_manifest(spec.out_dir, manifest)
            raise
        manifest["stages"][st] = record
        write_manifest(spec.out_dir, manifest)
        report[st] = "ran"
        log("[pipeline] %-10s %8.2f s, %d file(s)" % (st, record["seconds"], len(record["outputs"])))
    return {"out_dir": spec.out_dir, "stages": report, "manifest": manifest}


# ---------------------------------------------------------------------------------------------------------------- command line
def build_parser():
    """one flag per PipelineSpec field (the test-facing hooks excepted), named like the stage CLIs name theirs"""
    ap = argparse.ArgumentParser(prog="python -m avatarclip_amd.pipeline", description=__doc__.split("\n\n")[0])
    for f in dataclasses.fields(PipelineSpec):
        if f.name in HOOKS:
            continue
        flag = "--" + _FLAGS.get(f.name, f.name)
        if f.type is bool:
            ap.add_argument(flag, dest=f.name, action="store_true", default=f.default)
        elif f.name in ("from_stage", "until_stage"):
            ap.add_argument(flag, dest=f.name, choices=STAGES, default=None)
        else:
            ap.add_argument(flag, dest=f.name, type=f.type if f.type in (int, float) else str, default=f.default, required=f.name == "out_dir")
    return ap


def spec_from_args(argv=None):
    return PipelineSpec(**vars(build_parser().parse_args(argv)))


def main(argv=None):
    spec = spec_from_args(argv)
    try:
        result = run(spec)
    except ValueError as e:
        raise SystemExit(str(e))
    print(os.path.join(result["out_dir"], MANIFEST))


if __name__ == "__main__":
    main()
