"""Build and re-encode the two CLIP codebooks the pipeline searches: ShapeGen's (16-d LinearVAE codes and the CLIP embedding of each decoded
body, AvatarGen/ShapeGen/main.py:86-118) and AvatarAnimate's (32-d VPoser codes and the mean five-view embedding of each decoded pose,
AvatarAnimate/models/pose_generation.py:288-329).  The reference ships both as files and no code that makes them (main.py:86-91 and
pose_generation.py:298-300 only load them); the paper makes them by K-Means over latents sampled from the shape VAE and over VPoser latents of
a pose corpus.  Here:

    python -m avatarclip_amd.codebook shape-build    --AE_path_fname model_VAE_16.pth --template_obj zero_beta_smpl.obj --clip_weights ViT-B-16.pt \\
                                                     --k 2048 --n_samples 200000 --out shape_codebook.pth [--smpl_uv smpl_uv.obj]
    python -m avatarclip_amd.codebook shape-reencode --codebook_fname data/codebook.pth --AE_path_fname ... --template_obj ... --clip_weights ViT-B-16.pt --out ...
    python -m avatarclip_amd.codebook pose-build     --poses poses.npy --smpl SMPL_NEUTRAL.pkl --vposer data/vposer --clip_weights ... --k 4096 --out pose_codebook.pth
    python -m avatarclip_amd.codebook pose-reencode  --codebook data/codebook.pth --smpl ... --vposer ... --clip_weights ... --out ...

Every step runs on the kernels the consumers use: kmeans.kmeans (csrc/avc_codebook.hip) for the centres, LinearVAE.decode / VPoser's decoder,
mesh_render.render_batch under the cameras of the stage that will search the file (shapegen.render_body / textured_render_fn for shapes,
AnimateContext.get_pose_feature for poses), clip_score.render_embedding.  A codebook matches a run only when the same tower AND the same
texture made its embeddings, so each file gets a sidecar `<file>.json` that names them; pipeline.py reads it (check_provenance).  A re-encode
keeps the codes bit for bit and recomputes the embeddings alone.  The pose corpus is the user's: an [N, 63] array of body poses."""
import argparse
import hashlib
import io
import json
import os

import numpy as np
import torch

from . import clip_score
from . import kmeans as KM

SHAPE_CAMERA = dict(camera_distance=2.0, elevation=0.0, angles=(150,))        # ShapeGen/utils.py:10-27, as shapegen.render_body sets it
SIDECAR_VERSION = 1
WHITE = "white"


# ----------------------------------------------------------------------------------------------------------------- embeddings
@torch.no_grad()
def embed_shapes(model_AE, codes, faces, perceptor, render_fn=None, texture=None, image_size=256, chunk=256):
    """CLIP embedding of every decoded shape -> [K, 512] fp32.  In chunks: model_AE.decode, ONE mesh_render.render_batch call per chunk under
    ShapeGen's camera exactly as shapegen.render_body (white body) / shapegen.textured_render_fn (`texture`: the path of a textured .obj or its
    cubes) set it -- distance 2, elevation 0, azimuth 150, apply_rot_mat=False -- then clip_score.render_embedding.  `render_fn` (shape_gen's
    hook: vertices [V,3] array -> images [n,3,S,S]) replaces the render, one body at a time, the embedding averaged over its images."""
    from . import shapegen as SG
    from .mesh_render import render_batch
    dev = codes.device
    out = []
    if render_fn is not None:
        for c in codes:
            v = model_AE.decode(c.reshape(1, -1))
            out.append(clip_score.render_embedding(perceptor, render_fn(v[0].cpu().numpy())).mean(0))
        return torch.stack(out) if out else torch.zeros(0, 512, device=dev)
    cubes = None
    if texture is not None:
        from .texture import as_cubes
        cubes = as_cubes(texture, dev)
    # render_body hands float64 eyes to the renderer, textured_render_fn float32 ones: each path keeps the rounding it has always had
    eyes, dirs = SG.look_at_cameras(SHAPE_CAMERA["camera_distance"], SHAPE_CAMERA["elevation"], SHAPE_CAMERA["angles"],
                                    np.float64 if cubes is None else np.float32)
    for i in range(0, codes.shape[0], int(chunk)):
        v = model_AE.decode(codes[i:i + int(chunk)]).float().contiguous()
        images = render_batch(v, faces, eyes * v.shape[0], dirs * v.shape[0], cubes, image_size=image_size, apply_rot_mat=False)
        out.append(clip_score.render_embedding(perceptor, images))
    return torch.cat(out) if out else torch.zeros(0, 512, device=dev)


@torch.no_grad()
def embed_poses(ctx, codes, chunk=256, seed=0):
    """mean five-view CLIP embedding of every decoded pose -> [K, 512] fp32: in chunks, ctx.vp.decode(codes)["pose_body"] then
    ctx.get_pose_feature -- the path VPoserCodebook's scores are compared with, per-angle elevation draw included.  That draw comes from
    numpy's global generator: it is seeded with `seed` at the start of EVERY chunk (each entry sees the same five cameras, whatever the chunk
    size) and the caller's state is put back afterwards."""
    state = np.random.get_state()
    out = []
    try:
        for i in range(0, codes.shape[0], int(chunk)):
            np.random.seed(int(seed))
            z = codes[i:i + int(chunk)].float().to(ctx.device)
            pose = ctx.vp.decode(z)["pose_body"].reshape(z.shape[0], -1)
            out.append(ctx.get_pose_feature(pose).float())
    finally:
        np.random.set_state(state)
    return torch.cat(out) if out else torch.zeros(0, 512, device=ctx.device)


# ----------------------------------------------------------------------------------------------------------------- builders
def build_shape_codebook(model_AE, k, n_samples, seed, faces, perceptor, render_fn=None, texture=None, image_size=256, chunk=256, iters=100):
    """`n_samples` latents from N(0, I) under torch.Generator().manual_seed(seed) (drawn on the host), kmeans(k, seed), embed_shapes
    -> (codes [k, latent_dim], embeddings [k, 512], kmeans' info)"""
    dev = model_AE.dec2.weight.device
    z = torch.randn(int(n_samples), int(model_AE.latent_dim), generator=torch.Generator().manual_seed(int(seed))).to(dev)
    codes, _, info = KM.kmeans(z, k, iters=iters, seed=seed)
    return codes, embed_shapes(model_AE, codes, faces, perceptor, render_fn, texture, image_size, chunk), info


@torch.no_grad()
def encode_poses(ctx, poses, chunk=256):
    """VPoser latents of body poses [N, 63] (or [N, 21, 3]): ctx.vp.encode(poses).mean in chunks -> [N, 32] fp32 on the device"""
    p = torch.as_tensor(np.asarray(poses) if not torch.is_tensor(poses) else poses).float()
    p = p.reshape(p.shape[0], -1)
    if p.dim() != 2 or p.shape[1] != 63 or p.shape[0] == 0:
        raise ValueError("the pose corpus is [N, 63] body poses (21 joints, axis-angle), got %s" % (list(p.shape),))
    if not bool(torch.isfinite(p).all()):
        raise ValueError("the pose corpus holds a value that is not finite")
    return torch.cat([ctx.vp.encode(p[i:i + int(chunk)].to(ctx.device)).mean.float() for i in range(0, p.shape[0], int(chunk))]).contiguous()


def build_pose_codebook(ctx, poses, k, seed, chunk=256, iters=100):
    """encode_poses, kmeans(k, seed), embed_poses(seed) -> (codes [k, 32], embeddings [k, 512], kmeans' info)"""
    codes, _, info = KM.kmeans(encode_poses(ctx, poses, chunk), k, iters=iters, seed=seed)
    return codes, embed_poses(ctx, codes, chunk, seed), info


# ----------------------------------------------------------------------------------------------------------------- files
def read_shape_codebook(path):
    """(codes, embeddings) on the host, as shapegen.load_codebook reads the file"""
    from .shapegen import load_codebook
    return load_codebook(path, "cpu")


def read_pose_codebook(path):
    d = torch.load(path, map_location="cpu", weights_only=True)
    return d["codebook"], d["codebook_embedding"]


def _save_atomically(obj, path):
    buf = io.BytesIO()
    torch.save(obj, buf)                                   # (through a buffer: torch.save names the archive after the FILE it is given, and the
    tmp = "%s.tmp.%d" % (path, os.getpid())                #  bytes of a codebook must not depend on the temporary name)
    try:
        with open(tmp, "wb") as fh:
            fh.write(buf.getvalue())
            fh.flush()
            os.fsync(fh.fileno())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def write_shape_codebook(path, codes, embeddings, sidecar=None):
    """{codes: embeddings}, ONE entry keyed by the tensor and nothing else: ShapeGen/main.py:86-91 returns the last key of the file.
    Tensors only; a temporary name, then os.replace; then the sidecar (write_sidecar)."""
    codes, embeddings = codes.detach().float().cpu().contiguous(), embeddings.detach().float().cpu().contiguous()
    if codes.dim() != 2 or embeddings.dim() != 2 or codes.shape[0] != embeddings.shape[0]:
        raise ValueError("a shape codebook is codes [K, D] and embeddings [K, 512], got %s and %s" % (list(codes.shape), list(embeddings.shape)))
    _save_atomically({codes: embeddings}, path)
    if sidecar is not None:
        write_sidecar(path, sidecar)


def write_pose_codebook(path, codes, embeddings, sidecar=None):
    """{"codebook", "codebook_embedding"} as pose_generation.py:298-300 reads it; written like write_shape_codebook"""
    codes, embeddings = codes.detach().float().cpu().contiguous(), embeddings.detach().float().cpu().contiguous()
    if codes.dim() != 2 or embeddings.dim() != 2 or codes.shape[0] != embeddings.shape[0]:
        raise ValueError("a pose codebook is codes [K, D] and embeddings [K, 512], got %s and %s" % (list(codes.shape), list(embeddings.shape)))
    _save_atomically({"codebook": codes, "codebook_embedding": embeddings}, path)
    if sidecar is not None:
        write_sidecar(path, sidecar)


# ----------------------------------------------------------------------------------------------------------------- provenance
SIDECAR_KEYS = ("version", "kind", "K", "D", "tower", "clip_sha256", "texture", "image_size", "seed", "n_samples", "n_poses", "kmeans_iterations",
                "final_inertia", "empty")


def sidecar_path(path):
    return str(path) + ".json"


def variant_name(variant):
    """"ViT-B/32" / "ViT-B/16" of clip_vit.vision_variant's (patch, tokens), a patch size, a tower (its .patch) or the name itself"""
    if isinstance(variant, str):
        return variant
    patch = getattr(variant, "patch", variant)
    if isinstance(patch, (tuple, list)):
        patch = patch[0]
    return "ViT-B/%d" % int(patch)


def file_sha256(path):
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for block in iter(lambda: fh.read(1 << 22), b""):
            h.update(block)
    return h.hexdigest()


def texture_digest(texture):
    """"white" for None, else the sha256 of the bytes of the loaded float32 cubes (pipeline.texture_fingerprint's digest of --smpl_uv, which
    covers the .obj, its .mtl and the image); `texture`: the path of the textured .obj or the cubes"""
    if texture is None:
        return WHITE
    if isinstance(texture, (str, os.PathLike)):
        from .texture import load_obj_texture
        texture = load_obj_texture(os.fspath(texture))[2]
    a = texture.detach().cpu().numpy() if hasattr(texture, "detach") else np.asarray(texture)
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def make_sidecar(kind, codes, tower, clip_sha256, texture, image_size, seed=None, n_samples=None, n_poses=None, info=None):
    """the provenance of a codebook file: what made its embeddings (tower variant, sha256 of the CLIP weights, texture digest or "white",
    image size, the seed of the draws) and, for a built one, what made its codes (n_samples / n_poses, k-means' iterations, final inertia
    and empty clusters; None in a re-encoded file, whose codes came from elsewhere)"""
    if kind not in ("shape", "pose"):
        raise ValueError("a codebook is of kind shape or pose, got %r" % (kind,))
    info = info or {}
    return {"version": SIDECAR_VERSION, "kind": kind, "K": int(codes.shape[0]), "D": int(codes.shape[1]), "tower": variant_name(tower),
            "clip_sha256": clip_sha256, "texture": texture_digest(texture), "image_size": int(image_size),
            "seed": None if seed is None else int(seed), "n_samples": None if n_samples is None else int(n_samples),
            "n_poses": None if n_poses is None else int(n_poses), "kmeans_iterations": info.get("iterations"),
            "final_inertia": info.get("final_inertia"), "empty": info.get("empty")}


def write_sidecar(path, sidecar):
    """<path>.json, atomically"""
    target = sidecar_path(path)
    tmp = "%s.tmp.%d" % (target, os.getpid())
    with open(tmp, "w") as fh:
        json.dump(sidecar, fh, indent=1, sort_keys=True)
        fh.write("\n")
    os.replace(tmp, target)


def read_sidecar(path):
    """the sidecar of a codebook file, or None when it has none"""
    if path is None or not os.path.isfile(sidecar_path(path)):
        return None
    with open(sidecar_path(path)) as fh:
        return json.load(fh)


def check_provenance(path, tower_variant, texture):
    """What is wrong with searching the codebook `path` with a tower of `tower_variant` (see variant_name) on renders of `texture` (None:
    the white body; a path or cubes) -> a list of problems, one line each.  Empty when all matches -- and when the file has no sidecar: a
    shipped codebook says nothing about itself and is used as before."""
    side = read_sidecar(path) if path is not None else None
    if side is None:
        return []
    problems = []
    want = variant_name(tower_variant)
    if side.get("tower") != want:
        problems.append("the codebook %s holds %s embeddings (%s) and would be searched with a %s tower: re-encode it "
                        "(python -m avatarclip_amd.codebook %s-reencode)" % (path, side.get("tower"), sidecar_path(path), want, side.get("kind", "shape")))
    have = texture_digest(texture)
    if side.get("texture") != have:
        name = lambda t: "the white body" if t == WHITE else "the texture %s" % str(t)[:12]
        problems.append("the codebook %s was made with %s and this run renders %s: re-encode it with the same --smpl_uv "
                        "(python -m avatarclip_amd.codebook %s-reencode)" % (path, name(side.get("texture")), name(have), side.get("kind", "shape")))
    return problems


# ----------------------------------------------------------------------------------------------------------------- re-encoding
def reencode_shape(path, model_AE, faces, perceptor, render_fn=None, texture=None, image_size=256, chunk=256):
    """the codes of the shape codebook `path` as they are (bit for bit) with embeddings recomputed by embed_shapes -> (codes, embeddings), on
    the host"""
    codes, _ = read_shape_codebook(path)
    dev = model_AE.dec2.weight.device
    return codes, embed_shapes(model_AE, codes.float().to(dev), faces, perceptor, render_fn, texture, image_size, chunk).cpu()


def reencode_pose(path, ctx, chunk=256, seed=0):
    """likewise for the pose codebook `path`: embed_poses on its codes -> (codes, embeddings), on the host"""
    codes, _ = read_pose_codebook(path)
    return codes, embed_poses(ctx, codes, chunk, seed).cpu()


# ----------------------------------------------------------------------------------------------------------------- command line
def build_parser():
    ap = argparse.ArgumentParser(prog="python -m avatarclip_amd.codebook", description="build or re-encode the shape and pose CLIP codebooks")
    sub = ap.add_subparsers(dest="command", required=True)

    def common(p):
        p.add_argument("--clip_weights", type=str, default=os.environ.get("AVC_CLIP_WEIGHTS"), help="the CLIP checkpoint whose image tower makes the embeddings")
        p.add_argument("--smpl_uv", type=str, default=None, help="the textured body (data/smpl_uv.obj with its .mtl and image); default: the white body")
        p.add_argument("--image_size", type=int, default=256)
        p.add_argument("--seed", type=int, default=0)
        p.add_argument("--chunk", type=int, default=256, help="bodies rendered and embedded per call")
        p.add_argument("--gpu", type=int, default=0)
        p.add_argument("--out", type=str, required=True, help="the codebook file to write (its sidecar goes to <out>.json)")

    def shape(p):
        p.add_argument("--AE_path_fname", type=str, default="./data/model_VAE_16.pth")
        p.add_argument("--template_obj", type=str, required=True, help="the SMPL template (v_template, faces) as an .obj")

    def pose(p):
        p.add_argument("--smpl", required=True)
        p.add_argument("--vposer", required=True, help="human_body_prior's VPoser model directory")
        p.add_argument("--hip_posing", action="store_true", help="pose the body with smpl_lbs.pose_hip_grad, as animate's flag does")

    def clustering(p):
        p.add_argument("--k", type=int, required=True, help="the number of codes")
        p.add_argument("--iters", type=int, default=100, help="the limit of k-means' iterations")

    p = sub.add_parser("shape-build", help="sample the shape VAE, cluster, embed")
    shape(p); clustering(p); common(p)
    p.add_argument("--n_samples", type=int, required=True, help="latents drawn from N(0, I)")
    p = sub.add_parser("shape-reencode", help="keep a shape codebook's codes, recompute its embeddings")
    shape(p); common(p)
    p.add_argument("--codebook_fname", type=str, required=True)
    p = sub.add_parser("pose-build", help="encode a pose corpus with VPoser, cluster, embed")
    pose(p); clustering(p); common(p)
    p.add_argument("--poses", type=str, required=True, help="the corpus: an .npy of [N, 63] body poses")
    p = sub.add_parser("pose-reencode", help="keep a pose codebook's codes, recompute its embeddings")
    pose(p); common(p)
    p.add_argument("--codebook", type=str, required=True)
    return ap


def _load_vposer(path):
    try:
        from human_body_prior.models.vposer_model import VPoser
        from human_body_prior.tools.model_loader import load_model
    except ImportError as e:
        raise SystemExit("the VPoser body prior comes from the `human_body_prior` package (pose_generation.py:15-16), which is not installed: %s" % e)
    return load_model(path, model_code=VPoser, remove_words_in_model_weights="vp_model.", disable_grad=True)[0]


def run(args, vposer=None):
    """one subcommand on parsed arguments; `vposer`: a VPoser-like object instead of --vposer's directory (pipeline.PipelineSpec.vposer's
    rule).  Returns the sidecar it wrote."""
    from . import clip_vit
    if not args.clip_weights:
        raise SystemExit("the CLIP checkpoint is an input (--clip_weights)")
    dev = torch.device("cuda", int(args.gpu))
    sd = clip_vit.load_state_dict(args.clip_weights)
    perceptor = clip_vit.ClipVision({k: v.float() for k, v in sd.items()}, dev)
    sha = file_sha256(args.clip_weights)
    kind, action = args.command.split("-")
    build = action == "build"
    if kind == "shape":
        from . import shapegen as SG
        from .smpl_prior import read_obj
        v_template, faces = read_obj(args.template_obj)
        model_AE = SG.create_load_AE(v_template.size, 16, v_template, args.AE_path_fname, dev)
        if build:
            codes, emb, info = build_shape_codebook(model_AE, args.k, args.n_samples, args.seed, faces, perceptor, texture=args.smpl_uv,
                                                    image_size=args.image_size, chunk=args.chunk, iters=args.iters)
        else:
            (codes, emb), info = reencode_shape(args.codebook_fname, model_AE, faces, perceptor, texture=args.smpl_uv, image_size=args.image_size,
                                                chunk=args.chunk), None
        side = make_sidecar("shape", codes, perceptor, sha, args.smpl_uv, args.image_size, args.seed if build else None,
                            n_samples=args.n_samples if build else None, info=info)
        write_shape_codebook(args.out, codes, emb, side)
        return side
    from . import animate as A
    from . import smpl_lbs
    vp = vposer if vposer is not None else _load_vposer(args.vposer)
    vp = vp.to(dev).eval() if hasattr(vp, "to") else vp
    ctx = A.AnimateContext(perceptor, None, smpl_lbs.load_smpl_arrays(args.smpl, dev), vp, device=dev, image_size=args.image_size,
                           posing="hip" if args.hip_posing else "torch", texture=args.smpl_uv)
    n_poses = None
    if build:
        poses = np.load(args.poses)
        n_poses = int(poses.shape[0])
        codes, emb, info = build_pose_codebook(ctx, poses, args.k, args.seed, chunk=args.chunk, iters=args.iters)
    else:
        (codes, emb), info = reencode_pose(args.codebook, ctx, chunk=args.chunk, seed=args.seed), None
    side = make_sidecar("pose", codes, perceptor, sha, args.smpl_uv, args.image_size, args.seed, n_poses=n_poses, info=info)
    write_pose_codebook(args.out, codes, emb, side)
    return side


def main(argv=None, vposer=None):
    args = build_parser().parse_args(argv)
    side = run(args, vposer=vposer)
    print("%s: %d codes of %d values, %s embeddings, texture %s -> %s" % (args.command, side["K"], side["D"], side["tower"], side["texture"][:12], args.out))


if __name__ == "__main__":
    main()
