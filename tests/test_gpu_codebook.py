"""avatarclip_amd/codebook.py on the device, on the project's seeded stand-ins (the LinearVAE and template of scripts/pipeline_config5.py and
tests/test_gpu_pipeline.py, runner.clip_vit_random_state_dict, oracle.animate_standins.StandInVPoser, tests/drive_standins' SMPL-shaped
arrays), image_size 64, K = 8: the four subcommands write files the existing loaders and stages take, the codes are kmeans' centres, the
embeddings are what the consuming stage would compute one body at a time, a re-encode keeps the codes and reproduces or replaces the
embeddings, and a sidecar silences or raises what pipeline.py says about the tower.

Tolerance between the chunked embeddings and the one-body-at-a-time path: cosine > 0.9999, the one tests/test_gpu_clip.py:509 grants
encode_image between a batch of 12 and batches of 2 of the same images (the renders themselves are per-image launches of one rasteriser)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from tests import drive_standins as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
K, SIZE, SEED = 8, 64, 3
COS = 0.9999                     # tests/test_gpu_clip.py:509


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    from avatarclip_amd import shapegen as SG
    from avatarclip_amd.runner import clip_vit_random_state_dict
    d = str(tmp_path_factory.mktemp("codebook"))
    p = lambda name: os.path.join(d, name)
    z = np.load(os.path.join(GOLDEN, "smpl_views.npz"))
    v_template, faces = z["mesh_v"].astype(np.float32), z["mesh_f"].astype(np.int32)
    SG.writeOBJ(p("template.obj"), v_template, faces)
    torch.manual_seed(0)
    vae = SG.LinearVAE(v_template.size, 16, torch.from_numpy(v_template))
    with torch.no_grad():
        vae.dec2.weight.mul_(0.02)
        vae.dec2.bias.zero_()
    sd = vae.state_dict()
    sd["enc1.weight"] = torch.zeros(1, 1).expand_as(sd["enc1.weight"])          # (never read: stored as one repeated zero)
    torch.save(sd, p("model_VAE_16.pth"))
    torch.save(clip_vit_random_state_dict(0), p("clip.pth"))
    torch.save(clip_vit_random_state_dict(1), p("clip_other.pth"))
    a = S.template_arrays(K=len(v_template))
    np.savez(p("smpl.npz"), v_template=v_template, posedirs=a["posedirs"].numpy(), J_regressor=a["J_regressor"].numpy(), parents=a["parents"].numpy(),
             lbs_weights=a["lbs_weights"].numpy(), faces=faces)
    np.save(p("poses.npy"), (np.random.RandomState(0).randn(200, 63) * 0.3).astype(np.float32))
    return dict(dir=d, p=p, v_template=v_template, faces=faces)


def _shape_args(assets, command, out, clip="clip.pth", extra=()):
    p = assets["p"]
    return [command, "--AE_path_fname", p("model_VAE_16.pth"), "--template_obj", p("template.obj"), "--clip_weights", p(clip), "--image_size", str(SIZE),
            "--out", p(out)] + list(extra)


@pytest.fixture(scope="module")
def shape_book(assets):
    from avatarclip_amd import codebook as CB
    CB.main(_shape_args(assets, "shape-build", "shape.pth", extra=["--k", str(K), "--n_samples", "256", "--seed", str(SEED)]))
    return assets["p"]("shape.pth")


@pytest.fixture(scope="module")
def towers(assets):
    from avatarclip_amd import clip_vit, shapegen as SG
    perceptor = clip_vit.ClipVision(clip_vit.load_state_dict(assets["p"]("clip.pth")), DEV)
    model_AE = SG.create_load_AE(assets["v_template"].size, 16, assets["v_template"], assets["p"]("model_VAE_16.pth"), DEV)
    return perceptor, model_AE


def test_shape_build_writes_kmeans_centres_and_the_embeddings_shape_gen_would_compute(assets, shape_book, towers):
    from avatarclip_amd import clip_score, codebook as CB, kmeans as KM, shapegen as SG
    perceptor, model_AE = towers
    codes, emb = SG.load_codebook(shape_book, DEV)
    assert codes.shape == (K, 16) and emb.shape == (K, 512) and codes.dtype == emb.dtype == torch.float32
    z = torch.randn(256, 16, generator=torch.Generator().manual_seed(SEED)).to(DEV)
    centres, _, info = KM.kmeans(z, K, seed=SEED)
    assert torch.equal(codes, centres)                                         # bit for bit
    with torch.no_grad():
        one = torch.stack([clip_score.render_embedding(perceptor, SG.render_body(model_AE.decode(c[None])[0].cpu().numpy(), assets["faces"], device=DEV,
                                                                                 image_size=SIZE)).mean(0) for c in codes])
    cos = torch.cosine_similarity(emb, one, dim=-1)
    print("shape: min cosine chunked vs one at a time = %.7f" % float(cos.min()))
    assert float(cos.min()) > COS
    assert float(torch.cosine_similarity(emb[0], emb[1], dim=0)) < 1.0          # (the entries are not one embedding repeated)
    side = CB.read_sidecar(shape_book)
    assert side["kind"] == "shape" and (side["K"], side["D"]) == (K, 16) and side["tower"] == "ViT-B/32" and side["texture"] == "white"
    assert side["clip_sha256"] == CB.file_sha256(assets["p"]("clip.pth")) and side["image_size"] == SIZE and side["seed"] == SEED
    assert side["n_samples"] == 256 and side["kmeans_iterations"] == info["iterations"] and side["empty"] == info["empty"]
    assert side["final_inertia"] == info["final_inertia"]
    n_txt = torch.randn(1, 512, generator=torch.Generator().manual_seed(2)).to(DEV)
    zero = clip_score.render_embedding(perceptor, SG.render_body(model_AE.decode(torch.zeros(1, 16, device=DEV))[0].cpu().numpy(), assets["faces"],
                                                                 device=DEV, image_size=SIZE)).mean(0)
    render_fn = lambda v: SG.render_body(v, assets["faces"], device=DEV, image_size=SIZE)
    v, _, best, cosines = SG.shape_gen(model_AE, assets["faces"], perceptor, codes, emb, n_txt, n_txt + (emb[5] - zero)[None], render_fn=render_fn)
    assert best == 5 and v.shape == assets["v_template"].shape and cosines.shape == (K,)      # the stage runs on the file and finds the planted code


def test_a_second_shape_build_gives_the_same_bytes(assets, shape_book):
    from avatarclip_amd import codebook as CB
    CB.main(_shape_args(assets, "shape-build", "shape_again.pth", extra=["--k", str(K), "--n_samples", "256", "--seed", str(SEED), "--chunk", "8"]))
    again = assets["p"]("shape_again.pth")
    assert open(again, "rb").read() == open(shape_book, "rb").read()
    assert CB.read_sidecar(again) == CB.read_sidecar(shape_book)


def test_shape_reencode_keeps_the_codes_and_follows_the_tower(assets, shape_book):
    from avatarclip_amd import codebook as CB
    codes, emb = CB.read_shape_codebook(shape_book)
    CB.main(_shape_args(assets, "shape-reencode", "shape_same.pth", extra=["--codebook_fname", shape_book]))
    c1, e1 = CB.read_shape_codebook(assets["p"]("shape_same.pth"))
    assert torch.equal(c1, codes) and torch.equal(e1, emb)                       # the same tower: the embeddings bit for bit
    CB.main(_shape_args(assets, "shape-reencode", "shape_other.pth", clip="clip_other.pth", extra=["--codebook_fname", shape_book]))
    c2, e2 = CB.read_shape_codebook(assets["p"]("shape_other.pth"))
    assert torch.equal(c2, codes) and c2.numpy().tobytes() == codes.numpy().tobytes()
    assert float(torch.cosine_similarity(e2, emb, dim=-1).max()) < 0.9           # other weights: other embeddings
    side, old = CB.read_sidecar(assets["p"]("shape_other.pth")), CB.read_sidecar(shape_book)
    assert side["clip_sha256"] == CB.file_sha256(assets["p"]("clip_other.pth")) != old["clip_sha256"]
    assert side["n_samples"] is None and side["kmeans_iterations"] is None and side["K"] == K


def test_pose_build_writes_what_vposer_codebook_searches(assets, towers):
    from avatarclip_amd import animate as A, codebook as CB, kmeans as KM, smpl_lbs
    from oracle.animate_standins import StandInVPoser, text_feature_of
    p = assets["p"]
    state = np.random.get_state()
    np.random.seed(77)
    before = np.random.get_state()
    CB.main(["pose-build", "--poses", p("poses.npy"), "--smpl", p("smpl.npz"), "--vposer", "unused", "--clip_weights", p("clip.pth"), "--k", str(K),
             "--seed", str(SEED), "--image_size", str(SIZE), "--out", p("pose.pth")], vposer=StandInVPoser(0))
    after = np.random.get_state()
    np.random.set_state(state)
    assert before[0] == after[0] and (before[1] == after[1]).all() and before[2:] == after[2:]      # the caller's generator is untouched
    ctx = A.AnimateContext(towers[0], text_feature_of, smpl_lbs.load_smpl_arrays(p("smpl.npz"), DEV), StandInVPoser(0).to(DEV), device=DEV, image_size=SIZE)
    gen = A.VPoserCodebook(ctx, codebook_path=p("pose.pth"), pre_topk=K, topk=3)
    assert gen.codebook.shape == (K, 32) and gen.codebook_embedding.shape == (K, 512)
    poses = gen.get_topk_poses("a rendered 3d man is arguing")
    assert 1 <= poses.shape[0] <= 3 and poses.shape[1] == 63 and torch.isfinite(poses).all()
    latents = CB.encode_poses(ctx, np.load(p("poses.npy")))
    centres, _, info = KM.kmeans(latents, K, seed=SEED)
    assert torch.equal(gen.codebook, centres)
    state = np.random.get_state()
    try:
        one = []
        for c in gen.codebook:
            np.random.seed(SEED)
            with torch.no_grad():
                one.append(ctx.get_pose_feature(ctx.vp.decode(c[None])["pose_body"].reshape(1, -1))[0])
    finally:
        np.random.set_state(state)
    cos = torch.cosine_similarity(gen.codebook_embedding, torch.stack(one), dim=-1)
    print("pose: min cosine chunked vs one at a time = %.7f" % float(cos.min()))
    assert float(cos.min()) > COS
    side = CB.read_sidecar(p("pose.pth"))
    assert side["kind"] == "pose" and side["D"] == 32 and side["n_poses"] == 200 and side["n_samples"] is None and side["seed"] == SEED
    assert side["kmeans_iterations"] == info["iterations"]
    CB.main(["pose-reencode", "--codebook", p("pose.pth"), "--smpl", p("smpl.npz"), "--vposer", "unused", "--clip_weights", p("clip.pth"),
             "--seed", str(SEED), "--image_size", str(SIZE), "--chunk", "3", "--out", p("pose_same.pth")], vposer=StandInVPoser(0))
    c1, e1 = CB.read_pose_codebook(p("pose_same.pth"))
    assert torch.equal(c1, gen.codebook.cpu())
    assert float(torch.cosine_similarity(e1, gen.codebook_embedding.cpu(), dim=-1).min()) > COS       # chunks of 3: the same cameras for every entry


def test_the_sidecar_decides_what_the_pipeline_says_about_a_b16_tower(assets, shape_book, monkeypatch):
    from avatarclip_amd import codebook as CB, pipeline as P
    from avatarclip_amd.runner import clip_vit_random_state_dict
    p = assets["p"]
    torch.save(clip_vit_random_state_dict(0, patch=16), p("clip16.pth"))
    codes, emb = CB.read_shape_codebook(shape_book)
    CB.write_shape_codebook(p("shape16.pth"), codes, emb, dict(CB.read_sidecar(shape_book), tower="ViT-B/16"))
    monkeypatch.setattr(P, "_B16_WARNED", False)
    run = P.Run(P.PipelineSpec(out_dir=p("out"), clip_weights=p("clip16.pth")), {"stages": {}})
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        t = run.tower(retrieval=True, codebook=p("shape16.pth"))
        assert t.patch == 16 and not [x for x in w if "ViT-B/32 or ViT-B/16" in str(x.message)]
        run.tower(retrieval=True, codebook=shape_book)                           # its sidecar names ViT-B/32
        assert len([x for x in w if "ViT-B/32 or ViT-B/16" in str(x.message)]) == 1
    spec = P.PipelineSpec(out_dir=p("out"), until_stage="shape", clip_weights=p("clip16.pth"), codebook_fname=shape_book, template_obj=p("template.obj"),
                          AE_path_fname=p("model_VAE_16.pth"), text_embeddings={"neutral_txt": torch.zeros(1, 512), "target_txt": torch.ones(1, 512)})
    problems = P.check(spec)
    assert len(problems) == 1 and "ViT-B/32 embeddings" in problems[0] and "ViT-B/16 tower" in problems[0] and "(stage shape)" in problems[0]
    assert P.check(P.PipelineSpec(**dict(vars(spec), codebook_fname=p("shape16.pth")))) == []
