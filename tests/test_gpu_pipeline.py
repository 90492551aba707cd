"""avatarclip_amd/pipeline.py on the device: the whole chain, prompt -> shape -> 108 views -> NeuS init -> CLIP-guided appearance -> mesh ->
motion -> .pc2 -> .glb -> previews, once, at the smallest sizes at which every hand-off is still the real file, on the project's seeded
stand-ins written out as files (the LinearVAE / codebook construction of scripts/pipeline_config5.py, runner.clip_vit_random_state_dict,
oracle.animate_standins, tests/drive_standins' SMPL-shaped arrays at the template's vertex count).  One module-scoped fixture runs it; the
tests share its directory: the chain completes, the pipeline adds nothing to what its stages write, one tower is built, and a second and
third run re-run what they must and nothing else."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from tests import drive_standins as S

gpu = pytest.mark.gpu
pytestmark = gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda"
N_CODES, PLANTED = 8, 3
MOTION_TEXT = "a rendered 3d man is arguing"
ANIMATE = "general { mode = motion\n text = unset }\npose_generator { type = VPoserCodebook }\nmotion_generator { type = MotionInterpolation }"
AFTER_MOTION = ["motion", "drive", "rig", "preview"]


def _confs():
    import bench
    init = bench.make_conf(64, 32, small=True)                  # 20 steps of 256 rays on the 64 x 64 views
    for k, v in (("train.batch_size", 256), ("train.warm_up_end", 0), ("train.end_iter", 20), ("train.save_freq", 20)):
        init.put(k, v)
    clip = bench.make_conf(32, 32, small=True)                  # 3 steps at 32 x 32 x 32 samples
    for k, v in (("train.warm_up_end", 0), ("train.end_iter", 3), ("train.save_freq", 3)):
        clip.put(k, v)
    return init, clip


def _write_assets(d):
    """every asset as a file under d; returns (spec fields, what the by-hand comparisons need)"""
    from avatarclip_amd import clip_score, clip_vit, shapegen as SG
    from avatarclip_amd.conf import ConfigFactory
    from avatarclip_amd.runner import clip_vit_random_state_dict
    from oracle.animate_standins import StandInVPoser, text_feature_of
    p = lambda name: os.path.join(d, name)
    z = np.load(os.path.join(GOLDEN, "smpl_views.npz"))
    v_template, faces = z["mesh_v"].astype(np.float32), z["mesh_f"].astype(np.int32)
    SG.writeOBJ(p("template.obj"), v_template, faces)
    # ShapeGen's blobs, as scripts/pipeline_config5.py makes them (the encoder half is never read: stored as one repeated zero)
    torch.manual_seed(0)
    vae = SG.LinearVAE(v_template.size, 16, torch.from_numpy(v_template))
    with torch.no_grad():
        vae.dec2.weight.mul_(0.02)
        vae.dec2.bias.zero_()
    sd = vae.state_dict()
    sd["enc1.weight"] = torch.zeros(1, 1).expand_as(sd["enc1.weight"])
    torch.save(sd, p("model_VAE_16.pth"))
    del vae, sd
    torch.save(clip_vit_random_state_dict(0), p("clip.pth"))
    model_AE = SG.create_load_AE(v_template.size, 16, v_template, p("model_VAE_16.pth"), DEV)
    perceptor = clip_vit.ClipVision(clip_vit.load_state_dict(p("clip.pth")), DEV)
    codes = torch.randn(N_CODES, 16, generator=torch.Generator().manual_seed(1)).to(DEV)
    embed = lambda c: clip_score.render_embedding(perceptor, SG.render_body(model_AE.decode(c)[0].cpu().numpy(), faces, device=DEV)).mean(0)
    with torch.no_grad():
        emb = torch.stack([embed(c[None]) for c in codes])
        zero_emb = embed(torch.zeros(1, 16, device=DEV))
    torch.save({codes.cpu(): emb.cpu()}, p("shape_codebook.pth"))
    n_txt = torch.randn(1, 512, generator=torch.Generator().manual_seed(2))
    unit = lambda seed: torch.nn.functional.normalize(torch.randn(1, 512, generator=torch.Generator().manual_seed(seed)), dim=1)
    text_embeddings = {"neutral_txt": n_txt, "target_txt": n_txt + (emb[PLANTED] - zero_emb).cpu()[None],       # points at the planted code
                       "prompt": unit(11), "face_prompt": unit(12), "back_prompt": unit(13)}
    # SMPL-shaped arrays on the template's own vertices and faces, the stand pose, AvatarAnimate's pose codebook
    a = S.template_arrays(K=len(v_template))
    np.savez(p("smpl.npz"), v_template=v_template, posedirs=a["posedirs"].numpy(), J_regressor=a["J_regressor"].numpy(), parents=a["parents"].numpy(),
             lbs_weights=a["lbs_weights"].numpy(), faces=faces)
    np.save(p("stand_pose.npy"), np.load(os.path.join(GOLDEN, "rig.npz"))["stand_pose"])
    g = np.load(os.path.join(GOLDEN, "animate.npz"))
    torch.save({"codebook": torch.from_numpy(g["cb_codebook"]), "codebook_embedding": torch.from_numpy(g["cb_embedding"])}, p("pose_codebook.pth"))
    init, clip = _confs()
    fields = dict(init_conf=init, appearance_conf=clip, animate_conf=ConfigFactory.parse_string(ANIMATE), motion_text=MOTION_TEXT,
                  clip_weights=p("clip.pth"), smpl=p("smpl.npz"), pose_npy=p("stand_pose.npy"), template_obj=p("template.obj"),
                  AE_path_fname=p("model_VAE_16.pth"), codebook_fname=p("shape_codebook.pth"), vposer=StandInVPoser(0), codebook=p("pose_codebook.pth"),
                  image_size=64, mesh_resolution=40, voxel_divisor=16, preview_size=64, preview_views=4,
                  text_embeddings=text_embeddings, text_feature=text_feature_of)
    return fields, dict(model_AE=model_AE, perceptor=perceptor, faces=faces, n_vertices=len(v_template))


def _mtimes(root):
    return {os.path.join(d, f): os.stat(os.path.join(d, f)).st_mtime_ns for d, _, fs in os.walk(root) for f in fs if f != "pipeline.json"}


@pytest.fixture(scope="module")
def chain(tmp_path_factory):
    """the run itself, then a second and a third run on the same directory; ClipVision.__init__ and Runner.train_clip are wrapped to count
    the towers and to see the weights the appearance stage starts from"""
    from avatarclip_amd import clip_vit, pipeline as P
    from avatarclip_amd.runner import Runner
    d = str(tmp_path_factory.mktemp("pipeline"))
    os.makedirs(os.path.join(d, "assets"))
    fields, hand = _write_assets(os.path.join(d, "assets"))
    spec = P.PipelineSpec(out_dir=os.path.join(d, "out"), **fields)
    towers, started_from = [], []
    init0, train_clip0 = clip_vit.ClipVision.__init__, Runner.train_clip

    def counted_init(self, *a, **kw):
        towers.append(1)
        return init0(self, *a, **kw)

    def seen_train_clip(self):
        started_from.append(self.sdf_network.lin0.weight_v.detach().clone())
        return train_clip0(self)

    quiet = lambda *a: None
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(clip_vit.ClipVision, "__init__", counted_init)
        mp.setattr(Runner, "train_clip", seen_train_clip)
        first = P.run(spec, log=quiet)
        n_first = len(towers)
        for st in P.STAGES:
            print("%-10s %7.2f s" % (st, first["manifest"]["stages"][st]["seconds"]))
        before = _mtimes(spec.out_dir)
        second = P.run(spec, log=quiet)
        after_second = _mtimes(spec.out_dir)
        third = P.run(dataclasses.replace(spec, motion_text="a rendered 3d man is dancing"), log=quiet)
        after_third = _mtimes(spec.out_dir)
        n_resumed = len(towers) - n_first
        # a second checkpoint for the retrieval: its own directory, as far as the stage that needs the main tower
        del towers[:]
        P.run(dataclasses.replace(spec, out_dir=os.path.join(d, "out_retrieval"), retrieval_clip_weights=spec.clip_weights, until_stage="appearance"),
              log=quiet)
        n_retrieval = len(towers)
    return dict(spec=spec, hand=hand, first=first, second=second, third=third, before=before, after_second=after_second, after_third=after_third,
                n_first=n_first, n_resumed=n_resumed, n_retrieval=n_retrieval, started_from=started_from, root=d)


def _gif(path):
    from PIL import Image
    with Image.open(path) as im:
        return im.n_frames, im.size


def test_the_chain_completes_and_every_hand_off_is_the_real_file(chain):
    from avatarclip_amd import drive, mesh, pipeline as P, rig
    from avatarclip_amd.smpl_prior import read_obj
    out = chain["spec"].out_dir
    m = chain["first"]["manifest"]["stages"]
    assert chain["first"]["stages"] == {st: "ran" for st in P.STAGES} and all(m[st]["status"] == "done" for st in P.STAGES)
    path = lambda st, key: os.path.join(out, m[st]["outputs"][key]["path"])
    # shape: the template's vertex count, the planted code
    v, f = read_obj(os.path.join(out, "shape", "coarse_shape.obj"))
    assert v.shape == (chain["hand"]["n_vertices"], 3) and np.array_equal(f, chain["hand"]["faces"])
    import json
    with open(os.path.join(out, "shape", "shape.json")) as fh:
        doc = json.load(fh)
    assert doc["code"] == PLANTED and len(doc["cosines"]) == N_CODES and doc["cosine"] == max(doc["cosines"])
    # dataset: 108 views of 64 x 64, the posed mesh
    from PIL import Image
    pngs = sorted(os.listdir(os.path.join(out, "render", "img")))
    assert pngs == ["%04d.png" % i for i in range(108)] and Image.open(os.path.join(out, "render", "img", "0000.png")).size == (64, 64)
    with open(os.path.join(out, "render", "transforms_train.json")) as fh:
        assert len(json.load(fh)["frames"]) == 108
    pv, pf = read_obj(os.path.join(out, "shape", "posed.obj"))
    assert pv.shape == v.shape and np.array_equal(pf, f) and np.isfinite(pv).all() and not np.allclose(pv, v)
    # init -> appearance: train_clip started from the init checkpoint
    init_ckpt = path("init", "checkpoint")
    assert os.path.basename(init_ckpt) == "ckpt_000020.pth" and os.path.basename(path("appearance", "checkpoint")) == "ckpt_000003.pth"
    saved = torch.load(init_ckpt, map_location=DEV, weights_only=True)["sdf_network_fine"]["lin0.weight_v"]
    assert len(chain["started_from"]) == 2 and torch.equal(chain["started_from"][0], saved)
    # mesh, motion
    ply = path("mesh", "ply")
    assert os.path.dirname(ply) == os.path.join(out, "exp_clip", "meshes")
    mv, mt, mc = mesh.read_ply(ply)
    assert len(mv) > 0 and len(mt) > 0 and mc is not None
    motion = np.load(os.path.join(out, "anim", "motion.npy"))
    assert motion.shape == (60, 69) and np.isfinite(motion).all()
    assert sorted(os.listdir(os.path.join(out, "anim"))) == ["candidate_%d.npy" % i for i in range(5)] + ["motion.npy"]
    # drive, rig
    cv, _, _ = mesh.read_ply(os.path.join(out, "drive", "avatar_cleaned_apose.ply"))
    head, frames = drive.read_pc2(os.path.join(out, "drive", "motion.pc2"))
    assert 0 < len(cv) <= len(mv) and head[1:] == (1, len(cv), 0.0, 60.0, 60) and frames.shape == (60, len(cv), 3) and np.isfinite(frames).all()
    r = rig.read_glb(os.path.join(out, "rig", "avatar.glb"))
    assert len(r["animation"]) == 24 and all(len(ch["times"]) == 60 for ch in r["animation"])
    assert np.load(os.path.join(out, "rig", "avatar_rig.npz"))["blend_weights"].shape == (24, len(r["attributes"]["POSITION"]))
    # previews: the turn-table has the views, the played ones the motion's frames
    assert sorted(os.listdir(os.path.join(out, "preview"))) == ["drive.gif", "mesh.gif", "motion.gif", "rig.gif"]
    assert _gif(os.path.join(out, "preview", "mesh.gif")) == (4, (64, 64))
    for name in ("drive", "rig", "motion"):
        assert _gif(os.path.join(out, "preview", name + ".gif")) == (60, (64, 64))


def test_the_pipeline_adds_nothing_to_what_its_stages_write(chain, tmp_path):
    from avatarclip_amd import drive, rig, shapegen as SG
    spec, hand, out = chain["spec"], chain["hand"], chain["spec"].out_dir
    same = lambda a, b: open(a, "rb").read() == open(b, "rb").read()
    ply = os.path.join(out, chain["first"]["manifest"]["stages"]["mesh"]["outputs"]["ply"]["path"])
    # (anim/motion.npy is the third run's by now; drive/ and rig/ were written from it)
    motion = os.path.join(out, "anim", "motion.npy")
    _, pc2 = drive.generate_animation(ply, motion, spec.smpl, spec.pose_npy, str(tmp_path / "drive"), name="avatar")
    glb, npz = rig.build_rig(ply, spec.smpl, spec.pose_npy, str(tmp_path / "rig"), name="avatar", motion=motion, voxel_divisor=16)
    assert same(pc2, os.path.join(out, "drive", "motion.pc2")) and same(glb, os.path.join(out, "rig", "avatar.glb"))
    assert same(str(tmp_path / "drive" / "avatar_cleaned_apose.ply"), os.path.join(out, "drive", "avatar_cleaned_apose.ply"))
    codebook, clip_codebook = SG.load_codebook(spec.codebook_fname, DEV)
    te = spec.text_embeddings
    v, _, best, _ = SG.shape_gen(hand["model_AE"], hand["faces"], hand["perceptor"], codebook, clip_codebook, te["neutral_txt"].to(DEV), te["target_txt"].to(DEV))
    SG.writeOBJ(str(tmp_path / "by_hand.obj"), v, hand["faces"])
    assert best == PLANTED and same(str(tmp_path / "by_hand.obj"), os.path.join(out, "shape", "coarse_shape.obj"))


def test_one_tower_is_built_in_the_whole_run(chain):
    assert chain["n_first"] == 1                 # shape, appearance (and motion, had it needed one) share it
    assert chain["n_resumed"] == 0               # nothing the second and third run re-ran needs a tower
    assert chain["n_retrieval"] == 2             # --retrieval_clip_weights: one more, for the codebook search


def test_a_second_run_runs_nothing_and_a_new_motion_text_reruns_its_consumers(chain):
    from avatarclip_amd import pipeline as P
    assert chain["second"]["stages"] == {st: "skipped" for st in P.STAGES}
    assert chain["after_second"] == chain["before"]                                   # no output's mtime moved
    assert chain["third"]["stages"] == {st: ("ran" if st in AFTER_MOTION else "skipped") for st in P.STAGES}
    moved = {os.path.relpath(p, chain["spec"].out_dir).split(os.sep)[0] for p, t in chain["after_third"].items() if chain["before"].get(p) != t}
    assert moved == {"anim", "drive", "rig", "preview"}
    ckpts = os.path.join(chain["spec"].out_dir, "exp_clip", "checkpoints")
    assert {p: t for p, t in chain["after_third"].items() if p.startswith(ckpts)} == {p: t for p, t in chain["before"].items() if p.startswith(ckpts)} != {}
    a, b, c = (chain[k]["manifest"]["stages"] for k in ("first", "second", "third"))
    assert all(a[st]["fingerprint"] == c[st]["fingerprint"] for st in P.STAGES if st not in AFTER_MOTION)
    assert all(a[st]["fingerprint"] != c[st]["fingerprint"] for st in AFTER_MOTION)
