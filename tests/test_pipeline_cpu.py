"""avatarclip_amd/pipeline.py without a device: the stage functions are recording stubs, so what runs here is the pipeline's own part --
stage order, the --from / --until / --force range, the skip rule, how fingerprints propagate (downstream and only downstream), the
manifest after a failed stage, the check before the first stage, and the command line."""
import dataclasses
import json
import os
import subprocess
import sys
import warnings

import pytest

from avatarclip_amd import pipeline as P
from avatarclip_amd.conf import ConfigFactory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = ("clip_weights", "bpe", "smpl", "pose_npy", "template_obj", "AE_path_fname", "codebook_fname", "codebook", "realnvp", "motion_vae")
ANIMATE = "general { mode = motion\n text = a rendered 3d man is arguing }\npose_generator { type = %s }\nmotion_generator { type = %s\n%s }"
ALL = list(P.STAGES)
AFTER_MOTION = ["motion", "drive", "rig", "preview"]


class _VPoser:
    """a VPoser-like object: the pipeline only hands it on"""


def _spec(tmp_path, pose="VPoserCodebook", motion="MotionInterpolation", motion_keys="", **kw):
    a = tmp_path / "assets"
    a.mkdir(exist_ok=True)
    for name in ASSETS:
        if not (a / name).exists():
            (a / name).write_bytes(("content of %s" % name).encode())
    (a / "init.conf").write_text("general { base_exp_dir = ./exp }\ntrain { end_iter = 20 }\nrevision = 2\n")
    fields = dict(out_dir=str(tmp_path / "out"), init_conf=str(a / "init.conf"),
                  appearance_conf=ConfigFactory.parse_string("general { base_exp_dir = ./exp }\nclip { prompt = a 3D rendering of a nurse in unreal engine }\n"
                                                             "train { end_iter = 3\n use_face_prompt = True }"),
                  animate_conf=ConfigFactory.parse_string(ANIMATE % (pose, motion, motion_keys)), vposer=_VPoser(),
                  **{name: str(a / name) for name in ASSETS})
    fields.update(kw)
    return P.PipelineSpec(**fields)


@pytest.fixture
def calls(monkeypatch):
    """every stage replaced by a stub that records its name and writes two small files of its own"""
    made = []

    def stub(name):
        def fn(run):
            assert isinstance(run, P.Run)
            made.append(name)
            out = {}
            for k in ("a", "b"):
                out[k] = os.path.join(run.dir("stub_" + name), k + ".bin")
                with open(out[k], "wb") as fh:
                    fh.write(("%s/%s " % (name, k)).encode() * 10)
            return out
        return fn

    for st in P.STAGES:
        monkeypatch.setattr(P, "stage_" + st, stub(st))
    return made


def _rerun(calls, spec, **changes):
    del calls[:]
    out = P.run(dataclasses.replace(spec, **changes), log=lambda *a: None)
    return list(calls), out


def _manifest(spec):
    with open(os.path.join(spec.out_dir, P.MANIFEST)) as fh:
        return json.load(fh)


def test_stage_order_and_manifest(tmp_path, calls):
    spec = _spec(tmp_path)
    out = P.run(spec, log=lambda *a: None)
    assert calls == ALL == ["shape", "dataset", "init", "appearance", "mesh", "motion", "drive", "rig", "preview"]
    assert out["stages"] == {st: "ran" for st in ALL}
    m = _manifest(spec)
    assert m == out["manifest"] and m["version"] == P.MANIFEST_VERSION and list(m["stages"]) == sorted(ALL)
    fps = P.fingerprints(spec)
    import hashlib
    for st in ALL:
        rec = m["stages"][st]
        assert rec["status"] == "done" and rec["fingerprint"] == fps[st] and len(fps[st]) == 64 and rec["seconds"] >= 0
        assert sorted(rec["outputs"]) == ["a", "b"]
        for o in rec["outputs"].values():
            with open(os.path.join(spec.out_dir, o["path"]), "rb") as fh:
                data = fh.read()
            assert not os.path.isabs(o["path"]) and o["size"] == len(data) and o["sha256"] == hashlib.sha256(data).hexdigest()
    assert len(set(fps.values())) == len(ALL)
    assert not [f for f in os.listdir(spec.out_dir) if ".tmp" in f]              # the temporary file was renamed into place
    assert P.run(dict(dataclasses.asdict(spec), vposer=spec.vposer, appearance_conf=spec.appearance_conf, animate_conf=spec.animate_conf),
                 log=lambda *a: None)["stages"] == {st: "skipped" for st in ALL}   # a dict of the fields is a spec too
    with pytest.raises(ValueError, match="unknown spec field"):
        P.run({"out_dir": str(tmp_path), "prompts": "x"})


def test_from_until_force(tmp_path, calls):
    spec = _spec(tmp_path)
    got, out = _rerun(calls, spec, until_stage="init")
    assert got == ["shape", "dataset", "init"]
    assert [out["stages"][st] for st in ALL] == ["ran"] * 3 + ["not selected"] * 6
    with pytest.raises(ValueError, match="stage drive reads the outputs of stage mesh"):      # upstream of the range: must have finished
        _rerun(calls, spec, from_stage="drive")
    assert calls == []
    assert _rerun(calls, spec, from_stage="appearance", until_stage="motion")[0] == ["appearance", "mesh", "motion"]
    assert _rerun(calls, spec)[0] == ["drive", "rig", "preview"]                              # the rest; what is done is skipped
    assert _rerun(calls, spec, from_stage="motion", until_stage="rig")[0] == []
    got, out = _rerun(calls, spec, from_stage="motion", until_stage="rig", force=True)
    assert got == ["motion", "drive", "rig"]
    assert [out["stages"][st] for st in ALL] == ["not selected"] * 5 + ["ran"] * 3 + ["not selected"]
    assert _rerun(calls, spec)[0] == []                                                       # forcing changed no fingerprint
    for bad in (dict(from_stage="texture"), dict(from_stage="rig", until_stage="mesh")):
        with pytest.raises(ValueError):
            _rerun(calls, spec, **bad)


def test_skip_rule(tmp_path, calls):
    spec = _spec(tmp_path)
    assert _rerun(calls, spec)[0] == ALL
    assert _rerun(calls, spec)[0] == []                                 # same fingerprints, outputs present
    victim = os.path.join(spec.out_dir, "stub_drive", "a.bin")
    os.remove(victim)
    assert _rerun(calls, spec)[0] == ["drive"]                          # an output deleted: that stage alone (no fingerprint moved)
    with open(victim, "r+b") as fh:
        fh.truncate(5)
    assert _rerun(calls, spec)[0] == ["drive"]                          # an output truncated
    size = os.path.getsize(victim)
    with open(victim, "wb") as fh:
        fh.write(b"#" * size)
    assert _rerun(calls, spec)[0] == []                                 # same size, other bytes: outputs are not re-hashed for a skip
    m = _manifest(spec)
    m["stages"]["mesh"]["status"] = "running"                           # what a killed run leaves behind
    P.write_manifest(spec.out_dir, m)
    assert _rerun(calls, spec)[0] == ["mesh"]


@pytest.mark.parametrize("change,expect", [
    (dict(motion_text="a rendered 3d man is dancing"), AFTER_MOTION),
    (dict(preview_size=128), ["preview"]),
    (dict(preview_views=8), ["preview"]),
    (dict(voxel_divisor=64), ["rig", "preview"]),
    (dict(mesh_resolution=128), ["mesh", "drive", "rig", "preview"]),
    (dict(prompt="a 3D rendering of a witch in unreal engine"), ["appearance", "mesh", "drive", "rig", "preview"]),
    (dict(face_prompt="the face of a witch"), ["appearance", "mesh", "drive", "rig", "preview"]),
    (dict(target_txt="a 3d rendering of a tall person in unreal engine"), [st for st in ALL if st != "motion"]),
    (dict(image_size=128), [st for st in ALL if st not in ("shape", "motion")]),
    (dict(posing="hip"), AFTER_MOTION),
])
def test_a_changed_setting_reruns_its_stage_and_what_reads_it(tmp_path, calls, change, expect):
    spec = _spec(tmp_path)
    assert _rerun(calls, spec)[0] == ALL
    assert _rerun(calls, spec, **change)[0] == expect
    assert _rerun(calls, spec, **change)[0] == []
    before, after = P.fingerprints(spec), P.fingerprints(dataclasses.replace(spec, **change))
    assert [st for st in ALL if before[st] != after[st]] == expect


@pytest.mark.parametrize("asset,expect", [
    ("pose_npy", [st for st in ALL if st not in ("shape", "motion")]),            # read by dataset, drive and rig
    ("codebook_fname", [st for st in ALL if st != "motion"]),                     # ShapeGen's codebook
    ("codebook", AFTER_MOTION),                                                   # the pose codebook
    ("motion_vae", AFTER_MOTION),
    ("init.conf", ["init", "appearance", "mesh", "drive", "rig", "preview"]),
    ("realnvp", []),                                                              # no stage of this conf reads it
])
def test_a_changed_asset_byte_reruns_exactly_its_consumers(tmp_path, calls, asset, expect):
    spec = _spec(tmp_path, motion="MotionOptimizer", motion_keys="clip_coef = 0")
    assert _rerun(calls, spec)[0] == ALL
    path = tmp_path / "assets" / asset
    data = bytearray(path.read_bytes())
    data[-2] ^= 1
    path.write_bytes(bytes(data))
    assert _rerun(calls, spec)[0] == expect
    assert _rerun(calls, spec)[0] == []


def test_a_failed_stage_leaves_a_valid_manifest_and_the_next_run_starts_there(tmp_path, calls, monkeypatch):
    spec = _spec(tmp_path)
    good = P.stage_mesh

    def dies(run):
        calls.append("mesh!")
        with open(os.path.join(run.dir("stub_mesh"), "a.bin"), "wb") as fh:
            fh.write(b"half")
        raise RuntimeError("out of memory")

    monkeypatch.setattr(P, "stage_mesh", dies)
    with pytest.raises(RuntimeError, match="out of memory"):
        P.run(spec, log=lambda *a: None)
    assert calls == ["shape", "dataset", "init", "appearance", "mesh!"]
    m = _manifest(spec)                                                  # json.load: the file is whole
    assert [m["stages"][st]["status"] for st in ("shape", "dataset", "init", "appearance", "mesh")] == ["done"] * 4 + ["failed"]
    assert "out of memory" in m["stages"]["mesh"]["error"] and "motion" not in m["stages"]
    monkeypatch.setattr(P, "stage_mesh", good)
    assert _rerun(calls, spec)[0] == ["mesh", "motion", "drive", "rig", "preview"]
    assert all(rec["status"] == "done" for rec in _manifest(spec)["stages"].values())


def test_check_names_every_problem_in_one_error_before_any_stage(tmp_path, calls):
    spec = _spec(tmp_path)
    assert P.check(spec) == []
    gone = ("smpl", "template_obj", "clip_weights", "codebook")
    for name in gone:
        os.remove(getattr(spec, name))
    with pytest.raises(ValueError) as e:
        P.run(dataclasses.replace(spec, init_conf=str(tmp_path / "nowhere.conf"), bpe=None), log=lambda *a: None)
    text = str(e.value)
    for name in gone:
        assert "--%s = %s does not exist" % (name, getattr(spec, name)) in text
    assert "--init_conf = %s does not exist" % (tmp_path / "nowhere.conf") in text and "--bpe is not set" in text
    for name, stage in (("smpl", "dataset"), ("smpl", "motion"), ("smpl", "drive"), ("smpl", "rig"), ("smpl", "preview"), ("template_obj", "shape"),
                        ("clip_weights", "appearance"), ("codebook", "motion")):
        assert "--%s = %s does not exist (stage %s)" % (name, getattr(spec, name), stage) in text
    assert calls == [] and not os.path.exists(spec.out_dir)
    # a stage outside the range asks for nothing
    assert P.check(dataclasses.replace(spec, until_stage="shape", template_obj=spec.bpe, clip_weights=spec.bpe)) == []


def test_check_refuses_what_the_motion_stage_would_die_of(tmp_path, calls):
    base = _spec(tmp_path, motion="MotionOptimizer")                     # clip_coef: animate's default 0.001
    with pytest.raises(ValueError, match="MotionOptimizer with clip_coef = 0.001 needs --renderer_gradient"):
        P.run(base, log=lambda *a: None)
    assert calls == []
    assert P.check(dataclasses.replace(base, renderer_gradient=True)) == []
    assert P.check(_spec(tmp_path, motion="MotionOptimizer", motion_keys="clip_coef = 0")) == []
    # the motion VAE: a missing path is refused, not replaced by a randomly initialised network
    for bad in (None, str(tmp_path / "assets" / "no_such_vae.pth")):
        p = P.check(dataclasses.replace(base, renderer_gradient=True, motion_vae=bad))
        assert len(p) == 1 and "--motion_vae" in p[0] and "(stage motion)" in p[0]
    p = P.check(_spec(tmp_path, pose="VPoserRealNVP", realnvp=None))
    assert len(p) == 1 and "--realnvp is not set" in p[0]
    for pose in ("PoseOptimizer", "VPoserOptimizer"):
        p = P.check(_spec(tmp_path, pose=pose))
        assert len(p) == 1 and pose in p[0] and "--renderer_gradient" in p[0]
        assert P.check(_spec(tmp_path, pose=pose, renderer_gradient=True)) == []
    p = P.check(_spec(tmp_path, pose="PoseSampler", motion="MotionDiffusion"))             # both generator types are looked up
    assert len(p) == 2 and "PoseSampler" in p[0] and "MotionDiffusion" in p[1]
    p = P.check(_spec(tmp_path, vposer=None))
    assert p == ["--vposer is not set (stage motion)"]
    p = P.check(_spec(tmp_path, pose_type="a_pose", posing="numpy"))
    assert len(p) == 2
    with pytest.raises(ValueError, match="2 problem"):
        P.run(_spec(tmp_path, pose="PoseOptimizer", motion="MotionOptimizer"), log=lambda *a: None)
    assert calls == []


def test_command_line_maps_onto_the_spec_field_by_field(tmp_path):
    values, argv = {}, []
    for i, f in enumerate(dataclasses.fields(P.PipelineSpec)):
        if f.name in P.HOOKS:
            continue
        flag = "--" + {"from_stage": "from", "until_stage": "until"}.get(f.name, f.name)
        if f.type is bool:
            values[f.name] = True
            argv.append(flag)
            continue
        if f.name in ("from_stage", "until_stage"):
            values[f.name] = "dataset" if f.name == "from_stage" else "rig"
        elif f.name == "pose_type":
            values[f.name] = "t_pose"
        elif f.type is int:
            values[f.name] = 100 + i
        elif f.type is float:
            values[f.name] = 0.5 + i
        else:
            values[f.name] = "value of %s" % f.name
        argv += [flag, str(values[f.name])]
    spec = P.spec_from_args(argv)
    assert spec == P.PipelineSpec(**values)
    assert spec.text_embeddings is None and spec.text_feature is None              # the hooks have no flag
    flags = {s for a in P.build_parser()._actions for s in a.option_strings}
    for name in ("clip_weights", "bpe", "smpl", "vposer", "codebook", "motion_vae", "pose_npy", "template_obj", "AE_path_fname", "codebook_fname",
                 "retrieval_clip_weights", "renderer_gradient", "from", "until", "force"):
        assert "--" + name in flags
    assert not {"--text_embeddings", "--text_feature", "--views_per_iter", "--shard_view"} & flags
    defaults = P.spec_from_args(["--out_dir", "D"])
    assert defaults == P.PipelineSpec(out_dir="D") and not defaults.force and not defaults.renderer_gradient and defaults.voxel_divisor == 256
    with pytest.raises(SystemExit):
        P.spec_from_args([])                                                        # --out_dir is required
    with pytest.raises(SystemExit, match="problem"):
        P.main(["--out_dir", str(tmp_path / "o")])                                  # nothing else given: the check's list, no traceback


def test_b16_main_tower_without_a_retrieval_checkpoint_warns_once(tmp_path, monkeypatch):
    from avatarclip_amd import clip_vit
    built = []

    class Tower:
        def __init__(self, sd, device):
            self.patch = sd["patch"]
            built.append(self.patch)

    monkeypatch.setattr(clip_vit, "ClipVision", Tower)
    monkeypatch.setattr(clip_vit, "load_state_dict", lambda path: {"patch": 16 if "16" in path else 32})
    monkeypatch.setattr(P, "_B16_WARNED", False)
    run = P.Run(P.PipelineSpec(out_dir=str(tmp_path), clip_weights="ViT-B-16.pt"), {"stages": {}})
    run._device = "cpu"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        main = run.tower()
        assert not w                                                                 # train_clip's use: nothing to say
        assert run.tower(retrieval=True) is main and run.tower(retrieval=True) is main
    assert len(w) == 1 and "ViT-B/32 or ViT-B/16" in str(w[0].message) and "--retrieval_clip_weights" in str(w[0].message)
    assert built == [16]
    both = P.Run(P.PipelineSpec(out_dir=str(tmp_path), clip_weights="ViT-B-16.pt", retrieval_clip_weights="ViT-B-32.pt"), {"stages": {}})
    both._device = "cpu"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert both.tower(retrieval=True).patch == 32 and both.tower().patch == 16 and both.tower(retrieval=True) is both.tower(retrieval=True)
    assert not w and built == [16, 32, 16]


# ---- the three additions to existing modules that the pipeline calls: each keeps the present behaviour as its default
def test_pose_shape_is_the_posing_of_shapegen_render_main(tmp_path):
    import numpy as np
    import torch
    from avatarclip_amd import shapegen_render as SR
    from avatarclip_amd import smpl_lbs
    from tests import drive_standins as S
    a = S.template_arrays()
    faces = np.arange(30, dtype=np.int32).reshape(10, 3)
    np.savez(tmp_path / "smpl.npz", faces=faces, **{k: v.numpy() for k, v in a.items()})
    stand = (np.random.RandomState(0).randn(1, 72) * 0.3).astype(np.float32)
    np.save(tmp_path / "stand_pose.npy", stand)
    shape = a["v_template"].numpy() * 1.1
    tpose = np.zeros((1, 72), np.float32)
    tpose[0, 0] = np.pi / 2
    for pose_type, pose in (("stand_pose", stand), ("t_pose", tpose)):
        v, f = SR.pose_shape(shape, str(tmp_path / "smpl.npz"), pose_type, str(tmp_path / "stand_pose.npy"), device="cpu")
        rot = smpl_lbs.batch_rodrigues(torch.from_numpy(pose.reshape(-1, 3))).reshape(1, 24, 3, 3)
        ref, _ = smpl_lbs.lbs(torch.from_numpy(shape)[None], rot, a["posedirs"], a["J_regressor"], a["parents"], a["lbs_weights"])
        assert v.dtype == np.float32 and np.array_equal(v, ref[0].numpy()) and np.array_equal(f, faces)


def test_animate_run_takes_a_second_context_for_the_pose_generator(tmp_path):
    import numpy as np
    import torch
    from avatarclip_amd import animate as A
    from oracle.animate_standins import StandInVPoser, text_feature_of
    z = np.load(os.path.join(ROOT, "tests", "golden", "animate.npz"))
    assets = dict(codebook=torch.from_numpy(z["cb_codebook"]), codebook_embedding=torch.from_numpy(z["cb_embedding"]))
    conf = lambda d: ConfigFactory.parse_string("general { base_exp_dir = %s\n mode = motion\n text = a rendered 3d man is arguing }\n"
                                                "pose_generator { type = VPoserCodebook }\nmotion_generator { type = MotionInterpolation }" % (tmp_path / d))
    ctx = A.AnimateContext(None, text_feature_of, None, StandInVPoser(0), device="cpu")
    other = A.AnimateContext(None, lambda text: text_feature_of(text, seed=7), None, StandInVPoser(0), device="cpu")
    p_ctx, m_ctx = A.run(conf("a"), ctx, pose_assets=assets)
    p_both, m_both = A.run(conf("b"), ctx, pose_assets=assets, pose_ctx=other)
    p_other, m_other = A.run(conf("c"), other, pose_assets=assets)
    assert torch.equal(p_both, p_other) and not torch.equal(p_both, p_ctx)         # the poses are the second context's
    assert torch.equal(m_both, m_other) and m_both.shape == m_ctx.shape == (60, 69)


def test_init_clip_takes_a_tokenizer_instead_of_building_one():
    import bench
    import torch
    from avatarclip_amd.runner import Runner

    class Tokenizer:
        sot, eot = 1, 2
        asked = []

        def encode(self, text):
            self.asked.append(text)
            return [3 + len(text)]

    class Perceptor:
        _text_sd = {"token_embedding.weight": None}                      # "carries a text tower"

        def encode_text(self, tokens):
            return torch.full((1, 512), float(tokens[0, 1]))

    conf = bench.make_conf(16, 16, small=True)
    conf.put("clip.face_prompt", "the face")
    conf.put("clip.back_prompt", "the back of it")
    r = Runner(None, mode="train_clip", conf=conf, device=torch.device("cpu"))
    tk = Tokenizer()
    r.init_clip(perceptor=Perceptor(), tokenizer=tk)                     # no BPE table anywhere: building one would warn and fall back
    assert tk.asked == [conf.get_string("clip.prompt"), "the face", "the back of it"]
    assert float(r.encoded_face_text[0, 0]) == 3 + len("the face") and float(r.encoded_back_text[0, 0]) == 3 + len("the back of it")


def test_module_imports_neither_bench_nor_tests_nor_oracle():
    code = ("import sys; import avatarclip_amd.pipeline as P; P.build_parser(); "
            "bad = sorted(m for m in sys.modules if m.split('.')[0] in ('bench', 'tests', 'oracle')); print(bad); sys.exit(1 if bad else 0)")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    with open(P.__file__) as fh:
        src = fh.read()
    assert "import bench" not in src and "from oracle" not in src and "from tests" not in src
