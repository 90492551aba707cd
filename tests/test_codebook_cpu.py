"""avatarclip_amd/codebook.py without a GPU: the two file layouts through the loaders that exist, the sidecar, check_provenance, the command
line, and what pipeline.py makes of a sidecar (the ViT-B/16 warning and the pre-flight line)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from avatarclip_amd import codebook as CB
from avatarclip_amd import pipeline as P


def _tensors(k=6, d=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(k, d, generator=g), torch.randn(k, 512, generator=g)


def test_the_shape_file_is_one_entry_keyed_by_the_codes_and_loads_as_before(tmp_path):
    from avatarclip_amd import shapegen as SG
    codes, emb = _tensors()
    path = str(tmp_path / "shape.pth")
    CB.write_shape_codebook(path, codes, emb)
    raw = torch.load(path, map_location="cpu", weights_only=True)              # tensors only
    assert len(raw) == 1 and list(raw.keys())[-1].shape == (6, 16)              # ShapeGen/main.py:86-91 returns the last key
    c, e = SG.load_codebook(path, "cpu")
    assert torch.equal(c, codes) and torch.equal(e, emb) and c.dtype == e.dtype == torch.float32
    assert sorted(os.listdir(tmp_path)) == ["shape.pth"]                        # no temporary file stays, no sidecar unless asked for
    assert CB.read_sidecar(path) is None and CB.check_provenance(path, "ViT-B/16", None) == []
    first = open(path, "rb").read()
    CB.write_shape_codebook(path, codes, emb)
    assert open(path, "rb").read() == first                                     # the same tensors: the same bytes
    with pytest.raises(ValueError, match="codes \\[K, D\\] and embeddings \\[K, 512\\]"):
        CB.write_shape_codebook(path, codes, emb[:3])
    assert open(path, "rb").read() == first                                     # a refused write leaves the file alone


def test_the_pose_file_loads_in_vposer_codebook(tmp_path):
    from avatarclip_amd import animate as A
    from oracle.animate_standins import StandInVPoser
    codes, emb = _tensors(9, 32, 1)
    path = str(tmp_path / "pose.pth")
    CB.write_pose_codebook(path, codes, emb)
    raw = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(raw) == ["codebook", "codebook_embedding"]
    ctx = type("Ctx", (), {"device": torch.device("cpu"), "vp": StandInVPoser(0)})()
    gen = A.VPoserCodebook(ctx, codebook_path=path, pre_topk=4, topk=2)
    assert torch.equal(gen.codebook, codes) and torch.equal(gen.codebook_embedding, emb)
    assert torch.equal(CB.read_pose_codebook(path)[0], codes)


def test_the_sidecar_round_trips_and_check_provenance_reports(tmp_path):
    codes, emb = _tensors()
    path = str(tmp_path / "shape.pth")
    info = {"iterations": 7, "final_inertia": 12.5, "empty": [3]}
    side = CB.make_sidecar("shape", codes, (16, 197), "ab" * 32, None, 64, seed=4, n_samples=256, info=info)
    assert set(side) == set(CB.SIDECAR_KEYS)
    assert side == {"version": 1, "kind": "shape", "K": 6, "D": 16, "tower": "ViT-B/16", "clip_sha256": "ab" * 32, "texture": "white", "image_size": 64,
                    "seed": 4, "n_samples": 256, "n_poses": None, "kmeans_iterations": 7, "final_inertia": 12.5, "empty": [3]}
    CB.write_shape_codebook(path, codes, emb, side)
    assert sorted(os.listdir(tmp_path)) == ["shape.pth", "shape.pth.json"] and CB.sidecar_path(path) == path + ".json"
    assert CB.read_sidecar(path) == side and json.load(open(path + ".json")) == side
    assert CB.check_provenance(path, "ViT-B/16", None) == [] == CB.check_provenance(path, 16, None)
    tower = type("T", (), {"patch": 32})()
    other = CB.check_provenance(path, tower, None)
    assert len(other) == 1 and "ViT-B/16 embeddings" in other[0] and "ViT-B/32 tower" in other[0] and "shape-reencode" in other[0]
    cubes = torch.rand(4, 2, 2, 2, 3)
    both = CB.check_provenance(path, (32, 50), cubes)
    assert len(both) == 2 and "the white body" in both[1] and CB.texture_digest(cubes)[:12] in both[1]
    textured = CB.make_sidecar("pose", _tensors(6, 32)[0], 32, "cd" * 32, cubes, 256, seed=0, n_poses=200, info=info)
    assert textured["texture"] == CB.texture_digest(cubes.numpy()) != "white" and textured["n_samples"] is None and textured["n_poses"] == 200
    CB.write_pose_codebook(str(tmp_path / "pose.pth"), *_tensors(6, 32), sidecar=textured)
    assert CB.check_provenance(str(tmp_path / "pose.pth"), 32, cubes) == []
    white = CB.check_provenance(str(tmp_path / "pose.pth"), 32, None)
    assert len(white) == 1 and "renders the white body" in white[0] and "pose-reencode" in white[0]
    with pytest.raises(ValueError, match="shape or pose"):
        CB.make_sidecar("motion", codes, 32, "", None, 64)


def test_the_texture_digest_is_the_pipeline_s_fingerprint(tmp_path):
    from tests.test_texture_cpu import _fixture
    path = _fixture(tmp_path)
    assert CB.texture_digest(path) == P.texture_fingerprint(path)["smpl_uv"]
    assert CB.texture_digest(None) == "white"


def test_command_line():
    ap = CB.build_parser()
    a = ap.parse_args(["shape-build", "--AE_path_fname", "vae.pth", "--template_obj", "t.obj", "--clip_weights", "c.pt", "--k", "8", "--n_samples", "256",
                       "--seed", "3", "--chunk", "4", "--out", "o.pth", "--smpl_uv", "uv.obj", "--image_size", "64"])
    assert (a.command, a.AE_path_fname, a.template_obj, a.clip_weights, a.k, a.n_samples, a.seed, a.chunk, a.out, a.smpl_uv, a.image_size) == \
        ("shape-build", "vae.pth", "t.obj", "c.pt", 8, 256, 3, 4, "o.pth", "uv.obj", 64)
    a = ap.parse_args(["shape-reencode", "--codebook_fname", "cb.pth", "--template_obj", "t.obj", "--clip_weights", "c.pt", "--out", "o.pth"])
    assert a.command == "shape-reencode" and a.codebook_fname == "cb.pth" and a.seed == 0 and a.chunk == 256 and not hasattr(a, "k")
    a = ap.parse_args(["pose-build", "--poses", "p.npy", "--smpl", "s.pkl", "--vposer", "vp", "--clip_weights", "c.pt", "--k", "4096", "--out", "o.pth",
                       "--hip_posing"])
    assert (a.command, a.poses, a.smpl, a.vposer, a.k, a.hip_posing, a.smpl_uv) == ("pose-build", "p.npy", "s.pkl", "vp", 4096, True, None)
    a = ap.parse_args(["pose-reencode", "--codebook", "cb.pth", "--smpl", "s.pkl", "--vposer", "vp", "--clip_weights", "c.pt", "--out", "o.pth"])
    assert a.command == "pose-reencode" and a.codebook == "cb.pth" and not a.hip_posing
    for argv in ([], ["shape-build", "--out", "o"], ["pose-build", "--k", "3", "--out", "o"], ["cluster"]):
        with pytest.raises(SystemExit):
            ap.parse_args(argv)
    with pytest.raises(ValueError, match=r"\[N, 63\]"):
        CB.encode_poses(None, np.zeros((4, 60), np.float32))


def _towers(monkeypatch):
    from avatarclip_amd import clip_vit

    class Tower:
        def __init__(self, sd, device):
            self.patch = sd["patch"]

    monkeypatch.setattr(clip_vit, "ClipVision", Tower)
    monkeypatch.setattr(clip_vit, "load_state_dict", lambda path: {"patch": 16 if "16" in path else 32})
    monkeypatch.setattr(clip_vit, "vision_variant", lambda sd: (sd["patch"], 197 if sd["patch"] == 16 else 50))
    monkeypatch.setattr(P, "_B16_WARNED", False)


def test_a_sidecar_that_names_the_main_tower_silences_the_b16_warning(tmp_path, monkeypatch):
    _towers(monkeypatch)
    codes, emb = _tensors()
    mine, shipped, other = (str(tmp_path / n) for n in ("mine.pth", "shipped.pth", "other.pth"))
    CB.write_shape_codebook(mine, codes, emb, CB.make_sidecar("shape", codes, 16, "", None, 256))
    CB.write_shape_codebook(shipped, codes, emb)
    CB.write_shape_codebook(other, codes, emb, CB.make_sidecar("shape", codes, 32, "", None, 256))
    run = P.Run(P.PipelineSpec(out_dir=str(tmp_path), clip_weights="ViT-B-16.pt"), {"stages": {}})
    run._device = "cpu"
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        run.tower(retrieval=True, codebook=mine)
        assert not w                                                            # re-encoded for this tower: nothing to say
        run.tower(retrieval=True, codebook=other)
        assert len(w) == 1 and "ViT-B/32 or ViT-B/16" in str(w[0].message)      # a sidecar naming the other variant does not silence it
    monkeypatch.setattr(P, "_B16_WARNED", False)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        run.tower(retrieval=True, codebook=shipped)
        run.tower(retrieval=True)
    assert len(w) == 1                                                          # no sidecar: exactly as before, once


def test_a_sidecar_of_another_variant_or_texture_is_one_preflight_line_each(tmp_path, monkeypatch):
    _towers(monkeypatch)
    codes, emb = _tensors()
    book = str(tmp_path / "shape.pth")
    for name in ("ViT-B-16.pt", "ViT-B-32.pt"):
        (tmp_path / name).write_bytes(b"")
    spec = lambda **kw: P.PipelineSpec(out_dir=str(tmp_path / "o"), until_stage="shape", codebook_fname=book, **kw)
    lines = lambda s: [p for p in P.check(s) if "codebook" in p and "does not exist" not in p and "is not set" not in p]
    CB.write_shape_codebook(book, codes, emb)
    assert lines(spec(clip_weights=str(tmp_path / "ViT-B-16.pt"))) == []        # no sidecar: nothing is read, nothing is said
    CB.write_sidecar(book, CB.make_sidecar("shape", codes, 32, "", None, 256))
    got = lines(spec(clip_weights=str(tmp_path / "ViT-B-16.pt")))
    assert len(got) == 1 and "ViT-B/32 embeddings" in got[0] and "ViT-B/16 tower" in got[0] and got[0].endswith("(stage shape)")
    assert lines(spec(clip_weights=str(tmp_path / "ViT-B-32.pt"))) == []
    assert lines(spec(clip_weights=str(tmp_path / "ViT-B-16.pt"), retrieval_clip_weights=str(tmp_path / "ViT-B-32.pt"))) == []
    CB.write_sidecar(book, CB.make_sidecar("shape", codes, 32, "", torch.rand(4, 2, 2, 2, 3), 256))
    got = lines(spec(clip_weights=str(tmp_path / "ViT-B-32.pt")))
    assert len(got) == 1 and "renders the white body" in got[0]
    with pytest.raises(ValueError, match="renders the white body"):             # the line is part of the collected error of a run
        P.run(spec(clip_weights=str(tmp_path / "ViT-B-32.pt")), log=lambda *a: None)
