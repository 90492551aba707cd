"""CLIP ViT-B/16 on the host side, without a GPU: the variant is read from the checkpoint (clip_vit.vision_variant), the seeded
stand-in weights exist for both towers (runner.clip_vit_random_state_dict), and the CPU oracle under PATCH = 16 / TOKENS = 197 -- the
reference of the GPU tests in test_gpu_clip_b16.py -- is itself pinned against transformers' CLIP vision tower at patch 16."""
import hashlib

import pytest
import torch

from oracle import clip_vit_oracle as C


def _b16(monkeypatch):
    monkeypatch.setattr(C, "PATCH", 16)
    monkeypatch.setattr(C, "TOKENS", 197)


def test_vision_variant_reads_the_two_supported_towers():
    from avatarclip_amd import clip_vit as V
    from avatarclip_amd.runner import clip_vit_random_state_dict
    assert V.vision_variant(clip_vit_random_state_dict(0)) == (32, 50)
    assert V.vision_variant(clip_vit_random_state_dict(0, patch=16)) == (16, 197)
    assert V.ClipVision is V.ClipVisionB32
    # the module constants keep their ViT-B/32 values
    assert (V.PATCH, V.TOKENS, V.WIDTH, V.HEADS, V.LAYERS, V.RES, V.EMBED) == (32, 50, 768, 12, 12, 224, 512)


def _vit_l14_like():
    # the shapes vision_variant looks at, of ViT-L/14: width 1024, patch 14, 257 tokens, 24 layers (no other tensor is read)
    sd = {"visual.conv1.weight": torch.zeros(1024, 3, 14, 14), "visual.positional_embedding": torch.zeros(257, 1024)}
    for i in range(24):
        sd["visual.transformer.resblocks.%d.ln_1.weight" % i] = torch.zeros(1024)
    return sd


def _patch16_with_50_rows():
    from avatarclip_amd.runner import clip_vit_random_state_dict
    sd = dict(clip_vit_random_state_dict(0, patch=16))
    sd["visual.positional_embedding"] = sd["visual.positional_embedding"][:50].clone()
    return sd


def _no_visual_keys():
    # (what is left of a checkpoint without an image tower: the text tower's keys only)
    return {"token_embedding.weight": torch.zeros(8, 512), "positional_embedding": torch.zeros(77, 512)}


@pytest.mark.parametrize("make, found", [(_vit_l14_like, "width 1024"), (_patch16_with_50_rows, "patch 16, 50 tokens"),
                                         (_no_visual_keys, "no ViT image tower")])
def test_vision_variant_refuses_everything_else_and_names_both_variants(make, found):
    from avatarclip_amd import clip_vit as V
    with pytest.raises(ValueError) as e:
        V.vision_variant(make())
    msg = str(e.value)
    assert "ViT-B/32" in msg and "ViT-B/16" in msg and "50 tokens" in msg and "197 tokens" in msg, msg
    assert found in msg, msg
    # the class refuses with the same error, on the CPU, before a device or the library is touched
    with pytest.raises(ValueError):
        V.ClipVision(make(), "cuda")


def _digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(str(tuple(sd[k].shape)).encode())
        h.update(sd[k].contiguous().numpy().tobytes())
    return h.hexdigest()


def test_seeded_stand_in_weights_default_draw_is_unchanged_and_patch_16_has_the_b16_shapes():
    from avatarclip_amd.runner import clip_vit_random_state_dict
    sd = clip_vit_random_state_dict(0)
    # sha256 over (key, shape, bytes) in key order / of single tensors, computed with the function as it was before the `patch` keyword
    assert _digest(sd) == "80beacddd40c82dd76af764da1da0d9e68ec196623951d00deb12e25f945ae06"
    one = lambda k: hashlib.sha256(sd[k].numpy().tobytes()).hexdigest()
    assert one("visual.conv1.weight") == "00df7ea6ea015a729abd6036862ea4ec903871048215c580b064e96bcabf4638"
    assert one("visual.positional_embedding") == "2383df7e25b47c8cd9a692800770ac63310674e50e4b1c26dbc9807edc7e8d26"
    assert one("visual.proj") == "15938b749da18d208a23b63dc3f58c51918cce47d254bf646cc1411d8a1bb369"
    assert _digest(clip_vit_random_state_dict(0, patch=32)) == _digest(sd)
    s16 = clip_vit_random_state_dict(0, patch=16)
    assert set(s16) == set(sd)
    assert tuple(s16["visual.conv1.weight"].shape) == (768, 3, 16, 16)
    assert tuple(s16["visual.positional_embedding"].shape) == (197, 768)
    for k in sd:
        if k not in ("visual.conv1.weight", "visual.positional_embedding"):
            assert s16[k].shape == sd[k].shape, k
    with pytest.raises(ValueError):
        clip_vit_random_state_dict(0, patch=14)


def test_patched_oracle_matches_transformers_clip_vision_at_patch_16(monkeypatch):
    tr = pytest.importorskip("transformers")
    _b16(monkeypatch)
    sd = C.random_state_dict(0)
    assert tuple(sd["visual.conv1.weight"].shape) == (768, 3, 16, 16) and sd["visual.positional_embedding"].shape[0] == 197
    cfg = tr.CLIPVisionConfig(patch_size=16)
    assert (cfg.hidden_size, cfg.num_hidden_layers, cfg.patch_size, cfg.image_size, cfg.projection_dim, cfg.hidden_act) == \
        (768, 12, 16, 224, 512, "quick_gelu")
    model = tr.CLIPVisionModelWithProjection(cfg).eval()
    missing, unexpected = model.load_state_dict(C.to_hf_state_dict(sd), strict=False)
    assert not unexpected and all("position_ids" in m for m in missing), (missing, unexpected)
    img = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = model(pixel_values=img).image_embeds
        out = C.encode_image(sd, img)
    print("patched oracle vs transformers at patch 16: max |diff|", (out - ref).abs().max().item())
    assert torch.allclose(out, ref, atol=1e-4, rtol=0), (out - ref).abs().max()
