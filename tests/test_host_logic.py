"""CPU tests of the host-side logic: conf parser, ray generation vs the golden vectors, camera helpers,
fields state-dict compatibility with the reference checkpoint layout, C-ABI symbol export."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import load_case, GOLDEN, ROOT

EXAMPLE_CONF = """
general {
    base_exp_dir = ./exp/smpl/example
    recording = [
        ./,
        ./models
    ]
}
train {
    learning_rate = 5e-4
    end_iter = 30000
    use_white_bkgd = False
    warm_up_end = 500
    mask_weight = 1.0   # trailing comment
    add_no_texture = True
}
clip {
    prompt = a 3D rendering of a {TOREPLACE} in unreal engine
}
model {
    nerf {
        D = 4,
        skips=[4],
        use_viewdirs=True
    }
    sdf_network {
        d_out = 129
        skip_in = [3]
        scale = 1.0
    }
    neus_renderer {
        up_sample_steps = 4     # 1 for simple coarse-to-fine sampling
        perturb = 1.0
    }
}
"""


def test_conf_parser_subset():
    from avatarclip_amd.conf import ConfigFactory
    c = ConfigFactory.parse_string(EXAMPLE_CONF)
    assert c["general.base_exp_dir"] == "./exp/smpl/example"
    assert c["general.recording"] == ["./", "./models"]
    assert c.get_float("train.learning_rate") == 5e-4 and c.get_int("train.end_iter") == 30000
    assert c.get_bool("train.use_white_bkgd") is False and c.get_bool("train.add_no_texture") is True
    assert c.get_float("train.mask_weight") == 1.0
    assert c.get_string("clip.prompt") == "a 3D rendering of a {TOREPLACE} in unreal engine"
    assert c["model.nerf.D"] == 4 and c["model.nerf.skips"] == [4] and c["model.nerf.use_viewdirs"] is True
    assert dict(c["model.sdf_network"]) == {"d_out": 129, "skip_in": [3], "scale": 1.0}
    assert c["model.neus_renderer.up_sample_steps"] == 4
    assert c.get_float("train.anneal_end", default=0.0) == 0.0
    try:
        c.get_float("train.clip_weight")
        assert False
    except KeyError:
        pass


def test_rays_match_reference_golden():
    from avatarclip_amd.dataset import SMPL_Dataset
    from avatarclip_amd import utils as U
    z = np.load(os.path.join(GOLDEN, "rays_cam.npz"))
    ds = SMPL_Dataset(None, device="cpu", H=256, W=256)
    assert abs(ds.focal - float(z["focal"])) < 1e-9
    pose = torch.from_numpy(z["pose58"])
    for lvl in (4, 2.25):
        o, v = ds.gen_rays_pose(pose, lvl)
        assert np.allclose(o.numpy(), z["rays_o_l%s" % lvl], atol=1e-6) and np.allclose(v.numpy(), z["rays_v_l%s" % lvl], atol=1e-6)
    o, v = ds.gen_rays_pose(pose, 4)
    near, far = ds.near_far_from_sphere(o.reshape(-1, 3), v.reshape(-1, 3))
    assert np.allclose(near.numpy(), z["near_l4"], atol=1e-6) and np.allclose(far.numpy(), z["far_l4"], atol=1e-6)
    np.random.seed(0)
    for k in range(8):
        eye, theta, phi, is_front = U.random_eye_normal()
        at = U.random_at().astype(np.float32)
        eye = eye.astype(np.float32) + at
        assert np.allclose(eye, z["cam_eye"][k]) and np.allclose(at, z["cam_at"][k])
        assert np.allclose(U.lookat(eye, at, np.array([0, 1, 0])), z["cam_pose"][k], atol=1e-6)
        assert np.allclose([theta, phi, is_front], z["cam_aux"][k])
    for i in range(6):
        assert np.allclose(U.sphere_coord(0.3 * i, 0.7 * i), z["sphere_coord"][i])


def test_fields_state_dict_compat_and_torch_forward():
    """Reference checkpoint keys load unmodified; the API-compat torch forward equals the oracle."""
    from avatarclip_amd import fields
    from oracle import neus_oracle as O
    rec, sd_sdf, sd_col, variance = load_case("neus_small.npz")
    sdf = fields.SDFNetwork(d_out=129, d_in=3, d_hidden=128, n_layers=3, skip_in=[3], multires=6, bias=0.5, scale=1.0,
                            geometric_init=True, weight_norm=True)
    col = fields.RenderingNetwork(d_feature=128, mode="no_view_dir", d_in=6, d_out=3, d_hidden=128, n_layers=1,
                                  weight_norm=True, multires_view=0, squeeze_out=True, extra_color=True)
    assert set(sdf.state_dict().keys()) == set(sd_sdf.keys())
    assert set(col.state_dict().keys()) == set(sd_col.keys())
    sdf.load_state_dict(sd_sdf)
    col.load_state_dict(sd_col)
    x = torch.rand(64, 3) - 0.5
    assert torch.allclose(sdf(x), O.sdf_forward(sd_sdf, x), atol=1e-6)
    n = torch.randn(64, 3)
    feat = torch.randn(64, 128)
    assert torch.allclose(col(x, n, None, feat), O.color_forward(sd_col, x, n, feat), atol=1e-6)
    # dense flattening order == packing.param_shapes
    from avatarclip_amd import packing as PK
    from avatarclip_amd.engine import flatten_dense
    flat = flatten_dense(sdf, col, PK.SMALL)
    assert flat.numel() == PK.layout_for(PK.SMALL).nparam


def test_runner_loads_the_reference_s_own_conf_and_shipped_checkpoint(tmp_path, monkeypatch):
    """the reference's shipped `pretrained_models/zero_beta_stand_pose_small.pth` through the product's OWN loading path --
    Runner.__init__ on the reference's confs/examples_small/example.conf UNMODIFIED (its relative `train.pretrain`, main.py:153-155 -> Runner.load_pretrain,
    main.py:611-618 incl. the non-strict colour load that leaves `extra_lin` at its seeded init) -- and not only via a golden state dict.  The loaded
    weights must equal the ones oracle/gen_golden.py read with the reference's modules (tests/golden/neus_small.npz).  Needs the reference tree (build
    container); the GPU box never holds it."""
    from oracle import ref_loader
    if not ref_loader.reference_available():
        pytest.skip("no reference tree on this machine")
    from avatarclip_amd.conf import ConfigFactory
    from avatarclip_amd.runner import Runner
    ag = ref_loader.REF_AG
    conf_path = os.path.join(ag, "confs", "examples_small", "example.conf")
    conf = ConfigFactory.parse_string(open(conf_path).read())
    assert conf.get_string("train.pretrain") == "./pretrained_models/zero_beta_stand_pose_small.pth"
    conf.put("general.base_exp_dir", str(tmp_path / "exp"))          # (the only edit: the reference tree is read-only)
    monkeypatch.chdir(ag)                                            # the conf's paths are relative to AppearanceGen/, as `python main.py` runs there
    r = Runner(conf_path, mode="train_clip", conf=conf, device=torch.device("cpu"), allow_standins=True)
    rec, sd_sdf, sd_col, variance = load_case("neus_small.npz")
    for k, v in sd_sdf.items():
        assert torch.equal(r.sdf_network.state_dict()[k], v), k
    assert torch.equal(r.deviation_network.variance.detach(), variance)
    ck = r._torch_load(os.path.join(ag, "pretrained_models", "zero_beta_stand_pose_small.pth"))     # (the tensors-only unpickler + numpy scalars: the file's optimizer state holds one)
    loaded = r.color_network.state_dict()
    for k, v in ck["color_network_fine"].items():                    # every tensor the checkpoint HAS is loaded ...
        assert torch.equal(loaded[k], v), k
    assert {k for k in loaded if k not in ck["color_network_fine"]} == {"extra_lin.bias", "extra_lin.weight_g", "extra_lin.weight_v"}   # ... main.py:617
    assert r.iter_step == 0 and set(ck.keys()) >= {"sdf_network_fine", "variance_network_fine", "color_network_fine"}


def test_c_abi_exports_every_declared_symbol():
    from avatarclip_amd import build
    path = build.build()
    lib = ctypes.CDLL(path)

    def declared(header):
        hdr = open(os.path.join(ROOT, "include", header)).read()
        hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
        return re.findall(r"\b(avc_\w+)\s*\(", hdr)
    names = declared("avc.h")
    assert len(names) >= 14
    for n in names:
        assert hasattr(lib, n), n
    lib.avc_version.restype = ctypes.c_int
    assert lib.avc_version() >= 1
    # the binding derives itself from the same header: it binds every declared name, with one argtype per declared parameter
    from avatarclip_amd import lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "avc.h")).read(), flags=re.S)
    bound = L.load()
    for n, params in re.findall(r"\b(avc_\w+)\s*\(([^)]*)\)\s*;", hdr):
        count = 0 if params.strip() in ("", "void") else len(params.split(","))
        assert len(getattr(bound, n).argtypes) == count, n
    assert len(re.findall(r"\b(avc_\w+)\s*\(([^)]*)\)\s*;", hdr)) == len(names)
    # the entry points of the retired role-specialised backward (profiles/r04_ring_handoff.md) are gone from the library
    for n in ("avc_bwd_ring_ctl_bytes", "avc_bwd_ring_payload_bytes", "avc_bwd_ring_types", "avc_render_points_bwd_ring"):
        assert not hasattr(lib, n), n


def test_gaussian_blur_matches_depthwise_convolution():
    """runner._gaussian_blur (shifted multiply-adds) == the separable depthwise convolution of torchvision's GaussianBlur"""
    import torch.nn.functional as F
    from avatarclip_amd.runner import _gaussian_blur
    torch.manual_seed(3)
    x = torch.rand(1, 1, 40, 36)
    ksize, sigma = (5, 9), 1.3

    def k1d(k):
        r = torch.arange(k, dtype=x.dtype) - (k - 1) / 2
        w = torch.exp(-0.5 * (r / sigma) ** 2)
        return w / w.sum()
    ref = F.pad(x, (2, 2, 4, 4), mode="reflect")
    ref = F.conv2d(ref, k1d(5).view(1, 1, 1, -1))
    ref = F.conv2d(ref, k1d(9).view(1, 1, -1, 1))
    out = _gaussian_blur(x, ksize, sigma)
    assert out.shape == x.shape
    assert (out - ref).abs().max() < 1e-6


def test_conf_parser_reads_every_reference_conf():
    """the reference's own conf files (pyhocon syntax) parse with our HOCON subset and carry every key Runner reads.
    Runs only where the reference checkout is mounted (the build container)."""
    import glob
    import os
    from avatarclip_amd.conf import ConfigFactory
    from oracle import ref_loader
    root = os.path.join(ref_loader.REF_AG, "confs")
    files = sorted(glob.glob(os.path.join(root, "**", "*.conf"), recursive=True))
    if not files:
        pytest.skip("reference checkout not present")
    for f in files:
        text = open(f).read().replace("CASE_NAME", "case")
        c = ConfigFactory.parse_string(text)
        assert c.get_string("general.base_exp_dir")
        assert c.get_int("train.end_iter") > 0 and c.get_float("train.learning_rate") > 0
        assert c.get_int("model.sdf_network.d_hidden") in (128, 256)
        assert c.get_int("model.neus_renderer.n_samples") > 0 and c.get_int("model.neus_renderer.up_sample_steps") == 4
        sk = c["model.sdf_network"]["skip_in"]
        assert list(sk) == [c.get_int("model.sdf_network.n_layers")]
        if "clip" in c:
            assert isinstance(c.get_string("clip.prompt"), str) and len(c.get_string("clip.prompt")) > 3


def test_h2d_helpers_on_cpu_and_constant_cache():
    """avatarclip_amd/h2d.py: on a CPU device `upload` is a plain conversion, `const` returns ONE cached tensor per (values, device, dtype)"""
    import numpy as np
    import torch
    from avatarclip_amd import h2d
    a = h2d.upload(np.arange(12.0).reshape(3, 4), "cpu")
    assert a.dtype == torch.float32 and a.shape == (3, 4) and float(a[2, 3]) == 11.0
    c1 = h2d.const((0.5, 0.25, 0.125), "cpu")
    c2 = h2d.const([0.5, 0.25, 0.125], "cpu")
    assert c1 is c2 and c1.tolist() == [0.5, 0.25, 0.125]
    assert h2d.const((0.5, 0.25, 0.125), "cpu", torch.float64) is not c1


def test_panel_plan_arithmetic():
    """engine.plan_panels: how a ray set is cut into chunks (F panels) and slabs (G panels) for a memory budget -- the cases of
    BASELINE's configurations on a 288-GB device and the degenerate ones"""
    from avatarclip_amd.engine import plan_panels
    blk_f, blk_g = 89 * 2048 + 1024, 83 * 2048                      # full nets (csrc/avc_mlp.h: PanelLayout)
    gib = 1 << 30
    budget = int(266 * 0.8) * gib
    nbytes = lambda rays, slab, S: ((rays * S + 31) // 32 + 1) * blk_f + ((slab * S + 31) // 32 + 1) * blk_g
    # 512^2 x 64 spp: one chunk, two slabs of 256 Ki blocks
    chunk, slab = plan_panels(512 * 512, 64, budget, blk_f, blk_g, 256 * 1024, 32 * 1024)
    assert (chunk, slab) == (262144, 131072) and nbytes(chunk, slab, 64) < 140 * gib
    # 512^2 x 128 spp (config 3 per GPU): still one chunk, the slab halved until it fits
    chunk, slab = plan_panels(512 * 512, 128, budget, blk_f, blk_g, 256 * 1024, 32 * 1024)
    assert chunk == 262144 and slab == 32768 and nbytes(chunk, slab, 128) <= budget
    # 224^2: everything in one slab
    assert plan_panels(224 * 224, 64, budget, blk_f, blk_g, 256 * 1024, 32 * 1024) == (50176, 50176)
    # a 3-GiB budget: chunks of whole slabs, multiples of 32 rays, inside the budget
    chunk, slab = plan_panels(512 * 512, 64, 3 * gib, blk_f, blk_g, 256 * 1024, 32 * 1024)
    assert 0 < slab <= chunk < 262144 and chunk % 32 == 0 and slab % 32 == 0 and nbytes(chunk, slab, 64) <= 3 * gib
    # samples per ray that do not divide the block: slab boundaries still fall on blocks
    chunk, slab = plan_panels(1000, 48, 1 << 26, 33 * 2048 + 1024, 35 * 2048, 160, 32 * 1024)
    assert slab % 32 == 0 and chunk % 32 == 0 and (slab * 48) % 32 == 0 and slab < chunk < 1000
    # tiny ray sets are never cut
    assert plan_panels(1, 64, 1 << 26, blk_f, blk_g, 256 * 1024, 32 * 1024) == (1, 1)
    assert plan_panels(33, 64, 1 << 26, blk_f, blk_g, 256 * 1024, 32 * 1024) == (33, 33)
    # one gradient slab or two is decided by the memory that is FREE, not by a constant (Engine.plan: budget = min(AVC_PANEL_GIB,
    # 80 % of the free HBM); default slab = 512 Ki blocks): an empty 288-GB MI355X takes 512^2 x 64 spp in one 84-GiB slab
    # (87 + 84 = 172 GiB), the same device with 100 GB held by somebody else falls back to two 42-GiB slabs, with 160 GB held to
    # eight, and the view is still ONE forward chunk
    full_dev = int(0.8 * 268 * gib)
    assert plan_panels(512 * 512, 64, min(224 * gib, full_dev), blk_f, blk_g, 512 * 1024, 32 * 1024) == (262144, 262144)
    assert plan_panels(512 * 512, 64, int(0.8 * 175 * gib), blk_f, blk_g, 512 * 1024, 32 * 1024) == (262144, 131072)
    assert plan_panels(512 * 512, 64, int(0.8 * 150 * gib), blk_f, blk_g, 512 * 1024, 32 * 1024) == (262144, 65536)
    assert plan_panels(512 * 512, 64, int(0.8 * 125 * gib), blk_f, blk_g, 512 * 1024, 32 * 1024) == (262144, 32768)
    chunk, slab = plan_panels(512 * 512, 64, int(0.8 * 100 * gib), blk_f, blk_g, 512 * 1024, 32 * 1024)   # below ~96 GiB the view is cut
    assert chunk < 262144 and nbytes(chunk, slab, 64) <= 80 * gib


def test_softplus_direct_form_and_relu_mask_bit_order_restated():
    """The two instruction-level rewrites of round 3, restated in numpy / plain Python (the GPU parity tests exercise the kernels; this
    pins the arithmetic they rely on without a GPU):
      * csrc/avc_common.h softplus2: H = median(log2(1 + 2^t), t, 128) in fp32 equals the split form max(t, 0) + log2(1 + 2^-|t|)
        over the whole range, including t >= 128 where 2^t overflows and the logarithm returns +inf;
      * csrc/avc_common.h relu_frags / relu_mask_bit: gathering bit p from the LOW half and bit 16 + p from the HIGH half of register
        pair p (v_pk_min_u16 + v_lshl_or), folded to 16 bits as (m & 0xff) | (m >> 8), puts accumulator register r at bit
        (r >> 1) + 8 (r & 1) -- the position the backward kernel tests."""
    t = np.concatenate([np.linspace(-200, 200, 4001), np.array([-1e4, -127.9, 126.5, 127.999, 128.0, 128.5, 300.0, 6e4])]).astype(np.float32)
    with np.errstate(over="ignore"):
        L = np.log2(np.float32(1) + np.exp2(t)).astype(np.float32)           # +inf where 2^t overflows
    direct = np.median(np.stack([L, t, np.full_like(t, 128.0)]), axis=0).astype(np.float32)
    split = (np.maximum(t, 0) + np.log2(np.float32(1) + np.exp2(-np.abs(t)))).astype(np.float32)
    assert np.isfinite(direct).all()
    assert np.abs(direct - split).max() <= 2e-6 * max(1.0, 0) + np.abs(split).max() * 2.4e-7     # one fp32 ulp of the larger values
    assert (direct[t >= 128] == t[t >= 128]).all()
    # mask bit order: registers a[0..15] of one lane -> 8 register pairs (a[2p], a[2p+1]) after the f16 conversion
    rng = np.random.default_rng(0)
    for _ in range(50):
        a = rng.standard_normal(16).astype(np.float32)
        a[rng.integers(0, 16, 4)] = 0.0
        m = 0
        for p in range(8):
            lo, hi = a[2 * p] > 0, a[2 * p + 1] > 0           # v_pk_max_i16 + v_pk_min_u16: 1 per half whose relu'd f16 pattern is non-zero
            m |= (int(lo) | (int(hi) << 16)) << p
        bits = (m & 0xFF) | (m >> 8)
        for r in range(16):
            assert ((bits >> ((r >> 1) + 8 * (r & 1))) & 1) == int(a[r] > 0), (r, a)
        assert bits < (1 << 16)


def test_bench_runs_its_extra_legs_only_with_full():
    """a plain `bench.py` run is the headline alone; --full adds the extra_configs legs and the CPU baseline (single-GPU runs), and
    --no-extra / --no-cpu-baseline drop one of them again"""
    import bench
    plain = ["--gpus", "1", "--steps", "10", "--warmup", "5"]
    assert bench.optional_legs(bench.parse_args(plain), 1) == (False, False)
    assert bench.optional_legs(bench.parse_args(plain + ["--dump-outputs", "d"]), 1) == (False, False)
    full = plain + ["--full"]
    assert bench.optional_legs(bench.parse_args(full), 1) == (True, True)
    assert bench.optional_legs(bench.parse_args(full + ["--no-extra"]), 1) == (False, True)
    assert bench.optional_legs(bench.parse_args(full + ["--no-cpu-baseline"]), 1) == (True, False)
    assert bench.optional_legs(bench.parse_args(full + ["--small"]), 1) == (False, True)
    assert bench.optional_legs(bench.parse_args(full + ["--res", "224"]), 1) == (False, True)
    assert bench.optional_legs(bench.parse_args(["--gpus", "2", "--full"]), 2) == (False, False)
