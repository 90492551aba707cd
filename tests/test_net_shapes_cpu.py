"""The host half of the scaled-down network shapes (no GPU): which confs packing.spec_from_conf accepts and under which net id, the
generated offsets header, and the emulated wave / weight-gradient / unpack chain at the four new shapes on their fixtures' weights."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from avatarclip_amd import packing as PK
from oracle import analytic as A
from tests import wave_emulator as E
from tests.helpers import ROOT
from tests.net_shapes_common import ALL_SHAPES, NEW_SHAPES, SHAPE_IDS, confs, decode_masks, encode_masks, load_shape_case
from tests.test_packing_emulation import dense_grads_flat, flat_from_net


def test_spec_from_conf_accepts_the_six_shapes_and_names_them_when_it_refuses():
    assert [(sp.H, sp.NMID, sp.NCMID) for _, _, sp in PK.SUPPORTED] == ALL_SHAPES and [i for i, _, _ in PK.SUPPORTED] == list(range(6))
    for net_id, shape in enumerate(ALL_SHAPES):
        spec = PK.NetSpec(*shape)
        got = PK.spec_from_conf(*confs(spec))
        assert got == spec and got.net_id == net_id, shape
    assert (PK.FULL.net_id, PK.SMALL.net_id) == (0, 1)

    def refused(sdf, col):
        with pytest.raises(NotImplementedError) as e:
            PK.spec_from_conf(sdf, col)
        msg = str(e.value)
        for H, nmid, ncmid in ALL_SHAPES:
            assert "d_hidden %d with SDF n_layers %d + colour n_layers %d" % (H, nmid + 2, ncmid + 1) in msg, (H, nmid, ncmid, msg)
    for shape in ((128, 2, 0), (192, 2, 1), (512, 2, 1)):       # a mixed depth, a width between two supported ones, a wider net
        refused(*confs(PK.NetSpec(*shape)))
    for shape in ALL_SHAPES:                                     # every other key the kernels hard-code stays checked at every shape
        sdf, col = confs(PK.NetSpec(*shape))
        refused(dict(sdf, multires=4), col)
        refused(dict(sdf, skip_in=[1]), col)
        refused(dict(sdf, d_out=shape[0]), col)
        refused(dict(sdf, scale=2.0), col)
        refused(dict(sdf, d_in=2), col)
        refused(sdf, dict(col, mode="idr"))
        refused(sdf, dict(col, squeeze_out=False))
    with pytest.raises(KeyError):
        PK.NetSpec(192, 2, 1).net_id                             # a shape outside the table has no id (it used to be "1")


def test_generated_offsets_header_has_one_specialisation_per_shape_and_is_the_committed_one():
    spec = importlib.util.spec_from_file_location("gen_offsets", os.path.join(ROOT, "scripts", "gen_offsets.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    txt = mod.render()
    assert txt == open(os.path.join(ROOT, "avatarclip_amd", "csrc", "avc_offsets_gen.h")).read()
    assert txt.count("template <> struct Off<") == len(PK.SUPPORTED) == 6
    mlp_h = open(os.path.join(ROOT, "avatarclip_amd", "csrc", "avc_mlp.h")).read()
    avc_h = open(os.path.join(ROOT, "include", "avc.h")).read()
    for net_id, name, sp in PK.SUPPORTED:
        lay = PK.layout_for(sp)
        vals = ", ".join(str(int(v)) for v in lay.offsets)
        assert "struct Off<%s> { static constexpr AvcOffsets value = {{%s}}; };" % (name, vals) in txt
        # the same list in the device code (type and dispatch entry) and in the ABI header
        assert "typedef NetT<%d, %d, %d> %s;" % (sp.H, sp.NMID, sp.NCMID, name) in mlp_h
        assert "case %d: return f(NetTag<%s>{});" % (net_id, name) in mlp_h
        assert lay.offsets[PK.OFF["OFF_TAB_END"]] * 4 <= 10240              # AVC_TAB_LDS_BYTES: the fp32 table fits its LDS window
    assert "#define AVC_NET_COUNT 6" in avc_h
    assert [int(l.split()[2]) for l in avc_h.splitlines() if l.startswith("#define AVC_NET_") and "COUNT" not in l] == list(range(6))


def test_split_sum_buffers_of_every_supported_shape_are_whole_float4s():
    """avc_weight_grad_reduce / _unpack move four floats per lane over [gout | gbias], and Engine.points_bwd has no other tail: both
    sizes are multiples of 4 in every row of packing.SUPPORTED."""
    for _, name, sp in PK.SUPPORTED:
        lay = PK.layout_for(sp)
        assert lay.gout_size % 4 == 0 and lay.gbias_size % 4 == 0, (name, lay.gout_size, lay.gbias_size)


@pytest.mark.parametrize("shape", NEW_SHAPES, ids=SHAPE_IDS)
def test_emulated_wave_matches_analytic_at_the_new_shapes(shape):
    """the statement of tests/test_packing_emulation.py::test_emulated_wave_matches_analytic, same 1e-6 gate, on the fixture's weights"""
    spec = PK.NetSpec(*shape)
    rec, sd_sdf, sd_col, variance = load_shape_case(shape)
    net = A.dense_net(sd_sdf, sd_col, torch.float64)
    lay = PK.layout_for(spec)
    flat = flat_from_net(net, lay)
    blob = E.Blob(lay, flat)
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(64, 3, generator=g, dtype=torch.float64) * 2 - 1) * 0.8
    d_sdf = torch.randn(64, 1, generator=g, dtype=torch.float64)
    d_n = torch.randn(64, 3, generator=g, dtype=torch.float64)
    d_rgb = torch.randn(64, 6, generator=g, dtype=torch.float64)
    f = A.mlp_forward(net, x)
    mb = A.mlp_backward(net, f, d_sdf, d_n, d_rgb)
    ref = dense_grads_flat(mb, lay)
    blocks = []
    for b in range(2):
        sl = slice(32 * b, 32 * b + 32)
        panels, (sdf, n, rgb) = E.backward_wave(spec, blob, x[sl].numpy(), d_sdf[sl, 0].numpy(), d_n[sl].numpy(), d_rgb[sl].numpy())
        assert np.allclose(sdf, f["sdf"][sl, 0].numpy(), atol=1e-9)
        assert np.allclose(n, f["n"][sl].numpy(), atol=1e-8)
        assert np.allclose(rgb, f["rgb6"][sl].numpy(), atol=1e-9)
        blocks.append(panels)
    gout, gbias = E.weight_grad(lay, blocks)
    assert blocks[0]["colsum"].shape == (lay.cs_size,)
    grad = E.unpack_grad(lay, gout, gbias, sum(b["colsum"] for b in blocks))
    off = 0
    for pname, shp in lay.shapes:
        n_ = int(np.prod(shp))
        a, b_ = grad[off:off + n_], ref[off:off + n_]
        err = np.abs(a - b_).max() / (np.abs(b_).max() + 1e-30)
        assert err < 1e-6, (pname, err)
        off += n_


def test_spec_taking_mask_code_agrees_with_the_two_net_one_and_round_trips():
    from tests import panel_restatement as PR
    rs = np.random.RandomState(0)
    for shape in ALL_SHAPES:
        spec = PK.NetSpec(*shape)
        raw = rs.randint(0, 1 << 16, size=3 * 2 * spec.HT * 64).astype(np.uint16)
        pat = decode_masks(raw, spec)
        assert pat.shape == (3, spec.NCMID + 1, spec.HT, 2, 64, 8)
        back = encode_masks(pat, spec).reshape(3, 2, spec.HT, 64)
        assert np.array_equal(back[:, :spec.NCMID + 1], raw.reshape(3, 2, spec.HT, 64)[:, :spec.NCMID + 1]) and not back[:, spec.NCMID + 1:].any()
        if spec in (PK.FULL, PK.SMALL):
            assert np.array_equal(pat, PR.decode_masks(raw, spec))
