"""Shared by tests/test_net_shapes_cpu.py and tests/test_gpu_net_shapes.py: the scaled-down network shapes (packing.SUPPORTED beyond the
two the reference ships), their reference fixtures (scripts/gen_golden_shapes.py) and the spec-taking mask code of the panel tests."""
import glob
import os
from functools import lru_cache

import numpy as np
import torch

from avatarclip_amd import packing as PK
from tests.helpers import GOLDEN

ALL_SHAPES = [(256, 2, 1), (128, 1, 0), (128, 2, 1), (256, 1, 0), (64, 2, 1), (64, 1, 0)]     # in the order of their net ids
NEW_SHAPES = ALL_SHAPES[2:]
SHAPE_IDS = ["%d_%d_%d" % s for s in NEW_SHAPES]


def confs(spec):
    """the reference's network sections (confs/examples/*.conf: model.sdf_network / model.rendering_network) at this shape"""
    H = spec.H
    sdf = dict(d_out=H + 1, d_in=3, d_hidden=H, n_layers=spec.NMID + 2, skip_in=[spec.NMID + 2], multires=6, bias=0.5, scale=1.0,
               geometric_init=True, weight_norm=True)
    col = dict(d_feature=H, mode="no_view_dir", d_in=6, d_out=3, d_hidden=H, n_layers=spec.NCMID + 1, weight_norm=True,
               multires_view=0, squeeze_out=True, extra_color=True)
    return sdf, col


@lru_cache(maxsize=None)
def _load(shape):
    """the parts of one fixture (disjoint keys, each file below the size limit for a committed file) merged; loaded once and shared"""
    paths = sorted(glob.glob(os.path.join(GOLDEN, "neus_shape_%d_%d_%d*.npz" % shape)))
    assert paths, shape
    rec = {}
    for p in paths:
        z = np.load(p)
        assert not set(z.files) & set(rec), p
        rec.update({k: z[k] for k in z.files})
    return rec


def load_shape_case(shape):
    """(rec, sdf state dict, colour state dict, variance) as tests/helpers.load_case; fresh tensors over the shared arrays"""
    rec = {k: torch.from_numpy(v.copy()) for k, v in _load(tuple(shape)).items()}
    sd = {p: {k[len(p) + 1:]: v for k, v in rec.items() if k.startswith(p + ".")} for p in ("sdf", "col", "var")}
    return rec, sd["sdf"], sd["col"], sd["var"]["variance"]


# ---- the ReLU masks for any NetSpec (tests/panel_restatement.py: decode_masks / encode_masks know the two shipped nets only).
# include/avc.h: [layer][tile][lane] x 16 bits per block, 2 * HT * 64 words whatever NCMID is, bit (r >> 1) + 8 (r & 1) = feature row r of
# the lane's 16 rows; rows 0..7 are the slots of the tile's first fragment, 8..15 of its second.
_MASK_BIT = np.array([[(r >> 1) + 8 * (r & 1) for r in range(8 * e, 8 * e + 8)] for e in range(2)])            # [e][j]


def decode_masks(raw_u16, spec, nblk=None):
    """-> bool [nblk][layer][tile][2][64][8], the > 0 pattern in the shape of the R1 (/ R2) fragments; a layer the shape does not have
    (NCMID = 0: the second) is left out"""
    per_block = 2 * spec.HT * 64
    raw = np.asarray(raw_u16).reshape(-1).view(np.uint16)
    nblk = raw.size // per_block if nblk is None else nblk
    m = raw[:nblk * per_block].reshape(nblk, 2, spec.HT, 64).astype(np.uint32)
    out = (m[:, :, :, None, :, None] >> _MASK_BIT[None, None, None, :, None, :]) & 1                            # [b][layer][t][e][lane][j]
    return out[:, :spec.NCMID + 1].astype(bool)


def encode_masks(pattern, spec):
    """the inverse of decode_masks: bool [nblk][layer][tile][2][64][8] -> uint16 [nblk * 2 * HT * 64] (a missing layer: zeros)"""
    pattern = np.asarray(pattern, bool)
    m = np.zeros((pattern.shape[0], 2, spec.HT, 64), np.uint32)
    m[:, :pattern.shape[1]] = (pattern.astype(np.uint32) << _MASK_BIT[None, None, None, :, None, :]).sum(axis=(3, 5))
    return m.astype(np.uint16).reshape(-1)


def seeded_renderer(spec, dev, seed=0):
    """tests/engine_cases._nets at any supported shape: the project's modules with their seeded geometric init"""
    from avatarclip_amd import fields, renderer
    torch.manual_seed(seed)
    sdf_conf, col_conf = confs(spec)
    sdf = fields.SDFNetwork(**{k: v for k, v in sdf_conf.items() if k in ("d_out", "d_in", "d_hidden", "n_layers", "skip_in", "multires")})
    col = fields.RenderingNetwork(**{k: v for k, v in col_conf.items() if k in ("d_feature", "mode", "d_in", "d_out", "d_hidden", "n_layers", "extra_color")})
    var = fields.SingleVarianceNetwork(0.3)
    sdf, col, var = sdf.to(dev), col.to(dev), var.to(dev)
    return renderer.NeuSRenderer(None, sdf, var, col, 32, 32, 0, 4, 1.0, True)
