"""Informational timing of one 224 x 224 rays x 64 samples render iteration (pack, hierarchical sampling, training forward, backward with
the weight-gradient products) at every supported network shape (packing.SUPPORTED), one GPU, seeded geometric-init nets -- the NeuS half
of a CLIP-guided step, without CLIP and Adam.  Nothing is tuned per shape and no target is attached (profiles/net_shapes.md).
    python scripts/net_shapes_time.py [--res 224] [--iters 7] [--warmup 3] [--json OUT]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avatarclip_amd import fields, packing as PK, renderer  # noqa: E402
from oracle import neus_oracle as O  # noqa: E402


def time_shape(spec, res, iters, warmup, dev):
    torch.manual_seed(0)
    H = spec.H
    sdf = fields.SDFNetwork(d_out=H + 1, d_in=3, d_hidden=H, n_layers=spec.NMID + 2, skip_in=[spec.NMID + 2], multires=6)
    col = fields.RenderingNetwork(d_feature=H, mode="no_view_dir", d_in=6, d_out=3, d_hidden=H, n_layers=spec.NCMID + 1, extra_color=True)
    var = fields.SingleVarianceNetwork(0.3)
    sdf, col, var = sdf.to(dev), col.to(dev), var.to(dev)
    ren = renderer.NeuSRenderer(None, sdf, var, col, 32, 32, 0, 4, 1.0, True)
    assert ren.engine.net == spec.net_id
    pose = torch.from_numpy(O.lookat(np.array([0., 0.2, 1.5]), np.zeros(3), np.array([0., 1, 0]))).float()
    o, v = O.gen_rays_pose(pose, res, res, 0.5 * res / np.tan(np.pi / 6))
    ro, rd = o.reshape(-1, 3).contiguous().to(dev), v.reshape(-1, 3).contiguous().to(dev)
    near, far = O.near_far_from_sphere(ro, rd)
    bg = torch.zeros(1, 3, device=dev)
    times = []
    for i in range(warmup + iters):
        for p in list(sdf.parameters()) + list(col.parameters()) + list(var.parameters()):
            p.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        flat = ren.flat_params()
        pk = ren.engine.pack(flat)
        z = ren.sample_z(pk, ro, rd, near, far, 1.0)
        ret = ren.render_core(ro, rd, z, 2.0 / 32, bg, 1.0, flat)
        loss = ret["color"].mean() + ret["extra_color"].mean() + 0.1 * ret["gradient_error"] + ret["weights"].sum(-1).mean()
        loss.backward()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    assert np.isfinite(loss.item())
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=224)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    rows = []
    for net_id, name, spec in PK.SUPPORTED:
        med, lo, hi = time_shape(spec, args.res, args.iters, args.warmup, dev)
        rows.append(dict(net=net_id, H=spec.H, NMID=spec.NMID, NCMID=spec.NCMID, ms_median=med, ms_min=lo, ms_max=hi))
        print("net %d  %-15s H %3d, %d + %d layers: %8.2f ms (min %.2f, max %.2f) per %d x %d x 64 render iteration"
              % (net_id, name, spec.H, spec.NMID + 2, spec.NCMID + 1, med, lo, hi, args.res, args.res), flush=True)
    if args.json:
        json.dump(rows, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
