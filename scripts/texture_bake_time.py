"""One texture bake timed at production size (profiles/texture_bake.md): an analytic ellipsoid "body" meshed by the project's own marching
cubes at --res 512 as the dense mesh, vertex clustering at --divisor 64, a --size 2048 atlas.  Prints one JSON line: the sizes, the bake
split into grid build, query and the rest (bake.bake_texture's stats, after a small warm-up bake), the candidate triangles per query, and
beside it a chunked brute-force torch fp64 closest-point baseline (every query against every dense triangle) on --baseline of the bake's
own queries, with the number of those queries on which the two agree bit for bit.
    python scripts/texture_bake_time.py [--res 512] [--divisor 64] [--size 2048] [--baseline 4096] [--out profiles/texture_bake.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from avatarclip_amd import bake, mesh, rig  # noqa: E402
from avatarclip_amd import lib as L  # noqa: E402

AXES = (0.30, 0.85, 0.20)                 # semi-axes of the body in the [-1, 1]^3 box


def ellipsoid(points):
    a = torch.tensor(AXES, device=points.device)
    return torch.linalg.norm(points / a, dim=-1) - 1.0


def brute_force(p, v, t, q_chunk=512, f_chunk=16384):
    """torch fp64, every query against every triangle in blocks: Ericson 5.1.5 in the order of csrc/avc_bake.h as a chain of torch.where
    (the first rule that holds), a running (d2, index) minimum with ties to the lower index.  Degenerate triangles are skipped."""
    vv = v.double()
    A, B, C = (vv[t[:, k].long()] for k in range(3))
    ab, ac = B - A, C - A
    n = torch.linalg.cross(ab, ac)
    dead = (n == 0).all(1)
    dot = lambda x, y: (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]
    best = torch.full((p.shape[0],), float("inf"), device=p.device, dtype=torch.float64)
    arg = torch.full((p.shape[0],), -1, device=p.device, dtype=torch.int64)
    for q0 in range(0, p.shape[0], q_chunk):
        P = p[q0:q0 + q_chunk, None, :]
        for f0 in range(0, t.shape[0], f_chunk):
            a, b, c = A[None, f0:f0 + f_chunk], B[None, f0:f0 + f_chunk], C[None, f0:f0 + f_chunk]
            eab, eac = b - a, c - a
            ap, bp, cp = P - a, P - b, P - c
            d1, d2, d3, d4, d5, d6 = dot(eab, ap), dot(eac, ap), dot(eab, bp), dot(eac, bp), dot(eab, cp), dot(eac, cp)
            vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
            one, zero = torch.ones_like(d1), torch.zeros_like(d1)
            s_ab, w_ac, w_bc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
            g = 1.0 / ((va + vb) + vc)
            s_f, w_f = vb * g, vc * g
            rules = [((d1 <= 0) & (d2 <= 0), (one, zero, zero)), ((d3 >= 0) & (d4 <= d3), (zero, one, zero)),
                     ((vc <= 0) & (d1 >= 0) & (d3 <= 0), (1.0 - s_ab, s_ab, zero)), ((d6 >= 0) & (d5 <= d6), (zero, zero, one)),
                     ((vb <= 0) & (d2 >= 0) & (d6 <= 0), (1.0 - w_ac, zero, w_ac)),
                     ((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), (zero, 1.0 - w_bc, w_bc))]
            bc = [(1.0 - s_f) - w_f, s_f, w_f]
            for cond, val in reversed(rules):
                bc = [torch.where(cond, val[k], bc[k]) for k in range(3)]
            e = P - ((bc[0][..., None] * a + bc[1][..., None] * b) + bc[2][..., None] * c)
            dd = dot(e, e)
            dd = torch.where(dead[None, f0:f0 + f_chunk] | torch.isnan(dd), torch.full_like(dd, float("inf")), dd)
            m, k = dd.min(1)                                   # (the first minimum of the block)
            k = torch.where(dd == m[:, None], torch.arange(dd.shape[1], device=p.device)[None], dd.shape[1]).min(1).values + f0
            better = m < best[q0:q0 + q_chunk]                 # blocks ascend: a tie keeps the earlier, lower index
            best[q0:q0 + q_chunk] = torch.where(better, m, best[q0:q0 + q_chunk])
            arg[q0:q0 + q_chunk] = torch.where(better, k, arg[q0:q0 + q_chunk])
    return arg, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--divisor", type=int, default=64)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--baseline", type=int, default=4096, help="queries of the brute-force baseline (0: none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    v, t = mesh.extract_geometry([-1, -1, -1], [1, 1, 1], args.res, 0.0, ellipsoid, dev)
    v = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev)
    t = torch.from_numpy(t).to(dev)
    c = ((torch.sin(v * 40.0) * 0.5 + 0.5) * 255.0).round().clamp(0, 255).to(torch.uint8).contiguous()       # stripes 0.16 wide: finer than a 1/64 cell
    sv, st, _ = rig.simplify_mesh(v, t, c, args.divisor)
    rec = dict(res=args.res, divisor=args.divisor, size=args.size, dense_vertices=int(v.shape[0]), dense_triangles=int(t.shape[0]),
               simple_vertices=int(sv.shape[0]), simple_triangles=int(st.shape[0]))
    bake.closest_on_mesh(v[:4096].double(), v, t)                      # warm-up: the library's code objects, torch's sort and allocator
    torch.cuda.synchronize()
    stats = {}
    t0 = time.perf_counter()
    uv, image = bake.bake_texture(sv, st, v, t, c, args.size, stats=stats)
    rec["bake_seconds"] = time.perf_counter() - t0
    rec.update(stats)
    rec["owned_fraction"] = stats["texels"] / float(args.size) ** 2
    if args.baseline:
        G, P = bake.atlas_cells(st.shape[0], args.size)
        _, owner = bake.atlas_layout(st.shape[0], args.size)
        texels = np.flatnonzero(owner.reshape(-1) >= 0)
        texels = np.random.RandomState(0).choice(texels, min(args.baseline, len(texels)), replace=False).astype(np.int32)
        tex_d = torch.from_numpy(texels).to(dev)
        pts = torch.empty(len(texels), 3, device=dev, dtype=torch.float64)
        L.call("avc_bake_texel_points", tex_d, len(texels), args.size, P, G, sv, sv.shape[0], st, st.shape[0], pts)
        grid = bake.build_grid(v, t)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tri, _, d2 = bake.query_grid(pts, v, t, grid)
        torch.cuda.synchronize()
        rec["baseline_queries"], rec["kernel_seconds_on_them"] = len(texels), time.perf_counter() - t0
        t0 = time.perf_counter()
        arg, best = brute_force(pts, v, t)
        torch.cuda.synchronize()
        rec["brute_force_seconds"] = time.perf_counter() - t0
        rec["brute_force_seconds_per_million_queries"] = rec["brute_force_seconds"] / len(texels) * 1e6
        rec["brute_force_agrees_on"] = int(((arg == tri.long()) & (best == d2)).sum())
    print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
