"""Stage times of the drive step (avatarclip_amd/drive.py) at production size: K = 6890 template vertices, avatar meshes from marching cubes
at 256^3 and 512^3 (avatar_field), T = 60 frames.  Stages: islands (components + island choice + compaction), nearest template vertex, per-template
transforms (stand-pose inverses + 60 frames), skinning (the unposing + all 60 frames in one call, with its HBM write rate), and the
device -> host hand-off + .pc2 write.  Medians of --reps synchronised runs.
    python scripts/drive_time.py [--res 256 512] [--reps 5] [--out profiles/r08_drive_time.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from avatarclip_amd import drive, mesh  # noqa: E402
from tests import drive_standins as S  # noqa: E402

COPY_TBS = 6.29     # measured float4 copy rate of one MI355X (MI355X_MICROARCH.md)


def body_field(res, dev):
    """u = -sdf of a standing figure + detached blobs (tests/drive_standins.body_sdf) on a res^3 grid over [-1, 1]^3, on the device"""
    g = torch.linspace(-1, 1, res, device=dev)
    out = torch.empty(res, res, res, device=dev)
    caps = [((0, -0.05, 0), (0, 0.35, 0), 0.17), ((0, 0.38, 0), (0, 0.5, 0), 0.05), ((-0.15, 0.33, 0), (-0.55, 0.1, 0), 0.05),
            ((0.15, 0.33, 0), (0.55, 0.1, 0), 0.05), ((-0.09, -0.1, 0), (-0.14, -0.85, 0), 0.07), ((0.09, -0.1, 0), (0.14, -0.85, 0), 0.07),
            ((0, 0.58, 0), (0, 0.58, 0), 0.12), ((0.7, 0.7, 0.3), (0.7, 0.7, 0.3), 0.1), ((-0.7, -0.6, -0.4), (-0.7, -0.6, -0.4), 0.08)]
    for x0 in range(0, res, 32):
        xs = g[x0:x0 + 32]
        p = torch.stack(torch.meshgrid(xs, g, g, indexing="ij"), -1)
        d = None
        for a, b, r in caps:
            a, b = torch.tensor(a, device=dev), torch.tensor(b, device=dev)
            ab = b - a
            t = ((p - a) @ ab / (ab @ ab).clamp_min(1e-12)).clamp(0, 1)
            di = (p - (a + t[..., None] * ab)).norm(dim=-1) - r
            d = di if d is None else torch.minimum(d, di)
        out[x0:x0 + len(xs)] = -d
    return out


def avatar_field(res, dev, f=50.0):
    """the figure dilated by 0.2 and filled with a gyroid lattice of period 2 pi / f: a surface with as many vertices as a validate_mesh
    avatar has at these resolutions (0.7 M at 256^3, ~2.9 M at 512^3; a real one: ~0.6 M / 2.6 M, profiles/HISTORY.md), islands included"""
    u = body_field(res, dev) + 0.2
    g = torch.linspace(-1, 1, res, device=dev)
    for x0 in range(0, res, 32):
        X, Y, Z = torch.meshgrid(g[x0:x0 + 32] * f, g * f, g * f, indexing="ij")
        gy = torch.sin(X) * torch.cos(Y) + torch.sin(Y) * torch.cos(Z) + torch.sin(Z) * torch.cos(X)
        u[x0:x0 + 32] = torch.minimum(u[x0:x0 + 32], gy * 0.05 + 0.02)
    return u


def timed(fn, reps):
    ts, r = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, r


def run(res, reps, T=60, K=6890):
    dev = torch.device("cuda")
    v, t = mesh.marching_cubes(avatar_field(res, dev), 0.0)
    v = (v / (res - 1.0) * 2.0 - 1.0).contiguous()
    c = torch.full((v.shape[0], 4), 200, device=dev, dtype=torch.uint8)
    v = torch.from_numpy(drive.rotate_vertices(v.cpu().numpy())).to(dev)
    a = {k: (x.to(dev) if k != "parents" else x) for k, x in S.template_arrays(K=K).items()}
    rot = drive.read_pose_my(S.motion(T)).to(dev)
    stand = np.random.RandomState(0).randn(72).astype(np.float32) * 0.2
    rec = dict(res=res, mesh_vertices=int(v.shape[0]), mesh_triangles=int(t.shape[0]), K=K, T=T)
    rec["islands_ms"], (vc, tc, cc) = timed(lambda: drive.cleanup_mesh(v, t, c), reps)
    M = int(vc.shape[0])
    rec["M"] = M
    template, pose_rot = drive.load_template_smpl(a, stand)
    rec["nearest_ms"], nearest = timed(lambda: drive.find_nearest_ind(vc, template), reps)
    rec["transforms_ms"], (inv, xf) = timed(lambda: (drive.rows3(torch.linalg.inv(drive.template_transforms(a, pose_rot))),
                                                    drive.rows3(drive.template_transforms(a, rot))), reps)
    tpose = drive.skin_apply(inv, nearest, vc)[0]
    out = torch.empty(T, M, 3, device=dev)
    rec["skin_unpose_ms"], _ = timed(lambda: drive.skin_apply(inv, nearest, vc), reps)
    rec["skin_frames_ms"], _ = timed(lambda: drive.skin_apply(xf, nearest, tpose, out=out), reps)
    wbytes = T * M * 12
    rec["skin_frames_write_TBs"] = wbytes / (rec["skin_frames_ms"] * 1e-3) / 1e12
    rec["skin_frames_fraction_of_copy_rate"] = rec["skin_frames_write_TBs"] / COPY_TBS
    del out
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "m.pc2")
        rec["d2h_write_ms"], _ = timed(lambda: drive.write_pc2(p, drive.posed_frames(a, tpose, nearest, rot), vcount=M, num_samples=T), 1)
        rec["pc2_bytes"] = os.path.getsize(p)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    recs = []
    for r in args.res:
        rec = run(r, args.reps)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
