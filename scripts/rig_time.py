"""Stage times of the rig step (avatarclip_amd/rig.py) at production size: avatar meshes from marching cubes at 256^3 and 512^3
(scripts/drive_time.avatar_field), K = 6890 template vertices, T = 60 frames.  Stages: the vertex clustering (whole call, and its HIP
kernels one by one from torch.profiler), the same clustering restated in numpy on this machine's CPU, nearest template vertex, skin
packing, rotations -> quaternions, and the whole step with its device -> host copies and file writes; the sizes of the .glb and of the
.pc2 drive writes for the same motion.  Medians of --reps synchronised runs.
    python scripts/rig_time.py [--res 256 512] [--reps 5] [--out profiles/r09_rig_time.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from avatarclip_amd import drive, mesh, rig  # noqa: E402
from drive_time import avatar_field, timed  # noqa: E402
from tests import drive_standins as S  # noqa: E402
from tests import rig_standins as RS  # noqa: E402


def kernel_times(fn):
    """device time of every kernel of one call of fn, microseconds, by name (torch.profiler)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        us = getattr(e, "device_time_total", None)
        us = getattr(e, "cuda_time_total", 0.0) if us is None else us
        if us:
            out[e.key[:90]] = round(float(us), 1)
    return out


def run(res, reps, T=60, K=6890):
    dev = torch.device("cuda")
    v, t = mesh.marching_cubes(avatar_field(res, dev), 0.0)
    v = (v / (res - 1.0) * 2.0 - 1.0).contiguous()
    c = ((v + 1) * 127.5).clamp(0, 255).to(torch.uint8).contiguous()
    rec = dict(res=res, mesh_vertices=int(v.shape[0]), mesh_triangles=int(t.shape[0]), K=K, T=T, voxel_divisor=256)
    rec["simplify_ms"], (sv, st, sc) = timed(lambda: rig.simplify_mesh(v, t, c, 256), reps)
    rec["M"], rec["triangles_out"] = int(sv.shape[0]), int(st.shape[0])
    try:
        rec["simplify_kernels_us"] = kernel_times(lambda: rig.simplify_mesh(v, t, c, 256))
    except Exception as e:       # the profiler is a convenience here: the stage times above do not depend on it
        rec["simplify_kernels_us"] = "profiler unavailable: %s" % e
    vn, tn, cn = v.cpu().numpy(), t.cpu().numpy(), c.cpu().numpy()
    t0 = time.perf_counter()
    rv, rt, rcol, _ = RS.restated_simplify(vn, tn, cn, 256)
    rec["restated_simplify_cpu_ms"] = (time.perf_counter() - t0) * 1e3
    rec["bit_identical_to_restatement"] = bool(np.array_equal(sv.cpu().numpy(), rv) and np.array_equal(st.cpu().numpy(), rt) and
                                               np.array_equal(sc.cpu().numpy(), rcol))
    a = {k: (x.to(dev) if k != "parents" else x) for k, x in S.template_arrays(K=K).items()}
    stand = np.random.RandomState(0).randn(72).astype(np.float32) * 0.2
    template, pose_rot = drive.load_template_smpl(a, stand)
    rot_v = torch.from_numpy(drive.rotate_vertices(sv.cpu().numpy())).to(dev)
    rec["nearest_ms"], nearest = timed(lambda: drive.find_nearest_ind(rot_v, template), reps)
    rec["skin_pack_ms"], (jn, wn, _) = timed(lambda: rig.skin_pack(a["lbs_weights"], nearest), reps)
    rec["skin_sets"] = int(jn.shape[0])
    rot = drive.read_pose_my(S.motion(T)).to(dev)
    rec["rot_to_quat_ms"], _ = timed(lambda: rig.rot_to_quat(rot), reps)
    with tempfile.TemporaryDirectory() as d:
        np.save(os.path.join(d, "m.npy"), S.motion(T))
        rec["whole_step_ms"], (glb, npz) = timed(lambda: rig.build_rig((vn, tn, cn), a, stand, d, motion=os.path.join(d, "m.npy")), 1)
        rec["glb_bytes"], rec["npz_bytes"] = os.path.getsize(glb), os.path.getsize(npz)
        t0 = time.perf_counter()
        rig.read_glb(glb)
        rec["read_glb_ms"] = (time.perf_counter() - t0) * 1e3
    rec["host_and_files_ms"] = rec["whole_step_ms"] - rec["simplify_ms"] - rec["nearest_ms"] - rec["skin_pack_ms"] - rec["rot_to_quat_ms"]
    rec["pc2_bytes_same_motion_unsimplified"] = 32 + T * int(v.shape[0]) * 12
    rec["animation_bytes"] = T * 4 + T * 24 * 16
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
