"""smpl_lbs.pose_hip (csrc/avc_smpl.hip: two launches) against smpl_lbs.lbs under no_grad (torch: about a hundred launches), on the same
device and the same inputs at SMPL's real sizes (V = 6890, tests/drive_standins.template_arrays(K=6890)), T = 1, 60 and 1024; and the whole
motion.gif of 60 frames at 512^2 as animate.run(preview=True) writes it.  The two posing paths are timed in ONE process, ALTERNATED: --rounds
rounds of (--inner calls of one, a synchronise, --inner calls of the other, a synchronise), host clock, after a warm-up of both; per path
the median over the rounds of the time per call and the spread (min .. max).  The device time of every kernel of one call of each comes
from torch.profiler in a pass of its own.  Nothing is fixed in advance: the figures go to profiles/r14_pose_preview.md.
    python scripts/pose_preview_time.py [--rounds 9] [--inner 20] [--out profiles/r14_pose_preview_time.json]"""
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
from avatarclip_amd import preview, smpl_lbs  # noqa: E402
from rig_time import kernel_times  # noqa: E402
from tests import drive_standins as S  # noqa: E402


def lbs_no_grad(a, pose):
    """what AnimateContext.posed_vertices does, without a gradient"""
    with torch.no_grad():
        T = pose.shape[0]
        rot = smpl_lbs.batch_rodrigues(pose.reshape(-1, 3)).reshape(T, 24, 3, 3)
        v, _ = smpl_lbs.lbs(a["v_template"][None].expand(T, -1, -1), rot, a["posedirs"], a["J_regressor"], a["parents"], a["lbs_weights"])
        return v


def per_call_ms(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def alternated(fa, fb, rounds, inner):
    for _ in range(3):
        fa()
        fb()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(per_call_ms(fa, inner))
        tb.append(per_call_ms(fb, inner))
    stat = lambda ts: dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)))
    return stat(ta), stat(tb)


def body_arrays(dev):
    """an SMPL-sized body that holds together under a pose: the template mesh of tests/golden/smpl_views.npz, smooth distance weights
    around 24 of its vertices, drive_standins' pose blend shapes"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "smpl_views.npz"))
    v, f = z["mesh_v"].astype(np.float32), z["mesh_f"].astype(np.int32)
    a = S.template_arrays(K=len(v))
    rs = np.random.RandomState(0)
    d = np.linalg.norm(v[:, None] - v[rs.choice(len(v), 24, replace=False)][None], axis=-1)
    w = np.exp(-(d / 0.15) ** 2) + 1e-6
    jreg = np.exp(-(d.T / 0.05) ** 2) + 1e-9
    a.update(v_template=torch.from_numpy(v), lbs_weights=torch.from_numpy((w / w.sum(1, keepdims=True)).astype(np.float32)),
             J_regressor=torch.from_numpy((jreg / jreg.sum(1, keepdims=True)).astype(np.float32)))
    a = {k: (x.to(dev) if k != "parents" else x) for k, x in a.items()}
    a["faces"] = f
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--frames", type=int, nargs="*", default=[1, 60, 1024])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    recs = [dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=str(torch.version.hip), rounds=args.rounds, inner=args.inner)]
    print(json.dumps(recs[0]), flush=True)
    a = {k: (x.to(dev) if k != "parents" else x) for k, x in S.template_arrays(K=6890).items()}
    for T in args.frames:
        pose = torch.from_numpy(S.motion(T)).to(dev).reshape(T, 24, 3)
        hip, ref = lambda: smpl_lbs.pose_hip(a, pose), lambda: lbs_no_grad(a, pose)
        inner = max(2, args.inner // 10) if T > 256 else args.inner
        sh, sr = alternated(hip, ref, args.rounds, inner)
        rec = dict(case="posing", V=6890, T=T, inner=inner, pose_hip=sh, lbs_no_grad=sr, ratio_of_medians=sr["median_ms"] / sh["median_ms"],
                   worst_difference_m=float((hip() - ref()).abs().max()))
        try:
            kh, kr = kernel_times(hip), kernel_times(ref)
            rec["pose_hip_kernels_us"], rec["lbs_distinct_kernels"], rec["lbs_kernels_us_total"] = kh, len(kr), round(sum(kr.values()), 1)
        except Exception as e:       # the profiler is a convenience here: the call times above do not depend on it
            rec["pose_hip_kernels_us"] = "profiler unavailable: %s" % e
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    # the whole motion.gif: 60 poses -> vertices -> one framed camera -> 60 images at 512^2 (ss 2) -> the file
    b = body_arrays(dev)
    motion = S.motion(60)[:, 3:]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "motion.gif")
        stages = {}

        def gif():
            t0 = time.perf_counter()
            v = smpl_lbs.pose_hip(b, torch.from_numpy(preview.body_pose(motion)))
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            eyes, ats, near, far = preview.frame_cameras(v, 1, up="y")
            img = preview.render_frames(v, b["faces"], None, eyes, ats, up="y", image_size=512, near=near, far=far)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            preview.save_frames(img, out)
            t3 = time.perf_counter()
            stages.setdefault("pose_ms", []).append((t1 - t0) * 1e3)
            stages.setdefault("render_ms", []).append((t2 - t1) * 1e3)
            stages.setdefault("encode_and_write_ms", []).append((t3 - t2) * 1e3)
            stages.setdefault("total_ms", []).append((t3 - t0) * 1e3)
        gif()
        stages.clear()
        for _ in range(5):
            gif()
        rec = dict(case="motion.gif", frames=60, size=512, ss=2, bytes=os.path.getsize(out),
                   **{k: dict(median=float(np.median(x)), min=float(min(x)), max=float(max(x))) for k, x in stages.items()})
    print(json.dumps(rec), flush=True)
    recs.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
