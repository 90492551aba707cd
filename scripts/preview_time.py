"""Frame times of the preview renderer (avatarclip_amd/preview.py, csrc/avc_preview.hip): a synthetic avatar mesh of about 1 M triangles
(marching cubes of scripts/drive_time.avatar_field) at 512^2, ss = 2, N = 36 turn-table views, and an SMPL-sized mesh (a subdivided
icosahedron cut to 13 776 faces) at 512^2, ss = 2 and ss = 1.  Per case: ms per frame of the whole render_frames call (host set-up, the
three launches per chunk, no device -> host copy), and the device time of each kernel from torch.profiler.  Medians of --reps
synchronised runs after one warm-up.  There is no number to compare with: the reference's pyrender path does not run here.
The close-up leg (csrc/avc_preview_clip.hip) renders the SAME large mesh as a --focus head turn-table at 512^2, ss = 2, once with
clip=True and once with clip=False (the same cameras; what the renderer did before the clipper: such faces are dropped), and counts the
faces per frame that go through the clipper.
    python scripts/preview_time.py [--res 216] [--reps 5] [--out profiles/r12_preview_time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from avatarclip_amd import lib as L  # noqa: E402
from avatarclip_amd import mesh, preview  # noqa: E402
from drive_time import avatar_field, timed  # noqa: E402
from rig_time import kernel_times  # noqa: E402
from tests import preview_scenes as PS  # noqa: E402


def case(name, v, t, c, size, ss, views, reps):
    eyes, ats, near, far = preview.frame_cameras(v, views, 10.0, "y", 40.0, 0.05)
    fn = lambda: preview.render_frames(v, t, c, eyes, ats, up="y", fov=40.0, image_size=size, ss=ss, near=near, far=far)
    fn()
    ms, img = timed(fn, reps)
    rec = dict(case=name, vertices=int(v.shape[0]), triangles=int(t.shape[0]), size=size, ss=ss, views=views, ms_per_call=ms, ms_per_frame=ms / views,
               covered_fraction=float((img != 255).any(-1).float().mean()))
    try:
        rec["kernels_us_per_call"] = kernel_times(fn)
    except Exception as e:       # the profiler is a convenience here: the frame times above do not depend on it
        rec["kernels_us_per_call"] = "profiler unavailable: %s" % e
    return rec


def clipper_faces(v, t, eyes, ats, near, far, raster):
    """faces per frame with an invalid corner (they go through the clipper), from avc_preview_project's own output"""
    import math
    cams = torch.from_numpy(preview.look_frames(eyes, ats, "y")).to(v.device)
    n, V = cams.shape[0], v.shape[0]
    proj = torch.empty(n, V, 4, device=v.device, dtype=torch.int32)
    L.call("avc_preview_project", v.expand(n, -1, -1).contiguous(), n, V, cams, math.tan(math.radians(40.0) * 0.5), near, far, raster, proj)
    bad = proj[:, :, 2] < 0
    return bad[:, t.long()].any(-1).sum(1).cpu().tolist()


def close_up(name, v, t, c, size, ss, views, reps):
    eyes, ats, near, far = preview.frame_cameras(v, views, 10.0, "y", 40.0, 0.05, focus=preview.FOCUS["head"])
    per_frame = clipper_faces(v, t, eyes, ats, near, far, size * ss)
    recs = []
    for clip in (True, False):
        fn = lambda: preview.render_frames(v, t, c, eyes, ats, up="y", fov=40.0, image_size=size, ss=ss, near=near, far=far, clip=clip)
        fn()
        ms, img = timed(fn, reps)
        rec = dict(case="%s_head_clip_%s" % (name, "on" if clip else "off"), vertices=int(v.shape[0]), triangles=int(t.shape[0]), size=size, ss=ss,
                   views=views, ms_per_call=ms, ms_per_frame=ms / views, covered_fraction=float((img != 255).any(-1).float().mean()),
                   clipper_faces_per_frame=dict(min=min(per_frame), median=float(np.median(per_frame)), max=max(per_frame)))
        try:
            rec["kernels_us_per_call"] = kernel_times(fn)
        except Exception as e:
            rec["kernels_us_per_call"] = "profiler unavailable: %s" % e
        recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=216, help="marching-cubes grid of the large mesh (216^3: about 1 M triangles)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda")
    recs = [dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=str(torch.version.hip))]
    print(json.dumps(recs[0]), flush=True)
    v, t = mesh.marching_cubes(avatar_field(args.res, dev), 0.0)
    v = (v / (args.res - 1.0) * 2.0 - 1.0).contiguous()
    c = ((v + 1) * 127.5).clamp(0, 255).to(torch.uint8).contiguous()
    sv, st, sc = PS.icosphere(5)                                       # 20 480 faces; the first 13 776 (SMPL's count) are kept
    st = st[:13776]
    cases = [("avatar_%d" % args.res, v, t, c, 512, 2, 36), ("smpl_sized", torch.from_numpy(sv).to(dev), torch.from_numpy(st).to(dev), torch.from_numpy(sc).to(dev), 512, 2, 36),
             ("smpl_sized", torch.from_numpy(sv).to(dev), torch.from_numpy(st).to(dev), torch.from_numpy(sc).to(dev), 512, 1, 36)]
    for a in cases:
        rec = case(*a, reps=args.reps)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    for rec in close_up("avatar_%d" % args.res, v, t, c, 512, 2, 36, args.reps):
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
