"""Time the textured render against the grey one: PoseOptimizer's 5 views at S = 256 of an SMPL-sized mesh (the template of
tests/golden/smpl_views.npz: 6 890 vertices, 13 776 faces, random 8^3 cubes), forward and forward + backward, grey and RGB in one process, and
the CLIP ViT-B/32 image pass of the same 5 views beside them (random weights: the time does not depend on them).  Prints one line per
measurement (median and minimum of --reps timed repetitions after --warmup untimed ones, HIP events around each repetition) and a JSON line;
profiles/texture_render.md records a run.

    python scripts/texture_render_time.py [--reps 50] [--warmup 10] [--size 256]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args(argv)
    from avatarclip_amd import animate as A
    from avatarclip_amd import clip_score, clip_vit
    from avatarclip_amd import mesh_render as M
    from avatarclip_amd.shapegen_render import get_points_from_angles
    from oracle import clip_vit_oracle as C
    dev = torch.device("cuda")
    z = np.load(os.path.join(ROOT, "tests", "golden", "smpl_views.npz"))
    v, f = z["mesh_v"].astype(np.float32), z["mesh_f"].astype(np.int64)
    rs = np.random.RandomState(0)
    tex = torch.from_numpy(rs.uniform(0, 1, (len(f), 8, 8, 8, 3)).astype(np.float32)).to(dev)
    eyes = [get_points_from_angles(A.CAMERA_DISTANCE, 0.1 * i, a).astype(np.float32) for i, a in enumerate(A.DEFAULT_ANGLES)]
    dirs = [(-e / np.linalg.norm(e)).astype(np.float32) for e in eyes]
    S, n = args.size, len(eyes)
    vw = torch.from_numpy(v).to(dev)[None].requires_grad_(True)
    g1 = torch.randn(n, S, S, device=dev)
    g3 = torch.randn(n, 3, S, S, device=dev)
    perceptor = clip_vit.ClipVisionB32(C.random_state_dict(0), dev)

    def grey(backward):
        img = M.render_grey_batch(vw, f, eyes, dirs, image_size=S)
        if backward:
            vw.grad = None
            img.backward(g1)

    def rgb(backward):
        img = M.render_rgb_batch(vw, f, tex, eyes, dirs, image_size=S)
        if backward:
            vw.grad = None
            img.backward(g3)

    with torch.no_grad():
        images = M.render_rgb_batch(vw.detach(), f, tex, eyes, dirs, image_size=S)
    out = {"views": n, "S": S, "faces": int(len(f)), "reps": args.reps}
    for name, fn in (("grey forward", lambda: grey(False)), ("grey forward+backward", lambda: grey(True)), ("rgb forward", lambda: rgb(False)),
                     ("rgb forward+backward", lambda: rgb(True)),
                     ("vit forward", lambda: clip_score.render_embedding(perceptor, images))):
        with torch.set_grad_enabled("backward" in name):
            med, lo = timed(fn, args.reps, args.warmup)
        out[name] = {"median_ms": round(med, 4), "min_ms": round(lo, 4)}
        print("%-24s median %8.3f ms   min %8.3f ms" % (name, med, lo))
    # the launches alone, without the wrapper's torch (rot_mat, face light, camera upload, projection Jacobian): the rasteriser's own share
    from avatarclip_amd import lib as L
    from avatarclip_amd.smpl_prior import camera_frame, face_light
    faces2, fi, vf_ptr, vf_ent = M._topology(f, len(v), dev)
    vr = (vw.detach() @ torch.tensor(M.ROT_MAT, device=dev)).repeat(n, 1, 1).contiguous()
    lt = face_light(vr[0], fi)[None].repeat(n, 1).contiguous()
    cam = torch.from_numpy(np.stack([camera_frame(e, d) for e, d in zip(eyes, dirs)])).to(dev)
    F2, V = faces2.shape[0], len(v)
    ndc, fidx = torch.empty(n, V, 3, device=dev), torch.empty(n, 2 * S, 2 * S, dtype=torch.int32, device=dev)
    im1, im3, unlit = torch.empty(n, S, S, device=dev), torch.empty(n, S, S, 3, device=dev), torch.empty(n, 2 * S, 2 * S, 3, device=dev)
    scratch = torch.full((n * L.load().avc_rasterize_scratch_bytes(F2, 2 * S),), 255, dtype=torch.uint8, device=dev)
    fg, gn, gl = torch.empty(n, F2, 6, device=dev), torch.empty(n, V, 3, device=dev), torch.empty(n, F2, device=dev)
    width = float(np.tan(np.deg2rad(M.VIEWING_ANGLE)))
    g3c = g3.permute(0, 2, 3, 1).contiguous()
    kernels = (
        ("grey save kernels", lambda: L.call("avc_rasterize_mesh_save", vr, n, V, faces2, F2, cam, width, lt, S, M.NEAR, M.FAR, ndc, im1, fidx, scratch)),
        ("rgb save kernels", lambda: L.call("avc_rasterize_mesh_tex_save", vr, n, V, faces2, F2, cam, width, lt, tex, len(f), 8, 1e-4, S, M.NEAR, M.FAR, ndc,
                                            im3, unlit, fidx, scratch)),
        ("grey grad kernels", lambda: L.call("avc_rasterize_mesh_grad", g1, ndc, n, V, faces2, F2, lt, fidx, S, 1e-4, vf_ptr, vf_ent, fg, gn, gl)),
        ("rgb grad kernels", lambda: L.call("avc_rasterize_mesh_tex_grad", g3c, ndc, n, V, faces2, F2, lt, unlit, fidx, S, 1e-4, vf_ptr, vf_ent, fg, gn, gl)))
    for name, fn in kernels:
        med, lo = timed(fn, args.reps, args.warmup)
        out[name] = {"median_ms": round(med, 4), "min_ms": round(lo, 4)}
        print("%-24s median %8.3f ms   min %8.3f ms" % (name, med, lo))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
