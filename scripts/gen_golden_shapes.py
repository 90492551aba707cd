"""Generate tests/golden/neus_shape_<H>_<NMID>_<NCMID>*.npz: one reference render + autograd gradients per scaled-down network shape
(packing.SUPPORTED beyond the two the reference ships), by RUNNING THE REFERENCE'S OWN MODULES as oracle/gen_golden.py does for
neus_full.npz.  Needs the reference tree (oracle/ref_loader.py); TEST INFRASTRUCTURE ONLY.
    python scripts/gen_golden_shapes.py

Per shape: torch.manual_seed(0), geometric init + the weight perturbation of neus_full.npz, variance 0.45; the first 512 rays of the
48 x 48 view of neus_full.npz, 32 + 32 samples, 4 up-sampling steps, injected jitter, cos_anneal 0.3, the random per-ray loss
coefficients of oracle/gen_golden.py: scalar_loss (seed 4).  (512 rays, not fewer: with 96 the colour-branch gradients sat at ReLU-flip
noise above the gradient gate, see oracle/gen_golden.py.)

Only what the tests read is kept: rays, near / far, jitter, z_final, the out_* keys the render statement compares, coef_*, loss,
grad_* and the state dicts -- no per-step up-sampling traces, no out_gradients.  A fixture is written as one or more PARTS of disjoint
keys, neus_shape_<..>.npz, neus_shape_<..>.p1.npz, ..., each below the repository's 1 MiB limit for a committed file (the 256-wide
state dict alone is 1.1 MB); tests/net_shapes_common.py: load_shape_case merges them.
"""
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from avatarclip_amd import packing as PK  # noqa: E402
from oracle import ref_loader  # noqa: E402
from oracle.gen_golden import extract_functions, run_case, sd_np  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
PART_RAW_BYTES = 900 * 1024        # raw bytes per part; float weights barely compress, so a part stays under 1 MiB on disk
KEEP_OUT = ("color_fine", "extra_color_fine", "weight_sum", "weights", "mid_z_vals", "inside_sphere", "gradient_error")
NEW_SHAPES = [sp for _, _, sp in PK.SUPPORTED if (sp.H, sp.NMID, sp.NCMID) not in ((256, 2, 1), (128, 1, 0))]


def confs(spec):
    H = spec.H
    sdf = dict(ref_loader.FULL_SDF, d_out=H + 1, d_hidden=H, n_layers=spec.NMID + 2, skip_in=[spec.NMID + 2])
    col = dict(ref_loader.FULL_COLOR, d_feature=H, d_hidden=H, n_layers=spec.NCMID + 1)
    return sdf, col


def stem(spec):
    return "neus_shape_%d_%d_%d" % (spec.H, spec.NMID, spec.NCMID)


def write_parts(spec, rec):
    for old in glob.glob(os.path.join(GOLD, stem(spec) + "*.npz")):
        os.remove(old)
    parts, cur, size = [], {}, 0
    for k in sorted(rec):
        n = rec[k].nbytes
        assert n <= PART_RAW_BYTES, k
        if cur and size + n > PART_RAW_BYTES:
            parts.append(cur)
            cur, size = {}, 0
        cur[k] = rec[k]
        size += n
    parts.append(cur)
    for i, part in enumerate(parts):
        path = os.path.join(GOLD, stem(spec) + (".npz" if i == 0 else ".p%d.npz" % i))
        np.savez_compressed(path, **part)
        sz = os.path.getsize(path)
        print("  %s %d bytes, %d keys" % (os.path.basename(path), sz, len(part)))
        assert sz < 1024 * 1024, path


def main():
    R = ref_loader.load_reference()
    AG = R.ref_ag
    ds_fns = extract_functions(os.path.join(AG, "models", "dataset.py"), ["gen_rays_pose", "near_far_from_sphere"], "SMPL_Dataset")
    ut_fns = extract_functions(os.path.join(AG, "models", "utils.py"), ["norm_np_arr", "lookat"])
    for f in ut_fns.values():
        f.__globals__.update(ut_fns)
    # the view of neus_full.npz (oracle/gen_golden.py: main)
    NF = 512
    fake_self = type("DS", (), {})()
    fake_self.W = fake_self.H = 48
    f48 = 0.5 * 48 / np.tan(np.pi / 6)
    fake_self.K = torch.from_numpy(np.array([[f48, 0, 24.0], [0, f48, 24.0], [0, 0, 1]]))
    eye = np.array([0.6, 0.4, 1.3], dtype=np.float32)
    pose = torch.from_numpy(ut_fns["lookat"](eye, np.zeros(3, np.float32), np.array([0, 1, 0]))).float()
    o, v = ds_fns["gen_rays_pose"](fake_self, pose, 2)
    ro, rd = o.reshape(-1, 3).float().contiguous(), v.reshape(-1, 3).float().contiguous()
    nearf, farf = ds_fns["near_far_from_sphere"](fake_self, ro, rd)
    ro, rd, nearf, farf = ro[:NF], rd[:NF], nearf[:NF], farf[:NF]
    jitter = torch.rand(NF, 1, generator=torch.Generator().manual_seed(3))

    for spec in NEW_SHAPES:
        print(stem(spec))
        sdf_conf, col_conf = confs(spec)
        assert PK.spec_from_conf(sdf_conf, col_conf) == spec
        torch.manual_seed(0)
        sdf = R.SDFNetwork(**sdf_conf)
        col = R.RenderingNetwork(**col_conf)
        var = R.SingleVarianceNetwork(0.3)
        with torch.no_grad():  # move off the degenerate init so every weight matters (PE columns are 0 at init)
            for p in list(sdf.parameters()) + list(col.parameters()):
                p.add_(torch.randn_like(p) * 0.02 * p.abs().mean().clamp(min=0.05))
            var.variance.fill_(0.45)
        rec = run_case(R, sdf, col, var, 32, 32, 4, ro, rd, nearf, farf, jitter, None, 0.3, seed=4)
        keep = {k: a for k, a in rec.items()
                if k in ("rays_o", "rays_d", "near", "far", "jitter", "bg", "cos_anneal", "z_final", "loss")
                or k.startswith(("coef_", "grad_")) or (k.startswith("out_") and k[4:] in KEEP_OUT)}
        keep.update(sd_np(sdf.state_dict(), "sdf."))
        keep.update(sd_np(col.state_dict(), "col."))
        keep.update(sd_np(var.state_dict(), "var."))
        gn = np.sqrt(sum(float((a.astype(np.float64) ** 2).sum()) for k, a in keep.items() if k.startswith("grad_")))
        for k, a in keep.items():   # the gradient test's 2e-2 allowance is for colour-branch tensors only
            if k.startswith("grad_sdf.") and np.abs(a).max() >= 1e-7:
                assert np.linalg.norm(a.astype(np.float64)) >= 1e-4 * gn, ("an SDF tensor below 1e-4 of the gradient norm", k)
        print("  loss %.6f  |grad| %.4e  weight_sum mean %.3f" % (float(keep["loss"]), gn, float(keep["out_weight_sum"].mean())))
        write_parts(spec, keep)


if __name__ == "__main__":
    main()
