"""In-tree build of libavc.so (hipcc, gfx950).  The .so is git-ignored but travels with the gpurun snapshot."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, os.environ.get("AVC_LIB_NAME", "libavc.so"))
SOURCES = ["avc_core.hip", "avc_mlp_fwd.hip", "avc_mlp_bwd.hip", "avc_wgrad.hip", "avc_rays.hip", "avc_vit.hip", "avc_vit_attn.hip", "avc_vit_gemm.hip", "avc_mcubes.hip", "avc_raster.hip", "avc_raster_grad.hip", "avc_raster_tex.hip", "avc_params.hip", "avc_glue.hip", "avc_drive.hip", "avc_rig.hip", "avc_preview.hip", "avc_smpl.hip", "avc_smpl_grad.hip", "avc_codebook.hip", "avc_bake.hip", "avc_preview_clip.hip"]
ABI_HEADER = os.path.join("..", "..", "include", "avc.h")          # the one declaration of the C ABI (lib.py parses it), relative to CSRC
TEXTURE_HEADER = "avc_texture.h"                                   # the textured-render entry points (lib.py parses it too), in CSRC: include/ holds avc.h alone
CODEBOOK_HEADER = "avc_codebook.h"                                 # the k-means entry points (csrc/avc_codebook.hip), declared beside their source as well
PREVIEW_CLIP_HEADER = "avc_preview_clip.h"                         # the preview's clipping entry points (csrc/avc_preview_clip.hip), declared beside their source
BAKE_HEADER = "avc_bake.h"                                         # the texture bake's entry points (csrc/avc_bake.hip) and the preview's textured shade, likewise
HEADERS = ["avc_common.h", "avc_stage.h", "avc_mlp.h", "avc_bwd_body.h", "avc_offsets_gen.h", "avc_raster.h", "avc_raster_grad.h", "avc_smpl.h", "avc_vit.h", ABI_HEADER,
           TEXTURE_HEADER, CODEBOOK_HEADER, BAKE_HEADER, "avc_preview.h", PREVIEW_CLIP_HEADER]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-comment"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def _gen_offsets():
    """csrc/avc_offsets_gen.h = the packed-blob offsets of packing.py as compile-time constants (scripts/gen_offsets.py)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_offsets", os.path.join(os.path.dirname(HERE), "scripts", "gen_offsets.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main()


def build(force: bool = False, verbose: bool = False) -> str:
    """libavc.so (or $AVC_LIB_NAME)"""
    _gen_offsets()
    srcs = [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs, jobs = [], []
    for s in srcs:
        src = os.path.join(CSRC, s)
        obj = os.path.join(CSRC, s.replace(".hip", os.environ.get("AVC_OBJ_SUFFIX", "") + ".o"))
        objs.append(obj)
        if force or _stale(obj, [src] + hdrs):
            jobs.append([_hipcc()] + FLAGS + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), r.stderr[-4000:]))

    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 4)) as ex:
            list(ex.map(run, jobs))
    if jobs or force or _stale(LIB, objs):
        tmp = "%s.%d.tmp" % (LIB, os.getpid())       # concurrent builders: nobody ever maps a half-written library
        run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs)
        os.replace(tmp, LIB)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
