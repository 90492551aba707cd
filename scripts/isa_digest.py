#!/usr/bin/env python
"""SHA-256 of the gfx950 assembly of every csrc/*.hip, compiled with the flags of avatarclip_amd.build (no GPU needed).

    python scripts/isa_digest.py [--keep DIR] [FILE.hip ...]

Two checkouts that print the same table ship the same device code: run it before and after a refactor of the kernels and compare.
-fuse-cuid=none makes the output reproducible (otherwise the __hip_cuid_* symbol differs between two compiles of one source).
--keep DIR leaves the .s files in DIR for `diff`."""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avatarclip_amd import build as B  # noqa: E402


def digest(src, outdir):
    out = os.path.join(outdir, src.replace(".hip", ".s"))
    cmd = [B._hipcc()] + B.FLAGS + B.SOURCE_FLAGS.get(src, []) + ["--cuda-device-only", "-fuse-cuid=none", "-S", os.path.join(B.CSRC, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), r.stderr[-4000:]))
    with open(out, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--keep", metavar="DIR", help="leave the .s files here")
    ap.add_argument("sources", nargs="*", help="default: build.SOURCES and the ring source")
    a = ap.parse_args()
    srcs = a.sources or B.SOURCES + [B.RING_SOURCE]
    B._gen_offsets()
    with tempfile.TemporaryDirectory() as tmp:
        outdir = a.keep or tmp
        os.makedirs(outdir, exist_ok=True)
        with ThreadPoolExecutor(max_workers=min(len(srcs), 16)) as ex:
            for s, d in zip(srcs, ex.map(lambda s: digest(s, outdir), srcs)):
                print("%-24s %s" % (s, d))


if __name__ == "__main__":
    main()
