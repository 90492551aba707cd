#!/usr/bin/env python
"""SHA-256 of the gfx950 assembly of every csrc/*.hip, compiled with the flags of avatarclip_amd.build (no GPU needed).

    python scripts/isa_digest.py [--keep DIR] [--per-kernel] [FILE.hip ...]

Two checkouts that print the same table ship the same device code: run it before and after a refactor of the kernels and compare.
-fuse-cuid=none makes the output reproducible (otherwise the __hip_cuid_* symbol differs between two compiles of one source).
--keep DIR leaves the .s files in DIR for `diff`.  --per-kernel prints one digest per kernel symbol instead of one per file (the text
from the symbol's .globl / .protected line through its .end_amdhsa_kernel, local labels without the function's ordinal in the file): for a
file that gained or lost a kernel, or was compiled with other flags, it shows which of the kernels both builds have are the same."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avatarclip_amd import build as B  # noqa: E402


def assemble(src, outdir):
    out = os.path.join(outdir, src.replace(".hip", ".s"))
    cmd = [B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-fuse-cuid=none", "-S", os.path.join(B.CSRC, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed: %s\n%s" % (" ".join(cmd), r.stderr[-4000:]))
    with open(out, "rb") as f:
        return f.read()


def kernels(asm):
    """[(symbol, its text)] in file order"""
    text = asm.decode()
    out = []
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)$", text, re.M):
        name = m.group(1)
        start = re.search(r"^\t\.(?:globl|protected)\t%s\b" % re.escape(name), text, re.M).start()
        end = text.index("\t.end_amdhsa_kernel\n", m.end()) + len("\t.end_amdhsa_kernel\n")
        # local labels carry the function's ordinal in the file (.LBB4_11, .Lfunc_end4, BB4_11 in the loop comments): names the assembler drops, not code
        out.append((name, re.sub(r"(?<!\w)(\.L)?(BB|func_begin|func_end)\d+", r"\1\2", text[start:end])))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--keep", metavar="DIR", help="leave the .s files here")
    ap.add_argument("--per-kernel", action="store_true", help="one digest per kernel symbol")
    ap.add_argument("sources", nargs="*", help="default: build.SOURCES")
    a = ap.parse_args()
    srcs = a.sources or B.SOURCES
    B._gen_offsets()
    with tempfile.TemporaryDirectory() as tmp:
        outdir = a.keep or tmp
        os.makedirs(outdir, exist_ok=True)
        with ThreadPoolExecutor(max_workers=min(len(srcs), 16)) as ex:
            for s, asm in zip(srcs, ex.map(lambda s: assemble(s, outdir), srcs)):
                if a.per_kernel:
                    for name, text in kernels(asm):
                        print("%-24s %s %s" % (s, hashlib.sha256(text.encode()).hexdigest(), name))
                else:
                    print("%-24s %s" % (s, hashlib.sha256(asm).hexdigest()))


if __name__ == "__main__":
    main()
