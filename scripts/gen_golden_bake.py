"""tests/golden/bake_sphere.npz: the texture bake's end-to-end case (tests/bake_scenes.py) as the numpy restatement computes it -- the
64 x 32 sphere's float32 vertices, and per owned texel of the 128 x 128 atlas the closest dense triangle, whether that choice is ambiguous
between two palette colours, and the two restated images.  Brute force, some 20 s; tests/test_bake_cpu.py recomputes it.

    python scripts/gen_golden_bake.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from tests import bake_scenes as BS
    inputs = BS.bake_inputs(recorded=False)
    ref = BS.bake_reference(inputs)
    np.savez_compressed(BS.GOLD, v=inputs["dense"][0], tri=ref["tri"].astype(np.int32), image=ref["image"], flat_image=ref["flat_image"],
                        ambiguous=ref["ambiguous"])
    print("%s: %d texels, %d ambiguous (%.2f %%), %d bytes" % (BS.GOLD, len(ref["tri"]), ref["ambiguous"].sum(), 100.0 * ref["ambiguous"].mean(),
                                                             os.path.getsize(BS.GOLD)))


if __name__ == "__main__":
    main()
