"""Generates tests/golden/corrdense_*.npz from the REFERENCE's own correlation kernels: the dense stride-1 configuration
Correlation(md, 1, md, 1, 1) that PWC-Net calls (csrc/correlation_dense.hip).

Run in the dev container only (needs the reference checkout):
    make -C oracle ref && python tests/golden/make_golden_corr_dense.py

As make_golden.py: oracle/_ref/libfn2_ref.so is the reference's device code under the CPU SIMT shim, launched with its own grid
and block geometry; inputs are seeded and stored next to everything the reference produced.  float32 only (the wrapper runs
float32 and float64).  The prefix is corrdense_, not corr_: conftest.golden_files("corr") globs corr_*.npz.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.oracle import Oracle  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 20261016

# (name, B, C, H, W, md)
CASES = [("md4_c34_18x24", 1, 34, 18, 24, 4), ("md4_c196_6x8", 1, 196, 6, 8, 4), ("md3_c32_17x22", 1, 32, 17, 22, 3)]


def main():
    ref = Oracle(ref=True)
    rng = np.random.default_rng(SEED)
    for (name, B, C, H, W, md) in CASES:
        in1 = rng.standard_normal((B, C, H, W)).astype(np.float32)
        in2 = rng.standard_normal((B, C, H, W)).astype(np.float32)
        out = ref.corr_fwd(in1, in2, md, 1, md, 1, 1)
        gout = rng.standard_normal(out.shape).astype(np.float32)
        g1, g2 = ref.corr_bwd(in1, in2, gout, md, 1, md, 1, 1)
        path = os.path.join(OUT, f"corrdense_{name}.npz")
        np.savez_compressed(path, in1=in1, in2=in2, out=out, gout=gout, g1=g1, g2=g2, params=np.array([md, 1, md, 1, 1], np.int32))
        print("corrdense", name, out.shape, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
