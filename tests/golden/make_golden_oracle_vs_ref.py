"""Generates tests/golden/oracle_vs_ref_calls.npz: the reference kernels' answers (oracle/_ref/libfn2_ref.so, the reference's
own device code under the CPU SIMT shim) to every call tests/test_oracle_vs_ref.py makes, so that those tests also run where
oracle/_ref/ cannot be built.  Dev container only (after `make -C oracle ref`):
    python tests/golden/make_golden_oracle_vs_ref.py"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(OUT)
sys.path[:0] = [TESTS, os.path.dirname(TESTS)]
from oracle.oracle import Oracle  # noqa: E402
from ref_recording import Recorder  # noqa: E402
import test_oracle_vs_ref as t  # noqa: E402


def main():
    orc, rec = Oracle(), Recorder(Oracle(ref=True))
    for case in t.CASES:                                   # the parametrisations of tests/test_oracle_vs_ref.py
        for dt in (np.float32, np.float64):
            t.test_corr_live(orc, rec, case, dt)
    t.test_resample_live(orc, rec)
    for ks in (2, 3):
        t.test_resample_kernel_size_live(orc, rec, ks)
    for dt in (np.float32, np.float64):
        t.test_chnorm_live(orc, rec, dt)
    rec.save(os.path.join(OUT, "oracle_vs_ref_calls.npz"))
    print("recorded", len(rec.calls), "arrays")


if __name__ == "__main__":
    main()
