"""Which correlation kernels the dispatcher of libflownet2_hip.so would try for a call, asked on a machine without a GPU:
fn2_debug_correlation_plan (csrc/fn2_debug.h) walks the kernel table of csrc/capi.hip -- the one the entry points walk -- and
returns the candidates in the order FN2_CORR_AUTO tries them, or the code the entry point returns before any launch.  Pointers are
passed as addresses and never dereferenced.  corr_dispatch_cases.py holds the table; tests/test_gpu_corr_dispatch.py and
scripts/corr_dispatch_trace.py run the same calls on the GPU."""
import os
import re

import pytest

from conftest import PKG

import fn2_capi
from corr_dispatch_cases import A4, A8, A16, BACKWARD_AUTO, BF16, DEBUG, EALIGN, EINVAL, F32, F64, FORWARD_AUTO, FORWARD_FORCED, HALF, P20, plan


def test_f64_case_uses_the_backward_channel_group():
    """The f64 rows of the table take C = md::BCG, the smallest channel count the fp64 kernels accept."""
    s = open(os.path.join(PKG, "csrc", "correlation_mfma_f64.hip")).read()
    bck = int(re.search(r"constexpr int BCK = (\d+);", s).group(1))
    bnct = int(re.search(r"constexpr int BNCT = (\d+), BCG = BNCT \* BCK;", s).group(1))
    f64_cases = [c for c in FORWARD_AUTO + BACKWARD_AUTO if c[2] == F64]
    assert len(f64_cases) == 2 and all(c[3][1] == bck * bnct for c in f64_cases)


@pytest.mark.parametrize("case", FORWARD_AUTO + FORWARD_FORCED + BACKWARD_AUTO + DEBUG, ids=lambda c: c[0])
def test_plan(case):
    _, direction, dtype, shape, params, kw, want = case
    assert plan(direction, dtype, shape, params, **kw) == want


def test_plan_reports_more_candidates_than_it_stores():
    """max_ids bounds what is written, not what is counted; an empty batch plans nothing."""
    import ctypes
    ids = (ctypes.c_int * 2)(-7, -7)
    p = ctypes.c_void_p(A16)
    fn = fn2_capi.debug_lib().fn2_debug_correlation_plan
    args = (F32, 1, 64, 2, 8) + P20 + (fn2_capi.FN2_CORR_AUTO,)
    assert fn(0, p, p, p, None, None, ctypes.c_int64(0), *args, ids, 1) == 3 and list(ids) == [fn2_capi.CORR_KERNELS.index("F16X2"), -7]
    assert fn(1, p, p, p, p, p, ctypes.c_int64(0), *args, ids, 0) == 3 and list(ids) == [fn2_capi.CORR_KERNELS.index("F16X2"), -7]
    assert fn(2, p, p, p, p, p, ctypes.c_int64(0), *args, ids, 2) == EINVAL
    assert plan("forward", F32, (0, 64, 2, 8), P20) == [] and plan("backward", F32, (0, 64, 2, 8), P20) == []
    # the checks in front of the table, in the entry points' order: null, then element alignment, then algo
    assert plan("forward", F32, (1, 64, 2, 8), P20, ptrs=(A16, 0, A16 + 2), algo=9) == EINVAL
    assert plan("forward", F32, (1, 64, 2, 8), P20, ptrs=(A16, A16, A16 + 2), algo=9) == EALIGN
    assert plan("backward", F32, (1, 64, 2, 8), P20, ptrs=(A16, A16, A16, A16, A16 + 2), algo=9) == EALIGN
    assert plan("forward", F32, (1, 64, 2, 8), P20, out_bs=7055) == EINVAL        # a batch stride below the natural 441 * 2 * 8
    assert plan("forward", HALF, (1, 128, 2, 8), P20, ptrs=(A16 + 2, A16, A16)) == ["H16", "DIRECT"]   # the 16-bit row: its predicate alone
    assert plan("forward", BF16, (1, 128, 2, 8), P20, ptrs=(A8, A4, A16), algo=fn2_capi.FN2_CORR_MFMA_F16X2) == ["H16"]
