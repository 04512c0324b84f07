"""The calls that pin the correlation dispatcher (csrc/capi.hip): per case the plan fn2_debug_correlation_plan must report -- the
kernels (fn2_capi.CORR_KERNELS) in the order the dispatcher would try them, or the code the entry point returns before any launch.
A case is (id, direction, dtype, (B, C, H, W), (pad, k, md, s1, s2), keywords of fn2_capi.correlation_plan, plan)."""
import fn2_capi
from fn2_capi import FN2_CORR_DIRECT as DIRECT, FN2_CORR_MFMA_BF16X3 as BF16X3, FN2_CORR_MFMA_F16X2 as F16X2, FN2_CORR_MFMA_F32 as MFMA_F32
from fn2_capi import FN2_BF16 as BF16, FN2_F16 as HALF, FN2_F32 as F32, FN2_F64 as F64, FN2_DEBUG_CORR_DENSE as DENSE9000

EINVAL, EDTYPE, EALIGN, EUNSUPPORTED = -1, -2, -3, -4
A16, A8, A4 = 0x1000, 0x1008, 0x1004          # an address aligned to 16 bytes, to 8 only, to 4 only
P20 = (20, 1, 20, 1, 2)                        # FlowNetC's configuration


def md(r, s2=2):
    return (r, 1, r, 1, s2)                    # pad = md = r, k 1, s1 1


DENSE4 = md(4, 1)                              # PWC-Net's
K3 = (3, 3, 4, 1, 2)
FLOWNETC, WIDE, SMALL = (1, 64, 2, 8), (1, 64, 2, 72), (1, 16, 2, 2)
N_FLOWNETC = 441 * 2 * 8                       # the natural batch stride of FLOWNETC's output


def plan(direction, dtype, shape, params, **kw):
    return fn2_capi.correlation_plan(direction, dtype, shape, *params, **kw)


def _f(name, dtype, shape, params, want, **kw):
    return ("fwd " + name, "forward", dtype, shape, params, kw, want)


def _b(name, dtype, shape, params, want, **kw):
    return ("bwd " + name, "backward", dtype, shape, params, kw, want)


FORWARD_AUTO = [
    _f("flownetc", F32, FLOWNETC, P20, ["F16X2", "MFMA_F32", "DIRECT"]),
    _f("in1 at 8", F32, FLOWNETC, P20, ["MFMA_F32", "DIRECT"], ptrs=(A8, A16, A16)),
    _f("in1 at 4", F32, FLOWNETC, P20, ["DIRECT"], ptrs=(A4, A16, A16)),
    _f("odd out_bs", F32, FLOWNETC, P20, ["DIRECT"], out_bs=N_FLOWNETC + 1),
    _f("wide", F32, WIDE, P20, ["F16X2", "MFMA_F32", "DIRECT"]),
    _f("md 4", F32, SMALL, md(4), ["MFMA_F32", "DIRECT"]),
    _f("md 22", F32, SMALL, md(22), ["DIRECT"]),
    _f("md 1", F32, SMALL, md(1), ["DIRECT"]),
    _f("half", HALF, (1, 128, 2, 8), P20, ["H16", "DIRECT"]),
    _f("bf16", BF16, (1, 128, 2, 8), P20, ["H16", "DIRECT"]),
    _f("bf16 C 64", BF16, (1, 64, 2, 8), P20, ["DIRECT"]),
    _f("f64", F64, (1, 64, 2, 2), P20, ["F64", "DIRECT"]),
    _f("dense 192 tiles", F32, (8, 4, 48, 64), DENSE4, ["DENSE", "DIRECT"]),
    _f("dense 96 tiles", F32, (8, 4, 48, 32), DENSE4, ["DIRECT"]),
    _f("k 3", F32, (1, 3, 5, 6), K3, ["DIRECT"]),
]

FORWARD_FORCED = [
    _f("direct", F32, FLOWNETC, P20, ["DIRECT"], algo=DIRECT),
    _f("mfma_f32", F32, FLOWNETC, P20, ["MFMA_F32"], algo=MFMA_F32),
    _f("bf16x3", F32, FLOWNETC, P20, ["MFMA_F32"], algo=BF16X3),
    _f("f16x2 on md 4", F32, SMALL, md(4), EUNSUPPORTED, algo=F16X2),
    _f("f16x2 in1 at 8", F32, FLOWNETC, P20, EUNSUPPORTED, algo=F16X2, ptrs=(A8, A16, A16)),
    _f("f16x2 on half", HALF, (1, 128, 2, 8), P20, ["H16"], algo=F16X2),
    _f("mfma_f32 on half", HALF, (1, 128, 2, 8), P20, EUNSUPPORTED, algo=MFMA_F32),
    _f("algo 5", F32, FLOWNETC, P20, EINVAL, algo=5),
    _f("algo -1", F32, FLOWNETC, P20, EINVAL, algo=-1),
    _f("dtype 7", 7, FLOWNETC, P20, EDTYPE),
]

BACKWARD_AUTO = [
    _b("flownetc", F32, FLOWNETC, P20, ["F16X2", "MFMA_F32", "DIRECT"]),
    _b("grad_in1 at 8", F32, FLOWNETC, P20, ["MFMA_F32", "DIRECT"], ptrs=(A16, A16, A16, A8, A16)),
    _b("grad_in1 at 4", F32, FLOWNETC, P20, ["MFMA_F32", "DIRECT"], ptrs=(A16, A16, A16, A4, A16)),
    _b("grad_out at 4", F32, FLOWNETC, P20, ["DIRECT"], ptrs=(A16, A16, A4, A16, A16)),
    _b("wide", F32, WIDE, P20, ["F16X2", "MFMA_F32", "DIRECT"]),
    _b("md 4 C 16", F32, SMALL, md(4), ["DIRECT"]),
    _b("md 4 C 32", F32, (1, 32, 2, 2), md(4), ["MFMA_F32", "DIRECT"]),
    _b("half", HALF, FLOWNETC, P20, ["H16", "DIRECT"]),
    _b("half wide", HALF, WIDE, P20, ["DIRECT"]),
    _b("f64", F64, (1, 64, 2, 2), P20, ["F64", "DIRECT"]),
    _b("dense 96 tiles", F32, (8, 4, 48, 32), DENSE4, ["DENSE", "DIRECT"]),
    _b("stride1 2", F32, (1, 4, 8, 8), (4, 1, 4, 2, 2), EUNSUPPORTED),
]

DEBUG = [
    _f("9000 dense", F32, (8, 4, 48, 32), DENSE4, ["DENSE"], algo=DENSE9000),
    _b("9000 dense", F32, (8, 4, 48, 32), DENSE4, ["DENSE"], algo=DENSE9000),
    _f("9000 flownetc", F32, FLOWNETC, P20, EUNSUPPORTED, algo=DENSE9000),
    _b("9000 flownetc", F32, FLOWNETC, P20, EUNSUPPORTED, algo=DENSE9000),
    _f("5001", F32, FLOWNETC, P20, ["F16X2"], algo=5001),
    _b("6001", F32, FLOWNETC, P20, ["F16X2"], algo=6001),
    _f("5001 on md 4", F32, (1, 32, 2, 2), md(4), EUNSUPPORTED, algo=5001),
    _b("6001 on md 4", F32, (1, 32, 2, 2), md(4), EUNSUPPORTED, algo=6001),
    _f("101 on md 4", F32, (1, 32, 2, 2), md(4), ["MFMA_F32"], algo=101),
    _b("101 on md 4", F32, (1, 32, 2, 2), md(4), ["MFMA_F32"], algo=101),
    _f("101 on half", HALF, (1, 128, 2, 8), P20, EUNSUPPORTED, algo=101),
    _b("101 on half", HALF, FLOWNETC, P20, EUNSUPPORTED, algo=101),
]
