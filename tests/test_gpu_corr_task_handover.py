"""What a task of the persistent correlation kernels computes does not depend on which workgroup ran it or on what that
workgroup ran before: every task samples its own operands and takes its own scale exponents (csrc/correlation_f16x2*.hip,
csrc/correlation_f16_fwd.hip / _bwd.hip: sample_issue, sample_scales, publish).  A batch that needs more tasks than the grid
has workgroups (256) is run whole -- workgroups then run two or three tasks, and between them the next task's sample, scales,
first operand chunks and register sets are handed over while the current task still computes -- and each batch item is run
again alone (B = 1: fewer than 256 tasks, one per workgroup, no hand-over).  The item's slices must have identical bits.  The
items carry different magnitudes (family 6 and gradOutput 'items' of tests/corr_contract_ref.py; a row ramp for the 16-bit
kernels), so an exponent, sample or operand chunk taken from the neighbouring task changes the bits.

A second launch of the whole batch (through the explicit selector, which also names the kernel) must repeat the first one's
bits: a race between the publication of a task's scales and the matrix waves' reads would not.

Outputs are prefilled with NaN (every element must be written) and lie between sentinel guards that must stay untouched."""
import pytest
import torch

import corr_contract_ref as R
import lowp_ref as L

pytestmark = pytest.mark.gpu

CORR = L.CORR
SLOPE = 0.1
GUARD = 64            # elements before and after an output (keeps the 16-byte alignment of every type)
SENTINEL = 12345.0    # exact in half, bfloat16 and float32


def _bits(x):
    return x.contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int16)


def _guarded(shape, dev, dtype):
    """(flat, out): out is a NaN-filled tensor of `shape` inside flat, GUARD sentinel elements on either side."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev)
    out = flat[GUARD:GUARD + n].view(shape)
    out.fill_(float("nan"))
    return flat, out


def _written(what, *pairs):
    for flat, out in pairs:
        assert bool((flat[:GUARD] == SENTINEL).all() & (flat[-GUARD:] == SENTINEL).all()), f"{what}: a write outside the output"
        assert not bool(torch.isnan(out).any()), f"{what}: unwritten output elements"


def _forward(ad, bd, what, algo=None):
    import fn2_capi
    B, C, H, W = ad.shape
    flat, out = _guarded((B,) + L.out_shape(H, W, *CORR), ad.device, ad.dtype)
    fn2_capi.correlation_forward(ad, bd, *CORR, algo=fn2_capi.FN2_CORR_AUTO if algo is None else algo, out=out)
    _written(what, (flat, out))
    return out


def _forward_fused(ad, bd, what):
    """The fused LeakyReLU + store into channels 8 .. 8 + 441 of a concat buffer; the other channels must keep their bits."""
    import fn2_capi
    B, C, H, W = ad.shape
    nOut, oH, oW = L.out_shape(H, W, *CORR)
    flat, buf = _guarded((B, 8 + nOut + 3, oH, oW), ad.device, ad.dtype)
    buf[:, :8] = 3.0
    buf[:, 8 + nOut:] = -5.0
    fn2_capi.correlation_forward_fused(ad, bd, buf, 8, SLOPE, *CORR)
    _written(what, (flat, buf))
    assert bool((buf[:, :8] == 3.0).all() & (buf[:, 8 + nOut:] == -5.0).all()), f"{what}: a write outside the slice"
    return buf[:, 8:8 + nOut]


def _backward(ad, bd, gd, what, algo=None):
    import fn2_capi
    p1, p2 = _guarded(ad.shape, ad.device, ad.dtype), _guarded(ad.shape, ad.device, ad.dtype)
    fn2_capi.correlation_backward(ad, bd, gd, *CORR, algo=fn2_capi.FN2_CORR_AUTO if algo is None else algo, out=(p1[1], p2[1]))
    _written(what, p1, p2)
    return p1[1], p2[1]


def _same(whole, alone, i, what):
    assert torch.equal(_bits(whole[i:i + 1]), _bits(alone)), \
        f"{what}: item {i} of the batch differs from the item run alone in {int((_bits(whole[i:i + 1]) != _bits(alone)).sum())} elements"


def _inputs32(shape, dev):
    """Family 6 (items at 2^30, 2^-30, 1, ...) with gradOutput 'items' (2^20, 1, 2^-40, ...)."""
    B, C, H, W = shape
    a, b = R.family_inputs(6, shape, seed=sum(shape))
    go = R.grad_output("items", (B,) + L.out_shape(H, W, *CORR), sum(shape) + 6)
    return a.to(dev), b.to(dev), go.to(dev)


def _check_backward(ad, bd, gd, items, what):
    import fn2_capi
    w1, w2 = _backward(ad, bd, gd, what)
    s1, s2 = _backward(ad, bd, gd, what + " second launch", algo=fn2_capi.FN2_CORR_MFMA_F16X2)
    assert torch.equal(_bits(s1), _bits(w1)) and torch.equal(_bits(s2), _bits(w2)), f"{what}: a second launch gives other bits"
    for i in items:
        g1, g2 = _backward(ad[i:i + 1], bd[i:i + 1], gd[i:i + 1], f"{what} item {i} alone")
        _same(w1, g1, i, what + " grad_input1")
        _same(w2, g2, i, what + " grad_input2")


def _check_forward(ad, bd, items, what, fused=True):
    import fn2_capi
    whole = _forward(ad, bd, what)
    again = _forward(ad, bd, what + " second launch", algo=fn2_capi.FN2_CORR_MFMA_F16X2)
    assert torch.equal(_bits(again), _bits(whole)), f"{what}: a second launch gives other bits"
    fwhole = _forward_fused(ad, bd, what + " fused") if fused else None
    for i in items:
        _same(whole, _forward(ad[i:i + 1], bd[i:i + 1], f"{what} item {i} alone"), i, what)
        if fused:
            _same(fwhole, _forward_fused(ad[i:i + 1], bd[i:i + 1], f"{what} fused item {i} alone"), i, what + " fused")


# 264, 288 and 528 tasks (tests/test_gpu_f32_contract.py BWD_MULTI); of the 22 items: the first ones, the ones the first
# workgroups' second tasks fall into (256 / 24 tasks per item: items 10 and 11), and the last
NARROW_BWD = [((11, 192, 14, 56), range(11)), ((3, 256, 48, 64), range(3)), ((22, 64, 48, 8), (0, 1, 10, 11, 21))]


@pytest.mark.parametrize("shape,items", NARROW_BWD, ids=["x".join(map(str, c[0])) for c in NARROW_BWD])
def test_narrow_backward_items_do_not_depend_on_the_schedule(dev, shape, items):
    ad, bd, gd = _inputs32(shape, dev)
    _check_backward(ad, bd, gd, items, f"f16x2 bwd {shape}")


NARROW_FWD = [(9, 320, 48, 8), (4, 64, 48, 64)]
WIDE = (2, 192, 46, 128)
LOWP = (4, 256, 56, 64)


@pytest.mark.parametrize("shape", NARROW_FWD, ids=lambda s: "x".join(map(str, s)))
def test_narrow_forward_items_do_not_depend_on_the_schedule(dev, shape):
    """72 tasks per item: 648 and 288 tasks on at most 256 workgroups; plain and fused."""
    ad, bd, _ = _inputs32(shape, dev)
    _check_forward(ad, bd, range(shape[0]), f"f16x2 fwd {shape}")


def test_wide_kernels_items_do_not_depend_on_the_schedule(dev):
    """The column-window kernels: 336 forward tasks (42 row-group pairs x 4 windows per item), 288 backward tasks."""
    shape = WIDE
    ad, bd, gd = _inputs32(shape, dev)
    _check_forward(ad, bd, range(2), f"f16x2 wide fwd {shape}")
    _check_backward(ad, bd, gd, range(2), f"f16x2 wide bwd {shape}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["half", "bf16"])
def test_16bit_kernels_items_do_not_depend_on_the_schedule(dev, dtype):
    """The half / bfloat16 matrix kernels (the same persistent grids): 336 forward and 448 backward tasks; a row ramp
    (lowp_ref family 5), so that the tasks of a workgroup read other magnitudes."""
    shape = LOWP
    a, b = L.family_inputs(5, shape, dtype, seed=sum(shape))
    go = L.grad_output("normal", (shape[0],) + L.out_shape(*shape[2:], *CORR), dtype, sum(shape))
    ad, bd, gd = a.to(dev), b.to(dev), go.to(dev)
    _check_forward(ad, bd, range(shape[0]), f"{dtype} fwd {shape}")
    _check_backward(ad, bd, gd, range(shape[0]), f"{dtype} bwd {shape}")
