"""The fused MultiScale loss kernel (csrc/multiscale_loss.hip) per element against float64, at every geometry it accepts: the contract,
its rounding counts and the checks are tests/multiscale_ref.py (tests/test_multiscale_contract_host.py runs the same checks on a float32
emulation and on deliberately wrong kernels).  No tolerance here is a constant: each is a bound computed from the inputs, or equality
of bits.  Every result buffer is filled with NaN before a call, so an element the kernel does not write shows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import multiscale_ref as R

pytestmark = pytest.mark.gpu

DIV_FLOW = 0.05
# (B, H, W, start_scale, num_scales) -- what each one exercises:
SHAPES = [
    (2, 100, 202, 4, 5),   # ragged in both directions; W % 4 != 0: the scalar level-0 path with k = 4; coarsest level 1 x 3
    (2, 100, 200, 4, 5),   # the float4 path (and, below, the same target one float past a 16-byte boundary: the scalar path)
    (1, 37, 70, 1, 5),     # start_scale 1: 256 one-pixel cells per workgroup
    (2, 48, 80, 2, 4),     # start_scale 2, four levels
    (1, 64, 96, 8, 3),     # start_scale 8, three levels
    (1, 70, 300, 16, 5),   # start_scale 16, k_max = 256 > H: levels 3 and 4 have no elements
    (3, 16, 16, 4, 1),     # one level; one cell per workgroup edge
    (1, 130, 70, 4, 5),    # W < 2 k_max
    (2, 96, 96, 1, 3),     # 1152 workgroups: five trips of the last workgroup's strided loop
]
MISALIGNED = (2, 100, 200, 4, 5)
EMPTY_LEVELS = (1, 70, 300, 16, 5)
OTHER = (1, 20, 44, 2, 3)  # the call of another geometry on a workspace primed by the shapes above (its partial sums end elsewhere)
EXACT_SHAPES = [(2, 100, 202, 4, 5), (1, 37, 70, 1, 5)]

_refs = {}


def sid(shape):
    return "%dx%dx%d_s%d_n%d" % tuple(shape)


def seeded(shape):
    if shape not in _refs:
        target, outs, w = R.seeded_inputs(shape)
        _refs[shape] = (target, outs, w, R.Ref(target, outs, w, shape[3], DIV_FLOW))
    return _refs[shape]


def other():
    """The inputs of the call of another geometry, with a grad_scale of its own."""
    if "other" not in _refs:
        target, outs, w = R.seeded_inputs(OTHER)
        _refs["other"] = (target, outs, w, R.Ref(target, outs, w, OTHER[3], DIV_FLOW, grad_scale=3.0))
    return _refs["other"]


def error_codes():
    """FN2_* of include/flownet2_hip.h."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flownet2_hip.h")
    with open(path) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(FN2_(?:OK|E[A-Z]+))\s*=\s*(-?\d+)", f.read())}


def nan_like(t):
    return torch.full_like(t, float("nan"))


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def workspace_bytes(shape):
    import fn2_capi
    return int(fn2_capi.lib().fn2_multiscale_workspace_bytes(*shape))


def call(dev, shape, target, outs, weights, norm, div_flow=DIV_FLOW, grad_scale=1.0, ws=None, ws_bytes=None, primed=0, fused=True,
         null_levels=(), want_grads=True, null_weights=False):
    """One call of fn2_multiscale_loss_fused (or fn2_multiscale_loss) through ctypes.  ``target``: a device tensor or None; ``outs``: device
    tensors; levels in ``null_levels`` are passed as null pointers (prediction and gradient).  Returns (rc, sums, loss_epe, grads) as
    numpy arrays (grads: None at a null level)."""
    import fn2_capi
    B, H, W, s0, ns = shape
    sums = torch.full((2 * ns,), float("nan"), device=dev)
    loss_epe = torch.full((2,), float("nan"), device=dev)
    grads = [None if i in null_levels else nan_like(o) for i, o in enumerate(outs)] if want_grads else None
    if ws is None:
        ws_bytes = workspace_bytes(shape) if ws_bytes is None else ws_bytes
        ws = torch.full((max(workspace_bytes(shape), 64) // 4,), float("nan"), device=dev)     # any scratch memory will do unprimed
    elif ws_bytes is None:
        ws_bytes = ws.numel() * 4
    optr = ptr_array([None if i in null_levels else o for i, o in enumerate(outs)])
    gptr = ptr_array(grads) if want_grads else None
    wts = None if null_weights else (ctypes.c_float * len(outs))(*[float(w) for w in weights])
    lib = fn2_capi.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        if fused:
            rc = lib.fn2_multiscale_loss_fused(optr, ptr(target), ptr(sums), ptr(loss_epe), gptr, wts, ctypes.c_float(grad_scale), int(norm),
                                               B, H, W, s0, ns, ctypes.c_float(div_flow), ptr(ws), ctypes.c_size_t(ws_bytes), int(primed), stream)
        else:
            rc = lib.fn2_multiscale_loss(optr, ptr(target), ptr(sums), gptr, wts, ctypes.c_float(grad_scale), int(norm), B, H, W, s0, ns,
                                         ctypes.c_float(div_flow), ptr(ws), ctypes.c_size_t(ws_bytes), stream)
    torch.cuda.synchronize(dev)
    g = [None if t is None else t.cpu().numpy() for t in grads] if want_grads else None
    return rc, sums.cpu().numpy(), loss_epe.cpu().numpy(), g


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def one_float_past_16_bytes(t):
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.reshape(-1)
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_contract(ref, norm, sums, loss_epe, grads, tag):
    for name, rep in R.run_checks(ref, norm, sums, loss_epe, grads).items():
        print(f"MSRATIO {tag} norm{norm} {name} {rep.ratio:.4f} | {rep.worst}")
        assert rep.ok, rep


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("shape,misaligned", [(s, False) for s in SHAPES] + [(MISALIGNED, True)],
                         ids=[sid(s) for s in SHAPES] + [sid(MISALIGNED) + "_misaligned"])
def test_contract(dev, shape, misaligned, norm):
    """Gradients, sums and loss / epe inside the bounds of tests/multiscale_ref.py; the unprimed entry point and the primed one give the
    same bits; three primed calls on one workspace give the same bits (the ticket counter is left at zero); a call of another geometry
    on that workspace is still correct."""
    target, outs, w, ref = seeded(shape)
    assert ref.undetermined_count() == 0                                # a condition on the inputs, checked before the kernel's output
    td = to_dev(target, dev)
    if misaligned:
        td = one_float_past_16_bytes(td)
    else:
        assert td.data_ptr() % 16 == 0
    od = [to_dev(o, dev) for o in outs]
    tag = sid(shape) + ("_misaligned" if misaligned else "")

    rc, sums0, _, grads0 = call(dev, shape, td, od, w, norm, fused=False)
    assert rc == 0

    otarget, oouts, ow, oref = other()
    assert oref.undetermined_count() == 0
    nbytes = max(workspace_bytes(shape), workspace_bytes(OTHER))
    assert workspace_bytes(shape) != workspace_bytes(OTHER)
    ws = torch.zeros(nbytes // 4, device=dev)
    rc, sums, loss_epe, grads = call(dev, shape, td, od, w, norm, ws=ws, ws_bytes=workspace_bytes(shape), primed=1)
    assert rc == 0
    assert_contract(ref, norm, sums, loss_epe, grads, tag)
    assert same_bits(sums, sums0) and all(same_bits(a, b) for a, b in zip(grads, grads0)), "unprimed and primed calls differ"
    for _ in range(2):
        rc, s2, le2, g2 = call(dev, shape, td, od, w, norm, ws=ws, ws_bytes=workspace_bytes(shape), primed=1)
        assert rc == 0
        assert same_bits(s2, sums) and same_bits(le2, loss_epe) and all(same_bits(a, b) for a, b in zip(g2, grads))
    assert int(ws[:1].view(torch.int32).item()) == 0, "the ticket counter is not left at zero"
    rc, s3, le3, g3 = call(dev, OTHER, to_dev(otarget, dev), [to_dev(o, dev) for o in oouts], ow, norm, grad_scale=3.0, ws=ws, primed=1)
    assert rc == 0
    for rep in R.run_checks(oref, norm, s3, le3, g3).values():
        assert rep.ok, ("another geometry on the primed workspace", rep)


@pytest.mark.parametrize("norm", [1, 2])
def test_levels_without_elements(dev, norm):
    """k = 128 and 256 exceed H = 70: levels 3 and 4 are empty.  As empty tensors and as null pointers: same bits, their sums exactly 0,
    nothing of them in loss / epe; and the autograd node takes the empty tensors."""
    import multiscale_loss_cuda
    shape = EMPTY_LEVELS
    target, outs, w, ref = seeded(shape)
    assert [o.size for o in outs[3:]] == [0, 0]
    td, od = to_dev(target, dev), [to_dev(o, dev) for o in outs]
    ws = torch.zeros(workspace_bytes(shape) // 4, device=dev)
    rc, sa, la, ga = call(dev, shape, td, od, w, norm, ws=ws, primed=1)
    assert rc == 0
    rc, sb, lb, gb = call(dev, shape, td, od, w, norm, ws=ws, primed=1, null_levels=(3, 4))
    assert rc == 0
    assert gb[3] is None and gb[4] is None
    assert_contract(ref, norm, sb, lb, gb, sid(shape) + "_null")
    assert same_bits(sa, sb) and same_bits(la, lb) and all(same_bits(a, b) for a, b in zip(ga[:3], gb[:3]))
    for s in (sa, sb):
        assert s[3] == 0 and s[4] == 0 and s[8] == 0 and s[9] == 0
    of = [o.clone().requires_grad_(True) for o in od]
    loss, epe = multiscale_loss_cuda.apply(td, of, shape[3], DIV_FLOW, w, norm)
    got = np.array([float(loss.detach()), float(epe.detach())], np.float32)
    assert same_bits(got, la), (got, la)
    loss.backward()
    for i, o in enumerate(of):
        assert o.grad is not None and o.grad.shape == o.shape
        assert same_bits(o.grad.cpu().numpy(), ga[i]) or o.numel() == 0


@pytest.mark.parametrize("norm", [1, 2])
def test_empty_batch(dev, norm):
    """B = 0: all sums are 0 and nothing is launched (the scratch memory is not touched, not even the ticket counter's clear)."""
    import multiscale_loss_cuda
    shape = (0, 32, 32, 4, 2)
    w = [0.32, 0.16]
    outs = [torch.empty((0, 2, 8, 8), device=dev), torch.empty((0, 2, 4, 4), device=dev)]
    pattern = torch.arange(1, 65, dtype=torch.float32, device=dev)
    for target in (torch.empty((0, 2, 32, 32), device=dev), torch.zeros(4, device=dev)):   # (an empty tensor's pointer may be null)
        ws = pattern.clone()
        rc, sums, loss_epe, grads = call(dev, shape, target, outs, w, norm, ws=ws, primed=0)
        assert rc == 0
        assert np.array_equal(sums, np.zeros(4, np.float32)) and np.array_equal(loss_epe, np.zeros(2, np.float32))
        assert torch.equal(ws, pattern)
    of = [o.clone().requires_grad_(True) for o in outs]
    loss, epe = multiscale_loss_cuda.apply(torch.empty((0, 2, 32, 32), device=dev), of, 4, DIV_FLOW, w, norm)
    assert float(loss.detach()) == 0 and float(epe.detach()) == 0
    loss.backward()
    assert all(o.grad is not None and o.grad.shape == o.shape for o in of)


@pytest.mark.parametrize("shape", EXACT_SHAPES, ids=sid)
def test_exact_case(dev, shape):
    """Integer targets, div_flow = 2^-3, dyadic predictions (multiples of 2^-11 or coarser, multiscale_ref.exact_inputs): every pooled
    mean, difference and L1 partial sum is a float32 number in any order, so L1 sums and norm-1 gradients equal the float64 values bit
    for bit; predictions planted equal to the pooled target give gradient exactly 0 under both norms (a zero norm gives 0, not NaN)."""
    target, outs, w, df = R.exact_inputs(shape)
    ref = R.Ref(target, outs, w, shape[3], df)
    assert sum(int((d == 0).sum()) for d in ref.d) >= 20
    td, od = to_dev(target, dev), [to_dev(o, dev) for o in outs]
    rc, s1, le1, g1 = call(dev, shape, td, od, w, 1, div_flow=df)
    assert rc == 0
    rc, s2, le2, g2 = call(dev, shape, td, od, w, 2, div_flow=df)
    assert rc == 0
    rep = R.check_exact(ref, s1, g1, g2)
    assert rep.ok, rep
    assert same_bits(s1, s2)
    assert_contract(ref, 1, s1, le1, g1, sid(shape) + "_exact")
    assert_contract(ref, 2, s2, le2, g2, sid(shape) + "_exact")


@pytest.mark.parametrize("g", [1.0, -3.0, 2.0 ** -20])
def test_scale_grads(dev, g):
    """fn2_multiscale_scale_grads: out = float32(in * g) bit for bit (one rounding of an exact product), a level with numel 0 and null
    pointers skipped, and a level longer than one pass of the 2048 x 256 grid."""
    import fn2_capi
    rng = np.random.default_rng(5)
    sizes = [1000, 0, 77, 2048 * 256 + 300]
    ins = [None if n == 0 else to_dev((rng.standard_normal(n) * 1e-3).astype(np.float32), dev) for n in sizes]
    outs = [None if t is None else nan_like(t) for t in ins]
    scale = torch.tensor([g], dtype=torch.float32, device=dev)
    numel = (ctypes.c_int64 * len(sizes))(*sizes)
    with torch.cuda.device(dev):
        rc = fn2_capi.lib().fn2_multiscale_scale_grads(ptr_array(ins), ptr_array(outs), numel, len(sizes), ptr(scale),
                                                       ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    assert rc == 0
    for i, (a, b) in enumerate(zip(ins, outs)):
        if a is None:
            continue
        want = (a.cpu().numpy().astype(np.float64) * np.float64(np.float32(g))).astype(np.float32)
        rep = R.Report("scale_grads")
        rep.equal(i, b.cpu().numpy(), want)
        assert rep.ok, rep


@pytest.mark.parametrize("norm", [1, 2])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["half", "bfloat16"])
def test_half_and_bfloat16_predictions(dev, dtype, norm):
    """Through multiscale_loss_cuda.apply: loss and EPE are those of a float32 run on the widened predictions, bit for bit, each gradient is
    the float32 gradient rounded once to the prediction's dtype -- and that float32 run satisfies the contract."""
    import multiscale_loss_cuda
    shape = (2, 48, 80, 2, 4)
    target, outs, w, _ = seeded(shape)
    td = to_dev(target, dev)
    o16 = [to_dev(o, dev).to(dtype) for o in outs]
    wide = [o.float() for o in o16]
    ref = R.Ref(target, [o.cpu().numpy() for o in wide], w, shape[3], DIV_FLOW)
    assert ref.undetermined_count() == 0
    a = [o.clone().requires_grad_(True) for o in o16]
    b = [o.clone().requires_grad_(True) for o in wide]
    la, ea = multiscale_loss_cuda.apply(td, a, shape[3], DIV_FLOW, w, norm)
    lb, eb = multiscale_loss_cuda.apply(td, b, shape[3], DIV_FLOW, w, norm)
    assert la.dtype == torch.float32 and torch.equal(la.detach(), lb.detach()) and torch.equal(ea.detach(), eb.detach())
    la.backward()
    lb.backward()
    for x, y in zip(a, b):
        assert x.grad.dtype == dtype and torch.equal(x.grad, y.grad.to(dtype))
    le = np.array([float(lb.detach()), float(eb.detach())], np.float32)
    grads = [y.grad.cpu().numpy() for y in b]
    rep = R.check_loss_epe(ref, le, norm)
    assert rep.ok, rep
    rep = R.check_grads_l1(ref, grads) if norm == 1 else R.check_grads_l2(ref, grads)
    assert rep.ok, rep


def test_rejections(dev):
    """Calls the header documents as rejected return its codes and launch nothing: results and scratch memory stay as they were."""
    import fn2_capi
    E = error_codes()
    assert E["FN2_OK"] == 0 and E["FN2_EINVAL"] < 0 and E["FN2_EUNSUPPORTED"] < 0 and E["FN2_EINVAL"] != E["FN2_EUNSUPPORTED"]
    B, H, W = 1, 64, 64
    target = torch.zeros((B, 2, H, W), device=dev)
    outs = [torch.zeros((B, 2, H, W), device=dev) for _ in range(7)]    # (roomy: a call accepted by mistake stays inside them)
    w = [0.1] * 7
    pattern = torch.arange(1, 16385, dtype=torch.float32, device=dev)

    def rejected(shape, want, n=None, **kw):
        ws = pattern.clone()
        n = shape[4] if n is None else n
        kw.setdefault("ws_bytes", ws.numel() * 4)
        for fused in (True, False):
            if kw.get("null_weights") and not fused:
                continue
            rc, sums, loss_epe, grads = call(dev, shape, target, outs[:n], w[:n], 1, ws=ws, primed=0, fused=fused, **kw)
            assert rc == E[want], (shape, fused, rc, want)
            assert np.isnan(sums).all() and np.isnan(loss_epe).all() and all(np.isnan(g).all() for g in grads)
            assert torch.equal(ws, pattern)

    lib = fn2_capi.lib()
    for shape, want in (((B, H, W, 4, 6), "FN2_EUNSUPPORTED"), ((B, H, W, 4, 7), "FN2_EINVAL"), ((B, H, W, 3, 2), "FN2_EINVAL"),
                        ((B, H, W, 32, 1), "FN2_EUNSUPPORTED"), ((B, H, W, 0, 2), "FN2_EINVAL"), ((B, H, W, 4, 0), "FN2_EINVAL")):
        rejected(shape, want, n=max(shape[4], 1))
        assert lib.fn2_multiscale_workspace_bytes(*shape) == 0
    good = (B, H, W, 4, 3)
    need = workspace_bytes(good)
    assert need > 64
    rejected(good, "FN2_EINVAL", ws_bytes=need - 1)                      # a workspace that is too small
    rejected(good, "FN2_EINVAL", null_weights=True)                     # the fused entry point needs the weights
    ws = pattern.clone()
    rc, sums, loss_epe, grads = call(dev, good, target, outs[:3], w[:3], 1, ws=ws, ws_bytes=need, primed=0)
    assert rc == 0 and not np.isnan(sums).any() and not np.isnan(loss_epe).any()             # and the same call, complete, is taken
    with pytest.raises(RuntimeError, match=r"1\.\.5 predictions"):
        import multiscale_loss_cuda
        multiscale_loss_cuda.apply(target, outs[:6], 4, DIV_FLOW, w[:6], 1)
