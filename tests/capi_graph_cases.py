"""The capture cases of tests/test_gpu_capi_graph.py: every entry point of include/*.h that takes a ``void *stream``, called raw (ctypes,
fn2_capi) the way a caller without PyTorch would, once per host-side sequence it can enqueue.  tests/test_capi_graph_cases_host.py holds
this table to the headers: an entry point without a case fails the host suite.

A Case says how to draw its inputs at a small shape (``inputs(seed)``: name -> CPU tensor), what it writes (``outputs``: name -> Out),
which buffers the header calls scratch (``scratch``: name -> bytes, poisoned with 0xFF before every replay) or primed (``primed``: name
-> bytes, zeroed once and never touched again), how to fill the inputs that are another entry point's results (``derive``, run eagerly
after the fresh values are in place), how to make the call (``call(T)``: T maps every name to its device buffer; returns the return
codes) and, for an output summed with float atomics, the float64 bound its layer's own GPU test applies (``check``).  Nothing here
allocates device memory: the GPU test owns the buffers.

Out.kind: "bits" -- the header promises repeatable bits: the replay must equal the eager call bit for bit; "atomic" -- fp32 atomics in
unspecified order: inside the bound of ``check``, exactly the seed (zero) where no contribution arrives; "zero" -- the empty batch:
exactly zero after every replay.  Out.part selects the elements the entry point writes where the buffer is larger (the channel
slice of the fused correlation forward); the rest must keep its poison."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

import corr_lookup_ref as RL
import fn2_capi
import forward_warp_ref as RS
import multiscale_ref as RM
import warp_contract_ref as RW
from corr_dispatch_cases import DENSE4, FLOWNETC, K3, P20, md
from resample_det_ref import warped_grad
from test_gpu_corr_lookup import _coords as lookup_coords
from test_gpu_multiscale_contract import DIV_FLOW, OTHER

F32, F16, BF16, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
Out = namedtuple("Out", "shape dtype kind part", defaults=("bits", None))
CF, CI64, CSZ = ctypes.c_float, ctypes.c_int64, ctypes.c_size_t


class Case:
    def __init__(self, id, fns, inputs, outputs, call, scratch=None, primed=None, derived=None, derive=None, check=None):
        self.id, self.fns, self.inputs, self.outputs, self.call = id, tuple(fns), inputs, outputs, call
        self.scratch, self.primed, self.derived, self.derive, self.check = scratch or {}, primed or {}, derived or {}, derive, check
        self.corr_plan = None      # correlation: (direction, the row AUTO must take, dtype code, shape, parameters, the buffers' names)
        assert all(o.kind in ("bits", "atomic", "zero") for o in outputs.values()), id
        assert check is not None or not any(o.kind == "atomic" for o in outputs.values()), id

    def __repr__(self):
        return self.id


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def raised(_):
    """The return code of a call through one of fn2_capi's wrappers, which raise on any other."""
    return 0


def nbytes(t):
    return t.numel() * t.element_size()


def _normal(seed, *shapes, dtype=F32, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(s, generator=g) * scale).to(dtype) for s in shapes]


def _np(rng, shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


CASES = []


def case(*a, **kw):
    CASES.append(Case(*a, **kw))


# ------------------------------------------------------------------ Correlation: one call per row of the dispatcher's table
def corr_out_shape(H, W, pad, k, mdisp, s1, s2):
    """fn2_correlation_output_shape in Python (the header's formula), so that the table needs no built library."""
    border = (k - 1) // 2 + mdisp
    return ((mdisp // s2) * 2 + 1) ** 2, -(-(H + 2 * pad - 2 * border) // s1), -(-(W + 2 * pad - 2 * border) // s1)


# (the row of kCorrRows FN2_CORR_AUTO takes, dtype, forward shape, backward shape, parameters): the calls of
# tests/corr_dispatch_cases.py that tests/test_gpu_corr_dispatch.py runs
CORR_ROWS = [
    ("F16X2", F32, FLOWNETC, FLOWNETC, P20),
    ("MFMA_F32", F32, (1, 32, 2, 2), (1, 32, 2, 2), md(4)),
    ("H16", F16, (1, 128, 2, 8), FLOWNETC, P20),
    ("H16", BF16, (1, 128, 2, 8), FLOWNETC, P20),
    ("F64", F64, (1, 64, 2, 2), (1, 64, 2, 2), P20),
    ("DENSE", F32, (8, 4, 48, 64), (8, 4, 48, 32), DENSE4),
    ("DIRECT", F32, (1, 3, 5, 6), (1, 3, 5, 6), K3),
]
EXTRA = 3          # channels in front of the correlation's slice of the concat buffer (conv_redir's place)
SLOPE = 0.1


def _corr_cases(row, dtype, fshape, bshape, params):
    tag = "%s-%s" % (row, str(dtype).split(".")[1])
    code = fn2_capi._dtype_code(torch.empty(0, dtype=dtype))
    es = torch.empty(0, dtype=dtype).element_size()

    def fwd(kind):
        B, C, H, W = fshape
        nOut, oH, oW = corr_out_shape(H, W, *params)
        fused = kind == "fused"
        oshape = (B, EXTRA + nOut if fused else nOut, oH, oW)

        def inputs(seed):
            a, b = _normal(seed, fshape, fshape, dtype=dtype)
            return {"in1": a, "in2": b}

        def call(T):
            lib, head = fn2_capi.lib(), (p(T["in1"]), p(T["in2"]))
            dims = (code, B, C, H, W) + tuple(params)
            if kind == "plain":
                return [lib.fn2_correlation_forward(*head, p(T["out"]), *dims, stream())]
            if kind == "ex":
                return [lib.fn2_correlation_forward_ex(*head, p(T["out"]), *dims, fn2_capi.FN2_CORR_AUTO, stream())]
            dst = ctypes.c_void_p(T["out"].data_ptr() + EXTRA * oH * oW * es)
            return [lib.fn2_correlation_forward_fused(*head, dst, CI64(oshape[1] * oH * oW), CF(SLOPE), *dims, fn2_capi.FN2_CORR_AUTO, stream())]

        name = {"plain": "fn2_correlation_forward", "ex": "fn2_correlation_forward_ex", "fused": "fn2_correlation_forward_fused"}[kind]
        c = Case("%s-%s" % (name, tag), [name], inputs, {"out": Out(oshape, dtype, "bits", (lambda t: t[:, EXTRA:]) if fused else None)}, call)
        if not fused:
            c.corr_plan = ("forward", row, code, fshape, params, ("in1", "in2", "out"))
        return c

    def bwd(kind):
        B, C, H, W = bshape
        nOut, oH, oW = corr_out_shape(H, W, *params)
        fused = kind == "fused"
        gshape = (B, EXTRA + nOut if fused else nOut, oH, oW)

        def inputs(seed):
            a, b, go = _normal(seed + 50, bshape, bshape, gshape, dtype=dtype)
            d = {"in1": a, "in2": b, "grad_out": go}
            if fused:
                d["out_act"] = _normal(seed + 70, gshape, dtype=dtype)[0]      # only its sign is read
            return d

        def wsb():
            return int(fn2_capi.lib().fn2_correlation_backward_fused_workspace_bytes(code, B, H, W, *params))

        def call(T):
            lib, head = fn2_capi.lib(), (p(T["in1"]), p(T["in2"]))
            tail = (p(T["grad_in1"]), p(T["grad_in2"]), code, B, C, H, W) + tuple(params)
            if kind == "plain":
                return [lib.fn2_correlation_backward(*head, p(T["grad_out"]), *tail, stream())]
            if kind == "ex":
                return [lib.fn2_correlation_backward_ex(*head, p(T["grad_out"]), *tail, fn2_capi.FN2_CORR_AUTO, stream())]
            off, bs = EXTRA * oH * oW * es, CI64(gshape[1] * oH * oW)
            return [lib.fn2_correlation_backward_fused(*head, ctypes.c_void_p(T["out_act"].data_ptr() + off), bs,
                                                       ctypes.c_void_p(T["grad_out"].data_ptr() + off), bs, CF(SLOPE), p(T["workspace"]),
                                                       CSZ(nbytes(T["workspace"])), *tail, fn2_capi.FN2_CORR_AUTO, stream())]

        name = {"plain": "fn2_correlation_backward", "ex": "fn2_correlation_backward_ex", "fused": "fn2_correlation_backward_fused"}[kind]
        c = Case("%s-%s" % (name, tag), [name], inputs, {"grad_in1": Out(bshape, dtype), "grad_in2": Out(bshape, dtype)}, call,
                 scratch={"workspace": wsb} if fused else None)
        if not fused:
            c.corr_plan = ("backward", row, code, bshape, params, ("in1", "in2", "grad_out", "grad_in1", "grad_in2"))
        return c

    kinds = ("plain", "ex") + (("fused",) if params == P20 else ())     # the fused pair: FlowNetC's configuration only
    return [fwd(k) for k in kinds] + [bwd(k) for k in kinds]


for _row in CORR_ROWS:
    CASES.extend(_corr_cases(*_row))


# ------------------------------------------------------------------ Resample2d, ChannelNorm
RESAMPLE = (2, 3, 5, 7)            # warp_contract_ref.UNTILED_SHAPES[0]
CHNORM = (1, 2, 7, 9)              # warp_contract_ref.CHNORM_SHAPES[1]


def _resample_inputs(seed, gout=True):
    B, C, H, W = RESAMPLE
    rng = np.random.default_rng(300 + seed)
    d = {"img": _np(rng, RESAMPLE), "flow": torch.from_numpy(RW.noise(B, H, W, seed=seed))}
    if gout:
        d["grad_out"] = _np(rng, RESAMPLE)
    return d


def _resample_dims():
    B, C, H, W = RESAMPLE
    return (B, C, H, W, H, W, 1, 1)


case("fn2_resample2d_forward", ["fn2_resample2d_forward"], lambda seed: _resample_inputs(seed, gout=False), {"out": Out(RESAMPLE, F32)},
     lambda T: [fn2_capi.lib().fn2_resample2d_forward(p(T["img"]), None, p(T["flow"]), p(T["out"]), *_resample_dims(), stream())])


def _resample_bwd_call(T):
    T["grad_img"].zero_()                                   # the caller's duty (header): captured as a fill kernel
    return [fn2_capi.lib().fn2_resample2d_backward(p(T["img"]), None, p(T["flow"]), p(T["grad_out"]), p(T["grad_img"]), p(T["grad_flow"]),
                                                   *_resample_dims(), stream())]


def _check_grad_img(got, ref_img, flow, gout, prefill, what):
    """``got`` inside grad_input1's bracket (warp_contract_ref.resample_bwd64); a cell no pixel reaches keeps the prefill's bits."""
    b = RW.resample_bwd64(ref_img, flow, gout, 1, prefill=prefill)
    ok = ~b.excluded[:, None]
    ratio = RW.ratio_and_check(got, b.gimg, b.gimg_delta, ok, what)
    keep = ~b.reached & ok
    pre = np.zeros_like(got) if prefill is None else prefill
    assert RW.same_bits(got, pre)[keep].all(), f"{what}: a cell no pixel reaches is not what it started as"
    assert b.reached.any()
    return ratio


def _resample_bwd_check(inp, got, eager):
    return _check_grad_img(got["grad_img"], inp["img"], inp["flow"], inp["grad_out"], None, "grad_img of fn2_resample2d_backward")


_B, _C, _H, _W = RESAMPLE
case("fn2_resample2d_backward", ["fn2_resample2d_backward"], _resample_inputs,
     {"grad_img": Out(RESAMPLE, F32, "atomic"), "grad_flow": Out((_B, 2, _H, _W), F32)}, _resample_bwd_call, check=_resample_bwd_check)


def _resample_det_wsb():
    B, C, H, W = RESAMPLE
    return int(fn2_capi.lib().fn2_resample2d_backward_det_workspace_bytes(B, C, H, W, H, W, 1))


def _resample_det_call(T):
    T["grad_img"].zero_()
    return [fn2_capi.lib().fn2_resample2d_backward_det(p(T["img"]), None, p(T["flow"]), p(T["grad_out"]), p(T["grad_img"]), p(T["grad_flow"]),
                                                       *_resample_dims(), p(T["workspace"]), CSZ(nbytes(T["workspace"])), stream())]


case("fn2_resample2d_backward_det", ["fn2_resample2d_backward_det"], _resample_inputs,
     {"grad_img": Out(RESAMPLE, F32), "grad_flow": Out((_B, 2, _H, _W), F32)}, _resample_det_call, scratch={"workspace": _resample_det_wsb})


def _chnorm_fwd(T, dtype_code=fn2_capi.FN2_F32):
    return fn2_capi.lib().fn2_channelnorm_forward(p(T["in"]), p(T["out"]), dtype_code, *CHNORM, stream())


case("fn2_channelnorm_forward", ["fn2_channelnorm_forward"], lambda seed: {"in": _normal(400 + seed, CHNORM)[0]},
     {"out": Out((CHNORM[0], 1) + CHNORM[2:], F32)}, lambda T: [_chnorm_fwd(T)])


def _chnorm_derive(T):
    assert _chnorm_fwd(T) == 0


case("fn2_channelnorm_backward", ["fn2_channelnorm_backward"],
     lambda seed: dict(zip(("in", "grad_out"), _normal(410 + seed, CHNORM, (CHNORM[0], 1) + CHNORM[2:]))), {"grad_in": Out(CHNORM, F32)},
     lambda T: [fn2_capi.lib().fn2_channelnorm_backward(p(T["in"]), p(T["out"]), p(T["grad_out"]), None, p(T["grad_in"]), fn2_capi.FN2_F32,
                                                        *CHNORM, stream())],
     derived={"out": ((CHNORM[0], 1) + CHNORM[2:], F32)}, derive=_chnorm_derive)


# ------------------------------------------------------------------ the fused warp rows
PAIR_RAGGED = (2, 2, 17, 33)       # B, C, H, W of warp_contract_ref.FUSED_SHAPES[2]: one lane per pixel
# grad_pair != NULL: C = 3 tileable (H >= 16, W >= 32, W % 4 == 0, ragged tiles), C = 3 not tileable, C != 3
PAIR_GRAD_SHAPES = {"c3-tiled": (2, 3, 33, 68), "c3-untiled": (2, 3, 17, 33), "c2": PAIR_RAGGED}
DIV = 20.0


def _pair_inputs(shape, seed, grad=None, dtype=F32):
    B, C, H, W = shape
    rng = np.random.default_rng(500 + seed + 7 * C)
    d = {"pair": _np(rng, (B, 2 * C, H, W)).to(dtype), "flow": torch.from_numpy(RW.noise(B, H, W, seed=seed + C)).to(dtype)}
    if grad == "cat":
        d["grad_cat"] = _np(rng, (B, 3 * C + 3, H, W)).to(dtype)
    if grad == "norm":
        d["grad_norm"] = _np(rng, (B, 1, H, W)).to(dtype)
    return d


def _cat_fwd(T, shape, out="out"):
    return fn2_capi.lib().fn2_warp_diff_norm_cat(p(T["pair"]), p(T["flow"]), p(T[out]), CF(DIV), *shape, 1, stream())


def _norm_fwd(T, shape, out="out"):
    return fn2_capi.lib().fn2_warp_diff_norm(p(T["pair"]), p(T["flow"]), p(T[out]), *shape, 1, stream())


def _cat_shape(shape):
    B, C, H, W = shape
    return (B, 3 * C + 3, H, W)


case("fn2_warp_diff_norm_cat", ["fn2_warp_diff_norm_cat"], lambda seed: _pair_inputs(PAIR_RAGGED, seed),
     {"out": Out(_cat_shape(PAIR_RAGGED), F32)}, lambda T: [_cat_fwd(T, PAIR_RAGGED)])
case("fn2_warp_diff_norm", ["fn2_warp_diff_norm"], lambda seed: _pair_inputs(PAIR_RAGGED, seed),
     {"out": Out((PAIR_RAGGED[0], 1) + PAIR_RAGGED[2:], F32)}, lambda T: [_norm_fwd(T, PAIR_RAGGED)])


def _norm_bwd_derive(T):
    assert _norm_fwd(T, PAIR_RAGGED, "norm") == 0


case("fn2_warp_diff_norm_backward", ["fn2_warp_diff_norm_backward"], lambda seed: _pair_inputs(PAIR_RAGGED, seed, "norm"),
     {"grad_flow": Out((PAIR_RAGGED[0], 2) + PAIR_RAGGED[2:], F32)},
     lambda T: [fn2_capi.lib().fn2_warp_diff_norm_backward(p(T["pair"]), p(T["flow"]), p(T["norm"]), p(T["grad_norm"]), p(T["grad_flow"]),
                                                           *PAIR_RAGGED, 1, stream())],
     derived={"norm": ((PAIR_RAGGED[0], 1) + PAIR_RAGGED[2:], F32)}, derive=_norm_bwd_derive)


def _cat_bwd_wsb(shape):
    return lambda: int(fn2_capi.lib().fn2_warp_diff_norm_cat_backward_det_workspace_bytes(*shape))


def _cat_bwd(T, shape, det, grad_pair="grad_pair", grad_cat="grad_cat", grad_flow="grad_flow"):
    lib = fn2_capi.lib()
    args = (p(T["pair"]), p(T["flow"]), p(T["out_cat"]), p(T[grad_cat]), p(T[grad_pair]) if grad_pair else None, p(T[grad_flow]), CF(DIV)) + \
        tuple(shape) + (1,)
    if det:
        return lib.fn2_warp_diff_norm_cat_backward_det(*args, p(T["workspace"]), CSZ(nbytes(T["workspace"])), stream())
    return lib.fn2_warp_diff_norm_cat_backward(*args, stream())


def _cat_bwd_case(tag, shape, det, with_pair):
    B, C, H, W = shape
    name = "fn2_warp_diff_norm_cat_backward" + ("_det" if det else "")
    outputs = {"grad_flow": Out((B, 2, H, W), F32)}
    if with_pair:
        # [:, :C] is a gather (bits); [:, C:] the seed plus the scatter: fp32 atomics, or fixed point in the _det twin (bits)
        outputs["grad_pair"] = Out((B, 2 * C, H, W), F32, "bits" if det else "atomic")

    def derive(T):
        assert _cat_fwd(T, shape, "out_cat") == 0

    def check(inp, got, eager):
        gp, gcat = got["grad_pair"], inp["grad_cat"]
        assert RW.same_bits(gp[:, :C], eager["grad_pair"][:, :C]).all(), "the first image's gradient (a gather) differs from the eager call"
        gw = warped_grad(inp["pair"], inp["out_cat"], gcat)
        return _check_grad_img(gp[:, C:], inp["pair"][:, C:], inp["flow"], gw, np.ascontiguousarray(gcat[:, C:2 * C]), f"grad_pair[:, C:] of {name}")

    return Case("%s-%s" % (name, tag), [name], lambda seed: _pair_inputs(shape, seed, "cat"), outputs,
                lambda T: [_cat_bwd(T, shape, det, "grad_pair" if with_pair else None)], scratch={"workspace": _cat_bwd_wsb(shape)} if det else None,
                derived={"out_cat": (_cat_shape(shape), F32)}, derive=derive, check=check if with_pair and not det else None)


for _det in (False, True):
    CASES.append(_cat_bwd_case("null-pair", PAIR_RAGGED, _det, False))
    for _tag, _shape in PAIR_GRAD_SHAPES.items():
        CASES.append(_cat_bwd_case(_tag, _shape, _det, True))

WARP16 = (2, 3, 50, 104)           # B, C, H, W of tests/test_gpu_warp16.py's RAGGED pair


def _warp16_cases():
    out = []
    for dtype in (F16, BF16):
        tag, code = str(dtype).split(".")[1], fn2_capi._dtype_code(torch.empty(0, dtype=dtype))
        B, C, H, W = WARP16
        lib = fn2_capi.lib
        out.append(Case("fn2_warp_diff_norm_cat_16-" + tag, ["fn2_warp_diff_norm_cat_16"], lambda seed, d=dtype: _pair_inputs(WARP16, seed, dtype=d),
                        {"out": Out(_cat_shape(WARP16), dtype)},
                        lambda T, c=code: [lib().fn2_warp_diff_norm_cat_16(p(T["pair"]), p(T["flow"]), p(T["out"]), c, CF(DIV), *WARP16, 1, stream())]))
        out.append(Case("fn2_warp_diff_norm_cat_backward_16-" + tag, ["fn2_warp_diff_norm_cat_backward_16"],
                        lambda seed, d=dtype: _pair_inputs(WARP16, seed, "cat", dtype=d), {"grad_flow": Out((B, 2, H, W), dtype)},
                        lambda T, c=code: [lib().fn2_warp_diff_norm_cat_backward_16(p(T["pair"]), p(T["flow"]), p(T["grad_cat"]), p(T["grad_flow"]), c,
                                                                                    CF(DIV), *WARP16, 1, stream())]))
        out.append(Case("fn2_warp_diff_norm_16-" + tag, ["fn2_warp_diff_norm_16"], lambda seed, d=dtype: _pair_inputs(WARP16, seed, dtype=d),
                        {"out": Out((B, 1, H, W), dtype)},
                        lambda T, c=code: [lib().fn2_warp_diff_norm_16(p(T["pair"]), p(T["flow"]), p(T["out"]), c, *WARP16, 1, stream())]))
        out.append(Case("fn2_warp_diff_norm_backward_16-" + tag, ["fn2_warp_diff_norm_backward_16"],
                        lambda seed, d=dtype: _pair_inputs(WARP16, seed, "norm", dtype=d), {"grad_flow": Out((B, 2, H, W), dtype)},
                        lambda T, c=code: [lib().fn2_warp_diff_norm_backward_16(p(T["pair"]), p(T["flow"]), p(T["grad_norm"]), p(T["grad_flow"]), c,
                                                                                *WARP16, 1, stream())]))
    return out


CASES.extend(_warp16_cases())


# ------------------------------------------------------------------ MultiScale
MS_STANDARD = (2, 48, 80, 2, 4)    # a standard case of tests/test_gpu_multiscale_contract.py (SHAPES[3])
MS_EMPTY = (0, 32, 32, 4, 2)       # its test_empty_batch


def ms_wsb(shape):
    return lambda: max(int(fn2_capi.lib().fn2_multiscale_workspace_bytes(*shape)), 64)


def _ms_inputs(shape, seed):
    target, outs, _ = RM.seeded_inputs(shape, seed)
    d = {"target": torch.from_numpy(target)}
    d.update({"pred%d" % i: torch.from_numpy(o) for i, o in enumerate(outs)})
    return d


def _ms_outputs(shape, fused, grads, suffix="", kind="bits"):
    B, H, W, s0, ns = shape
    d = {"sums" + suffix: Out((2 * ns,), F32, kind)}
    if fused:
        d["loss_epe" + suffix] = Out((2,), F32, kind)
    if grads:
        d.update({"grad%d%s" % (i, suffix): Out(s, F32) for i, s in enumerate(RM.level_shapes(B, H, W, s0, ns))})
    return d


def ms_call(T, entry, shape, norm, grads, primed=0, grad_scale=1.0, suffix="", ws="workspace"):
    B, H, W, s0, ns = shape
    lib = fn2_capi.lib()
    outs = ptr_array([T["pred%d%s" % (i, suffix)] for i in range(ns)])
    gptr = ptr_array([T["grad%d%s" % (i, suffix)] for i in range(ns)]) if grads else None
    wts = (ctypes.c_float * ns)(*[0.32 / 2 ** i for i in range(ns)])
    geo = (B, H, W, s0, ns, CF(DIV_FLOW), p(T[ws]), CSZ(int(lib.fn2_multiscale_workspace_bytes(*shape))))
    head = (outs, p(T["target" + suffix]), p(T["sums" + suffix]))
    if entry == "fn2_multiscale_l1_epe":
        return lib.fn2_multiscale_l1_epe(*head, gptr, wts, CF(grad_scale), *geo, stream())
    if entry == "fn2_multiscale_loss":
        return lib.fn2_multiscale_loss(*head, gptr, wts, CF(grad_scale), norm, *geo, stream())
    return lib.fn2_multiscale_loss_fused(*head, p(T["loss_epe" + suffix]), gptr, wts, CF(grad_scale), norm, *geo, primed, stream())


def _ms_case(entry, shape, norm, grads, primed=False):
    fused = entry == "fn2_multiscale_loss_fused"
    empty = shape[0] == 0
    tag = "%s-%s-L%d-%s" % (entry, "empty" if empty else "primed" if primed else "unprimed", norm, "grads" if grads else "nograds")
    ws = {"workspace": ms_wsb(shape)}
    return Case(tag, [entry], lambda seed: _ms_inputs(shape, seed), _ms_outputs(shape, fused, grads, kind="zero" if empty else "bits"),
                lambda T: [ms_call(T, entry, shape, norm, grads, primed=int(primed))], scratch=None if primed else ws, primed=ws if primed else None)


for _grads in (True, False):
    CASES.append(_ms_case("fn2_multiscale_l1_epe", MS_STANDARD, 1, _grads))
    for _norm in (1, 2):
        CASES.append(_ms_case("fn2_multiscale_loss", MS_STANDARD, _norm, _grads))
        CASES.append(_ms_case("fn2_multiscale_loss_fused", MS_STANDARD, _norm, _grads))
        CASES.append(_ms_case("fn2_multiscale_loss_fused", MS_STANDARD, _norm, _grads, primed=True))
CASES.append(_ms_case("fn2_multiscale_l1_epe", MS_EMPTY, 1, True))
CASES.append(_ms_case("fn2_multiscale_loss", MS_EMPTY, 2, True))
CASES.append(_ms_case("fn2_multiscale_loss_fused", MS_EMPTY, 1, True))
CASES.append(_ms_case("fn2_multiscale_loss_fused", MS_EMPTY, 2, False, primed=True))

SCALE_SIZES = [1000, 0, 77]        # test_scale_grads' levels without the one longer than a pass of the grid


def _scale_call(T):
    live = [i for i, n in enumerate(SCALE_SIZES) if n]
    ins = ptr_array([T["unit%d" % i] if i in live else None for i in range(len(SCALE_SIZES))])
    outs = ptr_array([T["grad%d" % i] if i in live else None for i in range(len(SCALE_SIZES))])
    return [fn2_capi.lib().fn2_multiscale_scale_grads(ins, outs, (ctypes.c_int64 * len(SCALE_SIZES))(*SCALE_SIZES), len(SCALE_SIZES), p(T["scale"]),
                                                      stream())]


def _scale_inputs(seed):
    rng = np.random.default_rng(600 + seed)
    d = {"unit%d" % i: _np(rng, (n,), 1e-3) for i, n in enumerate(SCALE_SIZES) if n}
    d["scale"] = torch.tensor([1.5 + seed], dtype=F32)
    return d


case("fn2_multiscale_scale_grads", ["fn2_multiscale_scale_grads"], _scale_inputs,
     {"grad%d" % i: Out((n,), F32) for i, n in enumerate(SCALE_SIZES) if n}, _scale_call)


# ------------------------------------------------------------------ the six sibling libraries
CORR1D = ((2, 20, 9, 70), 4)       # shape, pad = md; stride1 = stride2 = 1, two-sided: nOut = 2 md + 1, oH x oW = H x W
LOOKUP = dict(B=2, C=5, s1=(13, 19), s2=(13, 19), r=3, coords="c")      # family c stays at the borders: the middle of fmap2 gets no term
UPSAMPLE = dict(B=2, C=2, H=5, W=67, f=8)
SPLAT = (1, 2, 17, 67)
CENSUS = (1, 1, 17, 67)
SMOOTH = (1, 1, 1, 17, 65)         # N, F, C, H, W


def _corr1d_go():
    (B, C, H, W), m = CORR1D
    return (B, 2 * m + 1, H, W)


case("fn2x_correlation1d_forward", ["fn2x_correlation1d_forward"], lambda seed: dict(zip(("in1", "in2"), _normal(700 + seed, CORR1D[0], CORR1D[0]))),
     {"out": Out(_corr1d_go(), F32)},
     lambda T: [raised(fn2_capi.correlation1d_forward(T["in1"], T["in2"], CORR1D[1], CORR1D[1], 1, 1, out=T["out"]))])
case("fn2x_correlation1d_backward", ["fn2x_correlation1d_backward"],
     lambda seed: dict(zip(("in1", "in2", "grad_out"), _normal(710 + seed, CORR1D[0], CORR1D[0], _corr1d_go()))),
     {"grad_in1": Out(CORR1D[0], F32), "grad_in2": Out(CORR1D[0], F32)},
     lambda T: [raised(fn2_capi.correlation1d_backward(T["in1"], T["in2"], T["grad_out"], CORR1D[1], CORR1D[1], 1, 1, out=(T["grad_in1"], T["grad_in2"]))
               )])


def _lookup_inputs(seed, gout=False):
    L = LOOKUP
    f1, f2 = _normal(800 + seed, (L["B"], L["C"]) + L["s1"], (L["B"], L["C"]) + L["s2"])
    d = {"fmap1": f1, "fmap2": f2, "coords": lookup_coords(L["coords"], L["B"], *L["s1"], *L["s2"], L["r"], seed=seed)}
    if gout:
        d["grad_out"] = _normal(820 + seed, (L["B"], (2 * L["r"] + 1) ** 2) + L["s1"])[0]
    return d


LOOKUP_SCALE = float(LOOKUP["C"]) ** -0.5


def _lookup_check(inp, got, eager):
    L = LOOKUP
    _, (e2, S2, n2) = RL.backward(inp["fmap1"], inp["fmap2"], inp["coords"], inp["grad_out"], L["r"], LOOKUP_SCALE)
    g2 = got["grad_fmap2"]
    err, delta = np.abs(g2.astype(np.float64) - e2), RL.delta_grad2(e2, S2, n2, LOOKUP_SCALE)
    assert (err <= delta).all(), "grad_fmap2 of fn2l_corr_lookup_backward: %.3g x the bound" % float((err / np.maximum(delta, 1e-300)).max())
    assert (n2 > 0).any() and (n2 == 0).any() and (g2[n2 == 0] == 0).all(), "grad_fmap2 is not exactly zero where no term arrives"
    return float((err / np.maximum(delta, 1e-300)).max())


case("fn2l_corr_lookup_forward", ["fn2l_corr_lookup_forward"], _lookup_inputs,
     {"out": Out((LOOKUP["B"], (2 * LOOKUP["r"] + 1) ** 2) + LOOKUP["s1"], F32)},
     lambda T: [raised(fn2_capi.corr_lookup_forward(T["fmap1"], T["fmap2"], T["coords"], LOOKUP["r"], LOOKUP_SCALE, out=T["out"]))])
case("fn2l_corr_lookup_backward", ["fn2l_corr_lookup_backward"], lambda seed: _lookup_inputs(seed, gout=True),
     {"grad_fmap1": Out((LOOKUP["B"], LOOKUP["C"]) + LOOKUP["s1"], F32), "grad_fmap2": Out((LOOKUP["B"], LOOKUP["C"]) + LOOKUP["s2"], F32, "atomic")},
     lambda T: [raised(fn2_capi.corr_lookup_backward(T["fmap1"], T["fmap2"], T["coords"], T["grad_out"], LOOKUP["r"], LOOKUP_SCALE,
                                              out=(T["grad_fmap1"], T["grad_fmap2"])))], check=_lookup_check)


def _upsample_shapes():
    U = UPSAMPLE
    return ((U["B"], U["C"], U["H"], U["W"]), (U["B"], 9 * U["f"] ** 2, U["H"], U["W"]), (U["B"], U["C"], U["f"] * U["H"], U["f"] * U["W"]))


def _upsample_inputs(seed, gout=False):
    fs, ms, os_ = _upsample_shapes()
    rng = np.random.default_rng(900 + seed)
    d = {"flow": _np(rng, fs, 10.0), "mask": _np(rng, ms, 3.0)}
    if gout:
        d["grad_out"] = _np(rng, os_)
    return d


def _upsample_wsb():
    U = UPSAMPLE
    return max(int(fn2_capi.upsample_lib().fn2u_convex_upsample_backward_workspace_bytes(U["B"], U["C"], U["H"], U["W"])), 4)


case("fn2u_convex_upsample_forward", ["fn2u_convex_upsample_forward"], _upsample_inputs, {"out": Out(_upsample_shapes()[2], F32)},
     lambda T: [raised(fn2_capi.convex_upsample_forward(T["flow"], T["mask"], UPSAMPLE["f"], float(UPSAMPLE["f"]), out=T["out"]))])
case("fn2u_convex_upsample_backward", ["fn2u_convex_upsample_backward"], lambda seed: _upsample_inputs(seed, gout=True),
     {"grad_flow": Out(_upsample_shapes()[0], F32), "grad_mask": Out(_upsample_shapes()[1], F32)},
     lambda T: [raised(fn2_capi.convex_upsample_backward(T["flow"], T["mask"], T["grad_out"], UPSAMPLE["f"], float(UPSAMPLE["f"]),
                                                  out=(T["grad_flow"], T["grad_mask"]), workspace=T["workspace"]))],
     scratch={"workspace": _upsample_wsb})


def _splat_inputs(seed, gout=False):
    B, C, H, W = SPLAT
    rng = np.random.default_rng(1000 + seed)
    d = {"input": _np(rng, SPLAT), "flow": torch.from_numpy(RS.flow_family("smooth", B, H, W, seed=seed))}
    if gout:
        d["grad_out"] = _np(rng, SPLAT)
    return d


def _splat_check(inp, got, eager):
    ref, S, n = RS.forward(inp["input"], inp["flow"])
    out = got["out"]
    err, bound = np.abs(out.astype(np.float64) - ref), RS.forward_bound(S, n)
    assert (err <= bound).all(), "out of fn2s_forward_warp_forward: %.3g x the bound" % float((err / bound).max())
    assert (S > 0).any() and (np.ascontiguousarray(out).view(np.uint32)[S == 0] == 0).all(), "a cell without contributions is not +0"
    return float((err / bound).max())


def _splat_det_wsb():
    return max(int(fn2_capi.splat_lib().fn2s_forward_warp_forward_det_workspace_bytes(*SPLAT)), 8)


case("fn2s_forward_warp_forward", ["fn2s_forward_warp_forward"], _splat_inputs, {"out": Out(SPLAT, F32, "atomic")},
     lambda T: [raised(fn2_capi.forward_warp_forward(T["input"], T["flow"], out=T["out"]))], check=_splat_check)
case("fn2s_forward_warp_forward_det", ["fn2s_forward_warp_forward_det"], _splat_inputs, {"out": Out(SPLAT, F32)},
     lambda T: [raised(fn2_capi.forward_warp_forward_det(T["input"], T["flow"], out=T["out"], workspace=T["workspace"]))],
     scratch={"workspace": _splat_det_wsb})
case("fn2s_forward_warp_backward", ["fn2s_forward_warp_backward"], lambda seed: _splat_inputs(seed, gout=True),
     {"grad_input": Out(SPLAT, F32), "grad_flow": Out((SPLAT[0], 2) + SPLAT[2:], F32)},
     lambda T: [raised(fn2_capi.forward_warp_backward(T["input"], T["flow"], T["grad_out"], out=(T["grad_input"], T["grad_flow"])))])


def _census_inputs(seed, gout=False):
    g = torch.Generator().manual_seed(1100 + seed)
    d = {"im1": torch.rand(CENSUS, generator=g), "im2": torch.rand(CENSUS, generator=g)}
    if gout:
        d["grad_out"] = torch.randn(CENSUS[0], 1, *CENSUS[2:], generator=g)
    return d


case("fn2c_census_forward", ["fn2c_census_forward"], _census_inputs, {"out": Out((CENSUS[0], 1) + CENSUS[2:], F32)},
     lambda T: [raised(fn2_capi.census_forward(T["im1"], T["im2"], out=T["out"]))])
case("fn2c_census_backward", ["fn2c_census_backward"], lambda seed: _census_inputs(seed, gout=True),
     {"grad_im1": Out(CENSUS, F32), "grad_im2": Out(CENSUS, F32)},
     lambda T: [raised(fn2_capi.census_backward(T["im1"], T["im2"], T["grad_out"], grads=(T["grad_im1"], T["grad_im2"])))])


def _smooth_inputs(seed, gout=False):
    N, F, C, H, W = SMOOTH
    g = torch.Generator().manual_seed(1200 + seed)
    d = {"flow": torch.randn(N, F, H, W, generator=g), "image": torch.rand(N, C, H, W, generator=g)}
    if gout:
        d["grad_out"] = torch.randn(N, 2, H, W, generator=g)
    return d


case("fn2m_smoothness_forward", ["fn2m_smoothness_forward"], _smooth_inputs, {"out": Out((SMOOTH[0], 2) + SMOOTH[3:], F32)},
     lambda T: [raised(fn2_capi.smoothness_forward(T["flow"], T["image"], out=T["out"]))])
case("fn2m_smoothness_backward", ["fn2m_smoothness_backward"], lambda seed: _smooth_inputs(seed, gout=True),
     {"grad_flow": Out((SMOOTH[0], SMOOTH[1]) + SMOOTH[3:], F32)},
     lambda T: [raised(fn2_capi.smoothness_backward(T["flow"], T["image"], T["grad_out"], out=T["grad_flow"]))])


# ------------------------------------------------------------------ composites: two calls in one graph on one shared scratch buffer
def _two_ms_inputs(seed):
    d = {k + "_a": v for k, v in _ms_inputs(MS_STANDARD, seed).items()}
    d.update({k + "_b": v for k, v in _ms_inputs(OTHER, seed + 10).items()})
    return d


def _two_ms_call(T):
    return [ms_call(T, "fn2_multiscale_loss_fused", MS_STANDARD, 1, True, suffix="_a"),
            ms_call(T, "fn2_multiscale_loss_fused", OTHER, 2, True, grad_scale=3.0, suffix="_b")]


case("two-unprimed-multiscale-calls-share-a-scratch", ["fn2_multiscale_loss_fused"], _two_ms_inputs,
     {**_ms_outputs(MS_STANDARD, True, True, "_a"), **_ms_outputs(OTHER, True, True, "_b")}, _two_ms_call,
     scratch={"workspace": lambda: max(ms_wsb(MS_STANDARD)(), ms_wsb(OTHER)())})

TWO_DET = PAIR_GRAD_SHAPES["c3-untiled"]


def _two_det_inputs(seed):
    d = _pair_inputs(TWO_DET, seed, "cat")
    d["grad_cat_b"] = _normal(1300 + seed, _cat_shape(TWO_DET), scale=2.0)[0]
    return d


def _two_det_derive(T):
    assert _cat_fwd(T, TWO_DET, "out_cat") == 0


def _two_det_call(T):
    return [_cat_bwd(T, TWO_DET, True), _cat_bwd(T, TWO_DET, True, "grad_pair_b", "grad_cat_b", "grad_flow_b")]


_B, _C, _H, _W = TWO_DET
case("two-det-pair-gradients-share-a-workspace", ["fn2_warp_diff_norm_cat_backward_det"], _two_det_inputs,
     {"grad_pair": Out((_B, 2 * _C, _H, _W), F32), "grad_flow": Out((_B, 2, _H, _W), F32),
      "grad_pair_b": Out((_B, 2 * _C, _H, _W), F32), "grad_flow_b": Out((_B, 2, _H, _W), F32)}, _two_det_call,
     scratch={"workspace": _cat_bwd_wsb(TWO_DET)}, derived={"out_cat": (_cat_shape(TWO_DET), F32)}, derive=_two_det_derive)

assert len({c.id for c in CASES}) == len(CASES), "case ids must be unique"


def covered():
    """The C-ABI functions the table calls."""
    return {fn for c in CASES for fn in c.fns}
