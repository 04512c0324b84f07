"""ctypes view of the C ABI (include/flownet2_hip.h) for callers that hold raw device pointers --
used by the parity tests and bench.py to reach entry points the pybind modules do not expose
(e.g. the ``*_ex`` algorithm selectors).  Raises if libflownet2_hip.so has not been built: there
is no fallback implementation.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libflownet2_hip.so")
DEBUG_LIB_PATH = os.path.join(_HERE, "lib", "libflownet2_hip_debug.so")   # same kernels + fn2_debug_* (csrc/fn2_debug.h)

FN2_F32, FN2_F16, FN2_F64, FN2_BF16 = 0, 1, 2, 3
FN2_CORR_AUTO, FN2_CORR_DIRECT, FN2_CORR_MFMA_F32, FN2_CORR_MFMA_BF16X3, FN2_CORR_MFMA_F16X2 = 0, 1, 2, 3, 4

EXPORTS = [
    "fn2_strerror", "fn2_abi_version", "fn2_correlation_output_shape",
    "fn2_correlation_forward", "fn2_correlation_forward_ex", "fn2_correlation_forward_fused",
    "fn2_correlation_backward", "fn2_correlation_backward_ex",
    "fn2_correlation_backward_fused_workspace_bytes", "fn2_correlation_backward_fused",
    "fn2_resample2d_forward", "fn2_resample2d_backward", "fn2_warp_diff_norm_cat",
    "fn2_warp_diff_norm_cat_backward", "fn2_warp_diff_norm", "fn2_warp_diff_norm_backward",
    "fn2_channelnorm_forward", "fn2_channelnorm_backward",
    "fn2_multiscale_workspace_bytes", "fn2_multiscale_l1_epe", "fn2_multiscale_loss",
    "fn2_multiscale_loss_fused", "fn2_multiscale_scale_grads",
    "fn2_resample2d_backward_det_workspace_bytes", "fn2_resample2d_backward_det",
    "fn2_warp_diff_norm_cat_backward_det_workspace_bytes", "fn2_warp_diff_norm_cat_backward_det",
    "fn2_warp_diff_norm_cat_16", "fn2_warp_diff_norm_cat_backward_16", "fn2_warp_diff_norm_16", "fn2_warp_diff_norm_backward_16",
]

# profiling / ablation entry points (csrc/fn2_debug.h): not in include/flownet2_hip.h, results wrong by design; exported by
# libflownet2_hip_debug.so only
DEBUG_EXPORTS = ["fn2_debug_correlation_forward", "fn2_debug_correlation_backward", "fn2_debug_set_buffer",
                 "fn2_debug_resample2d_forward", "fn2_debug_resample2d_backward", "fn2_debug_stream_copy", "fn2_debug_mfma_probe",
                 "fn2_debug_xcc_census", "fn2_debug_correlation_plan"]
CORR_KERNELS = ("H16", "F16X2", "MFMA_F32", "F64", "DENSE", "DIRECT")   # csrc/fn2_debug.h FN2_CORR_KERNEL_*, in FN2_CORR_AUTO's order

# the one debug variant whose results are correct: the dense stride-1 kernels (csrc/correlation_dense.hip) by name, for
# correlation_forward / correlation_backward(..., algo=FN2_DEBUG_CORR_DENSE); FN2_EUNSUPPORTED outside their domain
FN2_DEBUG_CORR_DENSE = 9000

# libflownet2_hip_ext.so (include/flownet2_hip_ext.h): layers outside the drop-in boundary, a library and an ABI of their own
EXT_LIB_PATH = os.path.join(_HERE, "lib", "libflownet2_hip_ext.so")
EXT_EXPORTS = ["fn2x_abi_version", "fn2x_correlation1d_output_shape", "fn2x_correlation1d_forward", "fn2x_correlation1d_backward"]
FN2X_CORR1D_AUTO, FN2X_CORR1D_GENERAL, FN2X_CORR1D_TILED = 0, 1, 2

# libflownet2_hip_lookup.so (include/flownet2_hip_lookup.h): CorrLookup, RAFT's correlation lookup
LOOKUP_LIB_PATH = os.path.join(_HERE, "lib", "libflownet2_hip_lookup.so")
LOOKUP_EXPORTS = ["fn2l_abi_version", "fn2l_corr_lookup_forward", "fn2l_corr_lookup_backward"]
FN2L_LOOKUP_AUTO, FN2L_LOOKUP_GENERAL, FN2L_LOOKUP_STAGED = 0, 1, 2

# libflownet2_hip_upsample.so (include/flownet2_hip_upsample.h): ConvexUpsample, RAFT's convex flow upsampling
UPSAMPLE_LIB_PATH = os.path.join(_HERE, "lib", "libflownet2_hip_upsample.so")
UPSAMPLE_EXPORTS = ["fn2u_abi_version", "fn2u_convex_upsample_forward", "fn2u_convex_upsample_backward",
                    "fn2u_convex_upsample_backward_workspace_bytes"]

# libflownet2_hip_splat.so (include/flownet2_hip_splat.h): ForwardWarp, forward flow splatting
SPLAT_LIB_PATH = os.path.join(_HERE, "lib", "libflownet2_hip_splat.so")
SPLAT_EXPORTS = ["fn2s_abi_version", "fn2s_forward_warp_forward", "fn2s_forward_warp_forward_det_workspace_bytes",
                 "fn2s_forward_warp_forward_det", "fn2s_forward_warp_backward"]
FN2S_AUTO, FN2S_GENERAL, FN2S_TILED = 0, 1, 2

# libflownet2_hip_census.so (include/flownet2_hip_census.h): the ternary census distance
CENSUS_LIB_PATH = os.path.join(_HERE, "lib", "libflownet2_hip_census.so")
CENSUS_EXPORTS = ["fn2c_abi_version", "fn2c_census_forward", "fn2c_census_backward"]

# libflownet2_hip_smooth.so (include/flownet2_hip_smooth.h): the edge-aware smoothness term
SMOOTH_LIB_PATH = os.path.join(_HERE, "lib", "libflownet2_hip_smooth.so")
SMOOTH_EXPORTS = ["fn2m_abi_version", "fn2m_smoothness_forward", "fn2m_smoothness_backward"]
FN2M_EDGE = {"exponential": 0, "gaussian": 1}

# preview -- libflownet2_hip_sample.so (include/preview/flownet2_hip_sample.h): CorrSample, the lookup of a prebuilt correlation
# pyramid (RAFT's CorrBlock); ABI version 0, may change until released
SAMPLE_LIB_PATH = os.path.join(_HERE, "lib", "libflownet2_hip_sample.so")
SAMPLE_EXPORTS = ["fn2p_abi_version", "fn2p_corr_sample_forward", "fn2p_corr_sample_backward"]

# incubating -- libflownet2_hip_pyramid.so (include/preview/flownet2_hip_pyramid.h): CorrPyramid, the build of that pyramid and the
# fold of its gradients; ABI version 0, may change until released
PYRAMID_LIB_PATH = os.path.join(_HERE, "lib", "libflownet2_hip_pyramid.so")
PYRAMID_EXPORTS = ["fn2y_abi_version", "fn2y_corr_pyramid_forward", "fn2y_corr_pyramid_fold"]
FN2Y_MAX_LEVELS = 4

# staging -- libflownet2_hip_ssim.so (include/staging/flownet2_hip_ssim.h): the structural-similarity distance; ABI version 0, may
# change until released
SSIM_LIB_PATH = os.path.join(_HERE, "lib", "libflownet2_hip_ssim.so")
SSIM_EXPORTS = ["fn2i_abi_version", "fn2i_ssim_forward", "fn2i_ssim_backward"]
FN2I_BORDER = {"zero": 0, "reflect": 1}

# staging -- libflownet2_hip_sample1d.so (include/staging/flownet2_hip_sample1d.h): CorrSample1d, the lookup of a prebuilt 1-D
# correlation pyramid (RAFT-Stereo's CorrBlock1D); ABI version 0, may change until released
SAMPLE1D_LIB_PATH = os.path.join(_HERE, "lib", "libflownet2_hip_sample1d.so")
SAMPLE1D_EXPORTS = ["fn2h_abi_version", "fn2h_corr_sample1d_forward", "fn2h_corr_sample1d_backward"]

_INT, _PTR = ctypes.c_int, ctypes.c_void_p
_RESTYPES = {"fn2_strerror": ctypes.c_char_p, "fn2_debug_set_buffer": None}   # every other entry point returns int or size_t
# name -> (the global that holds the path (scripts point it at another build before the first call), exports, the names that
# return size_t, explicit argtypes); "debug" is libflownet2_hip_debug.so, where the size queries keep ctypes' int
_LIBS = {
    "": ("LIB_PATH", EXPORTS, ("fn2_multiscale_workspace_bytes", "fn2_correlation_backward_fused_workspace_bytes",
                               "fn2_resample2d_backward_det_workspace_bytes", "fn2_warp_diff_norm_cat_backward_det_workspace_bytes"),
         {"fn2_strerror": [_INT]}),
    "debug": ("DEBUG_LIB_PATH", EXPORTS + DEBUG_EXPORTS, (), {}),
    "ext": ("EXT_LIB_PATH", EXT_EXPORTS, (), {}),
    "lookup": ("LOOKUP_LIB_PATH", LOOKUP_EXPORTS, (), {}),
    "upsample": ("UPSAMPLE_LIB_PATH", UPSAMPLE_EXPORTS, ("fn2u_convex_upsample_backward_workspace_bytes",), {}),
    "splat": ("SPLAT_LIB_PATH", SPLAT_EXPORTS, ("fn2s_forward_warp_forward_det_workspace_bytes",),
              {"fn2s_forward_warp_forward_det": [_PTR] * 4 + [ctypes.c_size_t] + [_INT] * 4 + [_PTR]}),
    "census": ("CENSUS_LIB_PATH", CENSUS_EXPORTS, (),
               {"fn2c_census_forward": [_PTR] * 3 + [_INT] * 5 + [ctypes.c_float, _INT, _PTR],
                "fn2c_census_backward": [_PTR] * 5 + [_INT] * 5 + [ctypes.c_float, _INT, _PTR]}),
    "smooth": ("SMOOTH_LIB_PATH", SMOOTH_EXPORTS, (),
               {"fn2m_smoothness_forward": [_PTR] * 3 + [_INT] * 7 + [ctypes.c_float, ctypes.c_float, _PTR],
                "fn2m_smoothness_backward": [_PTR] * 4 + [_INT] * 7 + [ctypes.c_float, ctypes.c_float, _PTR]}),
    "sample": ("SAMPLE_LIB_PATH", SAMPLE_EXPORTS, (),
               {"fn2p_corr_sample_forward": [_PTR] * 3 + [_INT] + [_PTR] * 2 + [_INT] * 4 + [_PTR],
                "fn2p_corr_sample_backward": [_PTR] * 2 + [_INT] + [_PTR] * 3 + [_INT] * 4 + [_PTR]}),
    "pyramid": ("PYRAMID_LIB_PATH", PYRAMID_EXPORTS, (),
                {"fn2y_corr_pyramid_forward": [_PTR] * 3 + [_INT] * 7 + [_PTR],
                 "fn2y_corr_pyramid_fold": [_PTR, _INT, _PTR] + [_INT] * 6 + [_PTR]}),
    "ssim": ("SSIM_LIB_PATH", SSIM_EXPORTS, (),
             {"fn2i_ssim_forward": [_PTR] * 3 + [_INT] * 5 + [ctypes.c_float, ctypes.c_float, _INT, _PTR],
              "fn2i_ssim_backward": [_PTR] * 5 + [_INT] * 5 + [ctypes.c_float, ctypes.c_float, _INT, _PTR]}),
    "sample1d": ("SAMPLE1D_LIB_PATH", SAMPLE1D_EXPORTS, (),
                 {"fn2h_corr_sample1d_forward": [_PTR] * 2 + [_INT, _PTR, ctypes.c_longlong, _PTR] + [_INT] * 4 + [_PTR],
                  "fn2h_corr_sample1d_backward": [_PTR, _INT, _PTR, ctypes.c_longlong] + [_PTR] * 2 + [_INT] * 4 + [_PTR]}),
}
_loaded = {}


def _load(name):
    """The library `name` of _LIBS with its return and argument types set, loaded once.  ``import torch`` first so that the HIP
    runtime torch already mapped (same soname) is the one the kernels register with.  Every library is self-contained: it loads
    without any of the others."""
    if name not in _loaded:
        import torch  # noqa: F401
        path_global, exports, size_t, argtypes = _LIBS[name]
        path = globals()[path_global]
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: run `python flownet2-pytorch_amd/build.py`" +
                               ("" if name == "debug" else " (the HIP kernels are the only implementation)"))
        dll = ctypes.CDLL(path)
        for fn in exports:
            if name == "debug" and not hasattr(dll, fn):      # (A/B runs load older builds that lack the newer entry points)
                continue
            getattr(dll, fn).restype = ctypes.c_size_t if fn in size_t else _RESTYPES.get(fn, _INT)
        for fn, types in argtypes.items():
            getattr(dll, fn).argtypes = types
        _loaded[name] = dll
    return _loaded[name]


def lib():
    """libflownet2_hip.so (include/flownet2_hip.h)."""
    return _load("")


def debug_lib():
    """libflownet2_hip_debug.so: the product kernels plus the profiling instantiations (scripts/, ablations)."""
    return _load("debug")


def ext_lib():
    """libflownet2_hip_ext.so: Correlation1d (csrc/correlation_1d.hip)."""
    return _load("ext")


def lookup_lib():
    """libflownet2_hip_lookup.so: CorrLookup (csrc/corr_lookup.hip)."""
    return _load("lookup")


def upsample_lib():
    """libflownet2_hip_upsample.so: ConvexUpsample (csrc/convex_upsample.hip)."""
    return _load("upsample")


def splat_lib():
    """libflownet2_hip_splat.so: ForwardWarp (csrc/forward_warp.hip)."""
    return _load("splat")


def census_lib():
    """libflownet2_hip_census.so: the ternary census distance (csrc/census.hip)."""
    return _load("census")


def smooth_lib():
    """libflownet2_hip_smooth.so: the edge-aware smoothness term (csrc/smooth.hip)."""
    return _load("smooth")


def sample_lib():
    """libflownet2_hip_sample.so (preview): CorrSample (csrc/corr_sample.hip)."""
    return _load("sample")


def pyramid_lib():
    """libflownet2_hip_pyramid.so (incubating): CorrPyramid (csrc/corr_pyramid.hip)."""
    return _load("pyramid")


def ssim_lib():
    """libflownet2_hip_ssim.so (staging): the structural-similarity distance (csrc/ssim.hip)."""
    return _load("ssim")


def sample1d_lib():
    """libflownet2_hip_sample1d.so (staging): CorrSample1d (csrc/corr_sample1d.hip)."""
    return _load("sample1d")


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: {lib().fn2_strerror(rc).decode()} (code {rc})")


def _dtype_code(t):
    import torch
    return {torch.float32: FN2_F32, torch.float16: FN2_F16, torch.float64: FN2_F64, torch.bfloat16: FN2_BF16}[t.dtype]


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream(t):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def correlation_output_shape(H, W, pad, k, md, s1, s2):
    n, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(lib().fn2_correlation_output_shape(H, W, pad, k, md, s1, s2, ctypes.byref(n), ctypes.byref(oh),
                                             ctypes.byref(ow)), "fn2_correlation_output_shape")
    return n.value, oh.value, ow.value


def correlation_forward(in1, in2, pad, k, md, s1, s2, algo=FN2_CORR_AUTO, out=None):
    import torch
    B, C, H, W = in1.shape
    nOut, oH, oW = correlation_output_shape(H, W, pad, k, md, s1, s2)
    if out is None:
        out = torch.empty((B, nOut, oH, oW), dtype=in1.dtype, device=in1.device)
    # algo >= 100: profiling instantiations, only reachable through the debug entry point
    fn, what = ((debug_lib().fn2_debug_correlation_forward, "fn2_debug_correlation_forward") if algo >= 100 else
                (lib().fn2_correlation_forward_ex, "fn2_correlation_forward_ex"))
    with torch.cuda.device_of(in1):
        check(fn(_p(in1), _p(in2), _p(out), _dtype_code(in1), B, C, H, W, pad, k, md, s1, s2, algo, _stream(in1)), what)
    return out


def correlation_plan(direction, dtype, shape, pad, k, md, s1, s2, algo=FN2_CORR_AUTO, ptrs=(0x1000,) * 5, out_bs=0):
    """fn2_debug_correlation_plan (needs no GPU): the CORR_KERNELS the dispatcher would try for this call, in its order, or the negative
    code the entry point returns before any launch.  ``ptrs``: addresses (never dereferenced) of in1, in2, out ("forward"; ``out_bs``: the
    output's batch stride, 0 = contiguous) or in1, in2, grad_out, grad_in1, grad_in2 ("backward"); ``algo`` >= 100: a debug variant."""
    ids = (ctypes.c_int * len(CORR_KERNELS))()
    ptrs = [ctypes.c_void_p(a) for a in tuple(ptrs) + (0,) * (5 - len(ptrs))]
    n = debug_lib().fn2_debug_correlation_plan({"forward": 0, "backward": 1}[direction], *ptrs, ctypes.c_int64(out_bs), dtype, *shape,
                                               pad, k, md, s1, s2, algo, ids, len(ids))
    return n if n < 0 else [CORR_KERNELS[i] for i in ids[:n]]


def correlation1d_output_shape(H, W, pad, md, s1, s2, sd=0):
    n, oh, ow = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    check(ext_lib().fn2x_correlation1d_output_shape(H, W, pad, md, s1, s2, sd, ctypes.byref(n), ctypes.byref(oh), ctypes.byref(ow)),
          "fn2x_correlation1d_output_shape")
    return n.value, oh.value, ow.value


def correlation1d_forward(in1, in2, pad, md, s1, s2, sd=0, algo=FN2X_CORR1D_AUTO, out=None):
    """fn2x_correlation1d_forward on device tensors; ``algo``: FN2X_CORR1D_AUTO / _GENERAL / _TILED; ``out``: a preallocated result."""
    import torch
    B, C, H, W = in1.shape
    nOut, oH, oW = correlation1d_output_shape(H, W, pad, md, s1, s2, sd)
    if out is None:
        out = torch.empty((B, nOut, oH, oW), dtype=in1.dtype, device=in1.device)
    with torch.cuda.device_of(in1):
        check(ext_lib().fn2x_correlation1d_forward(_p(in1), _p(in2), _p(out), _dtype_code(in1), B, C, H, W, pad, md, s1, s2, sd, algo,
                                                   _stream(in1)), "fn2x_correlation1d_forward")
    return out


def correlation1d_backward(in1, in2, gout, pad, md, s1, s2, sd=0, algo=FN2X_CORR1D_AUTO, out=None):
    import torch
    B, C, H, W = in1.shape
    g1, g2 = out if out is not None else (torch.empty_like(in1), torch.empty_like(in2))
    with torch.cuda.device_of(in1):
        check(ext_lib().fn2x_correlation1d_backward(_p(in1), _p(in2), _p(gout), _p(g1), _p(g2), _dtype_code(in1), B, C, H, W, pad, md,
                                                    s1, s2, sd, algo, _stream(in1)), "fn2x_correlation1d_backward")
    return g1, g2


def corr_lookup_forward(fmap1, fmap2, coords, radius, scale, algo=FN2L_LOOKUP_AUTO, out=None):
    """fn2l_corr_lookup_forward on contiguous device tensors; ``algo``: FN2L_LOOKUP_AUTO / _GENERAL / _STAGED; ``out``: a
    preallocated B x (2 radius + 1)^2 x H x W result."""
    import torch
    B, C, H, W = fmap1.shape
    H2, W2 = fmap2.shape[2:]
    assert fmap1.is_contiguous() and fmap2.is_contiguous() and coords.is_contiguous() and tuple(coords.shape) == (B, 2, H, W)
    if out is None:
        out = torch.empty((B, (2 * radius + 1) ** 2, H, W), dtype=fmap1.dtype, device=fmap1.device)
    with torch.cuda.device_of(fmap1):
        check(lookup_lib().fn2l_corr_lookup_forward(_p(fmap1), _p(fmap2), _p(coords), _p(out), _dtype_code(fmap1), B, C, H, W, H2, W2,
                                                    radius, ctypes.c_float(scale), algo, _stream(fmap1)), "fn2l_corr_lookup_forward")
    return out


def corr_lookup_backward(fmap1, fmap2, coords, gout, radius, scale, algo=FN2L_LOOKUP_AUTO, out=None):
    """fn2l_corr_lookup_backward: (grad_fmap1, grad_fmap2); ``out``: the two preallocated gradients (no pre-zeroing needed)."""
    import torch
    B, C, H, W = fmap1.shape
    H2, W2 = fmap2.shape[2:]
    assert fmap1.is_contiguous() and fmap2.is_contiguous() and coords.is_contiguous() and gout.is_contiguous()
    g1, g2 = out if out is not None else (torch.empty_like(fmap1), torch.empty_like(fmap2))
    with torch.cuda.device_of(fmap1):
        check(lookup_lib().fn2l_corr_lookup_backward(_p(fmap1), _p(fmap2), _p(coords), _p(gout), _p(g1), _p(g2), _dtype_code(fmap1), B, C,
                                                     H, W, H2, W2, radius, ctypes.c_float(scale), algo, _stream(fmap1)),
              "fn2l_corr_lookup_backward")
    return g1, g2


def _sample_geometry(levels, coords):
    """(the host arrays H2, W2 and the pointer array of ``levels``, B, H, W): levels are (B H W) x [1 x] H2_l x W2_l, contiguous."""
    B, _, H, W = coords.shape
    L = len(levels)
    assert coords.is_contiguous() and all(t.is_contiguous() and t.shape[0] == B * H * W for t in levels)
    H2, W2 = (ctypes.c_int * L)(*[t.shape[-2] for t in levels]), (ctypes.c_int * L)(*[t.shape[-1] for t in levels])
    return H2, W2, (ctypes.c_void_p * L)(*[t.data_ptr() for t in levels]), B, H, W


def corr_sample_forward(levels, coords, radius, out=None):
    """fn2p_corr_sample_forward on contiguous device tensors; ``out``: a preallocated B x (L (2 radius + 1)^2) x H x W result."""
    import torch
    H2, W2, ptrs, B, H, W = _sample_geometry(levels, coords)
    if out is None:
        out = torch.empty((B, len(levels) * (2 * radius + 1) ** 2, H, W), dtype=coords.dtype, device=coords.device)
    with torch.cuda.device_of(coords):
        check(sample_lib().fn2p_corr_sample_forward(ptrs, H2, W2, len(levels), _p(coords), _p(out), B, H, W, radius, _stream(coords)),
              "fn2p_corr_sample_forward")
    return out


def corr_sample_backward(levels, coords, gout, radius, out=None):
    """fn2p_corr_sample_backward: the gradients of ``levels`` (which give the shapes only); ``out``: the preallocated gradients
    (no pre-zeroing needed: every element is written)."""
    import torch
    grads = list(out) if out is not None else [torch.empty_like(t) for t in levels]
    H2, W2, ptrs, B, H, W = _sample_geometry(grads, coords)
    assert gout.is_contiguous() and [g.shape for g in grads] == [t.shape for t in levels]
    with torch.cuda.device_of(coords):
        check(sample_lib().fn2p_corr_sample_backward(H2, W2, len(grads), _p(coords), _p(gout), ptrs, B, H, W, radius, _stream(coords)),
              "fn2p_corr_sample_backward")
    return grads


def _sample1d_geometry(levels, coords):
    """(the host array W2 and the pointer array of ``levels``, coords' batch stride, B, H, W): levels are (B H W) x [1 x 1 x] W2_l,
    contiguous; coords is B x 2 x H x W (channel 0 is read in place) or B x 1 x H x W, contiguous."""
    B, C, H, W = coords.shape
    L = len(levels)
    assert coords.is_contiguous() and C in (1, 2) and all(t.is_contiguous() and t.shape[0] == B * H * W == t.numel() // t.shape[-1]
                                                          for t in levels)
    return (ctypes.c_int * L)(*[t.shape[-1] for t in levels]), (ctypes.c_void_p * L)(*[t.data_ptr() for t in levels]), C * H * W, B, H, W


def corr_sample1d_forward(levels, coords, radius, out=None):
    """fn2h_corr_sample1d_forward on contiguous device tensors; ``out``: a preallocated B x (L (2 radius + 1)) x H x W result."""
    import torch
    W2, ptrs, cbs, B, H, W = _sample1d_geometry(levels, coords)
    if out is None:
        out = torch.empty((B, len(levels) * (2 * radius + 1), H, W), dtype=coords.dtype, device=coords.device)
    with torch.cuda.device_of(coords):
        check(sample1d_lib().fn2h_corr_sample1d_forward(ptrs, W2, len(levels), _p(coords), cbs, _p(out), B, H, W, radius, _stream(coords)),
              "fn2h_corr_sample1d_forward")
    return out


def corr_sample1d_backward(levels, coords, gout, radius, out=None):
    """fn2h_corr_sample1d_backward: the gradients of ``levels`` (which give the shapes only); ``out``: the preallocated gradients
    (no pre-zeroing needed: every element is written)."""
    import torch
    grads = list(out) if out is not None else [torch.empty_like(t) for t in levels]
    W2, ptrs, cbs, B, H, W = _sample1d_geometry(grads, coords)
    assert gout.is_contiguous() and [g.shape for g in grads] == [t.shape for t in levels]
    with torch.cuda.device_of(coords):
        check(sample1d_lib().fn2h_corr_sample1d_backward(W2, len(grads), _p(coords), cbs, _p(gout), ptrs, B, H, W, radius, _stream(coords)),
              "fn2h_corr_sample1d_backward")
    return grads


def corr_pyramid_forward(fmap1, fmap2, num_levels, out=None):
    """fn2y_corr_pyramid_forward on contiguous float32 device tensors: the ``num_levels`` levels, (B H W) x 1 x (H2 >> l) x (W2 >> l);
    ``out``: the preallocated levels (no initialisation needed: every element is written)."""
    import torch
    B, C, H, W = fmap1.shape
    H2, W2 = fmap2.shape[2:]
    assert fmap1.is_contiguous() and fmap2.is_contiguous() and fmap2.shape[:2] == fmap1.shape[:2]
    levels = list(out) if out is not None else [torch.empty((B * H * W, 1, H2 >> l, W2 >> l), dtype=fmap1.dtype, device=fmap1.device)
                                                for l in range(num_levels)]
    assert all(t.is_contiguous() and t.numel() == B * H * W * (H2 >> l) * (W2 >> l) for l, t in enumerate(levels))
    ptrs = (ctypes.c_void_p * num_levels)(*[t.data_ptr() for t in levels])
    with torch.cuda.device_of(fmap1):
        check(pyramid_lib().fn2y_corr_pyramid_forward(_p(fmap1), _p(fmap2), ptrs, num_levels, B, C, H, W, H2, W2, _stream(fmap1)),
              "fn2y_corr_pyramid_forward")
    return levels


def corr_pyramid_fold(grads, shape, out=None):
    """fn2y_corr_pyramid_fold: G, (B H W) x H2 x W2, from the levels' gradients ``grads`` (contiguous float32 device tensors; None =
    a missing gradient, but not all of them); ``shape`` = (B, C, H, W, H2, W2); ``out``: a preallocated G (fully written)."""
    import torch
    B, C, H, W, H2, W2 = shape
    first = next(g for g in grads if g is not None)
    assert all(g is None or (g.is_contiguous() and g.numel() == B * H * W * (H2 >> l) * (W2 >> l)) for l, g in enumerate(grads))
    if out is None:
        out = torch.empty((B * H * W, H2, W2), dtype=first.dtype, device=first.device)
    ptrs = (ctypes.c_void_p * len(grads))(*[None if g is None else g.data_ptr() for g in grads])
    with torch.cuda.device_of(first):
        check(pyramid_lib().fn2y_corr_pyramid_fold(ptrs, len(grads), _p(out), B, C, H, W, H2, W2, _stream(first)), "fn2y_corr_pyramid_fold")
    return out


def _upsample_factor(flow, mask, factor):
    B, C, H, W = flow.shape
    assert flow.is_contiguous() and mask.is_contiguous() and tuple(mask.shape) == (B, 9 * factor * factor, H, W)
    return B, C, H, W


def convex_upsample_forward(flow, mask, factor, scale, out=None):
    """fn2u_convex_upsample_forward on contiguous device tensors (flow float32; mask float32, float16 or bfloat16); ``out``: a
    preallocated float32 B x C x factor H x factor W result."""
    import torch
    B, C, H, W = _upsample_factor(flow, mask, factor)
    if out is None:
        out = torch.empty((B, C, factor * H, factor * W), dtype=flow.dtype, device=flow.device)
    with torch.cuda.device_of(flow):
        check(upsample_lib().fn2u_convex_upsample_forward(_p(flow), _p(mask), _p(out), _dtype_code(mask), B, C, H, W, factor,
                                                          ctypes.c_float(scale), _stream(flow)), "fn2u_convex_upsample_forward")
    return out


def convex_upsample_backward(flow, mask, gout, factor, scale, out=None, workspace=None):
    """fn2u_convex_upsample_backward: (grad_flow, grad_mask); ``out``: the two preallocated gradients (no pre-zeroing needed);
    ``workspace``: a device buffer of fn2u_convex_upsample_backward_workspace_bytes, allocated here if None."""
    import torch
    B, C, H, W = _upsample_factor(flow, mask, factor)
    assert gout.is_contiguous() and tuple(gout.shape) == (B, C, factor * H, factor * W)
    gf, gm = out if out is not None else (torch.empty_like(flow), torch.empty_like(mask))
    if workspace is None:
        nbytes = upsample_lib().fn2u_convex_upsample_backward_workspace_bytes(B, C, H, W)
        workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=flow.device)
    with torch.cuda.device_of(flow):
        check(upsample_lib().fn2u_convex_upsample_backward(_p(flow), _p(mask), _p(gout), _p(gf), _p(gm), _p(workspace), _dtype_code(mask),
                                                           B, C, H, W, factor, ctypes.c_float(scale), _stream(flow)),
              "fn2u_convex_upsample_backward")
    return gf, gm


def correlation_forward_fused(in1, in2, buffer, channel_offset, negative_slope, pad, k, md, s1, s2, algo=FN2_CORR_AUTO):
    """LeakyReLU(correlation) written into channels [channel_offset, +nOut) of the contiguous N x Ctot x oH x oW `buffer`."""
    import torch
    B, C, H, W = in1.shape
    nOut, oH, oW = correlation_output_shape(H, W, pad, k, md, s1, s2)
    assert buffer.is_contiguous() and buffer.shape[0] == B and tuple(buffer.shape[2:]) == (oH, oW)
    assert 0 <= channel_offset and channel_offset + nOut <= buffer.shape[1]
    dst = ctypes.c_void_p(buffer.data_ptr() + channel_offset * oH * oW * buffer.element_size())
    with torch.cuda.device_of(in1):
        check(lib().fn2_correlation_forward_fused(_p(in1), _p(in2), dst, ctypes.c_int64(buffer.shape[1] * oH * oW),
                                                  ctypes.c_float(negative_slope), _dtype_code(in1), B, C, H, W, pad, k,
                                                  md, s1, s2, algo, _stream(in1)), "fn2_correlation_forward_fused")
    return buffer


def correlation_backward(in1, in2, gout, pad, k, md, s1, s2, algo=FN2_CORR_AUTO, out=None):
    import torch
    B, C, H, W = in1.shape
    g1, g2 = out if out is not None else (torch.empty_like(in1), torch.empty_like(in2))
    fn, what = ((debug_lib().fn2_debug_correlation_backward, "fn2_debug_correlation_backward") if algo >= 100 else
                (lib().fn2_correlation_backward_ex, "fn2_correlation_backward_ex"))
    with torch.cuda.device_of(in1):
        check(fn(_p(in1), _p(in2), _p(gout), _p(g1), _p(g2), _dtype_code(in1), B, C, H, W, pad, k, md, s1, s2, algo,
                 _stream(in1)), what)
    return g1, g2


def correlation_backward_fused(in1, in2, buffer, grad_buffer, channel_offset, negative_slope, pad, k, md, s1, s2, algo=FN2_CORR_AUTO):
    """Gradients of the correlation branch of cat((redir, leaky_relu(corr(in1, in2)))): `buffer` is the forward's concat buffer
    (correlation_forward_fused), `grad_buffer` the gradient wrt it, both contiguous N x Ctot x oH x oW."""
    import torch
    B, C, H, W = in1.shape
    nOut, oH, oW = correlation_output_shape(H, W, pad, k, md, s1, s2)
    assert buffer.is_contiguous() and grad_buffer.is_contiguous() and buffer.shape == grad_buffer.shape
    es = buffer.element_size()
    off = channel_offset * oH * oW * es
    wsb = lib().fn2_correlation_backward_fused_workspace_bytes(_dtype_code(in1), B, H, W, pad, k, md, s1, s2)
    ws = torch.empty(max(wsb // es, 1), dtype=in1.dtype, device=in1.device)
    g1, g2 = torch.empty_like(in1), torch.empty_like(in2)
    bs = ctypes.c_int64(buffer.shape[1] * oH * oW)
    with torch.cuda.device_of(in1):
        check(lib().fn2_correlation_backward_fused(_p(in1), _p(in2), ctypes.c_void_p(buffer.data_ptr() + off), bs,
                                                   ctypes.c_void_p(grad_buffer.data_ptr() + off), bs, ctypes.c_float(negative_slope),
                                                   _p(ws), ctypes.c_size_t(wsb), _p(g1), _p(g2), _dtype_code(in1), B, C, H, W,
                                                   pad, k, md, s1, s2, algo, _stream(in1)), "fn2_correlation_backward_fused")
    return g1, g2


def warp_diff_norm_cat(pair, flow, div_flow=20.0, bilinear=True):
    """cat(pair, warp(pair[:, C:], flow), flow / div_flow, ||pair[:, :C] - warped||_2) (models.py:133-138) in one pass."""
    import torch
    B, C2, H, W = pair.shape
    C = C2 // 2
    assert pair.is_contiguous() and flow.is_contiguous() and pair.dtype == torch.float32 and C2 == 2 * C
    out = torch.empty((B, 3 * C + 3, H, W), dtype=pair.dtype, device=pair.device)
    with torch.cuda.device_of(pair):
        check(lib().fn2_warp_diff_norm_cat(_p(pair), _p(flow), _p(out), ctypes.c_float(div_flow), B, C, H, W,
                                           1 if bilinear else 0, _stream(pair)), "fn2_warp_diff_norm_cat")
    return out


def warp_diff_norm_cat_backward(pair, flow, out_cat, grad_cat, div_flow=20.0, bilinear=True, want_grad_pair=True):
    """fn2_warp_diff_norm_cat_backward through ctypes: returns (grad_pair or None, grad_flow)."""
    import torch
    B, C2, H, W = pair.shape
    C = C2 // 2
    assert pair.is_contiguous() and flow.is_contiguous() and out_cat.is_contiguous() and grad_cat.is_contiguous()
    gpair = torch.full_like(pair, float("nan")) if want_grad_pair else None
    gflow = torch.full_like(flow, float("nan"))
    with torch.cuda.device_of(pair):
        check(lib().fn2_warp_diff_norm_cat_backward(_p(pair), _p(flow), _p(out_cat), _p(grad_cat), _p(gpair) if want_grad_pair else None,
                                                    _p(gflow), ctypes.c_float(div_flow), B, C, H, W, 1 if bilinear else 0,
                                                    _stream(pair)), "fn2_warp_diff_norm_cat_backward")
    return gpair, gflow


def warp_diff_norm(pair, flow, bilinear=True):
    """||pair[:, :C] - warp(pair[:, C:], flow)||_2 (models.py:157-161): B x 1 x H x W."""
    import torch
    B, C2, H, W = pair.shape
    assert pair.is_contiguous() and flow.is_contiguous() and pair.dtype == torch.float32
    out = torch.full((B, 1, H, W), float("nan"), dtype=pair.dtype, device=pair.device)
    with torch.cuda.device_of(pair):
        check(lib().fn2_warp_diff_norm(_p(pair), _p(flow), _p(out), B, C2 // 2, H, W, 1 if bilinear else 0, _stream(pair)), "fn2_warp_diff_norm")
    return out


def warp_diff_norm_backward(pair, flow, norm, grad_norm, bilinear=True):
    import torch
    B, C2, H, W = pair.shape
    assert pair.is_contiguous() and flow.is_contiguous() and norm.is_contiguous() and grad_norm.is_contiguous()
    gflow = torch.full_like(flow, float("nan"))
    with torch.cuda.device_of(pair):
        check(lib().fn2_warp_diff_norm_backward(_p(pair), _p(flow), _p(norm), _p(grad_norm), _p(gflow), B, C2 // 2, H, W,
                                                1 if bilinear else 0, _stream(pair)), "fn2_warp_diff_norm_backward")
    return gflow


def _check16(pair, *others):
    import torch
    assert pair.dtype in (torch.float16, torch.bfloat16) and pair.shape[1] % 2 == 0
    for t in (pair,) + others:
        assert t.is_contiguous() and t.dtype == pair.dtype


def warp_diff_norm_cat_16(pair, flow, div_flow=20.0, bilinear=True, out=None):
    """fn2_warp_diff_norm_cat_16: the concat row on half / bfloat16 tensors as they are (``out``: a preallocated result)."""
    import torch
    B, C2, H, W = pair.shape
    _check16(pair, flow)
    if out is None:
        out = torch.full((B, 3 * (C2 // 2) + 3, H, W), float("nan"), dtype=pair.dtype, device=pair.device)
    with torch.cuda.device_of(pair):
        check(lib().fn2_warp_diff_norm_cat_16(_p(pair), _p(flow), _p(out), _dtype_code(pair), ctypes.c_float(div_flow), B, C2 // 2, H, W,
                                              1 if bilinear else 0, _stream(pair)), "fn2_warp_diff_norm_cat_16")
    return out


def warp_diff_norm_cat_backward_16(pair, flow, grad_cat, div_flow=20.0, bilinear=True):
    """fn2_warp_diff_norm_cat_backward_16: the flow gradient of the concat row, the warp and the norm recomputed."""
    import torch
    B, C2, H, W = pair.shape
    _check16(pair, flow, grad_cat)
    gflow = torch.full_like(flow, float("nan"))
    with torch.cuda.device_of(pair):
        check(lib().fn2_warp_diff_norm_cat_backward_16(_p(pair), _p(flow), _p(grad_cat), _p(gflow), _dtype_code(pair),
                                                       ctypes.c_float(div_flow), B, C2 // 2, H, W, 1 if bilinear else 0, _stream(pair)),
              "fn2_warp_diff_norm_cat_backward_16")
    return gflow


def warp_diff_norm_16(pair, flow, bilinear=True):
    import torch
    B, C2, H, W = pair.shape
    _check16(pair, flow)
    out = torch.full((B, 1, H, W), float("nan"), dtype=pair.dtype, device=pair.device)
    with torch.cuda.device_of(pair):
        check(lib().fn2_warp_diff_norm_16(_p(pair), _p(flow), _p(out), _dtype_code(pair), B, C2 // 2, H, W, 1 if bilinear else 0,
                                          _stream(pair)), "fn2_warp_diff_norm_16")
    return out


def warp_diff_norm_backward_16(pair, flow, grad_norm, bilinear=True):
    import torch
    B, C2, H, W = pair.shape
    _check16(pair, flow, grad_norm)
    gflow = torch.full_like(flow, float("nan"))
    with torch.cuda.device_of(pair):
        check(lib().fn2_warp_diff_norm_backward_16(_p(pair), _p(flow), _p(grad_norm), _p(gflow), _dtype_code(pair), B, C2 // 2, H, W,
                                                   1 if bilinear else 0, _stream(pair)), "fn2_warp_diff_norm_backward_16")
    return gflow


def multiscale_l1_epe(outputs, target, weights, start_scale=4, div_flow=0.05, want_grads=False, grad_scale=1.0, norm=1):
    """SURVEY.md 8f N3 (losses.py:52-86): returns (sums, grads).  sums is a device tensor of 2*n floats --
    sums[i] = sum |out_i - AvgPool_{k_i}(div_flow * target)|, sums[n+i] = sum of the per-pixel channel 2-norms; grads
    (if requested) are grad_scale * weights[i] / numel(out_i) * sign(out_i - t_i) for norm = 1 (L1) and
    grad_scale * weights[i] / (numel(out_i) / 2) * (out_i - t_i) / ||out_i - t_i||_2 for norm = 2 (L2, losses.py:64-67)."""
    import torch
    n = len(outputs)
    B, two, H, W = target.shape
    assert two == 2 and target.is_contiguous() and target.dtype == torch.float32
    for i, o in enumerate(outputs):
        k = start_scale << i
        assert o.is_contiguous() and o.dtype == torch.float32 and tuple(o.shape) == (B, 2, H // k, W // k), (i, o.shape)
    sums = torch.empty(2 * n, dtype=torch.float32, device=target.device)
    grads = [torch.empty_like(o) for o in outputs] if want_grads else None
    wsb = lib().fn2_multiscale_workspace_bytes(B, H, W, start_scale, n)
    ws = torch.empty(max(wsb // 4, 1), dtype=torch.float32, device=target.device)
    outs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outputs])
    gptr = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads]) if want_grads else None
    wts = (ctypes.c_float * n)(*[float(w) for w in weights])
    with torch.cuda.device_of(target):
        check(lib().fn2_multiscale_loss(outs, _p(target), _p(sums), gptr, wts, ctypes.c_float(grad_scale), int(norm), B, H, W,
                                        start_scale, n, ctypes.c_float(div_flow), _p(ws), ctypes.c_size_t(wsb),
                                        _stream(target)), "fn2_multiscale_loss")
    return sums, grads


def _splat_shape(inp, flow):
    B, C, H, W = inp.shape
    assert inp.is_contiguous() and flow.is_contiguous() and tuple(flow.shape) == (B, 2, H, W)
    return B, C, H, W


def forward_warp_forward(inp, flow, algo=FN2S_AUTO, out=None):
    """fn2s_forward_warp_forward on contiguous float32 device tensors; ``algo``: FN2S_AUTO / _GENERAL / _TILED; ``out``: a
    preallocated result (cleared by the entry point)."""
    import torch
    B, C, H, W = _splat_shape(inp, flow)
    if out is None:
        out = torch.empty_like(inp)
    with torch.cuda.device_of(inp):
        check(splat_lib().fn2s_forward_warp_forward(_p(inp), _p(flow), _p(out), B, C, H, W, algo, _stream(inp)), "fn2s_forward_warp_forward")
    return out


def forward_warp_forward_det(inp, flow, out=None, workspace=None):
    """fn2s_forward_warp_forward_det; ``workspace``: a device buffer of fn2s_forward_warp_forward_det_workspace_bytes (no
    initialisation needed), allocated here if None."""
    import torch
    B, C, H, W = _splat_shape(inp, flow)
    if out is None:
        out = torch.empty_like(inp)
    if workspace is None:
        nbytes = splat_lib().fn2s_forward_warp_forward_det_workspace_bytes(B, C, H, W)
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=inp.device)
    with torch.cuda.device_of(inp):
        check(splat_lib().fn2s_forward_warp_forward_det(_p(inp), _p(flow), _p(out), _p(workspace), workspace.numel() * workspace.element_size(),
                                                        B, C, H, W, _stream(inp)), "fn2s_forward_warp_forward_det")
    return out


def forward_warp_backward(inp, flow, gout, want_input=True, want_flow=True, out=(None, None)):
    """fn2s_forward_warp_backward: (grad_input, grad_flow), None for one that is not wanted (its pointer is passed as NULL); ``out``:
    preallocated results."""
    import torch
    B, C, H, W = _splat_shape(inp, flow)
    assert gout.is_contiguous() and gout.shape == inp.shape
    gi = (out[0] if out[0] is not None else torch.empty_like(inp)) if want_input else None
    gf = (out[1] if out[1] is not None else torch.empty_like(flow)) if want_flow else None
    null = ctypes.c_void_p(0)
    with torch.cuda.device_of(inp):
        check(splat_lib().fn2s_forward_warp_backward(_p(inp), _p(flow), _p(gout), _p(gi) if want_input else null, _p(gf) if want_flow else null,
                                                     B, C, H, W, _stream(inp)), "fn2s_forward_warp_backward")
    return gi, gf


def _census_shape(im1, im2):
    N, C, H, W = im1.shape
    assert im1.is_contiguous() and im2.is_contiguous() and im2.shape == im1.shape
    return N, C, H, W


def census_forward(im1, im2, max_distance=3, scale=255.0, normalize=True, out=None):
    """fn2c_census_forward on contiguous float32 device tensors; ``out``: a preallocated N x 1 x H x W result (fully written)."""
    import torch
    N, C, H, W = _census_shape(im1, im2)
    if out is None:
        out = torch.empty((N, 1, H, W), dtype=im1.dtype, device=im1.device)
    with torch.cuda.device_of(im1):
        check(census_lib().fn2c_census_forward(_p(im1), _p(im2), _p(out), N, C, H, W, int(max_distance), float(scale), 1 if normalize else 0,
                                               _stream(im1)), "fn2c_census_forward")
    return out


def census_backward(im1, im2, gout, max_distance=3, scale=255.0, normalize=True, want1=True, want2=True, grads=(None, None)):
    """fn2c_census_backward: (grad_im1, grad_im2), None for one that is not wanted (its pointer is passed as NULL); ``grads``:
    preallocated results."""
    import torch
    N, C, H, W = _census_shape(im1, im2)
    assert gout.is_contiguous() and tuple(gout.shape) == (N, 1, H, W)
    g1 = (grads[0] if grads[0] is not None else torch.empty_like(im1)) if want1 else None
    g2 = (grads[1] if grads[1] is not None else torch.empty_like(im2)) if want2 else None
    null = ctypes.c_void_p(0)
    with torch.cuda.device_of(im1):
        check(census_lib().fn2c_census_backward(_p(im1), _p(im2), _p(gout), _p(g1) if want1 else null, _p(g2) if want2 else null, N, C, H, W,
                                                int(max_distance), float(scale), 1 if normalize else 0, _stream(im1)), "fn2c_census_backward")
    return g1, g2


def _smooth_shape(flow, image):
    N, F, H, W = flow.shape
    assert flow.is_contiguous() and image.is_contiguous() and image.shape[0] == N and tuple(image.shape[2:]) == (H, W)
    return N, F, image.shape[1], H, W


def smoothness_forward(flow, image, order=1, edge_weighting="exponential", alpha=150.0, eps=0.001, out=None):
    """fn2m_smoothness_forward on contiguous float32 device tensors; ``out``: a preallocated N x 2 x H x W result (fully written)."""
    import torch
    N, F, C, H, W = _smooth_shape(flow, image)
    if out is None:
        out = torch.empty((N, 2, H, W), dtype=flow.dtype, device=flow.device)
    with torch.cuda.device_of(flow):
        check(smooth_lib().fn2m_smoothness_forward(_p(flow), _p(image), _p(out), N, F, C, H, W, int(order), FN2M_EDGE[edge_weighting],
                                                   float(alpha), float(eps), _stream(flow)), "fn2m_smoothness_forward")
    return out


def smoothness_backward(flow, image, gout, order=1, edge_weighting="exponential", alpha=150.0, eps=0.001, out=None):
    """fn2m_smoothness_backward: grad_flow; ``out``: a preallocated N x F x H x W result (fully written)."""
    import torch
    N, F, C, H, W = _smooth_shape(flow, image)
    assert gout.is_contiguous() and tuple(gout.shape) == (N, 2, H, W)
    if out is None:
        out = torch.empty_like(flow)
    with torch.cuda.device_of(flow):
        check(smooth_lib().fn2m_smoothness_backward(_p(flow), _p(image), _p(gout), _p(out), N, F, C, H, W, int(order), FN2M_EDGE[edge_weighting],
                                                    float(alpha), float(eps), _stream(flow)), "fn2m_smoothness_backward")
    return out


def ssim_forward(im1, im2, max_distance=1, c1=1e-4, c2=9e-4, border="zero", out=None):
    """fn2i_ssim_forward on contiguous float32 device tensors; ``out``: a preallocated N x C x H x W result (fully written)."""
    import torch
    N, C, H, W = _census_shape(im1, im2)
    if out is None:
        out = torch.empty_like(im1)
    with torch.cuda.device_of(im1):
        check(ssim_lib().fn2i_ssim_forward(_p(im1), _p(im2), _p(out), N, C, H, W, int(max_distance), float(c1), float(c2), FN2I_BORDER[border],
                                           _stream(im1)), "fn2i_ssim_forward")
    return out


def ssim_backward(im1, im2, gout, max_distance=1, c1=1e-4, c2=9e-4, border="zero", want1=True, want2=True, grads=(None, None)):
    """fn2i_ssim_backward: (grad_im1, grad_im2), None for one that is not wanted (its pointer is passed as NULL); ``grads``:
    preallocated results."""
    import torch
    N, C, H, W = _census_shape(im1, im2)
    assert gout.is_contiguous() and gout.shape == im1.shape
    g1 = (grads[0] if grads[0] is not None else torch.empty_like(im1)) if want1 else None
    g2 = (grads[1] if grads[1] is not None else torch.empty_like(im2)) if want2 else None
    null = ctypes.c_void_p(0)
    with torch.cuda.device_of(im1):
        check(ssim_lib().fn2i_ssim_backward(_p(im1), _p(im2), _p(gout), _p(g1) if want1 else null, _p(g2) if want2 else null, N, C, H, W,
                                            int(max_distance), float(c1), float(c2), FN2I_BORDER[border], _stream(im1)), "fn2i_ssim_backward")
    return g1, g2
