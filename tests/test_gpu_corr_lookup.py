"""CorrLookup on the GPU (csrc/corr_lookup.hip through libflownet2_hip_lookup.so, corr_lookup_cuda and the Python layer).

1. the general forward and grad_fmap1 lie within the header's bounds of the float64 reference (tests/corr_lookup_ref.py);
2. the staged kernels (FN2L_LOOKUP_STAGED) have the general kernels' bits on every coordinate family, at pointer offsets of 0 and
   1 element;
3. grad_fmap2 lies within its any-order bound and is exactly zero where the reference has no term;
4. every door (AUTO at the C ABI, the pybind module, the autograd Function and Module, another stream, non-contiguous inputs)
   gives those bits;
5. AlternateCorrBlock against RAFT's pooled all-pairs composition in float64, channel and level order pinned by a one-pixel fmap2;
6. coords.requires_grad, a second backward and deterministic mode raise (warn_only: warns);
7. forward + backward allocate the output and the two gradients, nothing of the all-pairs volume's size;
8. the forward is not slower than the composition's;  9. AUTO is the kernel the header names;
10. forward + backward captured into a hipGraph: every replay clears grad_fmap2 before the scatter.

Every output is pre-filled with NaN (an unwritten element shows) and sits inside a larger allocation filled with a sentinel that
must be untouched afterwards.  Feature maps are the finite families of corr_contract_ref.family_inputs.

Coordinate families (fmap2 pixels; _coords):
  a  the identity scaled onto fmap2 plus a smooth fractional flow, |flow| < 3;
  b  integers, negative ones and ones beyond the far border included;
  c  fractions just below 0, just below -r - 1 and just above W2 - 1 + r (floor versus truncation; windows cut on each side);
  d  everything outside, at -100 and W2 + 100: the output is exactly zero;
  e1 family a with one pixel per tile moved 40 pixels away;  e2 uniform random coordinates (both: the fallback path);
  f  every tile's bounding box exactly at the header's staged limit (fx in x, fy in y) and one over it (fx1, fy1), built from
     the published macros;
  g  family a with NaN, +-inf, +-1e30 and +-2^20 in at most 5 % of the pixels."""
import statistics

import numpy as np
import pytest
import torch

import corr_contract_ref as R
import corr_lookup_ref as RL

pytestmark = pytest.mark.gpu

SENTINEL = -7777.0
GUARD = 64
AUTO, GENERAL, STAGED = 0, 1, 2
M = RL.header_macros()
TW, TH, PW, PH = M["FN2L_TILE_W"], M["FN2L_TILE_H"], M["FN2L_PATCH_W"], M["FN2L_PATCH_H"]
STAGED_MAX_R = M["FN2L_STAGED_MAX_RADIUS"]

FMAP1 = [(13, 19), (3, 5)]
FMAP2 = [(13, 19), (6, 9), (3, 4), (1, 2)]
CHANNELS = [1, 5, 34]
COORD_FAMILIES = ["a", "b", "c", "d", "e1", "e2", "fx", "fx1", "fy", "fy1", "g"]
FEATURE_FAMILIES = (1, 2, 3, 5, 6, 7, 8)   # the finite ones that do not tie in2 to in1


# ------------------------------------------------------------------ helpers
def _guarded(shape, dev, off=0):
    n = int(np.prod(shape))
    whole = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    view = whole[GUARD + off:GUARD + off + n].view(shape)
    view.fill_(float("nan"))
    assert view.data_ptr() % 16 == (off * 4) % 16
    return view, whole


def _untouched(whole, view, what):
    n, lo = view.numel(), view.storage_offset()
    assert bool((whole[:lo] == SENTINEL).all()) and bool((whole[lo + n:] == SENTINEL).all()), f"{what}: wrote outside its output"


def _place(t, dev, off=0):
    if not off:
        return t.to(dev)
    flat = torch.empty(t.numel() + off, dtype=t.dtype, device=dev)
    v = flat[off:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off * 4
    return v


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, what
    assert not torch.isnan(want).any(), f"{what}: the general kernel left or produced NaN"
    bad = got.contiguous().view(torch.int32) != want.contiguous().view(torch.int32)
    n = int(bad.sum())
    if n:
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ from the general kernel; first at flat index {i}: "
                             f"{float(got.flatten()[i])!r} vs {float(want.flatten()[i])!r}")


def _features(fam, C, s1, s2, seed, B=2):
    f1 = R.family_inputs(fam, (B, C) + tuple(s1), seed)[0]
    f2 = R.family_inputs(fam, (B, C) + tuple(s2), seed + 1)[1]
    assert bool(torch.isfinite(f1).all()) and bool(torch.isfinite(f2).all())
    return f1, f2


def _coords(fam, B, H, W, H2, W2, r, seed):
    """B x 2 x H x W float32 coordinates of one family (module docstring)."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ident = np.stack([xs * (W2 / W), ys * (H2 / H)])[None].repeat(B, 0)
    ph = rng.uniform(0, 6.28, (B, 2, 1, 1))
    flow = 2.9 * np.sin(0.23 * xs[None, None] + 0.31 * ys[None, None] + ph) * np.cos(0.17 * ys[None, None] - ph)
    a = ident + flow
    lim = np.array([W2, H2], dtype=np.float64)[None, :, None, None]
    if fam == "a":
        c = a
    elif fam == "b":
        c = np.stack([rng.integers(-r - 2, W2 + r + 2, (B, H, W)), rng.integers(-r - 2, H2 + r + 2, (B, H, W))], 1).astype(np.float64)
    elif fam == "c":
        c = np.empty((B, 2, H, W))
        for k, n in enumerate((W2, H2)):
            vals = np.array([-2.0 ** -12, -(r + 1) - 2.0 ** -10, n - 1 + r + 2.0 ** -10, -0.3, n - 0.7, 0.4])
            c[:, k] = vals[rng.integers(0, len(vals), (B, H, W))]
    elif fam == "d":
        c = np.where(rng.random((B, 2, H, W)) < 0.5, -100.0, lim + 100.0)
        c[:, 1] = np.where(rng.random((B, H, W)) < 0.3, a[:, 1], c[:, 1])   # (one axis outside is enough)
    elif fam == "e1":
        c = a.copy()
        c[:, :, ::TH, ::TW] += 40.0
    elif fam == "e2":
        c = np.stack([rng.uniform(-r - 2, W2 + r + 2, (B, H, W)), rng.uniform(-r - 2, H2 + r + 2, (B, H, W))], 1)
    elif fam in ("fx", "fx1", "fy", "fy1"):
        # every pixel of a tile at one place, the tile's first pixel moved so that the box is the limit (or one more) wide
        c = np.broadcast_to(np.array([1.5, 0.25])[None, :, None, None] + rng.uniform(0, 0.5, (B, 2, 1, 1)), (B, 2, H, W)).copy()
        ax, patch = (0, PW) if fam[1] == "x" else (1, PH)
        c[:, ax, ::TH, ::TW] += patch - (2 * r + 2) + (1 if fam.endswith("1") else 0)
    elif fam == "g":
        c = a.copy()
        bad = [np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 20, -(2.0 ** 20)]
        n = min(int(0.05 * B * H * W), 2 * len(bad))
        assert n >= 1
        for k, p in enumerate(rng.choice(B * H * W, n, replace=False)):
            b, y, x = np.unravel_index(p, (B, H, W))
            c[b, k % 2, y, x] = bad[(k // 2 + k) % len(bad)]
    else:
        raise AssertionError(fam)
    return torch.from_numpy(np.ascontiguousarray(c).astype(np.float32))


def _fwd(f1, f2, co, r, scale, algo, off=0, what="forward"):
    import fn2_capi
    B, C, H, W = f1.shape
    out, whole = _guarded((B, (2 * r + 1) ** 2, H, W), f1.device, off)
    fn2_capi.corr_lookup_forward(f1, f2, co, r, scale, algo=algo, out=out)
    _untouched(whole, out, what)
    assert not torch.isnan(out).any(), f"{what}: elements left unwritten"
    return out


def _bwd(f1, f2, co, go, r, scale, algo, off=0, what="backward"):
    import fn2_capi
    (g1, w1), (g2, w2) = _guarded(f1.shape, f1.device, off), _guarded(f2.shape, f1.device, off)
    fn2_capi.corr_lookup_backward(f1, f2, co, go, r, scale, algo=algo, out=(g1, g2))
    _untouched(w1, g1, what + " grad_fmap1")
    _untouched(w2, g2, what + " grad_fmap2")
    assert not torch.isnan(g1).any() and not torch.isnan(g2).any(), f"{what}: elements left unwritten"
    return g1, g2


def _within(got, exact, delta, what):
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - exact)
    ratio = float((err / np.maximum(delta, 1e-300)).max())
    assert (err <= delta).all(), f"{what}: {ratio:.3g} x the bound"
    return ratio


# ------------------------------------------------------------------ 1, 3: the general kernels inside the header's bounds
# (r, C, fmap1, fmap2, coordinate family, feature family): every r, C, shape and family at least once; the float64 reference
# walks every tap and corner, so the r = 8 cases stay few
BOUND_CASES = [
    (0, 5, (13, 19), (13, 19), "a", 1), (0, 1, (3, 5), (1, 2), "c", 2), (0, 34, (13, 19), (6, 9), "b", 3), (0, 5, (13, 19), (3, 4), "g", 5),
    (1, 34, (13, 19), (13, 19), "a", 2), (1, 5, (3, 5), (6, 9), "c", 6), (1, 1, (13, 19), (1, 2), "e2", 7), (1, 5, (13, 19), (13, 19), "d", 1),
    (3, 5, (13, 19), (13, 19), "c", 8), (3, 34, (3, 5), (3, 4), "a", 1), (3, 1, (13, 19), (6, 9), "g", 3), (3, 5, (13, 19), (13, 19), "fx1", 2),
    (4, 34, (13, 19), (13, 19), "a", 6), (4, 5, (13, 19), (6, 9), "c", 5), (4, 1, (3, 5), (1, 2), "b", 1), (4, 5, (13, 19), (3, 4), "e1", 7),
    (4, 5, (13, 19), (13, 19), "g", 8), (4, 5, (13, 19), (13, 19), "fy", 3),
    (8, 5, (13, 19), (13, 19), "a", 2), (8, 34, (3, 5), (6, 9), "c", 1), (8, 1, (13, 19), (1, 2), "g", 6),
]


@pytest.mark.parametrize("case", BOUND_CASES, ids=lambda c: "r%d-C%d-%dx%d-%dx%d-%s-fam%d" % (c[0], c[1], *c[2], *c[3], c[4], c[5]))
def test_general_kernels_inside_the_headers_bounds(dev, case):
    r, C, s1, s2, cfam, ffam = case
    B, (H, W), (H2, W2) = 2, s1, s2
    f1, f2 = _features(ffam, C, s1, s2, seed=r + C)
    co = _coords(cfam, B, H, W, H2, W2, r, seed=7 * r + C)
    scale = float(C) ** -0.5
    go = R.grad_output("normal", (B, (2 * r + 1) ** 2, H, W), seed=r + 3)
    what = f"{case}"
    exact, S = RL.forward(f1.numpy(), f2.numpy(), co.numpy(), r, scale)
    (e1, S1), (e2, S2, n2) = RL.backward(f1.numpy(), f2.numpy(), co.numpy(), go.numpy(), r, scale)
    f1d, f2d, cod, god = f1.to(dev), f2.to(dev), co.to(dev), go.to(dev)
    out = _fwd(f1d, f2d, cod, r, scale, GENERAL, what=what)
    g1, g2 = _bwd(f1d, f2d, cod, god, r, scale, GENERAL, what=what)
    ratios = (_within(out, exact, RL.delta_forward(exact, S, C, scale), what + " forward"),
              _within(g1, e1, RL.delta_grad1(e1, S1, r, scale), what + " grad_fmap1"),
              _within(g2, e2, RL.delta_grad2(e2, S2, n2, scale), what + " grad_fmap2"))
    print(f"  {what}: error / bound forward {ratios[0]:.3f}, grad_fmap1 {ratios[1]:.3f}, grad_fmap2 {ratios[2]:.3f}")
    # exactly zero where the reference has no term
    assert bool((out.cpu()[torch.from_numpy(S == 0)] == 0).all()) and bool((g1.cpu()[torch.from_numpy(S1 == 0)] == 0).all())
    assert bool((g2.cpu()[torch.from_numpy(n2 == 0)] == 0).all()), what + ": grad_fmap2 is not exactly zero where no term arrives"
    ok = torch.from_numpy(RL.decode(co.numpy())[4])
    if cfam == "d":
        assert bool((out == 0).all()) and bool((g1 == 0).all()) and bool((g2 == 0).all())
    if cfam == "g":   # pixels without taps: zeros out, no gradient in; the others as if the bad pixels were not there
        assert not bool(ok.all())
        assert bool((out.cpu().permute(0, 2, 3, 1)[~ok] == 0).all()) and bool((g1.cpu().permute(0, 2, 3, 1)[~ok] == 0).all())
        clean = _coords("a", B, H, W, H2, W2, r, seed=7 * r + C).to(dev)
        same = _fwd(f1d, f2d, clean, r, scale, GENERAL, what=what)
        assert torch.equal(out.cpu().permute(0, 2, 3, 1)[ok], same.cpu().permute(0, 2, 3, 1)[ok]), what + ": a bad pixel changed another"
    else:
        assert bool(ok.all())


# ------------------------------------------------------------------ 2: staged == general, bit for bit
@pytest.mark.parametrize("r", [0, 1, 3, 4])
@pytest.mark.parametrize("s1", FMAP1, ids=lambda s: "%dx%d" % s)
def test_staged_has_the_general_kernels_bits(dev, s1, r):
    """Forward and grad_fmap1, every fmap2 shape, channel count and coordinate family, outputs and inputs at pointer offsets of
    0 and 1 element.  (grad_fmap2 is the atomic scatter under every selector: test 3.)"""
    B, (H, W) = 2, s1
    for n, s2 in enumerate(FMAP2):
        H2, W2 = s2
        for C in CHANNELS:
            f1, f2 = _features(FEATURE_FAMILIES[(n + C + r) % len(FEATURE_FAMILIES)], C, s1, s2, seed=r + C)
            scale = float(C) ** -0.5
            go = R.grad_output("normal", (B, (2 * r + 1) ** 2, H, W), seed=C)
            for cfam in COORD_FAMILIES:
                co = _coords(cfam, B, H, W, H2, W2, r, seed=11 * r + C + n)
                for off in (0, 1):
                    what = f"r {r} C {C} {s1} {s2} family {cfam} offset {off}"
                    f1d, f2d, cod, god = (_place(t, dev, off) for t in (f1, f2, co, go))
                    want = _fwd(f1d, f2d, cod, r, scale, GENERAL, off, what)
                    _same_bits(_fwd(f1d, f2d, cod, r, scale, STAGED, off, what), want, what + " forward")
                    w1, _ = _bwd(f1d, f2d, cod, god, r, scale, GENERAL, off, what)
                    g1, _ = _bwd(f1d, f2d, cod, god, r, scale, STAGED, off, what)
                    _same_bits(g1, w1, what + " grad_fmap1")
                    if cfam == "d":
                        assert bool((want == 0).all()) and bool((w1 == 0).all()), what


def test_staged_limit_families_straddle_the_limit():
    """Family f is built from the header's macros: the tile's first pixel sits exactly patch - (2 r + 2) (or one more) from the
    others, so floor(coords) spans the staged limit (or exceeds it by one)."""
    for r in (0, 1, 3, 4):
        for fam, ax, patch in (("fx", 0, PW), ("fy", 1, PH)):
            for extra in (0, 1):
                co = _coords(fam + ("1" if extra else ""), 2, 13, 19, 13, 19, r, seed=r).numpy()
                fl = np.floor(co[:, ax, :TH, :TW])
                span = fl.max(axis=(1, 2)) - fl.min(axis=(1, 2))
                assert (span + 2 * r + 2 == patch + extra).all(), (r, fam, extra, span)


# ------------------------------------------------------------------ 4: every door
def test_every_door_gives_the_auto_bits(dev):
    import corr_lookup_cuda
    import fn2_capi
    from networks.correlation_package import CorrLookup, CorrLookupFunction
    r, C, s1, s2 = 3, 5, (13, 19), (6, 9)
    B, (H, W), (H2, W2) = 2, s1, s2
    f1, f2 = _features(1, C, s1, s2, seed=4)
    co = _coords("a", B, H, W, H2, W2, r, seed=5)
    go = R.grad_output("normal", (B, 49, H, W), seed=6)
    scale = float(C) ** -0.5
    f1d, f2d, cod, god = f1.to(dev), f2.to(dev), co.to(dev), go.to(dev)
    want = _fwd(f1d, f2d, cod, r, scale, AUTO)
    _same_bits(want, _fwd(f1d, f2d, cod, r, scale, GENERAL), "AUTO against the general kernel")
    w1, w2 = _bwd(f1d, f2d, cod, god, r, scale, AUTO)
    (_, _), (e2, S2, n2) = RL.backward(f1.numpy(), f2.numpy(), co.numpy(), go.numpy(), r, scale)
    d2 = RL.delta_grad2(e2, S2, n2, scale)

    def grads(g1, g2, what):   # grad_fmap1: the bits; grad_fmap2 (atomics, arrival order): the any-order bound
        _same_bits(g1, w1, what + " grad_fmap1")
        _within(g2, e2, d2, what + " grad_fmap2")

    grads(w1, w2, "C ABI")
    o = torch.empty(0, device=dev)
    corr_lookup_cuda.forward(f1d, f2d, cod, o, r, scale)
    _same_bits(o, want, "corr_lookup_cuda.forward")
    p1, p2 = torch.empty(0, device=dev), torch.empty(0, device=dev)
    corr_lookup_cuda.backward(f1d, f2d, cod, god, p1, p2, r, scale)
    grads(p1, p2, "corr_lookup_cuda.backward")
    _same_bits(corr_lookup_cuda.forward_alloc(f1d, f2d, cod, r, scale), want, "forward_alloc")
    grads(*corr_lookup_cuda.backward_alloc(f1d, f2d, cod, god, r, scale), "backward_alloc")
    doors = (("corr_lookup_cuda.apply", lambda x, y, c: corr_lookup_cuda.apply(x, y, c, r, scale)),
             ("CorrLookupFunction.apply", lambda x, y, c: CorrLookupFunction.apply(x, y, c, r, scale)),
             ("CorrLookup", CorrLookup(r)), ("CorrLookup(scale)", CorrLookup(r, scale)))
    for name, fn in doors:
        a, b = f1d.clone().requires_grad_(True), f2d.clone().requires_grad_(True)
        out = fn(a, b, cod)
        _same_bits(out.detach(), want, name)
        out.backward(god)
        grads(a.grad, b.grad, name)
    # non-contiguous inputs: transposed storage of all four tensors
    nc = [t.transpose(2, 3).contiguous().transpose(2, 3) for t in (f1d, f2d, cod, god)]
    assert not any(t.is_contiguous() for t in nc)
    a, b = nc[0].clone(memory_format=torch.preserve_format).requires_grad_(True), nc[1].clone(memory_format=torch.preserve_format).requires_grad_(True)
    out = CorrLookup(r)(a, b, nc[2])
    _same_bits(out.detach(), want, "non-contiguous inputs")
    out.backward(nc[3])
    grads(a.grad.contiguous(), b.grad.contiguous(), "non-contiguous inputs")
    # a non-default stream
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        so = fn2_capi.corr_lookup_forward(f1d, f2d, cod, r, scale)
        s1_, s2_ = fn2_capi.corr_lookup_backward(f1d, f2d, cod, god, r, scale)
        mo = CorrLookup(r)(f1d, f2d, cod)
    s.synchronize()
    _same_bits(so, want, "forward on another stream")
    _same_bits(mo, want, "module on another stream")
    grads(s1_, s2_, "backward on another stream")
    # other element types are refused, not converted
    with pytest.raises(RuntimeError, match="float32"):
        corr_lookup_cuda.forward_alloc(f1d.half(), f2d.half(), cod.half(), r, scale)
    with pytest.raises(RuntimeError, match="radius"):
        corr_lookup_cuda.forward_alloc(f1d, f2d, cod, 9, scale)


# ------------------------------------------------------------------ 5: AlternateCorrBlock
def test_alternate_corr_block_against_rafts_pooled_composition(dev):
    """3 levels, r = 3, 2 x 16 x 24 x 32, against compose() in float64 on the CPU, which pools the all-pairs volume as RAFT does.
    Tolerance: the header's forward bound of each level (S from the float64-pooled fmap2), summed over the levels.  The layer
    pools fmap2 in fp32 instead, at most 4 roundings per level relative to the pooled |fmap2|; for this data (unit normal) that
    is a few 2^-24 S_0, inside the two other levels' share of the sum.  coords / 2^i is exact."""
    from networks.correlation_package import AlternateCorrBlock
    B, C, H, W, r, L = 2, 16, 24, 32, 3, 3
    D2 = (2 * r + 1) ** 2
    f1, f2 = _features(1, C, (H, W), (H, W), seed=9)
    co = _coords("a", B, H, W, H, W, r, seed=10)
    scale = float(C) ** -0.5
    got = AlternateCorrBlock(f1.to(dev), f2.to(dev), num_levels=L, radius=r)(co.to(dev))
    assert got.shape == (B, L * D2, H, W)
    want = RL.compose(f1.double(), f2.double(), co.double(), r, scale, num_levels=L).numpy()
    tol = np.zeros((B, D2, H, W))
    lvl = f2.double()
    for i in range(L):
        if i:
            lvl = torch.nn.functional.avg_pool2d(lvl, 2, stride=2)
        exact, S = RL.forward(f1.numpy(), lvl.numpy(), (co / 2 ** i).numpy(), r, scale)
        # the reference is the composition, level by level -- where fl32(c - floor(c)) is exact (the header: not for -1 < c < 0)
        c_i = (co / 2 ** i).numpy()
        exact_fx = ~((c_i > -1) & (c_i < 0)).any(axis=1)[:, None]
        assert (np.abs(exact - want[:, i * D2:(i + 1) * D2]) < 1e-12)[np.broadcast_to(exact_fx, exact.shape)].all()
        assert np.abs(exact - want[:, i * D2:(i + 1) * D2]).max() < 1e-6
        tol += RL.delta_forward(exact, S, C, scale)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    ratio = float((err.reshape(B, L, D2, H, W) / tol[:, None]).max())
    print(f"  AlternateCorrBlock: error / summed bound {ratio:.3f}")
    assert ratio <= 1.0
    assert np.abs(want).max() > 0.1
    # channel and level order: fmap2's only non-zero pixel is (y, x) = (8, 12); fmap1 is all ones; integer identity coordinates
    one = torch.zeros(1, C, H, W)
    one[0, 0, 8, 12] = 1.0
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ident = torch.stack([xs, ys])[None]
    out = AlternateCorrBlock(torch.ones(1, C, H, W, device=dev), one.to(dev), num_levels=L, radius=r)(ident.to(dev)).cpu()
    D = 2 * r + 1
    px = out[0, :, 8, 11]          # the pixel left of it: level 0 sees it at i - r = +1, j - r = 0
    expect = torch.zeros(L * D2)
    expect[(r + 1) * D + r] = scale                                   # level 0: (12, 8) - (11, 8) = (+1, 0), weight 1
    expect[D2 + (r + 1) * D + r] = expect[D2 + r * D + r] = 0.5 * 0.25 * scale        # level 1: 1/4 at (6, 4), seen from (5.5, 4)
    expect[2 * D2 + (r + 1) * D + r] = 0.25 / 16 * scale              # level 2: 1/16 at (3, 2), seen from (2.75, 2)
    expect[2 * D2 + r * D + r] = 0.75 / 16 * scale
    assert torch.equal(px, expect), (px.nonzero().flatten().tolist(), expect.nonzero().flatten().tolist())
    py = out[0, :, 6, 12]          # two rows above it: level 0 sees it at i - r = 0, j - r = +2
    assert py[r * D + r + 2] == scale and int((py[:D2] != 0).sum()) == 1


# ------------------------------------------------------------------ 6: what is refused
def test_coords_gradient_second_backward_and_deterministic_mode(dev):
    from networks.correlation_package import CorrLookup
    r, C, s1 = 1, 5, (3, 5)
    f1, f2 = _features(1, C, s1, s1, seed=1)
    co = _coords("a", 2, 3, 5, 3, 5, r, seed=2).to(dev)
    go = R.grad_output("normal", (2, 9, 3, 5), seed=3).to(dev)
    layer = CorrLookup(r)
    with pytest.raises(RuntimeError, match="detach"):
        layer(f1.to(dev).requires_grad_(True), f2.to(dev), co.clone().requires_grad_(True))
    with torch.no_grad():   # grad mode off: nothing to train wrongly
        assert layer(f1.to(dev), f2.to(dev), co.clone().requires_grad_(True)).shape == (2, 9, 3, 5)
    a, b = f1.to(dev).requires_grad_(True), f2.to(dev).requires_grad_(True)
    out = layer(a, b, co)
    with pytest.raises(RuntimeError, match="not differentiable a second time"):
        torch.autograd.grad(out, a, go.clone().requires_grad_(True), create_graph=True)
    want = torch.autograd.grad(layer(a, b, co), (a, b), go)
    try:
        torch.use_deterministic_algorithms(True)
        out = layer(a, b, co)       # the forward is deterministic
        with pytest.raises(RuntimeError, match="corr_lookup_cuda.backward"):
            torch.autograd.grad(out, (a, b), go)
        torch.use_deterministic_algorithms(True, warn_only=True)
        out = layer(a, b, co)
        with pytest.warns(UserWarning, match="corr_lookup_cuda.backward"):
            got = torch.autograd.grad(out, (a, b), go)
    finally:
        torch.use_deterministic_algorithms(False)
    assert torch.equal(got[0], want[0]) and torch.allclose(got[1], want[1], rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------ 10: hipGraph replay of the backward
def test_backward_replays_from_a_hip_graph(dev):
    """grad_fmap2 is a scatter of float atomics into a tensor the library clears on the stream first; captured into a hipGraph
    that clear has to run on EVERY replay.  The module's forward and backward are captured once and replayed on three sets of
    values in the captured buffers, the captured gradients poisoned with NaN before each replay: grad_fmap1 has the eager
    call's bits, grad_fmap2 lies inside its any-order bound and is exactly zero where no term arrives."""
    from networks.correlation_package import CorrLookup
    r, C, s1, s2 = 3, 5, (13, 19), (6, 9)
    B, (H, W), (H2, W2) = 2, s1, s2
    scale = float(C) ** -0.5

    def values(seed):
        f1, f2 = _features(1, C, s1, s2, seed=seed)
        return f1, f2, _coords("a", B, H, W, H2, W2, r, seed=seed + 2), R.grad_output("normal", (B, (2 * r + 1) ** 2, H, W), seed=seed + 3)

    f1, f2, co, go = (t.to(dev) for t in values(50))
    a, b = f1.requires_grad_(True), f2.requires_grad_(True)
    layer = CorrLookup(r)

    def step():
        return torch.autograd.grad(layer(a, b, co), (a, b), go)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g1, g2 = step()
    for seed in (60, 70, 80):
        fresh = values(seed)
        with torch.no_grad():
            for dst, src in zip((a, b, co, go), fresh):
                dst.copy_(src)
            g1.fill_(float("nan"))
            g2.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        e1, _ = _bwd(a.detach(), b.detach(), co, go, r, scale, AUTO, what=f"eager backward, seed {seed}")
        _same_bits(g1, e1, f"grad_fmap1 replayed, seed {seed}")
        _, (x2, S2, n2) = RL.backward(*(t.numpy() for t in fresh), r, scale)
        _within(g2, x2, RL.delta_grad2(x2, S2, n2, scale), f"grad_fmap2 replayed, seed {seed}")
        assert bool((g2.cpu()[torch.from_numpy(n2 == 0)] == 0).all())


# ------------------------------------------------------------------ 7: memory
def test_forward_and_backward_allocate_only_their_results(dev):
    """1 x 16 x 64 x 96, r = 4, one level: the peak above the inputs stays below output + both gradients + 1 MB; the all-pairs
    volume alone would be (64 * 96)^2 * 4 B = 151 MB."""
    from networks.correlation_package import CorrLookup
    B, C, H, W, r = 1, 16, 64, 96, 4
    f1, f2 = _features(1, C, (H, W), (H, W), seed=2, B=B)
    a, b = f1.to(dev).requires_grad_(True), f2.to(dev).requires_grad_(True)
    co = _coords("a", B, H, W, H, W, r, seed=3).to(dev)
    go = torch.ones(B, 81, H, W, device=dev)
    layer = CorrLookup(r)
    layer(a, b, co).backward(go)   # warm-up: the module, the kernels' code objects
    a.grad = b.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    out = layer(a, b, co)
    out.backward(go)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    budget = 4 * (out.numel() + a.numel() + b.numel()) + (1 << 20)
    print(f"  peak {peak / 2 ** 20:.2f} MiB above the inputs, budget {budget / 2 ** 20:.2f} MiB, all-pairs volume {(H * W) ** 2 * 4 / 2 ** 20:.0f} MiB")
    assert peak <= budget, (peak, budget)
    assert a.grad is not None and b.grad is not None and float(b.grad.abs().max()) > 0


# ------------------------------------------------------------------ 8, 9: timing
def _windows(fns, calls=10, windows=5):
    """HIP-event times (ms per call) of alternating windows of `calls` calls of each function, after a warm-up."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(windows):
        for fn, t in zip(fns, ts):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) / calls)
    return ts


def _timing_inputs(dev, shape=(2, 64, 48, 64), r=4):
    B, C, H, W = shape
    f1, f2 = _features(1, C, (H, W), (H, W), seed=3, B=B)
    co = _coords("a", B, H, W, H, W, r, seed=4)
    return f1.to(dev), f2.to(dev), co.to(dev), float(C) ** -0.5


def test_forward_is_not_slower_than_the_composition(dev):
    """2 x 64 x 48 x 64, r = 4, family-a coordinates, medians over 5 alternating windows of 10 calls.  Only "not slower" is
    asserted; the ratio is printed (DESIGN.md 4.11 records it)."""
    from networks.correlation_package import CorrLookup
    r = 4
    f1d, f2d, cod, scale = _timing_inputs(dev)
    layer = CorrLookup(r)
    with torch.no_grad():
        ref, out = RL.compose(f1d, f2d, cod, r, scale), layer(f1d, f2d, cod)
        # (a sanity check that the two are the same function, not a precision pin: tests 1 - 3 are those)
        assert float((out - ref).abs().max()) <= 1e-4 * float(ref.abs().max())
        tl, tc = _windows([lambda: layer(f1d, f2d, cod), lambda: RL.compose(f1d, f2d, cod, r, scale)])
    ml, mc = statistics.median(tl), statistics.median(tc)
    print(f"  CorrLookup forward {ml * 1e3:.1f} us, composition {mc * 1e3:.1f} us: {mc / ml:.1f} x")
    assert ml <= mc, (tl, tc)


def test_auto_is_the_staged_kernel_for_small_radii(dev):
    """The header: AUTO takes the staged kernels for every r <= FN2L_STAGED_MAX_RADIUS (no measured point has the general kernel
    ahead), the general ones above.  Bits cannot tell the kernels apart, a time can: at 2 x 64 x 48 x 64, r = 4, AUTO's median
    lies inside the spread of FN2L_LOOKUP_STAGED's windows (10 % each way), and if the two kernels' windows do not overlap every
    AUTO window is on the staged side.  r = 5: AUTO runs (the general kernel), STAGED is refused."""
    import fn2_capi
    r = STAGED_MAX_R
    f1d, f2d, cod, scale = _timing_inputs(dev, r=r)
    out = torch.empty(2, (2 * r + 1) ** 2, 48, 64, device=dev)
    ta, ts, tg = _windows([lambda algo=algo: fn2_capi.corr_lookup_forward(f1d, f2d, cod, r, scale, algo=algo, out=out) for algo in (AUTO, STAGED, GENERAL)])
    ma = statistics.median(ta)
    print(f"  forward 2x64x48x64 r {r}: AUTO {ma * 1e3:.1f} us, staged {statistics.median(ts) * 1e3:.1f} us [{min(ts) * 1e3:.1f}, {max(ts) * 1e3:.1f}], "
          f"general {statistics.median(tg) * 1e3:.1f} us [{min(tg) * 1e3:.1f}, {max(tg) * 1e3:.1f}]")
    assert 0.9 * min(ts) <= ma <= 1.1 * max(ts), (ta, ts, tg)
    if max(ts) < min(tg):
        assert max(ta) < min(tg), (ta, ts, tg)
    elif max(tg) < min(ts):
        assert min(ta) > max(tg), (ta, ts, tg)
    big = torch.empty(2, (2 * r + 3) ** 2, 48, 64, device=dev)
    _same_bits(fn2_capi.corr_lookup_forward(f1d, f2d, cod, r + 1, scale, algo=AUTO), fn2_capi.corr_lookup_forward(f1d, f2d, cod, r + 1, scale, algo=GENERAL, out=big),
               "AUTO above the staged radius")
    with pytest.raises(RuntimeError):
        fn2_capi.corr_lookup_forward(f1d, f2d, cod, r + 1, scale, algo=STAGED)
