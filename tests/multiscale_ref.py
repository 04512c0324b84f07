"""The per-element contract of the fused MultiScale loss kernel (csrc/multiscale_loss.hip) against float64, in numpy: exact values,
error bounds counted from the kernel's roundings, an emulation of the kernel's float32 arithmetic in its summation order, and one
``check_*`` function per contract.  A helper module for tests/test_multiscale_contract_host.py (CPU) and
tests/test_gpu_multiscale_contract.py (GPU), which call the same checks -- not a conftest.

Notation: u = 2^-24 (unit roundoff of float32, round to nearest), gamma_n = n u / (1 - n u).  ``fl`` is one float32 rounding.  No
bound below is a constant fitted to results: each is computed from the inputs.  Underflow is excluded (the inputs of the tests keep every
nonzero product and difference far above 2^-126; ``Ref`` asserts it for the products).

(a) Exact values.  t = float64(float32(div_flow)) * float64(target) (a product of two float32 values: exact in float64).  For level i,
    k_i = start_scale << i, H_i = H // k_i, W_i = W // k_i (floor geometry: only cells that lie fully inside the image exist),
    m_i = mean of t over the k_i x k_i cell, A_i = mean of |t| over it, d_i = float64(out_i) - m_i.  (The float64 sums behind m_i carry a
    relative error below k_i^2 2^-53 <= 2^-37 A_i, 2^-13 of the smallest bound below; exact for the dyadic inputs of the exact case.)

(b) The kernel's pooled mean.  Level 0: a lane forms sum = fl(sum + fl(div_flow * T)) over the s0^2 elements of its cell, starting from 0:
    one product rounding and at most s0^2 - 1 inexact additions per term (0 + x is exact), s0^2 roundings.  Contracted into FMAs the
    product rounding disappears; fewer roundings, same bound, and the truth in (a) is the exact product either way.  Every level up is
    (a + b) + (c + d): two more roundings per term.  The division by k_i^2, a power of two, is exact.  So
        |m^_i - m_i| <= e_m,i = gamma_(s0^2 + 2 i) * A_i.
    The difference is one more rounding: d^ = fl(out - m^), |d^ - (out - m^)| <= u |out - m^| <= u (|d| + e_m), hence
        |d^ - d| <= dd = e_m + u (|d| + e_m).
    A subtraction is exact in sign: sign(d^) = sign(out - m^), which is sign(d) wherever |d| > e_m.

(c) Gradients (the only per-element outputs).
    gw_i = float32(float64(grad_scale) * float64(float32(w_i)) / N_i) as ms_launch forms it, N_i = 2 B H_i W_i (norm 1), B H_i W_i (norm 2).
    norm 1: g^ = sign(d^) gw exactly.  Elements with |d| > e_m: g^ == sign(d) gw bit for bit.  Elements with |d| <= e_m are undetermined:
        one of {-gw, 0, +gw}.
    norm 2, per pixel with d = (d_0, d_1), r = ||d||, D = ||(dd_0, dd_1)||, r^ = ||d^|| (exact norm of the computed differences):
        e^ = sqrt_rn(fl(fl(d^_0^2) + fl(d^_1^2)))            three roundings under the root (two with an FMA), the root correctly rounded:
           = r^ sqrt(1 + th_2) (1 + dl),  |th_2| <= gamma_2,  |sqrt(1 + th_2) - 1| <= gamma_2 / (2 - gamma_2) = u / (1 - 3u)
           = r^ (1 + th_e),               |th_e| <= eps_e = 2u / (1 - 3u)
        g   = fl(gw / e^),  g^_c = fl(g d^_c) = gw (d^_c / r^) F,   F = (1 + dl_5)(1 + dl_6) / (1 + th_e),
                                                                    |F - 1| <= eta = (1 + u)^2 / (1 - eps_e) - 1    (about 4u)
        and, for unit vectors in the plane, || d^/r^ - d/r || <= 2 ||d^ - d|| / (r + r^) <= D / (r - D / 2)   (r^ >= r - D).  So
        |g^_c - gw d_c / r| <= gw * ( D / (r - D / 2) + eta )                               for every pixel with r > D.
        Pixels with r <= D are undetermined; there only ||g^|| <= gw (1 + eta) is claimed (g^ = 0 where e^ == 0).

(d) Sums.  A lane's L1 term is fl(|d^_0| + |d^_1|) (1 rounding); then the 64-lane shuffle tree (6), the four-wave combine (2), in the last
    workgroup ceil(nblocks / 256) strided additions, its tree (6) and combine (2):
        depth_L1 = 17 + ceil(nblocks / 256),   depth_EPE = 16 + ceil(nblocks / 256)   (the EPE term needs no channel addition)
        |S^_L1 - sum |d||  <= sum dd + gamma_depth_L1 * sum (|d| + dd)
        |e^ - r| <= D + eps_e (r + D) per pixel, so
        |S^_EPE - sum r|   <= sum (D + eps_e (r + D)) + gamma_depth_EPE * (1 + eps_e) sum (r + D).
    loss / epe = sum_i fl(S^_i coef_i), added sequentially from 0: one product rounding and at most ns - 1 additions per term, with
    coef_i = float32(float64(float32(w_i)) / N_i) as ms_launch forms it (the truth uses these float32 factors exactly):
        |loss^ - sum_i coef_i S_i| <= sum_i coef_i bound_i + gamma_ns * sum_i coef_i (S_i + bound_i).
"""
import numpy as np

U = 2.0 ** -24
EPS_E = 2 * U / (1 - 3 * U)
ETA = (1 + U) ** 2 / (1 - EPS_E) - 1
F32 = np.float32
MAX_CELLS = 16                          # finest cells per workgroup edge (k_max / start_scale <= 16)


def gamma(n):
    return n * U / (1 - n * U)


def geometry(B, H, W, s0, ns):
    """k_max, workgroups per row / column, workgroups -- ms_geometry of the kernel's host code."""
    kmax = s0 << (ns - 1)
    assert s0 >= 1 and s0 & (s0 - 1) == 0 and s0 <= 16 and kmax // s0 <= MAX_CELLS
    bx, by = -(-W // kmax), -(-H // kmax)
    return kmax, bx, by, B * bx * by


def level_shapes(B, H, W, s0, ns):
    return [(B, 2, H // (s0 << i), W // (s0 << i)) for i in range(ns)]


def unit_weight(w, grad_scale, n_elems):
    """gw_i / coef_i as ms_launch forms them: a float64 product and quotient, rounded once to float32; 0 for an empty level."""
    if n_elems == 0:
        return F32(0)
    return F32(np.float64(F32(grad_scale)) * np.float64(F32(w)) / np.float64(n_elems))


def seeded_inputs(shape, seed=0):
    """target ~ 5 N(0,1), predictions ~ 0.3 N(0,1), FlowNet2's weights 0.32 / 2^i: the distributions of the training loss's inputs."""
    B, H, W, s0, ns = shape
    rng = np.random.default_rng(1000 * seed + 131 * B + 17 * H + 3 * W + 7 * s0 + ns)
    target = (rng.standard_normal((B, 2, H, W)) * 5.0).astype(F32)
    outs = [(rng.standard_normal(s) * 0.3).astype(F32) for s in level_shapes(B, H, W, s0, ns)]
    return target, outs, [0.32 / 2 ** i for i in range(ns)]


def exact_inputs(shape, seed=0):
    """Inputs on which every pooled mean, difference and L1 sum is a float32 number whatever the order of the additions: integer targets
    in [-64, 64], div_flow = 0.125 (t: multiples of 2^-3, |t| <= 8; a pooled sum has at most 2^16 terms: below 2^22 units of 2^-3),
    predictions multiples of 2^-q_i, q_i <= 11, with |out| < 16.  The quantum of d_i is min(2^-q_i, 2^-3 / k_i^2) and |d| < 24, so every
    partial sum of |d| over a level is an integer below 24 N_i in units of that quantum: exact if 24 N_i < 2^24 quantum.  q_i is the
    largest q <= 11 that keeps this (fine levels with thousands of elements get coarser predictions); ``Ref.assert_exact`` verifies the
    condition on the values themselves.  About 1 % of the pixels get predictions equal to the pooled target in both channels (d = 0),
    and as many in one channel only.  Returns (target, outs, weights, div_flow)."""
    B, H, W, s0, ns = shape
    rng = np.random.default_rng(77 + seed + 131 * B + 17 * H + 3 * W + 7 * s0 + ns)
    target = rng.integers(-64, 65, (B, 2, H, W)).astype(F32)
    t = 0.125 * target.astype(np.float64)
    outs = []
    for i, s in enumerate(level_shapes(B, H, W, s0, ns)):
        k = s0 << i
        n = int(np.prod(s))
        q = 11
        while q > 0 and 24 * n >= 2.0 ** (24 - q):
            q -= 1
        o = rng.integers(-(16 << q) + 1, 16 << q, s).astype(np.float64) * 2.0 ** -q
        if n:
            m = pooled(t, k)[0]
            both = rng.random((s[0], 1, s[2], s[3])) < 0.01
            one = rng.random(s) < 0.005
            o = np.where(both | one, m, o)
        outs.append(o.astype(F32))
        assert np.array_equal(outs[-1].astype(np.float64), o)
    return target, outs, [0.32 / 2 ** i for i in range(ns)], 0.125


def pooled(t, k):
    """(mean of t, mean of |t|) over the full k x k cells of a B x 2 x H x W float64 array."""
    B, C, H, W = t.shape
    Hi, Wi = H // k, W // k
    c = t[:, :, :Hi * k, :Wi * k].reshape(B, C, Hi, k, Wi, k)
    return c.sum(axis=(3, 5)) / (k * k), np.abs(c).sum(axis=(3, 5)) / (k * k)


class Ref:
    """Exact values (a) and bounds (b)-(d) for one set of inputs.  Per level i: m, A, d, e_m, dd (B x 2 x H_i x W_i, float64)."""

    def __init__(self, target, outs, weights, s0, div_flow, grad_scale=1.0):
        target = np.asarray(target)
        assert target.dtype == np.float32 and all(np.asarray(o).dtype == np.float32 for o in outs)
        self.B, _, self.H, self.W = target.shape
        self.s0, self.ns = s0, len(outs)
        self.kmax, self.bx, self.by, self.nblocks = geometry(self.B, self.H, self.W, s0, self.ns)
        self.weights, self.grad_scale, self.div_flow = list(weights), grad_scale, F32(div_flow)
        t = np.float64(self.div_flow) * target.astype(np.float64)
        nz = np.abs(t[t != 0])
        assert nz.size == 0 or nz.min() > 2.0 ** -100, "the bounds exclude underflow"
        self.m, self.A, self.d, self.e_m, self.dd = [], [], [], [], []
        for i, o in enumerate(outs):
            k = s0 << i
            m, A = pooled(t, k)
            assert o.shape == m.shape, (i, o.shape, m.shape)
            d = np.asarray(o).astype(np.float64) - m
            e_m = gamma(s0 * s0 + 2 * i) * A
            self.m.append(m); self.A.append(A); self.d.append(d); self.e_m.append(e_m)
            self.dd.append(e_m + U * (np.abs(d) + e_m))

    def n_elems(self, i, norm):
        return self.d[i].size // (2 if norm == 2 else 1)

    def gw(self, i, norm):
        return unit_weight(self.weights[i], self.grad_scale, self.n_elems(i, norm))

    def coef(self, i, which):           # which: 0 for the L1 sums (w / elements), 1 for the 2-norm sums (w / pixels)
        return unit_weight(self.weights[i], 1.0, self.d[i].size // (2 if which else 1))

    def r_D(self, i):
        return np.sqrt((self.d[i] ** 2).sum(axis=1)), np.sqrt((self.dd[i] ** 2).sum(axis=1))

    def undetermined(self, i, norm):
        """Boolean mask of the elements (norm 1) or pixels (norm 2) whose gradient the contract leaves open."""
        if norm == 1:
            return np.abs(self.d[i]) <= self.e_m[i]
        r, D = self.r_D(i)
        return r <= D

    def undetermined_count(self):
        return sum(int(self.undetermined(i, n).sum()) for i in range(self.ns) for n in (1, 2))

    def sums_and_bounds(self):
        """(exact 2 ns sums, their bounds) -- part (d)."""
        trips = -(-self.nblocks // 256)
        S, Bd = np.zeros(2 * self.ns), np.zeros(2 * self.ns)
        for i in range(self.ns):
            a, dd = np.abs(self.d[i]), self.dd[i]
            r, D = self.r_D(i)
            S[i] = a.sum()
            Bd[i] = dd.sum() + gamma(17 + trips) * (a + dd).sum()
            S[self.ns + i] = r.sum()
            Bd[self.ns + i] = (D + EPS_E * (r + D)).sum() + gamma(16 + trips) * (1 + EPS_E) * (r + D).sum()
        return S, Bd

    def loss_epe_and_bounds(self, norm):
        """(exact [loss, epe], bounds): the weighted means with the kernel's float32 factors.  norm 2: loss is the epe expression."""
        S, Bd = self.sums_and_bounds()
        val, bnd = np.zeros(2), np.zeros(2)
        for which in (0, 1):
            for i in range(self.ns):
                c = np.float64(self.coef(i, which))
                j = which * self.ns + i
                val[which] += c * S[j]
                bnd[which] += c * Bd[j] + gamma(self.ns) * c * (S[j] + Bd[j])
        if norm == 2:
            val[0], bnd[0] = val[1], bnd[1]
        return val, bnd

    def assert_exact(self):
        """The condition of ``exact_inputs``: every partial sum of the kernel is a float32 number, so the order cannot matter."""
        for i in range(self.ns):
            a = np.abs(self.d[i])
            if a.size == 0:
                continue
            nzq = a[a != 0]
            quantum = 2.0 ** -40
            while nzq.size and np.all(nzq / (2 * quantum) == np.round(nzq / (2 * quantum))):
                quantum *= 2
            assert a.sum() < 2.0 ** 24 * quantum, (i, a.sum(), quantum)
            assert np.array_equal(self.d[i].astype(F32).astype(np.float64), self.d[i])
            assert np.array_equal(self.m[i].astype(F32).astype(np.float64), self.m[i])
            k = self.s0 << i
            assert self.A[i].max() * k * k < 2.0 ** 21                      # pooled sums: below 2^24 units of 2^-3


# ------------------------------------------------------------------------------------------------------------------------------
# (f) checks.  Each returns a Report; ``ok`` is the verdict, ``ratio`` the largest error / bound (0 for exact contracts), ``worst``
# describes the worst element: level, index, got, want, bound.

class Report:
    def __init__(self, name):
        self.name, self.ok, self.ratio, self.worst = name, True, 0.0, ""

    def fail(self, msg):
        if self.ok:
            self.worst = msg
        self.ok = False

    def bounded(self, level, got, want, bound, what=""):
        """|got - want| <= bound elementwise; NaN fails; bound == 0 demands equality."""
        got, want, bound = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(bound, np.float64)
        if got.size == 0:
            return
        err = np.abs(got - want)
        err = np.where(np.isnan(err), np.inf, err)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        j = int(np.argmax(ratio))
        top = float(ratio.reshape(-1)[j])
        if top > self.ratio or not self.worst:
            idx = tuple(int(v) for v in np.unravel_index(j, ratio.shape)) if ratio.ndim else ()
            self.worst = (f"{self.name}{what}: level {level} index {idx} got {got.reshape(-1)[j]!r} want {want.reshape(-1)[j]!r} "
                          f"bound {np.broadcast_to(bound, ratio.shape).reshape(-1)[j]!r} error/bound {top:.3g}")
            self.ratio = max(self.ratio, top)
        if top > 1.0:
            self.ok = False

    def equal(self, level, got, want, what=""):
        got, want = np.asarray(got), np.asarray(want)
        if got.shape != want.shape:
            return self.fail(f"{self.name}{what}: level {level} shape {got.shape} != {want.shape}")
        bad = ~(got == want)                                            # NaN is unequal; -0 == +0
        if bad.any():
            j = int(np.argmax(bad))
            idx = tuple(int(v) for v in np.unravel_index(j, bad.shape))
            self.fail(f"{self.name}{what}: level {level} index {idx} got {got.reshape(-1)[j]!r} want {want.reshape(-1)[j]!r} "
                      f"bound 0 ({int(bad.sum())} of {bad.size} differ)")

    def __repr__(self):
        return f"<{'ok' if self.ok else 'FAIL'} ratio {self.ratio:.3g} {self.worst}>"


def check_grads_l1(ref, grads):
    """(c) norm 1.  ``grads``: per level a float32 array (None: a level without elements that was passed as a null pointer)."""
    rep = Report("grad L1")
    for i in range(ref.ns):
        d, gw = ref.d[i], ref.gw(i, 1)
        if d.size == 0:
            continue
        g = np.asarray(grads[i])
        if g.dtype != np.float32 or g.shape != d.shape:
            rep.fail(f"grad L1: level {i} dtype/shape {g.dtype} {g.shape}")
            continue
        und = ref.undetermined(i, 1)
        want = (np.sign(d) * np.float64(gw)).astype(F32)
        rep.equal(i, np.where(und, want, g), want)
        open_ok = (g == gw) | (g == -gw) | (g == 0)
        rep.equal(i, np.where(und, open_ok, True), np.ones(d.shape, bool), " (undetermined element not in {-gw, 0, gw})")
    return rep


def check_grads_l2(ref, grads):
    """(c) norm 2."""
    rep = Report("grad L2")
    for i in range(ref.ns):
        d = ref.d[i]
        if d.size == 0:
            continue
        g = np.asarray(grads[i])
        if g.dtype != np.float32 or g.shape != d.shape:
            rep.fail(f"grad L2: level {i} dtype/shape {g.dtype} {g.shape}")
            continue
        gw = np.float64(ref.gw(i, 2))
        r, D = ref.r_D(i)
        und = (r <= D)[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.where(und, 0.0, gw * d / r[:, None])
            bound = np.where(und, np.inf, gw * (D / (r - D / 2) + ETA)[:, None])
        g64 = g.astype(np.float64)
        rep.bounded(i, np.where(und, 0.0, g64), want, np.broadcast_to(bound, d.shape))
        norm = np.sqrt((g64 ** 2).sum(axis=1))
        lim = gw * (1 + ETA) * (1 + 2 * U)                              # (the float64 norm of two float32 numbers: far below 2u)
        rep.bounded(i, np.where(und[:, 0], norm, 0.0), 0.0, lim, " (norm at an undetermined pixel)")
    return rep


def check_sums(ref, sums):
    """(d) the 2 ns sums.  A level without elements must give exactly 0."""
    rep = Report("sums")
    S, Bd = ref.sums_and_bounds()
    sums = np.asarray(sums)
    if sums.dtype != np.float32 or sums.shape != S.shape:
        rep.fail(f"sums: dtype/shape {sums.dtype} {sums.shape}")
        return rep
    for j in range(2 * ref.ns):
        rep.bounded(j % ref.ns, sums[j], S[j], Bd[j], " (L1)" if j < ref.ns else " (EPE)")
    return rep


def check_loss_epe(ref, loss_epe, norm):
    rep = Report("loss_epe")
    val, bnd = ref.loss_epe_and_bounds(norm)
    le = np.asarray(loss_epe)
    if le.dtype != np.float32 or le.shape != (2,):
        rep.fail(f"loss_epe: dtype/shape {le.dtype} {le.shape}")
        return rep
    rep.bounded("all", le[0], val[0], bnd[0], " (loss)")
    rep.bounded("all", le[1], val[1], bnd[1], " (epe)")
    if norm == 2:
        rep.equal("all", le[:1], le[1:], " (norm 2: loss is the epe expression)")
    return rep


def check_exact(ref, sums, grads_l1, grads_l2):
    """The exact case: L1 sums and norm-1 gradients equal the float64 values bit for bit; d == 0 gives gradient 0 under both norms."""
    rep = Report("exact")
    ref.assert_exact()
    S, _ = ref.sums_and_bounds()
    rep.equal("all", np.asarray(sums)[:ref.ns], S[:ref.ns].astype(F32), " (L1 sums)")
    for i in range(ref.ns):
        d = ref.d[i]
        if d.size == 0:
            continue
        rep.equal(i, np.asarray(grads_l1[i]), (np.sign(d) * np.float64(ref.gw(i, 1))).astype(F32), " (norm-1 gradient)")
        g2 = np.asarray(grads_l2[i])
        rep.equal(i, np.where(d == 0, g2, 0), np.zeros(d.shape, F32), " (norm-2 gradient where d == 0)")
    return rep


ALL_MUTANTS = ("drop_last", "partial_edge", "three_children", "wrong_plane", "gw_next_n", "l2_d0_both", "sign0_plus", "first_256",
               "no_div_flow")


# ------------------------------------------------------------------------------------------------------------------------------
# (e) The kernel in float32 numpy, in its summation order.  fma=True contracts a * b + c into one rounding the way the compiler may
# (emulated as float32(float64(a) * float64(b) + float64(c)): the product is exact, the sum is rounded to 53 bits and then to 24 -- a
# double rounding that can differ from a true FMA in rare ties, which is inside the bounds like any other rounding).

def _fma(a, b, c, fma):
    if fma:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    return (a * b).astype(F32) + c


def _tree(v):
    """The 64-lane __shfl_down tree (what lane 0 holds), then nothing else: v is (..., 64)."""
    off = 32
    while off:
        v = v[..., :off] + v[..., off:2 * off]
        off >>= 1
    return v[..., 0]


def _block_reduce(per_thread):
    """(nblocks, 256) per-lane values -> (nblocks,): four wave trees, then (w0 + w1) + (w2 + w3)."""
    w = _tree(per_thread.reshape(-1, 4, 64))
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def emulate(target, outs, weights, s0, div_flow, norm, grad_scale=1.0, fma=False, mutant=None):
    """Returns (sums float32[2 ns], loss_epe float32[2], grads list of float32 arrays).  ``mutant``: one of ALL_MUTANTS, a deliberately
    wrong kernel for the host test."""
    assert mutant is None or mutant in ALL_MUTANTS
    target = np.asarray(target, F32)
    B, _, H, W = target.shape
    ns = len(outs)
    kmax, bx, by, nblocks = geometry(B, H, W, s0, ns)
    df = F32(1.0) if mutant == "no_div_flow" else F32(div_flow)
    n = kmax // s0
    GH, GW = by * n, bx * n                                             # the grid of finest cells the workgroups cover
    H0, W0 = H // s0, W // s0
    L = np.zeros((B, 2, GH, GW), F32)
    if mutant == "partial_edge":                                        # every cell that starts inside the image, the outside read as 0
        tp = np.zeros((B, 2, GH * s0, GW * s0), F32)
        tp[:, :, :H, :W] = target
        src, h0, w0 = tp, min(GH, -(-H // s0)), min(GW, -(-W // s0))
    else:
        src, h0, w0 = target, H0, W0
    acc = np.zeros((B, 2, h0, w0), F32)
    for yy in range(s0):
        for xx in range(s0):
            if mutant == "drop_last" and yy == s0 - 1 and xx == s0 - 1:
                continue
            acc = _fma(np.broadcast_to(df, acc.shape), src[:, :, yy:h0 * s0:s0, xx:w0 * s0:s0], acc, fma)
    L[:, :, :h0, :w0] = acc
    sums = np.zeros(2 * ns, F32)
    grads, partial = [], np.zeros((nblocks, 2 * ns), F32)
    k = s0
    for i in range(ns):
        Hi, Wi = H // k, W // k
        o = np.asarray(outs[i], F32).reshape(B, 2, Hi, Wi) if outs[i] is not None else np.zeros((B, 2, Hi, Wi), F32)
        nel = lambda kk, nrm: (B * (H // kk) * (W // kk)) * (1 if nrm == 2 else 2)
        gw = unit_weight(weights[i], grad_scale, nel(2 * k if mutant == "gw_next_n" else k, norm))
        l1 = np.zeros((B, GH, GW), F32)
        ep = np.zeros((B, GH, GW), F32)
        g = np.zeros((B, 2, Hi, Wi), F32)
        inv = F32(k * k)
        # the cells this level compares: rows / columns gy < Hi, gx < Wi; the prediction is read at the flat index the kernel forms
        ch, cw = Hi, Wi
        if mutant == "partial_edge":
            ch, cw = min(GH, -(-H // k)), min(GW, -(-W // k))
        if o.size:
            flat = o.reshape(-1)
            plane = Hi * Wi
            plane1 = (H // (2 * k)) * (W // (2 * k)) if mutant == "wrong_plane" else plane
            gy, gx = np.meshgrid(np.arange(ch), np.arange(cw), indexing="ij")
            idx = (np.arange(B)[:, None, None] * 2 * Hi + gy[None]) * Wi + gx[None]           # (B, ch, cw)
            rd = lambda j: np.where(j < flat.size, flat[np.minimum(j, flat.size - 1)], F32(0))
            d0 = rd(idx) - L[:, 0, :ch, :cw] / inv
            d1 = rd(idx + plane1) - L[:, 1, :ch, :cw] / inv
            l1[:, :ch, :cw] = np.abs(d0) + np.abs(d1)
            e = np.sqrt(_fma(d0, d0, (d1 * d1).astype(F32), fma))
            ep[:, :ch, :cw] = e
            if norm == 2:
                with np.errstate(divide="ignore", invalid="ignore"):
                    gg = np.where(e > 0, gw / e, F32(0)).astype(F32)
                g0, g1 = gg * d0, gg * (d0 if mutant == "l2_d0_both" else d1)
            else:
                zero = gw if mutant == "sign0_plus" else F32(0)
                sg = lambda d: np.where(d > 0, gw, np.where(d < 0, -gw, zero)).astype(F32)
                g0, g1 = sg(d0), sg(d1)
            gf = g.reshape(-1)
            inside = (gy < Hi) & (gx < Wi)                              # the kernel's own cells last: a mutant's stray stores lose
            for sel in (~inside, inside):
                for jj, val in ((idx, g0), (idx + plane, g1)):
                    j, v = jj[:, sel], val[:, sel]
                    keep = j < gf.size
                    gf[j[keep]] = v[keep]
        grads.append(g)
        # per-workgroup partial sums: lane = cy * n_i + cx inside the workgroup's n_i x n_i cells
        ni = kmax // k
        for v, col in ((l1, i), (ep, ns + i)):
            lanes = v.reshape(B, by, ni, bx, ni).transpose(0, 1, 3, 2, 4).reshape(nblocks, ni * ni)
            per = np.zeros((nblocks, 256), F32)
            per[:, :ni * ni] = lanes
            partial[:, col] = _block_reduce(per)
        if i + 1 < ns:
            a, b, c, d = L[:, :, 0::2, 0::2], L[:, :, 0::2, 1::2], L[:, :, 1::2, 0::2], L[:, :, 1::2, 1::2]
            L = (a + b) + (c if mutant == "three_children" else (c + d))
            GH, GW, k = GH // 2, GW // 2, 2 * k
    if nblocks == 0:
        return sums, np.zeros(2, F32), grads
    # the last workgroup: lane-strided rows, tree, four waves
    used = partial[:256] if mutant == "first_256" else partial
    trips = -(-used.shape[0] // 256)
    pad = np.zeros((trips * 256, 2 * ns), F32)
    pad[:used.shape[0]] = used
    acc = np.zeros((256, 2 * ns), F32)
    for tr in range(trips):
        acc = acc + pad[tr * 256:(tr + 1) * 256]
    sums = _block_reduce(np.ascontiguousarray(acc.T)).astype(F32)
    coef = np.array([unit_weight(weights[i], 1.0, 2 * B * (H // (s0 << i)) * (W // (s0 << i))) for i in range(ns)] +
                    [unit_weight(weights[i], 1.0, B * (H // (s0 << i)) * (W // (s0 << i))) for i in range(ns)], F32)
    terms = sums * coef
    l, e = F32(0), F32(0)
    for i in range(ns):
        l, e = l + terms[i], e + terms[ns + i]
    return sums, np.array([e if norm == 2 else l, e], F32), grads


def run_checks(ref, norm, sums, loss_epe, grads):
    """Every contract on one result: a dict name -> Report."""
    reps = {"sums": check_sums(ref, sums), "loss_epe": check_loss_epe(ref, loss_epe, norm)}
    reps["grads"] = check_grads_l1(ref, grads) if norm == 1 else check_grads_l2(ref, grads)
    return reps
