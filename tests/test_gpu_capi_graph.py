"""Every stream-taking entry point of the C ABI (include/*.h) captured RAW into a hipGraph and replayed -- what a caller without PyTorch
links against, and what the module-level capture tests (tests/test_gpu_pipelines.py) never reach: there torch allocates, zeroes and primes
the buffers; here the entry points get arbitrary memory.  The cases are tests/capi_graph_cases.py (held to the headers by
tests/test_capi_graph_cases_host.py).

Per case: every buffer is allocated before the capture, inside a guard of sentinel bytes; three warm-up calls on a side stream, then the
capture of the raw call on torch's current stream.  Then three replays, before each of which
  * a fresh, differently seeded set of values is copied into the captured input buffers,
  * every output is filled with NaN and every scratch workspace with 0xFF bytes (a primed MultiScale workspace is zeroed once, before
    the warm-up, and never touched again: the kernel's own ticket reset has to hold across replays),
and after each of which the same entry point is called eagerly on the same values into separate, equally poisoned buffers:
  * an output with repeatable bits must have the eager call's bits;
  * an output summed with fp32 atomics must lie inside the float64 bound its layer's own test applies, and keep its seed's bits
    (zero) where no contribution arrives;
  * every output must be non-trivial and free of NaN; the empty batch's sums must be exactly zero.
The guards must be intact at the end."""
import numpy as np
import pytest
import torch

import capi_graph_cases as G
import fn2_capi

pytestmark = pytest.mark.gpu

GUARD = 256            # bytes on either side of every buffer
SENTINEL = 0xA5
SEEDS = (1, 2, 3)
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _guarded(shape, dtype, dev):
    """A contiguous ``shape`` view of ``dtype``, 64-byte aligned, inside an allocation whose first and last GUARD bytes hold SENTINEL."""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    whole = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    view = whole[GUARD:GUARD + n].view(dtype).view(shape)
    assert view.data_ptr() % 64 == 0 and view.numel() == int(np.prod(shape))
    return view, whole


def _untouched(whole, what):
    assert bool((whole[:GUARD] == SENTINEL).all()) and bool((whole[-GUARD:] == SENTINEL).all()), f"{what}: wrote outside its buffer"


def _poison(t):
    if t.numel():
        t.view(-1).view(torch.uint8).fill_(0xFF)          # NaN in every floating type


def _bits(t):
    return t.contiguous().view(_INT[t.element_size()])


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = _bits(got) != _bits(want)
    n = int(bad.sum())
    if n:
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ from the eager call; first at flat index {i}: "
                             f"{float(got.flatten()[i])!r} vs {float(want.flatten()[i])!r}")


def _capture(step):
    """The pattern of tests/test_gpu_pipelines.py: three warm-up runs on a side stream, then the capture."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            assert step() == 0
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc = step()
    assert rc == 0, "the captured call returned a code"
    return graph


def _host(t):
    t = t.detach().cpu()
    return (t.float() if t.dtype in (torch.float16, torch.bfloat16) else t).numpy()


class Buffers:
    """The device buffers of one case: inputs and derived inputs once, outputs / scratch / primed workspaces twice (graph, eager)."""

    def __init__(self, case, dev):
        self.case, self.wholes = case, {}
        first = case.inputs(0)
        self.inputs = {k: self._new("input " + k, tuple(v.shape), v.dtype, dev) for k, v in first.items()}
        self.derived = {k: self._new("derived " + k, s, d, dev) for k, (s, d) in case.derived.items()}
        self.sides = []
        for side in ("graph", "eager"):
            out = {k: self._new(f"{side} output {k}", o.shape, o.dtype, dev) for k, o in case.outputs.items()}
            scratch = {k: self._new(f"{side} scratch {k}", (int(n()),), torch.uint8, dev) for k, n in case.scratch.items()}
            primed = {k: self._new(f"{side} primed {k}", (int(n()),), torch.uint8, dev) for k, n in case.primed.items()}
            for t in primed.values():
                t.zero_()                                # once; never touched again
            self.sides.append((out, scratch, {**self.inputs, **self.derived, **out, **scratch, **primed}))
        self.load(first)

    def _new(self, what, shape, dtype, dev):
        view, whole = _guarded(shape, dtype, dev)
        self.wholes[what] = whole
        return view

    def load(self, values):
        for k, v in values.items():
            self.inputs[k].copy_(v)
        for t in self.derived.values():
            _poison(t)
        if self.case.derive:
            self.case.derive({**self.inputs, **self.derived})
        torch.cuda.synchronize()

    def poison(self, side):
        out, scratch, _ = self.sides[side]
        for t in list(out.values()) + list(scratch.values()):
            _poison(t)

    def step(self, side):
        rcs = self.case.call(self.sides[side][2])
        return next((rc for rc in rcs if rc != 0), 0)

    def intact(self):
        for what, whole in self.wholes.items():
            _untouched(whole, f"{self.case.id}, {what}")


def _assert_corr_row(case, buf):
    direction, row, code, shape, params, names = case.corr_plan
    T = buf.sides[0][2]
    plan = fn2_capi.correlation_plan(direction, code, shape, *params, ptrs=[T[n].data_ptr() for n in names])
    assert plan[0] == row, (case.id, plan)


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.id)
def test_entry_point_replays_from_a_hip_graph(dev, case):
    with torch.cuda.device(dev):
        buf = Buffers(case, dev)
        if case.corr_plan:
            _assert_corr_row(case, buf)
        buf.poison(0)
        graph = _capture(lambda: buf.step(0))
        for seed in SEEDS:
            fresh = case.inputs(seed)
            buf.load(fresh)
            buf.poison(0)
            graph.replay()
            torch.cuda.synchronize()
            got = {k: t.clone() for k, t in buf.sides[0][0].items()}
            buf.poison(1)
            assert buf.step(1) == 0
            torch.cuda.synchronize()
            eager = buf.sides[1][0]
            for k, o in case.outputs.items():
                what = f"{case.id}, seed {seed}, {k}"
                g, e = got[k], eager[k]
                if o.part is not None:                   # a slice of a larger buffer: the rest keeps its poison
                    rest = torch.ones_like(g, dtype=torch.bool)
                    o.part(rest).fill_(False)
                    assert bool(torch.isnan(g[rest]).all()), f"{what}: wrote outside its slice"
                    g, e = o.part(g), o.part(e)
                assert not bool(torch.isnan(g).any()), f"{what}: NaN left after the replay"
                if o.kind == "zero":
                    assert bool((_bits(g) == 0).all()), f"{what}: the empty batch's result is not exactly zero"
                elif g.numel():
                    assert float(g.abs().max()) > 0, f"{what}: trivial"
                if o.kind != "atomic":
                    same_bits(g, e, what)
            if case.check:
                inp = {k: _host(v) for k, v in {**buf.inputs, **buf.derived}.items()}
                ratio = case.check(inp, {k: _host(v) for k, v in got.items()}, {k: _host(v) for k, v in eager.items()})
                print(f"CAPIGRAPH {case.id} seed {seed}: error / bound {ratio:.3f}")
        for primed in (s[2] for s in buf.sides):
            for k in case.primed:
                assert int(primed[k][:4].view(torch.int32).item()) == 0, f"{case.id}: the ticket counter is not left at zero"
        buf.intact()
