"""Host-side model of the neighbour row blocks the f16x2 correlation backward walks (no GPU).  A task (row group rg of 4 centre lattice
rows) meets the NU = 6 blocks u of 4 neighbour lattice rows 4rg - 10 + 4u .. +3; only the blocks with a row inside the parity lattice
[0, HL) are walked (`bwd_u_range`, csrc/corr_params.h).  The rule is restated here, checked against brute force, read back from the
source, and the per-workgroup step counts of the persistent kernel are modelled from its task order (csrc/correlation_f16x2_bwd.hip:
channel group fastest, then row group, gradient, y parity, batch item; workgroup w runs tasks xcd_remap(w), + 256, ...)."""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "flownet2-pytorch_amd", "csrc")
DR, NU = 10, 6


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def u_range(rg, HL, dr=DR, nu=NU):
    """bwd_u_range of corr_params.h (Python's >> floors like the arithmetic shift there)."""
    lo, hi = (dr - 4 * rg) >> 2, (HL - 1 + dr - 4 * rg) >> 2
    return max(lo, 0), min(hi, nu - 1)


def xcd_remap(bid, nblk, nx=8):
    q, r = divmod(nblk, nx)
    xcd, idx = bid % nx, bid // nx
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + idx


def steps_per_workgroup(B, C, H, W, max_grid=256):
    """Row-block steps each workgroup of corr_bwd_f16x2 executes (both gradients in one launch)."""
    HL, NRG, NCGR = H // 2, (H // 2 + 3) // 4, C // 64
    ntasks = 2 * B * 2 * NRG * NCGR
    grid = min(ntasks, max_grid)
    out = []
    for w in range(grid):
        n = 0
        for t in range(xcd_remap(w, grid), ntasks, grid):
            rg = (t // NCGR) % NRG
            lo, hi = u_range(rg, HL)
            n += hi - lo + 1
        out.append(n)
    return out, ntasks


MAX_GRID = 256
BWD_FILES = ("correlation_f16x2_bwd.hip", "correlation_f16x2_bwd_wide.hip", "correlation_f16_bwd.hip")


def wpx_bwd_wide():
    """WPX of the column-window backward, read out of its source."""
    m = re.search(r"^constexpr int WPX = (\d+);", src("correlation_f16x2_bwd_wide.hip"), re.M)
    return int(m.group(1))


def bwd_ntasks(B, C, H, nxw=1):
    """Tasks of one backward launch (both gradients): 2 B 2 NRG (C / 64), times the centre windows of the wide kernel."""
    return 2 * B * 2 * ((H // 2 + 3) // 4) * nxw * (C // 64)


def _pairs(ntasks, decode, max_grid=MAX_GRID):
    grid = min(ntasks, max_grid)
    out = []
    for w in range(grid):
        ts = list(range(xcd_remap(w, grid), ntasks, grid))
        out.append([(decode(t0), decode(t1)) for t0, t1 in zip(ts, ts[1:])])
    return out


def handovers(B, C, H, W, flip_outer=False):
    """For each workgroup of corr_bwd_f16x2 the (task, next task) pairs it runs, each task decoded to (cg, rg, gradient, py, n)
    in get_task's order: channel group fastest, then row group, gradient, y parity, batch item.  A workgroup with one task has
    no pair.  flip_outer: the order of correlation_f16_bwd.hip (half / bfloat16): ..., row group, y parity, item, gradient."""
    NRG, NCGR = (H // 2 + 3) // 4, C // 64

    def decode(t):
        cg, t = t % NCGR, t // NCGR
        rg, t = t % NRG, t // NRG
        if flip_outer:
            py, t = t & 1, t >> 1
            return cg, rg, t // B, py, t % B
        flip, t = t % 2, t >> 1
        return cg, rg, flip, t & 1, t >> 1
    return _pairs(bwd_ntasks(B, C, H), decode)


def handovers_wide(B, C, H, W):
    """The same for corr_bwd_f16x2_wide, tasks decoded to (cg, rg, gradient, py, n, xw): NXW = ceil(W / WPX) centre windows, in
    that kernel's get_task order -- channel group fastest, then window, row group, y parity, item, gradient."""
    NRG, NCGR, NXW = (H // 2 + 3) // 4, C // 64, -(-W // wpx_bwd_wide())

    def decode(t):
        cg, t = t % NCGR, t // NCGR
        xw, t = t % NXW, t // NXW
        rg, t = t % NRG, t // NRG
        py, t = t & 1, t >> 1
        return cg, rg, t // B, py, t % B, xw
    return _pairs(bwd_ntasks(B, C, H, nxw=NXW), decode)


def test_range_is_the_blocks_that_meet_the_image():
    for HL in range(1, 41):
        for rg in range((HL + 3) // 4):
            real = [u for u in range(NU) if any(0 <= 4 * rg - DR + 4 * u + r < HL for r in range(4))]
            lo, hi = u_range(rg, HL)
            assert real == list(range(lo, hi + 1)), (HL, rg, real, lo, hi)
            assert lo <= 2 <= hi or lo <= 3 <= hi                     # never empty: a block that holds centre rows meets the image
            assert lo <= 2 <= hi, (HL, rg)                            # ... and u = 2, the block the operand sample reads, is one of them
            # the rule as correlation_mfma_bwd.hip states it
            assert all((4 * rg - DR + 4 * u + 3 >= 0 and 4 * rg - DR + 4 * u <= HL - 1) == (lo <= u <= hi) for u in range(NU))


def test_rule_is_in_the_sources():
    s = src("corr_params.h")
    assert "__host__ __device__ constexpr URange bwd_u_range(int rg, int HL, int dr = 10, int nu = 6)" in s
    assert "const int lo = (dr - 4 * rg) >> 2, hi = (HL - 1 + dr - 4 * rg) >> 2;" in s
    assert "return URange{lo < 0 ? 0 : lo, hi > nu - 1 ? nu - 1 : hi};" in s
    k = src("correlation_f16x2_bwd.hip")
    assert "constexpr int DR = 10, D = 21, NU = 6;" in k and "URange r = bwd_u_range(k.rg, HL, DR, NU);" in k
    assert "const unsigned grid = ntasks < 256 ? (unsigned)ntasks : 256u;" in k
    assert "k.cg = t % p.NCGR; t /= p.NCGR;" in k and "k.rg = t % p.NRG; t /= p.NRG;" in k    # the task order modelled above
    # both wave roles walk the same range
    assert k.count("const URange ur = task_u(tk);") == 2


def test_benchmark_shape_is_balanced():
    """8x256x48x64: row groups walk 4, 5, 6, 6, 5, 4 blocks; every workgroup's three tasks have row groups {0, 2, 4} or {1, 3, 5}, i.e.
    15 steps of the 18 the full loop ran -- for every workgroup, so none keeps the old length."""
    assert [u_range(rg, 24)[1] - u_range(rg, 24)[0] + 1 for rg in range(6)] == [4, 5, 6, 6, 5, 4]
    steps, ntasks = steps_per_workgroup(8, 256, 48, 64)
    assert ntasks == 768 and len(steps) == 256
    assert set(steps) == {15}
    assert sum(steps) == 15 * 256 and sum(steps) % 256 == 0 and sum(steps) // 256 == 15
    assert sorted(xcd_remap(w, 256) for w in range(256)) == list(range(256))


def test_print_spread_of_other_shapes():
    """For DESIGN 4.3 / 4.4 (no assertion): the per-workgroup spread where the counts do not balance -- 56 rows (Sintel-size maps, 56 x 128:
    the wide kernel has the narrow kernel's row geometry per 64-px window and pass) and smaller batches of the 48 x 64 map."""
    for shape in ((8, 256, 56, 128), (8, 256, 56, 64), (1, 256, 48, 64), (4, 256, 48, 64)):
        B, C, H, W = shape
        steps, ntasks = steps_per_workgroup(B, C, H, min(W, 64))
        full = [6 * len(range(xcd_remap(w, len(steps)), ntasks, len(steps))) for w in range(len(steps))]
        print("%s: tasks %d, steps per workgroup min %d max %d (all six blocks: max %d), total %d of %d"
              % (shape, ntasks, min(steps), max(steps), max(full), sum(steps), sum(full)))
