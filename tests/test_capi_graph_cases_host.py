"""tests/capi_graph_cases.py against the headers: every function of include/*.h that takes a ``void *stream`` has a capture case, and the
table names nothing the headers do not declare.  No count is written down here and nothing is excluded: a new entry point without a case
fails this file by name.  The cases' own promises (ids, the sequences the issue of each function asks for) are checked too, without a GPU."""
import glob
import os
import re

import capi_graph_cases as G

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
DECLARATION = re.compile(r"\b(?:int|size_t)\s+(fn2\w*)\s*\(([^;{}]*?)\)\s*;", re.S)
COMMENT = re.compile(r"/\*.*?\*/", re.S)


def stream_taking(text):
    """The functions a header's text declares with a ``void *stream`` parameter."""
    return {m.group(1) for m in DECLARATION.finditer(COMMENT.sub(" ", text)) if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2))}


def declared():
    headers = sorted(glob.glob(os.path.join(INCLUDE, "*.h")))
    assert len(headers) >= 7, headers
    names = set()
    for h in headers:
        with open(h) as f:
            found = stream_taking(f.read())
        assert found, f"{h}: no stream-taking declaration found (has the header's style changed?)"
        names |= found
    return names


def test_every_stream_taking_entry_point_has_a_capture_case():
    want, have = declared(), G.covered()
    assert not want - have, f"entry points without a capture case in tests/capi_graph_cases.py: {sorted(want - have)}"
    assert not have - want, f"capture cases for functions no header declares: {sorted(have - want)}"


def test_the_parser_sees_a_new_entry_point():
    """A dummy declaration added to a header's text is found (and would fail the test above by name); one without a stream is not."""
    with open(os.path.join(INCLUDE, "flownet2_hip_census.h")) as f:
        text = f.read()
    grown = text.replace("#if defined(__GNUC__)\n#pragma GCC visibility pop", "int fn2_x(void *stream);\nint fn2_y(int a);\n#if defined(__GNUC__)\n#pragma GCC visibility pop")
    assert grown != text
    assert stream_taking(grown) - stream_taking(text) == {"fn2_x"}
    assert "fn2_x" not in G.covered()
    # multi-line declarations and the size queries next to them
    names = declared()
    assert "fn2_correlation_backward_fused" in names and "fn2_multiscale_scale_grads" in names
    assert "fn2_correlation_backward_fused_workspace_bytes" not in names and "fn2_abi_version" not in names


def test_removing_a_case_is_noticed():
    for victim in ("fn2_multiscale_scale_grads", "fn2c_census_backward"):
        left = {fn for c in G.CASES if victim not in c.fns for fn in c.fns}
        assert declared() - left == {victim}


def _ids(prefix):
    return [c.id for c in G.CASES if c.id.startswith(prefix)]


def test_each_host_side_sequence_has_a_case_of_its_own():
    for name in ("fn2_warp_diff_norm_cat_backward", "fn2_warp_diff_norm_cat_backward_det"):
        assert {i[len(name) + 1:] for i in _ids(name + "-")} == {"null-pair", "c3-tiled", "c3-untiled", "c2"}, name
    B, C, H, W = G.PAIR_GRAD_SHAPES["c3-tiled"]
    assert C == 3 and H >= 16 and W >= 32 and W % 4 == 0                      # the header's conditions for the LDS-window kernel
    B, C, H, W = G.PAIR_GRAD_SHAPES["c3-untiled"]
    assert C == 3 and not (H >= 16 and W >= 32 and W % 4 == 0)
    assert G.PAIR_GRAD_SHAPES["c2"][1] != 3
    ms = [c.id for c in G.CASES if c.id.startswith("fn2_multiscale_l")]
    for entry in ("fn2_multiscale_l1_epe", "fn2_multiscale_loss", "fn2_multiscale_loss_fused"):
        mine = [i[len(entry) + 1:] for i in ms if i.startswith(entry + "-")]
        assert any(i.startswith("unprimed") for i in mine) and any(i.startswith("empty") for i in mine), entry
        assert any(i.endswith("-grads") for i in mine) and any(i.endswith("-nograds") for i in mine), entry
        if entry != "fn2_multiscale_l1_epe":
            assert any("-L1-" in i for i in mine) and any("-L2-" in i for i in mine), entry
    assert any(i.startswith("fn2_multiscale_loss_fused-primed") for i in ms)
    rows = {"F16X2-float32", "MFMA_F32-float32", "H16-float16", "H16-bfloat16", "F64-float64", "DENSE-float32", "DIRECT-float32"}
    for name in ("fn2_correlation_forward", "fn2_correlation_forward_ex", "fn2_correlation_backward", "fn2_correlation_backward_ex"):
        assert {i[len(name) + 1:] for i in _ids(name + "-")} == rows, name
    flownetc = {"F16X2-float32", "H16-float16", "H16-bfloat16", "F64-float64"}     # the rows on FlowNetC's configuration
    for name in ("fn2_correlation_forward_fused", "fn2_correlation_backward_fused"):
        assert {i[len(name) + 1:] for i in _ids(name + "-")} == flownetc, name


def test_inputs_differ_from_seed_to_seed_and_atomic_outputs_have_a_bound():
    for c in G.CASES:
        a, b = c.inputs(1), c.inputs(2)
        assert set(a) == set(b) and not set(a) & (set(c.outputs) | set(c.scratch) | set(c.primed) | set(c.derived)), c.id
        assert any(a[k].numel() and not bool((a[k] == b[k]).all()) for k in a) or all(v.numel() == 0 for v in a.values()), c.id
        assert all(o.kind != "atomic" for o in c.outputs.values()) or c.check is not None, c.id
    atomic = {c.fns[0] for c in G.CASES for o in c.outputs.values() if o.kind == "atomic"}
    assert atomic == {"fn2_resample2d_backward", "fn2_warp_diff_norm_cat_backward", "fn2l_corr_lookup_backward", "fn2s_forward_warp_forward"}
