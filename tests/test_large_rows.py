"""The large-batch routes held to the recorded fixtures and the oracle at small shapes.

Below 2 049 rows the small-row programs (csrc/rowprog.hip) take every plain dense product: in the library (Ctx::gemm,
the NODE_SMALL_ROWS / proj_fast / out_one / out_heads_one decisions of csrc/layers.hip) and in the Python modules
(cgat_amd.rowprog.eligible in mlp.py, nets.py, roost.py and ops.linear).  The recorded fixtures (tests/golden/tiny.npz,
base.npz: 14 and 160 atoms) and nearly every oracle case of tests/test_hip_golden.py (<= 1 200 atoms) therefore compare
a branch the benchmark's 83 340 atoms never take.  CGAT_ROWPROG_MAX_ROWS=0 CGAT_ROWPROG_PY_MAX_ROWS=0 switches the
small-row programs off; both are read once per process, so the comparisons run in a child, tests/large_rows_worker.py:

  routes (no GPU)   what the switch moves at small shapes, set by set
  fixtures          every tiny and base case at tol = 1e-4 unchanged; the base cases also in bf16x6, f16x3 and f32
  oracle            every case of tests/oracle_cases.py (the table tests/test_hip_golden.py runs) at TOL unchanged, and
                    the three full-gradient cases
  branch switch     in this process, under the default limits: every case of the table launches at least one small-row
                    program -- a case that did not would prove nothing in the child
  natural shapes    2 304 atoms, just above the limit, in this process without the switch: first=True, vector attention
                    with five heads, the four-layer stack

The child checks per case that no small-row program ran while the library's launch counter grew.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

import oracle_cases
import recipe
from oracle_cases import TOL, compare_with_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "large_rows_worker.py")
CHILD_TIMEOUT = 900
OTHER_MODES = ("bf16x6", "f16x3", "f32")

_TINY_NAMES = sorted(recipe.tiny_cases(oracle_cases.oracle_ns()))
_BASE_NAMES = sorted(recipe.base_cases(oracle_cases.oracle_ns()))

# Table cases the child runs.  A case that launches no small-row program under the default limits
# (test_case_takes_the_small_row_branch_by_default) runs the same kernels either way: it is taken out HERE, by name with
# the reason, never silently.  None so far.
NOT_IN_CHILD = {}
CHILD_CASES = [n for n in oracle_cases.CASES if n not in NOT_IN_CHILD]
GROUP = 4          # cases per child: the start of a process (imports, the library's first launches) stays small beside the
                   # oracle's CPU time, and a child that ends early takes at most four cases with it
_GROUPS = [tuple(CHILD_CASES[i:i + GROUP]) for i in range(0, len(CHILD_CASES), GROUP)]


def _child(args, mode=None):
    env = dict(os.environ, CGAT_ROWPROG_MAX_ROWS="0", CGAT_ROWPROG_PY_MAX_ROWS="0")
    if mode is not None:
        env["CGAT_BILINEAR_MODE"] = mode
    return subprocess.run([sys.executable, WORKER, *args], env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)


_children = {}
_abnormal = []     # children that ended on anything but their last case's line: a fault, a HIP error, a time limit


def _cached_child(args, mode=None):
    """One run of the child per (arguments, mode) and module: the tests of its cases read the same output.  After a child
    that ended abnormally no further child is started on the GPU; the tests that needed one fail naming the first."""
    key = (tuple(args), mode)
    if key not in _children:
        assert not _abnormal, f"not started: an earlier child ended abnormally ({_abnormal[0]})"
        try:
            _children[key] = _child(args, mode)
        except subprocess.TimeoutExpired:
            _abnormal.append(f"{' '.join(args)} [{mode or 'default'}]: no end within {CHILD_TIMEOUT} s")
            raise
        if _children[key].returncode != 0:
            _abnormal.append(f"{' '.join(args)} [{mode or 'default'}]: status {_children[key].returncode}")
    return _children[key]


def _assert_case_ok(res, kind, name):
    """A case passes only on its OK line AND a zero exit status of its child."""
    lines = [l for l in res.stdout.splitlines() if l.startswith(f"LARGE_ROWS {kind} {name} ")]
    tail = "\n".join(res.stderr.strip().splitlines()[-15:])
    assert len(lines) == 1, f"{kind} {name}: no result line (child status {res.returncode})\n{tail}"
    assert lines[0] == f"LARGE_ROWS {kind} {name} OK", lines[0]
    assert res.returncode == 0, f"{kind} {name}: child status {res.returncode}\n{tail}"


# ---- routes: host arithmetic, no GPU --------------------------------------------------------------------------------
NODE_SIDES = {"node_launches", "node_ksplit", "node_gemm"}
_SCALES = {"have_scales", "node_scales"}
# The scalar-attention layer at SMALL = (300, 3600), BENCH widths, small-row programs off.  Forward sets and the f16x3 /
# f32 backward sets are the ABOVE rows of test_attn_workspace.ROUTES (asserted below).  24-bit backward: the ABOVE row has
# node_ksplit, but edge_ge_ksplit_groups never splits below 1 024 rows, so 300 atoms take the plain per-edge launches.
_ATTN_BWD_24 = {"rc", "vec", "out_fast", "out_heads_one", "node_launches", "ge_ksplit", "gw_launch"}
# edge_hidden at test_edge_hidden's `small` shape (301 atoms, 701 edges, both below the K split's 1 024 rows)
_HIDDEN_BWD = {"node_launches", "ge_launch", "gw_launch"}
_GEMM = {"node_gemm", "ge_gemm", "gw_gemm"}
EXPECTED = {
    "f16x3c": dict(attn_bwd=_ATTN_BWD_24, hidden_fwd={"fast"}, hidden_bwd=_HIDDEN_BWD),
    # bf16x6 has no ABOVE row in test_attn_workspace.ROUTES: the same predicates as f16x3c (mode_24bit)
    "bf16x6": dict(attn_fwd={"fused_infer", "fused_z", "out_fast", "proj_fast", "out_one"}, attn_bwd=_ATTN_BWD_24,
                   hidden_fwd={"fast"}, hidden_bwd=_HIDDEN_BWD),
    "f16x3": dict(hidden_fwd={"fast"}, hidden_bwd=_HIDDEN_BWD | _SCALES),
    "f32": dict(hidden_fwd=set(), hidden_bwd=_GEMM),
}


def test_switch_moves_every_small_shape_off_the_small_row_routes():
    """The child's route sets at SMALL / BENCH, test_edge_hidden's `small` shape and a 130-row hypernetwork, against sets
    written down from the predicates of csrc/layers.hip and against the default routes of this process."""
    import large_rows_worker
    from test_attn_workspace import ABOVE, BENCH, SMALL, route_row
    from test_edge_hidden import ROUTES as HIDDEN_ROUTES
    res = _child(["routes"])
    assert res.returncode == 0, res.stderr[-2000:]
    (line,) = [l for l in res.stdout.splitlines() if l.startswith("LARGE_ROWS_ROUTES ")]
    got = {m: {k: set(v) for k, v in d.items()} for m, d in json.loads(line.split(" ", 1)[1]).items()}
    assert sorted(got) == sorted(large_rows_worker.ROUTE_MODES)
    default_hnet = large_rows_worker.route_sets(hnet_rows=2100)        # this process: default limits, 2 100 rows
    for mode, sets in got.items():
        for key, s in sets.items():
            assert "node_small_rows" not in s, (mode, key, sorted(s))
        for key in ("attn_bwd", "hidden_bwd"):
            assert len(sets[key] & NODE_SIDES) == 1, (mode, key, sorted(sets[key]))
        want = dict(EXPECTED[mode])
        if mode != "bf16x6":
            fwd_above, bwd_above = route_row(mode, "f32", ABOVE, BENCH)
            want.setdefault("attn_fwd", fwd_above)
            want.setdefault("attn_bwd", bwd_above)
        for key, w in want.items():
            assert sets[key] == w, (mode, key, sorted(sets[key]), sorted(w))
        # the hypernetwork's routes do not depend on the limit: what the default takes at 2 100 rows
        assert sets["hnet_fwd"] == set(default_hnet[mode]["hnet_fwd"]), (mode, sorted(sets["hnet_fwd"]))
        assert sets["hnet_bwd"] == set(default_hnet[mode]["hnet_bwd"]), (mode, sorted(sets["hnet_bwd"]))
        # what the switch moved, against the same shapes under the default limits
        small_hidden = HIDDEN_ROUTES["small", mode][1]
        assert ("node_small_rows" in small_hidden) == (mode != "f32")
        assert sets["hidden_bwd"] == (small_hidden - {"node_small_rows"}) | (sets["hidden_bwd"] & NODE_SIDES)
        if mode in ("f16x3c", "bf16x6"):
            fwd_small, bwd_small = route_row(mode, "f32", SMALL, BENCH)
            assert sets["attn_fwd"] == fwd_small | {"proj_fast", "out_one"}
            assert sets["attn_bwd"] == (bwd_small - {"node_small_rows"}) | {"out_heads_one", "node_launches"}


# ---- fixtures ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cname", _TINY_NAMES)
def test_golden_tiny_on_the_large_batch_routes(cname):
    """tests/golden/tiny.npz (14 atoms) with the small-row programs off: check_case at 1e-4, as test_golden_tiny."""
    _assert_case_ok(_cached_child(["golden", "tiny"]), "golden_tiny", cname)


@pytest.mark.gpu
@pytest.mark.parametrize("cname", _BASE_NAMES)
@pytest.mark.parametrize("mode", ("default",) + OTHER_MODES)
def test_golden_base_on_the_large_batch_routes(mode, cname):
    """tests/golden/base.npz (160 atoms) with the small-row programs off, in the arithmetic mode the suite runs in and in
    the three others: check_case at 1e-4, as test_golden_base."""
    _assert_case_ok(_cached_child(["golden", "base"], None if mode == "default" else mode), "golden_base", cname)


# ---- oracle -----------------------------------------------------------------------------------------------------------
def _group_of(name):
    (grp,) = [g for g in _GROUPS if name in g]
    return grp


@pytest.mark.gpu
@pytest.mark.parametrize("name", CHILD_CASES)
def test_oracle_case_on_the_large_batch_routes(name):
    """One case of tests/oracle_cases.py through compare_with_oracle at TOL in a child with the small-row programs off."""
    _assert_case_ok(_cached_child(["oracle", *_group_of(name)]), "oracle", name)


@pytest.mark.gpu
@pytest.mark.parametrize("cname", _BASE_NAMES)
def test_full_gradients_on_the_large_batch_routes(cname):
    """test_golden_base_full_gradients_vs_oracle's body (admission limits included) with the small-row programs off."""
    _assert_case_ok(_cached_child(["full_gradients"]), "full_gradients", cname)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(oracle_cases.CASES))
def test_case_takes_the_small_row_branch_by_default(name):
    """The product's forward + backward of a table case in THIS process, default limits: it launches at least one
    small-row program, so the child's run of the same case is a run on other kernels."""
    from cgat_amd import ops, rowprog
    assert rowprog.MAX_ROWS > 0, "this test needs the default limits (CGAT_ROWPROG_*MAX_ROWS unset)"
    mk_prod, _, inputs, call = oracle_cases.case(name)
    ops.prof_enable(True)
    try:
        ops.prof_reset()
        oracle_cases.run_product_only(mk_prod, inputs, call)
        n = ops.prof_get("rowprog")[0]
    finally:
        ops.prof_reset()
        ops.prof_enable(False)
    print(f"{name}: {n} small-row programs under the default limits")
    assert (n >= 1) == (name not in NOT_IN_CHILD), (name, n)


# ---- natural shapes just above the limit: this process, no switch -----------------------------------------------------
def _layer_above_the_limit(heads, **kw):
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b, _ = P.synthetic_batch(192, 12, 12)
    g = torch.Generator().manual_seed(6)
    N, E = b.num_nodes, b.edge_index.shape[1]
    assert N > 2048 and (N, E) == (2304, 27648)
    inputs = {"x": torch.randn(N, 128, generator=g), "edge_index": b.edge_index,
              "edge_attr": torch.randn(E, 128, generator=g), "x_0": torch.randn(N, 128, generator=g)}
    call = lambda m, i: m(i["x"], i["edge_index"], i["edge_attr"], i["x_0"])
    compare_with_oracle(lambda: P.GATConvNodes(128, 128, 128, heads, **kw), lambda: O.GATConvNodes(128, 128, 128, heads, **kw),
                        inputs, call, tol=TOL)


@pytest.mark.gpu
def test_first_layer_vs_oracle_just_above_the_limit():
    """GATConvNodes(128, 128, 128, 3, first=True) at 2 304 atoms / 27 648 edges: H_Net_0 inside the layer and the node
    projections on the per-edge kernel, where the default configuration really changes branch."""
    _layer_above_the_limit(3, first=True)


@pytest.mark.gpu
def test_vector_attention_five_heads_vs_oracle_just_above_the_limit():
    """GATConvNodes(128, 128, 128, 5, vector_attention=True) on the same batch: edge_hidden's node side and the per-head
    second layers (HeadsLinearFn) past the small-row limit."""
    _layer_above_the_limit(5, vector_attention=True)


@pytest.mark.gpu
def test_four_layer_stack_vs_oracle_just_above_the_limit():
    """CGAtNet(200, 128, 4, msg_heads=3, neighbor_number=4, update_edges=True) at 2 304 atoms with 4 neighbours (E = 9 216,
    as many edges as test_full_stack_vs_oracle_random_init): embedding, edge updates' node-sized products and four node
    layers on the large-batch kernels; 192 crystals keep the output head and Roost on the small-row programs."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b, roost = P.synthetic_batch(192, 12, 4)
    N, E = b.num_nodes, b.edge_index.shape[1]
    assert N > 2048 and (N, E) == (2304, 9216)
    inputs = {"x": b.x, "edge_index": b.edge_index, "edge_attr": b.edge_attr, "batch": b.batch,
              "r0": roost[0], "r1": roost[1], "r2": roost[2], "r3": roost[3], "r4": roost[4]}

    def call(m, i):
        bb = recipe.GraphBatch(i["x"], i["edge_index"], i["edge_attr"], i["batch"])
        return m(bb, (t for t in (i["r0"], i["r1"], i["r2"], i["r3"], i["r4"])))
    mk = lambda ns: (lambda: ns.CGAtNet(200, 128, 4, msg_heads=3, neighbor_number=4, update_edges=True))
    compare_with_oracle(mk(P), mk(O), inputs, call, tol=TOL)
