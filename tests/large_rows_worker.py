"""Child process of tests/test_large_rows.py.  The small-row programs (csrc/rowprog.hip) take every dense product of at
most 2 048 rows, in the library (Ctx::gemm, the route structs of csrc/layers.hip) and in the Python modules
(cgat_amd.rowprog.eligible); both limits are read once per process, from CGAT_ROWPROG_MAX_ROWS and
CGAT_ROWPROG_PY_MAX_ROWS.  The parent starts this file with both set to 0, so that the recorded fixtures (N = 14 and 160)
and the oracle cases (N <= 1 200) run on the kernels the benchmark's 83 340 atoms run on.

  routes               the route sets of the scalar-attention layer, the edge_hidden op and the hypernetwork at small
                       shapes, as one JSON line (host arithmetic: no GPU)
  golden <tiny|base>   every case of that fixture file through golden_util.check_case at tol = 1e-4
  oracle <name>...     cases of tests/oracle_cases.py through compare_with_oracle at TOL
  full_gradients       the three base cases through oracle_cases.full_gradients_vs_oracle

Every case runs between ops.prof_reset() and a check that NO small-row program was launched while the library's launch
counter grew: the evidence that the comparison ran on the other branch.  One line per case,
    LARGE_ROWS <kind> <case> OK          or          LARGE_ROWS <kind> <case> FAIL <first line of the assertion>
An AssertionError fails its case and the next one runs; any other exception ends the process at once with a non-zero
status (after a fault nothing more is started on the GPU here)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

ROUTE_MODES = ("f16x3c", "bf16x6", "f16x3", "f32")
HNET_SHAPE = (130, 128, 2, 2)


def _switched_off():
    from cgat_amd import rowprog
    assert rowprog.MAX_ROWS == 0, f"cgat_amd.rowprog.MAX_ROWS is {rowprog.MAX_ROWS}: start this file with " \
                                  "CGAT_ROWPROG_MAX_ROWS=0 CGAT_ROWPROG_PY_MAX_ROWS=0"


def route_sets(hnet_rows=HNET_SHAPE[0]):
    """{mode: {"attn_fwd": [...], "attn_bwd": [...], "hidden_fwd": ..., "hidden_bwd": ..., "hnet_fwd": ..., "hnet_bwd": ...}}
    at the SMALL batch / BENCH layer of test_attn_workspace.py, the `small` shape of test_edge_hidden.py and the
    hypernetwork of HNET_SHAPE with `hnet_rows` rows, in the limits this process started with."""
    from cgat_amd import debug, ops
    from test_attn_workspace import BENCH, SMALL
    from test_edge_hidden import SHAPES
    was = ops.get_bilinear_mode()
    doc = {}
    try:
        for mode in ROUTE_MODES:
            ops.set_bilinear_mode(mode)
            doc[mode] = {
                "attn_fwd": sorted(debug.nodes_attention_route(*SMALL, *BENCH, backward=False)),
                "attn_bwd": sorted(debug.nodes_attention_route(*SMALL, *BENCH, backward=True)),
                "hidden_fwd": sorted(debug.edge_hidden_route(*SHAPES["small"])),
                "hidden_bwd": sorted(debug.edge_hidden_route(*SHAPES["small"], backward=True)),
                "hnet_fwd": sorted(debug.hnet_route(hnet_rows, *HNET_SHAPE[1:])),
                "hnet_bwd": sorted(debug.hnet_route(hnet_rows, *HNET_SHAPE[1:], backward=True)),
            }
    finally:
        ops.set_bilinear_mode(was)
    return doc


def routes():
    _switched_off()
    print("LARGE_ROWS_ROUTES " + json.dumps(route_sets()))


def _run_cases(kind, names, run_one):
    """run_one(name) under the launch counters; prints the case's line.  An exception other than AssertionError is not
    caught: it ends the process."""
    from cgat_amd import ops
    _switched_off()
    for name in names:
        ops.prof_enable(True)
        ops.prof_reset()
        before = ops.prof_launches()
        try:
            run_one(name)
            small = ops.prof_get("rowprog")[0]
            assert small == 0, f"{small} small-row programs were launched"
            assert ops.prof_launches() > before, "the library launched nothing"
            line = "OK"
        except AssertionError as err:
            line = "FAIL " + (str(err).strip().splitlines() or ["AssertionError"])[0]
        print(f"LARGE_ROWS {kind} {name} {line}", flush=True)
        ops.prof_reset()
        ops.prof_enable(False)


def golden(which):
    import recipe
    from golden_util import check_case
    from oracle_cases import TOL, product_ns
    cases = {"tiny": recipe.tiny_cases, "base": recipe.base_cases}[which](product_ns())
    _run_cases(f"golden_{which}", sorted(cases),
               lambda n: check_case(f"{which}.npz", n, cases[n], device="cuda:0", tol=TOL))


def oracle(names):
    import oracle_cases
    _run_cases("oracle", names, lambda n: oracle_cases.compare_with_oracle(
        *oracle_cases.case(n), tol=oracle_cases.TOL, label=f"large rows: {n}"))


def full_gradients():
    import recipe
    import oracle_cases
    names = sorted(recipe.base_cases(oracle_cases.oracle_ns()))
    _run_cases("full_gradients", names, oracle_cases.full_gradients_vs_oracle)


if __name__ == "__main__":
    cmd = sys.argv[1]
    {"routes": routes, "golden": lambda: golden(sys.argv[2]), "oracle": lambda: oracle(sys.argv[2:]),
     "full_gradients": full_gradients}[cmd]()
