"""What the hypernetwork orchestrators (csrc/hnet.hip) run at a given shape and arithmetic mode, and what a refactor of
them must not move: every workspace size.  Host arithmetic only (cgat_debug_hnet_route and the size queries make no
device call), so this file needs no GPU.

Routes.  The table below was written from the predicates of the orchestrators as they stood before the routes became a
named value (csrc/layers.hip of that commit, cited per condition), not from the query's output:
  t_batched      W == 128, an fp16-plane T mode (f16x3, f16x3c), n_hyper <= TPREP_MAX = 8          (:1826, opimage.hip:388)
  w_batched      W == 128 and n_hyper (n_fc + 2) <= WPREP_MAX = 48                                 (:1829)
  chained        w_batched, a mode with weight images (f16x3, f16x3c, bf16x6), n_fc + 1 <= CHAIN_MAX = 5      (:1908)
  ln_fused       W == 128                                                                          (:1978)
  dual           W == 128 in a split mode (all but f32)                                            (:2074, bilinear.hip:1363)
  chain*         chain_ok = w_batched, a mode with weight images, 1 <= n_fc <= CHAIN_MAX           (:1838)
  dw_deferred    chain_ok and n_hyper (n_fc + 2) <= DW_BATCH_MAX = 32                              (:1839)
  chain_queued   dw_deferred, rows <= 8192, 1 < n_hyper <= CHAIN_BATCH_MAX = 4, not f16x3; else `chain` under chain_ok (:1846)
  head_dw_queued dw_deferred (aligned operands); head_dw_rows: not deferred and W == 128           (:2018, :2023)
  dT_side        the overlapped backward                                                           (:2180)
  early_prep     overlapped, rows >= 16384, and the batched dT takes the operands: an fp16-plane T mode, W == 128,
                 n_hyper <= 8                                                                      (:2222, bilwgrad.hip:741, :801)
  dw_side        overlapped in f16x3c; dw_side_ws: overlapped in any other mode                    (:2277, :2196-2200)

Sizes.  tests/golden/hnet_workspace_bytes.json extends the hypernetwork grid of tests/test_bilinear_workspace.py by four
networks, recorded by `python tests/test_hnet_routes_cpu.py --record FILE` with the build of the commit before the
orchestrators moved to csrc/hnet.hip; the comparison is exact (integers)."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
GOLDEN = os.path.join(HERE, "golden", "hnet_workspace_bytes.json")

from test_bilinear_workspace import MODES, ROWS, _hnet_sizes, _mode   # noqa: E402

HNETS = [(128, 5, 2), (128, 3, 8), (128, 2, 5), (128, 1, 2)]

FWD_ALL = {"t_batched", "w_batched", "chained", "ln_fused"}
BWD_F16 = {"t_batched", "w_batched", "dual"}             # the fp16-plane T modes at width 128
DEFER = {"dw_deferred", "head_dw_queued"}
SIDE = {"dT_side"}

# (mode, rows, (W, n_fc, n_hyper), backward, overlapped, routes)
TABLE = [
    # f16x3c at the benchmark network: chains queued up to 8192 rows, one launch per layer above
    ("f16x3c", 1280, (128, 2, 4), False, False, FWD_ALL),
    ("f16x3c", 8192, (128, 2, 4), False, False, FWD_ALL),
    ("f16x3c", 1280, (128, 2, 4), True, False, BWD_F16 | DEFER | {"chain_queued"}),
    ("f16x3c", 8192, (128, 2, 4), True, False, BWD_F16 | DEFER | {"chain_queued"}),
    ("f16x3c", 8193, (128, 2, 4), True, False, BWD_F16 | DEFER | {"chain"}),
    # f16x3: never the batched chains (!mode_f16())
    ("f16x3", 1280, (128, 2, 4), False, False, FWD_ALL),
    ("f16x3", 1280, (128, 2, 4), True, False, BWD_F16 | DEFER | {"chain"}),
    ("f16x3", 8192, (128, 2, 4), True, False, BWD_F16 | DEFER | {"chain"}),
    ("f16x3", 83340, (128, 2, 4), True, False, BWD_F16 | DEFER | {"chain"}),
    # f32 and bf16x3: no weight images (wprep_image_floats() == 0), so no chain and nothing deferred; no batched T
    ("f32", 1280, (128, 2, 4), False, False, {"w_batched", "ln_fused"}),
    ("f32", 1280, (128, 2, 4), True, False, {"w_batched", "head_dw_rows"}),
    ("bf16x3", 1280, (128, 2, 4), False, False, {"w_batched", "ln_fused"}),
    ("bf16x3", 1280, (128, 2, 4), True, False, {"w_batched", "dual", "head_dw_rows"}),
    # bf16x6: chains, but T one by one
    ("bf16x6", 1280, (128, 2, 4), False, False, {"w_batched", "chained", "ln_fused"}),
    ("bf16x6", 1280, (128, 2, 4), True, False, {"w_batched", "dual", "chain_queued"} | DEFER),
    ("bf16x6", 83340, (128, 2, 4), True, False, {"w_batched", "dual", "chain"} | DEFER),
    # n_fc = 5: n_fc + 1 > CHAIN_MAX in the forward; the backward's chain has n_fc layers
    ("f16x3c", 2100, (128, 5, 2), False, False, {"t_batched", "w_batched", "ln_fused"}),
    ("f16x3c", 2100, (128, 5, 2), True, False, BWD_F16 | DEFER | {"chain_queued"}),
    ("f16x3c", 2100, (128, 6, 2), True, False, BWD_F16 | {"head_dw_rows"}),
    # (128, 3, 8): 40 images <= 48, 40 weight gradients > 32
    ("f16x3c", 2100, (128, 3, 8), False, False, FWD_ALL),
    ("f16x3c", 2100, (128, 3, 8), True, False, BWD_F16 | {"chain", "head_dw_rows"}),
    # the capacities themselves: 32 weight gradients wait, 8 chains do not; 48 images are batched, 56 are not
    ("f16x3c", 2100, (128, 2, 8), True, False, BWD_F16 | DEFER | {"chain"}),
    ("f16x3c", 2100, (128, 4, 8), False, False, FWD_ALL),
    ("f16x3c", 2100, (128, 5, 8), False, False, {"t_batched", "ln_fused"}),
    ("f16x3c", 2100, (128, 5, 8), True, False, {"t_batched", "dual", "head_dw_rows"}),
    ("f16x3c", 1280, (128, 2, 5), True, False, BWD_F16 | DEFER | {"chain"}),       # n_hyper > CHAIN_BATCH_MAX
    # one predicted layer: no batched chains
    ("f16x3c", 130, (128, 2, 1), False, False, FWD_ALL),
    ("f16x3c", 130, (128, 2, 1), True, False, BWD_F16 | DEFER | {"chain"}),
    # width 64: every flag off
    ("f16x3c", 130, (64, 2, 2), False, False, set()),
    ("f16x3c", 130, (64, 2, 2), True, False, set()),
    ("f16x3", 130, (64, 2, 2), True, False, set()),
    ("f32", 130, (64, 2, 2), True, False, set()),
    ("f16x3c", 16400, (64, 2, 2), True, True, SIDE | {"dw_side"}),
    # the overlapped backward: where the batched dense weight gradients go, and the early dT preparation
    ("f16x3c", 16383, (128, 2, 2), True, True, BWD_F16 | DEFER | SIDE | {"chain", "dw_side"}),
    ("f16x3c", 16384, (128, 2, 2), True, True, BWD_F16 | DEFER | SIDE | {"chain", "dw_side", "early_prep"}),
    ("f16x3", 16383, (128, 2, 2), True, True, BWD_F16 | DEFER | SIDE | {"chain", "dw_side_ws"}),
    ("f16x3", 16384, (128, 2, 2), True, True, BWD_F16 | DEFER | SIDE | {"chain", "dw_side_ws", "early_prep"}),
    ("bf16x6", 16384, (128, 2, 2), True, True, {"w_batched", "dual", "chain", "dw_side_ws"} | DEFER | SIDE),
    ("f32", 16384, (128, 2, 2), True, True, {"w_batched", "head_dw_rows", "dw_side_ws"} | SIDE),
    ("f16x3c", 1280, (128, 2, 4), True, True, BWD_F16 | DEFER | SIDE | {"chain_queued", "dw_side"}),
    ("f16x3c", 16384, (128, 2, 2), True, False, BWD_F16 | DEFER | {"chain"}),
]


@pytest.mark.parametrize("row", range(len(TABLE)))
def test_route_table(row):
    from cgat_amd import debug
    mode, rows, net, backward, overlapped, want = TABLE[row]
    with _mode(mode):
        got = debug.hnet_route(rows, *net, backward=backward, overlapped=overlapped)
    assert got == want, (TABLE[row][:5], sorted(got), sorted(want))


def test_route_names_cover_the_mask():
    """Every name of the table is a bit of the query, and the forms of one step exclude each other."""
    from cgat_amd import debug
    for mode, rows, net, backward, overlapped, want in TABLE:
        assert want <= set(debug.HNET_ROUTE_BITS["backward" if backward else "forward"])
        assert not {"chain", "chain_queued"} <= want and not {"head_dw_queued", "head_dw_rows"} <= want
        assert not {"dw_side", "dw_side_ws"} <= want
    assert debug.hnet_route(130, 128, 9, 2) == set() and debug.hnet_route(130, 128, 2, 9, backward=True) == set()   # refused


def measure():
    """{mode: {"rows,W,n_fc,n_hyper": [forward, backward, backward side, saved floats]}}"""
    doc = {}
    for mode in MODES:
        with _mode(mode):
            doc[mode] = {",".join(map(str, (n,) + h)): _hnet_sizes(n, *h) for n in ROWS for h in HNETS}
    return doc


def test_workspace_sizes_are_the_recorded_ones():
    want = json.load(open(GOLDEN))["sizes"]
    got = measure()
    assert sorted(got) == sorted(want) == sorted(MODES)
    for mode in want:
        assert sorted(got[mode]) == sorted(want[mode]) and len(want[mode]) == len(ROWS) * len(HNETS), mode
        for shape, sizes in want[mode].items():
            assert got[mode][shape] == sizes, (mode, shape, got[mode][shape], sizes)


if __name__ == "__main__":      # python tests/test_hnet_routes_cpu.py --record FILE
    out_path = sys.argv[sys.argv.index("--record") + 1]
    doc = {"what": "bytes returned by cgat_hnet_{forward,backward,backward_side}_workspace_bytes, floats by cgat_hnet_saved_floats",
           "command": "python tests/test_hnet_routes_cpu.py --record FILE   (build of the commit before the hypernetwork "
                      "orchestrators moved to csrc/hnet.hip; no GPU needed)",
           "sizes": measure()}
    json.dump(doc, open(out_path, "w"), indent=0, separators=(",", ":"))
    print(sum(len(v) for v in doc["sizes"].values()), "sizes recorded")
