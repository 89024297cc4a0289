"""What a refactor of the attention orchestrators (csrc/layers.hip) must not move: every workspace size, and the route
each shape takes.

Sizes.  The size queries of the scalar-attention layer and of the edge_hidden op are dry passes over null operands: host
arithmetic on the dims, no device call, so this file needs no GPU.  tests/golden/attn_workspace_bytes.json holds their
values over a grid of batch sizes, layer widths, arithmetic modes and edge-storage modes, recorded by
`python tests/test_attn_workspace.py --record FILE` with the build of the commit BEFORE the orchestrators were split into
route structs and named steps; the comparison is exact (integers).

Routes.  cgat_debug_nodes_attention_route (include/cgat_hip.h) returns the route structs the orchestrators run on as bit
masks.  ROUTES below says which route a shape takes in which mode; it was written down by reading the predicates of that
same earlier commit (edge_z_fast, edge_zx_fast, edge_ge_fast, edge_gw_fast, edge_infer_fused, edge_ge_ksplit_groups,
edge_rc_shape, rowprog_max_rows and the inline conditions of attn_forward_impl / attn_backward_impl /
edge_first_layer_backward_tail), not from the query's output.  tests/test_hip_golden.py runs the rows that can run
against the oracle.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "golden", "attn_workspace_bytes.json")

BATCHES = [(0, 0), (1, 1), (300, 3600), (2049, 24588), (16400, 196800), (83340, 1000080)]
LAYERS = [(128, 128, 3, 256), (128, 128, 5, 256), (128, 128, 8, 256), (128, 128, 1, 256), (128, 128, 3, 128),
          (128, 128, 3, 384), (128, 64, 3, 256), (64, 64, 3, 64)]
HIDDEN_W2 = [200, 256, 1536]
MODES = ["f32", "bf16x6", "bf16x3", "f16x3", "f16x3c"]
STORAGES = ["f32", "bf16", "f32+gz", "bf16-mma"]


def _plan(N, E):
    from cgat_amd import _lib
    return _lib.Plan(N, E, None, None, None, None, None, None)


def _attn_sizes(N, E, Cn, Ce, H, Hd):
    from cgat_amd import _lib
    plan, p = _plan(N, E), _lib.AttnParams(Cn, Ce, H, Hd, *([None] * 8))
    lib = _lib.lib
    return [lib.cgat_nodes_attention_forward_workspace_bytes(C.byref(plan), C.byref(p)),
            lib.cgat_nodes_attention_infer_workspace_bytes(C.byref(plan), C.byref(p)),
            lib.cgat_nodes_attention_backward_workspace_bytes(C.byref(plan), C.byref(p)),
            lib.cgat_nodes_attention_saved_floats(N, E, H, Hd)]


def _hidden_sizes(N, E, Cn, Ce, W2):
    from cgat_amd import _lib
    plan = _plan(N, E)
    return [_lib.lib.cgat_edge_hidden_forward_workspace_bytes(C.byref(plan), Cn, Ce, W2),
            _lib.lib.cgat_edge_hidden_backward_workspace_bytes(C.byref(plan), Cn, Ce, W2)]


class _modes:
    """Arithmetic mode and edge storage for the block, restored afterwards."""

    def __init__(self, mode, storage):
        self.want = (mode, storage)

    def __enter__(self):
        from cgat_amd import ops
        self.was = (ops.get_bilinear_mode(), ops.get_edge_storage())
        ops.set_bilinear_mode(self.want[0])
        ops.set_edge_storage(self.want[1])

    def __exit__(self, *exc):
        from cgat_amd import ops
        ops.set_bilinear_mode(self.was[0])
        ops.set_edge_storage(self.was[1])


def measure():
    """{"mode/storage": {"attn": {"N,E,C,Ce,H,Hd": [forward, infer, backward, saved floats]},
                         "edge_hidden": {"N,E,C,Ce,W2": [forward, backward]}}}"""
    doc = {}
    for mode in MODES:
        for storage in STORAGES:
            with _modes(mode, storage):
                attn = {",".join(map(str, b + l)): _attn_sizes(*b, *l) for b in BATCHES for l in LAYERS}
                widths = sorted({l[:2] for l in LAYERS})
                hidden = {",".join(map(str, b + w + (w2,))): _hidden_sizes(*b, *w, w2)
                          for b in BATCHES for w in widths for w2 in HIDDEN_W2}
            doc[f"{mode}/{storage}"] = {"attn": attn, "edge_hidden": hidden}
    return doc


def test_workspace_sizes_are_the_recorded_ones():
    want = json.load(open(GOLDEN))["sizes"]
    got = measure()
    assert sorted(got) == sorted(want)
    for key in want:
        for op in ("attn", "edge_hidden"):
            assert sorted(got[key][op]) == sorted(want[key][op]), (key, op)
            for shape, sizes in want[key][op].items():
                assert got[key][op][shape] == sizes, (key, op, shape, got[key][op][shape], sizes)
    assert sum(len(v["attn"]) for v in want.values()) == len(MODES) * len(STORAGES) * len(BATCHES) * len(LAYERS)


def test_modes_are_restored():
    from cgat_amd import ops
    was = (ops.get_bilinear_mode(), ops.get_edge_storage())
    measure()
    assert (ops.get_bilinear_mode(), ops.get_edge_storage()) == was


# ---- routes ---------------------------------------------------------------------------------------------------------
# (mode, storage, (N, E), (C, Ce, H, Hd)) -> (forward routes, backward routes); names as in cgat_amd.debug.ROUTE_BITS.
# The two batches the oracle test runs: 25 and 192 crystals of 12 atoms with 12 neighbours (300 and 2 304 atoms; the
# small-row programs take up to 2 048 rows).
SMALL, ABOVE, LARGE = (300, 3600), (2304, 27648), (83340, 1000080)
BENCH = (128, 128, 3, 256)
# 24-bit modes at the benchmark widths, rebuilt gZ: the K-split edge product below 192 row tiles
_FWD24 = {"fused_infer", "fused_z", "out_fast"}
_BWD24 = {"rc", "vec", "out_fast", "node_small_rows", "ge_ksplit", "gw_launch"}
ROUTES = [
    # f16x3c at the benchmark widths.  N <= 2048: the node side on the small-row programs (projections, g_x as the GEMM
    # pair); E = 3 600 is 15 row tiles of 256 -> six K groups
    ("f16x3c", "f32", SMALL, BENCH, _FWD24, _BWD24),
    # N > 2048: the projections on the per-edge kernel, fc_out_M as one K = H * Hd launch, its input gradients for all
    # heads at once; 9 node row tiles -> g_x as K-split slabs; 108 edge row tiles -> two K groups
    ("f16x3c", "f32", ABOVE, BENCH, _FWD24 | {"proj_fast", "out_one"},
     {"rc", "vec", "out_fast", "out_heads_one", "node_ksplit", "ge_ksplit", "gw_launch"}),
    ("f16x3c", "f32", (2049, 24588), BENCH, _FWD24 | {"proj_fast", "out_one"},
     {"rc", "vec", "out_fast", "out_heads_one", "node_ksplit", "ge_ksplit", "gw_launch"}),
    # the benchmark batch: 326 node and 3 907 edge row tiles (>= 192) -> the plain per-edge launches on both sides
    ("f16x3c", "f32", LARGE, BENCH, _FWD24 | {"proj_fast", "out_one"},
     {"rc", "vec", "out_fast", "out_heads_one", "node_launches", "ge_launch", "gw_launch"}),
    ("bf16x6", "f32", SMALL, BENCH, _FWD24, _BWD24),
    # f16x3: the x_j projection folded into the per-edge kernel, no fused inference (24-bit modes only), no K split;
    # maxima of gZ / e and of Gi / Gj / x -> fp16 forms of the per-edge launches on both sides
    ("f16x3", "f32", SMALL, BENCH, {"zx", "out_fast"},
     {"rc", "vec", "have_scales", "out_fast", "node_small_rows", "node_scales", "ge_launch", "gw_launch"}),
    ("f16x3", "f32", ABOVE, BENCH, {"zx", "proj_fast", "out_fast"},
     {"rc", "vec", "have_scales", "out_fast", "node_launches", "node_scales", "ge_launch", "gw_launch"}),
    # f32: no split kernel anywhere, gZ stored, generic GEMMs
    ("f32", "f32", SMALL, BENCH, set(), {"vec", "node_gemm", "ge_gemm", "gw_gemm"}),
    ("f32", "f32", ABOVE, BENCH, set(), {"vec", "node_gemm", "ge_gemm", "gw_gemm"}),
    # Hd = 128: one column block per head -- not the bit-plane kernels' shape and not the one-launch fc_out_M (odd
    # blocks per head), but gZ is still rebuilt; W2 = 768 is six column blocks -> three K groups
    ("f16x3c", "f32", SMALL, (128, 128, 3, 128), _FWD24, _BWD24),
    # edge storage "f32+gz": gZ stored (column-blocked) at the fast widths, same launches on the stored operand
    ("f16x3c", "f32+gz", SMALL, BENCH, _FWD24, _BWD24 - {"rc"}),
    # bf16 storage of Z: by the six-pass per-edge kernel in the 24-bit modes, by edge_zx in f16x3
    ("f16x3c", "bf16", SMALL, BENCH, _FWD24 | {"z_bf16"}, _BWD24 | {"z_bf16", "z_bf16_six"}),
    ("f16x3", "bf16", SMALL, BENCH, {"zx", "z_bf16", "out_fast"},
     {"rc", "vec", "have_scales", "z_bf16", "out_fast", "node_small_rows", "node_scales", "ge_launch", "gw_launch"}),
    # "bf16-mma": one-pass bf16 operands over the rebuilt rows have no K-split form
    ("f16x3c", "bf16-mma", SMALL, BENCH, _FWD24 | {"z_bf16"},
     (_BWD24 - {"ge_ksplit"}) | {"z_bf16", "z_bf16_six", "ge_launch"}),
    # width 64: nothing of the fast family, the generic tail (and the inference forward is not fused)
    ("f16x3c", "f32", SMALL, (64, 64, 3, 64), set(), {"vec", "node_gemm", "ge_gemm", "gw_gemm"}),
    # Ce = 64 beside C = 128: node side fast, edge side generic on a stored gZ
    ("f16x3c", "f32", SMALL, (128, 64, 3, 256), {"out_fast"},
     {"vec", "out_fast", "node_small_rows", "ge_gemm", "gw_gemm"}),
]


def route_row(mode, storage, batch, layer):
    rows = [r for r in ROUTES if r[:4] == (mode, storage, batch, layer)]
    assert len(rows) == 1
    return rows[0][4], rows[0][5]


def test_every_route_is_named_by_some_shape():
    from cgat_amd import debug
    seen_f, seen_b = set(), set()
    for mode, storage, batch, layer, fwd, bwd in ROUTES:
        with _modes(mode, storage):
            got_f = debug.nodes_attention_route(*batch, *layer, backward=False)
            got_b = debug.nodes_attention_route(*batch, *layer, backward=True)
        assert got_f == fwd, (mode, storage, batch, layer, sorted(got_f), sorted(fwd))
        assert got_b == bwd, (mode, storage, batch, layer, sorted(got_b), sorted(bwd))
        seen_f |= fwd
        seen_b |= bwd
    assert seen_f == set(debug.ROUTE_BITS["forward"])
    assert seen_b == set(debug.ROUTE_BITS["backward"])


def test_infer_fused_query_is_the_route_bit():
    from cgat_amd import _lib, debug
    for mode, storage, batch, layer, fwd, _ in ROUTES:
        with _modes(mode, storage):
            plan, p = _plan(*batch), _lib.AttnParams(*layer, *([None] * 8))
            assert _lib.lib.cgat_nodes_attention_infer_fused(C.byref(plan), C.byref(p)) == int("fused_infer" in fwd)


if __name__ == "__main__":      # python tests/test_attn_workspace.py --record FILE
    out_path = sys.argv[sys.argv.index("--record") + 1]
    doc = {"what": "bytes returned by cgat_nodes_attention_{forward,infer,backward}_workspace_bytes, floats by "
                   "cgat_nodes_attention_saved_floats, bytes by cgat_edge_hidden_{forward,backward}_workspace_bytes",
           "command": "python tests/test_attn_workspace.py --record FILE   (build of the commit before the attention "
                      "orchestrators were split into route structs and steps; no GPU needed)",
           "sizes": measure()}
    json.dump(doc, open(out_path, "w"), indent=0, separators=(",", ":"))
    print(sum(len(v["attn"]) + len(v["edge_hidden"]) for v in doc["sizes"].values()), "shapes recorded")
