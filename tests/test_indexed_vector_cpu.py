"""The indexed route of vector-attention node layers without a GPU: the switch (default off, env CGAT_INDEXED_VECTOR_ATTN,
getter / setter), the five C entries exported and bound, a table of cgat_edge_hidden_indexed_ok answers, and the dry-run
workspace sizes at the shapes of tests/test_edge_hidden_indexed.py -- the forward's does not grow with E.  No device is
touched."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cgat_edge_hidden_indexed_ok", "cgat_edge_hidden_forward_indexed_workspace_bytes",
         "cgat_edge_hidden_forward_indexed", "cgat_edge_hidden_backward_indexed_workspace_bytes",
         "cgat_edge_hidden_backward_indexed")
MODES = ("f16x3c", "bf16x6", "f16x3", "f32")
CASES = {   # tests/test_edge_hidden_indexed.py: N, E, C, Ce, W2, R
    "small": (301, 701, 128, 128, 512, 13),
    "one_class": (301, 701, 128, 128, 512, 1),
    "exact_pieces": (301, 768, 128, 128, 512, 3),
    "wide": (301, 1207, 128, 128, 2560, 25),
    "large_rows": (2101, 5003, 128, 128, 512, 65),
    "widths": (203, 1207, 64, 32, 192, 13),
    "hub": (301, 1400, 128, 128, 512, 13),
}


class _modes:
    def __init__(self, mode, storage="f32"):
        self.mode, self.storage = mode, storage

    def __enter__(self):
        from cgat_amd import ops
        self.prev = (ops.get_bilinear_mode(), ops.get_edge_storage())
        ops.set_bilinear_mode(self.mode)
        ops.set_edge_storage(self.storage)

    def __exit__(self, *a):
        from cgat_amd import ops
        ops.set_bilinear_mode(self.prev[0])
        ops.set_edge_storage(self.prev[1])


def _switch_in_child(env_value):
    env = {k: v for k, v in os.environ.items() if k != "CGAT_INDEXED_VECTOR_ATTN"}
    if env_value is not None:
        env["CGAT_INDEXED_VECTOR_ATTN"] = env_value
    r = subprocess.run([sys.executable, "-c", "import cgat_amd as P; print(P.get_indexed_vector_attention())"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().splitlines()[-1]


def test_switch_default_env_and_round_trip():
    import cgat_amd as P
    assert _switch_in_child(None) == "False"          # default off
    assert _switch_in_child("1") == "True"
    assert _switch_in_child("0") == "False"
    assert "set_indexed_vector_attention" in P.__all__ and "get_indexed_vector_attention" in P.__all__
    prev = P.get_indexed_vector_attention()
    try:
        P.set_indexed_vector_attention(True)
        assert P.get_indexed_vector_attention() is True
        P.set_indexed_vector_attention(False)
        assert P.get_indexed_vector_attention() is False
    finally:
        P.set_indexed_vector_attention(prev)


def test_symbols_exported_and_bound():
    from cgat_amd import _lib, ops
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.PROTOTYPES, n
    for n in ("EdgeHiddenIndexedFn", "EdgeHiddenHeadsIndexedFn", "edge_hidden_indexed_ok"):
        assert hasattr(ops, n), n
    from cgat_amd import nets                  # (the route predicate: folded into the layer's one route decision)
    assert callable(nets.nodes_route) and "edge_hidden_indexed_ok" in nets.NodeFacts._fields
    assert callable(nets.GATConvNodes.route)


def test_predicate_table():
    from cgat_amd import _lib, ops
    for mode in MODES:
        with _modes(mode):
            for name, (N, E, Cn, Ce, W2, R) in CASES.items():
                plan = _lib.Plan(N, E, 0, 0, 0, 0, 0, 0)
                assert ops.edge_hidden_indexed_ok(plan, Cn, Ce, W2, R), (mode, name)
            plan = _lib.Plan(301, 701, 0, 0, 0, 0, 0, 0)
            assert ops.edge_hidden_indexed_ok(plan, 128, 128, 512, 256), mode
            assert ops.edge_hidden_indexed_ok(plan, 128, 128, 4 * 4096 + 4, 13), mode      # column-wise: no width limit
            assert not ops.edge_hidden_indexed_ok(plan, 128, 128, 512, 257), mode
            assert not ops.edge_hidden_indexed_ok(plan, 128, 128, 512, 0), mode
            assert not ops.edge_hidden_indexed_ok(plan, 128, 128, 510, 13), mode           # W2 % 4 != 0
            assert not ops.edge_hidden_indexed_ok(_lib.Plan(301, 0, 0, 0, 0, 0, 0, 0), 128, 128, 512, 13), mode
            assert not ops.edge_hidden_indexed_ok(_lib.Plan(0, 0, 0, 0, 0, 0, 0, 0), 128, 128, 512, 13), mode
        for storage in ("bf16", "bf16-mma"):
            with _modes(mode, storage):
                assert not ops.edge_hidden_indexed_ok(_lib.Plan(301, 701, 0, 0, 0, 0, 0, 0), 128, 128, 512, 13), (mode, storage)


def test_workspace_sizes():
    """Forward: Pi, Pj [N, W2], Te [R, W2] and the weight image -- the same for every E.  Backward: a gZ buffer of E * W2
    floats (used when g_is_pre = 0), the class-sum partials, Gi, Gj, gT and scratch; no [E, Ce] buffer on top of gZ's."""
    from cgat_amd import _lib
    lib = _lib.lib
    for mode in MODES:
        with _modes(mode):
            for name, (N, E, Cn, Ce, W2, R) in CASES.items():
                plan = _lib.Plan(N, E, 0, 0, 0, 0, 0, 0)
                fwd = lib.cgat_edge_hidden_forward_indexed_workspace_bytes(C.byref(plan), Cn, Ce, W2, R)
                bwd = lib.cgat_edge_hidden_backward_indexed_workspace_bytes(C.byref(plan), Cn, Ce, W2, R)
                print(f"[indexed-vector] {mode} {name}: workspace forward {fwd} backward {bwd}")
                assert 4 * (2 * N + R) * W2 <= fwd < (1 << 36), (mode, name, fwd)
                pieces = lib.cgat_indexed_class_pieces(E, R)
                assert 4 * (E + 2 * N + R + pieces) * W2 <= bwd < (1 << 38), (mode, name, bwd)
                for E2 in (10 * E, 1000000):
                    plan2 = _lib.Plan(N, E2, 0, 0, 0, 0, 0, 0)
                    assert lib.cgat_edge_hidden_forward_indexed_workspace_bytes(C.byref(plan2), Cn, Ce, W2, R) == fwd, \
                        (mode, name, E2)
