"""Shell-indexed edge features (cgat_amd.IndexedEdgeAttr, cgat_nodes_attention_infer_indexed), the checks that need no GPU:
the C ABI's symbols, dry queries of the predicate and the workspace, and the precondition itself pinned to the oracle --
in the shipped network the edge features of every layer are a function of the shell id alone."""
import ctypes as C
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cgat_nodes_attention_infer_indexed_ok", "cgat_nodes_attention_infer_indexed_workspace_bytes",
         "cgat_nodes_attention_infer_indexed")


def test_symbols_in_library_header_and_binding():
    from cgat_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "cgat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in _lib.PROTOTYPES, n
    import cgat_amd as P
    assert P.get_indexed_edge_attr() is False or os.environ.get("CGAT_INDEXED_EDGE_ATTR") == "1"
    for n in ("IndexedEdgeAttr", "set_indexed_edge_attr", "get_indexed_edge_attr"):
        assert hasattr(P, n) and n in P.__all__


def test_dry_queries_predicate_and_workspace():
    """N = 20 000, E = 240 000, H = 3, Hd = 256, R = 13: taken in all four arithmetic modes, not under edge storage bf16,
    not above 256 table rows; the workspace grows with E by the logits and alpha alone (2 * 4 * H bytes per edge: bounded
    here by 16 * H * E plus the 256-byte rounding of the carve-outs)."""
    import cgat_amd  # noqa: F401
    from cgat_amd import _lib, ops
    N, E, H, Hd, R = 20000, 240000, 3, 256, 13
    p = _lib.AttnParams(128, 128, H, Hd, *([0] * 8))

    def plan(e):
        return _lib.Plan(N, e, 0, 0, 0, 0, 0, 0)

    def ok(r, e=E, params=p):
        return _lib.lib.cgat_nodes_attention_infer_indexed_ok(C.byref(plan(e)), C.byref(params), r)

    def ws(e):
        return _lib.lib.cgat_nodes_attention_infer_indexed_workspace_bytes(C.byref(plan(e)), C.byref(p), R)
    prev = (ops.get_bilinear_mode(), ops.get_edge_storage())
    try:
        ops.set_edge_storage("f32")
        for mode in ("f16x3c", "bf16x6", "f16x3", "f32"):
            ops.set_bilinear_mode(mode)
            assert ok(R) == 1, mode
            assert ok(1) == 1 and ok(25) == 1 and ok(65) == 1 and ok(256) == 1, mode
            assert ok(257) == 0 and ok(0) == 0, mode
            assert ok(R, e=E + 1) == 1, mode                       # no E * H % 4 condition
            for c in (64, 128):                                     # C, Ce in {64, 128}; H <= 8; H * Hd <= 2048
                for h in (1, 5, 8):
                    hd = int((2 * c + c) / 1.5)
                    assert ok(R, params=_lib.AttnParams(c, c, h, hd, *([0] * 8))) == 1, (mode, c, h)
            assert ok(R, params=_lib.AttnParams(128, 128, 9, 128, *([0] * 8))) == 0
            assert ok(R, params=_lib.AttnParams(128, 128, 8, 512, *([0] * 8))) == 0
            grow = ws(2 * E) - ws(E)
            assert 0 < grow <= 16 * H * E + 4096, (mode, grow)
            assert ws(E) < 2 * (2 * N * 2 * H * Hd * 4) + 64 * 2 ** 20, (mode, ws(E))   # Pi, Pj and small change: no E * H * Hd
        ops.set_bilinear_mode("f16x3c")
        ops.set_edge_storage("bf16")
        assert ok(R) == 0
    finally:
        ops.set_bilinear_mode(prev[0])
        ops.set_edge_storage(prev[1])


def _tiny_batch():
    import cgat_amd as P
    b, roost = P.synthetic_batch(3, 5, 4, seed=3)
    assert int(b.edge_attr.min()) >= 1 and int(b.edge_attr.max()) <= 4
    return b, roost


def _edge_rows_by_shell(no_hyper):
    """Forward hooks on the oracle's Edge layers: (shell ids, [(edge features going in, edge update coming out), ...])."""
    from oracle import cgat_oracle as O
    b, roost = _tiny_batch()
    torch.manual_seed(2)
    net = O.CGAtNet(200, 16, 3, nbr_embedding_size=16, neighbor_number=4, msg_heads=3, update_edges=True,
                    no_hyper=no_hyper).eval()
    seen = []
    hooks = [g["Edge"].register_forward_hook(lambda m, inp, out: seen.append((inp[2].detach(), out.detach())))
             for g in net.graphs]
    with torch.no_grad():
        net(b, roost)
    for h in hooks:
        h.remove()
    assert len(seen) == 3
    return b.edge_attr, seen


def _spread(shell, rows):
    """Largest deviation between rows of equal shell id, relative to the largest entry."""
    worst = 0.0
    for s in shell.unique():
        r = rows[shell == s]
        worst = max(worst, float((r - r[0]).abs().max()))
    return worst / float(rows.abs().max())


def test_precondition_edge_features_depend_on_shell_alone():
    """The algebra of DESIGN.md section 4 against the oracle: with the shipped no_hyper=True the edge features entering
    every Edge layer and the update it returns are equal on edges of equal shell id (1e-6 relative) -- the lookup form is
    exact for every layer -- and with no_hyper=False (the per-edge hypernetwork update reads the atoms) they are not."""
    shell, seen = _edge_rows_by_shell(True)
    assert shell.unique().numel() > 1
    for k, (ea_in, upd) in enumerate(seen):
        assert _spread(shell, ea_in) <= 1e-6, k
        assert _spread(shell, upd) <= 1e-6, k
    shell, seen = _edge_rows_by_shell(False)
    assert _spread(shell, seen[0][1]) > 1e-3               # the first update already separates them
    assert _spread(shell, seen[1][0]) > 1e-3
