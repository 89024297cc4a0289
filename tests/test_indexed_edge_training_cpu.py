"""The training route of shell-indexed edge features without a GPU: the C entries are exported and bound, the host-only
predicate answers as include/cgat_hip.h states, and the dry-run sizes show what the route is for -- a saved buffer of
E*H + N*H floats, workspaces that grow with E by a few scalars, the sign words and the class-sum partials per
edge and not by the E x 2*H*Hd pre-activations.  No device is touched."""
import ctypes as C

NAMES = ("cgat_nodes_attention_train_indexed_ok", "cgat_nodes_attention_indexed_saved_floats",
         "cgat_nodes_attention_forward_indexed_workspace_bytes", "cgat_nodes_attention_forward_indexed",
         "cgat_nodes_attention_backward_indexed_workspace_bytes", "cgat_nodes_attention_backward_indexed",
         "cgat_indexed_class_pieces", "cgat_indexed_class_plan", "cgat_indexed_class_plan_workspace_bytes",
         "cgat_debug_nodes_attention_signs_indexed_workspace_bytes",
         "cgat_debug_nodes_attention_signs_indexed")
MODES = ("f16x3c", "bf16x6", "f16x3", "f32")


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


def test_symbols_exported_and_bound():
    import cgat_amd as P
    from cgat_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n) and n in _lib.PROTOTYPES, n
    assert callable(P.set_indexed_edge_training) and callable(P.get_indexed_edge_training)
    assert "set_indexed_edge_training" in P.__all__ and "get_indexed_edge_training" in P.__all__
    assert hasattr(P.debug, "note_attention_indexed")
    prev = P.get_indexed_edge_training()
    try:
        P.set_indexed_edge_training(True)
        assert P.get_indexed_edge_training() is True
        P.set_indexed_edge_training(False)
        assert P.get_indexed_edge_training() is False
    finally:
        P.set_indexed_edge_training(prev)


def test_predicate():
    from cgat_amd import _lib, ops
    plan = _lib.Plan(3000, 36000, 0, 0, 0, 0, 0, 0)
    for mode in MODES:
        with _modes(mode):
            for H in (1, 3, 5, 8):
                for R in (1, 13, 25, 256):
                    assert ops.train_indexed_ok(plan, 128, 128, H, 256, R), (mode, H, R)
                assert not ops.train_indexed_ok(plan, 128, 128, H, 256, 257), (mode, H)
                assert not ops.train_indexed_ok(plan, 128, 128, H, 256, 0), (mode, H)
            assert ops.train_indexed_ok(plan, 64, 64, 3, 128, 13), mode           # C = 64: Hd = 128
            assert not ops.train_indexed_ok(plan, 128, 128, 3, 36, 13), mode      # H * Hd % 32 != 0: no whole mask words
            assert not ops.train_indexed_ok(plan, 128, 128, 3, 254, 13), mode     # Hd % 4 != 0
            assert not ops.train_indexed_ok(plan, 128, 128, 9, 128, 13), mode     # more than 8 heads
        for storage in ("bf16", "bf16-mma"):
            with _modes(mode, storage):
                assert not ops.train_indexed_ok(plan, 128, 128, 3, 256, 13), (mode, storage)
    empty = _lib.Plan(3000, 0, 0, 0, 0, 0, 0, 0)
    assert not ops.train_indexed_ok(empty, 128, 128, 3, 256, 13)


def test_saved_floats():
    """N = 20 000, E = 240 000, H = 3, Hd = 256: at most E*H + N*H*Hd + N*H + 256 floats and below 2 % of the dense
    route's saved buffer.  The buffer holds alpha and ssum: S [N, H*Hd], 3.99 % of the dense buffer by itself, is formed
    again in the backward."""
    from cgat_amd import _lib
    N, E, H, Hd = 20000, 240000, 3, 256
    got = _lib.lib.cgat_nodes_attention_indexed_saved_floats(N, E, H, Hd)
    dense = _lib.lib.cgat_nodes_attention_saved_floats(N, E, H, Hd)
    print(f"[indexed-train] saved floats {got}; dense {dense}: {got / dense:.4f}")
    assert E * H + N * H <= got <= E * H + N * H * Hd + N * H + 256, got
    assert got < 0.02 * dense, (got, dense)
    for n, e, h, hd in ((1, 1, 1, 4), (1281, 15371, 5, 128), (3000, 36001, 8, 256)):       # padding at odd sizes
        g = _lib.lib.cgat_nodes_attention_indexed_saved_floats(n, e, h, hd)
        assert e * h + n * h <= g <= e * h + n * h + 64, (n, e, h, hd, g)


def test_dry_run_workspace_growth():
    """Per additional edge: forward 2 H floats (logits, and nothing else); backward 2 H floats (tt, ga), 2*H*Hd / 8 bytes
    of sign words and 2*H*Hd / 256 floats of class-sum partials -- with slack for the 256-byte rounding of every
    carve-out and for scratch regions sized by E, far below the 4 * 2*H*Hd bytes per edge of stored pre-activations."""
    from cgat_amd import _lib
    lib = _lib.lib
    N, H, Hd, R = 20000, 3, 256, 13
    W2 = 2 * H * Hd
    p = _lib.AttnParams(128, 128, H, Hd, *([0] * 8))
    for mode in MODES:
        with _modes(mode):
            size = {}
            for E in (240000, 480000, 960000):
                plan = _lib.Plan(N, E, 0, 0, 0, 0, 0, 0)
                size[E] = (lib.cgat_nodes_attention_forward_indexed_workspace_bytes(C.byref(plan), C.byref(p), R),
                           lib.cgat_nodes_attention_backward_indexed_workspace_bytes(C.byref(plan), C.byref(p), R),
                           lib.cgat_debug_nodes_attention_signs_indexed_workspace_bytes(C.byref(plan), C.byref(p), R))
                assert all(0 < v < (1 << 40) for v in size[E]), size[E]
            for a, b in ((240000, 480000), (480000, 960000)):
                dE = b - a
                fwd, bwd = (size[b][0] - size[a][0]) / dE, (size[b][1] - size[a][1]) / dE
                per_edge_bwd = 4 * 2 * H + W2 / 8 + 4 * W2 / 256
                print(f"[indexed-train] {mode}: bytes per added edge forward {fwd:.1f} (logits {4 * H}), backward {bwd:.1f} "
                      f"(scalars + mask words + partials {per_edge_bwd:.1f}); stored Z would be {4 * W2}")
                assert 0 <= fwd <= 2 * 4 * H + 8, fwd
                assert per_edge_bwd - 1 <= bwd <= per_edge_bwd + 4 * H + 8, bwd
                assert bwd < 0.05 * 4 * W2


def test_class_piece_bound():
    from cgat_amd import _lib
    for E, R in ((1, 1), (255, 13), (256, 13), (257, 13), (36000, 25), (1000000, 256)):
        assert _lib.lib.cgat_indexed_class_pieces(E, R) == -(-E // 256) + R
