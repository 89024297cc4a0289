"""The forward without grad of the scalar-attention node layer (ops.nodes_attention_infer, cgat_nodes_attention_infer):
taken under torch.no_grad() / when nothing requires grad, bit-identical to the training forward, no saved buffer, and at
the benchmark widths no per-edge activations (the logits launch + the fused message / weighted-sum launch of
csrc/edgez.hip)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def test_infer_symbols_and_dry_run_sizes():
    """CPU: the three entry points are exported and bound; at BASELINE configs[1] (1 000 crystals, N = 20 000, E = 240 000,
    C = Ce = 128, H = 3, Hd = 256) in f16x3c the fused route is taken and its workspace is a fraction of what the training
    forward needs (workspace + saved buffer).  Dry-run queries: no device is touched."""
    import cgat_amd  # noqa: F401
    from cgat_amd import _lib, ops
    lib = C.CDLL(_lib.LIB_PATH)
    names = ("cgat_nodes_attention_infer_fused", "cgat_nodes_attention_infer_workspace_bytes", "cgat_nodes_attention_infer")
    for n in names:
        assert hasattr(lib, n) and n in _lib.PROTOTYPES
    N, E, H, Hd = 20000, 240000, 3, 256
    plan = _lib.Plan(N, E, 0, 0, 0, 0, 0, 0)
    p = _lib.AttnParams(128, 128, H, Hd, *([0] * 8))
    prev = ops.get_bilinear_mode()
    try:
        ops.set_bilinear_mode("f16x3c")
        assert _lib.lib.cgat_nodes_attention_infer_fused(C.byref(plan), C.byref(p)) == 1
        inf = _lib.lib.cgat_nodes_attention_infer_workspace_bytes(C.byref(plan), C.byref(p))
        fwd = _lib.lib.cgat_nodes_attention_forward_workspace_bytes(C.byref(plan), C.byref(p))
        saved = _lib.lib.cgat_nodes_attention_saved_floats(N, E, H, Hd)
        assert inf < 0.25 * (fwd + 4 * saved), (inf, fwd, saved)
        ops.set_bilinear_mode("f16x3")        # the K = 256 per-edge kernel: no fused form, the saved buffer in the workspace
        assert _lib.lib.cgat_nodes_attention_infer_fused(C.byref(plan), C.byref(p)) == 0
        assert _lib.lib.cgat_nodes_attention_infer_workspace_bytes(C.byref(plan), C.byref(p)) >= 4 * saved
    finally:
        ops.set_bilinear_mode(prev)


# ---------------------------------------------------------------------------------------------------------------------
def _ragged_graph(seed=41, odd=False):
    """E not a multiple of 256, many atoms without incoming edges, segments of 65-256 rows, one hub of 3 000 rows, edges
    in random order.  E % 4 == 0 (the training forward's S is then 16-byte aligned and its weighted sum takes the
    vector / long-segment kernels), or odd (its scalar kernel: one chain over every segment, the hub included)."""
    rs = np.random.RandomState(seed)
    N = 5000
    deg = np.zeros(N, dtype=np.int64)
    deg[0] = 3000
    deg[1:41] = rs.randint(65, 257, size=40)
    deg[41:2400] = rs.randint(0, 25, size=2359)          # ordinary atoms, some of them without incoming edges
    E = int(deg.sum())
    deg[41] += (1 if E % 2 == 0 else 0) if odd else (4 - E % 4) % 4 + (4 if (E + (4 - E % 4) % 4) % 256 == 0 else 0)
    E = int(deg.sum())
    dst = np.repeat(np.arange(N), deg)
    src = rs.randint(0, N, size=E)
    order = rs.permutation(E)
    ei = torch.from_numpy(np.stack([src[order], dst[order]])).long()
    assert E % 256 != 0 and E > 128 * 256
    return N, ei


def _graph(kind):
    import cgat_amd as P
    if kind in ("ragged", "ragged_odd"):
        return _ragged_graph(odd=kind == "ragged_odd")
    b, _ = P.synthetic_batch({"c150": 150, "c1000": 1000}[kind], 20, 12, seed=5)
    return b.num_nodes, b.edge_index


def _inputs(N, ei, seed=6):
    g = torch.Generator().manual_seed(seed)
    E = ei.shape[1]
    return (torch.randn(N, 128, generator=g).to(DEV), ei.to(DEV), torch.randn(E, 128, generator=g).to(DEV),
            torch.randn(N, 128, generator=g).to(DEV))


def _layer(first):
    import cgat_amd as P
    torch.manual_seed(1)
    return P.GATConvNodes(128, 128, 128, 3, concat=True, first=first).to(DEV)


class _mode:
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


def _tags(fn):
    from cgat_amd import ops
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.prof_enable(False)
    return out, {t: ops.prof_get(t)[0] for t in ("edge_logits", "edge_msg_wsum", "edge_z", "seg_wsum")}


@pytest.mark.gpu
def test_no_grad_layer_allocates_no_saved_buffer():
    """150 crystals (N = 3 000, E = 36 000): after a warm-up call, a no_grad layer call raises the peak allocation by far
    less than the per-edge activations Z would take (E * 2 * H * Hd * 4 bytes; the training forward allocates more than
    that for its saved buffer).  What remains is the output and the hypernetwork's own saved state."""
    N, ei = _graph("c150")
    x, ei, e, x0 = _inputs(N, ei)
    layer = _layer(False)
    E, H, Hd = ei.shape[1], 3, 256
    with torch.no_grad():
        layer(x, ei, e, x0)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = layer(x, ei, e, x0)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    assert y.shape == (N, 128)
    assert rise < 0.25 * E * 2 * H * Hd * 4, (rise, E * 2 * H * Hd * 4)


@pytest.mark.gpu
def test_route_by_grad_mode():
    """Under no_grad the logits and fused weighted-sum launches run and the per-edge Z launch and seg_wsum do not; with
    grad enabled it is the other way round."""
    N, ei = _graph("c150")
    x, ei, e, x0 = _inputs(N, ei)
    layer = _layer(False)
    with torch.no_grad():
        _, t = _tags(lambda: layer(x, ei, e, x0))
        route = layer.route(x, ei, e)
    assert t["edge_logits"] > 0 and t["edge_msg_wsum"] > 0 and t["edge_z"] == 0 and t["seg_wsum"] == 0, t
    assert route.kind in ("scalar", "layer_fused") and route.no_grad and not route.indexed, route
    _, t = _tags(lambda: layer(x.clone().requires_grad_(True), ei, e, x0))
    assert t["edge_logits"] == 0 and t["edge_msg_wsum"] == 0 and t["edge_z"] > 0 and t["seg_wsum"] > 0, t
    route = layer.route(x.clone().requires_grad_(True), ei, e)
    assert route.kind in ("scalar", "layer_fused") and not route.no_grad and not route.indexed, route


def _check_layer_bits(kind, mode, storage="f32", fused=True):
    N, ei = _graph(kind)
    x, ei, e, x0 = _inputs(N, ei)
    with _mode(mode, storage):
        for first in (True, False):
            layer = _layer(first)
            want = layer(x.clone().requires_grad_(True), ei, e.clone().requires_grad_(True), x0).detach()
            with torch.no_grad():
                got, t = _tags(lambda: layer(x, ei, e, x0))
                assert layer.route(x, ei, e).no_grad      # (fused or not: the library's choice behind the no-grad entry)
            assert (t["edge_msg_wsum"] > 0) == fused and t["edge_z"] == (0 if fused else t["edge_z"]), t
            assert torch.equal(got, want), (kind, mode, storage, first, float((got - want).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["c150", "c1000", "ragged", "ragged_odd"])
@pytest.mark.parametrize("mode", ["f16x3c", "bf16x6"])
def test_layer_bit_identical_to_training_forward(kind, mode):
    """ragged_odd: E * H % 4 != 0, where the training forward sums with its scalar kernel -- the entry point then runs
    the training forward's launches (no fused form), still without grad."""
    _check_layer_bits(kind, mode, fused=kind != "ragged_odd")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["c150", "c1000", "ragged"])
def test_layer_bit_identical_bf16_storage(kind):
    """Edge storage bf16: the message values are rounded to bf16 before LeakyReLU, as the stored Z is."""
    _check_layer_bits(kind, "f16x3c", storage="bf16")


@pytest.mark.gpu
def test_layer_bit_identical_fallback_mode():
    """f16x3 (the K = 256 per-edge kernel) has no fused form: the entry point runs the training forward's launches."""
    _check_layer_bits("c150", "f16x3", fused=False)


@pytest.mark.gpu
@pytest.mark.parametrize("embedding", [False, True])
def test_network_eval_route_on_equals_off(embedding):
    """CGAtNet(200, 128, 4, msg_heads=3) in eval() on 150 crystals under no_grad: the route on and the opt-out give the
    same bits (also the graph embedding)."""
    import cgat_amd as P
    b, roost = P.synthetic_batch(150, 20, 12, seed=7)
    b = b.to(DEV)
    roost = tuple(t.to(DEV) for t in roost)
    torch.manual_seed(1)
    net = P.CGAtNet(200, 128, 4, msg_heads=3, neighbor_number=12, update_edges=True).to(DEV).eval()
    outs = {}
    try:
        for on in (True, False):
            P.set_fused_inference(on)
            with torch.no_grad():
                out, t = _tags(lambda: net(b, roost, return_graph_embedding=embedding))
            assert (t["edge_msg_wsum"] > 0) == on, t
            outs[on] = out
    finally:
        P.set_fused_inference(True)
    a, c = outs[True], outs[False]
    for u, v in zip(a if isinstance(a, tuple) else (a,), c if isinstance(c, tuple) else (c,)):
        assert torch.equal(u, v)


@pytest.mark.gpu
def test_inference_route_vs_oracle():
    """150 crystals through the inference route against the oracle's forward, at the flat tolerance of
    test_hip_golden.py::test_nodes_layer_vs_oracle_above_small_row_limit (1e-4 of the largest output)."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b, _ = P.synthetic_batch(150, 20, 12, seed=5)
    g = torch.Generator().manual_seed(6)
    N, E = b.num_nodes, b.edge_index.shape[1]
    x, e, x0 = torch.randn(N, 128, generator=g), torch.randn(E, 128, generator=g), torch.randn(N, 128, generator=g)
    torch.manual_seed(1)
    om = O.GATConvNodes(128, 128, 128, 3, concat=True)
    pm = P.GATConvNodes(128, 128, 128, 3, concat=True)
    pm.load_state_dict(om.state_dict())
    pm = pm.to(DEV)
    with torch.no_grad():
        want = om(x, b.edge_index, e, x0)
        got, t = _tags(lambda: pm(x.to(DEV), b.edge_index.to(DEV), e.to(DEV), x0.to(DEV)))
    assert t["edge_msg_wsum"] > 0, t
    err = float((got.cpu() - want).abs().max())
    assert err <= 1e-4 * float(want.abs().max()), err


@pytest.mark.gpu
def test_inference_deterministic_and_captured():
    """Two inference calls give the same bits; an eval forward captured with torch.cuda.graph replays to the eager bits
    (child process: tests/infer_capture_worker.py)."""
    N, ei = _graph("ragged")
    x, ei, e, x0 = _inputs(N, ei)
    layer = _layer(False)
    with torch.no_grad():
        y1, y2 = layer(x, ei, e, x0), layer(x, ei, e, x0)
    assert torch.equal(y1, y2)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "infer_capture_worker.py")], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "INFER_CAPTURE_OK" in r.stdout, r.stdout[-2000:]
