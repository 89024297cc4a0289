"""The forward without grad of the scalar-attention node layer at the shapes the harness' scalar-attention network runs
(lightning_module.py --vector_attention: msg_heads = 5, max_nbr = 24): H * Hd = 1280 (up to 2048) and few-row batches
(64 crystals, below 128 row tiles of 256).  The fused route (edge_logits + edge_msg_wsum, csrc/edgez.hip) is taken
there, forms no per-edge activation, and stays bit-identical to the training forward."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
WORKER = os.path.join(ROOT, "tests", "infer_shapes_worker.py")

# (N, E, H): the harness' 1 000-crystal and 5 000-crystal (predict.py) batches at H = 5, its 64-crystal batch at 24 and
# 12 neighbours (60 - 120 row tiles of 256), and H = 8 at the 2048-column limit
SHAPES = [(20000, 480000, 5), (1280, 30720, 5), (1280, 15360, 3), (100000, 2400000, 5), (1280, 15360, 5),
          (20000, 480000, 8)]


def _query(N, E, H, Hd=256):
    from cgat_amd import _lib
    plan = _lib.Plan(N, E, 0, 0, 0, 0, 0, 0)
    p = _lib.AttnParams(128, 128, H, Hd, *([0] * 8))
    lib = _lib.lib
    return (lib.cgat_nodes_attention_infer_fused(C.byref(plan), C.byref(p)),
            lib.cgat_nodes_attention_infer_workspace_bytes(C.byref(plan), C.byref(p)),
            lib.cgat_nodes_attention_forward_workspace_bytes(C.byref(plan), C.byref(p)),
            lib.cgat_nodes_attention_saved_floats(N, E, H, Hd))


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


@pytest.mark.parametrize("storage", ["f32", "bf16"])
@pytest.mark.parametrize("mode", ["f16x3c", "bf16x6"])
def test_fused_route_taken_at_harness_shapes(mode, storage):
    """CPU, dry-run queries: in both 24-bit modes the fused route is taken at every shape above, and its workspace is
    a fraction of what the training forward needs (workspace + saved buffer), as in test_fused_inference.py."""
    import cgat_amd  # noqa: F401
    with _mode(mode, storage):
        for N, E, H in SHAPES:
            fused, inf, fwd, saved = _query(N, E, H)
            assert fused == 1, (mode, storage, N, E, H)
            assert inf < 0.25 * (fwd + 4 * saved), (N, E, H, inf, fwd, saved)


def test_fallback_kept_outside_scope():
    """CPU: f16x3, widths other than 128, more than 2048 columns per half or 8 heads, E * H % 4 != 0 and 32-bit gather
    offsets that would overflow keep the training forward's launches (the saved buffer in the workspace)."""
    import cgat_amd  # noqa: F401
    with _mode("f16x3"):
        for N, E, H in SHAPES:
            fused, inf, _, saved = _query(N, E, H)
            assert fused == 0 and inf >= 4 * saved, (N, E, H)
    with _mode("f16x3c"):
        assert _query(1280, 30720, 9)[0] == 0                     # 2304 columns
        assert _query(1280, 30720, 16, Hd=128)[0] == 0            # 16 heads: more than the alpha staging holds
        assert _query(1280, 30721, 5)[0] == 0                     # E * H % 4 != 0
        assert _query(600000, 2400000, 8)[0] == 0                 # N * 4 * 2 H Hd >= 2^32
    from cgat_amd import _lib
    with _mode("f16x3c"):
        plan = _lib.Plan(1280, 30720, 0, 0, 0, 0, 0, 0)
        p = _lib.AttnParams(64, 128, 5, 256, *([0] * 8))          # width 64
        assert _lib.lib.cgat_nodes_attention_infer_fused(C.byref(plan), C.byref(p)) == 0


# ---------------------------------------------------------------------------------------------------------------------
def _ragged_graph(seed, N, hub, n_mid, n_small):
    """E % 4 == 0 (E * H % 4 == 0 at any H), many atoms without incoming edges, segments of 65-256 rows (crossing the
    256-row sub-tiles of edge_msg_wsum), one hub above SEG_LONG = 256, edges in random order."""
    rs = np.random.RandomState(seed)
    deg = np.zeros(N, dtype=np.int64)
    deg[0] = hub
    deg[1:1 + n_mid] = rs.randint(65, 257, size=n_mid)
    deg[1 + n_mid:1 + n_mid + n_small] = rs.randint(0, 25, size=n_small)
    E = int(deg.sum())
    deg[1 + n_mid] += (4 - E % 4) % 4 + (4 if (E + (4 - E % 4) % 4) % 256 == 0 else 0)
    E = int(deg.sum())
    dst = np.repeat(np.arange(N), deg)
    src = rs.randint(0, N, size=E)
    order = rs.permutation(E)
    return N, torch.from_numpy(np.stack([src[order], dst[order]])).long()


def _graph(kind):
    import cgat_amd as P
    if kind == "ragged":                   # >= 128 row tiles of 256
        N, ei = _ragged_graph(41, 5000, 3000, 40, 2359)
        assert ei.shape[1] > 128 * 256
        return N, ei
    if kind == "ragged_few":               # < 128 row tiles: column groups over grid.y
        N, ei = _ragged_graph(43, 2000, 900, 20, 700)
        assert ei.shape[1] < 128 * 256
        return N, ei
    b, _ = P.synthetic_batch(64, 20, {"c64k12": 12, "c64k24": 24}[kind], seed=5)
    return b.num_nodes, b.edge_index


def _inputs(N, ei, seed=6):
    g = torch.Generator().manual_seed(seed)
    E = ei.shape[1]
    return (torch.randn(N, 128, generator=g).to(DEV), ei.to(DEV), torch.randn(E, 128, generator=g).to(DEV),
            torch.randn(N, 128, generator=g).to(DEV))


def _layer(first, H=5):
    import cgat_amd as P
    torch.manual_seed(1)
    return P.GATConvNodes(128, 128, 128, H, concat=True, first=first).to(DEV)


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


def _check_layer_bits(kind, mode, storage="f32", H=5):
    N, ei = _graph(kind)
    x, ei, e, x0 = _inputs(N, ei)
    with _mode(mode, storage):
        for first in (True, False):
            layer = _layer(first, H)
            want = layer(x.clone().requires_grad_(True), ei, e.clone().requires_grad_(True), x0).detach()
            with torch.no_grad():
                got, t = _tags(lambda: layer(x, ei, e, x0))
                route = layer.route(x, ei, e)
            assert t["edge_logits"] > 0 and t["edge_msg_wsum"] > 0 and t["edge_z"] == 0 and t["seg_wsum"] == 0, t
            assert route.kind in ("scalar", "layer_fused") and route.no_grad, route
            assert torch.equal(got, want), (kind, mode, storage, first, float((got - want).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ragged", "ragged_few", "c64k12", "c64k24"])
@pytest.mark.parametrize("mode", ["f16x3c", "bf16x6"])
def test_h5_layer_bit_identical_to_training_forward(kind, mode):
    """H = 5: the fused launches run (and neither the per-edge Z launch nor seg_wsum), with the training forward's
    bits, on ragged graphs (a hub above SEG_LONG, segments crossing sub-tiles, atoms without edges; many and few row
    tiles) and on 64-crystal batches at 12 and 24 neighbours."""
    _check_layer_bits(kind, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ragged", "ragged_few", "c64k24"])
def test_h5_layer_bit_identical_bf16_storage(kind):
    _check_layer_bits(kind, "f16x3c", storage="bf16")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ragged", "ragged_few"])
def test_h8_layer_bit_identical(kind):
    """H = 8 at Hd = 256: 2048 columns per half, the most the route takes."""
    _check_layer_bits(kind, "f16x3c", H=8)


@pytest.mark.gpu
def test_h5_no_grad_peak_below_quarter_of_opt_out():
    """1 000 crystals at 24 neighbours (E = 480 000), H = 5: the peak allocation of one no_grad layer call on the route
    is below a quarter of the opt-out's (the training forward, whose saved buffer holds Z [E, 2 H Hd])."""
    import cgat_amd as P
    b, _ = P.synthetic_batch(1000, 20, 24, seed=5)
    N, ei = b.num_nodes, b.edge_index
    x, ei, e, x0 = _inputs(N, ei)
    layer = _layer(False)
    rise = {}
    try:
        for on in (True, False):
            P.set_fused_inference(on)
            with torch.no_grad():
                layer(x, ei, e, x0)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                _, t = _tags(lambda: layer(x, ei, e, x0))
                rise[on] = torch.cuda.max_memory_allocated() - base
                assert layer.route(x, ei, e).no_grad == on
            assert (t["edge_msg_wsum"] > 0) == on, t
            torch.cuda.empty_cache()
    finally:
        P.set_fused_inference(True)
    assert rise[True] < 0.25 * rise[False], rise


def _harness_net():
    import cgat_amd as P
    torch.manual_seed(1)
    return P.CGAtNet(200, 128, 5, msg_heads=5, neighbor_number=24, vector_attention=False, global_vector_attention=True,
                     mean_pooling=False, rezero=True, update_edges=True).to(DEV).eval()


@pytest.mark.gpu
def test_harness_scalar_network_route_on_equals_off():
    """The harness' scalar-attention network (msg_heads = 5, 24 neighbours) on 64 crystals in eval() under no_grad:
    the route on and the opt-out give the same bits."""
    import cgat_amd as P
    b, roost = P.synthetic_batch(64, 20, 24, seed=7)
    b = b.to(DEV)
    roost = tuple(t.to(DEV) for t in roost)
    net = _harness_net()
    outs = {}
    try:
        for on in (True, False):
            P.set_fused_inference(on)
            with torch.no_grad():
                out, t = _tags(lambda: net(b, roost))
            assert (t["edge_msg_wsum"] > 0) == on, t
            outs[on] = out
    finally:
        P.set_fused_inference(True)
    assert torch.equal(outs[True], outs[False])


def _worker(args, env=None):
    r = subprocess.run([sys.executable, WORKER, *args], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.gpu
def test_harness_scalar_network_captured():
    """The 64-crystal no_grad forward of the harness' scalar network captures into a HIP graph and replays to the eager
    bits (child process: tests/infer_shapes_worker.py)."""
    assert "INFER_SHAPES_CAPTURE_OK" in _worker(["capture"])


@pytest.mark.gpu
def test_no_col_groups_same_bits(tmp_path):
    """CGAT_Z_COL_GROUPS=0 (no grid.y column groups at few row tiles; child process: the switch is read once) gives the
    bits of the default launch on the route, also equal to the training forward there."""
    out = str(tmp_path / "off.pt")
    assert "INFER_SHAPES_LAYER_OK" in _worker(["layer", out], env={"CGAT_Z_COL_GROUPS": "0"})
    off = torch.load(out)
    for kind in ("ragged_few", "c64k24"):
        N, ei = _graph(kind)
        x, ei, e, x0 = _inputs(N, ei)
        layer = _layer(False)
        with torch.no_grad():
            got = layer(x, ei, e, x0)
        assert torch.equal(got.cpu(), off[kind]), kind
