"""The training route of shell-indexed edge features on the GPU (cgat_amd.set_indexed_edge_training;
ops.NodesAttentionIndexedFn / NodeLayerIndexedFn; cgat_nodes_attention_forward_indexed / _backward_indexed,
csrc/edgeidx.hip): gradients against the oracle, forward bits, the ratio rule against the dense training route, saved
memory, determinism and locality, the whole-layer node and the network, ineligible shapes, capture and errors.

Tolerances, both the project's own (tests/test_indexed_edge_attr.py):
  flat   1e-4 of the largest reference entry per tensor, through test_hip_golden.py::_compare_with_oracle with the
         route's own derivative pattern forced on the oracle
  ratio  against the oracle in fp64 forced to the pattern each run recorded, the indexed route's largest error is at most
         2 x the dense training route's
Every figure is printed before it is asserted."""
import copy
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from test_fused_inference import DEV, _graph, _inputs, _mode
from test_indexed_edge_attr import FLAT, OP_CASES, RATIO, _graph_any, _index, _maxerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_TAGS = ("edge_idx_bwd_msg", "edge_idx_bwd_att", "edge_idx_class_sum")
KEPT_TAGS = ("edge_idx_logits", "edge_idx_wsum", "edge_gj")
GONE_TAGS = ("edge_z", "seg_wsum", "edge_seg_bwd", "edge_ge", "edge_gw")


def _tags(fn):
    """test_indexed_edge_attr.py::_tags over this file's tags."""
    from cgat_amd import ops
    ops.prof_reset()
    ops.prof_enable(True)
    n0 = ops.prof_launches()
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.prof_enable(False)
    t = {k: ops.prof_get(k)[0] for k in NEW_TAGS + KEPT_TAGS + GONE_TAGS}
    t["launches"] = ops.prof_launches() - n0
    return out, t


def _assert_indexed_tags(t, route=None):
    """`route`: layer.route(...) of the call the tags were counted over (_step.route); it names the same route."""
    assert all(t[k] > 0 for k in NEW_TAGS + KEPT_TAGS), t
    assert all(t[k] == 0 for k in GONE_TAGS), t
    assert route is None or (route.indexed and not route.no_grad and route.kind in ("scalar", "layer_fused")), route


def _assert_dense_tags(t, route=None):
    assert all(t[k] == 0 for k in NEW_TAGS + ("edge_idx_logits", "edge_idx_wsum")), t
    assert route is None or not route.indexed, route


class _train:
    """set_indexed_edge_training (and, for networks, set_indexed_edge_attr) for a block, restored afterwards."""

    def __init__(self, on, attr=None):
        self.on, self.attr = on, attr

    def __enter__(self):
        import cgat_amd as P
        self.prev = (P.get_indexed_edge_training(), P.get_indexed_edge_attr())
        P.set_indexed_edge_training(self.on)
        if self.attr is not None:
            P.set_indexed_edge_attr(self.attr)

    def __exit__(self, *a):
        import cgat_amd as P
        P.set_indexed_edge_training(self.prev[0])
        P.set_indexed_edge_attr(self.prev[1])


def _final_layer(C_, H, om=None):
    import cgat_amd as P
    from oracle import cgat_oracle as O
    torch.manual_seed(1)
    om = om or O.GATConvNodes(C_, C_, C_, H, concat=True, final=True)
    pm = P.GATConvNodes(C_, C_, C_, H, concat=True, final=True)
    pm.load_state_dict(om.state_dict())
    return om, pm.to(DEV)


def _case_inputs(kind, R, C_):
    N, ei = _graph_any(kind)
    g = torch.Generator().manual_seed(6)
    x, table = torch.randn(N, C_, generator=g), torch.randn(R, C_, generator=g)
    return N, ei, x, table, _index(ei.shape[1], R)


GRAD_NAMES = ("x", "table", "MH_A.fc_in.weight", "MH_A.fc_in.bias", "MH_A.fc_out.weight", "MH_A.fc_out.bias",
              "MH_M.fc_in.weight", "MH_M.fc_in.bias", "MH_M.fc_out.weight", "MH_M.fc_out.bias")


def _step(pm, x, ei, table, index, cot, indexed=True, x0=None):
    """One forward + backward of a layer: (output, {name: gradient}) for x, table and the layer's parameters."""
    import cgat_amd as P
    from cgat_amd import ops
    xg, tg = x.clone().requires_grad_(True), table.clone().requires_grad_(True)
    ea = P.IndexedEdgeAttr(tg, index) if indexed else ops.small_embedding(index, tg)
    _step.route = pm.route(xg, ei, ea)                # (what the call below takes: asserted beside its launch tags)
    y = pm(xg, ei, ea, x0)
    names = [n for n, _ in pm.named_parameters()]
    gs = torch.autograd.grad((y * cot).sum(), [xg, tg] + list(pm.parameters()), allow_unused=True)
    return y.detach(), dict(zip(["x", "table"] + names, gs))


# ---------------------------------------------------------------------------------------------------------------------
# 1. layer gradients against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,H,R,C_,mode", OP_CASES, ids=lambda v: str(v))
def test_layer_gradients_vs_oracle(kind, H, R, C_, mode):
    """This is the test that fails without the route: the switch does not exist, and with grad the layer runs edge_z and
    edge_gw."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    from test_hip_golden import _compare_with_oracle
    N, ei, x, table, index = _case_inputs(kind, R, C_)
    inputs = {"x": x, "edge_index": ei, "table": table, "index": index}

    def call(m, i):
        if isinstance(m, P.GATConvNodes):
            return m(i["x"], i["edge_index"], P.IndexedEdgeAttr(i["table"], i["index"]), None)
        # table[index] through F.embedding: the same rows, and a CPU backward that does not serialise on R = 1
        return m(i["x"], i["edge_index"], torch.nn.functional.embedding(i["index"], i["table"]), None)
    mk = lambda ns: (lambda: ns.GATConvNodes(C_, C_, C_, H, concat=True, final=True))
    with _mode(mode), _train(True):
        worst = _compare_with_oracle(mk(P), mk(O), inputs, call, tol=FLAT, label=f"indexed_train {kind} H{H} R{R} C{C_} {mode}")
        _, pm = _final_layer(C_, H)
        cot = torch.randn(N, C_, generator=torch.Generator().manual_seed(9)).to(DEV)
        (y, g), t = _tags(lambda: _step(pm, x.to(DEV), ei.to(DEV), table.to(DEV), index.to(DEV), cot))
    print(f"[indexed-train] layer {kind} H{H} R{R} C{C_} {mode}: worst err/|ref| {worst:.3e}; tags {t}")
    _assert_indexed_tags(t, _step.route)
    gt = g["table"]
    used = torch.zeros(R, dtype=torch.bool)
    used[index.unique()] = True
    row_max = gt.abs().amax(dim=1).cpu()
    print(f"[indexed-train]   table.grad row maxima: used min {float(row_max[used].min()):.3e}, unused max "
          f"{float(row_max[~used].max()) if (~used).any() else 0.0:.3e}")
    assert bool((row_max[~used] == 0).all()) and bool((row_max[used] > 0).all())
    assert all(torch.isfinite(v).all() for v in g.values())


# ---------------------------------------------------------------------------------------------------------------------
# 2. forward bits: the training forward is the forward without grad
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c150", "ragged"])
@pytest.mark.parametrize("first", [True, False])
def test_forward_bits_equal_no_grad(kind, first):
    import cgat_amd as P
    from test_fused_inference import _layer
    N, ei = _graph(kind)
    x, ei, _, x0 = _inputs(N, ei)
    table = torch.randn(13, 128, generator=torch.Generator().manual_seed(12)).to(DEV)
    index = _index(ei.shape[1], 13).to(DEV)
    pm = _layer(first)
    with _train(True):
        y, t = _tags(lambda: pm(x, ei, P.IndexedEdgeAttr(table.clone().requires_grad_(True), index), x0))
        assert y.requires_grad and t["edge_idx_logits"] > 0 and t["edge_idx_wsum"] > 0 and t["seg_wsum"] == 0, t
        route = pm.route(x, ei, P.IndexedEdgeAttr(table.clone().requires_grad_(True), index))
        assert route.indexed and not route.no_grad and route.kind in ("scalar", "layer_fused"), route
        with torch.no_grad():
            y0, t0 = _tags(lambda: pm(x, ei, P.IndexedEdgeAttr(table, index), x0))
            route = pm.route(x, ei, P.IndexedEdgeAttr(table, index))
        assert t0["edge_idx_wsum"] > 0, t0
        assert route.indexed and route.no_grad, route
    assert torch.equal(y.detach(), y0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the ratio rule against the dense training route
# ---------------------------------------------------------------------------------------------------------------------
RATIO_TENSORS = ("table", "MH_A.fc_in.weight", "MH_M.fc_in.weight", "MH_A.fc_out.weight", "x")


@pytest.mark.parametrize("kind,H", [("c150", 3), ("c150", 5), ("ragged", 3), ("ragged", 5)])
def test_ratio_rule_vs_dense_training(kind, H):
    """Recorded on an MI355X in f16x3c (tests/golden/indexed_train_error.json keeps the ratios of that run)."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    N, ei_cpu, x_cpu, table_cpu, index_cpu = _case_inputs(kind, 13, 128)
    om, pm = _final_layer(128, H)
    om64 = copy.deepcopy(om).double()
    x, ei, table, index = x_cpu.to(DEV), ei_cpu.to(DEV), table_cpu.to(DEV), index_cpu.to(DEV)
    cot_cpu = torch.randn(N, 128, generator=torch.Generator().manual_seed(9))
    cot = cot_cpu.to(DEV)

    def err64(indexed):
        rec = P.debug.record_masks(pm)
        with _train(indexed), rec as masks:
            (_, g), t = _tags(lambda: _step(pm, x, ei, table, index, cot, indexed=indexed))
        (_assert_indexed_tags if indexed else _assert_dense_tags)(t, _step.route)
        xr, tr = x_cpu.double().requires_grad_(True), table_cpu.double().requires_grad_(True)
        with O.forced_masks(om64, masks):
            y = om64(xr, ei_cpu, torch.nn.functional.embedding(index_cpu, tr), None)
            names = [n for n, _ in om64.named_parameters()]
            ref = dict(zip(["x", "table"] + names,
                           torch.autograd.grad((y * cot_cpu.double()).sum(), [xr, tr] + list(om64.parameters()))))
        return {k: _maxerr(g[k], ref[k]) for k in RATIO_TENSORS}
    e_idx, e_dense = err64(True), err64(False)
    for k in RATIO_TENSORS:
        print(f"[indexed-train] ratio {kind} H{H} grad {k}: err64 indexed {e_idx[k]:.3e} dense {e_dense[k]:.3e} "
              f"ratio {e_idx[k] / max(e_dense[k], 1e-300):.3f}")
    for k in RATIO_TENSORS:
        assert e_idx[k] <= RATIO * e_dense[k], (k, e_idx[k], e_dense[k])


# ---------------------------------------------------------------------------------------------------------------------
# 4. saved memory
# ---------------------------------------------------------------------------------------------------------------------
def test_saved_memory():
    """1 000 crystals (N = 20 000, E = 240 000), H = 3: what a layer's forward leaves allocated for its backward is its
    output, alpha and ssum (S is formed again in the backward): 13 MB, inside the stated bound of 75.8 MB and below 3 % of
    the 1.47 GB that Z alone would take.  Both are asserted."""
    import cgat_amd as P
    N, ei = _graph("c1000")
    x, ei, _, _ = _inputs(N, ei)
    E, H, Hd, C_ = ei.shape[1], 3, 256, 128
    table = torch.randn(13, 128, generator=torch.Generator().manual_seed(12)).to(DEV).requires_grad_(True)
    index = _index(E, 13).to(DEV)
    _, pm = _final_layer(128, 3)
    with _train(True):
        pm(x, ei, P.IndexedEdgeAttr(table, index), None).sum().backward()      # warm-up: plans, workspaces
        table.grad = None
        pm.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        y = pm(x, ei, P.IndexedEdgeAttr(table, index), None)
        torch.cuda.synchronize()
        rise = torch.cuda.memory_allocated() - base
        bound = 4 * (N * C_ + E * H + N * H * Hd + N * H) + (1 << 20)
        z_bytes = E * 2 * H * Hd * 4
        print(f"[indexed-train] forward keeps {rise} bytes (bound {bound}); Z alone would take {z_bytes}: {rise / z_bytes:.4f}")
        assert rise <= bound, (rise, bound)
        assert rise < 0.03 * z_bytes, (rise, z_bytes)
        y.sum().backward()
        torch.cuda.synchronize()
    grads = [table.grad] + [p.grad for p in pm.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)


# ---------------------------------------------------------------------------------------------------------------------
# 5. determinism and locality
# ---------------------------------------------------------------------------------------------------------------------
def test_deterministic_on_ragged():
    N, ei, x, table, index = _case_inputs("ragged", 13, 128)
    _, pm = _final_layer(128, 3)
    x, ei, table, index = x.to(DEV), ei.to(DEV), table.to(DEV), index.to(DEV)
    cot = torch.randn(N, 128, generator=torch.Generator().manual_seed(9)).to(DEV)
    with _train(True):
        (y1, g1), t = _tags(lambda: _step(pm, x, ei, table, index, cot))
        y2, g2 = _step(pm, x, ei, table, index, cot)
    _assert_indexed_tags(t, _step.route)
    assert torch.equal(y1, y2)
    for k in GRAD_NAMES:
        assert torch.equal(g1[k], g2[k]), k


def test_two_disjoint_copies_locality():
    """c150 twice as disjoint copies in one batch: the first copy's grad x rows are the bits of the single-copy run (the
    segment kernels see nothing of another segment; test_million_edge_stack_fwd_bwd_locality at a small size)."""
    N, ei, x, table, index = _case_inputs("c150", 13, 128)
    _, pm = _final_layer(128, 3)
    cot = torch.randn(N, 128, generator=torch.Generator().manual_seed(9))
    ei2, x2 = torch.cat([ei, ei + N], dim=1), torch.cat([x, x.flip(0)])
    idx2, cot2 = torch.cat([index, index.flip(0)]), torch.cat([cot, cot.flip(0)])
    with _train(True):
        y1, g1 = _step(pm, x.to(DEV), ei.to(DEV), table.to(DEV), index.to(DEV), cot.to(DEV))
        (y2, g2), t = _tags(lambda: _step(pm, x2.to(DEV), ei2.to(DEV), table.to(DEV), idx2.to(DEV), cot2.to(DEV)))
    _assert_indexed_tags(t, _step.route)
    assert torch.equal(y2[:N], y1)
    assert torch.equal(g2["x"][:N], g1["x"])


# ---------------------------------------------------------------------------------------------------------------------
# 6. the whole-layer node and the network
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [True, False])
def test_whole_layer_node_equals_separate_nodes(first):
    """NodeLayerIndexedFn (ops.overlap_enabled(): the hypernetwork's weight-gradient contractions on the side stream
    where that keeps the bits, ops._overlapped_hnet_keeps_bits) against NodesAttentionIndexedFn + HNetFn: same bits, every
    gradient, in every arithmetic mode."""
    from cgat_amd import ops
    from test_fused_inference import _layer
    N, ei = _graph("c150")
    x, ei, _, x0 = _inputs(N, ei)
    table = torch.randn(13, 128, generator=torch.Generator().manual_seed(12)).to(DEV)
    index = _index(ei.shape[1], 13).to(DEV)
    pm = _layer(first)
    cot = torch.randn(N, 128, generator=torch.Generator().manual_seed(13)).to(DEV)
    prev = ops.get_overlap_wgrad()
    res = []
    try:
        with _train(True):
            for overlap in (True, False):
                ops.set_overlap_wgrad(overlap)
                (y, g), t = _tags(lambda: _step(pm, x, ei, table, index, cot, x0=x0))
                _assert_indexed_tags(t, _step.route)
                res.append((y, g))
    finally:
        ops.set_overlap_wgrad(prev)
    for k, v in res[0][1].items():
        if v is not None and not torch.equal(v, res[1][1][k]):
            print(f"[indexed-train] whole layer first={first}: {k} differs by {_maxerr(v, res[1][1][k]):.3e} "
                  f"of {float(v.abs().max()):.3e}")
    assert torch.equal(res[0][0], res[1][0])
    for k, v in res[0][1].items():
        w = res[1][1][k]
        assert (v is None and w is None) or torch.equal(v, w), k


def _net_inputs():
    import cgat_amd as P
    b, roost = P.synthetic_batch(60, 20, 12, seed=8)
    return {"x": b.x, "edge_index": b.edge_index, "edge_attr": b.edge_attr, "batch": b.batch,
            "r0": roost[0], "r1": roost[1], "r2": roost[2], "r3": roost[3], "r4": roost[4]}


def _net_call(m, i):
    from test_hip_golden import recipe
    bb = recipe.GraphBatch(i["x"], i["edge_index"], i["edge_attr"], i["batch"])
    return m(bb, (t for t in (i["r0"], i["r1"], i["r2"], i["r3"], i["r4"])))


def test_network_training_vs_oracle(monkeypatch):
    """The 4-layer network at 60 crystals in train mode, both switches on: construction and call of
    test_indexed_edge_attr.py::test_training_under_switch_vs_oracle."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    from test_hip_golden import _compare_with_oracle
    taken = []
    orig = P.CGAtNet._graphs_indexed
    monkeypatch.setattr(P.CGAtNet, "_graphs_indexed", lambda self, *a: (taken.append(1), orig(self, *a))[1])
    mk = lambda ns: (lambda: ns.CGAtNet(200, 128, 4, msg_heads=3, neighbor_number=12, update_edges=True))
    with _train(True, attr=True):
        _, t = _tags(lambda: _compare_with_oracle(mk(P), mk(O), _net_inputs(), _net_call, label="indexed_edge_training_net"))
    print(f"[indexed-train] net60 tags {t}")
    assert taken, "the indexed form of the stack was not taken"
    assert all(t[k] > 0 for k in NEW_TAGS) and t["edge_z"] == 0 and t["edge_ge"] == 0 and t["edge_gw"] == 0, t


def test_network_training_switch_alone_changes_nothing():
    """set_indexed_edge_training(True) without set_indexed_edge_attr: no IndexedEdgeAttr reaches a layer -- outputs and
    gradients are the bits of both switches off."""
    import cgat_amd as P
    torch.manual_seed(1)
    net = P.CGAtNet(200, 128, 4, msg_heads=3, neighbor_number=12, update_edges=True).to(DEV).train()
    ins = {k: v.to(DEV) for k, v in _net_inputs().items()}
    res = []
    for on in (True, False):
        with _train(on, attr=False):
            net.zero_grad(set_to_none=True)
            y, t = _tags(lambda: _net_call(net, ins))
            y.square().sum().backward()
            torch.cuda.synchronize()
        _assert_dense_tags(t)
        res.append((y.detach(), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}))
    assert torch.equal(res[0][0], res[1][0]) and res[0][1].keys() == res[1][1].keys()
    for k, v in res[0][1].items():
        assert torch.equal(v, res[1][1][k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 7. ineligible shapes keep their path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["vector", "dropout", "bf16"])
def test_ineligible_keeps_dense_training_path(what):
    import cgat_amd as P
    N, ei = _graph("c150")
    x, ei, _, x0 = _inputs(N, ei)
    table = torch.randn(13, 128, generator=torch.Generator().manual_seed(12)).to(DEV)
    index = _index(ei.shape[1], 13).to(DEV)
    torch.manual_seed(1)
    pm = P.GATConvNodes(128, 128, 128, 3, concat=True, final=True, vector_attention=what == "vector",
                        dropout=0.1 if what == "dropout" else 0).to(DEV).train()
    cot = torch.randn(N, 128, generator=torch.Generator().manual_seed(13)).to(DEV)
    res = []
    with _mode("f16x3c", "bf16" if what == "bf16" else "f32"):
        for on in (True, False):
            with _train(on):
                (y, g), t = _tags(lambda: _step(pm, x, ei, table, index, cot))
            print(f"[indexed-train] ineligible {what} switch {on}: {t}")
            _assert_dense_tags(t, _step.route)
            # the dense training launches of each route: the per-edge forward, the segment sums, both per-edge products
            assert t["edge_z"] > 0 and t["seg_wsum"] > 0 and t["edge_ge"] > 0 and t["edge_gw"] > 0, t
            if what == "bf16":
                assert t["edge_seg_bwd"] > 0 and t["edge_gj"] > 0, t        # scalar attention: its segment backward
            res.append((y, g))
    if what != "dropout":                                                     # (the dropout case: tags only)
        assert torch.equal(res[0][0], res[1][0])
        for k, v in res[0][1].items():
            w = res[1][1][k]
            assert (v is None and w is None) or torch.equal(v, w), k


# ---------------------------------------------------------------------------------------------------------------------
# 8. capture
# ---------------------------------------------------------------------------------------------------------------------
def test_captured_step_replays_to_eager_bits():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "indexed_train_capture_worker.py")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "INDEXED_TRAIN_CAPTURE_OK" in r.stdout, r.stdout[-2000:]


# ---------------------------------------------------------------------------------------------------------------------
# 9. errors: raised in Python, before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_before_any_launch():
    import cgat_amd as P
    from cgat_amd import _lib, ops
    from test_fused_inference import _layer
    N, ei = _graph_any("c64")
    x, ei, _, _ = _inputs(N, ei)
    E = ei.shape[1]
    table = torch.randn(13, 128, generator=torch.Generator().manual_seed(12)).to(DEV).requires_grad_(True)
    index = _index(E, 13).to(DEV)
    pm = _layer(False)
    plan = ops.get_plan(ei, N)
    params = pm._attn_params()
    torch.cuda.synchronize()
    n0 = ops.prof_launches()
    fn = ops.NodesAttentionIndexedFn.apply
    with pytest.raises(ValueError):
        fn(x, table, index[:-1].clone(), plan, 3, *params)
    with pytest.raises(TypeError):
        fn(x, table, index.int(), plan, 3, *params)
    strided = torch.stack([index, index], dim=1)[:, 0]
    with pytest.raises(ValueError, match="contiguous"):
        fn(x, table, strided, plan, 3, *params)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(x, table.detach().cpu().requires_grad_(True), index, plan, 3, *params)
    # the C entry where the predicate says 0 (R = 257): CGAT_ERR_UNSUPPORTED, nothing launched
    ws_ = [w.detach() for w in params]
    p = _lib.AttnParams(128, 128, 3, ws_[0].shape[0] // 3, *[w.data_ptr() for w in ws_])
    assert not ops.train_indexed_ok(plan.c, 128, 128, 3, ws_[0].shape[0] // 3, 257)
    buf = torch.empty(1 << 20, dtype=torch.float32, device=DEV)
    vp = lambda t: C.c_void_p(t.data_ptr())
    rc = _lib.lib.cgat_nodes_attention_forward_indexed(C.byref(plan.c), C.byref(p), vp(x), vp(table), 257, vp(index), vp(buf),
                                                       vp(buf), vp(buf), buf.numel() * 4, None)
    assert rc == 4, (rc, _lib.lib.cgat_last_error())       # CGAT_ERR_UNSUPPORTED
    assert ops.prof_launches() == n0
