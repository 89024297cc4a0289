"""Shell-indexed edge features on the GPU: ops.nodes_attention_infer_indexed (cgat_nodes_attention_infer_indexed,
csrc/edgeidx.hip) against the dense forward without grad and the oracle, the layer and network surfaces that route to it
(cgat_amd.IndexedEdgeAttr, set_indexed_edge_attr), training under the switch, determinism, capture and errors.

Tolerances, both the project's own:
  flat   max |got - want| <= 1e-4 max |want| against the fp32 oracle (test_fused_inference.py::test_inference_route_vs_oracle)
  ratio  against the oracle evaluated in fp64 on the same inputs, the indexed route's largest error is at most 2 x the
         dense no-grad route's (test_edge_head_combine.py: a fused kernel against the sequence it replaces).  Both routes
         form the same sum of three fp32 terms; only W_e e comes from a different engine.
The oracle runs on the CPU, in fp32 and in fp64; a reference is computed once per set of inputs and shared by the cases
that use them.  Every figure is printed before it is asserted."""
import copy
import os
import subprocess
import sys

import pytest
import torch

from test_fused_inference import DEV, _graph, _inputs, _layer, _mode

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAT, RATIO = 1e-4, 2.0
DENSE_TAGS = ("edge_logits", "edge_msg_wsum", "edge_z", "seg_wsum")
IDX_TAGS = ("edge_idx_logits", "edge_idx_wsum")


def _tags(fn):
    from cgat_amd import ops
    ops.prof_reset()
    ops.prof_enable(True)
    n0 = ops.prof_launches()
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.prof_enable(False)
    t = {k: ops.prof_get(k)[0] for k in DENSE_TAGS + IDX_TAGS}
    t["launches"] = ops.prof_launches() - n0
    return out, t


def _maxerr(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


def _check_both(label, got, dense, want32, want64):
    """The flat bound against the fp32 oracle and the ratio rule against the fp64 one."""
    flat = _maxerr(got, want32) / float(want32.abs().max())
    e_idx, e_dense = _maxerr(got, want64), _maxerr(dense, want64)
    print(f"[indexed] {label}: err/|ref| {flat:.3e}  err64 indexed {e_idx:.3e}  dense {e_dense:.3e}  "
          f"ratio {e_idx / max(e_dense, 1e-300):.3f}")
    assert flat <= FLAT, (label, flat)
    assert e_idx <= RATIO * e_dense, (label, e_idx, e_dense)


_REFS = {}


def _oracle_refs(key, om, *args):
    """(fp32, fp64) outputs of the oracle module `om` on the CPU for CPU inputs `args`; computed once per key."""
    if key not in _REFS:
        with torch.no_grad():
            a64 = [t.double() if torch.is_tensor(t) and t.is_floating_point() else t for t in args]
            _REFS[key] = (om(*args), copy.deepcopy(om).double()(*a64))
    return _REFS[key]


def _index(E, R, seed=11):
    """Shell ids in [0, R) that leave rows unused wherever R allows: only the even rows, and never the last one."""
    g = torch.Generator().manual_seed(seed)
    used = torch.arange(0, max(R - 1, 1), 2)
    return used[torch.randint(0, used.numel(), (E,), generator=g)]


def _graph_any(kind):
    if kind == "c64":                      # N = 1 280: below the small-row limit
        import cgat_amd as P
        b, _ = P.synthetic_batch(64, 20, 12, seed=5)
        return b.num_nodes, b.edge_index
    return _graph(kind)


# ---------------------------------------------------------------------------------------------------------------------
# 2a. the op against the dense no-grad route and fp64
# ---------------------------------------------------------------------------------------------------------------------
OP_CASES = (
    [(k, 3, 13, 128, "f16x3c") for k in ("c150", "ragged", "ragged_odd", "c64")] +
    [("c150", h, 13, 128, "f16x3c") for h in (1, 5, 8)] +
    [("c150", 3, r, 128, "f16x3c") for r in (1, 25, 65)] +
    [("c150", 3, 13, 64, "f16x3c")] +
    [("c150", 3, 13, 128, m) for m in ("bf16x6", "f16x3", "f32")] +
    [("ragged", 3, 25, 128, "f32")])


@pytest.mark.parametrize("kind,H,R,C,mode", OP_CASES, ids=lambda v: str(v))
def test_op_vs_dense_and_fp64(kind, H, R, C, mode):
    """ragged_odd (E * H % 4 != 0) is the case that decided how this route runs fc_out_M: with attn_fwd_out's one K = H * Hd
    launch its error against fp64 was 2.18 x the dense route's (four input seeds: 1.60 - 2.72), because the dense route
    leaves that launch where its own S is misaligned; with one launch per head (K = Hd) it is 0.89 (0.71 - 1.74)."""
    import cgat_amd as P
    from cgat_amd import ops
    from oracle import cgat_oracle as O
    N, ei = _graph_any(kind)
    E = ei.shape[1]
    g = torch.Generator().manual_seed(6)
    x, table, index = torch.randn(N, C, generator=g), torch.randn(R, C, generator=g), _index(E, R)
    torch.manual_seed(1)
    om = O.GATConvNodes(C, C, C, H, concat=True, final=True)
    pm = P.GATConvNodes(C, C, C, H, concat=True, final=True)
    pm.load_state_dict(om.state_dict())
    pm = pm.to(DEV)
    want32, want64 = _oracle_refs((kind, H, R, C), om, x, ei, table[index], None)
    x, table, index, ei = x.to(DEV), table.to(DEV), index.to(DEV), ei.to(DEV)
    dense_e = table[index]
    plan = ops.get_plan(ei, N)
    with _mode(mode), torch.no_grad():
        assert ops.infer_indexed_ok(plan.c, C, C, H, pm.MH_A.hidden_layer_dim, R)
        got, t = _tags(lambda: ops.nodes_attention_infer_indexed(x, (table, index), plan, H, *pm._attn_params()))
        assert t["edge_idx_logits"] > 0 and t["edge_idx_wsum"] > 0 and all(t[k] == 0 for k in DENSE_TAGS), t
        dense = ops.nodes_attention_infer(x, dense_e, plan, H, *pm._attn_params())
        again = ops.nodes_attention_infer_indexed(x, P.IndexedEdgeAttr(table, index), plan, H, *pm._attn_params())
    assert torch.equal(got, again)
    _check_both(f"op {kind} H{H} R{R} C{C} {mode}", got, dense, want32, want64)


# ---------------------------------------------------------------------------------------------------------------------
# 2b. the layer
# ---------------------------------------------------------------------------------------------------------------------
def _layer_case(first):
    import cgat_amd as P
    from oracle import cgat_oracle as O
    N, ei_cpu = _graph("c150")
    x, ei, _, x0 = _inputs(N, ei_cpu)
    table = torch.randn(13, 128, generator=torch.Generator().manual_seed(12)).to(DEV)
    index = _index(ei.shape[1], 13).to(DEV)
    torch.manual_seed(1)
    om = O.GATConvNodes(128, 128, 128, 3, concat=True, first=first)
    pm = P.GATConvNodes(128, 128, 128, 3, concat=True, first=first)
    pm.load_state_dict(om.state_dict())
    refs = lambda: _oracle_refs(("layer", first), om, x.cpu(), ei_cpu, table[index].cpu(), x0.cpu())
    return refs, pm.to(DEV), x, ei, table, index, x0


@pytest.mark.parametrize("first", [True, False])
def test_layer_no_grad_takes_indexed_route(first):
    import cgat_amd as P
    refs, pm, x, ei, table, index, x0 = _layer_case(first)
    with torch.no_grad():
        got, t = _tags(lambda: pm(x, ei, P.IndexedEdgeAttr(table, index), x0))
        assert t["edge_idx_logits"] > 0 and t["edge_idx_wsum"] > 0 and all(t[k] == 0 for k in DENSE_TAGS), t
        route = pm.route(x, ei, P.IndexedEdgeAttr(table, index))
        assert route.indexed and route.no_grad and route.kind in ("scalar", "layer_fused"), route
        dense, t = _tags(lambda: pm(x, ei, table[index], x0))
        assert t["edge_idx_logits"] == 0 and t["edge_idx_wsum"] == 0 and t["edge_msg_wsum"] + t["seg_wsum"] > 0, t
        route = pm.route(x, ei, table[index])
        assert not route.indexed and route.no_grad and route.kind in ("scalar", "layer_fused"), route
    _check_both(f"layer first={first}", got, dense, *refs())


@pytest.mark.parametrize("first", [True, False])
def test_layer_with_grad_densifies_same_bits(first):
    """Grad enabled: the training launches run, and output and table.grad are the bits of a run on
    small_embedding(index, table) passed as a dense tensor -- it is the same code path."""
    import cgat_amd as P
    from cgat_amd import ops
    _, pm, x, ei, table, index, x0 = _layer_case(first)
    cot = torch.randn(x.shape, generator=torch.Generator().manual_seed(13)).to(DEV)
    res = []
    for indexed in (True, False):
        tb = table.clone().requires_grad_(True)
        ea = P.IndexedEdgeAttr(tb, index) if indexed else ops.small_embedding(index, tb)
        y, t = _tags(lambda: pm(x, ei, ea, x0))
        assert t["seg_wsum"] > 0 and t["edge_idx_logits"] == 0 and t["edge_idx_wsum"] == 0, t     # the training forward
        route = pm.route(x, ei, ea)
        assert not route.indexed and not route.no_grad and route.kind in ("scalar", "layer_fused"), route
        (gt,) = torch.autograd.grad((y * cot).sum(), [tb])
        res.append((y.detach(), gt))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].abs().max()) > 0 and float(res[0][1][-1].abs().max()) == 0      # the unused last row


def test_layer_recording_keeps_dense_route():
    import cgat_amd as P
    _, pm, x, ei, table, index, x0 = _layer_case(False)
    with torch.no_grad(), P.debug.record_masks(pm):
        _, t = _tags(lambda: pm(x, ei, P.IndexedEdgeAttr(table, index), x0))
        route = pm.route(x, ei, P.IndexedEdgeAttr(table, index))
    assert t["edge_idx_logits"] == 0 and t["edge_idx_wsum"] == 0 and t["seg_wsum"] > 0, t
    assert not route.indexed and not route.no_grad and route.kind in ("scalar", "layer_fused"), route


def test_edges_layer_accepts_indexed():
    """GATConvEdges: the shipped form returns a lookup over Pooling_NN(table); the hypernetwork form densifies."""
    import cgat_amd as P
    N, ei = _graph_any("c64")
    x, ei, _, x0 = _inputs(N, ei)
    table = torch.randn(13, 128, generator=torch.Generator().manual_seed(12)).to(DEV)
    ea = P.IndexedEdgeAttr(table, _index(ei.shape[1], 13).to(DEV))
    torch.manual_seed(3)
    shipped = P.GATConvEdges(128, 128, 128, 3, concat=True, no_hyper=True).to(DEV)
    hyper = P.GATConvEdges(128, 128, 128, 3, concat=True, no_hyper=False).to(DEV)
    with torch.no_grad():
        out = shipped(x, ei, ea, ea.dense())
        assert isinstance(out, P.IndexedEdgeAttr) and out.index is ea.index
        assert shipped.route(x, ei, ea) == ("rowwise", True, False) and hyper.route(x, ei, ea) == ("fast", False, False)
        assert torch.equal(out.table, shipped.Pooling_NN(table))
        assert _maxerr(out.dense(), shipped(x, ei, ea.dense(), ea.dense())) <= 1e-5 * float(out.table.abs().max())
        got = hyper(x, ei, ea, ea.dense())
        assert torch.is_tensor(got) and torch.equal(got, hyper(x, ei, ea.dense(), ea.dense()))


# ---------------------------------------------------------------------------------------------------------------------
# 2c. allocation
# ---------------------------------------------------------------------------------------------------------------------
def test_op_allocates_only_its_result():
    import cgat_amd as P
    from cgat_amd import ops
    N, ei = _graph("c1000")
    x, ei, _, _ = _inputs(N, ei)
    table = torch.randn(13, 128, generator=torch.Generator().manual_seed(12)).to(DEV)
    ea = P.IndexedEdgeAttr(table, _index(ei.shape[1], 13).to(DEV))
    pm = _layer(False)
    plan = ops.get_plan(ei, N)
    with torch.no_grad():
        ops.nodes_attention_infer_indexed(x, ea, plan, 3, *pm._attn_params())
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = ops.nodes_attention_infer_indexed(x, ea, plan, 3, *pm._attn_params())
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - base
    print(f"[indexed] allocation rise {rise} bytes, result {y.numel() * 4}")
    assert rise <= N * 128 * 4 + (1 << 20), rise


# ---------------------------------------------------------------------------------------------------------------------
# 2d. the network
# ---------------------------------------------------------------------------------------------------------------------
class _switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        import cgat_amd as P
        self.prev = P.get_indexed_edge_attr()
        P.set_indexed_edge_attr(self.on)

    def __exit__(self, *a):
        import cgat_amd as P
        P.set_indexed_edge_attr(self.prev)


def _net_pair(crystals, K=12, seed=7, **kw):
    """(the oracle's references as a function of the call's keywords, product net with the oracle's parameters on the GPU
    in eval mode, batch, roost)."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b_cpu, roost_cpu = P.synthetic_batch(crystals, 20, K, seed=seed)
    n_graph = kw.pop("n_graph", 4)
    torch.manual_seed(1)
    om = O.CGAtNet(200, 128, n_graph, **kw).eval()
    pm = P.CGAtNet(200, 128, n_graph, **kw).eval()
    pm.load_state_dict(om.state_dict())

    key = ("net", crystals, K, seed, n_graph, tuple(sorted(kw.items())))

    def refs(return_graph_embedding=False):
        """(fp32, fp64) of the oracle: one pass each to the graph embedding, the output network on top; shared."""
        if key not in _REFS:
            with torch.no_grad():
                b64 = P.GraphBatch(b_cpu.x.double(), b_cpu.edge_index, b_cpu.edge_attr, b_cpu.batch)
                r64 = tuple(t.double() if t.is_floating_point() else t for t in roost_cpu)
                om64 = copy.deepcopy(om).double()
                e32, e64 = om(b_cpu, roost_cpu, return_graph_embedding=True), om64(b64, r64, return_graph_embedding=True)
                _REFS[key] = {True: (e32, e64), False: (om.output_nn(e32), om64.output_nn(e64))}
        return _REFS[key][bool(return_graph_embedding)]
    return refs, pm.to(DEV), b_cpu.to(DEV), tuple(t.to(DEV) for t in roost_cpu)


def _run(net, b, roost, on, **call):
    with _switch(on), torch.no_grad():
        return _tags(lambda: net(b, roost, **call))


KW3 = dict(msg_heads=3, neighbor_number=12, update_edges=True)


@pytest.mark.parametrize("embedding", [False, True])
def test_network_60_crystals_vs_oracle(embedding):
    """Switch on against the fp32 oracle (flat) and against off by the ratio rule; switch off is the parent's eval forward:
    the bits of set_fused_inference's existing routes."""
    import cgat_amd as P
    refs, pm, b, roost = _net_pair(60, **KW3)
    call = dict(return_graph_embedding=embedding)
    on, t_on = _run(pm, b, roost, True, **call)
    off, t_off = _run(pm, b, roost, False, **call)
    assert t_on["edge_idx_wsum"] > 0 and all(t_on[k] == 0 for k in DENSE_TAGS), t_on
    assert t_off["edge_idx_wsum"] == 0 and t_off["edge_idx_logits"] == 0, t_off
    assert t_off["edge_msg_wsum"] + t_off["seg_wsum"] > 0, t_off          # (fused or not: by arithmetic mode)
    try:
        P.set_fused_inference(False)
        plain, _ = _run(pm, b, roost, False, **call)
    finally:
        P.set_fused_inference(True)
    assert torch.equal(off, plain)
    _check_both(f"net60 embedding={embedding}", on, off, *refs(**call))


@pytest.mark.parametrize("embedding", [False, True])
def test_network_150_crystals_on_vs_off(embedding):
    """Launches per forward, measured on an MI355X in the default mode: 157 on against 160 off (156 / 159 for the
    embedding)."""
    _, pm, b, roost = _net_pair(150, **KW3)
    call = dict(return_graph_embedding=embedding)
    _run(pm, b, roost, True, **call)                       # (plans, workspaces)
    on, t_on = _run(pm, b, roost, True, **call)
    off, t_off = _run(pm, b, roost, False, **call)
    err = _maxerr(on, off) / float(off.abs().max())
    print(f"[indexed] net150 embedding={embedding}: on - off {err:.3e}; launches on {t_on['launches']} off {t_off['launches']}")
    assert err <= FLAT, err
    assert t_on["edge_idx_logits"] > 0 and t_on["edge_idx_wsum"] > 0 and all(t_on[k] == 0 for k in DENSE_TAGS), t_on
    assert t_off["edge_msg_wsum"] + t_off["seg_wsum"] > 0 and t_off["edge_idx_wsum"] == 0, t_off
    assert t_on["launches"] < t_off["launches"], (t_on, t_off)


def test_network_ineligible_takes_the_same_path():
    """no_hyper=False, and one GATConvEdges subclass that overrides forward: the switch changes nothing, bit for bit."""
    import cgat_amd as P
    _, pm, b, roost = _net_pair(24, no_hyper=False, **KW3)
    on, t_on = _run(pm, b, roost, True)
    off, _ = _run(pm, b, roost, False)
    assert t_on["edge_idx_logits"] == 0 and t_on["edge_idx_wsum"] == 0, t_on
    assert torch.equal(on, off)

    class MyEdges(P.GATConvEdges):
        def forward(self, x, edge_index, edge_attr, x_0, size=None):
            return super().forward(x, edge_index, edge_attr, x_0, size)
    _, pm, b, roost = _net_pair(24, **KW3)
    pm.graphs[2]["Edge"].__class__ = MyEdges
    on, t_on = _run(pm, b, roost, True)
    off, _ = _run(pm, b, roost, False)
    assert t_on["edge_idx_logits"] == 0 and t_on["edge_idx_wsum"] == 0, t_on
    assert torch.equal(on, off)


def test_network_harness_default_vs_oracle():
    """The harness' constructor (vector attention: the node layers densify, only the edge update collapses)."""
    kw = dict(rezero=True, mean_pooling=False, neighbor_number=24, msg_heads=5, update_edges=True, vector_attention=True,
              global_vector_attention=True, n_graph=5)
    refs, pm, b, roost = _net_pair(24, K=24, **kw)
    on, t_on = _run(pm, b, roost, True)
    off, t_off = _run(pm, b, roost, False)
    want32, _ = refs()
    flat = _maxerr(on, want32) / float(want32.abs().max())
    print(f"[indexed] harness default: err/|ref| {flat:.3e}; on - off {_maxerr(on, off):.3e}; "
          f"launches on {t_on['launches']} off {t_off['launches']}")
    assert flat <= FLAT, flat
    assert t_on["edge_idx_logits"] == 0, t_on                # vector attention has no indexed node route


# ---------------------------------------------------------------------------------------------------------------------
# 2e. training under the switch
# ---------------------------------------------------------------------------------------------------------------------
def test_training_under_switch_vs_oracle(monkeypatch):
    """The 4-layer network at 60 crystals, train mode, forward and backward with the switch on: every parameter gradient
    -- nbr_embedding.weight's and the Edge.Pooling_NN ones are what the table chain reaches -- through the comparison,
    forced derivative patterns and admission limits of test_hip_golden.py::test_full_stack_vs_oracle_random_init."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    from test_hip_golden import _compare_with_oracle, recipe
    b, roost = P.synthetic_batch(60, 20, 12, seed=8)
    inputs = {"x": b.x, "edge_index": b.edge_index, "edge_attr": b.edge_attr, "batch": b.batch,
              "r0": roost[0], "r1": roost[1], "r2": roost[2], "r3": roost[3], "r4": roost[4]}
    taken = []
    orig = P.CGAtNet._graphs_indexed
    monkeypatch.setattr(P.CGAtNet, "_graphs_indexed", lambda self, *a: (taken.append(1), orig(self, *a))[1])

    def call(m, i):
        bb = recipe.GraphBatch(i["x"], i["edge_index"], i["edge_attr"], i["batch"])
        return m(bb, (t for t in (i["r0"], i["r1"], i["r2"], i["r3"], i["r4"])))
    mk = lambda ns: (lambda: ns.CGAtNet(200, 128, 4, msg_heads=3, neighbor_number=12, update_edges=True))
    with _switch(True):
        _compare_with_oracle(mk(P), mk(O), inputs, call, label="indexed_edge_attr_training")
    assert taken, "the indexed form of the stack was not taken"


# ---------------------------------------------------------------------------------------------------------------------
# 2f. determinism and capture
# ---------------------------------------------------------------------------------------------------------------------
def test_indexed_deterministic_and_captured():
    """Two eval calls with the switch on give the same bits (ragged graph: the hub's fixed split included); a
    torch.cuda.graph capture of the eval forward replays to the eager bits (child process:
    tests/indexed_capture_worker.py, as test_inference_deterministic_and_captured does)."""
    import cgat_amd as P
    from cgat_amd import ops
    N, ei = _graph("ragged")
    x, ei, _, x0 = _inputs(N, ei)
    table = torch.randn(13, 128, generator=torch.Generator().manual_seed(12)).to(DEV)
    ea = P.IndexedEdgeAttr(table, _index(ei.shape[1], 13).to(DEV))
    layer = _layer(False)
    with torch.no_grad():
        y1, t = _tags(lambda: layer(x, ei, ea, x0))
        y2 = layer(x, ei, ea, x0)
        assert layer.route(x, ei, ea).indexed and layer.route(x, ei, ea).no_grad
    assert t["edge_idx_wsum"] > 0, t
    assert torch.equal(y1, y2)
    _, pm, b, roost = _net_pair(60, **KW3)
    n1, _ = _run(pm, b, roost, True)
    n2, _ = _run(pm, b, roost, True)
    assert torch.equal(n1, n2)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "indexed_capture_worker.py")], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "INDEXED_CAPTURE_OK" in r.stdout, r.stdout[-2000:]


# ---------------------------------------------------------------------------------------------------------------------
# 2g. errors: raised in Python, before any launch
# ---------------------------------------------------------------------------------------------------------------------
def test_errors_before_any_launch():
    import cgat_amd as P
    from cgat_amd import ops
    N, ei = _graph_any("c64")
    x, ei, _, _ = _inputs(N, ei)
    E = ei.shape[1]
    table = torch.randn(13, 128, generator=torch.Generator().manual_seed(12)).to(DEV)
    index = _index(E, 13).to(DEV)
    pm = _layer(False)
    plan = ops.get_plan(ei, N)
    params = pm._attn_params()
    torch.cuda.synchronize()
    n0 = ops.prof_launches()
    bad = index.clone()
    bad[5] = 13
    with pytest.raises(IndexError):
        P.IndexedEdgeAttr(table, bad)
    neg = index.clone()
    neg[7] = -1
    with pytest.raises(IndexError):
        P.IndexedEdgeAttr(table, neg)
    with pytest.raises(TypeError):
        P.IndexedEdgeAttr(table, index.int())
    with pytest.raises(TypeError):
        P.IndexedEdgeAttr(table.double(), index)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.IndexedEdgeAttr(table.cpu(), index)
    with pytest.raises(ValueError):
        ops.nodes_attention_infer_indexed(x, P.IndexedEdgeAttr(table, index[:-1].clone()), plan, 3, *params)
    with pytest.raises(TypeError):
        ops.nodes_attention_infer_indexed(x, (table, index.int()), plan, 3, *params)
    assert ops.prof_launches() == n0
