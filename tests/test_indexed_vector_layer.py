"""Vector-attention node layers on shell-indexed edge features (cgat_amd.set_indexed_vector_attention;
ops.EdgeHiddenIndexedFn / EdgeHiddenHeadsIndexedFn; cgat_edge_hidden_forward_indexed / _backward_indexed, csrc/edgeidx.hip):
the layer and the harness-default network against the oracle, the switch off against the parent route bit for bit, saved
state, determinism, ineligible calls, capture.

Tolerances, both the project's own (tests/test_indexed_edge_attr.py):
  flat   1e-4 of the largest reference entry per tensor, through test_hip_golden.py::_compare_with_oracle with the route's
         own derivative pattern forced on the oracle (the network in training: that function's default admission limits,
         as test_hip_golden.py::test_lightning_default_stack_vs_oracle)
  ratio  the eval forward's error against the fp64 oracle is at most 2 x that of the same forward with the switch off
Every figure is printed before it is asserted."""
import os
import subprocess
import sys

import pytest
import torch

from test_fused_inference import DEV, _graph, _inputs, _mode
from test_indexed_edge_attr import FLAT, _check_both, _graph_any, _index, _maxerr, _net_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_TAGS = ("edge_idx_hidden", "edge_idx_class_sum")
# the per-edge launches of the dense first layer: the K = Ce forward product ("edge_z": csrc/edgez.hip tags the per-edge
# launch "edge_z" and the per-node projections, which stay, "edge_proj") and the two per-edge products of its backward
GONE_TAGS = ("edge_z", "edge_ge", "edge_gw")


def _tags(fn):
    from cgat_amd import ops
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.prof_enable(False)
    return out, {k: ops.prof_get(k)[0] for k in NEW_TAGS + GONE_TAGS}


def _assert_indexed_tags(t, backward=True, route=None):
    """`route`: layer.route(...) of the call the tags were counted over (_step.route); it names the same route."""
    assert t["edge_idx_hidden"] > 0 and (t["edge_idx_class_sum"] > 0 or not backward), t
    assert all(t[k] == 0 for k in GONE_TAGS), t
    assert route is None or route == ("vector", True, False), route


def _assert_dense_tags(t, route=None):
    assert all(t[k] == 0 for k in NEW_TAGS), t
    assert route is None or not route.indexed, route


class _vec:
    """set_indexed_vector_attention (and, for networks, set_indexed_edge_attr) for a block, restored afterwards."""

    def __init__(self, on, attr=None):
        self.on, self.attr = on, attr

    def __enter__(self):
        import cgat_amd as P
        self.prev = (P.get_indexed_vector_attention(), P.get_indexed_edge_attr())
        P.set_indexed_vector_attention(self.on)
        if self.attr is not None:
            P.set_indexed_edge_attr(self.attr)

    def __exit__(self, *a):
        import cgat_amd as P
        P.set_indexed_vector_attention(self.prev[0])
        P.set_indexed_edge_attr(self.prev[1])


def _vector_layer(H=3, cls=None, **kw):
    import cgat_amd as P
    torch.manual_seed(1)
    kw.setdefault("final", True)
    return (cls or P.GATConvNodes)(128, 128, 128, H, concat=True, vector_attention=True, **kw).to(DEV)


def _case(kind, R=13):
    N, ei = _graph_any(kind)
    g = torch.Generator().manual_seed(6)
    x, table = torch.randn(N, 128, generator=g), torch.randn(R, 128, generator=g)
    cot = torch.randn(N, 128, generator=torch.Generator().manual_seed(9))
    return N, ei, x, table, _index(ei.shape[1], R), cot


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


def _assert_same(a, b):
    assert torch.equal(a[0], b[0])
    assert a[1].keys() == b[1].keys()
    for k, v in a[1].items():
        w = b[1][k]
        assert (v is None and w is None) or torch.equal(v, w), k


def _layer_call(m, i):
    import cgat_amd as P
    if isinstance(m, P.GATConvNodes):
        return m(i["x"], i["edge_index"], P.IndexedEdgeAttr(i["table"], i["index"]), i.get("x_0"))
    return m(i["x"], i["edge_index"], torch.nn.functional.embedding(i["index"], i["table"]), i.get("x_0"))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the layer against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [1, 3, 5])
@pytest.mark.parametrize("kind", ["c150", "ragged", "c64"])
def test_layer_vs_oracle(kind, H):
    """This is the test that fails without the route: the switch does not exist, and the layer runs edge_z, edge_ge and
    edge_gw.  Output and the gradients of x, table and all eight parameters at flat 1e-4."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    from test_hip_golden import _compare_with_oracle
    N, ei, x, table, index, cot = _case(kind)
    inputs = {"x": x, "edge_index": ei, "table": table, "index": index}
    mk = lambda ns: (lambda: ns.GATConvNodes(128, 128, 128, H, concat=True, final=True, vector_attention=True))
    with _vec(True):
        worst = _compare_with_oracle(mk(P), mk(O), inputs, _layer_call, tol=FLAT, label=f"indexed_vector {kind} H{H}")
        pm = _vector_layer(H)
        (y, g), t = _tags(lambda: _step(pm, x.to(DEV), ei.to(DEV), table.to(DEV), index.to(DEV), cot.to(DEV)))
    print(f"[indexed-vector] layer {kind} H{H}: worst err/|ref| {worst:.3e}; tags {t}")
    _assert_indexed_tags(t, route=_step.route)
    assert len([k for k in g if k not in ("x", "table")]) == 8 and all(v is not None for v in g.values())
    used = torch.zeros(13, dtype=torch.bool)
    used[index.unique()] = True
    row_max = g["table"].abs().amax(dim=1).cpu()
    print(f"[indexed-vector]   table.grad row maxima: used min {float(row_max[used].min()):.3e}, unused max "
          f"{float(row_max[~used].max()):.3e}")
    assert bool((row_max[~used] == 0).all()) and bool((row_max[used] > 0).all())


@pytest.mark.parametrize("first", [True, False])
def test_first_and_non_first_layer_vs_oracle(first):
    """With the hypernetwork update (H_Net_0 / H_Net) behind the aggregation, c150."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    from test_hip_golden import _compare_with_oracle
    N, ei, x, table, index, _ = _case("c150")
    inputs = {"x": x, "edge_index": ei, "table": table, "index": index,
              "x_0": torch.randn(N, 128, generator=torch.Generator().manual_seed(14))}
    mk = lambda ns: (lambda: ns.GATConvNodes(128, 128, 128, 3, concat=True, first=first, vector_attention=True))
    with _vec(True):
        (worst, t) = _tags(lambda: _compare_with_oracle(mk(P), mk(O), inputs, _layer_call, tol=FLAT,
                                                        label=f"indexed_vector first={first}"))
    print(f"[indexed-vector] layer first={first}: worst err/|ref| {worst:.3e}; tags {t}")
    _assert_indexed_tags(t)


# ---------------------------------------------------------------------------------------------------------------------
# 2. switch off: the parent route, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [3, 5])
def test_switch_off_is_the_parent_route(H):
    N, ei, x, table, index, cot = (v.to(DEV) if torch.is_tensor(v) else v for v in _case("c150"))
    pm = _vector_layer(H)
    with _vec(False):
        off, t = _tags(lambda: _step(pm, x, ei, table, index, cot))
        parent, t2 = _tags(lambda: _step(pm, x, ei, table, index, cot, indexed=False))
    print(f"[indexed-vector] switch off H{H}: {t}; parent {t2}")
    _assert_dense_tags(t)
    _assert_dense_tags(t2, _step.route)
    assert t["edge_z"] > 0 and t["edge_ge"] > 0 and t["edge_gw"] > 0, t
    _assert_same(off, parent)


# ---------------------------------------------------------------------------------------------------------------------
# 3. saved state, determinism
# ---------------------------------------------------------------------------------------------------------------------
def test_no_saved_tensor_of_edge_feature_size():
    """Under saved_tensors_hooks: with the switch on nothing the layer step saves has E * Ce elements; with it off one
    does (the dense edge features)."""
    N, ei, x, table, index, cot = (v.to(DEV) if torch.is_tensor(v) else v for v in _case("c150"))
    E, Ce = ei.shape[1], 128
    pm = _vector_layer(5)
    sizes = {}
    for on in (True, False):
        seen = sizes[on] = []
        with _vec(on), torch.autograd.graph.saved_tensors_hooks(lambda v: (seen.append(v.numel()), v)[1], lambda v: v):
            _step(pm, x, ei, table, index, cot)
    print(f"[indexed-vector] saved tensors: on {sorted(set(sizes[True]))}; off {sorted(set(sizes[False]))}; E * Ce = {E * Ce}")
    assert E * Ce not in sizes[True] and E * 2 * 5 * 256 in sizes[True]
    assert E * Ce in sizes[False]


def test_deterministic_on_ragged():
    N, ei, x, table, index, cot = (v.to(DEV) if torch.is_tensor(v) else v for v in _case("ragged"))
    pm = _vector_layer(3)
    with _vec(True):
        a, t = _tags(lambda: _step(pm, x, ei, table, index, cot))
        b = _step(pm, x, ei, table, index, cot)
    _assert_indexed_tags(t, route=_step.route)
    _assert_same(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 4. ineligible calls keep today's path
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["dropout", "chunked", "bf16", "message", "strided_index"])
def test_ineligible_keeps_dense_path(what):
    import cgat_amd as P
    from cgat_amd import chunked
    N, ei, x, table, index, cot = (v.to(DEV) if torch.is_tensor(v) else v for v in _case("c150"))

    class MyNodes(P.GATConvNodes):
        def message(self, x_i, x_j, edge_attr, edge_index_i, plan=None):
            return super().message(x_i, x_j, edge_attr, edge_index_i, plan=plan)
    pm = _vector_layer(3, cls=MyNodes if what == "message" else None, dropout=0.1 if what == "dropout" else 0).train()
    if what == "strided_index":
        index = torch.stack([index, index], dim=1)[:, 0]
        assert not index.is_contiguous()
    x0 = torch.randn(N, 128, generator=torch.Generator().manual_seed(14)).to(DEV)   # (the chunked pass slices it)
    prev = chunked.max_edges_per_pass()
    res = []
    try:
        if what == "chunked":
            P.set_max_edges_per_pass(ei.shape[1] // 3)
        with _mode("f16x3c", "bf16" if what == "bf16" else "f32"):
            for on in (True, False):
                with _vec(on):
                    r, t = _tags(lambda: _step(pm, x, ei, table, index, cot, x0=x0))
                print(f"[indexed-vector] ineligible {what} switch {on}: {t}")
                _assert_dense_tags(t, _step.route)
                res.append(r)
    finally:
        P.set_max_edges_per_pass(prev)
    if what != "dropout":                                                     # (the dropout case draws: tags only)
        _assert_same(res[0], res[1])


# ---------------------------------------------------------------------------------------------------------------------
# 5. the harness-default network
# ---------------------------------------------------------------------------------------------------------------------
HARNESS = dict(rezero=True, mean_pooling=False, neighbor_number=24, msg_heads=5, update_edges=True, vector_attention=True,
               global_vector_attention=True, n_graph=5)


def test_network_training_vs_oracle(monkeypatch):
    """The harness constructor at 24 crystals, K = 24, train mode, forward + backward with set_indexed_edge_attr and the
    new switch on, through _compare_with_oracle with its default admission limits.

    Measured on an MI355X: passes in f16x3c (the default) and f16x3 (f32: not run).  In bf16x6 ONE tensor misses the flat bound: the
    scalar gradient of graphs.2.Node.Pooling_NN.damping, err 7.800e-08 against 6.834e-08 allowed (1.14e-4 of |ref| =
    6.834e-04).  On that scalar the oracle's own fp32 result is 8.914e-08 (1.30e-4 of |ref|) away from its fp64 result,
    more than the bound, and this route's value is 0.13 of that distance away from fp64; with the switch off the same
    scalar is at 1.16e-5 of |ref| (oracle fp32 noise 1.03e-4 there), in f16x3c at 6.8e-7 (on) and 3.6e-5 (off).  The bound
    and the case stay as they are; the bf16x6 run of this test fails."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    from test_hip_golden import _compare_with_oracle, recipe
    b, roost = P.synthetic_batch(24, 20, 24, seed=8)
    inputs = {"x": b.x, "edge_index": b.edge_index, "edge_attr": b.edge_attr, "batch": b.batch,
              "r0": roost[0], "r1": roost[1], "r2": roost[2], "r3": roost[3], "r4": roost[4]}
    taken = []
    orig = P.CGAtNet._graphs_indexed
    monkeypatch.setattr(P.CGAtNet, "_graphs_indexed", lambda self, *a: (taken.append(1), orig(self, *a))[1])

    def call(m, i):
        bb = recipe.GraphBatch(i["x"], i["edge_index"], i["edge_attr"], i["batch"])
        return m(bb, (t for t in (i["r0"], i["r1"], i["r2"], i["r3"], i["r4"])))
    kw = dict(HARNESS)
    n_graph = kw.pop("n_graph")
    mk = lambda ns: (lambda: ns.CGAtNet(200, 128, n_graph, **kw))
    with _vec(True, attr=True):
        worst, t = _tags(lambda: _compare_with_oracle(mk(P), mk(O), inputs, call, label="indexed_vector_net_training"))
    print(f"[indexed-vector] harness-default training: worst err/|ref| {worst:.3e}; tags {t}")
    assert taken, "the indexed form of the stack was not taken"
    _assert_indexed_tags(t)


def test_network_eval_vs_oracle_and_switch_off():
    refs, pm, b, roost = _net_pair(24, K=24, **HARNESS)

    def run(on):
        with _vec(on, attr=True), torch.no_grad():
            return _tags(lambda: pm(b, roost))
    on, t_on = run(True)
    off, t_off = run(False)
    print(f"[indexed-vector] harness-default eval tags: on {t_on}; off {t_off}")
    _assert_indexed_tags(t_on, backward=False)
    _assert_dense_tags(t_off)
    assert t_off["edge_z"] > 0, t_off
    _check_both("harness default eval, vector switch", on, off, *refs())


# ---------------------------------------------------------------------------------------------------------------------
# 6. capture
# ---------------------------------------------------------------------------------------------------------------------
def test_captured_step_replays_to_eager_bits():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "indexed_vector_capture_worker.py")], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "INDEXED_VECTOR_CAPTURE_OK" in r.stdout, r.stdout[-2000:]
