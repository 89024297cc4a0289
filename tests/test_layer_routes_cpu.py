"""The route decisions of GATConvNodes / GATConvEdges (cgat_amd.nets.nodes_route, edges_route) on hand-written fact records:
no tensor on a device, no plan, no launch.  Every expectation is read off the code the decision was transcribed from -- the
three-stage routing of the commit before it -- and its row cites that code: `nets.py:L` / `ops.py:L` are lines of
cgat_amd/nets.py and cgat_amd/ops.py at commit 5edc7c5 (GATConvNodes._indexed_route nets.py:276-294, _attn_dropout_route
341-349, propagate 395-411, _propagate_one 413-442, forward 475-486; GATConvEdges.forward 146-169; ops.infer_route
ops.py:319-326, indexed_route 415-426, train_indexed_route 480-501, vector_indexed_route 700-710)."""
import pytest
import torch

from cgat_amd import nets
from cgat_amd.hypernet import H_Net, H_Net_0
from cgat_amd.mlp import SimpleNetwork
from cgat_amd.nets import EdgeFacts, NodeFacts, Route

# a scalar-attention layer, dense edge features, eval mode, a backward to follow, every opt-in switch off
S = NodeFacts(N=300, E=1000, C=128, Ce=128, H=3, Hd=256, pooling=H_Net)
LF = S._replace(overlap=True)                                              # ... under ops.overlap_enabled()
V = S._replace(vector=True)                                                # the vector-attention layer
D = S._replace(drop=True, pool_supported=True)                             # training-mode attention dropout
IDX = dict(indexed_input=True, R=13, operands_ok=True)                     # an IndexedEdgeAttr arrives, operands in order
SI_NG = S._replace(grad_enabled=False, infer_indexed_ok=True, **IDX)       # ... under torch.no_grad()
SI_TR = S._replace(indexed_training=True, train_indexed_ok=True, **IDX)    # ... with a backward, training switch on
VI = V._replace(indexed_vector=True, edge_hidden_indexed_ok=True, **IDX)   # ... vector attention, vector switch on

NODE_ROWS = [
    # ---- each kind ----
    ("scalar", S, {}, Route("scalar")),                                                    # nets.py:421-422
    ("pair", S, dict(x_is_tensor=False), Route("pair")),                                   # nets.py:478-485
    ("pair-indexed-densifies", SI_NG, dict(x_is_tensor=False), Route("pair")),             # nets.py:284
    ("layer_fused", LF, {}, Route("layer_fused")),                                         # nets.py:417-420
    ("vector", V, {}, Route("vector")),                                                    # nets.py:423-424
    ("vector_dropout", D, {}, Route("vector_dropout")),                                    # nets.py:425-429
    ("message", S, dict(message_own=False), Route("message")),                             # nets.py:421, 430-441
    # ---- the scalar route and its forward without grad (ops.infer_route) ----
    ("scalar-no-grad-mode", S, dict(grad_enabled=False), Route("scalar", False, True)),    # ops.py:324-325
    ("scalar-nothing-requires-grad", S, dict(requires_grad=False), Route("scalar", False, True)),      # ops.py:326
    ("scalar-no-grad-switch-off", S, dict(grad_enabled=False, fused_infer=False), Route("scalar")),    # ops.py:322
    ("scalar-no-grad-recording", S, dict(grad_enabled=False, recording=True), Route("scalar")),        # ops.py:322
    ("scalar-update-overridden", S, dict(update_own=False), Route("scalar")),              # nets.py:421 (message alone)
    # ---- layer_fused and its neighbours ----
    ("layer_fused-final", LF, dict(final=True), Route("scalar")),                          # nets.py:417
    ("layer_fused-update-overridden", LF, dict(update_own=False), Route("scalar")),        # nets.py:418, 421
    ("layer_fused-message-overridden", LF, dict(message_own=False), Route("message")),     # nets.py:418, 430
    ("layer_fused-other-pooling", LF, dict(pooling=SimpleNetwork), Route("scalar")),       # nets.py:419
    ("layer_fused-h_net_0", LF, dict(pooling=H_Net_0, first=True), Route("layer_fused")),  # nets.py:419
    ("layer_fused-vector", LF, dict(vector=True), Route("vector")),                        # nets.py:417, 423
    ("layer_fused-drop", LF, dict(drop=True, pool_supported=True), Route("vector_dropout")),           # nets.py:417, 425
    ("layer_fused-no-grad", LF, dict(grad_enabled=False), Route("layer_fused", False, True)),          # nets.py:387-390
    # ---- vector ----
    ("vector-message-overridden", V, dict(message_own=False), Route("message")),           # nets.py:423, 430
    ("vector-no-grad", V, dict(grad_enabled=False), Route("vector")),                      # nets.py:423 (one form)
    ("vector-drop", V, dict(drop=True, pool_supported=True), Route("vector_dropout")),     # nets.py:425
    # ---- training-mode attention dropout (GATConvNodes._attn_dropout_route) ----
    ("drop-inner-pass", D, dict(inner_pass=True), Route("message")),                       # nets.py:409, 425
    ("drop-switch-off", D, dict(fused_dropout=False), Route("message")),                   # nets.py:345
    ("drop-message-overridden", D, dict(message_own=False), Route("message")),             # nets.py:345
    ("drop-update-overridden", D, dict(update_own=False), Route("vector_dropout")),        # nets.py:345 (message alone)
    ("drop-x-on-cpu", D, dict(x_cuda=False), Route("message")),                            # nets.py:345
    ("drop-edge-attr-on-cpu", D, dict(edge_attr_cuda=False), Route("message")),            # nets.py:346
    ("drop-x-not-f32", D, dict(x_f32=False), Route("message")),                            # nets.py:346
    ("drop-no-edges", D, dict(E=0), Route("message")),                                     # nets.py:346
    ("drop-pool-shape-refused", D, dict(pool_supported=False), Route("message")),          # nets.py:349
    # ---- an IndexedEdgeAttr on the scalar layer without grad (ops.indexed_route) ----
    ("indexed-no-grad", SI_NG, {}, Route("scalar", True, True)),                           # nets.py:294, ops.py:415-426
    ("indexed-no-grad-library-refuses", SI_NG, dict(infer_indexed_ok=False), Route("scalar", False, True)),  # ops.py:426
    ("indexed-no-grad-recording", SI_NG, dict(recording=True), Route("scalar")),           # ops.py:322, 420
    ("indexed-no-grad-switch-off", SI_NG, dict(fused_infer=False), Route("scalar")),       # ops.py:322, 420
    ("indexed-update-overridden", SI_NG, dict(update_own=False), Route("scalar", False, True)),        # nets.py:285, 421
    ("indexed-message-overridden", SI_NG, dict(message_own=False), Route("message")),      # nets.py:285, 430
    ("indexed-drop", SI_NG, dict(drop=True, pool_supported=True), Route("vector_dropout")),            # nets.py:284, 425
    ("indexed-over-budget", SI_NG, dict(over_budget=True), Route("scalar", False, True)),  # nets.py:286
    ("indexed-x-on-cpu", SI_NG, dict(x_cuda=False), Route("scalar", False, True)),         # nets.py:286
    ("indexed-x-not-f32", SI_NG, dict(x_f32=False), Route("scalar", False, True)),         # ops.py:418
    ("indexed-x-not-2d", SI_NG, dict(x_2d=False), Route("scalar", False, True)),           # ops.py:418
    ("indexed-no-grad-ignores-index-layout", SI_NG, dict(operands_ok=False), Route("scalar", True, True)),   # ops.py:415-426
    ("indexed-no-grad-layer_fused", SI_NG, dict(overlap=True), Route("layer_fused", True, True)),      # nets.py:381-384
    # ---- ... with a backward to follow (ops.train_indexed_route) ----
    ("indexed-grad-switch-off", SI_TR, dict(indexed_training=False), Route("scalar")),     # ops.py:484
    ("indexed-train", SI_TR, {}, Route("scalar", True, False)),                            # nets.py:294, ops.py:480-501
    ("indexed-train-recording", SI_TR, dict(recording=True), Route("scalar", True, False)),            # ops.py:483-484
    ("indexed-train-library-refuses", SI_TR, dict(train_indexed_ok=False), Route("scalar")),           # ops.py:501
    ("indexed-train-operands", SI_TR, dict(operands_ok=False), Route("scalar")),           # ops.py:491-494
    ("indexed-train-nothing-requires-grad", SI_TR, dict(requires_grad=False), Route("scalar", False, True)),  # ops.py:495, 426
    ("indexed-train-no-grad-mode", SI_TR, dict(grad_enabled=False, infer_indexed_ok=True), Route("scalar", True, True)),  # ops.py:484, 420
    ("indexed-train-x-not-f32", SI_TR, dict(x_f32=False), Route("scalar")),                # ops.py:486
    ("indexed-train-layer_fused", SI_TR, dict(overlap=True), Route("layer_fused", True, False)),       # nets.py:385-386
    ("indexed-train-final", SI_TR, dict(overlap=True, final=True), Route("scalar", True, False)),      # nets.py:417, 271
    ("indexed-train-over-budget", SI_TR, dict(over_budget=True), Route("scalar")),         # nets.py:286
    # ---- ... on the vector layer (ops.vector_indexed_route) ----
    ("indexed-vector-switch-off", VI, dict(indexed_vector=False), Route("vector")),        # ops.py:705
    ("indexed-vector", VI, {}, Route("vector", True)),                                     # nets.py:288-292, ops.py:700-710
    ("indexed-vector-no-grad", VI, dict(grad_enabled=False), Route("vector", True)),       # ops.py:703 (with grad and without)
    ("indexed-vector-recording", VI, dict(recording=True), Route("vector", True)),         # ops.py:703-704
    ("indexed-vector-library-refuses", VI, dict(edge_hidden_indexed_ok=False), Route("vector")),       # ops.py:710
    ("indexed-vector-operands", VI, dict(operands_ok=False), Route("vector")),             # ops.py:708
    ("indexed-vector-drop", VI, dict(drop=True, pool_supported=True), Route("vector_dropout")),        # nets.py:284, 425
    ("indexed-vector-drop-refused", VI, dict(drop=True), Route("message")),                # nets.py:284, 349, 430
    ("indexed-vector-over-budget", VI, dict(over_budget=True), Route("vector")),           # nets.py:286
    ("indexed-vector-update-overridden", VI, dict(update_own=False), Route("vector")),     # nets.py:285, 423
    ("indexed-vector-ignores-scalar-switches", V._replace(indexed_training=True, train_indexed_ok=True, infer_indexed_ok=True,
                                                          **IDX), {}, Route("vector")),    # nets.py:288-292
]


@pytest.mark.parametrize("name,base,flip,want", NODE_ROWS, ids=[r[0] for r in NODE_ROWS])
def test_nodes_route(name, base, flip, want):
    assert nets.nodes_route(base._replace(**flip)) == want


def test_every_kind_has_a_row():
    assert {r[3].kind for r in NODE_ROWS} == {"pair", "layer_fused", "scalar", "vector", "vector_dropout", "message"}
    assert sum(1 for r in NODE_ROWS if len(r[2]) == 1) >= 30               # single facts whose flip moves the call


EDGE_ROWS = [
    ("rowwise", EdgeFacts(), Route("rowwise")),                                                        # nets.py:153-154
    ("rowwise-indexed", EdgeFacts(indexed_input=True), Route("rowwise", True)),                        # nets.py:150-151
    ("fast", EdgeFacts(no_hyper=False), Route("fast")),                                                # nets.py:157-158
    ("fast-indexed-densifies", EdgeFacts(no_hyper=False, indexed_input=True), Route("fast")),          # nets.py:152
    ("generic-x-on-cpu", EdgeFacts(no_hyper=False, x_cuda=False), Route("generic")),                   # nets.py:157, 162-166
    ("generic-other-networks", EdgeFacts(no_hyper=False, networks_own=False), Route("generic")),       # nets.py:157
]


@pytest.mark.parametrize("name,facts,want", EDGE_ROWS, ids=[r[0] for r in EDGE_ROWS])
def test_edges_route(name, facts, want):
    assert nets.edges_route(facts) == want


def test_library_answers_are_asked_only_where_they_decide():
    """A dense call, and an indexed call that another fact already sends down the dense path, ask the library nothing."""
    def boom():
        raise AssertionError("asked")
    lazy = dict(pool_supported=boom, infer_indexed_ok=boom, train_indexed_ok=boom, edge_hidden_indexed_ok=boom)
    for f in (S, LF, V, S._replace(grad_enabled=False)):
        nets.nodes_route(f._replace(**lazy))
    for f in (SI_NG._replace(over_budget=True), SI_NG._replace(update_own=False), SI_TR._replace(indexed_training=False),
              VI._replace(indexed_vector=False), VI._replace(operands_ok=False)):
        lazy_f = f._replace(**lazy)
        assert not nets.nodes_route(lazy_f).indexed
    asked = []
    f = SI_TR._replace(train_indexed_ok=lambda: asked.append("train") or True, infer_indexed_ok=boom,
                       edge_hidden_indexed_ok=boom, pool_supported=boom)
    assert nets.nodes_route(f) == Route("scalar", True, False) and asked == ["train"]


def test_facts_and_route_of_a_call_on_the_cpu():
    """GATConvNodes.route / GATConvEdges.route gather the facts of a call and launch nothing: CPU tensors suffice."""
    import cgat_amd as P
    x, ei, ea = torch.zeros(4, 16), torch.zeros(2, 8, dtype=torch.long), torch.zeros(8, 16)
    layer = P.GATConvNodes(16, 16, 16, 3, concat=True, dropout=0.3).eval()
    f = layer._facts(x, ei, ea)
    assert (f.N, f.E, f.C, f.Ce, f.H, f.Hd, f.R) == (4, 8, 16, 16, 3, 32, 0)
    assert f.x_is_tensor and not f.x_cuda and f.x_f32 and f.x_2d and not f.edge_attr_cuda
    assert f.message_own and f.update_own and not f.drop and not f.vector and not f.final and f.pooling is H_Net
    assert f.requires_grad and f.grad_enabled == torch.is_grad_enabled() and not f.indexed_input and not f.inner_pass
    assert layer.route(x, ei, ea).kind in ("scalar", "layer_fused")
    with torch.no_grad():
        assert layer.route(x, ei, ea).no_grad is (P.get_fused_inference() and not P.debug.recording())
    assert layer.train().route(x, ei, ea) == Route("message")                  # drop, CPU tensors
    assert layer._facts(x, ei, ea, inner_pass=True).inner_pass
    assert layer.route((x, x), ei, ea) == Route("pair")

    class Own(P.GATConvNodes):
        def update(self, aggr_out, x_0, x, _mean_done=False):
            return aggr_out
    f = Own(16, 16, 16, 3, concat=True).eval()._facts(x, ei, ea)
    assert f.message_own and not f.update_own
    assert P.GATConvNodes(16, 16, 16, 3, vector_attention=True, final=True).eval().route(x, ei, ea) == Route("vector")
    assert P.GATConvEdges(16, 16, 16, 3, no_hyper=True).route(x, ei, ea) == Route("rowwise")
    assert P.GATConvEdges(16, 16, 16, 3, no_hyper=False).route(x, ei, ea) == Route("generic")
