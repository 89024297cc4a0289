"""Training-mode attention dropout of GATConvNodes on the operand-split route with the keep-mask pooling kernels
(nets.GATConvNodes._attn_dropout_route; ops.set_fused_attention_dropout): parity against the oracle with the drawn
masks replayed (the project's criterion, test_hip_golden._compare_with_oracle, unchanged), the route actually taken,
the same mask per edge as the MessagePassing-style route draws from the same seed, and eval mode / p = 1."""
import pytest
import torch

from test_hip_golden import _compare_with_oracle

pytestmark = pytest.mark.gpu

CALL = lambda m, i: m(i["x"], i["edge_index"], i["edge_attr"], i["x_0"])
# (crystals, atoms, neighbours): 480 atoms (the small-row branch of the row kernels) and 2 060 atoms, above its 2 048 rows
SMALL, LARGE = (24, 20, 12), (103, 20, 4)


def _layer_inputs(shape, seed=3, C=128):
    import cgat_amd as P
    b, _ = P.synthetic_batch(*shape, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    N, E = b.num_nodes, b.edge_index.shape[1]
    return {"x": torch.randn(N, C, generator=g), "edge_index": b.edge_index, "edge_attr": torch.randn(E, C, generator=g),
            "x_0": torch.randn(N, C, generator=g)}


@pytest.fixture
def switch():
    """Leaves the switch as it found it."""
    import cgat_amd as P
    was = P.get_fused_attention_dropout()
    yield P.set_fused_attention_dropout
    P.set_fused_attention_dropout(was)


def _parity(H, vector, shape, **extra):
    import cgat_amd as P
    from oracle import cgat_oracle as O
    torch.manual_seed(11)
    kw = dict(concat=True, dropout=0.3, vector_attention=vector, **extra)
    _compare_with_oracle(lambda: P.GATConvNodes(128, 128, 128, H, **kw), lambda: O.GATConvNodes(128, 128, 128, H, **kw),
                         _layer_inputs(shape), CALL)


@pytest.mark.parametrize("H,vector", [(3, False), (3, True), (5, True)], ids=["h3-scalar", "h3-vector", "h5-vector"])
def test_parity_small_batch(switch, H, vector):
    import cgat_amd as P
    assert P.get_fused_attention_dropout()
    _parity(H, vector, SMALL)


@pytest.mark.parametrize("H,vector", [(3, False), (3, True), (5, True)], ids=["h3-scalar", "h3-vector", "h5-vector"])
def test_parity_above_the_small_row_limit(switch, H, vector):
    ins = _layer_inputs(LARGE)
    assert ins["x"].shape[0] == 2060 and ins["edge_index"].shape[1] == 8240
    _parity(H, vector, LARGE, final=True)


def test_parity_first_layer_update(switch):
    """first=True, not final: the masked aggregate is the hypernetwork update's input."""
    _parity(3, False, SMALL, first=True)


def _train_step(layer, ins):
    for v in ins.values():
        if v.is_floating_point():
            v.grad = None
    y = CALL(layer, ins)
    y.square().sum().backward()
    torch.cuda.synchronize()
    return y


def _gpu_inputs(shape):
    return {k: (v.to("cuda:0").requires_grad_(True) if v.is_floating_point() else v.to("cuda:0"))
            for k, v in _layer_inputs(shape).items()}


@pytest.mark.parametrize("vector", [False, True], ids=["scalar", "vector"])
def test_route_taken(switch, vector):
    import cgat_amd as P
    from cgat_amd import ops
    torch.manual_seed(2)
    layer = P.GATConvNodes(128, 128, 128, 3, concat=True, dropout=0.3, vector_attention=vector).to("cuda:0")
    ins = _gpu_inputs(SMALL)
    counts = {}
    for on in (True, False):
        switch(on)
        ops.prof_reset(); ops.prof_enable(True)
        try:
            _train_step(layer, ins)
        finally:
            ops.prof_enable(False)
        counts[on] = (ops.prof_get("seg_attnpool_drop_fwd")[0], ops.prof_get("seg_attnpool_drop_bwd")[0])
        route = layer.route(ins["x"], ins["edge_index"], ins["edge_attr"])
        assert route == (("vector_dropout" if on else "message"), False, False), route
    assert counts[True][0] >= 1 and counts[True][1] >= 1, counts
    assert counts[False] == (0, 0), counts
    # a subclass overriding message() keeps the MessagePassing-style route
    switch(True)

    class Sub(P.GATConvNodes):
        def message(self, *args, **kw):
            return super().message(*args, **kw)
    torch.manual_seed(2)
    sub = Sub(128, 128, 128, 3, concat=True, dropout=0.3, vector_attention=vector).to("cuda:0")
    ops.prof_reset(); ops.prof_enable(True)
    try:
        _train_step(sub, ins)
    finally:
        ops.prof_enable(False)
    assert ops.prof_get("seg_attnpool_drop_fwd")[0] == 0
    assert sub.route(ins["x"], ins["edge_index"], ins["edge_attr"]) == ("message", False, False)


def test_chunked_execution_keeps_the_message_passing_route(switch):
    """Beyond max_edges_per_pass the layer runs over closed chunks; those keep the MessagePassing-style route."""
    import cgat_amd as P
    from cgat_amd import chunked, ops
    torch.manual_seed(2)
    layer = P.GATConvNodes(128, 128, 128, 3, concat=True, dropout=0.3).to("cuda:0")
    ins = _gpu_inputs(SMALL)
    was = chunked.max_edges_per_pass()
    P.set_max_edges_per_pass(ins["edge_index"].shape[1] // 3)
    ops.prof_reset(); ops.prof_enable(True)
    try:
        y = CALL(layer, ins)
        torch.cuda.synchronize()
        c = chunked.closed_chunks(ins["edge_index"], ins["x"].shape[0], chunked.max_edges_per_pass())[0]
        route = layer.route(ins["x"][c.n0:c.n1], c.edge_index, ins["edge_attr"][c.e0:c.e1], inner_pass=True)
    finally:
        ops.prof_enable(False)
        P.set_max_edges_per_pass(was)
    assert route == ("message", False, False), route
    assert bool(torch.isfinite(y).all())
    assert ops.prof_get("seg_attnpool_drop_fwd")[0] == 0
    assert ops.prof_get("seg_softmax")[0] >= 2                      # one segment softmax per chunk


@pytest.mark.parametrize("vector", [False, True], ids=["scalar", "vector"])
def test_same_mask_as_the_message_passing_route(switch, vector):
    """One seed, one mask per edge, whichever route runs (recorded in original edge order); the switched-off route
    still passes the oracle comparison (the switched-on one: the parity tests above)."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    torch.manual_seed(2)
    layer = P.GATConvNodes(128, 128, 128, 3, concat=True, dropout=0.3, vector_attention=vector).to("cuda:0")
    ins = _gpu_inputs(SMALL)
    E = ins["edge_index"].shape[1]
    masks = {}
    for on in (True, False):
        switch(on)
        torch.manual_seed(77)
        rec = P.debug.record_masks(layer)
        with rec:
            _train_step(layer, ins)
        assert len(rec.dropout) == 1
        masks[on] = rec.dropout[0]
    assert masks[True].shape == (E, 3, 128 if vector else 1)
    assert torch.equal(masks[True], masks[False])
    assert 0 < int((masks[True] == 0).sum()) < masks[True].numel()
    switch(False)
    torch.manual_seed(11)
    kw = dict(concat=True, dropout=0.3, vector_attention=vector)
    _compare_with_oracle(lambda: P.GATConvNodes(128, 128, 128, 3, **kw), lambda: O.GATConvNodes(128, 128, 128, 3, **kw),
                         _layer_inputs(SMALL), CALL)


@pytest.mark.parametrize("vector", [False, True], ids=["scalar", "vector"])
def test_eval_mode_and_full_dropout(switch, vector):
    """Eval mode: the layer with dropout is bit-identical to the layer without; p = 1: the aggregate is exactly zero."""
    import cgat_amd as P
    assert P.get_fused_attention_dropout()
    dev = "cuda:0"
    ins = {k: v.to(dev) for k, v in _layer_inputs(SMALL).items()}
    torch.manual_seed(1)
    drop = P.GATConvNodes(128, 128, 128, 3, concat=True, dropout=0.4, vector_attention=vector).to(dev)
    torch.manual_seed(1)
    plain = P.GATConvNodes(128, 128, 128, 3, concat=True, vector_attention=vector).to(dev)
    with torch.no_grad():
        y_train = CALL(drop, ins)
        y_plain = CALL(plain, ins)
        drop.eval()
        y_eval = CALL(drop, ins)
    assert torch.equal(y_eval, y_plain)
    assert not torch.equal(y_train, y_plain)
    torch.manual_seed(1)
    all_ = P.GATConvNodes(128, 128, 128, 3, concat=True, dropout=1.0, final=True, vector_attention=vector).to(dev)
    with torch.no_grad():
        assert float(CALL(all_, ins).abs().max()) == 0.0
