"""The head combination of GATConvEdges(no_hyper=False) as one kernel per direction (ops.EdgeHeadCombineFn,
csrc/edgecomb.hip) against the sequence of torch ops it replaces (reference CGAT.py:214-223):

  (1) the op against the same expression in fp64, bounded by 2 x the error of the fp32 torch sequence on the same
      inputs in the same run -- both round the same operations once each, in a different order;
  (2) a row whose logit overflows exp: non-finite values where the torch sequence has them (no max-subtraction);
  (3) bitwise determinism; (4) shapes the kernels do not take; (5) the layer against the oracle; (6) the switch.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

E_SIZES = (1, 257, 4099)
SHAPES = ((3, 1, 128), (5, 128, 128), (1, 1, 40), (8, 1, 64), (3, 16, 16), (2, 1, 256))     # (H, aF, Co)
# the fused form's error may be this many times the torch sequence's: room for the order of the roundings, nothing else
# (a CPU emulation of a reordered form gave 0.98 .. 1.43 x)
ORDER_FACTOR = 2.0


def eager_combine(sa, sm, keep, perm):
    """The sequence of torch ops in cgat_amd/nets.py with the route switched off (the yardstick)."""
    alpha = sa.exp()
    alpha = alpha / alpha.sum(dim=1, keepdim=True)
    if keep is not None:
        alpha = alpha * keep
    aggr = (sm * alpha).mean(dim=1)
    if perm is None:
        return aggr
    return torch.empty_like(aggr).index_copy(0, perm.long(), aggr)


def make_case(E, H, aF, Co, with_perm, with_keep, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * E + 31 * H + 3 * aF + Co + 2 * with_perm + with_keep)
    sa = (2.0 * torch.randn(E, H, aF, generator=g)).to(DEV)
    sm = torch.randn(E, H, Co, generator=g).to(DEV)
    cot = torch.randn(E, Co, generator=g).to(DEV)
    keep = ((torch.rand(E, H, aF, generator=g) < 0.7).float() / 0.7).to(DEV) if with_keep else None
    perm = torch.randperm(E, generator=g).to(torch.int32).to(DEV) if with_perm else None
    return sa, sm, keep, perm, cot


def _run(fn, sa, sm, keep, perm, cot, dtype=torch.float32):
    sa = sa.to(dtype).requires_grad_(True)
    sm = sm.to(dtype).requires_grad_(True)
    out = fn(sa, sm, None if keep is None else keep.to(dtype), perm)
    g_sa, g_sm = torch.autograd.grad((out * cot.to(dtype)).sum(), [sa, sm])
    return {"out": out.detach(), "g_sa": g_sa, "g_sm": g_sm}


def _rel(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def op_errors(E, H, aF, Co, with_perm, with_keep):
    """Max-norm relative error against the fp64 expression, per tensor: {"fused": {...}, "eager": {...}}."""
    from cgat_amd import ops
    case = make_case(E, H, aF, Co, with_perm, with_keep)
    ref = _run(eager_combine, *case, dtype=torch.float64)
    eager = _run(eager_combine, *case)
    fused = _run(ops.EdgeHeadCombineFn.apply, *case)
    res = {"fused": {}, "eager": {}, "fused_g_sa_absmax": float(fused["g_sa"].abs().max())}
    for k in ("out", "g_sa", "g_sm"):
        assert fused[k].shape == ref[k].shape and fused[k].dtype == torch.float32, k
        res["fused"][k] = _rel(fused[k], ref[k])
        res["eager"][k] = _rel(eager[k], ref[k])
    return res


@pytest.mark.parametrize("with_keep", [False, True], ids=["nokeep", "keep"])
@pytest.mark.parametrize("with_perm", [False, True], ids=["noperm", "perm"])
@pytest.mark.parametrize("H,aF,Co", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("E", E_SIZES)
def test_op_vs_fp64(E, H, aF, Co, with_perm, with_keep):
    r = op_errors(E, H, aF, Co, with_perm, with_keep)
    print(f"E={E} H={H} aF={aF} Co={Co} perm={with_perm} keep={with_keep}: "
          + ", ".join(f"{k} fused {r['fused'][k]:.3e} eager {r['eager'][k]:.3e}" for k in ("out", "g_sa", "g_sm")))
    if H == 1:
        # one head: alpha == 1, and the logit gradient alpha (q - alpha q) is exactly zero
        assert r["fused_g_sa_absmax"] == 0.0
    for k in ("out", "g_sa", "g_sm"):
        assert r["fused"][k] <= ORDER_FACTOR * r["eager"][k], (k, r["fused"][k], r["eager"][k])


@pytest.mark.parametrize("H,aF,Co", [(3, 1, 128), (5, 128, 128)], ids=lambda v: str(v))
def test_non_finite_row_as_the_torch_sequence(H, aF, Co):
    """exp(100) overflows fp32: without a max-subtraction the row's alpha is inf / inf.  The non-finite values of `out`
    sit exactly where the torch sequence has them."""
    from cgat_amd import ops
    sa, sm, keep, perm, _ = make_case(257, H, aF, Co, True, True, seed=1)
    sa[100, 1, 0] = 100.0
    want = eager_combine(sa, sm, keep, perm)
    got = ops.EdgeHeadCombineFn.apply(sa, sm, keep, perm)
    bad = ~torch.isfinite(want)
    assert int(bad.sum()) == (Co if aF == 1 else 1)
    assert torch.equal(~torch.isfinite(got), bad)
    assert torch.allclose(got[~bad], want[~bad], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("H,aF,Co", [(3, 1, 128), (5, 128, 128), (8, 1, 64)], ids=lambda v: str(v))
def test_determinism_bitwise(H, aF, Co):
    from cgat_amd import ops
    case = make_case(4099, H, aF, Co, True, True, seed=2)
    a = _run(ops.EdgeHeadCombineFn.apply, *case)
    b = _run(ops.EdgeHeadCombineFn.apply, *case)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_empty_and_single_gradient():
    """E == 0 launches nothing; a gradient that is not needed is not computed (null pointer in the C ABI)."""
    from cgat_amd import ops
    out = ops.EdgeHeadCombineFn.apply(torch.empty(0, 3, 1, device=DEV), torch.empty(0, 3, 128, device=DEV), None, None)
    assert out.shape == (0, 128)
    sa, sm, keep, perm, cot = make_case(257, 3, 1, 128, True, True, seed=3)
    both = _run(ops.EdgeHeadCombineFn.apply, sa, sm, keep, perm, cot)
    sa1 = sa.clone().requires_grad_(True)
    (g_sa,) = torch.autograd.grad((ops.EdgeHeadCombineFn.apply(sa1, sm, keep, perm) * cot).sum(), [sa1])
    sm1 = sm.clone().requires_grad_(True)
    (g_sm,) = torch.autograd.grad((ops.EdgeHeadCombineFn.apply(sa, sm1, keep, perm) * cot).sum(), [sm1])
    assert torch.equal(g_sa, both["g_sa"]) and torch.equal(g_sm, both["g_sm"])


# ---- the layer ------------------------------------------------------------------------------------------------------
def _layer_inputs(C, seed=40):
    import cgat_amd as P
    b, _ = P.synthetic_batch(6, 20, 12, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    N, E = b.num_nodes, b.edge_index.shape[1]
    assert E == 1440
    return {"x": torch.randn(N, C, generator=g), "edge_index": b.edge_index,
            "edge_attr": torch.randn(E, C, generator=g), "x_0": torch.randn(E, C, generator=g)}


def _call(m, i):
    return m(i["x"], i["edge_index"], i["edge_attr"], i["x_0"])


def _launches(fn):
    from cgat_amd import ops
    ops.prof_reset()
    ops.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.prof_enable(False)
    n = ops.prof_get("edge_combine")[0]
    ops.prof_reset()
    return out, n


def _generic_route_layer(P):
    """A GATConvEdges that overrides nothing but whose attention network is a MultiHeadNetwork SUBCLASS: the layer then
    takes the generic route (concatenated rows in the caller's edge order, no permutation)."""
    class SubMultiHead(P.MultiHeadNetwork):
        pass

    class Layer(P.GATConvEdges):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            old = self.MH_A
            self.MH_A = SubMultiHead(old.input_dim, old.output_dim, old.hidden_layer_dim, old.nb_heads)
    return Layer


LAYER_VARIANTS = {
    "scalar_first": dict(C=128, H=3, kw=dict(first=True)),
    "scalar": dict(C=128, H=3, kw=dict(first=False)),
    "vector_h5": dict(C=128, H=5, kw=dict(vector_attention=True)),
    "dropout": dict(C=64, H=3, kw=dict(dropout=0.25), train=True),
    "generic_route": dict(C=128, H=3, kw=dict(), generic=True),
}


@pytest.mark.parametrize("variant", sorted(LAYER_VARIANTS))
def test_layer_vs_oracle(variant):
    import cgat_amd as P
    from oracle import cgat_oracle as O
    from test_hip_golden import _compare_with_oracle
    v = LAYER_VARIANTS[variant]
    C, H = v["C"], v["H"]
    cls = _generic_route_layer(P) if v.get("generic") else P.GATConvEdges
    # the oracle draws the same parameters in the same order: the replaced MH_A of the generic-route layer is drawn
    # after the others, so its state is overwritten by load_state_dict like every other parameter
    mk_p = lambda: cls(C, C, C, H, concat=True, no_hyper=False, **v["kw"])
    mk_o = lambda: O.GATConvEdges(C, C, C, H, concat=True, no_hyper=False, **v["kw"])
    if v.get("train"):
        mk_p0, mk_o0 = mk_p, mk_o
        mk_p, mk_o = (lambda: mk_p0().train()), (lambda: mk_o0().train())
    assert P.get_fused_edge_combine()
    _, n = _launches(lambda: _compare_with_oracle(mk_p, mk_o, _layer_inputs(C), _call,
                                                  label=f"edge_head_combine layer {variant}"))
    assert n >= 2, "the layer did not run the fused head combination"


@pytest.mark.parametrize("C,H", [(30, 3), (64, 9)], ids=["Co30", "H9"])
def test_unsupported_shapes_keep_the_torch_sequence(C, H):
    import cgat_amd as P
    from cgat_amd import ops
    from oracle import cgat_oracle as O
    from test_hip_golden import _compare_with_oracle
    assert not ops.EdgeHeadCombineFn.supported(torch.empty(4, H, 1, device=DEV), torch.empty(4, H, C, device=DEV))
    with pytest.raises(ValueError, match="unsupported"):
        ops.EdgeHeadCombineFn.apply(torch.zeros(4, H, 1, device=DEV), torch.zeros(4, H, C, device=DEV), None, None)
    _, n = _launches(lambda: _compare_with_oracle(lambda: P.GATConvEdges(C, C, C, H, concat=True, no_hyper=False),
                                                  lambda: O.GATConvEdges(C, C, C, H, concat=True, no_hyper=False),
                                                  _layer_inputs(C), _call, label=f"edge_head_combine unsupported C={C} H={H}"))
    assert n == 0


def test_switch_selects_the_route():
    import cgat_amd as P
    torch.manual_seed(5)
    layer = P.GATConvEdges(128, 128, 128, 3, concat=True, no_hyper=False).to(DEV)
    inp = {k: v.to(DEV) for k, v in _layer_inputs(128).items()}

    def step():
        x, e = inp["x"].clone().requires_grad_(True), inp["edge_attr"].clone().requires_grad_(True)
        y = layer(x, inp["edge_index"], e, inp["x_0"])
        return [y.detach()] + list(torch.autograd.grad(y.square().sum(), [x, e] + list(layer.parameters())))
    assert P.get_fused_edge_combine()
    try:
        on, n_on = _launches(step)
        assert n_on == 2                                   # one launch per direction
        P.set_fused_edge_combine(False)
        assert not P.get_fused_edge_combine()
        off1, n_off = _launches(step)
        off2, _ = _launches(step)
        assert n_off == 0
        for a, b in zip(off1, off2):
            assert torch.equal(a, b)
        for a, b in zip(on, off1):                         # the two routes compute the same layer
            assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max())
    finally:
        P.set_fused_edge_combine(True)
