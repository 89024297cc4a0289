"""Parity of the HIP product (cgat_amd, through its reference-shaped module API and the C
ABI underneath) with
  (1) the golden vectors recorded from the unmodified reference (tests/golden/*.npz), and
  (2) the oracle on seeded inputs at sizes the oracle finishes in seconds,
  (3) size-independent properties at the BASELINE size (1M edges).

Tolerance (north_star): max-norm relative <= 1e-4, fp32, per tensor -- outputs, input
gradients and parameter gradients.
"""
import types

import numpy as np
import pytest
import torch

import recipe
from golden_util import check_case, floor_open, maxnorm_rel

pytestmark = pytest.mark.gpu
TOL = 1e-4
# largest |z| / max|z| of a pre-activation whose forced LeakyReLU / ReLU derivative may differ from the oracle's own
MAX_FORCED_REL_Z = 1e-5


def product_ns():
    import cgat_amd as P
    return types.SimpleNamespace(
        MultiHeadNetwork=P.MultiHeadNetwork, GATConvNodes=P.GATConvNodes, GATConvEdges=P.GATConvEdges,
        MHAttention=P.MHAttention, CGAtNet=P.CGAtNet, H_Net_0=P.H_Net_0, H_Net=P.H_Net,
        SimpleNetwork=P.SimpleNetwork, ResidualNetwork=P.ResidualNetwork, WeightedAttention=P.WeightedAttention,
        MessageLayer=P.MessageLayer, Roost=P.Roost, RoostSimpleNetwork=P.SimpleNetwork)


def oracle_ns():
    from oracle import cgat_oracle as O
    return types.SimpleNamespace(
        MultiHeadNetwork=O.MultiHeadNetwork, GATConvNodes=O.GATConvNodes, GATConvEdges=O.GATConvEdges,
        MHAttention=O.MHAttention, CGAtNet=O.CGAtNet, H_Net_0=O.H_Net_0, H_Net=O.H_Net,
        SimpleNetwork=O.SimpleNetwork, ResidualNetwork=O.ResidualNetwork, WeightedAttention=O.WeightedAttention,
        MessageLayer=O.MessageLayer, Roost=O.Roost, RoostSimpleNetwork=O.SimpleNetwork)


_TINY_NAMES = sorted(recipe.tiny_cases(oracle_ns()))
_BASE_NAMES = sorted(recipe.base_cases(oracle_ns()))


@pytest.mark.parametrize("cname", _TINY_NAMES)
def test_golden_tiny(cname):
    case = recipe.tiny_cases(product_ns())[cname]
    check_case("tiny.npz", cname, case, device="cuda:0", tol=TOL)


@pytest.mark.parametrize("cname", _BASE_NAMES)
def test_golden_base(cname):
    case = recipe.base_cases(product_ns())[cname]
    check_case("base.npz", cname, case, device="cuda:0", tol=TOL)


from golden_util import NOISE_MULT
# Gradients that are ZERO in exact arithmetic (MH_A.fc_out.bias by softmax shift invariance, the gate bias of Roost's
# pooling) come out as rounding noise in any summation order; a tensor whose largest entry is below ZERO_FLOOR of the
# largest gradient of the case is compared against that floor instead of against its own magnitude.
ZERO_FLOOR = 1e-6
# The floor `ZERO_FLOOR * case_scale` (case_scale = the largest gradient of the case) is only open to gradients that are
# NUMERICALLY ZERO: their fp64 reference value lies below fp32's resolution of the case (6e-8 of its largest gradient) --
# zero in exact arithmetic (MH_A.fc_out.bias by the softmax's shift invariance, Roost's gate bias) or the remainder of a
# >= 1e7-fold cancellation (tools/crypool_probe.py: in the sin-filled fixture `net_mean` every gradient of the crystal
# pooling's attention branch is such a remainder -- the logit gradient alpha (g - sum alpha g) is 4e-6 of its terms --
# and two correct fp32 evaluations of it differ by more than its value).  Everything else has to meet 1e-4 |ref| (or, for
# the sin-filled fixtures, the reference's own fp32 deviation from fp64).
NUM_ZERO = 1e-7


def _mode():
    import cgat_amd as P
    return P.get_bilinear_mode()


def _compare_with_oracle(mk_prod, mk_orac, inputs, call, tol=TOL, label=None):
    """Same seeded parameters (copied through the shared state_dict layout) and inputs.  The derivative pattern of every
    LeakyReLU / ReLU the HIP backward uses is recorded (cgat_amd.debug.record_masks: post-activation > 0, for the fused
    attention layer through the C ABI's cgat_debug_nodes_attention_signs) and FORCED on the oracle's fp32 and fp64 runs
    (oracle.forced_masks), so that no allowance for sign flips of near-zero pre-activations is needed.  Criterion per
    tensor, flat:
        ||hip - oracle32||_inf <= max(tol * ||oracle||_inf, ZERO_FLOOR * largest gradient of the case)
    No term for the oracle's own fp32 noise, none for flips.  Reported per tensor (gpurun_out/parity_report_<mode>.txt):
    err / |ref|, err / nf with nf = ||oracle32 - oracle64||_inf, and (hip - oracle64) / nf, i.e. how many times noisier
    than the reference's own fp32 arithmetic the HIP path is on that tensor."""
    import cgat_amd as P
    from oracle import cgat_oracle as _O
    torch.manual_seed(1)
    om = mk_orac()
    pm = mk_prod()
    pm.load_state_dict(om.state_dict())           # identical layout is part of the contract
    pm = pm.to("cuda:0")
    import copy
    om64 = copy.deepcopy(om).double()

    def prep(v, dev=None, dt=None):
        if not torch.is_tensor(v):
            return v
        if v.is_floating_point():
            v = v.to(dt) if dt is not None else v.clone()
            return (v.to(dev) if dev else v).requires_grad_(True)
        return v.to(dev) if dev else v
    oin = {k: prep(v) for k, v in inputs.items()}
    oin64 = {k: prep(v, dt=torch.float64) for k, v in inputs.items()}
    pin = {k: prep(v, dev="cuda:0") for k, v in inputs.items()}

    def grads(m, ins, y, c):
        leaves = [v for v in ins.values() if torch.is_tensor(v) and v.requires_grad]
        params = dict(m.named_parameters())
        g = torch.autograd.grad((y * c).sum(), leaves + list(params.values()), allow_unused=True)
        return [f"in{i}" for i in range(len(leaves))] + list(params), g

    rec = P.debug.record_masks(pm)
    with rec as masks:
        yp = call(pm, pin)
    cot = torch.randn(yp.shape, generator=torch.Generator().manual_seed(9))
    _, gp = grads(pm, pin, yp, cot.to("cuda:0"))
    # (training-mode attention dropout, CGAT.py:221 / 325: the keep-masks the HIP run drew are replayed on the oracle)
    with _O.forced_masks(om, masks) as f32, _O.dropout_masks(rec.dropout) as d32:
        yo = call(om, oin)
        names, go = grads(om, oin, yo, cot)
    with _O.forced_masks(om64, masks), _O.dropout_masks(rec.dropout):
        yo64 = call(om64, oin64)
        _, go64 = grads(om64, oin64, yo64, cot.double())
    assert not d32.masks, "dropout masks the oracle never consumed"
    assert f32.stats["layers"] > 0 or not masks, "no activation layer of the oracle took a recorded mask"
    assert all(not v for v in f32.masks.values()), "recorded masks the oracle never consumed: " + \
        ", ".join(k for k, v in f32.masks.items() if v)
    # forcing the HIP run's derivative pattern must only ever move pre-activations that are ZERO at fp32 resolution: a
    # wrong-sign bug on a large |z| would otherwise hide behind the mechanism
    assert f32.stats["max_rel_z"] <= MAX_FORCED_REL_Z, (
        f"a forced derivative pattern disagrees with the oracle's own sign at |z| / max|z| = {f32.stats['max_rel_z']:.2e}")
    failures, worst = [], 0.0
    case_scale = max(float(b.detach().abs().max()) for b in go64 if b is not None)
    import os
    title = label or os.environ.get("PYTEST_CURRENT_TEST", "case").split(" ")[0]
    lines = [f"[{title}] mode {_mode()}: LeakyReLU/ReLU derivative pattern forced on the oracle in {f32.stats['layers']} layers, "
             f"{f32.stats['disagree']} of {f32.stats['elements']} elements differed from the oracle's own sign "
             f"(largest |z| / max|z| among them {f32.stats['max_rel_z']:.1e})",
             "  tensor | err/|ref| | err/nf | (hip-ref64)/nf | nf/|ref| | verdict"]
    items = [("out", yp, yo, yo64)] + list(zip(names, gp, go, go64))
    for name, a, b, b64 in items:
        if b is None:
            assert a is None or float(a.abs().max()) == 0.0, name
            continue
        assert a is not None, name
        a = a.detach().cpu().double()
        ref_max = float(b64.detach().abs().max())
        nf = float((b.detach().double() - b64.detach()).abs().max())
        err = float((a - b.detach().double()).abs().max())
        err64 = float((a - b64.detach()).abs().max())
        num_zero = name != "out" and floor_open(ref_max, case_scale)
        allowed = max(tol * ref_max, ZERO_FLOOR * case_scale if num_zero else 0.0)
        worst = max(worst, err / max(ref_max, 1e-300))
        verdict = "ok" if err <= tol * ref_max else ("ok (zero-gradient floor)" if err <= allowed else "FAIL")
        lines.append(f"  {name:66s} {err / max(ref_max, 1e-300):.2e} {err / max(nf, 1e-300):8.2f} "
                     f"{err64 / max(nf, 1e-300):8.2f} {nf / max(ref_max, 1e-300):.2e}  {verdict}")
        if err > allowed:
            failures.append(f"{name}: err {err:.3e} allowed {allowed:.3e} |ref| {ref_max:.3e} oracle fp32 noise {nf:.3e}")
    _report(lines)
    assert not failures, "\n".join(failures)
    return worst


@pytest.mark.parametrize("heads", [1, 5])
def test_nodes_layer_other_head_counts_vs_oracle(heads):
    """Scalar attention at C = Ce = 128 with 1 and 5 heads (the benchmark has 3): the widths of the per-edge kernels,
    the sign-bit words and the head-per-wave pass of the segment backward all depend on H."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b, _ = P.synthetic_batch(40, 20, 12, seed=5)
    g = torch.Generator().manual_seed(6)
    N, E = b.num_nodes, b.edge_index.shape[1]
    inputs = {"x": torch.randn(N, 128, generator=g), "edge_index": b.edge_index,
              "edge_attr": torch.randn(E, 128, generator=g), "x_0": torch.randn(N, 128, generator=g)}
    call = lambda m, i: m(i["x"], i["edge_index"], i["edge_attr"], i["x_0"])
    _compare_with_oracle(lambda: P.GATConvNodes(128, 128, 128, heads, concat=True),
                         lambda: O.GATConvNodes(128, 128, 128, heads, concat=True), inputs, call)


@pytest.mark.parametrize("C,vector", [(64, False), (96, False), (64, True), (40, False)])
def test_nodes_layer_other_widths_vs_oracle(C, vector):
    """Feature widths other than 128 (the harness' --atom-fea-len is free): per-edge products, stored gZ and the
    hypernetwork's contractions as outer-product operands of the generic engine (gemm.hip / gemmsplit.hip), one layer
    forward + every gradient against the oracle at the flat tolerance.  40 is off the 16-byte grid of the engine's
    fast loader (hidden width 80)."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b, _ = P.synthetic_batch(30, 20, 12, seed=11)
    g = torch.Generator().manual_seed(12)
    N, E = b.num_nodes, b.edge_index.shape[1]
    inputs = {"x": torch.randn(N, C, generator=g), "edge_index": b.edge_index,
              "edge_attr": torch.randn(E, C, generator=g), "x_0": torch.randn(N, C, generator=g)}
    call = lambda m, i: m(i["x"], i["edge_index"], i["edge_attr"], i["x_0"])
    _compare_with_oracle(lambda: P.GATConvNodes(C, C, C, 3, concat=True, vector_attention=vector),
                         lambda: O.GATConvNodes(C, C, C, 3, concat=True, vector_attention=vector), inputs, call)


def test_single_predicted_layer_vs_oracle():
    """A hypernetwork of ONE predicted layer (n_hyper == 1; the module API never builds fewer than two): nothing is
    batched across predicted layers, no LayerNorm, the last layer's gradient is the first's.  HNetFn on one HyperLinear
    against the oracle's predict + apply, same parameters through the shared state_dict layout."""
    import cgat_amd as P
    from cgat_amd import hypernet, ops
    from oracle import cgat_oracle as O
    W, rows, hidden_layers = 128, 130, 3

    class Prod(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.hl = hypernet.HyperLinear(W, W, W, hidden_layers, W)

        def forward(self, h0, v):
            return ops.HNetFn.apply(h0, v, None, 1 + hidden_layers, 1, *self.hl.flat_params())

    class Orac(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.hl = O.HyperLinear(W, W, W, hidden_layers, W)

        def forward(self, h0, v):
            Wp, bp = self.hl.predict(h0)
            return O.HyperLinear.apply_predicted(Wp, bp, v.view(v.shape[0], 1, W)).view(v.shape[0], W)
    g = torch.Generator().manual_seed(31)
    inputs = {"h0": torch.randn(rows, W, generator=g), "v": torch.randn(rows, W, generator=g)}
    _compare_with_oracle(Prod, Orac, inputs, lambda m, i: m(i["h0"], i["v"]))


@pytest.mark.parametrize("first", [True, False])
def test_nodes_layer_vs_oracle_random_init(first):
    """Config 1 -> 2 of BASELINE.json at a size the oracle finishes in seconds: 60 crystals
    (N=1200, E=14400), C=Ce=128, H=3, default (random) initialisation, one GATConvNodes layer."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b, _ = P.synthetic_batch(60, 20, 12, seed=3)
    g = torch.Generator().manual_seed(4)
    N, E = b.num_nodes, b.edge_index.shape[1]
    inputs = {"x": torch.randn(N, 128, generator=g), "edge_index": b.edge_index,
              "edge_attr": torch.randn(E, 128, generator=g), "x_0": torch.randn(N, 128, generator=g)}
    call = lambda m, i: m(i["x"], i["edge_index"], i["edge_attr"], i["x_0"])
    _compare_with_oracle(lambda: P.GATConvNodes(128, 128, 128, 3, concat=True, first=first),
                         lambda: O.GATConvNodes(128, 128, 128, 3, concat=True, first=first), inputs, call)


@pytest.mark.gpu
def test_nodes_layer_vs_oracle_above_small_row_limit():
    """The same layer at 150 crystals (N = 3000, E = 36 000): more rows than the small-row programs take (2048), so the
    node side runs the large-batch kernels -- among them the ONE K = H * Hd launch for the per-head second layer of the
    message network and the heads-batched launch of its input gradients (layers.hip, round 6) -- forward and every
    gradient against the oracle."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b, _ = P.synthetic_batch(150, 20, 12, seed=5)
    g = torch.Generator().manual_seed(6)
    N, E = b.num_nodes, b.edge_index.shape[1]
    assert N > 2048
    inputs = {"x": torch.randn(N, 128, generator=g), "edge_index": b.edge_index,
              "edge_attr": torch.randn(E, 128, generator=g), "x_0": torch.randn(N, 128, generator=g)}
    call = lambda m, i: m(i["x"], i["edge_index"], i["edge_attr"], i["x_0"])
    _compare_with_oracle(lambda: P.GATConvNodes(128, 128, 128, 3, concat=True),
                         lambda: O.GATConvNodes(128, 128, 128, 3, concat=True), inputs, call)


def _runnable_route_rows():
    """The rows of test_attn_workspace.ROUTES that run here: fp32 edge storage, the default mode and f32, at the two
    batches P.synthetic_batch makes (25 / 192 crystals of 12 atoms: 300 atoms, and 2 304 -- the smallest whole batch
    past the small-row programs' 2 048 rows)."""
    from test_attn_workspace import ABOVE, BENCH, ROUTES, SMALL
    return [r[:4] for r in ROUTES if r[0] in ("f16x3c", "f32") and r[1] == "f32" and r[2] in (SMALL, ABOVE) and r[3] == BENCH]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,storage,batch,layer", _runnable_route_rows(),
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_nodes_layer_vs_oracle_on_the_named_route(mode, storage, batch, layer):
    """One layer forward + every gradient against the oracle on each route of the table in tests/test_attn_workspace.py
    that can run, and the route itself: cgat_debug_nodes_attention_route must name what the table says for this shape."""
    import cgat_amd as P
    from cgat_amd import ops
    from oracle import cgat_oracle as O
    from test_attn_workspace import _modes, route_row
    b, _ = P.synthetic_batch(batch[0] // 12, 12, 12, seed=5)
    g = torch.Generator().manual_seed(6)
    N, E = b.num_nodes, b.edge_index.shape[1]
    assert (N, E) == batch and layer == (128, 128, 3, 256)
    inputs = {"x": torch.randn(N, 128, generator=g), "edge_index": b.edge_index,
              "edge_attr": torch.randn(E, 128, generator=g), "x_0": torch.randn(N, 128, generator=g)}
    call = lambda m, i: m(i["x"], i["edge_index"], i["edge_attr"], i["x_0"])
    fwd, bwd = route_row(mode, storage, batch, layer)
    with _modes(mode, storage):
        assert P.debug.nodes_attention_route(N, E, *layer, backward=False) == fwd
        assert P.debug.nodes_attention_route(N, E, *layer, backward=True) == bwd
        _compare_with_oracle(lambda: P.GATConvNodes(128, 128, 128, 3, concat=True),
                             lambda: O.GATConvNodes(128, 128, 128, 3, concat=True), inputs, call)


@pytest.mark.gpu
def test_vector_attention_layer_vs_oracle_random_init():
    """vector_attention=True (the reference harness' shipped default) at the BASELINE widths: the
    operand-split first layer (edge_hidden op on the split-bf16 kernels) + channel-wise softmax against the oracle."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b, _ = P.synthetic_batch(60, 20, 12, seed=3)
    g = torch.Generator().manual_seed(4)
    N, E = b.num_nodes, b.edge_index.shape[1]
    inputs = {"x": torch.randn(N, 128, generator=g), "edge_index": b.edge_index,
              "edge_attr": torch.randn(E, 128, generator=g), "x_0": torch.randn(N, 128, generator=g)}
    call = lambda m, i: m(i["x"], i["edge_index"], i["edge_attr"], i["x_0"])
    _compare_with_oracle(lambda: P.GATConvNodes(128, 128, 128, 3, concat=True, vector_attention=True),
                         lambda: O.GATConvNodes(128, 128, 128, 3, concat=True, vector_attention=True), inputs, call)


def test_ragged_graphs_vs_oracle():
    """Ragged crystals (2..40 atoms), K=24 neighbours, H=5: the DCGAT-like shape of config 4."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    rs = np.random.RandomState(11)
    sizes = rs.randint(2, 41, size=30).tolist()
    b, _ = recipe.build_graphs(sizes, K=24, species_per_graph=rs.randint(1, 5, size=30).tolist(), seed=12)
    g = torch.Generator().manual_seed(5)
    N, E = b.num_nodes, b.edge_index.shape[1]
    inputs = {"x": torch.randn(N, 64, generator=g), "edge_index": b.edge_index,
              "edge_attr": torch.randn(E, 32, generator=g), "x_0": torch.randn(N, 64, generator=g)}
    call = lambda m, i: m(i["x"], i["edge_index"], i["edge_attr"], i["x_0"])
    _compare_with_oracle(lambda: P.GATConvNodes(64, 64, 32, 5, concat=True),
                         lambda: O.GATConvNodes(64, 64, 32, 5, concat=True), inputs, call)


def test_ragged_graphs_fast_widths_vs_oracle():
    """Ragged crystals (2..33 atoms, 7 neighbours) at the BENCHMARK widths (C = Ce = 128, H = 3, Hd = 256): E and N
    are multiples of neither 128 nor 256 nor 8, so every tiled kernel of the default path (edge_zx, edge_seg_bwd,
    edge_ge / edge_gw with their fp16 scales, the contraction kernels, rows_dw128) runs with partial last tiles."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    rs = np.random.RandomState(21)
    sizes = rs.randint(2, 34, size=41).tolist()
    b, _ = recipe.build_graphs(sizes, K=7, species_per_graph=rs.randint(1, 5, size=41).tolist(), seed=22)
    g = torch.Generator().manual_seed(15)
    N, E = b.num_nodes, b.edge_index.shape[1]
    assert E % 128 != 0 and N % 8 != 0
    inputs = {"x": torch.randn(N, 128, generator=g), "edge_index": b.edge_index,
              "edge_attr": torch.randn(E, 128, generator=g), "x_0": torch.randn(N, 128, generator=g)}
    call = lambda m, i: m(i["x"], i["edge_index"], i["edge_attr"], i["x_0"])
    _compare_with_oracle(lambda: P.GATConvNodes(128, 128, 128, 3, concat=True),
                         lambda: O.GATConvNodes(128, 128, 128, 3, concat=True), inputs, call)


def test_irregular_degrees_fast_widths_vs_oracle():
    """An arbitrary directed graph at the benchmark widths: atoms without incoming edges, atoms without outgoing edges,
    a hub with 300 incoming edges, E = 3001 (no tile size divides it).  The backward's rebuilt-gZ kernels walk
    destination segments (edge_seg_bwd, edge_ge), fixed-size slot tiles (edge_gw) and source segments (edge_gj): empty
    segments, a segment longer than a workgroup's tile and clamped tails all occur here."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    rs = np.random.RandomState(77)
    N, E = 500, 3001
    src = rs.randint(0, 400, size=E)                      # atoms 400..499 never send
    dst = rs.randint(100, 500, size=E)                    # atoms 0..99 never receive
    dst[:300] = 123                                       # a hub
    order = np.argsort(src, kind="stable")                # (source-major, like the reference's batches)
    ei = torch.from_numpy(np.stack([src[order], dst[order]])).long()
    g = torch.Generator().manual_seed(78)
    inputs = {"x": torch.randn(N, 128, generator=g), "edge_index": ei,
              "edge_attr": torch.randn(E, 128, generator=g), "x_0": torch.randn(N, 128, generator=g)}
    call = lambda m, i: m(i["x"], i["edge_index"], i["edge_attr"], i["x_0"])
    _compare_with_oracle(lambda: P.GATConvNodes(128, 128, 128, 3, concat=True),
                         lambda: O.GATConvNodes(128, 128, 128, 3, concat=True), inputs, call)


def _ragged_k24(n_crystals, seed):
    rs = np.random.RandomState(seed)
    sizes = rs.randint(2, 41, size=n_crystals).tolist()
    return recipe.build_graphs(sizes, K=24, species_per_graph=rs.randint(1, 5, size=n_crystals).tolist(), seed=seed + 1)


def test_lightning_default_layer_vs_oracle():
    """The layer shape the reference harness ships by default (lightning_module.py:427-593): C = Ce = 128, msg_heads = 5,
    max_nbr = 24, vector_attention = True, on ragged crystals (2..40 atoms) -- at width 128, i.e. on the fast routes
    (operand-split first layer, per-head second layers, one-kernel channel-wise softmax + weighted sum)."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b, _ = _ragged_k24(14, 51)
    g = torch.Generator().manual_seed(52)
    N, E = b.num_nodes, b.edge_index.shape[1]
    inputs = {"x": torch.randn(N, 128, generator=g), "edge_index": b.edge_index,
              "edge_attr": torch.randn(E, 128, generator=g), "x_0": torch.randn(N, 128, generator=g)}
    call = lambda m, i: m(i["x"], i["edge_index"], i["edge_attr"], i["x_0"])
    _compare_with_oracle(lambda: P.GATConvNodes(128, 128, 128, 5, concat=True, vector_attention=True),
                         lambda: O.GATConvNodes(128, 128, 128, 5, concat=True, vector_attention=True), inputs, call)


def test_lightning_default_stack_vs_oracle():
    """The whole network as the reference harness builds it by default (lightning_module.py:165-176 with the argparse
    defaults): CGAtNet(200, 128, n_graph=5, rezero=True, mean_pooling=False (concat), neighbor_number=24, msg_heads=5,
    update_edges=True, vector_attention=True, global_vector_attention=True, n_graph_roost=3), ragged crystals."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b, roost = _ragged_k24(8, 61)
    inputs = {"x": b.x, "edge_index": b.edge_index, "edge_attr": b.edge_attr, "batch": b.batch,
              "r0": roost[0], "r1": roost[1], "r2": roost[2], "r3": roost[3], "r4": roost[4]}

    def call(m, i):
        bb = recipe.GraphBatch(i["x"], i["edge_index"], i["edge_attr"], i["batch"])
        return m(bb, (t for t in (i["r0"], i["r1"], i["r2"], i["r3"], i["r4"])))
    kw = dict(rezero=True, mean_pooling=False, neighbor_number=24, msg_heads=5, update_edges=True, vector_attention=True,
              global_vector_attention=True, n_graph_roost=3)
    _compare_with_oracle(lambda: P.CGAtNet(200, 128, 5, **kw), lambda: O.CGAtNet(200, 128, 5, **kw), inputs, call)


def test_full_stack_vs_oracle_random_init():
    """Config 3 shape (msg_heads=3, 4 layers, 200-d embeddings) on 40 crystals, random init."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b, roost = P.synthetic_batch(40, 20, 12, seed=8)
    inputs = {"x": b.x, "edge_index": b.edge_index, "edge_attr": b.edge_attr, "batch": b.batch,
              "r0": roost[0], "r1": roost[1], "r2": roost[2], "r3": roost[3], "r4": roost[4]}

    def call(m, i):
        bb = recipe.GraphBatch(i["x"], i["edge_index"], i["edge_attr"], i["batch"])
        return m(bb, (t for t in (i["r0"], i["r1"], i["r2"], i["r3"], i["r4"])))
    mk = lambda ns: (lambda: ns.CGAtNet(200, 128, 4, msg_heads=3, neighbor_number=12, update_edges=True))
    _compare_with_oracle(mk(P), mk(O), inputs, call)


def _report(lines):
    """Per-tensor audit lines (which tolerance term admitted the tensor): printed, and appended to
    gpurun_out/parity_report.txt when that directory exists (copied to profiles/ from there)."""
    import os
    text = "\n".join(lines)
    print(text)
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(d):
        with open(os.path.join(d, f"parity_report_{_mode()}.txt"), "a") as f:
            f.write(text + "\n")


# fixture -> (most tensors admitted by the noise term, by the zero floor) in the 24-bit arithmetic modes.  Measured in
# round 4 (f16x3c): net_mean 3 + 46 of 274 (the 46: the whole composition branch and the crystal pooling's attention
# network, whose true gradients are ~1e-15 of the case's largest in this fixture, and the four exactly-zero MH_A output
# biases), nodes_first0 0 + 1 of 52, nodes_first1 3 + 1 of 50; the bounds leave room for borderline roundings only.
# Round 6: the crystal pooling's backward centres on the weighted sum divided by the rounded coefficients' own sum
# (csrc/segment.hip), so the logit gradients of a crystal add up to zero as the exact ones do: 40 of the 46 tensors that
# only the floor admitted before are now within 4 x the oracle's own fp32 deviation (net_mean: 228 plain + 40 noise + 6
# floor of 274).  The terms are tried in the order 1e-4 |ref|, noise, floor -- a tensor that moves from the floor to the
# noise term has a SMALLER error -- so the bounds are cumulative: floor <= lim[1], noise + floor <= lim[0] + lim[1].
_ADMIT_LIMITS = {"net_mean": (6, 48), "nodes_first0": (2, 2), "nodes_first1": (6, 2)}


@pytest.mark.parametrize("cname", _BASE_NAMES)
def test_golden_base_full_gradients_vs_oracle(cname):
    """The BASELINE-shaped fixtures store parameter gradients above PROBE_ABOVE elements as a 12-number probe (the
    16 512 x 128 head weights would be 8 MB each), and a probe bounds the largest element error only from below.
    Here every such gradient is compared ELEMENT BY ELEMENT with the oracle run on the same recipe case (the oracle
    itself is pinned to the reference by the same fixtures, tests/test_oracle_golden.py), with the activation derivative
    patterns of the HIP run forced on the oracle (see _compare_with_oracle).  These cases use closed-form sin-pattern
    parameters, cancellation-heavy by construction: the oracle's own fp32 run is 1e-5 .. 4e-5 of |ref| away from its
    fp64 run on many tensors, so the criterion keeps the noise term,
        err <= max(1e-4 |ref|, NOISE_MULT * nf, 1e-6 * largest gradient of the case)        NOISE_MULT = 4
    and the report lists for every tensor err / |ref|, err / nf, (hip - ref64) / nf and the term that admitted it."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    pc = recipe.base_cases(product_ns())[cname]
    oc = recipe.base_cases(oracle_ns())[cname]
    held = {}

    def rec(mod):
        cm = P.debug.record_masks(mod)
        held["masks"] = cm.masks
        return cm
    yp, gp, _ = recipe.run_case(pc, torch.float32, device="cuda:0", ctx=rec)
    forced_ctxs = []

    def forced(mod):
        forced_ctxs.append(O.forced_masks(mod, held["masks"]))
        return forced_ctxs[-1]
    yo, go, _ = recipe.run_case(oc, torch.float32, device="cpu", ctx=forced)
    yo64, go64, _ = recipe.run_case(oc, torch.float64, device="cpu", ctx=forced)
    assert maxnorm_rel(yp.detach().cpu().numpy(), yo64.detach().numpy()) <= TOL
    for fc in forced_ctxs:        # the forced patterns only moved pre-activations that are zero at fp32 resolution
        assert fc.stats["max_rel_z"] <= MAX_FORCED_REL_Z, fc.stats
    case_scale = max(float(g.abs().max()) for g in go64.values() if g is not None)
    lines = [f"[{cname}] mode {_mode()} (derivative patterns forced)",
             "  tensor | err/|ref| | err/nf | (hip-ref64)/nf | nf/|ref| | admitted by"]
    failures, admitted = [], {}
    for name, g64 in go64.items():
        if g64 is None:
            assert gp[name] is None or float(gp[name].abs().max()) == 0.0, name
            continue
        a = gp[name].detach().cpu().double()
        ref_max = float(g64.abs().max())
        nf = float((go[name].double() - g64).abs().max())
        err = float((a - go[name].double()).abs().max())
        err64 = float((a - g64).abs().max())
        terms = {"1e-4*|ref|": TOL * ref_max, f"{NOISE_MULT:g}*oracle_fp32_noise": NOISE_MULT * nf}
        if floor_open(ref_max, case_scale):              # numerically zero (see NUM_ZERO): the zero-gradient floor
            terms["1e-6*case_scale (|ref| <= 1e-7 case_scale)"] = ZERO_FLOOR * case_scale
        ok = [k for k, v in terms.items() if err <= v]
        admitted[ok[0] if ok else "NONE"] = admitted.get(ok[0] if ok else "NONE", 0) + 1
        lines.append(f"  {name:70s} {err / max(ref_max, 1e-300):.2e} {err / max(nf, 1e-300):8.2f} "
                     f"{err64 / max(nf, 1e-300):8.2f} {nf / max(ref_max, 1e-300):.2e}  {ok[0] if ok else 'NONE'}")
        if not ok:
            failures.append(f"{name}: err {err:.3e} > " + ", ".join(f"{k}={v:.3e}" for k, v in terms.items()))
    lines.append(f"  ADMITTED-BY {cname} {_mode()}: " + ", ".join(f"{k} = {v}" for k, v in sorted(admitted.items())))
    _report(lines)
    assert not failures, "\n".join(failures)
    # the number of tensors that need the noise term or the zero floor must not grow silently: bounds per fixture,
    # measured in round 4 (profiles/r04_parity_attribution.txt) with two tensors of slack for borderline roundings
    lim = _ADMIT_LIMITS.get(cname) if _mode() in ("f16x3c", "bf16x6") else None
    if lim is not None:
        n_noise = sum(v for k, v in admitted.items() if "noise" in k)
        n_floor = sum(v for k, v in admitted.items() if "case_scale" in k)
        assert n_floor <= lim[1] and n_noise + n_floor <= lim[0] + lim[1], (cname, admitted, lim)


def test_config1_full_size_forward_vs_oracle():
    """BASELINE configs[0] / [1] at FULL size: 1000 crystals x 20 atoms x 12 neighbours (N = 20 000, E = 240 000), one
    GATConvNodes layer forward (C = Ce = 128, H = 3, non-first, random init): the reference-equivalent CPU path
    (oracle, no_grad) against the HIP layer on the same tensors, max-norm relative <= 1e-4."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b, _ = P.synthetic_batch(1000, 20, 12, seed=0)
    g = torch.Generator().manual_seed(1000)
    N, E = b.num_nodes, b.edge_index.shape[1]
    assert (N, E) == (20000, 240000)
    x, e, x0 = (torch.randn(n, 128, generator=g) for n in (N, E, N))
    torch.manual_seed(1)
    om = O.GATConvNodes(128, 128, 128, 3, concat=True)
    pm = P.GATConvNodes(128, 128, 128, 3, concat=True)
    pm.load_state_dict(om.state_dict())
    pm = pm.to("cuda:0")
    with torch.no_grad():
        yo = om(x, b.edge_index, e, x0)
        yp = pm(x.to("cuda:0"), b.edge_index.to("cuda:0"), e.to("cuda:0"), x0.to("cuda:0"))
    err = maxnorm_rel(yp.cpu().numpy(), yo.numpy())
    _report([f"[config1 full size] out max-norm rel err vs oracle fp32: {err:.2e}"])
    assert err <= TOL


def test_dynamic_range_inside_one_batch():
    """Crystals whose cotangents differ by 1e6 in ONE batch: the f16x3 kernels scale gZ by ONE power of two per tensor
    (mfma_bf16.h), so the crystals with the small cotangents sit far down the fp16 range of that operand.  Their
    gradients must still be right RELATIVE TO THEIR OWN magnitude: per-crystal max-norm relative error of grad x and
    grad edge_attr vs the oracle's fp64 run."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    G, A, K = 48, 20, 12
    b, _ = P.synthetic_batch(G, A, K, seed=31)
    g = torch.Generator().manual_seed(32)
    N, E = b.num_nodes, b.edge_index.shape[1]
    x, e, x0 = (torch.randn(n, 128, generator=g) for n in (N, E, N))
    scale = torch.logspace(-3, 3, G).repeat_interleave(A).view(-1, 1)       # cotangent scale per crystal: 1e-3 .. 1e3
    cot = torch.randn(N, 128, generator=g) * scale
    torch.manual_seed(1)
    om = O.GATConvNodes(128, 128, 128, 3, concat=True).double()
    pm = P.GATConvNodes(128, 128, 128, 3, concat=True)
    pm.load_state_dict({k: v.float() for k, v in om.state_dict().items()})
    pm = pm.to("cuda:0")
    xp, ep = x.to("cuda:0").requires_grad_(True), e.to("cuda:0").requires_grad_(True)
    with P.debug.record_masks(pm) as masks:      # the LeakyReLU derivative pattern of the HIP backward (C ABI debug entry)
        yp = pm(xp, b.edge_index.to("cuda:0"), ep, x0.to("cuda:0"))
    gxp, gep = torch.autograd.grad((yp * cot.to("cuda:0")).sum(), [xp, ep])
    with O.forced_masks(om, masks) as forced:    # ... forced on the oracle: no flip allowance below
        xo, eo = x.double().requires_grad_(True), e.double().requires_grad_(True)
        gxo, geo = torch.autograd.grad((om(xo, b.edge_index, eo, x0.double()) * cot.double()).sum(), [xo, eo])
    assert forced.stats["max_rel_z"] <= MAX_FORCED_REL_Z, forced.stats
    worst = [f"  derivative pattern forced in {forced.stats['layers']} layers; {forced.stats['disagree']} of "
             f"{forced.stats['elements']} pre-activations on the other side of 0 in the oracle's fp64 run "
             f"(largest |z| / max|z| among them {forced.stats['max_rel_z']:.1e})"]
    for name, got, ref, per in (("grad_x", gxp, gxo, A), ("grad_edge_attr", gep, geo, A * K)):
        got, ref = got.cpu().double().view(G, per, -1), ref.view(G, per, -1)
        err = (got - ref).abs().amax(dim=(1, 2))
        ref_max = ref.abs().amax(dim=(1, 2))
        rel = err / ref_max
        ok = err <= TOL * ref_max                            # flat, per crystal, relative to the crystal's own gradient
        third = G // 3
        lo, hi = rel[:third].median(), rel[-third:].median()
        worst.append(f"  {name}: per-crystal rel err: median {float(rel.median()):.2e}, max {float(rel.max()):.2e}; third "
                     f"with the smallest cotangents: median {float(lo):.2e}, third with the largest: {float(hi):.2e}")
        bad = (~ok).nonzero().flatten().tolist()
        assert not bad, (name, [(i, f"err {float(err[i]):.3e} ref {float(ref_max[i]):.3e}") for i in bad])
        # the crystals with the SMALLEST cotangents (1e-3 .. 1e-1 of a batch whose largest is 1e3) are as accurate as
        # the largest ones: the per-tensor fp16 scales do not cost them their relative accuracy
        assert float(lo) <= max(1e-5, 4 * float(hi)), (name, lo, hi)
    _report([f"[dynamic range 1e6 inside one batch] mode {_mode()}"] + worst)


@pytest.mark.parametrize("overlap", [True, False])
def test_determinism_bitwise(overlap):
    """No atomics on the data path: two runs give bit-identical outputs and gradients, with the
    weight-gradient contractions on the side stream (default) and in serial order."""
    import cgat_amd as P
    from cgat_amd import ops
    was = ops.get_overlap_wgrad()                       # the raw tri-state, so that the per-mode default survives
    ops.set_overlap_wgrad(overlap)
    try:
        _determinism_body(P)
    finally:
        ops.set_overlap_wgrad(was)


def test_poisoned_scratch_changes_nothing():
    """No kernel reads workspace or library-sized scratch memory it has not written: the 2-layer network's step with every
    such buffer pre-filled with 0xFF bytes (NaN patterns), 0x7F and 0x00 gives bit-identical outputs and gradients.  (In a
    replayed hipGraph these buffers hold whatever a later operator of the previous replay left in the reused block.)"""
    import cgat_amd as P
    from cgat_amd import ops
    dev = torch.device("cuda:0")
    b, roost = P.synthetic_batch(64, 20, 12, seed=4)
    b = b.to(dev)
    roost = tuple(t.to(dev) for t in roost)
    torch.manual_seed(1)
    net = P.CGAtNet(200, 128, 2, msg_heads=3, neighbor_number=12, update_edges=True).to(dev)
    params = list(net.parameters())
    names = ["out"] + [n for n, _ in net.named_parameters()]

    def step():
        for p in params:
            p.grad = None
        out = net(b, roost)
        (out[:, 0] - b.y).abs().mean().backward()
        return out
    out = step()
    torch.cuda.synchronize()
    want = [out.detach().clone()] + [None if p.grad is None else p.grad.clone() for p in params]
    orig_ws, orig_sc = ops.workspace, ops._scratch
    try:
        for pat in (0xFF, 0x7F, 0x00):
            def ws(nbytes, device, pat=pat):
                return torch.empty(int(nbytes) + 4096, dtype=torch.uint8, device=device).fill_(pat)

            def sc(numel, dtype, device, pat=pat):
                t = orig_sc(numel, dtype, device)
                t.view(torch.uint8).fill_(pat)
                return t
            ops.workspace, ops._scratch = ws, sc
            y = step()
            torch.cuda.synchronize()
            got = [y] + [p.grad for p in params]
            bad = [n for n, a, w in zip(names, got, want) if a is not None and w is not None and not torch.equal(a, w)]
            assert not bad, f"pattern {pat:#x}: {len(bad)} tensors changed, e.g. {bad[:4]}"
    finally:
        ops.workspace, ops._scratch = orig_ws, orig_sc


def test_side_stream_equals_serial():
    """The overlapped backward computes the same gradients as the serial one (only the row split of the
    weight-gradient sums differs): 1e-5 max-norm relative on every gradient."""
    import cgat_amd as P
    from cgat_amd import ops
    # 6 000 atoms: below the row count at which the overlapped backward prepares the dT operands early on the side
    # stream; 16 400 atoms: above it
    for crystals in (300, 820):
        b, _ = P.synthetic_batch(crystals, 20, 12, seed=4)
        dev = "cuda:0"
        torch.manual_seed(3)
        m = P.GATConvNodes(128, 128, 128, 3, concat=True).to(dev)
        g = torch.Generator().manual_seed(9)
        N, E = b.num_nodes, b.edge_index.shape[1]
        assert (N >= 16384) == (crystals == 820)
        x, e, x0 = (torch.randn(s, 128, generator=g).to(dev) for s in (N, E, N))
        ei = b.edge_index.to(dev)
        was = ops.get_overlap_wgrad()                   # the raw tri-state, so that the per-mode default survives
        res = {}
        try:
            for mode in (True, False):
                ops.set_overlap_wgrad(mode)
                xx, ee = x.clone().requires_grad_(True), e.clone().requires_grad_(True)
                y = m(xx, ei, ee, x0)
                gr = torch.autograd.grad(y.square().sum(), [xx, ee] + list(m.parameters()))
                res[mode] = [y.detach().cpu().numpy()] + [t.detach().cpu().numpy() for t in gr]
        finally:
            ops.set_overlap_wgrad(was)
        for a, bb in zip(res[True], res[False]):
            assert maxnorm_rel(a, bb) <= 1e-5


def _determinism_body(P):
    b, _ = P.synthetic_batch(200, 20, 12, seed=2)
    dev = "cuda:0"
    torch.manual_seed(1)
    m = P.GATConvNodes(128, 128, 128, 3, concat=True).to(dev)
    g = torch.Generator().manual_seed(6)
    N, E = b.num_nodes, b.edge_index.shape[1]
    x, e, x0 = (torch.randn(s, 128, generator=g).to(dev) for s in (N, E, N))
    ei = b.edge_index.to(dev)
    outs = []
    for _ in range(2):
        xx, ee = x.clone().requires_grad_(True), e.clone().requires_grad_(True)
        y = m(xx, ei, ee, x0)
        gr = torch.autograd.grad(y.square().sum(), [xx, ee] + list(m.parameters()))
        outs.append([y.detach()] + [t.detach() for t in gr])
    for a, bb in zip(*outs):
        assert torch.equal(a, bb)


def test_million_edge_properties():
    """BASELINE size (G=4167 -> N=83 340, E=1 000 080): properties that need no oracle run.
    (a) permutation equivariance: relabelling the edges (same multiset) leaves the node output
        unchanged up to summation order; (b) graph locality: crystals are independent, so the
        first 50 crystals evaluated alone give the same rows as inside the big batch."""
    import cgat_amd as P
    dev = "cuda:0"
    b, _ = P.synthetic_batch(4167, 20, 12, seed=0)
    N, E = b.num_nodes, b.edge_index.shape[1]
    assert E == 1000080
    torch.manual_seed(1)
    m = P.GATConvNodes(128, 128, 128, 3, concat=True).to(dev)
    g = torch.Generator().manual_seed(7)
    x, e, x0 = (torch.randn(s, 128, generator=g).to(dev) for s in (N, E, N))
    ei = b.edge_index.to(dev)
    with torch.no_grad():
        y = m(x, ei, e, x0)
        perm = torch.randperm(E, generator=g).to(dev)
        y_perm = m(x, ei[:, perm].contiguous(), e[perm].contiguous(), x0)
        n_sub, e_sub = 50 * 20, 50 * 20 * 12
        y_sub = m(x[:n_sub].contiguous(), ei[:, :e_sub].contiguous(), e[:e_sub].contiguous(), x0[:n_sub].contiguous())
    assert torch.isfinite(y).all()
    assert maxnorm_rel(y_perm.cpu().numpy(), y.cpu().numpy()) <= 1e-5
    assert maxnorm_rel(y_sub.cpu().numpy(), y[:n_sub].cpu().numpy()) <= 1e-5


# Gradients with the other crystals replaced: the same terms in the same summation trees, exact zeros elsewhere; only an
# operand scale taken over a whole tensor (a power of two from its maximum) can differ between the two batches
STACK_LOCALITY_TOL = 1e-5


def test_million_edge_stack_fwd_bwd_locality():
    """BASELINE configs[2] at FULL size -- CGAtNet(200, 128, 4 layers, 3 heads), forward + backward, E = 1 000 080 --
    through properties that need no oracle run.  Crystals are independent (no edge and no composition pair crosses
    them).  With a cotangent that is non-zero on the first 50 crystals only:
      (a) REPLACING the other 4 117 crystals (new atoms, shells and compositions, same sizes) changes neither the 50
          outputs, nor the gradient of their inputs, nor ANY of the 307 parameter gradients -- the same kernels sum the
          same terms in the same trees, the other crystals contribute exact zeros; what may move is an operand scale
          taken over a whole tensor (a few 1e-7);
      (b) nothing leaks: the input gradient of the other crystals is exactly zero;
      (c) the 50 outputs equal those of the 50 crystals evaluated ALONE (other kernels at that row count: 1e-5).
    (The gradients of (c) are NOT compared: at 1 000 rows the dense layers run on other kernels, a pre-activation within
    an ulp of zero lands on the other side in one of the two evaluations, and a LeakyReLU / ReLU derivative that flips
    moves its row's gradients by 1e-3 .. 1e-2 -- the oracle comparisons force the derivative pattern for that reason.)"""
    import cgat_amd as P
    dev = "cuda:0"
    G, A, K, GS = 4167, 20, 12, 50
    b, roost = P.synthetic_batch(G, A, K, seed=0)
    assert b.edge_index.shape[1] == 1000080
    torch.manual_seed(1)
    net = P.CGAtNet(200, 128, 4, msg_heads=3, neighbor_number=K, update_edges=True).to(dev)
    params = dict(net.named_parameters())
    cot = torch.randn(GS, 2, generator=torch.Generator().manual_seed(3)).to(dev)

    def run(bb, rr):
        bb = bb.to(dev)
        rr = tuple(t.to(dev) for t in rr)
        bb.x.requires_grad_(True)
        out = net(bb, rr)
        g = torch.autograd.grad((out[:GS] * cot).sum(), [bb.x] + list(params.values()), allow_unused=True)
        return out[:GS].detach(), g[0].detach(), [None if t is None else t.detach() for t in g[1:]]

    y_a, gx_a, gp_a = run(b, roost)
    # atoms, edges and composition rows of a crystal are contiguous blocks
    n_sub, e_sub = GS * A, GS * A * K
    w, fea, sidx, nidx, cidx = roost
    nc_sub = int((cidx < GS).sum())
    mc_sub = int((sidx < nc_sub).sum())
    # (a) the same batch with every OTHER crystal replaced
    b2, roost2 = P.synthetic_batch(G, A, K, seed=77)
    x_b = torch.cat([b.x[:n_sub], b2.x[n_sub:]])
    ea_b = torch.cat([b.edge_attr[:e_sub], b2.edge_attr[e_sub:]])
    ei_b = torch.cat([b.edge_index[:, :e_sub], b2.edge_index[:, e_sub:]], dim=1)
    bb = P.GraphBatch(x_b, ei_b, ea_b, b.batch.clone(), b.y.clone(), num_graphs=G)
    w2, fea2 = w.clone(), fea.clone()
    g2 = torch.Generator().manual_seed(78)
    fea2[nc_sub:] = fea[nc_sub:][torch.randperm(fea.shape[0] - nc_sub, generator=g2)]     # other elements, same layout
    y_b, gx_b, gp_b = run(bb, (w2, fea2, sidx, nidx, cidx))
    assert torch.isfinite(y_a).all()
    err_y = maxnorm_rel(y_b.cpu().numpy(), y_a.cpu().numpy())
    err_gx = maxnorm_rel(gx_b[:n_sub].cpu().numpy(), gx_a[:n_sub].cpu().numpy())
    leak = max(float(gx_a[n_sub:].abs().max()), float(gx_b[n_sub:].abs().max()))
    worst, worst_name, bad = 0.0, "", []
    case_scale = max(float(c.abs().max()) for c in gp_a if c is not None)
    for name, a_, c in zip(params, gp_b, gp_a):
        assert (a_ is None) == (c is None), name
        if a_ is None:
            continue
        ref_max = float(c.abs().max())
        abs_err = float((a_ - c).abs().max())
        if ref_max <= NUM_ZERO * case_scale:       # zero in exact arithmetic (softmax shift invariance): rounding noise
            if abs_err > ZERO_FLOOR * case_scale:
                bad.append((name, abs_err, ref_max))
            continue
        if abs_err / ref_max > worst:
            worst, worst_name = abs_err / ref_max, name
        if abs_err > STACK_LOCALITY_TOL * ref_max:
            bad.append((name, abs_err / ref_max))
    # (c) the 50 crystals alone: forward
    sub = P.GraphBatch(b.x[:n_sub].clone(), b.edge_index[:, :e_sub].clone(), b.edge_attr[:e_sub].clone(),
                       b.batch[:n_sub].clone(), b.y[:GS].clone(), num_graphs=GS)
    sub_roost = tuple(t.to(dev) for t in (w[:nc_sub].clone(), fea[:nc_sub].clone(), sidx[:mc_sub].clone(),
                                          nidx[:mc_sub].clone(), cidx[:nc_sub].clone()))
    with torch.no_grad():
        y_sub = net(sub.to(dev), sub_roost)
    err_alone = maxnorm_rel(y_sub.cpu().numpy(), y_a.cpu().numpy())
    _report([f"[4-layer stack fwd+bwd locality at E = 1 000 080] mode {_mode()}: 50 crystals, the other 4 117 replaced: "
             f"out {err_y:.2e}, grad x {err_gx:.2e} (largest entry outside the 50 crystals {leak:.1e}), {len(params)} "
             f"parameter gradients, worst max-norm rel difference {worst:.2e} ({worst_name}); the 50 crystals alone: "
             f"out {err_alone:.2e}"])
    assert err_y <= 1e-6 and err_gx <= STACK_LOCALITY_TOL and leak == 0.0 and err_alone <= 1e-5, (err_y, err_gx, leak, err_alone)
    assert not bad, bad


@pytest.mark.gpu
def test_beyond_int32_element_counts():
    """7000 crystals -> E = 1 680 000 edges, E x 1536 = 2.58e9 pre-activations (> 2^31 elements): the LAST 50
    crystals -- where a 32-bit offset would wrap -- give the same outputs and input gradients inside the big batch as
    evaluated alone (crystals are independent), forward and backward."""
    import cgat_amd as P
    dev = "cuda:0"
    G, A, K = 7000, 20, 12
    b, _ = P.synthetic_batch(G, A, K, seed=5)
    N, E = b.num_nodes, b.edge_index.shape[1]
    assert E * 1536 > 2 ** 31
    torch.manual_seed(1)
    m = P.GATConvNodes(128, 128, 128, 3, concat=True).to(dev)
    g = torch.Generator().manual_seed(8)
    x, e, x0 = (torch.randn(s, 128, generator=g).to(dev) for s in (N, E, N))
    ei = b.edge_index.to(dev)
    n0, e0 = (G - 50) * A, (G - 50) * A * K
    cot = torch.randn(50 * A, 128, generator=g).to(dev)

    def run(xs, eis, es, x0s, sl):
        xs, es = xs.clone().requires_grad_(True), es.clone().requires_grad_(True)
        with P.debug.record_masks(m) as masks:           # the LeakyReLU derivative pattern the backward will use
            y = m(xs, eis, es, x0s)
        gx, ge = torch.autograd.grad((y[sl] * cot).sum(), [xs, es])
        return y[sl].detach(), gx[sl].detach(), ge, masks

    y_big, gx_big, ge_big, mk_big = run(x, ei, e, x0, slice(n0, N))
    y_sub, gx_sub, ge_sub, mk_sub = run(x[n0:].contiguous(), (ei[:, e0:] - n0).contiguous(), e[e0:].contiguous(),
                                        x0[n0:].contiguous(), slice(0, 50 * A))
    assert torch.isfinite(y_big).all()
    assert maxnorm_rel(y_big.cpu().numpy(), y_sub.cpu().numpy()) <= 1e-5
    # The 1 000-atom batch runs its dense layers on other kernels than the 140 000-atom one (csrc/rowprog.hip below 2 048
    # rows): a pre-activation within an ulp of zero can land on the other side, and ONE flipped LeakyReLU derivative moves
    # its row's gradients by 1e-4 .. 1e-3 (measured in the f32 and f16x3 modes: 1-2 of 18 M entries; none in the 24-bit
    # modes).  With identical derivative patterns the gradients agree to 1e-5; with a handful of flips the comparison
    # still catches what this test is about -- a wrapped 32-bit offset is an O(1) error.
    flips = 0
    for k in mk_big:
        for a_, b_ in zip(mk_big[k], mk_sub[k]):
            flips += int((a_[-b_.shape[0]:] != b_).sum())
    assert flips <= 8, flips
    gtol = 1e-5 if flips == 0 else 5e-3
    assert maxnorm_rel(gx_big.cpu().numpy(), gx_sub.cpu().numpy()) <= gtol
    assert maxnorm_rel(ge_big[e0:].cpu().numpy(), ge_sub.cpu().numpy()) <= gtol
