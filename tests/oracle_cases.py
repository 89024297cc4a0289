"""The oracle comparisons of tests/test_hip_golden.py as importable pieces (tests only): the criterion
(compare_with_oracle, full_gradients_vs_oracle) and ONE table of the seeded cases it runs on,

    CASES[name]() -> (mk_prod, mk_orac, inputs, call)

so that a second runner -- tests/large_rows_worker.py, a child process with the small-row programs switched off -- runs
exactly the cases tests/test_hip_golden.py runs.  An entry is a builder, not the tuple itself: the graphs and inputs of
a case (up to 1 200 atoms with 14 400 edges) are built when the case runs, not when the table is imported.

Tolerance (north_star): max-norm relative <= 1e-4, fp32, per tensor -- outputs, input gradients and parameter gradients.
"""
import copy
import os
import types

import numpy as np
import torch

import recipe
from golden_util import NOISE_MULT, floor_open, maxnorm_rel

TOL = 1e-4
# largest |z| / max|z| of a pre-activation whose forced LeakyReLU / ReLU derivative may differ from the oracle's own
MAX_FORCED_REL_Z = 1e-5
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


def _mode():
    import cgat_amd as P
    return P.get_bilinear_mode()


def report(lines):
    """Per-tensor audit lines (which tolerance term admitted the tensor): printed, and appended to
    gpurun_out/parity_report.txt when that directory exists (copied to profiles/ from there)."""
    text = "\n".join(lines)
    print(text)
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(d):
        with open(os.path.join(d, f"parity_report_{_mode()}.txt"), "a") as f:
            f.write(text + "\n")


def compare_with_oracle(mk_prod, mk_orac, inputs, call, tol=TOL, label=None):
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
    report(lines)
    assert not failures, "\n".join(failures)
    return worst


# fixture -> (most tensors admitted by the noise term, by the zero floor) in the 24-bit arithmetic modes.  Measured in
# round 4 (f16x3c): net_mean 3 + 46 of 274 (the 46: the whole composition branch and the crystal pooling's attention
# network, whose true gradients are ~1e-15 of the case's largest in this fixture, and the four exactly-zero MH_A output
# biases), nodes_first0 0 + 1 of 52, nodes_first1 3 + 1 of 50; the bounds leave room for borderline roundings only.
# Round 6: the crystal pooling's backward centres on the weighted sum divided by the rounded coefficients' own sum
# (csrc/segment.hip), so the logit gradients of a crystal add up to zero as the exact ones do: 40 of the 46 tensors that
# only the floor admitted before are now within 4 x the oracle's own fp32 deviation (net_mean: 228 plain + 40 noise + 6
# floor of 274).  The terms are tried in the order 1e-4 |ref|, noise, floor -- a tensor that moves from the floor to the
# noise term has a SMALLER error -- so the bounds are cumulative: floor <= lim[1], noise + floor <= lim[0] + lim[1].
ADMIT_LIMITS = {"net_mean": (6, 48), "nodes_first0": (2, 2), "nodes_first1": (6, 2)}


def full_gradients_vs_oracle(cname):
    """One BASELINE-shaped recipe case (tests/golden/recipe.py base_cases), every gradient element by element against the
    oracle run on the same case: the body of tests/test_hip_golden.py::test_golden_base_full_gradients_vs_oracle, whose
    docstring states the criterion."""
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
    report(lines)
    assert not failures, "\n".join(failures)
    # the number of tensors that need the noise term or the zero floor must not grow silently: bounds per fixture,
    # measured in round 4 (profiles/r04_parity_attribution.txt) with two tensors of slack for borderline roundings
    lim = ADMIT_LIMITS.get(cname) if _mode() in ("f16x3c", "bf16x6") else None
    if lim is not None:
        n_noise = sum(v for k, v in admitted.items() if "noise" in k)
        n_floor = sum(v for k, v in admitted.items() if "case_scale" in k)
        assert n_floor <= lim[1] and n_noise + n_floor <= lim[0] + lim[1], (cname, admitted, lim)


# ---- the case table --------------------------------------------------------------------------------------------------
CASES = {}


def _case(name):
    def reg(build):
        CASES[name] = build
        return build
    return reg


def case(name):
    """(mk_prod, mk_orac, inputs, call) of one table entry, built now."""
    return CASES[name]()


def _layer_call(m, i):
    return m(i["x"], i["edge_index"], i["edge_attr"], i["x_0"])


def _layer_inputs(edge_index, N, E, C, Ce, seed):
    g = torch.Generator().manual_seed(seed)
    return {"x": torch.randn(N, C, generator=g), "edge_index": edge_index,
            "edge_attr": torch.randn(E, Ce, generator=g), "x_0": torch.randn(N, C, generator=g)}


def _layer_case(batch, C, Ce, H, seed, **kw):
    """GATConvNodes(C, C, Ce, H, concat=True, **kw) of both namespaces on the graph of `batch` with seeded features."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    inputs = _layer_inputs(batch.edge_index, batch.num_nodes, batch.edge_index.shape[1], C, Ce, seed)
    return (lambda: P.GATConvNodes(C, C, Ce, H, concat=True, **kw), lambda: O.GATConvNodes(C, C, Ce, H, concat=True, **kw),
            inputs, _layer_call)


def _stack_inputs(b, roost):
    return {"x": b.x, "edge_index": b.edge_index, "edge_attr": b.edge_attr, "batch": b.batch,
            "r0": roost[0], "r1": roost[1], "r2": roost[2], "r3": roost[3], "r4": roost[4]}


def _stack_call(m, i):
    bb = recipe.GraphBatch(i["x"], i["edge_index"], i["edge_attr"], i["batch"])
    return m(bb, (t for t in (i["r0"], i["r1"], i["r2"], i["r3"], i["r4"])))


def _ragged_k24(n_crystals, seed):
    rs = np.random.RandomState(seed)
    sizes = rs.randint(2, 41, size=n_crystals).tolist()
    return recipe.build_graphs(sizes, K=24, species_per_graph=rs.randint(1, 5, size=n_crystals).tolist(), seed=seed + 1)


def _random_init(first):
    def build():                 # test_nodes_layer_vs_oracle_random_init: 60 crystals (N = 1200, E = 14400)
        import cgat_amd as P
        b, _ = P.synthetic_batch(60, 20, 12, seed=3)
        return _layer_case(b, 128, 128, 3, 4, first=first)
    return build


for _first in (True, False):
    CASES[f"nodes_random_init_first{int(_first)}"] = _random_init(_first)


def _heads(heads):
    def build():                 # test_nodes_layer_other_head_counts_vs_oracle
        import cgat_amd as P
        b, _ = P.synthetic_batch(40, 20, 12, seed=5)
        return _layer_case(b, 128, 128, heads, 6)
    return build


for _h in (1, 5):
    CASES[f"nodes_heads{_h}"] = _heads(_h)


def width_case_name(C, vector):
    return f"nodes_width{C}" + ("_vector" if vector else "")


def _width(C, vector):
    def build():                 # test_nodes_layer_other_widths_vs_oracle
        import cgat_amd as P
        b, _ = P.synthetic_batch(30, 20, 12, seed=11)
        return _layer_case(b, C, C, 3, 12, vector_attention=vector)
    return build


for _C, _vec in ((64, False), (96, False), (64, True), (40, False)):
    CASES[width_case_name(_C, _vec)] = _width(_C, _vec)


@_case("single_predicted_layer")
def _single_predicted_layer():   # test_single_predicted_layer_vs_oracle
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
    return Prod, Orac, inputs, lambda m, i: m(i["h0"], i["v"])


@_case("vector_attention_layer")
def _vector_attention_layer():   # test_vector_attention_layer_vs_oracle_random_init
    import cgat_amd as P
    b, _ = P.synthetic_batch(60, 20, 12, seed=3)
    return _layer_case(b, 128, 128, 3, 4, vector_attention=True)


@_case("ragged_k24")
def _ragged_graphs():            # test_ragged_graphs_vs_oracle
    rs = np.random.RandomState(11)
    sizes = rs.randint(2, 41, size=30).tolist()
    b, _ = recipe.build_graphs(sizes, K=24, species_per_graph=rs.randint(1, 5, size=30).tolist(), seed=12)
    return _layer_case(b, 64, 32, 5, 5)


@_case("ragged_fast_widths")
def _ragged_fast_widths():       # test_ragged_graphs_fast_widths_vs_oracle
    rs = np.random.RandomState(21)
    sizes = rs.randint(2, 34, size=41).tolist()
    b, _ = recipe.build_graphs(sizes, K=7, species_per_graph=rs.randint(1, 5, size=41).tolist(), seed=22)
    N, E = b.num_nodes, b.edge_index.shape[1]
    assert E % 128 != 0 and N % 8 != 0
    return _layer_case(b, 128, 128, 3, 15)


@_case("irregular_degrees")
def _irregular_degrees():        # test_irregular_degrees_fast_widths_vs_oracle
    import cgat_amd as P
    from oracle import cgat_oracle as O
    rs = np.random.RandomState(77)
    N, E = 500, 3001
    src = rs.randint(0, 400, size=E)                      # atoms 400..499 never send
    dst = rs.randint(100, 500, size=E)                    # atoms 0..99 never receive
    dst[:300] = 123                                       # a hub
    order = np.argsort(src, kind="stable")                # (source-major, like the reference's batches)
    ei = torch.from_numpy(np.stack([src[order], dst[order]])).long()
    inputs = _layer_inputs(ei, N, E, 128, 128, 78)
    return (lambda: P.GATConvNodes(128, 128, 128, 3, concat=True), lambda: O.GATConvNodes(128, 128, 128, 3, concat=True),
            inputs, _layer_call)


@_case("lightning_default_layer")
def _lightning_default_layer():  # test_lightning_default_layer_vs_oracle
    b, _ = _ragged_k24(14, 51)
    return _layer_case(b, 128, 128, 5, 52, vector_attention=True)


@_case("lightning_default_stack")
def _lightning_default_stack():  # test_lightning_default_stack_vs_oracle
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b, roost = _ragged_k24(8, 61)
    kw = dict(rezero=True, mean_pooling=False, neighbor_number=24, msg_heads=5, update_edges=True, vector_attention=True,
              global_vector_attention=True, n_graph_roost=3)
    return (lambda: P.CGAtNet(200, 128, 5, **kw), lambda: O.CGAtNet(200, 128, 5, **kw), _stack_inputs(b, roost),
            _stack_call)


@_case("full_stack_config3")
def _full_stack_config3():       # test_full_stack_vs_oracle_random_init
    import cgat_amd as P
    from oracle import cgat_oracle as O
    b, roost = P.synthetic_batch(40, 20, 12, seed=8)
    mk = lambda ns: (lambda: ns.CGAtNet(200, 128, 4, msg_heads=3, neighbor_number=12, update_edges=True))
    return mk(P), mk(O), _stack_inputs(b, roost), _stack_call


def run_product_only(mk_prod, inputs, call):
    """The product's forward and backward of a table case with no oracle beside it (seeded default initialisation, the
    cotangent of compare_with_oracle): for checks of WHAT a case launches."""
    torch.manual_seed(1)
    pm = mk_prod().to("cuda:0")
    pin = {}
    for k, v in inputs.items():
        if torch.is_tensor(v):
            v = v.to("cuda:0")
            if v.is_floating_point():
                v = v.clone().requires_grad_(True)
        pin[k] = v
    y = call(pm, pin)
    cot = torch.randn(y.shape, generator=torch.Generator().manual_seed(9)).to("cuda:0")
    leaves = [v for v in pin.values() if torch.is_tensor(v) and v.requires_grad]
    torch.autograd.grad((y * cot).sum(), leaves + list(pm.parameters()), allow_unused=True)
    torch.cuda.synchronize()
