"""The bit form of the scalar-attention layer's saved buffer (csrc/layers.hip attn_z_form).

Where the training forward runs its 256-row per-edge kernel in fp32 storage and the backward rebuilds gZ with the bit-plane
form of grad W_e, the forward stores no attention pre-activations Z_A: their columns of the saved buffer hold the
attention halves of the two per-node projections and one sign bit per element.  The backward takes the signs from the
bits, and forms grad MH_A.fc_out.weight -- the only consumer of the VALUES -- from LeakyReLU(z) = d z and
z = W_e e + Pi + Pj:
    grad wA[h, c] = sum_k W_e[(h, c), k] U[(h, c), k]  +  sum_t g_a[t, h] d (Pi[dst_t] + Pj[src_t]),
with U the column sums grad W_e's reducer already holds.  Everything else keeps its bits; that one gradient is re-rounded.

A/B is always edge storage "f32" (the bit form where it is taken) against "f32+za" (the attention pre-activations stored
at every shape) on identical inputs and weights.  The base shape is the smallest that takes the form: 136 crystals x 20
atoms x 12 neighbours = 2 720 atoms, 32 640 edges = 128 row tiles of 256.  The yardstick of the re-rounded gradient is the
oracle in fp64 (run on the GPU), never one form against the other alone: the figures of a run on an MI355X are in
tests/golden/attn_bit_form_error.json (`python tests/test_attn_bit_form.py --record FILE`).
"""
import ctypes as C
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "golden", "attn_bit_form_error.json")
MODE = "f16x3c"
WA = "param:MH_A.fc_out.weight"
AGREE = 1e-5        # the project's bound for a change of form (tests/test_chunked.py::test_rebuilt_gz_equals_stored_gz)
MARGIN = 1.25       # ... and the margin of the bit-plane tests against fp64
BASE = (136, 20, 12)
SEEDS = (0, 1, 2)
HEADS = (3, 5)


class _modes:
    def __init__(self, mode, storage):
        self.want = (mode, storage)

    def __enter__(self):
        from cgat_amd import ops
        self.was = (ops.get_bilinear_mode(), ops.get_edge_storage())
        ops.set_bilinear_mode(self.want[0])
        ops.set_edge_storage(self.want[1])

    def __exit__(self, *exc):
        from cgat_amd import ops
        ops.set_bilinear_mode(self.was[0])
        ops.set_edge_storage(self.was[1])


def _query(N, E, H=3, Hd=256, mode=MODE, storage="f32"):
    from cgat_amd import debug
    with _modes(mode, storage):
        return debug.nodes_attention_bit_form(N, E, 128, 128, H, Hd)


# ---- 1. the query (host only) ----------------------------------------------------------------------------------------
def test_query_host():
    assert _query(2720, 32640) and _query(2720, 32640, H=5)           # the base shape: 128 row tiles
    assert _query(83340, 1000080)                                      # the benchmark shape
    assert _query(2720, 32640, mode="bf16x6")                          # the other 24-bit mode
    assert not _query(2700, 32384)                                     # 127 row tiles: the few-row form of the forward
    for mode, storage in (("f16x3", "f32"), ("f32", "f32"), (MODE, "bf16"), (MODE, "f32+gz"), (MODE, "f32+za"),
                          (MODE, "bf16-mma")):
        assert not _query(83340, 1000080, mode=mode, storage=storage), (mode, storage)
    assert not _query(83340, 1000080, Hd=128)
    # the holes must exist: 2 N + ceil(E / 32) <= E
    assert 2 * 31000 + (64001 + 31) // 32 == 64001 and _query(31000, 64001)
    assert 2 * 31001 + (64002 + 31) // 32 == 64002 + 1 and not _query(31001, 64002)


def test_storage_names():
    from cgat_amd import ops
    was = ops.get_edge_storage()
    try:
        ops.set_edge_storage("f32+za")
        assert ops.get_edge_storage() == "f32+za"
    finally:
        ops.set_edge_storage(was)
    assert ops.get_edge_storage() == was


# ---- graphs and runs ---------------------------------------------------------------------------------------------------
def _ragged_edges(trim_to_256):
    """Crystals of 2 .. 40 atoms with 12 in-crystal neighbours per atom (random destinations: ragged in-degrees), then
    40 atoms that receive nothing, one atom of in-degree 1 and one hub of 300 > SEGB_LONG = 256 incoming edges.  About
    36 000 edges; E % 32 != 0, or E % 256 == 0 with the last edges dropped."""
    g = torch.Generator().manual_seed(77)
    sizes = []
    while sum(sizes) < 2900:
        sizes.append(int(torch.randint(2, 41, (1,), generator=g)))
    src, dst, n0 = [], [], 0
    for a in sizes:
        c = torch.arange(n0, n0 + a).repeat_interleave(12)
        src.append(c)
        dst.append(n0 + torch.randint(0, a, (a * 12,), generator=g))
        n0 += a
    n_cry = n0
    lonely = torch.arange(n_cry, n_cry + 40)                 # sources only: no incoming edge
    src.append(lonely)
    dst.append(torch.randint(0, n_cry, (40,), generator=g))
    one, hub = n_cry + 40, n_cry + 41
    src.append(torch.tensor([0]))
    dst.append(torch.tensor([one]))
    src.append(torch.randint(0, n_cry, (300,), generator=g))
    dst.append(torch.full((300,), hub))
    src.append(torch.tensor([one, hub, hub]))                # (the two feed something too)
    dst.append(torch.tensor([1, 2, 3]))
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    N, E = hub + 1, ei.shape[1]
    if trim_to_256:
        E = E // 256 * 256
        ei = ei[:, torch.randperm(ei.shape[1], generator=g)[:E]]
    elif E % 32 == 0:
        ei = ei[:, :-1]
    return ei.contiguous(), N


_CASES = {}


def _case(kind, H, seed):
    """Inputs, the layer, the results under both storages with the recorded sign masks, and the fp64 oracle's gradient of
    MH_A.fc_out.weight under those signs -- computed once per case and left unchanged."""
    key = (kind, H, seed)
    if key in _CASES:
        return _CASES[key]
    import cgat_amd as P
    from oracle import cgat_oracle as O
    dev = "cuda:0"
    if kind == "base":
        b, _ = P.synthetic_batch(*BASE, seed=seed)
        ei, N = b.edge_index, b.num_nodes
    else:
        ei, N = _ragged_edges(kind == "ragged256")
    E = ei.shape[1]
    g = torch.Generator().manual_seed(100 + seed)
    x, e, x0, cot = (torch.randn(n, 128, generator=g) for n in (N, E, N, N))
    torch.manual_seed(10 * H + seed)
    pm = P.GATConvNodes(128, 128, 128, H, concat=True).to(dev)
    c = {"ei": ei, "N": N, "E": E, "x": x, "e": e, "x0": x0, "cot": cot, "pm": pm, "H": H}
    with _modes(MODE, "f32"):
        c["bit_form"] = P.debug.nodes_attention_bit_form(N, E, 128, 128, H, 256)
        c["f32"], c["masks_f32"] = _layer_run(c, record=True)
    with _modes(MODE, "f32+za"):
        c["za"], c["masks_za"] = _layer_run(c, record=True)
    # the oracle in fp64 on the recorded derivative pattern (LeakyReLU' jumps at 0: see cgat_amd/debug.py)
    om = O.GATConvNodes(128, 128, 128, H, concat=True)
    om.load_state_dict(pm.state_dict())
    om = om.double().to(dev)
    xo, eo = (t.double().to(dev).requires_grad_(True) for t in (x, e))
    with O.forced_masks(om, {k: [m.to(dev) for m in v] for k, v in c["masks_za"].items()}):
        yo = om(xo, ei.to(dev), eo, x0.double().to(dev))
        c["ref"] = torch.autograd.grad((yo * cot.double().to(dev)).sum(), [om.MH_A.fc_out.weight])[0]
    _CASES[key] = c
    return c


def _layer_run(c, record=False, pm=None):
    import cgat_amd as P
    dev = "cuda:0"
    pm = pm if pm is not None else c["pm"]
    xx, ee, xx0 = (t.to(dev).requires_grad_(True) for t in (c["x"], c["e"], c["x0"]))
    for p in pm.parameters():
        p.grad = None
    masks = None
    if record:
        with P.debug.record_masks(pm) as masks:
            y = pm(xx, c["ei"].to(dev), ee, xx0)
    else:
        y = pm(xx, c["ei"].to(dev), ee, xx0)
    (y * c["cot"].to(dev)).sum().backward()
    res = {"out": y.detach().clone(), "grad_x": xx.grad.clone(), "grad_edge_attr": ee.grad.clone()}
    if xx0.grad is not None:
        res["grad_x0"] = xx0.grad.clone()
    for n, p in pm.named_parameters():
        if p.grad is not None:
            res["param:" + n] = p.grad.clone()
    return (res, masks) if record else res


def _errors(c):
    """max |grad - fp64| / max |fp64| of grad MH_A.fc_out.weight under the two storages, and their distance"""
    ref = c["ref"].reshape(-1)
    den = float(ref.abs().max())
    fig = {k: float((c[k][WA].reshape(-1).double() - ref).abs().max()) / den for k in ("f32", "za")}
    fig["between"] = float((c["f32"][WA].double() - c["za"][WA].double()).abs().max()) / den
    return fig


def _assert_only_wa_moves(c):
    a, o = c["f32"], c["za"]
    assert a.keys() == o.keys() and WA in a and "param:MH_A.fc_in.weight" in a and "grad_x0" in a
    for k in a:
        if k != WA:
            assert torch.equal(a[k], o[k]), k
    assert c["masks_f32"].keys() == c["masks_za"].keys() and "MH_A.fc_in.weight" in c["masks_za"]
    for k in c["masks_za"]:
        for u, v in zip(c["masks_f32"][k], c["masks_za"][k]):
            assert torch.equal(u, v), k


# ---- 1 (GPU). where the form is not taken the two storages are the same code ---------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("graphs,mode", [(135, MODE), (136, "f16x3")])
def test_storages_equal_where_the_form_is_not_taken(graphs, mode):
    import cgat_amd as P
    b, _ = P.synthetic_batch(graphs, 20, 12, seed=5)
    N, E = b.num_nodes, b.edge_index.shape[1]
    g = torch.Generator().manual_seed(9)
    c = {"ei": b.edge_index, "N": N, "E": E}
    c["x"], c["e"], c["x0"], c["cot"] = (torch.randn(n, 128, generator=g) for n in (N, E, N, N))
    torch.manual_seed(3)
    c["pm"] = P.GATConvNodes(128, 128, 128, 3, concat=True).to("cuda:0")
    with _modes(mode, "f32"):
        assert not P.debug.nodes_attention_bit_form(N, E, 128, 128, 3, 256)
        a = _layer_run(c)
    with _modes(mode, "f32+za"):
        o = _layer_run(c)
    assert a.keys() == o.keys()
    for k in a:
        assert torch.equal(a[k], o[k]), k


# ---- 2. what keeps its bits ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H", HEADS)
def test_everything_but_one_gradient_keeps_its_bits(H):
    """Output, grad x, grad edge_attr, grad x_0 and every parameter gradient except MH_A.fc_out.weight are bit-equal
    between the two storages, and so are the sign masks of cgat_debug_nodes_attention_signs (attention half from the
    stored bits).  Two steps under the bit form are bit-equal."""
    c = _case("base", H, 0)
    assert c["bit_form"]
    _assert_only_wa_moves(c)
    assert not torch.equal(c["f32"][WA], c["za"][WA])          # the form was taken: that gradient is re-rounded
    with _modes(MODE, "f32"):
        again = _layer_run(c)
    for k in again:
        assert torch.equal(again[k], c["f32"][k]), k


# ---- 3. grad MH_A.fc_out.weight against fp64 ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_fc_out_gradient_against_fp64():
    """Three seeds each of H = 3 and H = 5 at the base shape: the two storages agree to 1e-5 of the largest entry, and the
    largest error of the bit form against the fp64 oracle over the six cases is at most 1.25 x the largest error of the
    stored form over the same six (the CPU emulation of both forms has the new one below the old: DESIGN.md 4)."""
    worst = {"f32": 0.0, "za": 0.0}
    for H in HEADS:
        for seed in SEEDS:
            fig = _errors(_case("base", H, seed))
            print(f"H={H} seed={seed}: bit form {fig['f32']:.3e}  stored {fig['za']:.3e}  between {fig['between']:.3e}")
            assert fig["between"] <= AGREE, (H, seed, fig)
            worst = {k: max(worst[k], fig[k]) for k in worst}
    print(f"largest over the six cases: bit form {worst['f32']:.3e}  stored {worst['za']:.3e}")
    assert worst["f32"] <= MARGIN * worst["za"], worst


# ---- 4. zero weights ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["scattered", "head"])
def test_zero_weights_keep_their_gradient(which):
    """MH_A.fc_out.weight zero in scattered entries / in one whole head: nothing divides by it, so the gradient AT those
    entries is the true one -- finite, not zero where the fp64 oracle's is not, as close to the stored form's as anywhere
    (1e-5 of the largest entry), and no further from fp64 than 1.25 x the stored form's largest error on the same inputs
    (the bound of test_fc_out_gradient_against_fp64)."""
    import copy
    from oracle import cgat_oracle as O
    dev = "cuda:0"
    c = dict(_case("base", 3, 0))
    pm = copy.deepcopy(c["pm"])
    w = pm.MH_A.fc_out.weight
    zero = torch.zeros_like(w, dtype=torch.bool).reshape(3, -1)
    if which == "scattered":
        zero.view(-1)[torch.randperm(zero.numel(), generator=torch.Generator().manual_seed(5))[:97]] = True
    else:
        zero[1] = True
    zero = zero.reshape(w.shape)
    with torch.no_grad():
        w[zero] = 0.0
    c["pm"] = pm
    with _modes(MODE, "f32"):
        got, masks = _layer_run(c, record=True)
    with _modes(MODE, "f32+za"):
        stored = _layer_run(c)
    om = O.GATConvNodes(128, 128, 128, 3, concat=True)
    om.load_state_dict(pm.state_dict())
    om = om.double().to(dev)
    xo, eo = (t.double().to(dev).requires_grad_(True) for t in (c["x"], c["e"]))
    with O.forced_masks(om, {k: [m.to(dev) for m in v] for k, v in masks.items()}):
        yo = om(xo, c["ei"].to(dev), eo, c["x0"].double().to(dev))
        ref = torch.autograd.grad((yo * c["cot"].double().to(dev)).sum(), [om.MH_A.fc_out.weight])[0]
    g, s = got[WA].reshape(ref.shape), stored[WA].reshape(ref.shape)
    den = float(ref.abs().max())
    assert bool(torch.isfinite(g).all())
    err = float((g.double() - ref)[zero].abs().max()) / den
    err_all = float((g.double() - ref).abs().max()) / den
    err_stored = float((s.double() - ref).abs().max()) / den
    between = float((g.double() - s.double()).abs().max()) / den
    print(f"{which}: bit form at the zeroed entries {err:.3e}, at all entries {err_all:.3e}; stored form {err_stored:.3e}; "
          f"between the two {between:.3e}; largest |fp64| at the zeroed entries {float(ref[zero].abs().max()) / den:.3e}")
    assert float(ref[zero].abs().max()) > 1e-3 * den          # not zero by construction ...
    assert int((g[zero] != 0).sum()) >= int(0.99 * int(zero.sum()))   # ... and not zero in the result
    assert between <= AGREE
    assert err <= MARGIN * err_stored and err_all <= MARGIN * err_stored


# ---- 5. ragged graphs ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ragged", "ragged256"])
def test_ragged_graphs(kind):
    """Crystals of 2 .. 40 atoms, atoms without incoming edges, one of in-degree 1, a hub longer than SEGB_LONG; E not a
    multiple of 32, and the same batch cut to a multiple of 256."""
    c = _case(kind, 3, 0)
    assert 33000 <= c["E"] <= 40000 and (c["E"] % 256 == 0 if kind == "ragged256" else c["E"] % 32 != 0)
    deg = torch.bincount(c["ei"][1], minlength=c["N"])
    assert int((deg == 0).sum()) >= 40 and int(deg.max()) > 256
    assert c["bit_form"]
    _assert_only_wa_moves(c)
    with _modes(MODE, "f32"):
        again = _layer_run(c)
    for k in again:
        assert torch.equal(again[k], c["f32"][k]), k
    fig = _errors(c)
    print(f"{kind} (N={c['N']}, E={c['E']}): bit form {fig['f32']:.3e}  stored {fig['za']:.3e}  between {fig['between']:.3e}")
    assert fig["between"] <= AGREE
    assert fig["f32"] <= MARGIN * fig["za"]


# ---- 6. nothing unwritten is read, nothing saved is damaged ---------------------------------------------------------------
@pytest.mark.gpu
def test_poisoned_buffers_and_second_backward():
    from cgat_amd import ops
    c = _case("base", 3, 0)
    want = c["f32"]
    orig_ws, orig_sc = ops.workspace, ops._scratch
    try:
        with _modes(MODE, "f32"):
            for pat in (0xFF, 0x7F, 0x00):
                def ws(nbytes, device, pat=pat):
                    return torch.empty(int(nbytes) + 4096, dtype=torch.uint8, device=device).fill_(pat)

                def sc(numel, dtype, device, pat=pat):
                    t = orig_sc(numel, dtype, device)
                    t.view(torch.uint8).fill_(pat)
                    return t
                ops.workspace, ops._scratch = ws, sc
                got = _layer_run(c)
                torch.cuda.synchronize()
                bad = [k for k in want if not torch.equal(got[k], want[k])]
                assert not bad, f"pattern {pat:#x}: {bad[:4]}"
    finally:
        ops.workspace, ops._scratch = orig_ws, orig_sc
    # the backward writes nothing into the saved buffer: a second backward over the same graph gives the same bits
    dev = "cuda:0"
    pm = c["pm"]
    with _modes(MODE, "f32"):
        xx, ee, xx0 = (t.to(dev).requires_grad_(True) for t in (c["x"], c["e"], c["x0"]))
        y = pm(xx, c["ei"].to(dev), ee, xx0)
        loss = (y * c["cot"].to(dev)).sum()
        leaves = [xx, ee, xx0] + [p for p in pm.parameters()]
        g1 = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
        g2 = torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)
    for k, (u, v) in enumerate(zip(g1, g2)):
        assert (u is None and v is None) or torch.equal(u, v), k
    assert torch.equal(g1[1], want["grad_edge_attr"])


# ---- 7. capture -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_replayed_step_equals_eager():
    from cgat_amd.capture import GraphedStep
    c = _case("base", 3, 0)
    dev = "cuda:0"
    pm = c["pm"]
    params = list(pm.parameters())
    xx, ee, xx0 = (t.to(dev).requires_grad_(True) for t in (c["x"], c["e"], c["x0"]))
    ei, cot = c["ei"].to(dev), c["cot"].to(dev)

    def step():
        y = pm(xx, ei, ee, xx0)
        return [y.detach()] + list(torch.autograd.grad((y * cot).sum(), [xx, ee, xx0] + params, allow_unused=True))
    with _modes(MODE, "f32"):
        want = [None if t is None else t.clone() for t in step()]
        torch.cuda.synchronize()
        graphed = GraphedStep(step)
        for _ in range(3):
            got = graphed.replay()
            torch.cuda.synchronize()
            for k, (u, v) in enumerate(zip(got, want)):
                assert (u is None and v is None) or torch.equal(u, v), k
    assert torch.equal(want[0], c["f32"]["out"]) and torch.equal(want[2], c["f32"]["grad_edge_attr"])


if __name__ == "__main__":      # python tests/test_attn_bit_form.py --record FILE
    out_path = sys.argv[sys.argv.index("--record") + 1]
    doc = {"what": "max |grad MH_A.fc_out.weight - fp64 oracle| / max |fp64| of one GATConvNodes(128,128,128,H) layer step "
                   "in mode f16x3c under edge storage f32 (the bit form) and f32+za (attention pre-activations stored), "
                   "and the largest difference between the two, as a fraction of the same entry",
           "command": "python tests/test_attn_bit_form.py --record FILE   (MI355X)", "cases": {}}
    for kind, H, seed in [("base", H, s) for H in HEADS for s in SEEDS] + [("ragged", 3, 0), ("ragged256", 3, 0)]:
        c = _case(kind, H, seed)
        fig = _errors(c)
        doc["cases"][f"{kind}_H{H}_seed{seed}"] = {"N": c["N"], "E": c["E"], "bit_form": fig["f32"], "stored": fig["za"],
                                                   "between": fig["between"]}
        print(kind, H, seed, fig)
    base = [v for k, v in doc["cases"].items() if k.startswith("base")]
    doc["largest_over_base_cases"] = {"bit_form": max(v["bit_form"] for v in base), "stored": max(v["stored"] for v in base)}
    json.dump(doc, open(out_path, "w"), indent=1)
