"""The attention half of grad edge_attr on a one-plane bit operand (edge_ge_kernel<6, true, true>).

In the attention half  gZ[t, (h, c)] = ga[t, h] wA[h, c] d,  d = 1 or 0.01 by one stored bit m, so with
W'[(h, c), :] = wA[h, c] W_e[(h, c), :] the product is  ga[t, h] (P + 0.01 (cs_h - P)),  P = sum_c m W',  cs_h = sum_c W':
three matrix passes on a bit operand instead of six on a rebuilt, split one.  grad edge_attr therefore no longer has the
parent commit's bits; its yardstick is fp64, never the kernel against itself.

The product is run ALONE on its own inputs (mask, ga, wA, W_e, alpha, gS, dst) through cgat_debug_edge_ge_rebuilt
(include/cgat_hip.h; the launches the layer's backward takes, K groups at few row tiles) and compared with the fp64
product of exactly those inputs, so the figure is the kernel's own rounding error.  The parent's figures are in
tests/golden/edge_ge_parent_error.json, recorded on an MI355X with the parent build plus the same debug entry point by
`python tests/test_edge_ge_bitplane.py --record FILE --key parent`; the bound is 1.25 x those.  The measured figures of
both builds are in that file ("this_form": informational) and in DESIGN.md 4 item 7.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "golden", "edge_ge_parent_error.json")
MARGIN = 1.25

# (name, heads, atoms, edges per atom, hub in-degree): "few" = under 192 row tiles of 256 edges (the K-group launch,
# groups start at head boundaries), "many" = the plain launch
CASES = [("h3_few", 3, 1500, 4, 700), ("h3_many", 3, 14000, 4, 3000), ("h5_few", 5, 1500, 4, 700),
         ("h5_many", 5, 14000, 4, 3000)]


def _ragged_graph(n_atoms, K, hub_in, seed):
    """Atoms of the first 90 % send K edges each to random atoms of that range; the first `hub_in` of them send their
    first edge to atom 0 (a hub of in-degree > 256); the last 10 % neither send nor receive (empty atoms); a ragged
    number of edges is cut off the end so that E is no multiple of 256."""
    rng = np.random.default_rng(seed)
    live = int(n_atoms * 0.9)
    src = np.repeat(np.arange(live), K)
    dst = rng.integers(0, live, size=live * K)
    dst[np.arange(min(hub_in, live)) * K] = 0
    E = live * K - 37
    return torch.from_numpy(np.stack([src[:E], dst[:E]])).long()


def _layer_and_inputs(H, n_atoms, K, hub_in, seed=5):
    import cgat_amd as P
    from oracle import cgat_oracle as O
    ei = _ragged_graph(n_atoms, K, hub_in, seed)
    g = torch.Generator().manual_seed(seed + 1)
    N, E = n_atoms, ei.shape[1]
    x, e, x0, cot = (torch.randn(n, 128, generator=g) for n in (N, E, N, N))
    torch.manual_seed(1)
    om = O.GATConvNodes(128, 128, 128, H, concat=True)
    pm = P.GATConvNodes(128, 128, 128, H, concat=True)
    pm.load_state_dict(om.state_dict())
    return om, pm.to("cuda:0"), ei, x, e, x0, cot


def _hip_g_e(pm, ei, x, e, x0, cot):
    dev = "cuda:0"
    xx, ee = x.to(dev).requires_grad_(True), e.to(dev).requires_grad_(True)
    y = pm(xx, ei.to(dev), ee, x0.to(dev))
    (g_e,) = torch.autograd.grad((y * cot.to(dev)).sum(), [ee])
    return g_e


# ---- the product alone ----
# (name, H, Hd, atoms, edges per atom, hub in-degree, attention half only).  "few": under 192 row tiles, the K-group
# launch -- at Hd = 256 every group is one head, so groups START AT HEAD BOUNDARIES and lie wholly in one half; "many":
# the plain launch, both loops in one workgroup; "attn": alpha = 0, the message half contributes nothing and the figure
# is the attention half's alone; h2x384_few: groups of two column blocks start INSIDE a head of three -> the six-pass
# fallback edge_ge_kernel<6, true, false>
KCASES = [("h3_few", 3, 256, 1500, 4, 700, False), ("h3_many", 3, 256, 14000, 4, 3000, False),
          ("h5_few", 5, 256, 1500, 4, 700, False), ("h5_many", 5, 256, 14000, 4, 3000, False),
          ("h3_many_attn", 3, 256, 14000, 4, 3000, True), ("h5_few_attn", 5, 256, 1500, 4, 700, True),
          ("h2x384_few", 2, 384, 1500, 4, 700, False)]


def _kernel_inputs(H, Hd, n_atoms, K, hub_in, attn_only, seed=7):
    dev = "cuda:0"
    ei = _ragged_graph(n_atoms, K, hub_in, seed)
    dst = torch.sort(ei[1]).values.to(torch.int32)            # destination-sorted slots: the hub's run comes first
    E, W2 = dst.numel(), 2 * H * Hd
    g = torch.Generator().manual_seed(seed + 1)
    m = torch.rand(E, W2, generator=g) < 0.5
    deg = torch.bincount(dst.long(), minlength=n_atoms).clamp(min=1).float()
    alpha = torch.rand(E, H, generator=g) / deg[dst.long()].unsqueeze(1) * 2       # softmax-like: sums to ~1 per node
    ga = torch.randn(E, H, generator=g) * alpha * 0.3                               # logit gradients scale with alpha
    if attn_only:
        alpha = torch.zeros_like(alpha)
    gS = torch.randn(n_atoms, H * Hd, generator=g)
    wA = torch.randn(H * Hd, generator=g) * 0.06
    We = torch.randn(W2, 128, generator=g) * 0.03
    return [t.to(dev) for t in (m, ga, alpha, gS, wA, dst, We)]


def _mask_words(m):
    E, W2 = m.shape
    w = (m.view(E, W2 // 32, 32).long() << torch.arange(32, device=m.device)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def _kernel_error(H, Hd, n_atoms, K, hub_in, attn_only, runs=1):
    """max |out - fp64| / max |fp64| of the product on the inputs above; `runs` > 1 also asserts equal bits."""
    import cgat_amd as P
    m, ga, alpha, gS, wA, dst, We = _kernel_inputs(H, Hd, n_atoms, K, hub_in, attn_only)
    words = _mask_words(m)
    out = P.debug.edge_ge_rebuilt(words, ga, alpha, gS, wA, dst, We, H, Hd)
    for _ in range(runs - 1):
        assert torch.equal(out, P.debug.edge_ge_rebuilt(words, ga, alpha, gS, wA, dst, We, H, Hd))
    HHd, E = H * Hd, m.shape[0]
    slope = float(np.float32(0.01))
    worst, scale = 0.0, 0.0
    for r0 in range(0, E, 8192):
        r = slice(r0, min(E, r0 + 8192))
        d = torch.where(m[r], 1.0, slope).double()
        gzA = (ga[r].double().repeat_interleave(Hd, 1) * wA.double()) * d[:, :HHd]
        gzM = (alpha[r].double().repeat_interleave(Hd, 1) * gS[dst[r].long()].double()) * d[:, HHd:]
        ref = torch.cat([gzA, gzM], 1) @ We.double()
        worst = max(worst, float((out[r].double() - ref).abs().max()))
        scale = max(scale, float(ref.abs().max()))
    return worst / scale


# ---- CPU: the arithmetic of the new form, emulated ----
def _bf16_round(x):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("H", [3, 5])
def test_bitplane_arithmetic_emulated(H):
    """numpy emulation on random operands of the layer's shape (Hd = 256, 128 outputs): W' = fl(wA W) splits EXACTLY
    into three bf16 planes, and  ga (P + 0.01 (cs - P))  with fp32 sums is closer to fp64 than the parent's
    fl(fl(ga wA) d) rows times W (two roundings per element of the row operand against one per weight element); both
    sit well inside the 2e-6 of tests/test_chunked.py::test_rebuilt_gz_equals_stored_gz (bound here: half of it)."""
    rng = np.random.default_rng(H)
    T, Hd = 2048, 256
    m = rng.random((T, H, Hd)) < 0.5
    ga = (rng.standard_normal((T, H)) * 0.1).astype(np.float32)
    wA = (rng.standard_normal((H, Hd)) * 0.06).astype(np.float32)
    W = (rng.standard_normal((H, Hd, 128)) * 0.05).astype(np.float32)
    slope = np.float32(0.01)
    ref = np.einsum("th,hc,thc,hck->tk", ga.astype(np.float64), wA.astype(np.float64),
                    np.where(m, 1.0, np.float64(slope)), W.astype(np.float64))
    gz = ((ga[:, :, None] * wA[None]).astype(np.float32) * np.where(m, np.float32(1), slope)).astype(np.float32)
    parent = gz.reshape(T, -1) @ W.reshape(-1, 128)
    Wp = (wA[:, :, None] * W).astype(np.float32)
    p1 = _bf16_round(Wp)
    r1 = (Wp - p1).astype(np.float32)
    p2 = _bf16_round(r1)
    p3 = _bf16_round((r1 - p2).astype(np.float32))
    assert np.array_equal((p1.astype(np.float64) + p2 + p3).astype(np.float32), Wp)
    acc = np.zeros((T, 128), np.float32)
    for h in range(H):
        P_ = m[:, h].astype(np.float32) @ Wp[h]
        cs = Wp[h].sum(0, dtype=np.float32)
        u = (slope * (cs - P_).astype(np.float32) + P_).astype(np.float32)
        acc = (ga[:, h:h + 1] * u + acc).astype(np.float32)
    scale = np.abs(ref).max()
    err_new, err_parent = np.abs(acc - ref).max() / scale, np.abs(parent - ref).max() / scale
    print(f"H={H}: parent {err_parent:.3e}  bit-plane {err_new:.3e}")
    assert err_new <= 1e-6
    assert err_new <= MARGIN * err_parent


# ---- GPU ----
@pytest.mark.gpu
@pytest.mark.parametrize("case", KCASES, ids=[c[0] for c in KCASES])
def test_g_e_error_not_above_parent(case):
    """max-norm error of the product against fp64 on its own inputs <= 1.25 x the parent build's on the same inputs; two
    runs give equal bits."""
    name = case[0]
    parent = json.load(open(GOLDEN))["parent"][name]
    err = _kernel_error(*case[1:], runs=2)
    print(f"{name}: parent {parent:.4e}  this build {err:.4e}  ratio {err / parent:.3f}")
    assert err <= MARGIN * parent


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_two_runs_and_poisoned_workspace_give_equal_bits(case):
    from cgat_amd import ops
    _, H, n_atoms, K, hub_in = case
    _, pm, ei, x, e, x0, cot = _layer_and_inputs(H, n_atoms, K, hub_in)
    want = _hip_g_e(pm, ei, x, e, x0, cot)
    assert torch.equal(want, _hip_g_e(pm, ei, x, e, x0, cot))
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
            got = _hip_g_e(pm, ei, x, e, x0, cot)
            torch.cuda.synchronize()
            assert torch.equal(got, want), f"pattern {pat:#x}"
    finally:
        ops.workspace, ops._scratch = orig_ws, orig_sc


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[3]], ids=[CASES[0][0], CASES[2][0], CASES[3][0]])
def test_hipgraph_replay_gives_the_eager_bits(case):
    from cgat_amd.capture import GraphedStep
    _, H, n_atoms, K, hub_in = case
    _, pm, ei, x, e, x0, cot = _layer_and_inputs(H, n_atoms, K, hub_in)
    dev = "cuda:0"
    want = _hip_g_e(pm, ei, x, e, x0, cot).clone()
    xs, es, x0s, eis, cots = x.to(dev), e.to(dev).requires_grad_(True), x0.to(dev), ei.to(dev), cot.to(dev)

    def step():
        es.grad = None
        y = pm(xs, eis, es, x0s)
        (y * cots).sum().backward(inputs=[es])
        return es.grad
    graphed = GraphedStep(step)
    for _ in range(2):
        got = graphed.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, want)


if __name__ == "__main__":      # python tests/test_edge_ge_bitplane.py --record FILE [--key parent|this_form]
    out = sys.argv[sys.argv.index("--record") + 1]
    key = sys.argv[sys.argv.index("--key") + 1] if "--key" in sys.argv else "parent"
    doc = json.load(open(out)) if os.path.exists(out) else {
        "what": "max |out - fp64| / max |fp64| of grad edge_attr's product on its own inputs (cgat_debug_edge_ge_rebuilt)",
        "command": "python tests/test_edge_ge_bitplane.py --record FILE --key parent   (parent build with the same "
                   "debug entry point, MI355X)"}
    doc[key] = {c[0]: _kernel_error(*c[1:]) for c in KCASES}
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps(doc[key]))
