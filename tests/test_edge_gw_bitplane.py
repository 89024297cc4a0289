"""The attention half of grad W_e on a one-plane bit operand (edge_gw_kernel<6, true, true>).

In the attention half  gZ[t, (h, c)] = ga[t, h] wA[h, c] d,  d = 1 or 0.01 by one stored bit m.  With the coefficient
moved onto the other operand,  e'_h[t, :] = fl(ga[t, h] e[perm[t], :]),
    grad W_e[(h, c), :] = wA[h, c] (P + 0.01 (cs_h - P)),   P = sum_t m e'_h,   cs_h = sum_t e'_h:
three matrix passes on a bit operand instead of six on a rebuilt, split one, wA and the fold once per output.  The two
halves share one wave of workgroups, so the k-ranges are dealt per half; the message half's slab sums are regrouped.
grad W_e therefore no longer has the parent commit's bits; its yardstick is fp64, never the kernel against itself.

The product is run ALONE on its own inputs through cgat_debug_edge_gw_rebuilt (include/cgat_hip.h) and compared with the
fp64 product of exactly those inputs.  The parent's figures are in tests/golden/edge_gw_parent_error.json, recorded on an
MI355X with the parent build plus the same debug entry point (six passes on every column) by
`python tests/test_edge_gw_bitplane.py --record FILE --key parent`; the bound is 1.25 x those, per case and per half.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "golden", "edge_gw_parent_error.json")
MARGIN = 1.25
HD = 256

# (name, H, edges, atoms, in-degree of atom 0 or 0).  h3_flush: a k-range holds more than two flush groups of 2 048 slots
# in BOTH halves (at 256 workgroups a range of E = 14 000 is a few hundred slots); ragged: a hub and atoms without edges
KCASES = [("h3_e1500", 3, 1500, 300, 0), ("h3_e14000", 3, 14000, 2000, 0), ("h5_e1500", 5, 1500, 300, 0),
          ("h8_e3000", 8, 3000, 500, 0), ("h3_ragged", 3, 2301, 400, 700), ("h3_flush", 3, 300001, 20000, 0)]


def _kernel_inputs(H, E, n_atoms, hub, seed=11):
    """Destination-sorted slots on `n_atoms` atoms of which the last 10 % receive nothing (and atom 0 `hub` edges)."""
    dev = "cuda:0"
    g = torch.Generator().manual_seed(seed)
    live = int(n_atoms * 0.9)
    dst = torch.randint(0, live, (E,), generator=g)
    dst[:hub] = 0
    dst = torch.sort(dst).values.to(torch.int32)
    W2 = 2 * H * HD
    words = torch.randint(-2 ** 31, 2 ** 31, (E, W2 // 32), generator=g).to(torch.int32)     # the mask, 32 columns a word
    deg = torch.bincount(dst.long(), minlength=n_atoms).clamp(min=1).float()
    alpha = torch.rand(E, H, generator=g) / deg[dst.long()].unsqueeze(1) * 2
    ga = torch.randn(E, H, generator=g) * alpha * 0.3
    gS = torch.randn(n_atoms, H * HD, generator=g)
    wA = torch.randn(H * HD, generator=g) * 0.06
    e = torch.randn(E, 128, generator=g)
    perm = torch.randperm(E, generator=g).to(torch.int32)
    return [t.to(dev) for t in (words, ga, alpha, gS, wA, e, perm, dst)]


def _mask_bits(words):
    return ((words.unsqueeze(-1) >> torch.arange(32, device=words.device, dtype=torch.int32)) & 1).bool().flatten(1)


_CACHE = {}


def _case(name):
    """(inputs with the mask as words, fp64 product) of a case, computed once."""
    if name not in _CACHE:
        _, H, E, n_atoms, hub = next(c for c in KCASES if c[0] == name)
        words, ga, alpha, gS, wA, e, perm, dst = _kernel_inputs(H, E, n_atoms, hub)
        HHd, slope = H * HD, float(np.float32(0.01))
        ref = torch.zeros(2 * HHd, 128, dtype=torch.float64, device=words.device)
        for r0 in range(0, E, 8192):
            r = slice(r0, min(E, r0 + 8192))
            d = torch.where(_mask_bits(words[r]), 1.0, slope).double()
            gzA = (ga[r].double().repeat_interleave(HD, 1) * wA.double()) * d[:, :HHd]
            gzM = (alpha[r].double().repeat_interleave(HD, 1) * gS[dst[r].long()].double()) * d[:, HHd:]
            ref += torch.cat([gzA, gzM], 1).t() @ e[perm[r].long()].double()
        _CACHE[name] = ((words, ga, alpha, gS, wA, e, perm, dst), H, ref)
    return _CACHE[name]


def _figures(out, ref, HHd):
    """max |out - fp64| / max |fp64| of (a) the attention rows, (b) the message rows, (c) all rows"""
    err = (out.double() - ref).abs()
    return {"attention": float(err[:HHd].max() / ref[:HHd].abs().max()),
            "message": float(err[HHd:].max() / ref[HHd:].abs().max()),
            "full": float(err.max() / ref.abs().max())}


def _run(name, force_six=False):
    import cgat_amd as P
    t, H, ref = _case(name)
    out, took = P.debug.edge_gw_rebuilt(*t, H, HD, force_six=force_six)
    return out, took


# ---- CPU: the arithmetic of the new form, emulated ----
def _bf16_round(x):
    u = x.astype(np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def _emulated(H):
    rng = np.random.default_rng(H)
    T = 700
    m = rng.random((T, H, HD)) < 0.5
    ga = (rng.standard_normal((T, H)) * 0.1).astype(np.float32)
    wA = (rng.standard_normal((H, HD)) * 0.06).astype(np.float32)
    e = rng.standard_normal((T, 128)).astype(np.float32)
    slope = np.float32(0.01)
    ref = np.einsum("th,hc,thc,tk->hck", ga.astype(np.float64), wA.astype(np.float64),
                    np.where(m, 1.0, np.float64(slope)), e.astype(np.float64))
    ep = (ga[:, :, None] * e[:, None, :]).astype(np.float32)             # e'_h[t, :]: one fp32 rounding
    p1 = _bf16_round(ep)
    r1 = (ep - p1).astype(np.float32)
    p2 = _bf16_round(r1)
    p3 = _bf16_round((r1 - p2).astype(np.float32))
    split_exact = np.array_equal((p1.astype(np.float64) + p2 + p3).astype(np.float32), ep)
    planes = p1.astype(np.float64) + p2.astype(np.float64) + p3.astype(np.float64)
    P_ = np.einsum("thc,thk->hck", m.astype(np.float64), planes)          # fp64 sums of the three planes
    cs = planes.sum(0)                                                    # [H, 128]
    P32, cs32 = P_.astype(np.float32), cs.astype(np.float32)
    u = (slope * (cs32[:, None, :] - P32).astype(np.float32) + P32).astype(np.float32)
    out = (wA[:, :, None] * u).astype(np.float32)
    return split_exact, float(np.abs(out - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("H", [3, 5])
def test_bitplane_arithmetic_emulated(H):
    """What the FORM loses, independent of any kernel: one fp32 rounding per element of e' (exactly representable in three
    bf16 planes) and the three roundings of the fold.  Each is at most 2^-24 relative on its own value; the sum over 700
    slots of independent roundings stays within a few 2^-24 of the largest entry: bound 4 x 2^-24 = 2.4e-7.  The figures
    are recorded in tests/golden/edge_gw_parent_error.json ("emulated_form")."""
    split_exact, err = _emulated(H)
    print(f"H={H}: emulated form {err:.3e}")
    assert split_exact
    assert err <= 4 * 2.0 ** -24
    doc = json.load(open(GOLDEN))
    assert doc["emulated_form"][f"H{H}"] == pytest.approx(err, rel=1e-3)


# ---- GPU ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in KCASES])
def test_g_w_error_not_above_parent(name):
    """Per case and per half: error against fp64 <= 1.25 x the parent's on the same inputs; the forced six-pass form
    reproduces the parent's figures to every recorded digit."""
    parent = json.load(open(GOLDEN))["parent"][name]
    _, H, ref = _case(name)
    out, took = _run(name)
    assert took
    fig = _figures(out, ref, H * HD)
    six, took6 = _run(name, force_six=True)
    assert not took6
    fig6 = _figures(six, ref, H * HD)
    for k in ("attention", "message", "full"):
        print(f"{name} {k}: parent {parent[k]:.4e}  this build {fig[k]:.4e}  ratio {fig[k] / parent[k]:.3f}  "
              f"forced six-pass {fig6[k]:.4e}")
    for k in ("attention", "message", "full"):
        assert fig6[k] == parent[k], k
        assert fig[k] <= MARGIN * parent[k], k


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c[0] for c in KCASES])
def test_two_runs_poisoned_workspace_and_replay_give_equal_bits(name):
    import cgat_amd as P
    from cgat_amd import ops
    from cgat_amd.capture import GraphedStep
    t, H, _ = _case(name)
    want, _ = _run(name)
    assert torch.equal(want, _run(name)[0])
    orig_ws = ops.workspace
    try:
        for pat in (0xFF, 0x7F):
            ops.workspace = lambda nbytes, device, pat=pat: torch.empty(int(nbytes) + 4096, dtype=torch.uint8,
                                                                       device=device).fill_(pat)
            got, _ = _run(name)
            torch.cuda.synchronize()
            assert torch.equal(got, want), f"pattern {pat:#x}"
    finally:
        ops.workspace = orig_ws
    graphed = GraphedStep(lambda: P.debug.edge_gw_rebuilt(*t, H, HD)[0])
    for _ in range(3):
        got = graphed.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, want)


def _layer_run(pm, ei, x, e, x0, cot):
    dev = "cuda:0"
    xx, ee, xx0 = (t.to(dev).requires_grad_(True) for t in (x, e, x0))
    for p in pm.parameters():
        p.grad = None
    y = pm(xx, ei.to(dev), ee, xx0)
    (y * cot.to(dev)).sum().backward()
    res = {"out": y.detach().clone(), "grad_x": xx.grad.clone(), "grad_edge_attr": ee.grad.clone()}
    if xx0.grad is not None:
        res["grad_x0"] = xx0.grad.clone()
    for n, p in pm.named_parameters():
        if p.grad is not None:
            res["param:" + n] = p.grad.clone()
    return res


@pytest.mark.gpu
def test_layer_only_the_two_w_e_blocks_move():
    """GATConvNodes(128, 128, 128, 3) above the small-row limit, forward + backward: everything but the W_e blocks of the
    two first-layer weight gradients is bit-equal to the run with the route disabled; those blocks agree to 2e-6 of their
    largest entry (the bar of test_rebuilt_gz_equals_stored_gz for a re-rounded product)."""
    import cgat_amd as P
    b, _ = P.synthetic_batch(150, 20, 12)
    g = torch.Generator().manual_seed(3)
    N, E = b.num_nodes, b.edge_index.shape[1]
    x, e, x0, cot = (torch.randn(n, 128, generator=g) for n in (N, E, N, N))
    torch.manual_seed(1)
    pm = P.GATConvNodes(128, 128, 128, 3, concat=True).to("cuda:0")
    new = _layer_run(pm, b.edge_index, x, e, x0, cot)
    was = P.debug.edge_gw_force_six(True)
    try:
        old = _layer_run(pm, b.edge_index, x, e, x0, cot)
    finally:
        P.debug.edge_gw_force_six(was)
    assert new.keys() == old.keys()
    moved = 0
    for k in new:
        if k in ("param:MH_A.fc_in.weight", "param:MH_M.fc_in.weight"):
            a, o = new[k].reshape(3 * HD, 384), old[k].reshape(3 * HD, 384)
            assert torch.equal(a[:, :128], o[:, :128]) and torch.equal(a[:, 256:], o[:, 256:]), k
            d = float((a[:, 128:256] - o[:, 128:256]).abs().max() / o[:, 128:256].abs().max())
            print(f"{k} W_e block: {d:.3e} of its largest entry")
            assert d <= 2e-6, k
            moved += int(d > 0)
        else:
            assert torch.equal(new[k], old[k]), k
    assert moved == 2        # the route was taken: both halves are regrouped


@pytest.mark.gpu
def test_routing():
    """bf16-mma, f16x3, Hd != 256 and the stored-gZ / vector-attention layers do not take the new form and keep the bits of
    the forced six-pass call; the f32 mode has no such launch at all."""
    import cgat_amd as P
    from cgat_amd import ops
    t, H, _ = _case("h3_e1500")
    from cgat_amd._lib import CgatHipError
    mode0, storage0 = ops.get_bilinear_mode(), ops.get_edge_storage()
    assert _run("h3_e1500")[1]
    try:
        for mode, storage in (("f16x3", "f32"), ("bf16x6", "bf16-mma")):
            ops.set_bilinear_mode(mode)
            ops.set_edge_storage(storage)
            out, took = P.debug.edge_gw_rebuilt(*t, H, HD)
            six, _ = P.debug.edge_gw_rebuilt(*t, H, HD, force_six=True)
            assert not took and torch.equal(out, six), (mode, storage)
        ops.set_edge_storage("f32")
        ops.set_bilinear_mode("f32")
        with pytest.raises(CgatHipError, match=r"code 4\).*split arithmetic modes only"):     # CGAT_ERR_UNSUPPORTED
            P.debug.edge_gw_rebuilt(*t, H, HD)
    finally:
        ops.set_bilinear_mode(mode0)
        ops.set_edge_storage(storage0)
    # Hd = 128 (two heads per column-block pair)
    words, ga, alpha, gS, wA, e, perm, dst = _kernel_inputs(3, 1500, 300, 0)
    words = words[:, :2 * 6 * 128 // 32].contiguous()
    t128 = (words, ga.repeat(1, 2), alpha.repeat(1, 2), gS[:, :6 * 128].contiguous(), wA[:6 * 128].contiguous(), e, perm, dst)
    out, took = P.debug.edge_gw_rebuilt(*t128, 6, 128)
    six, _ = P.debug.edge_gw_rebuilt(*t128, 6, 128, force_six=True)
    assert not took and torch.equal(out, six)
    # vector attention: gZ is stored, the launch has nothing to rebuild from
    b, _ = P.synthetic_batch(150, 20, 12)
    g = torch.Generator().manual_seed(4)
    N, E = b.num_nodes, b.edge_index.shape[1]
    x, ee, x0, cot = (torch.randn(n, 128, generator=g) for n in (N, E, N, N))
    torch.manual_seed(2)
    pv = P.GATConvNodes(128, 128, 128, 3, concat=True, vector_attention=True).to("cuda:0")
    new = _layer_run(pv, b.edge_index, x, ee, x0, cot)
    was = P.debug.edge_gw_force_six(True)
    try:
        old = _layer_run(pv, b.edge_index, x, ee, x0, cot)
    finally:
        P.debug.edge_gw_force_six(was)
    for k in new:
        assert torch.equal(new[k], old[k]), k


if __name__ == "__main__":      # python tests/test_edge_gw_bitplane.py --record FILE [--key parent|this_form]
    out_path = sys.argv[sys.argv.index("--record") + 1]
    key = sys.argv[sys.argv.index("--key") + 1] if "--key" in sys.argv else "parent"
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {
        "what": "max |out - fp64| / max |fp64| of grad W_e's product on its own inputs (cgat_debug_edge_gw_rebuilt), "
                "per half of the rows and over all rows",
        "command": "python tests/test_edge_gw_bitplane.py --record FILE --key parent   (parent build with the same "
                   "debug entry point, six passes forced, MI355X)"}
    doc["emulated_form"] = {f"H{H}": _emulated(H)[1] for H in (3, 5)}
    doc[key] = {}
    for c in KCASES:
        o, _ = _run(c[0], force_six=(key == "parent"))
        doc[key][c[0]] = _figures(o, _case(c[0])[2], c[1] * HD)
    json.dump(doc, open(out_path, "w"), indent=1)
    print(json.dumps(doc[key]))
