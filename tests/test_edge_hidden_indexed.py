"""cgat_edge_hidden_forward_indexed / cgat_edge_hidden_backward_indexed -- the vector-attention first layer on shell-indexed
edge features, edge_attr[e] = table[index[e]] -- through the raw C ABI, in the harness of tests/test_edge_hidden.py:
outputs pre-filled with NaN, a workspace of exactly the queried size filled with 0xFF bytes and followed by a 4-KB guard
that must stay intact, inputs bit-unchanged, a second call bit-identical.

Reference: that file's fp64 formulae with e = table[index], plus

    g_table = index_add(index[perm], g_m[:, C:C+Ce])                      [R, Ce]

Bounds, both the project's own: TOL = 2e-5 max-norm relative (g_w_in per column block), and the ratio rule of
tests/test_indexed_edge_attr.py: the error against fp64 is at most RATIO = 2 times that of the DENSE op
(cgat_edge_hidden_forward / _backward) on the same inputs with e = table[index]; the dense op's g_table is the exact
(fp64) per-class sum of its g_edge_attr.  With g_is_pre = 0 the sign source is the hidden the call returned, and every
element whose sign differs from the fp64 pre-activation's must have |pre| <= 1e-5 max |pre|.  Every figure is printed
before it is asserted, as `EDGE_HIDDEN_IDX <case>/<mode>[/<variant>] <output> rel <r> err64 <indexed> dense <dense>`.

    case          N, E, C, Ce, W2             R     what it pins
    small         301, 701, 128, 128, 512     13    small-row node side; six used classes of one piece each
    one_class     301, 701, 128, 128, 512     1     every slot in one class (3 pieces); Te of one row
    exact_pieces  301, 768, 128, 128, 512     3     index = t % 3 in slot order: classes of exactly 256 rows
    wide          301, 1207, 128, 128, 2560   25    the harness-default width (H = 5, Hd = 256)
    large_rows    2101, 5003, 128, 128, 512   65    node side above the small-row limit; many rows
    widths        203, 1207, 64, 32, 192      13    generic engine, Ce != C
    hub           301, 1400, 128, 128, 512    13    one destination of 300 edges (> SEG_LONG), one atom without in-edges

Indices come from test_indexed_edge_attr._index (even rows only, never the last): the rows of g_table of unused classes
must be exactly 0, those of used classes non-zero."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_edge_hidden import (DEV, TOL, _assert_flips_near_zero, _call_backward, _call_forward, _graph, _guard_intact, _nan,
                              _ptr, _slope, _workspace, rel)
from test_indexed_edge_attr import RATIO, _index

pytestmark = pytest.mark.gpu

CASES = {   # name: N, E, C, Ce, W2, R
    "small": (301, 701, 128, 128, 512, 13),
    "one_class": (301, 701, 128, 128, 512, 1),
    "exact_pieces": (301, 768, 128, 128, 512, 3),
    "wide": (301, 1207, 128, 128, 2560, 25),
    "large_rows": (2101, 5003, 128, 128, 512, 65),
    "widths": (203, 1207, 64, 32, 192, 13),
    "hub": (301, 1400, 128, 128, 512, 13),
}
_cache = {}


def _graph_hub(N, E, seed):
    """One destination (atom 100) of 300 edges, the last atom without in-edges, edges source-major."""
    rs = np.random.RandomState(seed)
    src = rs.randint(0, N, size=E)
    dst = rs.randint(0, N - 1, size=E)
    dst[dst == 100] = 101
    dst[:300] = 100
    order = np.argsort(src, kind="stable")
    return torch.from_numpy(np.stack([src[order], dst[order]])).long()


class _Inputs:
    """The operands of one case (shared by every mode and test: never written) and the fp64 forward of the reference."""

    def __init__(self, case):
        from cgat_amd import ops
        N, E, Cn, Ce, W2, R = CASES[case]
        D = 2 * Cn + Ce
        g = torch.Generator().manual_seed(N + E + W2 + R)
        self.dims, self.R = (N, E, Cn, Ce, W2), R
        self.x = torch.randn(N, Cn, generator=g).to(DEV)
        self.table = torch.randn(R, Ce, generator=g).to(DEV)
        self.w = (torch.randn(W2, D, generator=g) * D ** -0.5).to(DEV)
        self.b = torch.randn(W2, generator=g).to(DEV)
        self.g = torch.randn(E, W2, generator=g).to(DEV)
        self.ei = (_graph_hub(N, E, N + E) if case == "hub" else _graph(N, E, N + E)).to(DEV)
        self.plan = ops.EdgePlan(self.ei, N)
        p = self.plan
        self.dst_s, self.src_s, self.perm = p.dst_sorted.long(), p.src_sorted.long(), p.dst_perm.long()
        if case == "exact_pieces":              # index[perm[t]] = t % 3
            self.index = torch.empty(E, dtype=torch.int64, device=DEV)
            self.index[self.perm] = torch.arange(E, device=DEV) % 3
        else:
            self.index = _index(E, R).to(DEV)
        self.used = torch.bincount(self.index, minlength=R) > 0
        deg_in = torch.bincount(self.ei[1], minlength=N)
        if case == "hub":
            assert int(deg_in.max()) == 300 and int(deg_in[N - 1]) == 0
        if case == "exact_pieces":
            assert torch.bincount(self.index, minlength=R).tolist() == [256, 256, 256]
        self.cls = ops._class_plan(self.index, p, R)
        self.e = self.table[self.index].contiguous()               # the dense op's edge features
        xd = self.x.double()
        self.m = torch.cat([xd[self.dst_s], self.e.double()[self.perm], xd[self.src_s]], 1)
        self.pre = self.m @ self.w.double().t() + self.b.double()
        self.hidden = torch.nn.functional.leaky_relu(self.pre, 0.01)


def _inputs(case):
    if case not in _cache:
        _cache[case] = _Inputs(case)
    return _cache[case]


def _reference_backward(inp, gZ):
    N, E, Cn, Ce, W2 = inp.dims
    g_m = gZ @ inp.w.double()
    g_x = torch.zeros(N, Cn, dtype=torch.float64, device=DEV)
    g_x.index_add_(0, inp.dst_s, g_m[:, :Cn])
    g_x.index_add_(0, inp.src_s, g_m[:, Cn + Ce:])
    g_t = torch.zeros(inp.R, Ce, dtype=torch.float64, device=DEV)
    g_t.index_add_(0, inp.index[inp.perm], g_m[:, Cn:Cn + Ce])
    return {"g_x": g_x, "g_table": g_t, "g_w_in": gZ.t() @ inp.m, "g_b_in": gZ.sum(0)}


def _raw_forward(plan, dims, R, x, table, index, w, b, nbytes=None, hidden=None, hmax=None):
    from cgat_amd import _lib
    N, E, Cn, Ce, W2 = dims
    full = _lib.lib.cgat_edge_hidden_forward_indexed_workspace_bytes(C.byref(plan.c), Cn, Ce, W2, R)
    nbytes = full if nbytes is None else nbytes
    ws = _workspace(full)
    rc = _lib.lib.cgat_edge_hidden_forward_indexed(C.byref(plan.c), Cn, Ce, W2, _ptr(w), _ptr(b), _ptr(x), _ptr(table), R,
                                                   _ptr(index), _ptr(hidden), _ptr(hmax), _ptr(ws), nbytes, None)
    return rc, ws, full


def _call_forward_indexed(inp):
    """One raw cgat_edge_hidden_forward_indexed on fresh NaN outputs and a fresh 0xFF workspace of exactly the queried size."""
    from cgat_amd import _lib
    N, E, Cn, Ce, W2 = inp.dims
    hidden, hmax = _nan(E, W2), _nan(1)
    ins = (inp.x, inp.table, inp.index, inp.w, inp.b)
    keep = [t.clone() for t in ins]
    rc, ws, nbytes = _raw_forward(inp.plan, inp.dims, inp.R, inp.x, inp.table, inp.index, inp.w, inp.b, None, hidden, hmax)
    _lib.check(rc, "cgat_edge_hidden_forward_indexed")
    torch.cuda.synchronize()
    assert _guard_intact(ws, nbytes), "forward wrote behind its workspace"
    assert all(torch.equal(a, k) for a, k in zip(ins, keep)), "forward changed an input"
    assert bool(torch.isfinite(hidden).all()) and bool(torch.isfinite(hmax).all())
    return hidden, hmax


def _raw_backward(plan, dims, R, x, table, index, cls, w, hidden, g_hidden, g_is_pre, absmax, out, nbytes=None):
    from cgat_amd import _lib
    N, E, Cn, Ce, W2 = dims
    full = _lib.lib.cgat_edge_hidden_backward_indexed_workspace_bytes(C.byref(plan.c), Cn, Ce, W2, R)
    nbytes = full if nbytes is None else nbytes
    ws = _workspace(full)
    rc = _lib.lib.cgat_edge_hidden_backward_indexed(
        C.byref(plan.c), Cn, Ce, W2, _ptr(w), _ptr(x), _ptr(table), R, _ptr(index), _ptr(cls[0]), _ptr(cls[1]), _ptr(cls[2]),
        _ptr(hidden), _ptr(g_hidden), 1 if g_is_pre else 0, None if absmax is None else _ptr(absmax), _ptr(out["g_x"]),
        _ptr(out["g_table"]), _ptr(out["g_w_in"]), _ptr(out["g_b_in"]), _ptr(ws), nbytes, None)
    return rc, ws, full


def _nan_grads(dims, R):
    N, E, Cn, Ce, W2 = dims
    return {"g_x": _nan(N, Cn), "g_table": _nan(R, Ce), "g_w_in": _nan(W2, 2 * Cn + Ce), "g_b_in": _nan(W2)}


def _call_backward_indexed(inp, hidden, g_hidden, g_is_pre=False, absmax=None):
    from cgat_amd import _lib
    out = _nan_grads(inp.dims, inp.R)
    ins = (inp.x, inp.table, inp.index, inp.w, hidden, g_hidden, *inp.cls) + (() if absmax is None else (absmax,))
    keep = [t.clone() for t in ins]
    rc, ws, nbytes = _raw_backward(inp.plan, inp.dims, inp.R, inp.x, inp.table, inp.index, inp.cls, inp.w, hidden, g_hidden,
                                   g_is_pre, absmax, out)
    _lib.check(rc, "cgat_edge_hidden_backward_indexed")
    torch.cuda.synchronize()
    assert _guard_intact(ws, nbytes), "backward wrote behind its workspace"
    assert all(torch.equal(a, k) for a, k in zip(ins, keep)), "backward changed an input"
    for name, t in out.items():
        assert bool(torch.isfinite(t).all()), f"{name} has elements that are not finite (or were never written)"
    return out


def _err64(a, b):
    return float((a.double() - b.double()).abs().max())


def _check(tag, name, got, dense, ref):
    """TOL against fp64 and the ratio rule against the dense op's error on the same inputs; prints before it asserts."""
    r, e_idx, e_dense = rel(got, ref), _err64(got, ref), _err64(dense, ref)
    print(f"EDGE_HIDDEN_IDX {tag} {name} rel {r:.3e} err64 {e_idx:.3e} dense {e_dense:.3e} "
          f"ratio {e_idx / max(e_dense, 1e-300):.3f}")
    return (name, r, e_idx, e_dense)


def _assert_all(figs):
    bad = [f for f in figs if not (f[1] <= TOL and f[2] <= RATIO * f[3])]
    assert not bad, bad


def _forward_checked(inp, tag):
    """Forward twice (bit-identical), against fp64 and the dense forward; returns the GPU hidden."""
    hidden, hmax = _call_forward_indexed(inp)
    again, hmax2 = _call_forward_indexed(inp)
    assert torch.equal(hidden, again) and torch.equal(hmax, hmax2), "two identical forward calls differ"
    dense, _ = _call_forward(inp.plan, inp.dims, inp.x, inp.e, inp.w, inp.b)
    figs = [_check(tag, "hidden", hidden, dense, inp.hidden)]
    print(f"EDGE_HIDDEN_IDX {tag} hmax {float(hmax):.9e} max|hidden| {float(hidden.abs().max()):.9e}")
    _assert_all(figs)
    assert torch.equal(hmax[0], hidden.abs().max()), (float(hmax), float(hidden.abs().max()))
    _assert_flips_near_zero(inp, hidden)
    return hidden


def _backward_checked(inp, hidden, g_hidden, tag, g_is_pre=False, absmax=None):
    """Backward twice (bit-identical), against the fp64 reference on the branch the GPU forward took and against the dense
    backward on the same hidden and gradient."""
    N, E, Cn, Ce, W2 = inp.dims
    out = _call_backward_indexed(inp, hidden, g_hidden, g_is_pre, absmax)
    again = _call_backward_indexed(inp, hidden, g_hidden, g_is_pre, absmax)
    assert all(torch.equal(out[k], again[k]) for k in out), "two identical backward calls differ"
    gZ = g_hidden.double() if g_is_pre else g_hidden.double() * _slope(hidden)
    ref = _reference_backward(inp, gZ)
    dense = _call_backward(inp.plan, inp.dims, inp.x, inp.e, inp.w, hidden, g_hidden, g_is_pre, absmax)
    dense["g_table"] = torch.zeros(inp.R, Ce, dtype=torch.float64, device=DEV).index_add_(0, inp.index, dense["g_e"].double())
    figs = [_check(tag, k, out[k], dense[k], ref[k]) for k in ("g_x", "g_table", "g_b_in")]
    blocks = {"g_w_in[W_i]": slice(0, Cn), "g_w_in[W_e]": slice(Cn, Cn + Ce), "g_w_in[W_j]": slice(Cn + Ce, None)}
    figs += [_check(tag, k, out["g_w_in"][:, s], dense["g_w_in"][:, s], ref["g_w_in"][:, s]) for k, s in blocks.items()]
    _assert_all(figs)
    # classes no edge uses: exactly 0; used classes: non-zero
    gt = out["g_table"]
    assert float(gt[~inp.used].abs().max()) == 0.0 if bool((~inp.used).any()) else True
    assert bool((gt[inp.used].abs().amax(1) > 0).all())
    return out


MODE_CASES = [(c, "f16x3c") for c in CASES] + [("small", m) for m in ("bf16x6", "f16x3", "f32")]


@pytest.mark.parametrize("case,mode", MODE_CASES, ids=lambda v: v)
def test_edge_hidden_indexed_vs_fp64(case, mode):
    """Forward and backward (g_is_pre = 0) of every case."""
    from cgat_amd import ops
    ops.set_bilinear_mode(mode)
    try:
        inp = _inputs(case)
        assert ops.edge_hidden_indexed_ok(inp.plan.c, inp.dims[2], inp.dims[3], inp.dims[4], inp.R)
        hidden = _forward_checked(inp, f"{case}/{mode}")
        _backward_checked(inp, hidden, inp.g, f"{case}/{mode}")
    finally:
        ops.set_bilinear_mode(ops.DEFAULT_MODE)


@pytest.mark.parametrize("has_absmax", [False, True])
@pytest.mark.parametrize("case", ["small", "wide"])
def test_edge_hidden_indexed_g_is_pre(case, has_absmax):
    """g_is_pre = 1: g_hidden is the pre-activation gradient itself, read in place (it must come back bit-identical);
    gpre_absmax, where given, is its exact maximum.  No sign allowance."""
    from cgat_amd import ops
    ops.set_bilinear_mode(ops.DEFAULT_MODE)
    inp = _inputs(case)
    hidden, _ = _call_forward_indexed(inp)
    absmax = inp.g.abs().max().reshape(1) if has_absmax else None
    _backward_checked(inp, hidden, inp.g, f"{case}/is_pre{'+max' if has_absmax else ''}", True, absmax)


def _refused(fn):
    """fn() -> rc: refused with an error code before any launch."""
    from cgat_amd import ops
    n0 = ops.prof_launches()
    rc = fn()
    torch.cuda.synchronize()
    assert rc != 0, "the call was not refused"
    assert ops.prof_launches() == n0, "a kernel was launched before the refusal"


def test_edge_hidden_indexed_refusals():
    """cgat_edge_hidden_indexed_ok is false for R = 257, E = 0, N = 0, W2 = 510 and under edge storage "bf16"; there, and with
    a workspace one byte short, both entries return an error before any launch and write nothing."""
    from cgat_amd import _lib, ops
    ops.set_bilinear_mode(ops.DEFAULT_MODE)
    inp = _inputs("small")
    N, E, Cn, Ce, W2 = inp.dims
    R = inp.R
    hidden_ok, _ = _call_forward_indexed(inp)
    g = torch.Generator().manual_seed(3)
    empty = ops.EdgePlan(torch.zeros(2, 0, dtype=torch.long, device=DEV), N)
    none = ops.EdgePlan(torch.zeros(2, 0, dtype=torch.long, device=DEV), 0)
    t257 = torch.randn(257, Ce, generator=g).to(DEV)
    w510 = inp.w[:510].contiguous()
    bad = {   # name: plan, dims, R, table, w, b
        "R=257": (inp.plan, inp.dims, 257, t257, inp.w, inp.b),
        "E=0": (empty, (N, 0, Cn, Ce, W2), R, inp.table, inp.w, inp.b),
        "N=0": (none, (0, 0, Cn, Ce, W2), R, inp.table, inp.w, inp.b),
        "W2=510": (inp.plan, (N, E, Cn, Ce, 510), R, inp.table, w510, inp.b[:510].contiguous()),
    }

    def both(name, plan, dims, R_, table, w, b):
        assert not ops.edge_hidden_indexed_ok(plan.c, dims[2], dims[3], dims[4], R_), name
        hidden, hmax = _nan(max(dims[1], 1), dims[4]), _nan(1)
        _refused(lambda: _raw_forward(plan, dims, R_, inp.x, table, inp.index, w, b, None, hidden, hmax)[0])
        assert bool(torch.isnan(hidden).all()) and bool(torch.isnan(hmax).all()), name
        out = _nan_grads(dims, R_)
        gh = inp.g[:, :dims[4]].contiguous()
        _refused(lambda: _raw_backward(plan, dims, R_, inp.x, table, inp.index, inp.cls, w, hidden_ok, gh, False, None,
                                       out)[0])
        assert all(bool(torch.isnan(t).all()) for t in out.values() if t.numel()), name

    for name, args in bad.items():
        both(name, *args)
    ops.set_edge_storage("bf16")
    try:
        both("bf16", inp.plan, inp.dims, R, inp.table, inp.w, inp.b)
    finally:
        ops.set_edge_storage("f32")
    assert ops.edge_hidden_indexed_ok(inp.plan.c, Cn, Ce, W2, R)
    # a workspace one byte short
    hidden, hmax = _nan(E, W2), _nan(1)
    full = _lib.lib.cgat_edge_hidden_forward_indexed_workspace_bytes(C.byref(inp.plan.c), Cn, Ce, W2, R)
    _refused(lambda: _raw_forward(inp.plan, inp.dims, R, inp.x, inp.table, inp.index, inp.w, inp.b, full - 1, hidden, hmax)[0])
    assert bool(torch.isnan(hidden).all()) and bool(torch.isnan(hmax).all())
    out = _nan_grads(inp.dims, R)
    full = _lib.lib.cgat_edge_hidden_backward_indexed_workspace_bytes(C.byref(inp.plan.c), Cn, Ce, W2, R)
    _refused(lambda: _raw_backward(inp.plan, inp.dims, R, inp.x, inp.table, inp.index, inp.cls, inp.w, hidden_ok, inp.g, False,
                                   None, out, full - 1)[0])
    assert all(bool(torch.isnan(t).all()) for t in out.values())


def test_edge_hidden_indexed_autograd_wrappers():
    """ops.EdgeHiddenIndexedFn through autograd at the `small` shape against the same reference: the wrapper's argument
    order, its g_is_pre = 0 call, hmax as a non-differentiable output, and no saved tensor of E * Ce elements."""
    from cgat_amd import ops
    ops.set_bilinear_mode(ops.DEFAULT_MODE)
    inp = _inputs("small")
    N, E, Cn, Ce, W2 = inp.dims
    x, t, w, b = (v.clone().requires_grad_(True) for v in (inp.x, inp.table, inp.w, inp.b))
    sizes = []
    with torch.autograd.graph.saved_tensors_hooks(lambda v: (sizes.append(v.numel()), v)[1], lambda v: v):
        hidden, hmax = ops.EdgeHiddenIndexedFn.apply(x, t, inp.index, inp.plan, w, b)
    assert E * Ce not in sizes and E * W2 in sizes, sizes
    assert hidden.requires_grad and not hmax.requires_grad
    hid = hidden.detach()
    assert torch.equal(hmax[0], hid.abs().max())
    assert rel(hid, inp.hidden) <= TOL
    grads = torch.autograd.grad((hidden * inp.g).sum(), [x, t, w, b])
    ref = _reference_backward(inp, inp.g.double() * _slope(hid))
    errs = {k: rel(v, ref[k]) for k, v in zip(("g_x", "g_table", "g_w_in", "g_b_in"), grads)}
    print(f"EDGE_HIDDEN_IDX small/autograd {errs}")
    assert all(v <= TOL for v in errs.values()), errs
