"""cgat_edge_hidden_forward / cgat_edge_hidden_backward -- the operand-split first layer of the vector-attention node
layer -- against a plain fp64 reference of the same operation, on every route the backward's router can take.

Reference (float64, slot order t of the plan: dst_s = plan.dst_sorted, src_s = plan.src_sorted, perm = plan.dst_perm):

    m      = cat[x[dst_s], e[perm], x[src_s]]                      [E, 2C+Ce]
    pre    = m @ w_in.T + b_in ;  hidden = leaky_relu(pre, 0.01)
    gZ     = g_hidden * where(sign_source > 0, 1, 0.01)            (g_is_pre: gZ = g_pre)
    g_w_in = gZ.T @ m ;  g_b_in = gZ.sum(0) ;  g_m = gZ @ w_in
    g_x    = index_add(dst_s, g_m[:, :C]) + index_add(src_s, g_m[:, C+Ce:]) ;  g_e[perm] = g_m[:, C:C+Ce]

With g_is_pre = 0, sign_source is the hidden the GPU call returned (the branch it took), and every element whose sign
differs from that of the fp64 pre-activation must have |pre| <= 1e-5 max |pre|.  With g_is_pre = 1 there is no allowance.

Every comparison is max-norm relative at TOL = 2e-5 (the kernel-level bound of tests/test_hip_kernels.py, all arithmetic
modes); g_w_in is compared per column block [W_i | W_e | W_j].  The calls go through the raw C ABI on buffers the test
owns: outputs pre-filled with NaN, a workspace of exactly the queried size filled with 0xFF bytes and followed by a 4-KB
guard, inputs checked bit-unchanged, a second identical call checked bit-identical.  Each comparison prints its figure
before it asserts, as `EDGE_HIDDEN_REL <case>/<mode>[/<variant>] <output> <rel>` (shown by `pytest -s` or `-rA`): the
record of how far inside the bound each route sits.

Route table -- which case pins which route (cgat_amd.debug.edge_hidden_route) in which arithmetic mode.  Each GPU test
asserts its row before it computes, and test_route_table asserts the whole table without a GPU, so a moved threshold
(edge_ge_ksplit_groups, rowprog_max_rows, the alignment predicates) fails a named assertion instead of thinning coverage.
C = Ce = 128 unless stated; "24-bit" = f16x3c and bf16x6.

    case      N, E, W2           mode      forward  backward
    small     301, 701, 512      24-bit    fast     node_small_rows ge_launch gw_launch
                                 f16x3     fast     the same + have_scales node_scales
                                 f32       -        node_gemm ge_gemm gw_gemm
    ksplit    1101, 3001, 1536   24-bit    fast     node_ksplit ge_ksplit gw_launch
    launches  2101, 2501, 256    24-bit    fast     node_launches ge_launch gw_launch        (W2 = 256 has no K-split)
                                 f16x3     fast     the same + have_scales node_scales
    mixed     2101, 5003, 512    f16x3c    fast     node_ksplit ge_ksplit gw_launch
    widths    203, 1207, 192     f16x3c    -        node_gemm ge_gemm gw_gemm                (C = 64, Ce = 32)
                                 f32       -        node_gemm ge_gemm gw_gemm
    is_pre    small, launches    f16x3 with a maximum:     as the f16x3 rows above (have_scales node_scales)
              (g_is_pre = 1)     f16x3 without a maximum:  as the 24-bit rows above (no scales: the six-pass forms)
                                 f16x3c:                   as the 24-bit rows above
    empty     5, 0 and 0, 0; 512 f16x3c, f16x3: no route asserted; the calls succeed, every gradient is exactly 0
"""
import ctypes as C

import numpy as np
import pytest
import torch

TOL = 2e-5

SHAPES = {   # name: N, E, C, Ce, W2
    "small": (301, 701, 128, 128, 512),
    "ksplit": (1101, 3001, 128, 128, 1536),
    "launches": (2101, 2501, 128, 128, 256),
    "mixed": (2101, 5003, 128, 128, 512),
    "widths": (203, 1207, 64, 32, 192),
}
_GEMM = {"node_gemm", "ge_gemm", "gw_gemm"}
_SCALES = {"have_scales", "node_scales"}
_SMALL = {"node_small_rows", "ge_launch", "gw_launch"}
_KSPLIT = {"node_ksplit", "ge_ksplit", "gw_launch"}
_LAUNCHES = {"node_launches", "ge_launch", "gw_launch"}
FAST, SLOW = {"fast"}, set()
# (shape, mode): (forward routes, backward routes with g_is_pre = 0)
ROUTES = {
    ("small", "f16x3c"): (FAST, _SMALL), ("small", "bf16x6"): (FAST, _SMALL), ("small", "f16x3"): (FAST, _SMALL | _SCALES),
    ("small", "f32"): (SLOW, _GEMM),
    ("ksplit", "f16x3c"): (FAST, _KSPLIT), ("ksplit", "bf16x6"): (FAST, _KSPLIT),
    ("launches", "f16x3c"): (FAST, _LAUNCHES), ("launches", "bf16x6"): (FAST, _LAUNCHES),
    ("launches", "f16x3"): (FAST, _LAUNCHES | _SCALES),
    ("mixed", "f16x3c"): (FAST, _KSPLIT),
    ("widths", "f16x3c"): (SLOW, _GEMM), ("widths", "f32"): (SLOW, _GEMM),
}
# (shape, mode, has_absmax): backward routes with g_is_pre = 1
ROUTES_IS_PRE = {
    ("small", "f16x3", True): _SMALL | _SCALES, ("small", "f16x3", False): _SMALL, ("small", "f16x3c", False): _SMALL,
    ("launches", "f16x3", True): _LAUNCHES | _SCALES, ("launches", "f16x3", False): _LAUNCHES,
    ("launches", "f16x3c", False): _LAUNCHES,
}


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    d = b.abs().max().item()
    return (a - b).abs().max().item() / (d if d > 0 else 1.0)


def _assert_routes(shape, mode, g_is_pre=None, has_absmax=False):
    """The route row of (shape, mode) in the CURRENT arithmetic mode (the caller has set `mode`)."""
    from cgat_amd import debug, ops
    assert ops.get_bilinear_mode() == mode
    dims = SHAPES[shape]
    if g_is_pre is None:
        fwd, bwd = ROUTES[shape, mode]
        assert debug.edge_hidden_route(*dims) == fwd, (shape, mode, "forward")
        assert debug.edge_hidden_route(*dims, backward=True) == bwd, (shape, mode, "backward")
    else:
        want = ROUTES_IS_PRE[shape, mode, has_absmax]
        got = debug.edge_hidden_route(*dims, backward=True, g_is_pre=True, has_absmax=has_absmax)
        assert got == want, (shape, mode, "g_is_pre", has_absmax)


def test_route_table():
    """The whole table of the module docstring against cgat_debug_edge_hidden_route: host only, no GPU.  Also: every
    route the router has is pinned by at least one row in every mode it exists in, and refused arguments give 0."""
    from cgat_amd import debug, ops
    try:
        for (shape, mode) in ROUTES:
            ops.set_bilinear_mode(mode)
            _assert_routes(shape, mode)
        for (shape, mode, has_absmax) in ROUTES_IS_PRE:
            ops.set_bilinear_mode(mode)
            _assert_routes(shape, mode, True, has_absmax)
        ops.set_bilinear_mode("f16x3c")
        assert debug.edge_hidden_route(5, 5, 0, 128, 512) == set()
        assert debug.edge_hidden_route(-1, 5, 128, 128, 512, backward=True) == set()
    finally:
        ops.set_bilinear_mode(ops.DEFAULT_MODE)
    pinned = {}
    for (shape, mode), (_, bwd) in ROUTES.items():
        pinned.setdefault(mode, set()).update(bwd)
    for mode in ("f16x3c", "bf16x6"):      # the K-split forms exist in the 24-bit modes only; scales in f16x3 only
        assert pinned[mode] >= _SMALL | _KSPLIT | _LAUNCHES
    assert pinned["f16x3"] >= _SMALL | _LAUNCHES | _SCALES
    assert pinned["f32"] == _GEMM and pinned["f16x3c"] >= _GEMM


# ---------------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"
GUARD = 4096
_cache = {}


def _graph(N, E, seed):
    """An arbitrary directed graph: the last ~5 % of the atoms never receive, the first ~5 % never send, one hub holds
    E / 10 incoming edges, edges source-major."""
    rs = np.random.RandomState(seed)
    k = max(1, N // 20)
    src = rs.randint(k, N, size=E)
    dst = rs.randint(0, N - k, size=E)
    dst[:E // 10] = N // 3
    order = np.argsort(src, kind="stable")
    return torch.from_numpy(np.stack([src[order], dst[order]])).long()


class _Inputs:
    """The operands of one shape (shared by every mode and test: never written) and the fp64 forward of the reference."""

    def __init__(self, shape, e_scale):
        from cgat_amd import ops
        N, E, Cn, Ce, W2 = SHAPES[shape]
        assert N % 8 and E % 8 and N % 128 and E % 128
        D = 2 * Cn + Ce
        g = torch.Generator().manual_seed(N + E + W2)
        self.dims = (N, E, Cn, Ce, W2)
        self.x = torch.randn(N, Cn, generator=g).to(DEV)
        self.e = (torch.randn(E, Ce, generator=g) * e_scale).to(DEV)
        self.w = (torch.randn(W2, D, generator=g) * D ** -0.5).to(DEV)
        self.b = torch.randn(W2, generator=g).to(DEV)
        self.g = torch.randn(E, W2, generator=g).to(DEV)
        self.ei = _graph(N, E, N + E).to(DEV)
        self.plan = ops.EdgePlan(self.ei, N)
        p = self.plan
        self.dst_s, self.src_s, self.perm = p.dst_sorted.long(), p.src_sorted.long(), p.dst_perm.long()
        # the graph is what the docstring says: atoms without incoming / outgoing edges, a hub
        deg_in = torch.bincount(self.ei[1], minlength=N)
        assert int((deg_in == 0).sum()) >= N // 20 and int((torch.bincount(self.ei[0], minlength=N) == 0).sum()) >= N // 20
        assert int(deg_in.max()) >= E // 10
        xd = self.x.double()
        self.m = torch.cat([xd[self.dst_s], self.e.double()[self.perm], xd[self.src_s]], 1)
        self.pre = self.m @ self.w.double().t() + self.b.double()
        self.hidden = torch.nn.functional.leaky_relu(self.pre, 0.01)


def _inputs(shape, e_scale=1.0):
    key = (shape, e_scale)
    if key not in _cache:
        _cache[key] = _Inputs(shape, e_scale)
    return _cache[key]


def _slope(sign_source):
    """LeakyReLU'(0.01) in float64 on the branch `sign_source` took."""
    one = torch.ones((), dtype=torch.float64, device=sign_source.device)
    return torch.where(sign_source > 0, one, 0.01 * one)


def _reference_backward(inp, gZ):
    """gZ: float64 [E, W2], the gradient of the pre-activation."""
    N, E, Cn, Ce, W2 = inp.dims
    g_m = gZ @ inp.w.double()
    g_x = torch.zeros(N, Cn, dtype=torch.float64, device=DEV)
    g_x.index_add_(0, inp.dst_s, g_m[:, :Cn])
    g_x.index_add_(0, inp.src_s, g_m[:, Cn + Ce:])
    g_e = torch.empty(E, Ce, dtype=torch.float64, device=DEV)
    g_e[inp.perm] = g_m[:, Cn:Cn + Ce]
    return {"g_x": g_x, "g_e": g_e, "g_w_in": gZ.t() @ inp.m, "g_b_in": gZ.sum(0)}


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def _workspace(nbytes):
    return torch.full((int(nbytes) + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)


def _guard_intact(ws, nbytes):
    return bool((ws[int(nbytes):] == 0xFF).all())


def _call_forward(plan, dims, x, e, w, b):
    """One raw cgat_edge_hidden_forward on fresh NaN outputs and a fresh 0xFF workspace of exactly the queried size."""
    from cgat_amd import _lib
    N, E, Cn, Ce, W2 = dims
    hidden, hmax = _nan(E, W2), _nan(1)
    nbytes = _lib.lib.cgat_edge_hidden_forward_workspace_bytes(C.byref(plan.c), Cn, Ce, W2)
    ws = _workspace(nbytes)
    keep = [t.clone() for t in (x, e, w, b)]
    _lib.check(_lib.lib.cgat_edge_hidden_forward(C.byref(plan.c), Cn, Ce, W2, _ptr(w), _ptr(b), _ptr(x), _ptr(e),
                                                 _ptr(hidden), _ptr(hmax), _ptr(ws), nbytes, None),
               "cgat_edge_hidden_forward")
    torch.cuda.synchronize()
    assert _guard_intact(ws, nbytes), "forward wrote behind its workspace"
    assert all(torch.equal(a, k) for a, k in zip((x, e, w, b), keep)), "forward changed an input"
    assert bool(torch.isfinite(hidden).all()) and bool(torch.isfinite(hmax).all())
    return hidden, hmax


def _call_backward(plan, dims, x, e, w, hidden, g_hidden, g_is_pre=False, absmax=None):
    from cgat_amd import _lib
    N, E, Cn, Ce, W2 = dims
    out = {"g_x": _nan(N, Cn), "g_e": _nan(E, Ce), "g_w_in": _nan(W2, 2 * Cn + Ce), "g_b_in": _nan(W2)}
    nbytes = _lib.lib.cgat_edge_hidden_backward_workspace_bytes(C.byref(plan.c), Cn, Ce, W2)
    ws = _workspace(nbytes)
    ins = (x, e, w, hidden, g_hidden) + (() if absmax is None else (absmax,))
    keep = [t.clone() for t in ins]
    _lib.check(_lib.lib.cgat_edge_hidden_backward(C.byref(plan.c), Cn, Ce, W2, _ptr(w), _ptr(x), _ptr(e), _ptr(hidden),
                                                  _ptr(g_hidden), 1 if g_is_pre else 0,
                                                  None if absmax is None else _ptr(absmax), _ptr(out["g_x"]),
                                                  _ptr(out["g_e"]), _ptr(out["g_w_in"]), _ptr(out["g_b_in"]), _ptr(ws),
                                                  nbytes, None), "cgat_edge_hidden_backward")
    torch.cuda.synchronize()
    assert _guard_intact(ws, nbytes), "backward wrote behind its workspace"
    assert all(torch.equal(a, k) for a, k in zip(ins, keep)), "backward changed an input"
    for name, t in out.items():
        assert bool(torch.isfinite(t).all()), f"{name} has elements that are not finite (or were never written)"
    return out


def _assert_flips_near_zero(inp, hidden):
    """Where the GPU took the other LeakyReLU branch than the fp64 pre-activation, that pre-activation is ~ 0."""
    flips = (hidden > 0) != (inp.pre > 0)
    worst = float(inp.pre.abs()[flips].max()) if bool(flips.any()) else 0.0
    assert worst <= 1e-5 * float(inp.pre.abs().max()), ("a LeakyReLU branch differs away from zero", worst)


def _forward_checked(inp, tag):
    """Forward twice (bit-identical), against fp64; returns the GPU hidden."""
    hidden, hmax = _call_forward(inp.plan, inp.dims, inp.x, inp.e, inp.w, inp.b)
    again, hmax2 = _call_forward(inp.plan, inp.dims, inp.x, inp.e, inp.w, inp.b)
    assert torch.equal(hidden, again) and torch.equal(hmax, hmax2), "two identical forward calls differ"
    r = rel(hidden, inp.hidden)
    print(f"EDGE_HIDDEN_REL {tag} hidden {r:.3e}")
    assert r <= TOL, ("hidden", r)
    assert torch.equal(hmax[0], hidden.abs().max()), (float(hmax), float(hidden.abs().max()))
    _assert_flips_near_zero(inp, hidden)
    return hidden


def _compare_backward(out, ref, Cn, Ce, tag):
    blocks = {"g_w_in[W_i]": slice(0, Cn), "g_w_in[W_e]": slice(Cn, Cn + Ce), "g_w_in[W_j]": slice(Cn + Ce, None)}
    errs = {k: rel(out[k], ref[k]) for k in ("g_x", "g_e", "g_b_in")}
    errs.update({k: rel(out["g_w_in"][:, s], ref["g_w_in"][:, s]) for k, s in blocks.items()})
    for k, v in errs.items():
        print(f"EDGE_HIDDEN_REL {tag} {k} {v:.3e}")
    assert all(v <= TOL for v in errs.values()), errs


def _backward_checked(inp, hidden, g_hidden, tag, g_is_pre=False, absmax=None):
    """Backward twice (bit-identical), against the fp64 reference on the branch the GPU forward took."""
    args = (inp.plan, inp.dims, inp.x, inp.e, inp.w, hidden, g_hidden, g_is_pre, absmax)
    out = _call_backward(*args)
    again = _call_backward(*args)
    assert all(torch.equal(out[k], again[k]) for k in out), "two identical backward calls differ"
    gZ = g_hidden.double() if g_is_pre else g_hidden.double() * _slope(hidden)
    _, _, Cn, Ce, _ = inp.dims
    _compare_backward(out, _reference_backward(inp, gZ), Cn, Ce, tag)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", list(ROUTES), ids=lambda v: v)
def test_edge_hidden_vs_fp64(shape, mode):
    """Forward and backward (g_is_pre = 0) of every row of the route table, at unit-scale operands."""
    from cgat_amd import ops
    ops.set_bilinear_mode(mode)
    try:
        _assert_routes(shape, mode)
        inp = _inputs(shape)
        hidden = _forward_checked(inp, f"{shape}/{mode}")
        _backward_checked(inp, hidden, inp.g, f"{shape}/{mode}")
    finally:
        ops.set_bilinear_mode(ops.DEFAULT_MODE)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode,has_absmax", list(ROUTES_IS_PRE), ids=lambda v: str(v))
def test_edge_hidden_backward_g_is_pre(shape, mode, has_absmax):
    """g_is_pre = 1: g_hidden is the pre-activation gradient itself and is read in place (it must come back bit-identical,
    which _call_backward checks); gpre_absmax, where given, is its exact maximum computed by torch."""
    from cgat_amd import ops
    ops.set_bilinear_mode(mode)
    try:
        _assert_routes(shape, mode, True, has_absmax)
        inp = _inputs(shape)
        hidden, _ = _call_forward(inp.plan, inp.dims, inp.x, inp.e, inp.w, inp.b)
        absmax = inp.g.abs().max().reshape(1) if has_absmax else None
        _backward_checked(inp, hidden, inp.g, f"{shape}/{mode}/is_pre{'+max' if has_absmax else ''}", True, absmax)
    finally:
        ops.set_bilinear_mode(ops.DEFAULT_MODE)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["g*1e-6", "g*1e3", "e*1e-3"])
@pytest.mark.parametrize("mode", ["f16x3", "f16x3c"])
def test_edge_hidden_operand_scales(mode, variant):
    """The `launches` shape with gradients far below / above unit scale and a small edge_attr: every result is held to
    2e-5 of its OWN maximum, so the per-tensor power-of-two scales of the f16x3 mode must carry the range (a real
    backward's gradients sit near the small end).  f16x3c is the control.  In f16x3 the g_is_pre = 1 form runs on the same
    operands with the exact maximum."""
    from cgat_amd import ops
    ops.set_bilinear_mode(mode)
    try:
        _assert_routes("launches", mode)
        inp = _inputs("launches", 1e-3 if variant == "e*1e-3" else 1.0)
        g = inp.g * {"g*1e-6": 1e-6, "g*1e3": 1e3, "e*1e-3": 1.0}[variant]
        tag = f"launches/{mode}/{variant}"
        hidden = _forward_checked(inp, tag)
        _backward_checked(inp, hidden, g, tag)
        if mode == "f16x3":
            _assert_routes("launches", mode, True, True)
            _backward_checked(inp, hidden, g, tag + "/is_pre+max", True, g.abs().max().reshape(1))
    finally:
        ops.set_bilinear_mode(ops.DEFAULT_MODE)


@pytest.mark.gpu
def test_edge_hidden_gradient_outlier_f16x3():
    """One element of g_hidden 4 096 times the largest other one (f16x3, `launches` shape): the per-tensor scale is set by
    the outlier and everything else sits twelve bits below it.  The tolerance stays global max-norm."""
    from cgat_amd import ops
    ops.set_bilinear_mode("f16x3")
    try:
        _assert_routes("launches", "f16x3")
        inp = _inputs("launches")
        hidden, _ = _call_forward(inp.plan, inp.dims, inp.x, inp.e, inp.w, inp.b)
        g = inp.g.clone()
        g[1234, 77] = 0.0
        g[1234, 77] = 4096.0 * float(g.abs().max())
        _backward_checked(inp, hidden, g, "launches/f16x3/outlier")
    finally:
        ops.set_bilinear_mode(ops.DEFAULT_MODE)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f16x3", "f16x3c"])
def test_edge_hidden_zero_gradient(mode):
    """All-zero g_hidden (`launches` shape): every gradient is exactly zero and finite -- a per-tensor maximum of 0 must
    not turn into a scale of infinity."""
    from cgat_amd import ops
    ops.set_bilinear_mode(mode)
    try:
        _assert_routes("launches", mode)
        inp = _inputs("launches")
        hidden, _ = _call_forward(inp.plan, inp.dims, inp.x, inp.e, inp.w, inp.b)
        out = _call_backward(inp.plan, inp.dims, inp.x, inp.e, inp.w, hidden, torch.zeros_like(inp.g))
        for name, t in out.items():
            assert float(t.abs().max()) == 0.0, name
    finally:
        ops.set_bilinear_mode(ops.DEFAULT_MODE)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [5, 0])
@pytest.mark.parametrize("mode", ["f16x3c", "f16x3"])
def test_edge_hidden_empty(mode, N):
    """No edges (and no atoms): the calls succeed, every gradient is written and exactly 0, hidden_absmax is 0."""
    from cgat_amd import ops
    ops.set_bilinear_mode(mode)
    try:
        dims = (N, 0, 128, 128, 512)
        g = torch.Generator().manual_seed(5)
        x, e = torch.randn(N, 128, generator=g).to(DEV), torch.zeros(0, 128, device=DEV)
        w = (torch.randn(512, 384, generator=g) * 384 ** -0.5).to(DEV)
        b = torch.randn(512, generator=g).to(DEV)
        plan = ops.EdgePlan(torch.zeros(2, 0, dtype=torch.long, device=DEV), N)
        hidden, hmax = _call_forward(plan, dims, x, e, w, b)
        assert hidden.shape == (0, 512) and float(hmax) == 0.0
        out = _call_backward(plan, dims, x, e, w, hidden, torch.zeros(0, 512, device=DEV))
        for name, t in out.items():
            assert t.numel() == 0 or float(t.abs().max()) == 0.0, name
    finally:
        ops.set_bilinear_mode(ops.DEFAULT_MODE)


@pytest.mark.gpu
def test_edge_hidden_autograd_wrapper():
    """ops.EdgeHiddenFn through autograd at the `small` shape against the same reference: the wrapper's argument order,
    its g_is_pre = 0 call, and hmax as a non-differentiable output."""
    from cgat_amd import ops
    ops.set_bilinear_mode(ops.DEFAULT_MODE)
    try:
        inp = _inputs("small")
        x, e, w, b = (t.clone().requires_grad_(True) for t in (inp.x, inp.e, inp.w, inp.b))
        hidden, hmax = ops.EdgeHiddenFn.apply(x, e, inp.plan, w, b)
        assert hidden.requires_grad and not hmax.requires_grad
        hid = hidden.detach()
        assert torch.equal(hmax[0], hid.abs().max())
        assert rel(hid, inp.hidden) <= TOL
        _assert_flips_near_zero(inp, hid)
        grads = torch.autograd.grad((hidden * inp.g).sum(), [x, e, w, b])
        out = dict(zip(("g_x", "g_e", "g_w_in", "g_b_in"), grads))
        _, _, Cn, Ce, _ = inp.dims
        _compare_backward(out, _reference_backward(inp, inp.g.double() * _slope(hid)), Cn, Ce, "small/autograd")
    finally:
        ops.set_bilinear_mode(ops.DEFAULT_MODE)
