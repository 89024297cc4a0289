"""Attention pooling with a dropout keep-mask (cgat_segment_attention_pool_dropout_*, the keep path of
ops.AttentionPoolFn; csrc/segment.hip) against the reference's sequence in fp64 on the CPU -- segment softmax with +eps,
times the keep-mask, times the message, index_add (CGAT.py:323-329) -- and the exact properties the layers rely on.

Segments: 37 of 0-29 rows, among them an empty one, one whose rows are all dropped and one of 3 001 rows (odd: many
rounds of the kernels' batched row requests plus a tail).  Tolerances: those of test_segment_attention_pool."""
import ctypes as C

import pytest
import torch

from test_hip_kernels import TOL, rel

pytestmark = pytest.mark.gpu

S, EMPTY, DROPPED, LONG = 37, 5, 11, 20
SHAPES = [(384, 384), (640, 640), (384, 3), (640, 5), (48, 3), (16, 1)]        # (F, aF)
EPS = 1e-16


@pytest.fixture(scope="module")
def env():
    from cgat_amd import _lib, ops
    return _lib, ops, torch.device("cuda:0")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _case(ops, dev, F, aF, permuted, indexed, p, seed=0):
    """Operands on the device plus everything the fp64 reference needs.  `keep_rows` is the mask in OPERAND row order
    (what the reference multiplies with); `keep` is what the kernel gets: the same rows, or -- `indexed` -- those rows
    stored in an unrelated order and reached through keep_idx (CSR position t -> keep row keep_idx[t])."""
    g = torch.Generator().manual_seed(1000 * F + 10 * aF + seed)
    counts = torch.randint(0, 30, (S,), generator=g)
    counts[EMPTY], counts[DROPPED], counts[LONG] = 0, 7, 3001
    seg = torch.repeat_interleave(torch.arange(S), counts)
    R = int(seg.numel())
    if permuted:
        seg = seg[torch.randperm(R, generator=g)]                      # rows in arbitrary order, reached through ridx
    plan = ops.SegmentPlan(seg.to(dev), S)
    ridx = plan.perm if permuted else None
    a = 3 * torch.randn(R, aF, generator=g)
    m = torch.randn(R, F, generator=g)
    keep_rows = (torch.rand(R, aF, generator=g) >= p).float() / (1.0 - p)
    keep_rows[seg == DROPPED] = 0.0
    keep, keep_idx = keep_rows, None
    if indexed:
        oper = plan.perm.cpu().long() if permuted else torch.arange(R)   # operand row of CSR position t
        q = torch.randperm(R, generator=g)
        keep = torch.empty_like(keep_rows)
        keep[q] = keep_rows[oper]
        keep_idx = q.to(torch.int32).to(dev)
    return dict(S=S, R=R, F=F, aF=aF, seg=seg, rowptr=plan.rowptr, ridx=ridx, a=a.to(dev), m=m.to(dev), keep=keep.to(dev),
                keep_idx=keep_idx, keep_rows=keep_rows)


def _reference(c, cot):
    """fp64, the reference's sequence written out; gradients from autograd."""
    seg, aF, F = c["seg"], c["aF"], c["F"]
    R = c["R"]
    ad = c["a"].detach().double().cpu().requires_grad_(True)
    md = c["m"].detach().double().cpu().requires_grad_(True)
    mx = torch.full((S, aF), -float("inf"), dtype=torch.float64).scatter_reduce(0, seg.view(-1, 1).expand(R, aF),
                                                                                  ad.detach(), "amax")
    ex = (ad - mx[seg]).exp()
    alpha = ex / (torch.zeros(S, aF, dtype=torch.float64).index_add(0, seg, ex) + EPS)[seg]      # softmax(+eps)
    alpha = alpha * c["keep_rows"].double()                                                       # F.dropout
    out = torch.zeros(S, F, dtype=torch.float64).index_add(0, seg, alpha.repeat_interleave(F // aF, dim=1) * md)
    g_a, g_m = torch.autograd.grad((out * cot.double().cpu()).sum(), [ad, md])
    return out.detach(), g_a, g_m


def _nan(*shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def _forward(lib, c, keep="case", keep_idx="case"):
    """Through the C ABI into NaN-filled outputs.  keep=None: the existing entry point without a mask."""
    dev = c["a"].device
    out, out_lo = _nan(c["S"], c["F"], dev=dev), _nan(c["S"], c["F"], dev=dev)
    mx, inv = _nan(c["S"], c["aF"], dev=dev), _nan(c["S"], c["aF"], dev=dev)
    k = c["keep"] if isinstance(keep, str) else keep
    ki = c["keep_idx"] if isinstance(keep_idx, str) else keep_idx
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if k is None:
        rc = lib.cgat_segment_attention_pool_forward(_ptr(c["a"]), c["aF"], None, _ptr(c["m"]), c["F"], _ptr(c["rowptr"]),
                                                     _ptr(c["ridx"]), c["S"], c["F"], EPS, _ptr(out), _ptr(mx), _ptr(inv),
                                                     _ptr(out_lo), st)
    else:
        rc = lib.cgat_segment_attention_pool_dropout_forward(_ptr(c["a"]), c["aF"], _ptr(k), _ptr(ki), _ptr(c["m"]), c["F"],
                                                             _ptr(c["rowptr"]), _ptr(c["ridx"]), c["S"], c["F"], EPS,
                                                             _ptr(out), _ptr(mx), _ptr(inv), _ptr(out_lo), st)
    assert rc == 0, lib.cgat_last_error()
    return out, mx, inv, out_lo


def _backward(lib, c, fwd, cot, keep="case", keep_idx="case"):
    dev = c["a"].device
    out, mx, inv, out_lo = fwd
    g_a, g_m = _nan(c["R"], c["aF"], dev=dev), _nan(c["R"], c["F"], dev=dev)
    k = c["keep"] if isinstance(keep, str) else keep
    ki = c["keep_idx"] if isinstance(keep_idx, str) else keep_idx
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if k is None:
        rc = lib.cgat_segment_attention_pool_backward(_ptr(c["a"]), c["aF"], None, _ptr(c["m"]), c["F"], _ptr(c["rowptr"]),
                                                      _ptr(c["ridx"]), c["S"], c["F"], _ptr(out), _ptr(mx), _ptr(inv),
                                                      _ptr(out_lo), _ptr(cot), _ptr(g_a), _ptr(g_m), c["F"], None, st)
    else:
        rc = lib.cgat_segment_attention_pool_dropout_backward(_ptr(c["a"]), c["aF"], _ptr(k), _ptr(ki), _ptr(c["m"]),
                                                              c["F"], _ptr(c["rowptr"]), _ptr(c["ridx"]), c["S"], c["F"],
                                                              _ptr(out), _ptr(mx), _ptr(inv), _ptr(out_lo), _ptr(cot),
                                                              _ptr(g_a), _ptr(g_m), c["F"], st)
    assert rc == 0, lib.cgat_last_error()
    return g_a, g_m


def _biteq(x, y):
    return torch.equal(x.view(torch.int32), y.view(torch.int32))


def _cot(c, seed=7):
    return torch.randn(c["S"], c["F"], generator=torch.Generator().manual_seed(seed)).to(c["a"].device)


@pytest.mark.parametrize("p", [0.3, 0.9])
@pytest.mark.parametrize("permuted,indexed", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["csr", "csr-keepidx", "ridx", "ridx-keepidx"])
@pytest.mark.parametrize("F,aF", SHAPES)
def test_parity_with_the_fp64_sequence(env, F, aF, permuted, indexed, p):
    """Through the op (forward and autograd) and, on the same operands, through the C ABI: both against fp64."""
    _lib, ops, dev = env
    c = _case(ops, dev, F, aF, permuted, indexed, p)
    a, m = c["a"].clone().requires_grad_(True), c["m"].clone().requires_grad_(True)
    assert ops.AttentionPoolFn.supported(a, m)
    cot = _cot(c)
    keep = c["keep"].clone().requires_grad_(True)
    out = ops.AttentionPoolFn.apply(a, None, m, c["rowptr"], c["ridx"], EPS, keep, c["keep_idx"])
    g_a, g_m, g_keep = torch.autograd.grad((out * cot).sum(), [a, m, keep], allow_unused=True)
    assert g_keep is None                                               # the mask gets no gradient
    ref, ref_ga, ref_gm = _reference(c, cot)
    errs = {"out": rel(out, ref), "g_a": rel(g_a, ref_ga), "g_m": rel(g_m, ref_gm)}
    print(f"F={F} aF={aF} permuted={permuted} indexed={indexed} p={p}: {errs}")
    assert errs["out"] <= TOL, errs
    assert errs["g_a"] <= 5e-5 and errs["g_m"] <= 5e-5, errs
    # the segment without rows and the segment whose rows are all dropped: exactly zero
    assert float(out.detach()[EMPTY].abs().max()) == 0.0 and float(out.detach()[DROPPED].abs().max()) == 0.0
    assert float(g_m[(c["seg"] == DROPPED).to(dev)].abs().max()) == 0.0
    # the C ABI on NaN-filled outputs gives what the op gave, bit for bit
    fwd = _forward(_lib.lib, c)
    cg_a, cg_m = _backward(_lib.lib, c, fwd, cot)
    assert _biteq(fwd[0], out.detach()) and _biteq(cg_a, g_a) and _biteq(cg_m, g_m)
    assert not any(bool(torch.isnan(t).any()) for t in (*fwd, cg_a, cg_m))


@pytest.mark.parametrize("permuted,indexed", [(False, False), (True, True)], ids=["csr", "ridx-keepidx"])
@pytest.mark.parametrize("F,aF", SHAPES)
def test_exact_invariants(env, F, aF, permuted, indexed):
    _lib, ops, dev = env
    lib = _lib.lib
    c = _case(ops, dev, F, aF, permuted, indexed, 0.3, seed=1)
    cot = _cot(c)
    before = {k: c[k].clone() for k in ("a", "m", "keep", "rowptr")}
    # keep == 1 everywhere: every output of both directions equals the op without a mask, bit for bit
    ones = torch.ones_like(c["keep"])
    plain_f = _forward(lib, c, keep=None)
    plain_b = _backward(lib, c, plain_f, cot, keep=None)
    ones_f = _forward(lib, c, keep=ones)
    ones_b = _backward(lib, c, ones_f, cot, keep=ones)
    for name, x, y in zip(("out", "mx", "inv", "out_lo", "g_a", "g_m"), ones_f + ones_b, plain_f + plain_b):
        assert not bool(torch.isnan(x).any()), name
        assert _biteq(x, y), name
    # keep == 0 everywhere: out and g_m are exactly zero, the normaliser is untouched
    zeros = torch.zeros_like(c["keep"])
    zero_f = _forward(lib, c, keep=zeros)
    zero_b = _backward(lib, c, zero_f, cot, keep=zeros)
    assert float(zero_f[0].abs().max()) == 0.0 and float(zero_b[1].abs().max()) == 0.0
    assert _biteq(zero_f[1], plain_f[1]) and _biteq(zero_f[2], plain_f[2])
    assert not bool(torch.isnan(zero_b[0]).any())
    # two calls agree bit for bit, and the mask leaves maximum and normaliser alone
    f1 = _forward(lib, c)
    b1 = _backward(lib, c, f1, cot)
    f2 = _forward(lib, c)
    b2 = _backward(lib, c, f2, cot)
    for name, x, y in zip(("out", "mx", "inv", "out_lo", "g_a", "g_m"), f1 + b1, f2 + b2):
        assert not bool(torch.isnan(x).any()), name
        assert _biteq(x, y), name
    assert _biteq(f1[1], plain_f[1]) and _biteq(f1[2], plain_f[2])
    # inputs are unchanged
    for k, v in before.items():
        assert torch.equal(c[k], v), k


def test_argument_checks(env):
    _lib, ops, dev = env
    lib = _lib.lib
    c = _case(ops, dev, 384, 3, False, False, 0.3)
    cv = _case(ops, dev, 48, 48, False, False, 0.3)
    a, m = c["a"].clone().requires_grad_(True), c["m"]
    mult = torch.ones(c["R"], 1, device=dev)
    torch.cuda.synchronize()
    n0 = ops.prof_launches()
    with pytest.raises(ValueError, match="multiplier"):                 # keep together with mult: an error, not a launch
        ops.AttentionPoolFn.apply(a, mult, m, c["rowptr"], None, EPS, c["keep"], None)
    with pytest.raises(ValueError, match="shape"):
        ops.AttentionPoolFn.apply(a, None, m, c["rowptr"], None, EPS, c["keep"][:, :1], None)
    with pytest.raises(TypeError, match="keep_idx"):
        ops.AttentionPoolFn.apply(a, None, m, c["rowptr"], None, EPS, c["keep"], torch.arange(c["R"], device=dev))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = torch.empty(S, 384, device=dev)
    mx, inv = torch.empty(S, 3, device=dev), torch.empty(S, 3, device=dev)
    # no mask at all, and a shape the kernels do not take (F / aF = 12 is no power of two times four)
    assert lib.cgat_segment_attention_pool_dropout_forward(_ptr(c["a"]), 3, None, None, _ptr(m), 384, _ptr(c["rowptr"]),
                                                           None, S, 384, EPS, _ptr(out), _ptr(mx), _ptr(inv), None, st) != 0
    assert b"keep" in lib.cgat_last_error()
    assert lib.cgat_segment_attention_pool_dropout_forward(_ptr(c["a"]), 32, _ptr(c["keep"]), None, _ptr(m), 384,
                                                           _ptr(c["rowptr"]), None, S, 384, EPS, _ptr(out), _ptr(mx),
                                                           _ptr(inv), None, st) != 0
    # one logit per feature: the mask is read as float4, so it must be 16-byte aligned
    odd = torch.ones(cv["R"] * 48 + 1, device=dev)[1:].view(cv["R"], 48)
    out48, mx48, inv48 = (torch.empty(S, 48, device=dev) for _ in range(3))
    assert lib.cgat_segment_attention_pool_dropout_forward(_ptr(cv["a"]), 48, _ptr(odd), None, _ptr(cv["m"]), 48,
                                                           _ptr(cv["rowptr"]), None, S, 48, EPS, _ptr(out48), _ptr(mx48),
                                                           _ptr(inv48), None, st) != 0
    assert b"aligned" in lib.cgat_last_error()
    # S == 0: OK, nothing launched
    assert lib.cgat_segment_attention_pool_dropout_forward(_ptr(c["a"]), 3, _ptr(c["keep"]), None, _ptr(m), 384,
                                                           _ptr(c["rowptr"]), None, 0, 384, EPS, _ptr(out), _ptr(mx),
                                                           _ptr(inv), None, st) == 0
    assert lib.cgat_segment_attention_pool_dropout_backward(_ptr(c["a"]), 3, _ptr(c["keep"]), None, _ptr(m), 384,
                                                            _ptr(c["rowptr"]), None, 0, 384, _ptr(out), _ptr(mx), _ptr(inv),
                                                            None, _ptr(out), _ptr(out), None, 384, st) == 0
    assert ops.prof_launches() == n0
