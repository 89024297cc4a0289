"""The gradient of the collapsed sparse-GP bound in the embeddings on the GPU (cgat_gp_fit_grad_inputs and gp_input_rows in
csrc/gpgrad.hip, bound_and_gradient(wrt_embeddings=True), cgat_amd.collapsed_bound, cgat_amd.deep_kernel_gradient; DESIGN
10e) against the fp64 restatement of tests/gp_input_grad_cases.py:

    grads["embeddings"] within gp_input_grad_cases.input_bound() (the project's 1e-4) of max |dF/dX| of fp64 autograd;
    the output's row stride, its padding and the rows behind it, rows of 1e30 behind X;
    two calls, and chunks of 64 rows against the default, bit for bit; colsum, d2sum and P bit for bit those of
    cgat_gp_fit_grad; the call without the keyword as before;
    collapsed_bound through X0 @ W against fp64 autograd in W; deep_kernel_gradient against one autograd graph over all
    batches; the refusals of the entry.

tests/test_gp_input_grad_cpu.py holds the recorded floors to the restatement."""
import pytest
import torch

import gp_grad_cases as Gc
import gp_input_grad_cases as Ic

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
NAMES = list(Ic.NAMES)
SENTINEL = -7.25


def _device_rows(X, pad, tail=0):
    """X on the device with a row stride of D + pad; the padding, and `tail` further rows behind X, hold 1e30."""
    buf = torch.empty(X.shape[0] + tail, X.shape[1] + pad, device=DEV).fill_(1e30)
    Xd = buf[:X.shape[0], :X.shape[1]]
    Xd.copy_(X)
    return Xd


def _pass(c, chunk_rows="case", tail=0):
    from cgat_amd import gp
    return gp._GradientPass("test", _device_rows(c["inp"]["X"], c["ldx_pad"], tail), c["y_norm"].to(DEV), c["inp"]["Z"],
                            c["chunk_rows"] if chunk_rows == "case" else chunk_rows)


def _sums(c, input_grad, chunk_rows="case", tail=0):
    """The sums of the data pass at the case's fp64 adjoints (and dX with `input_grad`), cloned."""
    p = _pass(c, chunk_rows, tail)
    p.stats.factor(c["s"], c["ell"], Gc.JITTER)
    out = p.sums(c["s"], c["ell"], 2.0 * c["adj"]["G_hat"], c["adj"]["g"], c["c"], input_grad=input_grad)
    return [t.clone() for t in out]


def _entry(c, p, dX, lddx, ztimg="own"):
    """cgat_gp_fit_grad_inputs on the operands of the _GradientPass `p` (factored) with the caller's output."""
    from cgat_amd import _lib
    from cgat_amd.ops import _ptr, _stream
    st = p.stats
    x, ops = st.x, st.ops
    w1timg = st.image(st.W1.T)
    g2img = st.image(2.0 * c["adj"]["G_hat"])
    g32 = c["adj"]["g"].to(torch.float32).to(DEV)
    zt = _ptr(ops["ztimg"]) if isinstance(ztimg, str) else ztimg
    with torch.cuda.device(x.device):
        rc = _lib.lib.cgat_gp_fit_grad_inputs(
            _ptr(x), x.stride(0), _ptr(st.y32), st.N, st.D, _ptr(ops["zimg"]), st.M, _ptr(ops["centroid"]), _ptr(ops["znorm"]),
            _ptr(st.w1img), _ptr(w1timg), _ptr(g2img), _ptr(g32), float(c["c"]), c["s"], 0.5 / (c["ell"] * c["ell"]), st.chunk,
            _ptr(p.colsum), _ptr(p.d2sum), _ptr(p.P), zt, None if dX is None else _ptr(dX), lddx, _ptr(st.ws), p.ws_bytes,
            _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("name", NAMES)
def test_embedding_gradient_parity(name):
    """M = D = 1, everything padded; three chunks of 64 rows with a partial last one (n150_m33_d5: the chunk offset of dX); an
    input row stride of D + 3 and D across 64 (n300_m96_d65); n1000_m129_d130; the largest M, the LDS tile full
    (n1100_m1024_d384); N below one tile."""
    c = Ic.case(name)
    sol, grads = _pass(c)(c["s"], c["ell"], Gc.JITTER, wrt_embeddings=True)
    assert set(grads) == set(Gc.GRADS) | {"embeddings"}
    dX = grads["embeddings"]
    assert dX.shape == (c["N"], c["D"]) and dX.dtype == torch.float32 and dX.device.type == "cuda" and dX.is_contiguous()
    assert not dX.requires_grad
    assert abs(sol["elbo"] - c["dense"]) <= Gc.ELBO_REL_BOUND * abs(c["dense"])
    err, scale = float((dX.cpu().to(torch.float64) - c["ref"]).abs().max()), float(c["ref"].abs().max())
    print(f"[gp-input-grad] {name}: dF/dX {err / scale:.3e} of max |dF/dX| = {scale:.3e} (bound {Ic.input_bound():.1e})")
    assert err <= Ic.input_bound() * scale
    # at the case's fp64 adjoints, as the fp32 floor is measured
    at64 = _sums(c, True)[3]
    err64 = float((at64.cpu().to(torch.float64) - c["ref"]).abs().max())
    print(f"[gp-input-grad] {name}: at the fp64 adjoints {err64 / scale:.3e}")
    assert err64 <= Ic.input_bound() * scale


@pytest.mark.parametrize("name", ["n300_m96_d65", "n150_m33_d5", "n31_m30_d7"])
def test_output_stride_padding_and_tail_rows(name):
    """The C entry with lddx = D + 3 and 64 rows behind the output: the padding columns and the tail rows keep their
    sentinel, the rows equal those of the contiguous call bit for bit; 64 rows of 1e30 behind X leave dX bit-identical."""
    c = Ic.case(name)
    N, D = c["N"], c["D"]
    plain = _sums(c, True)[3]
    p = _pass(c, tail=64)
    p.stats.factor(c["s"], c["ell"], Gc.JITTER)
    buf = torch.full((N + 64, D + 3), SENTINEL, device=DEV)
    assert _entry(c, p, buf, D + 3) == 0
    assert torch.equal(buf[:N, :D], plain) and bool(torch.isfinite(buf).all())
    assert bool((buf[:N, D:] == SENTINEL).all()) and bool((buf[N:] == SENTINEL).all())
    # a stride and a base that allow no 16-byte stores give the same bits as one that allows them
    wide = torch.full((N + 64, D + 4 - D % 4 + 4), SENTINEL, device=DEV)
    assert wide.stride(0) % 4 == 0 and _entry(c, p, wide, wide.stride(0)) == 0
    assert torch.equal(wide[:N, :D], plain) and bool((wide[:N, D:] == SENTINEL).all()) and bool((wide[N:] == SENTINEL).all())


def test_two_calls_bitwise_equal():
    c = Ic.case("n1100_m1024_d384")
    a, b = _sums(c, True), _sums(c, True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_chunks_do_not_change_a_row():
    """chunk_rows = 64 against the default: a row's dX depends only on its tile of 32 rows, and chunks start on tile
    boundaries."""
    for name in ("n150_m33_d5", "n300_m96_d65"):
        c = Ic.case(name)
        assert torch.equal(_sums(c, True, chunk_rows=64)[3], _sums(c, True, chunk_rows=None)[3])


@pytest.mark.parametrize("name", ["n150_m33_d5", "n1100_m1024_d384"])
def test_sums_are_those_of_the_plain_entry(name):
    c = Ic.case(name)
    plain, with_inputs = _sums(c, False), _sums(c, True)
    assert len(plain) == 3 and len(with_inputs) == 4
    assert all(torch.equal(a, b) for a, b in zip(plain, with_inputs))


def test_default_is_the_call_without_the_keyword():
    from cgat_amd import gp
    c = Ic.case("n300_m96_d65")
    args = (c["y_norm"].to(DEV), c["inp"]["Z"], c["s"], c["ell"])
    X = _device_rows(c["inp"]["X"], c["ldx_pad"])
    sol0, g0 = gp.bound_and_gradient(X, *args)
    sol1, g1 = gp.bound_and_gradient(X, *args, wrt_embeddings=False)
    sol2, g2 = gp.bound_and_gradient(X, *args, wrt_embeddings=True)
    assert set(g0) == set(g1) == set(Gc.GRADS) and set(g2) == set(Gc.GRADS) | {"embeddings"}
    for g in (g1, g2):
        assert torch.equal(g0["inducing_points"], g["inducing_points"])
        assert g0["log_lengthscale"] == g["log_lengthscale"] and g0["log_outputscale"] == g["log_outputscale"]
    assert sol0["elbo"] == sol1["elbo"] == sol2["elbo"]


@pytest.mark.parametrize("name", list(Ic.LINEAR_NAMES))
def test_collapsed_bound_backward_through_a_linear_map(name):
    """emb = X0 @ W on the device, bound.backward(): W.grad against fp64 autograd of dense_bound(X0 @ W) within four times
    what the eager fp32 arm shows (gp_input_grad_cases.weight_bound); the bound is fp64 and the solution's; twice the bound
    gives twice the gradient."""
    import cgat_amd as P
    lc = Ic.linear_case(name)
    X0, y = lc["X0"].to(DEV), lc["y_norm"].to(DEV)
    W = lc["W"].to(DEV).requires_grad_(True)
    bound, sol = P.collapsed_bound(X0 @ W, y, lc["Z"], lc["s"], lc["ell"], chunk_rows=lc["chunk_rows"])
    assert bound.dtype == torch.float64 and bound.dim() == 0 and bound.device.type == "cuda" and bound.requires_grad
    assert float(bound.detach()) == sol["elbo"]
    assert abs(sol["elbo"] - lc["elbo"]) <= Gc.ELBO_REL_BOUND * abs(lc["elbo"])
    bound.backward()
    once = W.grad.clone()
    assert once.dtype == torch.float32
    dev = Ic.deviation(once.cpu(), lc["ref"])
    print(f"[gp-input-grad] {name}: dF/dW {dev:.3e} (bound {Ic.weight_bound():.1e})")
    assert dev <= Ic.weight_bound()
    W.grad = None
    bound2, _ = P.collapsed_bound(X0 @ W, y, lc["Z"], lc["s"], lc["ell"], chunk_rows=lc["chunk_rows"])
    (2 * bound2).backward()
    assert torch.equal(W.grad, 2 * once)
    # embeddings without grad: a plain value
    plain, _ = P.collapsed_bound((X0 @ W).detach(), y, lc["Z"], lc["s"], lc["ell"], chunk_rows=lc["chunk_rows"])
    assert not plain.requires_grad and float(plain) == float(bound.detach())


@pytest.fixture(scope="module")
def deep_kernel():
    """The setup of tests/test_gp_head.py: a small CGAtNet, three synthetic batches of 4 graphs (N = 12), M = 5 inducing
    points taken from the embeddings, l = spread sqrt(D)."""
    import cgat_amd as P
    batches = []
    for seed in (8, 9, 10):
        b, roost = P.synthetic_batch(4, 20, 12, seed=seed)
        batches.append((b.to(DEV), tuple(t.to(DEV) for t in roost)))
    torch.manual_seed(1)
    net = P.CGAtNet(200, 64, 2, msg_heads=2, neighbor_number=12, update_edges=True).to(DEV)
    net.eval()
    with torch.no_grad():
        E = torch.cat([net(b, r, return_graph_embedding=True) for b, r in batches])
    N, D = E.shape
    Z = E[torch.randperm(N, generator=torch.Generator().manual_seed(3))[:5]].cpu().clone()
    spread = float((E - E.mean(0)).square().mean().sqrt())
    y = torch.randn(N, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    y = ((y - y.mean()) / y.std()).to(DEV)
    return dict(net=net, batches=batches, N=N, Z=Z, y=y, s=1.0, ell=spread * D ** 0.5)


def test_deep_kernel_gradient_equals_one_graph(deep_kernel):
    """Every parameter's .grad against one autograd graph that keeps all three forwards alive: both use the same dX and
    differ in the order of three fp32 addends, hence 1e-5 of each tensor's max-norm."""
    import cgat_amd as P
    k = deep_kernel
    net, batches, N = k["net"], k["batches"], k["N"]
    assert N == 12
    net.train()
    net.zero_grad(set_to_none=True)
    out = P.deep_kernel_gradient(net, batches, k["y"], k["Z"], k["s"], k["ell"])
    assert net.training                                              # restored
    assert set(out) == {"loss", "solution", "grads", "embeddings"} and set(out["grads"]) == set(Gc.GRADS)
    assert out["loss"] == -out["solution"]["elbo"] / N and out["embeddings"].shape[0] == N
    assert not out["embeddings"].requires_grad
    got = {n: (None if p.grad is None else p.grad.clone()) for n, p in net.named_parameters()}
    # a second call on zeroed grads: bit for bit
    net.zero_grad(set_to_none=True)
    again = P.deep_kernel_gradient(net, batches, k["y"], k["Z"], k["s"], k["ell"])
    assert again["loss"] == out["loss"]
    for n, p in net.named_parameters():
        assert (p.grad is None) == (got[n] is None) and (p.grad is None or torch.equal(p.grad, got[n])), n
    # the reference: one graph
    net.zero_grad(set_to_none=True)
    net.eval()
    E = torch.cat([net(b, r, return_graph_embedding=True) for b, r in batches])
    bound, sol = P.collapsed_bound(E, k["y"], k["Z"], k["s"], k["ell"])
    assert abs(sol["elbo"] - out["solution"]["elbo"]) <= 1e-6 * abs(sol["elbo"])
    bound.mul(-1.0 / N).backward()
    with_grad, worst = 0, (0.0, None)
    for n, p in net.named_parameters():
        assert (p.grad is None) == (got[n] is None), n
        if p.grad is None:
            continue
        scale = float(p.grad.abs().max())
        with_grad += scale > 0.0
        worst = max(worst, (float((p.grad - got[n]).abs().max()) / scale if scale else 0.0, n))
    print(f"[gp-input-grad] deep kernel: {with_grad} parameters with a gradient, worst deviation {worst[0]:.3e} ({worst[1]})")
    for n, p in net.named_parameters():
        if p.grad is not None:
            assert float((p.grad - got[n]).abs().max()) <= 1e-5 * float(p.grad.abs().max()), n
    assert with_grad > 0


def test_entry_refusals_leave_the_output_untouched():
    """A null dX, lddx < D and a misaligned Ztimg each return the argument error; nothing is written."""
    import ctypes as C
    c = Ic.case("n150_m33_d5")
    N, D = c["N"], c["D"]
    p = _pass(c)
    p.stats.factor(c["s"], c["ell"], Gc.JITTER)
    buf = torch.full((N, D), SENTINEL, device=DEV)
    for t in (p.colsum, p.d2sum, p.P):
        t.fill_(SENTINEL)
    assert _entry(c, p, None, D) == 1
    assert _entry(c, p, buf, D - 1) == 1
    assert _entry(c, p, buf, D, ztimg=C.c_void_p(p.stats.ops["ztimg"].data_ptr() + 4)) == 1
    assert _entry(c, p, buf, D, ztimg=None) == 1
    assert all(bool((t == SENTINEL).all()) for t in (buf, p.colsum, p.d2sum, p.P))
    assert _entry(c, p, buf, D) == 0 and not bool((buf == SENTINEL).any())
