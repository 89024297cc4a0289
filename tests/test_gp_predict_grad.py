"""The derivative of the sparse-GP head's prediction in its input on the GPU (cgat_gp_predict_backward in csrc/gpback.hip,
cgat_amd.predictive_backward, the autograd surface of GPHead.latent / predict / uncertainty, GPHead.nlpd)
against the fp64 restatement of tests/gp_predict_grad_cases.py:

    dL/dX of every case and arm within gp_predict_grad_cases.gradient_bound(arm) (the project's 1e-4) of the arm's own
    max |dL/dX| of fp64 autograd;
    the outputs carry a grad_fn exactly where autograd records, torch.autograd.grad equals the functional form bit for bit,
    the forward without grad is the forward with it bit for bit;
    chunks of 32, 64 and 288 rows and two calls, bit for bit; strided embeddings and a strided output through the C entry;
    head.nlpd(X0 @ W, y, noise).mean().backward() against fp64 autograd in W; the refusals of the entry.

tests/test_gp_predict_grad_cpu.py holds the recorded floors to the restatement."""
import ctypes as C

import pytest
import torch

import gp_predict_grad_cases as Pc

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
NAMES = list(Pc.NAMES)
SENTINEL = -7.25
OUTPUTS = ("mean_f", "var_f", "pred", "lower", "upper")


def _head(p):
    import cgat_amd as P
    return P.GPHead.from_tensors(p).to(DEV)


def _device_rows(X):
    """X on the device with its row stride; the padding holds 1e30."""
    Xd = torch.empty(X.shape[0], X.stride(0), device=DEV).fill_(1e30)[:, :X.shape[1]]
    Xd.copy_(X)
    assert Xd.stride(0) == X.stride(0)
    return Xd


def _on_device(g):
    return None if g is None else g.to(torch.float32).to(DEV)


def _weights(G, seed=21):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(G, generator=g).to(DEV) for k in OUTPUTS}


def _entry(head, x, gm, gv, dX, lddx, chunk=32768, M=None, ztimg="own", g2img="own", ws_bytes=None):
    """cgat_gp_predict_backward on the images of `head` with the caller's upstreams, output and workspace size."""
    from cgat_amd import _lib
    from cgat_amd.ops import _ptr, _stream
    im, back = head.prepare(), head.prepare_backward()
    G, D = x.shape
    need = _lib.lib.cgat_gp_predict_backward_workspace_bytes(G, im["M"], D, chunk)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    with torch.cuda.device(x.device):
        rc = _lib.lib.cgat_gp_predict_backward(
            _ptr(x), x.stride(0), G, D, _ptr(im["zimg"]), im["M"] if M is None else M, _ptr(im["centroid"]),
            _ptr(im["znorm"]), _ptr(back["w1img"]), _ptr(back["w1timg"]),
            _ptr(back["g2img"]) if isinstance(g2img, str) else g2img, _ptr(back["m"]), None if gm is None else _ptr(gm),
            None if gv is None else _ptr(gv), im["s"], im["inv_two_l2"], chunk,
            _ptr(back["ztimg"]) if isinstance(ztimg, str) else ztimg, _ptr(dX), lddx, _ptr(ws),
            need if ws_bytes is None else ws_bytes, _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("name", NAMES)
def test_gradient_parity(name):
    """Ragged last row tile and M, D off the tile sizes (g257_m37_d5); M padded to the full tile (g33_m1000_d128); the LDS
    tile full and a row stride larger than D (g300_m1024_d384); D across ten staged panels with the doubled lengthscale
    (g65_m129_d640); one row, one inducing point, one column; ZeroMean.  Each arm against its own max-norm."""
    import cgat_amd as P
    c = Pc.case(name)
    head, Xd = _head(c["p"]), _device_rows(c["X"])
    for arm in Pc.ARMS:
        a = c["arms"][arm]
        dX = P.predictive_backward(head, Xd, _on_device(a["gm"]), _on_device(a["gv"]))
        assert dX.shape == (c["G"], c["D"]) and dX.dtype == torch.float32 and dX.device.type == "cuda"
        assert dX.is_contiguous() and not dX.requires_grad
        dev = Pc.deviation(dX.cpu(), a["ref"])
        print(f"[gp-predict-grad] {name} {arm}: dL/dX {dev:.3e} of max |dL/dX| = {float(a['ref'].abs().max()):.3e} "
              f"(bound {Pc.gradient_bound(arm):.1e})")
        assert dev <= Pc.gradient_bound(arm), (arm, dev)


def test_autograd_surface():
    """With embeddings that require grad every output has a grad_fn and torch.autograd.grad of a weighted sum of the
    outputs is predictive_backward fed with latent_adjoints, bit for bit: of latent's two, of predict's three, and of all
    five of the one call both make.  Under no_grad, or with a plain tensor, the outputs are those bits without a graph.
    A second derivative raises."""
    import cgat_amd as P
    c = Pc.case("g257_m37_d5")
    head, Xd = _head(c["p"]), _device_rows(c["X"])
    std, w = head.prepare()["std"], _weights(c["G"])
    X = Xd.clone().requires_grad_(True)
    with_grad = dict(zip(OUTPUTS, head.latent(X) + head.predict(X)))
    unc = head.uncertainty(X)
    assert all(v.grad_fn is not None and v.requires_grad for v in with_grad.values()) and unc.grad_fn is not None
    assert torch.equal(unc, with_grad["upper"] - with_grad["pred"])

    def functional(keys, var_f):
        gm, gv = P.latent_adjoints(tuple(w[k] if k in keys else None for k in OUTPUTS), var_f, std)
        return P.predictive_backward(head, Xd, gm, gv)

    for keys, outs in ((OUTPUTS[:2], head.latent(X)), (OUTPUTS[2:], head.predict(X)), (OUTPUTS, head._run(X, True))):
        named = dict(zip(keys, outs))
        got, = torch.autograd.grad(sum((w[k] * named[k]).sum() for k in keys), X)
        assert got.shape == X.shape and got.dtype == torch.float32
        assert torch.equal(got, functional(keys, with_grad["var_f"].detach())), keys
    # uncertainty alone: the variance arm through upper, pred's share of the mean cancels only in exact arithmetic
    got, = torch.autograd.grad((w["upper"] * head.uncertainty(X)).sum(), X)
    gm, gv = P.latent_adjoints((None, None, -w["upper"], None, w["upper"]), with_grad["var_f"].detach(), std)
    assert torch.equal(got, P.predictive_backward(head, Xd, gm, gv))

    with torch.no_grad():
        silent = dict(zip(OUTPUTS, head.latent(X) + head.predict(X)))
    plain = dict(zip(OUTPUTS, head.latent(Xd) + head.predict(Xd)))
    for outs in (silent, plain):
        assert all(not v.requires_grad and v.grad_fn is None for v in outs.values())
        assert all(torch.equal(outs[k], with_grad[k]) for k in OUTPUTS)

    # a second derivative: the upstream gradient is itself part of a graph, and the backward is once differentiable
    scale = torch.ones(c["G"], device=DEV, requires_grad=True)
    once, = torch.autograd.grad((scale * head.latent(X)[0]).sum(), X, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        once.sum().backward()
    # a buffer that changes between the prediction and its backward is refused, not silently used
    mean_f, _ = head.latent(X)
    head.variational_mean.mul_(2.0)
    with pytest.raises(RuntimeError, match="changed"):
        mean_f.sum().backward()


def test_chunks_and_calls_do_not_change_a_row():
    """G = 257 in chunks of 32 (nine, the last of one row), 64 (five, ragged last), 288 (one) and the default: a row's dX
    depends only on its tile of 32 rows.  Two calls give the same bits."""
    import cgat_amd as P
    c = Pc.case("g257_m37_d5")
    head, Xd = _head(c["p"]), _device_rows(c["X"])
    for arm in Pc.ARMS:
        gm, gv = (_on_device(c["arms"][arm][k]) for k in ("gm", "gv"))
        ref = P.predictive_backward(head, Xd, gm, gv)
        assert torch.equal(ref, P.predictive_backward(head, Xd, gm, gv))
        for chunk in (32, 64, 288):
            assert torch.equal(ref, P.predictive_backward(head, Xd, gm, gv, chunk_rows=chunk)), (arm, chunk)


@pytest.mark.parametrize("name", ["g257_m37_d5", "g65_m129_d640"])
def test_strided_embeddings_and_output(name):
    """Embeddings with a padded row stride and as a transposed view give the bits of the contiguous call.  The C entry with
    lddx = D + 3 and 64 rows behind the output: the padding columns and the tail rows keep their sentinel and the values are
    those bits; a stride that allows 16-byte stores gives them too."""
    import cgat_amd as P
    c = Pc.case(name)
    head, G, D = _head(c["p"]), c["G"], c["D"]
    gm, gv = (_on_device(c["arms"]["both"][k]) for k in ("gm", "gv"))
    Xc = c["X"].contiguous().to(DEV)
    plain = P.predictive_backward(head, Xc, gm, gv)
    padded = torch.full((G, D + 5), 1e30, device=DEV)[:, :D]
    padded.copy_(Xc)
    transposed = Xc.T.contiguous().T
    assert padded.stride(0) == D + 5 and (G == 1 or D == 1 or transposed.stride(1) != 1)
    assert torch.equal(plain, P.predictive_backward(head, padded, gm, gv))
    assert torch.equal(plain, P.predictive_backward(head, transposed, gm, gv))
    X = transposed.clone().requires_grad_(True)
    mean_f, var_f = head.latent(X)
    got, = torch.autograd.grad((gm * mean_f).sum() + (gv * var_f).sum(), X)
    assert torch.equal(got, plain)
    for lddx in (D + 3, D + 4 - D % 4 + 4):
        buf = torch.full((G + 64, lddx), SENTINEL, device=DEV)
        assert _entry(head, padded, gm, gv, buf, lddx, chunk=64) == 0
        assert torch.equal(buf[:G, :D], plain) and bool(torch.isfinite(buf).all())
        assert bool((buf[:G, D:] == SENTINEL).all()) and bool((buf[G:] == SENTINEL).all())


def test_nlpd_backward_through_a_linear_map():
    """emb = X0 @ W on the device, head.nlpd(emb, y, noise).mean().backward(): the value against the fp64 restatement, W.grad
    against fp64 autograd within four times what the eager fp32 arm shows (gp_predict_grad_cases.nlpd_weight_bound)."""
    nc = Pc.nlpd_case()
    head = _head(nc["p"])
    X0, y = nc["X0"].to(DEV), nc["y"].to(DEV)
    W = nc["W"].to(DEV).requires_grad_(True)
    rows = head.nlpd(X0 @ W, y, nc["noise"])
    assert rows.shape == (X0.shape[0],) and rows.dtype == torch.float32 and rows.requires_grad
    loss = rows.mean()
    assert abs(float(loss.detach()) - nc["loss"]) <= Pc.PARITY * abs(nc["loss"])
    loss.backward()
    dev = Pc.deviation(W.grad.cpu(), nc["ref"])
    print(f"[gp-predict-grad] nlpd through a linear map: dL/dW {dev:.3e} (bound {Pc.nlpd_weight_bound():.1e})")
    assert dev <= Pc.nlpd_weight_bound()
    # without grad: a plain value of the same bits
    plain = head.nlpd((X0 @ W).detach(), y, nc["noise"])
    assert not plain.requires_grad and torch.equal(plain, rows.detach())


def test_refusals_launch_nothing():
    """M = 1025, a misaligned image, a short workspace, lddx < D and both upstreams null return the unsupported, argument
    or workspace error and leave the output untouched; a width mismatch, a CPU tensor and fp64 embeddings are refused by the
    Python layer."""
    import cgat_amd as P
    c = Pc.case("g257_m37_d5")
    head, Xd, G, D = _head(c["p"]), _device_rows(c["X"]), c["G"], c["D"]
    gm, gv = (_on_device(c["arms"]["both"][k]) for k in ("gm", "gv"))
    back = head.prepare_backward()
    buf = torch.full((G, D), SENTINEL, device=DEV)
    assert _entry(head, Xd, gm, gv, buf, D, M=1025) == 4
    assert _entry(head, Xd, gm, gv, buf, D, g2img=C.c_void_p(back["g2img"].data_ptr() + 4)) == 1
    assert _entry(head, Xd, gm, gv, buf, D, ztimg=C.c_void_p(back["ztimg"].data_ptr() + 4)) == 1
    assert _entry(head, Xd, gm, gv, buf, D, ws_bytes=15) == 3
    assert _entry(head, Xd, gm, gv, buf, D - 1) == 1
    assert _entry(head, Xd, None, None, buf, D) == 1
    assert _entry(head, Xd, gm, gv, buf, D, chunk=48) == 1
    assert bool((buf == SENTINEL).all())
    assert _entry(head, Xd, gm, gv, buf, D) == 0 and not bool((buf == SENTINEL).any())
    with pytest.raises(ValueError, match="width"):
        P.predictive_backward(head, torch.zeros(4, D + 1, device=DEV), torch.ones(4, device=DEV), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.predictive_backward(head, c["X"].contiguous(), gm, gv)
    with pytest.raises(TypeError, match="float32"):
        P.predictive_backward(head, Xd.double(), gm, gv)
    with pytest.raises(TypeError, match="float32"):
        head.latent(Xd.double().requires_grad_(True))
    with pytest.raises(ValueError, match="one value per row"):
        P.predictive_backward(head, Xd, gm[:-1], None)
    # nothing to do: zeros, no launch
    assert not bool(P.predictive_backward(head, Xd, None, None).any())
    assert P.predictive_backward(head, Xd[:0], gm[:0], None).shape == (0, D)


def test_bound_gradient_entry_is_unchanged_by_the_shared_code():
    """cgat_gp_fit_grad_inputs, whose product and stores the new kernel shares (gp_input_tile), after a backward of a
    prediction has run in this process: two calls bit for bit, and within its own bound of its fp64 reference."""
    import cgat_amd as P
    import gp_grad_cases as Gc
    import gp_input_grad_cases as Ic
    from cgat_amd import gp
    c = Pc.case("g64_m64_d16")
    P.predictive_backward(_head(c["p"]), _device_rows(c["X"]), *(_on_device(c["arms"]["both"][k]) for k in ("gm", "gv")))
    ic = Ic.case("n150_m33_d5")

    def run():
        p = gp._GradientPass("test", ic["inp"]["X"].to(DEV), ic["y_norm"].to(DEV), ic["inp"]["Z"], ic["chunk_rows"])
        p.stats.factor(ic["s"], ic["ell"], Gc.JITTER)
        return [t.clone() for t in p.sums(ic["s"], ic["ell"], 2.0 * ic["adj"]["G_hat"], ic["adj"]["g"], ic["c"], input_grad=True)]

    a, b = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert Ic.deviation(a[3].cpu(), ic["ref"]) <= Ic.input_bound()
