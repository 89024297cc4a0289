"""The gradient of the collapsed sparse-GP bound on the GPU (cgat_gp_fit_grad in csrc/gpgrad.hip, gp.fit_gradient_sums,
cgat_amd.bound_and_gradient, GPHead.fit(learn=...)) against the fp64 restatement of tests/gp_grad_cases.py:

    the three sums of the data pass, each within its bound of the fp64 block's max-norm (gp_grad_cases.block_bound: the
    project's 1e-4 for P; four times the recorded fp32 floor for colsum and d2sum, whose floor lies above a quarter of 1e-4);
    two calls bit-identical, chunked against unchunked within the block bound, rows past N without influence;
    sum(colsum) against the host's figure from the same call's statistics;
    the three total gradients within four times what the eager fp32 arm shows for them (gp_grad_cases.total_bound);
    the ascent of GPHead.fit(learn=...) on n600_m96_d5 against the fp64 optimum of the restatement.

tests/test_gp_grad_cpu.py holds the recorded floors and the optimum to the restatement."""
import math

import pytest
import torch

import gp_cases
import gp_fit_cases as F
import gp_grad_cases as Gc

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
NAMES = list(Gc.NAMES)


def _device_rows(X, pad, tail=0):
    """X on the device with a row stride of D + pad; the padding, and `tail` further rows behind X, hold 1e30."""
    buf = torch.empty(X.shape[0] + tail, X.shape[1] + pad, device=DEV).fill_(1e30)
    Xd = buf[:X.shape[0], :X.shape[1]]
    Xd.copy_(X)
    assert Xd.stride(0) == X.shape[1] + pad
    return Xd


def _sums(c, chunk_rows="case", tail=0):
    from cgat_amd import gp
    inp, adj = c["inp"], c["adj"]
    out = gp.fit_gradient_sums(_device_rows(inp["X"], c["ldx_pad"], tail), c["y_norm"].to(DEV), inp["Z"], c["s"], c["ell"],
                               2.0 * adj["G_hat"], adj["g"], c["c"],
                               chunk_rows=c["chunk_rows"] if chunk_rows == "case" else chunk_rows)
    return dict(zip(Gc.BLOCKS, out))


def _block_errors(got, ref):
    return {k: (float((got[k].cpu() - ref[k]).abs().max()), Gc.block_bound(k) * float(ref[k].abs().max())) for k in Gc.BLOCKS}


@pytest.mark.parametrize("name", NAMES)
def test_blocks_parity(name):
    """One inducing point and one column; three chunks with a partial last one (n150_m33_d5); a row stride above D
    (n300_m96_d65); two slabs of R^T Xc and the largest M, 8 x 3 output tiles (n1100_m1024_d384); N below one tile."""
    c = Gc.case(name)
    got = _sums(c)
    assert got["colsum"].shape == (c["M"],) and got["d2sum"].shape == (c["M"],) and got["P"].shape == (c["M"], c["D"])
    assert all(v.dtype == torch.float64 and v.device.type == "cuda" for v in got.values())
    figures = _block_errors(got, c["blocks"])
    print(f"[gp-grad] {name}: " + ", ".join(f"{k} {e:.3e} (bound {b:.3e})" for k, (e, b) in figures.items()))
    for k, (err, bound) in figures.items():
        assert err <= bound, (k, err, bound)


def test_two_calls_bitwise_equal():
    c = Gc.case("n1100_m1024_d384")
    a = {k: v.clone() for k, v in _sums(c).items()}
    b = _sums(c)
    assert all(torch.equal(a[k], b[k]) for k in Gc.BLOCKS)


def test_chunked_and_default_chunking_agree():
    c = Gc.case("n150_m33_d5")
    chunked, whole = _sums(c, 64), _sums(c, None)
    for k in Gc.BLOCKS:
        err = float((chunked[k] - whole[k]).abs().max())
        assert err <= Gc.block_bound(k) * float(c["blocks"][k].abs().max()), (k, err)


@pytest.mark.parametrize("name", ["n31_m30_d7", "n150_m33_d5"])
def test_rows_past_n_never_contribute(name):
    """The same result, bit for bit, with 64 rows of 1e30 behind the last row of X (N is no multiple of the 32-row tile)."""
    c = Gc.case(name)
    plain = {k: v.clone() for k, v in _sums(c).items()}
    padded = _sums(c, tail=64)
    assert all(torch.equal(plain[k], padded[k]) and bool(torch.isfinite(padded[k]).all()) for k in Gc.BLOCKS)


@pytest.mark.parametrize("name", NAMES)
def test_total_gradients_and_the_colsum_identity(name):
    """bound_and_gradient against autograd of the dense bound in fp64; sum_m colsum_m against 2 tr(G^ Psi) + m.beta / v
    from the same call's statistics, within the colsum bound times M."""
    from cgat_amd import gp
    c = Gc.case(name)
    inp, M = c["inp"], c["M"]
    p = gp._GradientPass("test", _device_rows(inp["X"], c["ldx_pad"]), c["y_norm"].to(DEV), inp["Z"], c["chunk_rows"])
    sol, grads = p(c["s"], c["ell"], Gc.JITTER)
    assert set(grads) == set(Gc.GRADS) and grads["inducing_points"].shape == (M, c["D"])
    assert grads["inducing_points"].dtype == torch.float64 and grads["inducing_points"].device.type == "cpu"
    assert abs(sol["elbo"] - c["dense"]) <= Gc.ELBO_REL_BOUND * abs(c["dense"])
    got = {k: torch.as_tensor(grads[k], dtype=torch.float64).reshape(c["autograd"][k].shape) for k in Gc.GRADS}
    figures = {k: (v, Gc.total_bound(k)) for k, v in Gc.deviations(got, c["autograd"]).items()}
    adj = gp.collapsed_adjoints(p.stats.gram, c["N"], c["s"], sol)
    host = adj["log_outputscale"] + c["N"] * c["s"] / (2.0 * sol["noise"])
    identity = abs(float(p.colsum.sum()) - host)
    identity_bound = Gc.block_bound("colsum") * float(c["blocks"]["colsum"].abs().max()) * M
    print(f"[gp-grad] {name}: " + ", ".join(f"{k} {e:.3e} (bound {b:.3e})" for k, (e, b) in figures.items())
          + f", identity {identity:.3e} (bound {identity_bound:.3e})")
    for k, (err, bound) in figures.items():
        assert err <= bound, (k, err, bound)
    assert identity <= identity_bound
    # the public function is the same two passes
    sol2, grads2 = gp.bound_and_gradient(_device_rows(inp["X"], c["ldx_pad"]), c["y_norm"].to(DEV), inp["Z"], c["s"], c["ell"],
                                         chunk_rows=c["chunk_rows"])
    assert sol2["elbo"] == sol["elbo"] and torch.equal(grads2["inducing_points"], grads["inducing_points"])
    assert grads2["log_lengthscale"] == grads["log_lengthscale"] and grads2["log_outputscale"] == grads["log_outputscale"]


def test_sums_before_any_factorisation_raise():
    """_GradientPass.sums needs the W1 of a factorisation; without one, and again after the inducing points were
    replaced, it says so and enqueues nothing."""
    from cgat_amd import gp
    c = Gc.case("n70_m1_d1")
    inp, adj = c["inp"], c["adj"]
    p = gp._GradientPass("test", inp["X"].to(DEV), c["y_norm"].to(DEV), inp["Z"], c["chunk_rows"])
    with pytest.raises(RuntimeError, match="no factorisation"):
        p.sums(c["s"], c["ell"], 2.0 * adj["G_hat"], adj["g"], c["c"])
    p.stats.factor(c["s"], c["ell"], Gc.JITTER)
    p.sums(c["s"], c["ell"], 2.0 * adj["G_hat"], adj["g"], c["c"])
    p.set_inducing_points(inp["Z"])
    with pytest.raises(RuntimeError, match="no factorisation"):
        p.sums(c["s"], c["ell"], 2.0 * adj["G_hat"], adj["g"], c["c"])


def _fit_n600(learn, **kw):
    import cgat_amd as P
    f = Gc.fit_case()
    inp = f["inp"]
    return P.GPHead.fit(inp["X"].to(DEV), inp["y"].to(DEV), inducing_points=inp["Z"], lengthscale=inp["lengthscale"],
                        outputscale=inp["outputscale"], learn=learn, **kw)


@pytest.fixture(scope="module")
def learned_scales():
    return _fit_n600(("lengthscale", "outputscale"))


def test_fit_learns_lengthscale_and_outputscale(learned_scales):
    f, rec = Gc.fit_case(), Gc.FIT_OPTIMUM
    head, report = learned_scales
    steps = report["steps"]
    print(f"[gp-grad fit] l {report['lengthscale']:.6f} (fp64 {f['lengthscale']:.6f}), s {report['outputscale']:.6f} "
          f"(fp64 {f['outputscale']:.6f}), bound {report['elbo']:.4f} (fp64 {f['elbo']:.4f}), {len(steps)} iterates, "
          f"{report['evaluations']} evaluations, active {report['active_bounds']}")
    assert len(steps) >= 2 and all(b >= a for a, b in zip(steps, steps[1:]))
    assert all(report["elbo"] > v for v in f["grid"].values())
    assert abs(report["elbo"] - f["elbo"]) <= Gc.ELBO_REL_BOUND * abs(f["elbo"])
    assert abs(report["lengthscale"] - f["lengthscale"]) <= rec["rel_l"] * f["lengthscale"]
    assert abs(report["outputscale"] - f["outputscale"]) <= rec["rel_s"] * f["outputscale"]
    assert report["active_bounds"] == [] and report["learned"] == ("lengthscale", "outputscale")
    assert report["evaluations"] >= len(steps) - 1 and len(report["candidates"]) == 1
    assert abs(float(head.lengthscale) - report["lengthscale"]) <= 1e-6 * report["lengthscale"]
    assert torch.equal(head.inducing_points.cpu(), f["inp"]["Z"])


def test_fit_learns_inducing_points_too(learned_scales):
    f = Gc.fit_case()
    head, report = _fit_n600(("lengthscale", "outputscale", "inducing_points"), max_iter=15)
    steps = report["steps"]
    print(f"[gp-grad fit] with Z: bound {report['elbo']:.4f} against {learned_scales[1]['elbo']:.4f}, {len(steps)} iterates, "
          f"{report['evaluations']} evaluations")
    assert all(b >= a for a, b in zip(steps, steps[1:]))
    assert report["elbo"] >= learned_scales[1]["elbo"]
    assert not torch.equal(head.inducing_points.cpu(), f["inp"]["Z"])
    Xt = f["inp"]["Xt"].to(DEV)
    mean_f, var_f = head.latent(Xt)
    pred, lower, upper = head.predict(Xt)
    got = {k: v.cpu() for k, v in dict(mean_f=mean_f, var_f=var_f, pred=pred, lower=lower, upper=upper).items()}
    from cgat_amd import gp
    own = {k: getattr(head, k).detach().cpu().to(torch.float64) for k in gp._KEYS}
    for k, (err, bound) in gp_cases.errors(got, gp_cases.direct_form(own, f["inp"]["Xt"]), own).items():
        assert err <= bound, (k, err, bound)


def test_bounds_hold_the_ascent_in_the_box():
    """A box that ends before the optimum: the ascent stops on it and says so."""
    f = Gc.fit_case()
    head, report = _fit_n600(("lengthscale", "outputscale"), bounds=dict(lengthscale=(0.5, 2.0)))
    assert report["lengthscale"] == pytest.approx(0.5 * f["inp"]["lengthscale"], rel=1e-12)
    assert report["active_bounds"] == ["lengthscale:lower"]
    assert all(b >= a for a, b in zip(report["steps"], report["steps"][1:]))
    with pytest.raises(ValueError, match="subset"):
        _fit_n600(("noise",))
    with pytest.raises(ValueError, match="factors"):
        _fit_n600(("lengthscale",), bounds=dict(lengthscale=(2.0, 4.0)))


def test_learn_empty_is_the_call_without_the_keyword():
    import cgat_amd as P
    from cgat_amd import gp
    c = F.case("n300_m96_d65")
    inp = c["inp"]
    args = dict(inducing_points=inp["Z"], lengthscale=[0.5 * inp["lengthscale"], inp["lengthscale"]], outputscale=inp["outputscale"])
    Xd, yd = inp["X"].to(DEV), inp["y"].to(DEV)
    (h1, r1), (h2, r2) = P.GPHead.fit(Xd, yd, **args), P.GPHead.fit(Xd, yd, learn=(), **args)
    assert r1 == r2 and "steps" not in r1
    assert all(torch.equal(getattr(h1, k), getattr(h2, k)) for k in gp._KEYS)
