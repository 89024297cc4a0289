"""The sparse-GP fit on the GPU (cgat_amd.GPHead.fit, gp.fit_statistics, cgat_gp_fit_stats, csrc/gpfit.hip) against the fp64
restatement of tests/gp_fit_cases.py, at the project's parity criterion (1e-4 max-norm relative):

    every block of the statistics within 1e-4 of that block's max-norm, N exact, the matrix exactly symmetric;
    the fitted head's predictions on 257 held-out rows within gp_cases.errors' bounds of the fp64 fit's (direct form);
    the bound within 1e-4 relative, the noise within gp_fit_cases.NOISE_REL_BOUND.

An eager fp32 evaluation sits at a quarter of each of these or lower (tests/test_gp_fit_cpu.py holds the inputs to that)."""
import pytest
import torch

import gp_cases
import gp_fit_cases as F

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
NAMES = sorted(F.CASES)


def _device_rows(X, pad):
    """X on the device with a row stride of D + pad; the padding holds 1e30."""
    Xd = torch.empty(X.shape[0], X.shape[1] + pad, device=DEV).fill_(1e30)[:, :X.shape[1]]
    Xd.copy_(X)
    assert Xd.stride(0) == X.shape[1] + pad
    return Xd


def _fit(c, **kw):
    import cgat_amd as P
    inp = c["inp"]
    args = dict(inducing_points=inp["Z"], lengthscale=inp["lengthscale"], outputscale=inp["outputscale"],
                chunk_rows=c["chunk_rows"])
    args.update(kw)
    return P.GPHead.fit(_device_rows(inp["X"], c["ldx_pad"]), inp["y"].to(DEV), **args)


@pytest.mark.parametrize("name", NAMES)
def test_statistics_parity(name):
    """One inducing point and one column; three chunks with a partial last one and M + 2 across a 32 boundary
    (n150_m33_d5); a row stride above D (n300_m96_d65); two slabs of the Gram product (N = 1100); Ma_p = 1056, i.e. nine
    row blocks of 128 with the last one partial (M = 1024); N below one tile with M + 2 = 32 (n31_m30_d7)."""
    from cgat_amd import gp
    c = F.case(name)
    inp, N, M = c["inp"], c["N"], c["M"]
    gram = gp.fit_statistics(_device_rows(inp["X"], c["ldx_pad"]), inp["y_stat"].to(DEV), inp["Z"], inp["outputscale"],
                             inp["lengthscale"], chunk_rows=c["chunk_rows"])
    assert gram.shape == (M + 2, M + 2) and gram.dtype == torch.float64 and gram.device.type == "cuda"
    gram = gram.cpu()
    figures = F.gram_errors(gram, c["gram_stat"])
    print(f"[gp-fit] {name}: " + ", ".join(f"{k} {e:.3e} (bound {b:.3e})" for k, (e, b) in figures.items()))
    for k, (err, bound) in figures.items():
        assert err <= bound, (k, err, bound)
    assert float(gram[M + 1, M + 1]) == float(N)
    assert torch.equal(gram, gram.T)


@pytest.mark.parametrize("name", NAMES)
def test_fit_parity(name):
    c = F.case(name)
    inp, sol = c["inp"], c["sol"]
    head, report = _fit(c)
    Xt = inp["Xt"].to(DEV)
    mean_f, var_f = head.latent(Xt)
    pred, lower, upper = head.predict(Xt)
    got = {k: v.cpu() for k, v in dict(mean_f=mean_f, var_f=var_f, pred=pred, lower=lower, upper=upper).items()}
    figures = gp_cases.errors(got, c["ref"], c["params"])
    noise_dev = abs(report["noise"] - sol["noise"]) / sol["noise"]
    elbo_dev = abs(report["elbo"] - sol["elbo"]) / abs(sol["elbo"])
    print(f"[gp-fit] {name}: " + ", ".join(f"{k} {e:.3e} (bound {b:.3e})" for k, (e, b) in figures.items())
          + f", noise {noise_dev:.3e} (bound {F.NOISE_REL_BOUND:.1e}), elbo {elbo_dev:.3e} (bound {F.ELBO_REL_BOUND:.1e})")
    for k, (err, bound) in figures.items():
        assert err <= bound, (k, err, bound)
    assert elbo_dev <= F.ELBO_REL_BOUND and noise_dev <= F.NOISE_REL_BOUND
    assert report["elbo_per_point"] == report["elbo"] / c["N"]
    assert report["lengthscale"] == inp["lengthscale"] and report["outputscale"] == inp["outputscale"]
    assert len(report["candidates"]) == 1 and report["candidates"][0]["elbo"] == report["elbo"]
    assert float(head.mean) == c["mean"] and float(head.std) == c["std"]
    assert head.inducing_points.device.type == "cuda" and torch.equal(head.inducing_points.cpu(), inp["Z"])


def test_two_runs_bitwise_equal():
    """Two slabs and 45 output tiles, the ninth row block of 128 partial (n1100_m1024_d384): the statistics and every
    buffer of the head repeat bit for bit."""
    from cgat_amd import gp
    c = F.case("n1100_m1024_d384")
    inp = c["inp"]
    Xd, yd = inp["X"].to(DEV), inp["y_stat"].to(DEV)
    a, b = (gp.fit_statistics(Xd, yd, inp["Z"], inp["outputscale"], inp["lengthscale"]) for _ in range(2))
    assert torch.equal(a, b)
    (h1, r1), (h2, r2) = _fit(c), _fit(c)
    assert all(torch.equal(getattr(h1, k), getattr(h2, k)) for k in gp._KEYS)
    assert r1["elbo"] == r2["elbo"] and r1["noise"] == r2["noise"]


def test_chunked_and_default_chunking_agree():
    from cgat_amd import gp
    c = F.case("n150_m33_d5")
    inp, N, M = c["inp"], c["N"], c["M"]
    Xd, yd = inp["X"].to(DEV), inp["y_stat"].to(DEV)
    chunked, whole = (gp.fit_statistics(Xd, yd, inp["Z"], inp["outputscale"], inp["lengthscale"], chunk_rows=ch).cpu()
                      for ch in (64, None))
    for k, (err, bound) in F.gram_errors(chunked, whole).items():
        assert err <= F.PARITY * float(F.blocks(c["gram_stat"])[k].abs().max()), (k, err)
    assert float(chunked[M + 1, M + 1]) == float(N) == float(whole[M + 1, M + 1])
    assert torch.equal(chunked, chunked.T) and torch.equal(whole, whole.T)


def test_grid_selects_the_candidate_the_restatement_ranks_first():
    c = F.case(F.GRID_CASE)
    elbos = F.grid_elbos()
    ells = sorted(elbos)
    want = max(elbos, key=elbos.get)
    head, report = _fit(c, lengthscale=ells)
    assert len(report["candidates"]) == 3 and [r["lengthscale"] for r in report["candidates"]] == ells
    assert report["lengthscale"] == want
    assert abs(float(head.lengthscale) - want) <= 1e-6 * want
    for row in report["candidates"]:
        ref = elbos[row["lengthscale"]]
        assert abs(row["elbo"] - ref) <= F.ELBO_REL_BOUND * abs(ref)
    assert report["elbo"] == max(r["elbo"] for r in report["candidates"])


def test_integer_inducing_points_median_lengthscale_and_seed():
    """An int draws that many distinct training rows with the seeded generator; "median" is the host's fp64 figure."""
    import cgat_amd as P
    c = F.case("n300_m96_d65")
    inp = c["inp"]
    Xd, yd = inp["X"].to(DEV), inp["y"].to(DEV)
    h1, r1 = P.GPHead.fit(Xd, yd, inducing_points=40, seed=3)
    h2, _ = P.GPHead.fit(Xd, yd, inducing_points=40, seed=3)
    h3, _ = P.GPHead.fit(Xd, yd, inducing_points=40, seed=4)
    Z = h1.inducing_points.cpu()
    assert Z.shape == (40, 65) and torch.equal(Z, h2.inducing_points.cpu()) and not torch.equal(Z, h3.inducing_points.cpu())
    rows = (Z[:, None, :] == inp["X"][None, :, :]).all(-1)
    assert bool((rows.sum(1) == 1).all()) and rows.any(0).sum() == 40
    assert r1["lengthscale"] == P.gp.median_lengthscale(Z) and r1["outputscale"] == 1.0
    pred, lower, upper = h1.predict(inp["Xt"].to(DEV))
    assert all(bool(torch.isfinite(v).all()) for v in (pred, lower, upper)) and float((upper - lower).min()) >= 0


def test_zero_mean_and_fixed_noise():
    c = F.case("n150_m33_d5")
    head, report = _fit(c, zero_mean=True)
    assert float(head.constant) == 0.0 and report["constant"] == 0.0
    ref = F.solve(c["gram"], c["N"], c["inp"]["outputscale"], zero_mean=True)
    assert abs(report["elbo"] - ref["elbo"]) <= F.ELBO_REL_BOUND * abs(ref["elbo"])
    _, report = _fit(c, noise=0.5, outputscale=torch.tensor(1.3, dtype=torch.float64))    # a 0-d tensor is a scalar
    assert report["noise"] == 0.5 and report["outputscale"] == 1.3 and len(report["candidates"]) == 1


def test_refusals():
    import cgat_amd as P
    from cgat_amd._lib import CgatHipError
    g = torch.Generator().manual_seed(0)
    X, y = torch.randn(1100, 8, generator=g).to(DEV), torch.randn(1100, generator=g).to(DEV)
    with pytest.raises(CgatHipError, match="M <= 1024"):
        P.GPHead.fit(X, y, inducing_points=1025, lengthscale=3.0)
    with pytest.raises(CgatHipError, match="M <= 1024"):
        P.gp.fit_statistics(X, y, X[:1025].cpu(), 1.0, 3.0)
    with pytest.raises(ValueError, match="two rows"):
        P.GPHead.fit(X[:1], y[:1], inducing_points=1, lengthscale=3.0)
    with pytest.raises(TypeError, match="float32"):
        P.GPHead.fit(X.double(), y, inducing_points=8, lengthscale=3.0)
    with pytest.raises(ValueError, match="width"):
        P.GPHead.fit(X, y, inducing_points=X[:8, :7].cpu(), lengthscale=3.0)
    with pytest.raises(ValueError, match="multiple of 32"):
        P.gp.fit_statistics(X, y, X[:8].cpu(), 1.0, 3.0, chunk_rows=48)
    with pytest.raises(ValueError, match="targets"):
        P.GPHead.fit(X, y[:-1], inducing_points=8, lengthscale=3.0)
