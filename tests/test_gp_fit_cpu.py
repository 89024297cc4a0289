"""CPU-side checks of the sparse-GP fit (cgat_amd/gp.py, csrc/gpfit.hip): the collapsed bound against the explicit one in
fp64, the host solver against the restatement, the fp32 floor the GPU tolerances are held against, the ABI entries and
the refusals.  No compute call of the library is made here.

The tests of the bound (collapsed = explicit, gradients, perturbations), the fp32 floor and the separation of the grid
case check the restatement of tests/gp_fit_cases.py alone: they hold the oracle and the inputs right and pass without the
package.  The tests of solve_collapsed, median_lengthscale, the ABI, the workspace query and the refusals run the package
and fail where it lacks the fit."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import gp_cases
import gp_fit_cases as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(F.CASES)


def _explicit_at(c):
    """The whitened rows and a closure evaluating the explicit bound of a case."""
    inp = c["inp"]
    A = F.whitened_rows(inp["X"], inp["Z"], inp["outputscale"], inp["lengthscale"])
    return lambda m, LS, const, v: F.explicit_elbo(A, c["y_norm"], inp["outputscale"], m, LS, const, v)


@pytest.mark.parametrize("name", NAMES)
def test_collapsed_equals_explicit_bound(name):
    """F at the solved (m, L_S, c, sigma^2) equals sum_n E_q[log N] - KL there, to 1e-10 relative; sigma^2 is interior to
    the search."""
    c = F.case(name)
    sol = c["sol"]
    explicit = float(_explicit_at(c)(sol["variational_mean"], sol["chol_variational_covar"], sol["constant"], sol["noise"]))
    assert abs(explicit - sol["elbo"]) <= 1e-10 * abs(explicit), (explicit, sol["elbo"])
    lo, hi = F.LOG_NOISE_BOUNDS
    assert lo + 1.0 < math.log(sol["noise"]) < hi - 1.0


@pytest.mark.parametrize("name", NAMES)
def test_gradients_of_the_explicit_bound_vanish(name):
    """Autograd gradients of the explicit bound w.r.t. m, tril(L_S) and c at the solution: below 1e-8 of the gradient norm
    at (0, I, 0)."""
    c = F.case(name)
    sol, M = c["sol"], c["M"]
    bound = _explicit_at(c)

    def grad_norm(m, LS, const):
        m, LS = m.clone().requires_grad_(True), LS.clone().requires_grad_(True)
        const = torch.tensor(float(const), dtype=torch.float64, requires_grad=True)
        gm, gL, gc = torch.autograd.grad(bound(m, LS, const, sol["noise"]), (m, LS, const))
        return math.sqrt(float(gm.square().sum() + gL.tril().square().sum() + gc.square()))

    at_start = grad_norm(torch.zeros(M, dtype=torch.float64), torch.eye(M, dtype=torch.float64), 0.0)
    at_solution = grad_norm(sol["variational_mean"], sol["chol_variational_covar"], sol["constant"])
    assert at_start > 0 and at_solution <= 1e-8 * at_start, (at_solution, at_start)


@pytest.mark.parametrize("name", NAMES)
def test_perturbations_only_lower_the_explicit_bound(name):
    c = F.case(name)
    sol, M = c["sol"], c["M"]
    bound = _explicit_at(c)
    best = float(bound(sol["variational_mean"], sol["chol_variational_covar"], sol["constant"], sol["noise"]))
    g = torch.Generator().manual_seed(5)
    for scale in (1e-3, 1e-1, 1.0):
        dm = scale * torch.randn(M, generator=g, dtype=torch.float64)
        dL = scale / math.sqrt(M) * torch.randn(M, M, generator=g, dtype=torch.float64).tril()
        LS = sol["chol_variational_covar"] + dL
        LS = LS - torch.diag(torch.diagonal(LS)) + torch.diag(torch.diagonal(LS).abs().clamp_min(1e-12))
        dc = scale * float(torch.randn((), generator=g, dtype=torch.float64))
        for args in ((sol["variational_mean"] + dm, sol["chol_variational_covar"], sol["constant"]),
                     (sol["variational_mean"], LS, sol["constant"]),
                     (sol["variational_mean"], sol["chol_variational_covar"], sol["constant"] + dc),
                     (sol["variational_mean"] + dm, LS, sol["constant"] + dc)):
            assert float(bound(*args, sol["noise"])) < best, scale


@pytest.mark.parametrize("name", NAMES)
def test_solve_collapsed_agrees_with_the_restatement(name):
    from cgat_amd import gp
    c = F.case(name)
    s, N = c["inp"]["outputscale"], c["N"]
    got, ref = gp.solve_collapsed(c["gram"], N, s), c["sol"]
    assert set(got) == {"variational_mean", "chol_variational_covar", "constant", "noise", "elbo"}
    assert abs(got["noise"] - ref["noise"]) <= 1e-6 * ref["noise"]
    assert abs(got["elbo"] - ref["elbo"]) <= 1e-10 * abs(ref["elbo"])
    assert abs(got["constant"] - ref["constant"]) <= 1e-6
    scale = float(ref["variational_mean"].abs().max())
    assert float((got["variational_mean"] - ref["variational_mean"]).abs().max()) <= 1e-6 * scale
    S_got = got["chol_variational_covar"] @ got["chol_variational_covar"].T
    S_ref = ref["chol_variational_covar"] @ ref["chol_variational_covar"].T
    assert float((S_got - S_ref).abs().max()) <= 1e-6 * float(S_ref.abs().max())
    assert float(got["chol_variational_covar"].triu(1).abs().max()) == 0


def test_solve_collapsed_honours_fixed_noise_and_zero_mean():
    from cgat_amd import gp
    c = F.case("n300_m96_d65")
    s, N = c["inp"]["outputscale"], c["N"]
    for kw in (dict(noise=0.37), dict(zero_mean=True), dict(noise=0.05, zero_mean=True)):
        got, ref = gp.solve_collapsed(c["gram"], N, s, **kw), F.solve(c["gram"], N, s, **kw)
        if "noise" in kw:
            assert got["noise"] == kw["noise"]
        else:
            assert abs(got["noise"] - ref["noise"]) <= 1e-6 * ref["noise"]
        if kw.get("zero_mean"):
            assert got["constant"] == 0.0
        assert abs(got["elbo"] - ref["elbo"]) <= 1e-10 * abs(ref["elbo"])
        assert got["elbo"] < c["sol"]["elbo"]                 # a constraint can only lower the optimum
        explicit = float(_explicit_at(c)(got["variational_mean"], got["chol_variational_covar"], got["constant"],
                                         got["noise"]))
        assert abs(explicit - got["elbo"]) <= 1e-10 * abs(explicit)


def test_median_lengthscale():
    from cgat_amd import gp
    Z = F.case("n150_m33_d5")["inp"]["Z"]
    d2 = torch.cdist(Z.double(), Z.double()) ** 2
    i, j = torch.tril_indices(33, 33, offset=-1)
    assert abs(gp.median_lengthscale(Z) - math.sqrt(float(d2[i, j].median()))) <= 1e-12
    with pytest.raises(ValueError):
        gp.median_lengthscale(Z[:1])


@pytest.mark.parametrize("name", NAMES)
def test_fp32_floor_of_the_cases(name):
    """An eager fp32 evaluation of the statistics (centred as the kernel centres, W1 from fp64 rounded to fp32, Gram in
    fp32 per chunk) and the head fitted from it, evaluated in fp32, stay under a quarter of every bound of the GPU test."""
    c = F.case(name)
    inp, N = c["inp"], c["N"]
    s, ell = inp["outputscale"], inp["lengthscale"]
    G32 = F.statistics_fp32(inp["X"], inp["y_stat"], inp["Z"], s, ell)
    for k, (err, bound) in F.gram_errors(G32, c["gram_stat"]).items():
        assert err <= 0.25 * bound, (k, err, bound)
    sol32 = F.solve(F.statistics_fp32(inp["X"], c["y_norm"].float(), inp["Z"], s, ell), N, s)
    noise_dev = abs(sol32["noise"] - c["sol"]["noise"]) / c["sol"]["noise"]
    elbo_dev = abs(sol32["elbo"] - c["sol"]["elbo"]) / abs(c["sol"]["elbo"])
    print(f"[gp-fit floor] {name}: noise {noise_dev:.3e}, elbo {elbo_dev:.3e}")
    assert noise_dev <= 0.25 * F.NOISE_REL_BOUND and elbo_dev <= 0.25 * F.ELBO_REL_BOUND
    p32 = {k: v.float() for k, v in F.head_params(inp, sol32, c["mean"], c["std"]).items()}
    got = gp_cases.factor_form(p32, inp["Xt"], dtype=torch.float32)
    for k, (err, bound) in gp_cases.errors(got, c["ref"], c["params"]).items():
        assert err <= 0.25 * bound, (k, err, bound)


def test_grid_case_separates_its_candidates():
    """The restated bounds of the three lengthscales of the GPU grid test differ by more than 1e-3 relative."""
    elbos = sorted(F.grid_elbos().values())
    assert all((b - a) > 1e-3 * abs(b) for a, b in zip(elbos, elbos[1:])), elbos


def test_abi_declares_gp_fit_entries():
    from cgat_amd import _lib
    src = open(os.path.join(ROOT, "include", "cgat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for n in ("cgat_gp_fit_stats_workspace_bytes", "cgat_gp_fit_stats"):
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert _lib.lib.cgat_abi_version() == 3


def test_workspace_query_positive_and_monotone():
    from cgat_amd import _lib
    q = _lib.lib.cgat_gp_fit_stats_workspace_bytes
    for N, M, D in ((1000000, 1000, 384), (1100, 1024, 384), (70, 1, 1)):
        sizes = [q(N, M, D, ch) for ch in (32, 64, 1024, 1056, 4096, 32768, 65536)]
        assert all(v > 0 for v in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert q(1000000, 1000, 384, 32) < q(1000000, 1000, 384, 32768)
    # the whitened chunk [Ma_p][chunk] is the floor of it
    assert q(1000000, 1000, 384, 32768) >= 1024 * 32768 * 4
    assert q(100, 1025, 8, 32768) == 0 and q(100, 8, 8, 48) == 0      # what the entry refuses


# cgat_gp_fit_stats_workspace_bytes at the cases' (N, M, D, chunk_rows) (None: the default of 32768) and at training size
WORKSPACE_BYTES = {"n70_m1_d1": 77824, "n150_m33_d5": 81920, "n300_m96_d65": 229376, "n1000_m129_d130": 851968,
                   "n1100_m1000_d128": 9306112, "n1100_m1024_d384": 10629120, "n31_m30_d7": 69632}


def test_workspace_query_pinned():
    """The sizes the query has returned since the entry exists: the chunk plan it shares with the entry must not move them."""
    from cgat_amd import _lib
    q = _lib.lib.cgat_gp_fit_stats_workspace_bytes
    assert set(WORKSPACE_BYTES) == set(F.CASES)
    for name, kw in F.CASES.items():
        assert q(kw["N"], kw["M"], kw["D"], kw.get("chunk_rows") or 32768) == WORKSPACE_BYTES[name], name
    assert q(1000000, 1000, 384, 32768) == 209715200
    assert q(100, 1025, 8, 32768) == 0 and q(100, 8, 8, 48) == 0 and q(0, 8, 8, 32) == 0


def test_fit_and_statistics_refuse_cpu_dtype_and_width():
    import cgat_amd as P
    inp = F.case("n150_m33_d5")["inp"]
    X, y, Z = inp["X"], inp["y"], inp["Z"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.GPHead.fit(X, y, inducing_points=Z, lengthscale=2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.gp.fit_statistics(X, inp["y_stat"], Z, 1.3, 2.0)
    with pytest.raises(TypeError, match="float32"):
        P.GPHead.fit(X.double(), y, inducing_points=Z, lengthscale=2.0)
    with pytest.raises(TypeError, match="float32"):
        P.gp.fit_statistics(X.double(), inp["y_stat"], Z, 1.3, 2.0)
    with pytest.raises(ValueError, match="width"):
        P.GPHead.fit(X[:, :4], y, inducing_points=Z, lengthscale=2.0)
    with pytest.raises(ValueError, match="width"):
        P.gp.fit_statistics(X[:, :4], inp["y_stat"], Z, 1.3, 2.0)
    with pytest.raises(ValueError, match="multiple of 32"):
        P.gp.fit_statistics(X, inp["y_stat"], Z, 1.3, 2.0, chunk_rows=48)


def test_solve_collapsed_refuses_a_wrong_shape():
    """A statistics matrix of the wrong rank or shape is a ValueError."""
    from cgat_amd import gp
    for bad in (torch.tensor(1.0), torch.zeros(3), torch.zeros(3, 4), torch.zeros(2, 2)):
        with pytest.raises(ValueError, match=r"\[M\+2, M\+2\]"):
            gp.solve_collapsed(bad, 10, 1.0)
