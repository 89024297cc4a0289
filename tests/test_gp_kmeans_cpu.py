"""CPU-side checks of the k-means inducing points (cgat_amd/gp.py, csrc/gpkmeans.hip): the fixtures of
tests/gp_kmeans_cases.py are what tests/test_gp_kmeans.py assumes of them, an eager fp32 evaluation sits at a quarter of
that test's numeric bounds, the ABI entries and the refusals that need no device.  No compute call of the library is made.

The fixture and floor tests check the restatement alone and pass without the package; the ABI test and the refusals run
the package and fail where it lacks the feature."""
import ctypes as C
import os
import re

import pytest
import torch

import gp_kmeans_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(K.CASES)
LLOYD = sorted(K.LLOYD_CASES)


@pytest.mark.parametrize("name", LLOYD)
def test_lloyd_fixtures_are_clear_of_ties_and_converge(name):
    """Every row of every step has gap > 100 B, so the GPU's assignments and centres can be compared directly; the loop
    moves the centres at least twice, converges within the steps the GPU test runs, and every inertia is more than
    4e-4 below the one before it: two values within 1e-4 relative of such a list are non-increasing too."""
    c = K.lloyd_case(name)
    ref = c["ref"]
    for st in ref["steps"]:
        assert float((st["gap"] / st["bound"]).min()) > 100.0
    assert ref["converged"] and 2 <= ref["iterations"] < K.LLOYD_ITERS
    assert len(ref["inertia"]) == ref["iterations"] + 1 and len(ref["empty"]) == ref["iterations"]
    assert len(ref["Z"]) == ref["iterations"] + 1
    ine = ref["inertia"]
    assert all(b < a * (1.0 - 4e-4) for a, b in zip(ine, ine[1:])), ine
    assert torch.equal(ref["Z"][0], c["Z0"]) and all(z.dtype == torch.float32 for z in ref["Z"])
    # the last two steps found one assignment: the returned centres are its means
    X, a = c["inp"]["X"].double(), ref["steps"][-1]["assign"]
    for m in range(c["M"]):
        assert float((ref["Z"][-1][m].double() - X[a == m].mean(0)).abs().max()) <= 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_step_fixtures_have_few_near_ties(name):
    """At most 2 % of the rows of a step case have gap <= B (the rule then only bounds their centre's distance)."""
    st = K.case(name)["step"]
    near = float((st["gap"] <= st["bound"]).double().mean())
    print(f"[gp-kmeans fixtures] {name}: {near:.4f} of the rows have gap <= B")
    assert near <= 0.02
    assert float(st["counts"].sum()) == K.case(name)["N"]


def _floor(X, Z, st):
    a, counts, wss, sums = K.eager_fp32_step(X, Z)
    fig = K.assignment_figures(a, st, Z, scale=0.25)
    assert fig["wrong_clear"] == 0 and fig["excess"] <= 1.0 and fig["not_lowest"] == 0, fig
    c_ref, w_ref, s_ref = K.sums_of(X, Z, a)
    assert torch.equal(counts, c_ref)
    for k, (err, bound) in K.sum_errors(wss, sums, w_ref, s_ref).items():
        assert err <= 0.25 * bound, (k, err, bound)


@pytest.mark.parametrize("name", NAMES)
def test_fp32_floor_of_the_step_cases(name):
    """An eager fp32 evaluation centred like the kernel meets the assignment rule with B / 4 and has wss and sums within a
    quarter of the GPU test's bound."""
    c = K.case(name)
    _floor(c["inp"]["X"], c["inp"]["Z"], c["step"])


@pytest.mark.parametrize("name", K.SPECIAL)
def test_fp32_floor_of_the_special_inputs(name):
    sp = K.special(name)
    _floor(sp["X"], sp["Z"], sp["step"])
    if name == "far_centre":
        assert float(sp["step"]["counts"][sp["marked"]]) == 0.0 and float((sp["step"]["gap"] / sp["step"]["bound"]).min()) > 1.0
    if name == "duplicates":
        first, copies = sp["marked"]
        assert copies and float(sp["step"]["counts"][first]) > 0 and all(float(sp["step"]["counts"][m]) == 0 for m in copies)


def test_fit_fixtures_have_an_fp32_floor_and_separate_their_starts():
    """The bound of an eager fp32 evaluation of the statistics at both starts of the fit tests is within a quarter of
    ELBO_REL_BOUND of the restated one, and the two starts' bounds differ by more than 1e-3 relative (the test of the
    ascent tells them apart at 1e-6)."""
    import gp_fit_cases as F
    for name, ells, s in (("n300_m9_d7", (3.0, 6.0), 1.3), ("n150_m6_d5", (4.0,), 1.0)):      # what the GPU tests pass
        c = K.lloyd_case(name)
        X, y = c["inp"]["X"], c["inp"]["y"]
        y_norm = F.normalise(y)[0]
        for ell in ells:
            elbos = []
            for Z in (c["Z0"], c["ref"]["Z"][-1]):
                want = K.restated_elbo(X, y, Z, s, ell)
                got = F.solve(F.statistics_fp32(X, y_norm.float(), Z, s, ell), c["N"], s)["elbo"]
                assert abs(got - want) <= 0.25 * F.ELBO_REL_BOUND * abs(want), (name, ell, got, want)
                elbos.append(want)
            assert abs(elbos[0] - elbos[1]) > 1e-3 * abs(elbos[0]), (name, ell, elbos)


@pytest.mark.parametrize("name", LLOYD)
def test_fp32_floor_of_the_lloyd_fixtures(name):
    c = K.lloyd_case(name)
    for Z, st in zip(c["ref"]["Z"], c["ref"]["steps"]):
        _floor(c["inp"]["X"], Z, st)


def test_rule_helpers():
    """lowest_argmin and first_of_equal return the lowest index; the bound is the documented formula."""
    d = torch.tensor([[2.0, 1.0, 1.0], [0.0, 0.0, 3.0]], dtype=torch.float64)
    assert K.lowest_argmin(d).tolist() == [1, 0]
    Z = torch.tensor([[1.0, 2.0], [3.0, 4.0], [1.0, 2.0], [3.0, 4.0]])
    assert K.first_of_equal(Z).tolist() == [0, 1, 0, 1]
    X = torch.tensor([[0.5, 0.25]])
    st = K.step(X, Z)
    cbar = Z.double().mean(0)
    want = 8 * 5 * 2.0 ** -24 * (float(((X.double() - cbar) ** 2).sum()) + float(((Z.double() - cbar) ** 2).sum(1).max()))
    assert abs(float(st["bound"][0]) - want) <= 1e-18 and int(st["assign"][0]) == 0 and float(st["gap"][0]) == 0.0
    fig = K.assignment_figures(torch.tensor([2]), st, Z)
    assert fig["not_lowest"] == 1 and fig["wrong_clear"] == 0 and fig["excess"] == 0.0


def test_abi_declares_gp_kmeans_entries():
    from cgat_amd import _lib
    src = open(os.path.join(ROOT, "include", "cgat_hip.h")).read()
    assert "gaussian_process.py:208-226" in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for n in ("cgat_gp_kmeans_step_workspace_bytes", "cgat_gp_kmeans_step"):
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert len(_lib.PROTOTYPES["cgat_gp_kmeans_step"][1]) == 16
    assert _lib.lib.cgat_abi_version() == 3


def test_workspace_query_is_the_gradient_pass_layout():
    from cgat_amd import _lib
    q, g = _lib.lib.cgat_gp_kmeans_step_workspace_bytes, _lib.lib.cgat_gp_fit_grad_workspace_bytes
    for kw in list(K.CASES.values()) + [dict(N=1000000, M=1000, D=384), dict(N=1000000, M=1000, D=640)]:
        args = (kw["N"], kw["M"], kw["D"], kw.get("chunk_rows") or 32768)
        assert q(*args) == g(*args) > 0, args
    assert q(100, 1025, 8, 32768) == 0 and q(100, 8, 8, 48) == 0 and q(0, 8, 8, 32) == 0     # what the entry refuses


def test_refusals_before_any_device_work():
    """A bad `init` or a negative `iters` is a ValueError even for inputs the device path would refuse first."""
    import cgat_amd as P
    inp = K.lloyd_case("n150_m6_d5")["inp"]
    X, y = inp["X"], inp["y"]                                       # on the CPU
    with pytest.raises(ValueError, match="init"):
        P.GPHead.fit(X, y, inducing_points=6, init="nonsense")
    with pytest.raises(ValueError, match="init"):
        P.GPHead.fit(X, y, inducing_points=6, init=("subset", "subset"))
    with pytest.raises(ValueError, match="init"):
        P.GPHead.fit(X, y, inducing_points=6, init=())
    with pytest.raises(ValueError, match="kmeans_iters"):
        P.GPHead.fit(X, y, inducing_points=6, init="kmeans", kmeans_iters=-1)
    with pytest.raises(ValueError, match="iters"):
        P.kmeans_inducing_points(X, 6, iters=-1)


def test_kmeans_refuses_cpu_dtype_width_and_chunking():
    import cgat_amd as P
    c = K.case("n150_m33_d5")
    X, Z = c["inp"]["X"], c["inp"]["Z"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.gp.kmeans_step(X, Z)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.kmeans_inducing_points(X, 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.GPHead.fit(X, X[:, 0], inducing_points=6, init="kmeans")
    with pytest.raises(TypeError, match="float32"):
        P.gp.kmeans_step(X.double(), Z)
    with pytest.raises(TypeError, match="float32"):
        P.kmeans_inducing_points(X.double(), 6)
    with pytest.raises(ValueError, match="width"):
        P.gp.kmeans_step(X[:, :4], Z)
    with pytest.raises(ValueError, match="width"):
        P.kmeans_inducing_points(X[:, :4], Z)
    with pytest.raises(ValueError, match=r"\[M, D\]"):
        P.gp.kmeans_step(X, Z[0])
    with pytest.raises(ValueError, match="multiple of 32"):
        P.gp.kmeans_step(X, Z, chunk_rows=48)
