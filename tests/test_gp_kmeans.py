"""K-means inducing points on the GPU (cgat_gp_kmeans_step in csrc/gpkmeans.hip, gp.kmeans_step,
cgat_amd.kmeans_inducing_points, GPHead.fit(init=...)) against the fp64 restatement of
tests/gp_kmeans_cases.py:

    per step  the assignment under the near-tie rule of that file (a row with gap > B receives the restatement's centre,
              any other row one within B of its minimum, never the higher of two bit-identical centres); counts exact;
              wss and sums within 1e-4 of their max-norm in the restatement (the project's parity criterion), evaluated
              at the assignment the kernel made once the rule has passed it
    the loop  on fixtures without near ties: assignments and the report equal to the restatement's, Z within 1e-4 of
              max |Z_ref - mean|, the inertia list within 1e-4 relative and non-increasing
    the fit   GPHead.fit(init=...) keeps the start with the larger bound; nothing asserts that k-means is that start.

An eager fp32 evaluation sits at a quarter of each numeric bound or lower (tests/test_gp_kmeans_cpu.py holds the fixtures to
that)."""
import pytest
import torch

import gp_fit_cases as F
import gp_kmeans_cases as K

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
NAMES = sorted(K.CASES)
LLOYD = sorted(K.LLOYD_CASES)


def _device_rows(X, pad=0):
    """X on the device with a row stride of D + pad; the padding holds 1e30."""
    Xd = torch.empty(X.shape[0], X.shape[1] + pad, device=DEV).fill_(1e30)[:, :X.shape[1]]
    Xd.copy_(X)
    assert Xd.stride(0) == X.shape[1] + pad
    return Xd


def _check_step(tag, out, X, Z, st=None):
    """Holds one kmeans_step result to the restatement; returns the assignment on the host."""
    N, (M, D) = X.shape[0], Z.shape
    st = K.step(X, Z) if st is None else st
    assert out["assign"].dtype == torch.int32 and out["assign"].shape == (N,)
    assert all(out[k].dtype == torch.float64 and out[k].device.type == "cuda" for k in ("counts", "wss", "sums"))
    assert out["counts"].shape == (M,) and out["wss"].shape == (M,) and out["sums"].shape == (M, D)
    a = out["assign"].cpu().to(torch.int64)
    assert int(a.min()) >= 0 and int(a.max()) < M
    fig = K.assignment_figures(a, st, Z)
    assert torch.equal(out["centroid"].cpu().double(), st["centroid"])
    counts, wss, sums = K.sums_of(X, Z, a, st["centroid"])
    errs = K.sum_errors(out["wss"].cpu(), out["sums"].cpu(), wss, sums)
    print(f"[gp-kmeans] {tag}: {fig}, " + ", ".join(f"{k} {e:.3e} (bound {b:.3e})" for k, (e, b) in errs.items()))
    assert fig["wrong_clear"] == 0 and fig["excess"] <= 1.0 and fig["not_lowest"] == 0, fig
    assert torch.equal(out["counts"].cpu(), counts)
    for k, (err, bound) in errs.items():
        assert err <= bound, (k, err, bound)
    return a


@pytest.mark.parametrize("name", NAMES)
def test_step_parity(name):
    """One row, one centre, one column; below one tile; three chunks with a partial last one and Mp = 64 (n150_m33_d5); a
    row stride above D and Dp = 128 (n300_m96_d65); two slabs and four chunks of centres per wave (n1100_m1024_d384);
    D = 640 with more centres than rows (n65_m129_d640)."""
    from cgat_amd import gp
    c = K.case(name)
    X, Z = c["inp"]["X"], c["inp"]["Z"]
    out = gp.kmeans_step(_device_rows(X, c["ldx_pad"]), Z, chunk_rows=c["chunk_rows"])
    _check_step(name, out, X, Z, c["step"])


def _special_step(name):
    from cgat_amd import gp
    sp = K.special(name)
    out = gp.kmeans_step(_device_rows(sp["X"], sp["ldx_pad"]), sp["Z"], chunk_rows=sp["chunk_rows"])
    return sp, out, _check_step(name, out, sp["X"], sp["Z"], sp["step"])


def test_rows_at_the_mean_of_the_centres_never_receive_a_padded_centre():
    """M = 33 pads to 64 centres whose image and norm are zero: for a row at the centroid their "distance" is 0."""
    _, _, a = _special_step("centroid_rows")
    assert int(a.max()) < 33


def test_duplicated_centres_use_the_lower_index():
    sp, out, a = _special_step("duplicates")
    first, copies = sp["marked"]
    assert int((a == first).sum()) > 0 and not any(int((a == m).sum()) for m in copies)
    assert all(float(out["counts"][m]) == 0.0 and float(out["sums"][m].abs().max()) == 0.0 for m in copies)


def test_a_centre_far_from_the_data_stays_where_it_is():
    import cgat_amd as P
    sp, out, _ = _special_step("far_centre")
    X, Z0, m = sp["X"], sp["Z"], sp["marked"]
    assert float(out["counts"][m]) == 0.0 and float(out["wss"][m]) == 0.0
    Z, report = P.kmeans_inducing_points(X.to(DEV), Z0, iters=1, chunk_rows=64)
    assert report["empty"] == [1] and report["iterations"] == 1 and not report["converged"]
    assert torch.equal(Z[m], Z0[m]) and not torch.equal(Z[0], Z0[0])
    want = K.update(Z0, sp["step"])
    assert float((Z - want).abs().max()) <= K.PARITY * float((want.double() - want.double().mean(0)).abs().max())


@pytest.mark.parametrize("name", LLOYD)
def test_lloyd_loop_follows_the_restatement(name):
    import cgat_amd as P
    c = K.lloyd_case(name)
    X, ref, M = c["inp"]["X"], c["ref"], c["M"]
    Xd = X.to(DEV)
    scale = float((ref["Z"][-1].double() - ref["Z"][-1].double().mean(0)).abs().max())
    for k in range(K.LLOYD_ITERS + 1):
        Z, report = P.kmeans_inducing_points(Xd, M, iters=k, seed=c["seed"], chunk_rows=c["chunk_rows"])
        assert Z.dtype == torch.float32 and Z.device.type == "cpu" and Z.shape == (M, c["D"])
        done = min(k, ref["iterations"])                           # updates made after k steps
        evaluated = min(k, len(ref["inertia"]))
        assert report["iterations"] == done and report["empty"] == ref["empty"][:done]
        assert report["converged"] == (k > ref["iterations"])
        assert float((Z - ref["Z"][done]).abs().max()) <= K.PARITY * scale
        got, want = report["inertia"], ref["inertia"][:evaluated]
        assert len(got) == evaluated and all(abs(a - b) <= K.PARITY * b for a, b in zip(got, want)), (got, want)
        assert all(b <= a for a, b in zip(got, got[1:])), got
        if k == 0:
            assert torch.equal(Z, c["Z0"])                         # the subset GPHead.fit draws, bit for bit
        if done < len(ref["steps"]):                               # the assignment the next step would evaluate
            a = _check_step(f"{name} step {done}", P.gp.kmeans_step(Xd, Z, chunk_rows=c["chunk_rows"]), X, Z)
            assert torch.equal(a, ref["steps"][done]["assign"])


def test_iters_zero_is_the_subset_of_fit():
    import cgat_amd as P
    c = K.lloyd_case("n300_m9_d7")
    Xd, yd = c["inp"]["X"].to(DEV), c["inp"]["y"].to(DEV)
    Z, report = P.kmeans_inducing_points(Xd, 9, iters=0, seed=3)
    head, _ = P.GPHead.fit(Xd, yd, inducing_points=9, lengthscale=4.0, seed=3)
    assert torch.equal(Z, head.inducing_points.cpu())
    assert report == dict(iterations=0, converged=False, inertia=[], empty=[])


def test_two_runs_bitwise_equal():
    """Two slabs, eight tiles of (M, D), four chunks of centres per wave: everything repeats bit for bit."""
    import cgat_amd as P
    c = K.case("n1100_m1024_d384")
    Xd, Z = c["inp"]["X"].to(DEV), c["inp"]["Z"]
    a, b = (P.gp.kmeans_step(Xd, Z) for _ in range(2))
    assert all(torch.equal(a[k], b[k]) for k in ("assign", "counts", "wss", "sums"))
    (Z1, r1), (Z2, r2) = (P.kmeans_inducing_points(Xd, Z, iters=2) for _ in range(2))
    assert torch.equal(Z1, Z2) and r1 == r2


def test_fit_keeps_the_start_with_the_larger_bound():
    import cgat_amd as P
    c = K.lloyd_case("n300_m9_d7")
    X, y, M, seed = c["inp"]["X"], c["inp"]["y"], c["M"], c["seed"]
    Xd, yd = X.to(DEV), y.to(DEV)
    kw = dict(inducing_points=M, lengthscale=[3.0, 6.0], outputscale=1.3, seed=seed)
    head, report = P.GPHead.fit(Xd, yd, init=("subset", "kmeans"), kmeans_iters=K.LLOYD_ITERS, **kw)
    rows = report["candidates"]
    assert [(r["init"], r["lengthscale"]) for r in rows] == [("subset", 3.0), ("subset", 6.0), ("kmeans", 3.0), ("kmeans", 6.0)]
    assert report["elbo"] == max(r["elbo"] for r in rows)
    best = max(rows, key=lambda r: r["elbo"])
    assert report["init"] == best["init"] and report["lengthscale"] == best["lengthscale"]
    assert report["kmeans"]["converged"] and report["kmeans"]["iterations"] == c["ref"]["iterations"]
    Zk, _ = P.kmeans_inducing_points(Xd, M, iters=K.LLOYD_ITERS, seed=seed)
    starts = {"subset": c["Z0"], "kmeans": Zk}
    assert torch.equal(head.inducing_points.cpu(), starts[report["init"]])
    for r in rows:                                                  # every candidate is the restated bound at its start
        want = K.restated_elbo(X, y, starts[r["init"]], 1.3, r["lengthscale"])
        print(f"[gp-kmeans] fit {r['init']} l = {r['lengthscale']}: elbo {r['elbo']:.4f}, restated {want:.4f}")
        assert abs(r["elbo"] - want) <= F.ELBO_REL_BOUND * abs(want)


def test_fit_init_subset_is_the_fit_without_init():
    import cgat_amd as P
    from cgat_amd import gp
    c = K.lloyd_case("n150_m6_d5")
    Xd, yd = c["inp"]["X"].to(DEV), c["inp"]["y"].to(DEV)
    kw = dict(inducing_points=6, seed=c["seed"], chunk_rows=64)
    (h0, r0), (h1, r1) = P.GPHead.fit(Xd, yd, **kw), P.GPHead.fit(Xd, yd, init="subset", **kw)
    assert set(r0) == {"noise", "elbo", "elbo_per_point", "constant", "lengthscale", "outputscale", "candidates"}
    assert all("init" not in r for r in r0["candidates"])
    assert all(torch.equal(getattr(h0, k), getattr(h1, k)) for k in gp._KEYS)
    assert r1["init"] == "subset" and r1["kmeans"] is None and all(r["init"] == "subset" for r in r1["candidates"])
    assert {k: r1[k] for k in r0 if k != "candidates"} == {k: r0[k] for k in r0 if k != "candidates"}
    assert [{k: v for k, v in r.items() if k != "init"} for r in r1["candidates"]] == r0["candidates"]
    assert torch.equal(h0.inducing_points.cpu(), c["Z0"]) and r0["lengthscale"] == gp.median_lengthscale(c["Z0"])


def test_fit_init_kmeans_starts_from_the_kmeans_centres():
    """The head's Z is kmeans_inducing_points' Z, "median" is taken from it, and the bound is the restated one there."""
    import cgat_amd as P
    from cgat_amd import gp
    c = K.lloyd_case("n150_m6_d5")
    X, y = c["inp"]["X"], c["inp"]["y"]
    Xd, yd = X.to(DEV), y.to(DEV)
    head, report = P.GPHead.fit(Xd, yd, inducing_points=6, seed=c["seed"], chunk_rows=64, init="kmeans", kmeans_iters=3)
    Zk, rk = P.kmeans_inducing_points(Xd, 6, iters=3, seed=c["seed"], chunk_rows=64)
    assert torch.equal(head.inducing_points.cpu(), Zk) and report["kmeans"] == rk and report["init"] == "kmeans"
    assert float((Zk - c["ref"]["Z"][3]).abs().max()) <= K.PARITY * float(c["ref"]["Z"][3].abs().max())
    assert report["lengthscale"] == gp.median_lengthscale(Zk) and len(report["candidates"]) == 1
    want = K.restated_elbo(X, y, Zk, 1.0, report["lengthscale"])
    assert abs(report["elbo"] - want) <= F.ELBO_REL_BOUND * abs(want), (report["elbo"], want)
    # a [M, D] start is used as it is, whatever `init` says
    h2, r2 = P.GPHead.fit(Xd, yd, inducing_points=c["Z0"], lengthscale=4.0, init="kmeans")
    assert torch.equal(h2.inducing_points.cpu(), c["Z0"]) and r2["kmeans"] is None and r2["init"] == "given"


def test_learn_ascends_from_the_winning_start():
    import cgat_amd as P
    c = K.lloyd_case("n150_m6_d5")
    Xd, yd = c["inp"]["X"].to(DEV), c["inp"]["y"].to(DEV)
    head, report = P.GPHead.fit(Xd, yd, inducing_points=6, seed=c["seed"], lengthscale=4.0, init=("kmeans", "subset"),
                                kmeans_iters=K.LLOYD_ITERS, learn=("lengthscale",), max_iter=3)
    rows = report["candidates"]
    assert [r["init"] for r in rows] == ["kmeans", "subset"]
    best = max(rows, key=lambda r: r["elbo"])
    # the ascent's first evaluation is the winner's bound (log l passes through exp), not the other start's
    assert report["init"] == best["init"] and abs(report["steps"][0] - best["elbo"]) <= 1e-6 * abs(best["elbo"])
    assert report["elbo"] >= report["steps"][0]
    Zk, _ = P.kmeans_inducing_points(Xd, 6, iters=K.LLOYD_ITERS, seed=c["seed"])
    assert torch.equal(head.inducing_points.cpu(), {"subset": c["Z0"], "kmeans": Zk}[report["init"]])


def test_refusals():
    import cgat_amd as P
    from cgat_amd._lib import CgatHipError
    g = torch.Generator().manual_seed(0)
    X = torch.randn(1100, 8, generator=g).to(DEV)
    with pytest.raises(CgatHipError, match="M <= 1024"):
        P.kmeans_inducing_points(X, 1025, iters=1)
    with pytest.raises(CgatHipError, match="M <= 1024"):
        P.gp.kmeans_step(X, X[:1025].cpu())
    with pytest.raises(ValueError, match="inducing points from"):
        P.kmeans_inducing_points(X[:5], 6)
    with pytest.raises(ValueError, match="multiple of 32"):
        P.kmeans_inducing_points(X, 8, chunk_rows=48)
    with pytest.raises(ValueError, match="width"):
        P.kmeans_inducing_points(X, X[:8, :7].cpu())
