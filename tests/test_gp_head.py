"""The sparse-GP head on the GPU (cgat_amd.GPHead, cgat_gp_predict, csrc/gphead.hip) against the fp64 restatement of
tests/gp_cases.py, at the project's parity criterion (DESIGN: 1e-4 max-norm relative):

    max|d mean_f| <= 1e-4 max|mean_f - c|,   max|d var_f| <= 1e-4 s,   pred / lower / upper within 1e-4 of their max-norm

An eager fp32 evaluation of the same factor form sits at <= 2.5e-5 of these norms (tests/test_gp_cpu.py holds the inputs
to that), so the bound leaves the kernel a factor of four over plain fp32 rounding and nothing more."""
import math
import os
import subprocess
import sys

import pytest
import torch

import gp_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _head(p, **kw):
    import cgat_amd as P
    return P.GPHead.from_tensors(p, **kw).to(DEV)


def _all_outputs(head, X):
    mean_f, var_f = head.latent(X)
    pred, lower, upper = head.predict(X)
    return {k: v.cpu() for k, v in dict(mean_f=mean_f, var_f=var_f, pred=pred, lower=lower, upper=upper).items()}


@pytest.mark.parametrize("name", sorted(gp_cases.CASES))
def test_parity_with_fp64_restatement(name):
    """Ragged last row tile, M and D off the tile sizes, M at the bound, one row / one inducing point / one column, a row
    stride larger than D (g300_m1024_d384), the doubled lengthscale (g65_m129_d640), ZeroMean (g64_m64_d16)."""
    p, X, ref = gp_cases.case(name)
    Xd = torch.empty(X.shape[0], X.stride(0), device=DEV).fill_(1e30)[:, :X.shape[1]]
    Xd.copy_(X)
    assert Xd.stride(0) == X.stride(0)
    got = _all_outputs(_head(p), Xd)
    figures = gp_cases.errors(got, ref, p)
    print(f"[gp-head] {name}: " + ", ".join(f"{k} {e:.3e} (bound {b:.3e})" for k, (e, b) in figures.items()))
    for k, (err, bound) in figures.items():
        assert err <= bound, (k, err, bound)
    assert all(v.shape == (X.shape[0],) and v.dtype == torch.float32 and not v.requires_grad for v in got.values())


def test_rows_on_inducing_points_and_far_rows():
    """Rows copied from Z (d^2 = 0 up to rounding: the clamp) give finite outputs with var_f >= 0 and still meet the
    parity bound; rows at 1e3 lengthscales, where every kernel value underflows, give mean_f == c and var_f == s
    exactly (and the confidence region of the prior)."""
    p, X, _ = gp_cases.case("g257_m37_d5")
    Z, ell = p["inducing_points"], float(p["lengthscale"])
    far = Z[:3].clone()
    far[:, 0] += 1e3 * ell
    far[2, 1] -= 1e3 * ell
    Xs = torch.cat([Z[:20], far, X[:10]])
    ref = gp_cases.factor_form(p, Xs)
    got = _all_outputs(_head(p), Xs.to(DEV))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert float(got["var_f"].min()) >= 0
    for k, (err, bound) in gp_cases.errors(got, ref, p).items():
        assert err <= bound, (k, err, bound)
    c, s = p["constant"], p["outputscale"]
    assert torch.equal(got["mean_f"][20:23], c.expand(3)) and torch.equal(got["var_f"][20:23], s.expand(3))
    tm, ts = p["mean"], p["std"]
    assert torch.allclose(got["upper"][20:23] - got["pred"][20:23], (2 * s.sqrt() * ts).expand(3), rtol=1e-6)


def test_empty_input_and_uncertainty():
    p, X, _ = gp_cases.case("g64_m64_d16")
    head = _head(p)
    outs = head.predict(torch.empty(0, 16, device=DEV)) + head.latent(torch.empty(0, 16, device=DEV))
    assert all(o.shape == (0,) and o.dtype == torch.float32 and o.device.type == "cuda" for o in outs)
    Xd = X.to(DEV)
    pred, _, upper = head.predict(Xd)
    assert torch.equal(head.uncertainty(Xd), upper - pred)


def test_more_than_1024_inducing_points_is_refused():
    from cgat_amd._lib import CgatHipError
    p, X = gp_cases.build_inputs(4, 1025, 8)
    head = _head(p)
    with pytest.raises(CgatHipError, match="M <= 1024"):
        head.predict(X.to(DEV))


def test_refuses_wrong_dtype_and_width():
    p, X, _ = gp_cases.case("g64_m64_d16")
    head = _head(p)
    with pytest.raises(TypeError, match="float32"):
        head.predict(X.to(DEV).double())
    with pytest.raises(ValueError, match="width"):
        head.predict(X.to(DEV)[:, :15])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head.predict(X)


def test_two_runs_bitwise_equal_and_buffers_invalidate():
    p, X, ref = gp_cases.case("g33_m1000_d128")
    head = _head(p)
    Xd = X.to(DEV)
    a, b = _all_outputs(head, Xd), _all_outputs(head, Xd)
    assert all(torch.equal(a[k], b[k]) for k in a)
    with torch.no_grad():
        head.constant.add_(1.0)                       # a changed buffer rebuilds the image
    c = _all_outputs(head, Xd)
    assert torch.allclose(c["mean_f"], a["mean_f"] + 1.0, rtol=0, atol=1e-5)
    assert torch.equal(c["var_f"], a["var_f"])


def test_predict_batch_equals_predict_of_embedding():
    """predict_batch on a small CGAtNet / synthetic batch equals predict(model(..., return_graph_embedding=True)) bit
    for bit, and leaves the model's training flag as it found it."""
    import cgat_amd as P
    b, roost = P.synthetic_batch(6, 20, 12, seed=8)
    b = b.to(DEV)
    roost = tuple(t.to(DEV) for t in roost)
    torch.manual_seed(1)
    net = P.CGAtNet(200, 128, 2, msg_heads=3, neighbor_number=12, update_edges=True).to(DEV)
    net.eval()
    with torch.no_grad():
        emb = net(b, roost, return_graph_embedding=True)
    G, D = emb.shape
    assert G == 6
    g = torch.Generator().manual_seed(2)
    spread = float(emb.std()) + 1e-3
    M = 40
    Z = emb.cpu()[torch.randint(0, G, (M,), generator=g)] + 0.5 * spread * torch.randn(M, D, generator=g)
    p, _ = gp_cases.build_inputs(1, M, D)
    p["inducing_points"], p["lengthscale"] = Z, torch.tensor(spread * math.sqrt(D))
    head = _head(p)
    want = head.predict(emb)
    net.train()
    got = head.predict_batch(net, b, roost)
    assert net.training
    assert all(torch.equal(u, v) for u, v in zip(got, want))
    assert float((want[2] - want[0]).min()) >= 0 and all(bool(torch.isfinite(v).all()) for v in want)


def test_captured_call_replays_to_the_eager_result():
    """One predict() captured with torch.cuda.graph replays to the eager bits, also after its static input was
    overwritten (child process: tests/gp_capture_worker.py, as the other capture tests do)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gp_capture_worker.py")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "GP_CAPTURE_OK" in r.stdout, r.stdout[-2000:]
