"""CPU-side checks of the derivative of the sparse-GP head's prediction in its input (cgat_amd/gp.py, csrc/gpback.hip,
DESIGN 10g): the two fp64 references against each other and against the decomposition, the fp32 floors the GPU tolerances
are held against, the reduction of the five outputs' gradients to (gm, gv), the ABI entry and its refusals.  No compute
call of the library is made here.

The tests of the references and the floors check the restatement of tests/gp_predict_grad_cases.py alone and pass without
the package; the adjoint, ABI, refusal and export tests fail where the package lacks the feature."""
import ctypes as C
import os
import re

import pytest
import torch

import gp_cases
import gp_predict_grad_cases as Pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(Pc.NAMES)
f64 = torch.float64


@pytest.mark.parametrize("name", NAMES)
def test_references_and_decomposition_agree(name):
    """Autograd through the factor form against autograd through the direct form, and the decomposition against both:
    1e-10 of max |dL/dX|, per arm."""
    c = Pc.case(name)
    for arm in Pc.ARMS:
        a = c["arms"][arm]
        assert a["ref"].shape == (c["G"], c["D"]) and a["ref"].dtype == f64
        between, dec = Pc.deviation(a["direct"], a["ref"]), Pc.deviation(a["dX"], a["ref"])
        print(f"[gp-predict-grad] {name} {arm}: direct against factor form {between:.2e}, decomposition {dec:.2e}, "
              f"max |dL/dX| {float(a['ref'].abs().max()):.3e}")
        assert between <= 1e-10 and dec <= 1e-10


def _over_threads(measure):
    worst, threads = 0.0, torch.get_num_threads()
    try:
        for th in (1, 2, 8):
            torch.set_num_threads(th)
            worst = max(worst, measure())
    finally:
        torch.set_num_threads(threads)
    return worst


@pytest.mark.parametrize("name", NAMES)
def test_fp32_floor_of_the_gradient(name):
    """The eager fp32 dL/dX against fp64 autograd, of max |dL/dX| of the arm, with 1, 2 and 8 threads: at or below
    gp_predict_grad_cases.GRADIENT_FLOOR, which lies at or below a quarter of PARITY, so that the GPU bound is PARITY."""
    c = Pc.case(name)
    for arm in Pc.ARMS:
        a = c["arms"][arm]
        worst = _over_threads(lambda: Pc.deviation(Pc.gradient32(c["p"], c["X"], a["gm"], a["gv"]), a["ref"]))
        print(f"[gp-predict-grad floor] {name} {arm}: dL/dX {worst:.2e}")
        assert worst <= Pc.GRADIENT_FLOOR[arm], (arm, worst)
        assert Pc.GRADIENT_FLOOR[arm] <= 0.25 * Pc.PARITY and Pc.gradient_bound(arm) == Pc.PARITY


def test_fp32_floor_of_the_nlpd_weight_gradient():
    """d mean(nlpd) / dW of the eager fp32 arm (embeddings, prediction, adjoints, dL/dX and X0^T dX in fp32) against fp64
    autograd: at or below gp_predict_grad_cases.NLPD_WEIGHT_FLOOR, of which the GPU test allows four times."""
    nc = Pc.nlpd_case()
    worst = _over_threads(lambda: Pc.deviation(Pc.nlpd_weight_gradient32(nc), nc["ref"]))
    print(f"[gp-predict-grad floor] nlpd through a linear map: dL/dW {worst:.2e}")
    assert worst <= Pc.NLPD_WEIGHT_FLOOR, worst
    assert Pc.nlpd_weight_bound() == 4 * Pc.NLPD_WEIGHT_FLOOR


def test_latent_adjoints_match_autograd_through_the_outputs():
    """A weighted sum of mean_f, var_f, pred, lower, upper and uncertainty = upper - pred, composed by gp_cases._finish in
    fp64: (gm, gv) of latent_adjoints against torch autograd in (mean_f, var_f), 1e-12; subsets of the outputs as well."""
    from cgat_amd.gp import latent_adjoints
    g = torch.Generator().manual_seed(11)
    n, tm, ts = 50, torch.tensor(-0.3, dtype=f64), torch.tensor(2.5, dtype=f64)
    mean_f = torch.randn(n, generator=g, dtype=f64).requires_grad_(True)
    var_f = (0.05 + torch.rand(n, generator=g, dtype=f64)).requires_grad_(True)
    w = {k: torch.randn(n, generator=g, dtype=f64) for k in ("mean_f", "var_f", "pred", "lower", "upper", "unc")}
    for keep in (tuple(w), ("pred",), ("lower",), ("upper", "var_f"), ("unc",), ("mean_f",), ("var_f",)):
        out = gp_cases._finish(mean_f, var_f, tm, ts)
        out["unc"] = out["upper"] - out["pred"]
        loss = sum((w[k] * out[k]).sum() for k in keep)
        ref_m, ref_v = torch.autograd.grad(loss, (mean_f, var_f), allow_unused=True)
        part = lambda k: w[k] if k in keep else None
        add = lambda a, b: b if a is None else a if b is None else a + b
        unc = part("unc")
        grads = (part("mean_f"), part("var_f"), add(part("pred"), None if unc is None else -unc), part("lower"),
                 add(part("upper"), unc))
        gm, gv = latent_adjoints(grads, var_f.detach(), float(ts))
        for got, ref in ((gm, ref_m), (gv, ref_v)):
            assert (got is None) == (ref is None), keep
            if ref is not None:
                assert float((got - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1.0), keep


def test_latent_adjoints_at_the_clamp():
    """Rows whose var_f the forward clamped to 0: the whole gv of the row is 0, gm is what it is elsewhere, and nothing
    infinite or NaN leaves the function, in fp32 as the autograd function calls it."""
    from cgat_amd.gp import latent_adjoints
    g = torch.Generator().manual_seed(12)
    n = 40
    var_f = torch.rand(n, generator=g)
    zero = torch.zeros(n, dtype=torch.bool)
    zero[::3] = True
    var_f[zero] = 0.0
    var_f[1] = 1e-45                                       # the smallest positive fp32: 1 / sqrt stays finite
    grads = tuple(torch.randn(n, generator=g) for _ in range(5))
    gm, gv = latent_adjoints(grads, var_f, 2.5)
    assert gm.dtype == gv.dtype == torch.float32
    assert bool((gv[zero] == 0).all()) and bool(torch.isfinite(gv).all()) and bool(torch.isfinite(gm).all())
    assert bool((gv[~zero] != 0).all())
    assert torch.equal(gm, grads[0] + 2.5 * grads[2] + 2.5 * grads[3] + 2.5 * grads[4])
    # the region alone, and nothing at all
    gm, gv = latent_adjoints((None, None, None, grads[3], None), var_f, 2.5)
    assert bool((gv[zero] == 0).all()) and bool(torch.isfinite(gv).all()) and torch.equal(gm, 2.5 * grads[3])
    assert latent_adjoints((None,) * 5, var_f, 2.5) == (None, None)


def test_abi_declares_the_entry():
    from cgat_amd import _lib
    src = open(os.path.join(ROOT, "include", "cgat_hip.h")).read()
    assert "gaussian_process.py:247-268" in src[src.index("backward of cgat_gp_predict"):]
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for n in ("cgat_gp_predict_backward", "cgat_gp_predict_backward_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % n, src)
        assert n in _lib.PROTOTYPES and hasattr(lib, n)
    assert _lib.ABI_VERSION == 3 and lib.cgat_abi_version() == 3
    assert _lib.PROTOTYPES["cgat_gp_predict_backward_workspace_bytes"] == _lib.PROTOTYPES["cgat_gp_fit_grad_workspace_bytes"]


def test_entry_refuses_bad_arguments_before_any_launch():
    """What cgat_gp_fit_grad_inputs refuses, and both upstream gradients null, from host memory that no kernel could read:
    every refusal precedes the launches."""
    from cgat_amd import _lib
    lib = _lib.lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(G=100, M=8, D=4, ldx=4, chunk=32, ws=p, ws_bytes=1 << 40, X=p, img=p, ztimg=p, dX=p, lddx=4, gm=p, gv=p):
        return lib.cgat_gp_predict_backward(X, ldx, G, D, img, M, p, p, p, p, p, p, gm, gv, 1.0, 0.5, chunk, ztimg, dX, lddx,
                                            ws, ws_bytes, None)

    def message():
        return lib.cgat_last_error().decode(errors="replace")

    assert call(M=1025) == 4 and "M <= 1024" in message()
    assert call(G=0) == 1 and call(chunk=48) == 1 and call(ldx=3) == 1 and call(X=None) == 1
    assert call(img=C.c_void_p(p.value + 4)) == 1 and "16-byte" in message()
    assert call(dX=None) == 1 and "gp_predict_backward: null" in message()
    assert call(ztimg=None) == 1 and "null" in message()
    assert call(gm=None, gv=None) == 1 and "null" in message()
    assert call(lddx=3) == 1 and "lddx" in message()
    assert call(ztimg=C.c_void_p(p.value + 4)) == 1 and "16-byte" in message()
    need = lib.cgat_gp_predict_backward_workspace_bytes(100, 8, 4, 32)
    assert need > 0 and lib.cgat_gp_predict_backward_workspace_bytes(100, 1025, 4, 32) == 0
    assert call(ws_bytes=need - 1) == 3 and "workspace" in message()
    assert call(ws=None) == 3


def test_public_functions_are_exported_and_refuse_cpu_tensors():
    import cgat_amd as P
    p, X, _ = gp_cases.case("g64_m64_d16")
    for n in ("predictive_backward", "latent_adjoints"):
        assert getattr(P, n) is getattr(P.gp, n) and n in P.__all__
    assert callable(P.GPHead.nlpd) and callable(P.GPHead.prepare_backward)
    head = P.GPHead.from_tensors(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.predictive_backward(head, X, torch.ones(X.shape[0]), None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head.nlpd(X.clone().requires_grad_(True), torch.zeros(X.shape[0]), 0.1)
    with pytest.raises(ValueError, match="noise"):
        head.nlpd(X, torch.zeros(X.shape[0]), 0.0)
