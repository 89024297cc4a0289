"""CPU-side checks of the gradient of the collapsed sparse-GP bound in the embeddings (cgat_amd/gp.py, gp_input_rows in
csrc/gpgrad.hip): the decomposition against torch autograd of the dense bound in fp64, the translation
identity that ties it to the data part of dF/dZ, the envelope argument by central differences through a linear map, the
fp32 floors the GPU tolerances are held against, the ABI entry and its refusals.  No compute call of the library is made
here.

The tests of the decomposition, the identity, the differences and the floors check the restatement of
tests/gp_input_grad_cases.py alone and pass without the package; the ABI, refusal and export tests fail where the package
lacks the entry."""
import ctypes as C
import os
import re

import pytest
import torch

import gp_grad_cases as Gc
import gp_input_grad_cases as Ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(Ic.NAMES)
LINEAR = list(Ic.LINEAR_NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_decomposition_equals_autograd(name):
    """(sum_m r_nm zc_m - rho_n xc_n) / l^2 against autograd of the dense bound in X at fixed (c, v): 1e-10 of max |dF/dX|."""
    c = Ic.case(name)
    assert c["dX"].shape == (c["N"], c["D"]) and c["dX"].dtype == torch.float64
    dev = Ic.deviation(c["dX"], c["ref"])
    print(f"[gp-input-grad] {name}: decomposition against autograd {dev:.2e}, max |dF/dX| {float(c['ref'].abs().max()):.3e}")
    assert dev <= 1e-10


@pytest.mark.parametrize("name", NAMES)
def test_translation_identity(name):
    """The bound does not change when X and Z move together, up to what passes through K_zz (which does not change at all):
    sum_n dF/dx_n = -sum_m (P - colsum o Zc)_m / l^2, the data part of dF/dZ."""
    c = Ic.case(name)
    lhs, rhs = c["dX"].sum(0), -c["dZ_data"].sum(0)
    scale = float(c["dX"].abs().sum(0).max())
    assert float((lhs - rhs).abs().max()) <= 1e-10 * scale
    assert float((c["ref"].sum(0) - rhs).abs().max()) <= 1e-10 * scale


@pytest.mark.parametrize("name", LINEAR)
def test_central_differences_through_a_linear_map(name):
    """Embeddings X0 @ W: F* with c and sigma^2 searched again at W +- h dW along dW = dF/dW / |dF/dW| against the analytic
    directional derivative <dF/dW, dW> at fixed (c, v) -- the envelope theorem for X -- 1e-6 relative; the decomposition
    X0^T dX against autograd in W, 1e-10."""
    lc = Ic.linear_case(name)
    assert Ic.deviation(lc["dW"], lc["ref"]) <= 1e-10
    assert abs(lc["dense"] - lc["elbo"]) <= 1e-10 * abs(lc["elbo"])
    W64 = lc["W"].to(torch.float64)
    direction = lc["ref"] / lc["ref"].norm()
    analytic = float((lc["ref"] * direction).sum())
    h = 1e-4
    fd = (Ic.resolved_bound_through(lc, W64 + h * direction) - Ic.resolved_bound_through(lc, W64 - h * direction)) / (2 * h)
    print(f"[gp-input-grad] {name}: <dF/dW, dW> {analytic:.8e} (differences {fd:.8e})")
    assert abs(fd - analytic) <= 1e-6 * abs(analytic)


@pytest.mark.parametrize("name", NAMES)
def test_fp32_floor_of_the_input_gradient(name):
    """The eager fp32 dF/dX against fp64 autograd, of max |dF/dX|, with 1, 2 and 8 threads and chunks of 1024 and 4096
    rows, at the case's fp64 adjoints: at or below gp_input_grad_cases.INPUT_FLOOR, which lies at or below a quarter of
    PARITY, so that the GPU bound is PARITY.  The arm with the statistics in fp32 as well is printed next to it and held
    below a quarter of PARITY, so that it leads to the same bound."""
    c = Ic.case(name)
    worst, worst32 = 0.0, 0.0
    threads = torch.get_num_threads()
    try:
        for th in (1, 2, 8):
            torch.set_num_threads(th)
            for chunk in (1024, 4096):
                at64, at32 = Ic.input_gradient32_of_case(c, chunk)
                worst, worst32 = max(worst, Ic.deviation(at64, c["ref"])), max(worst32, Ic.deviation(at32, c["ref"]))
    finally:
        torch.set_num_threads(threads)
    print(f"[gp-input-grad floor] {name}: dF/dX {worst:.2e}, with fp32 statistics {worst32:.2e}")
    assert worst <= Ic.INPUT_FLOOR, worst
    assert worst32 <= 0.25 * Ic.PARITY, worst32
    assert Ic.INPUT_FLOOR <= 0.25 * Ic.PARITY and Ic.input_bound() == Ic.PARITY


@pytest.mark.parametrize("name", LINEAR)
def test_fp32_floor_of_the_weight_gradient(name):
    """dF/dW of the eager fp32 arm (embeddings, statistics, dF/dX and X0^T dX in fp32) against fp64 autograd: at or below
    gp_input_grad_cases.WEIGHT_FLOOR, of which the GPU test of collapsed_bound allows four times."""
    lc = Ic.linear_case(name)
    worst = 0.0
    threads = torch.get_num_threads()
    try:
        for th in (1, 2, 8):
            torch.set_num_threads(th)
            for chunk in (1024, 4096):
                worst = max(worst, Ic.deviation(Ic.weight_gradient32(lc, chunk), lc["ref"]))
    finally:
        torch.set_num_threads(threads)
    print(f"[gp-input-grad floor] {name}: dF/dW {worst:.2e}")
    assert worst <= Ic.WEIGHT_FLOOR, worst
    assert Ic.weight_bound() == 4 * Ic.WEIGHT_FLOOR


def test_abi_declares_the_entry():
    from cgat_amd import _lib
    src = open(os.path.join(ROOT, "include", "cgat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    n = "cgat_gp_fit_grad_inputs"
    assert re.search(r"\b%s\s*\(" % n, src)
    assert n in _lib.PROTOTYPES and hasattr(lib, n)
    # the arguments of cgat_gp_fit_grad up to P, then Ztimg, dX, lddx, then the workspace and the stream
    base, new = _lib.PROTOTYPES["cgat_gp_fit_grad"][1], _lib.PROTOTYPES[n][1]
    assert new[:len(base) - 3] == base[:-3] and new[-3:] == base[-3:]
    assert new[len(base) - 3:-3] == [C.c_void_p, C.c_void_p, C.c_int64]


def test_entry_refuses_bad_arguments_before_any_launch():
    """What cgat_gp_fit_grad refuses, and a null dX or Ztimg, lddx < D and a misaligned Ztimg, from host memory that no
    kernel could read: every refusal precedes the launches."""
    from cgat_amd import _lib
    lib = _lib.lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(N=100, M=8, D=4, ldx=4, chunk=32, ws=p, ws_bytes=1 << 40, X=p, img=p, ztimg=p, dX=p, lddx=4):
        return lib.cgat_gp_fit_grad_inputs(X, ldx, p, N, D, img, M, p, p, p, p, p, p, 0.0, 1.0, 0.5, chunk, p, p, p, ztimg, dX,
                                           lddx, ws, ws_bytes, None)

    def message():
        return lib.cgat_last_error().decode(errors="replace")

    assert call(M=1025) == 4 and "M <= 1024" in message()
    assert call(N=0) == 1 and call(chunk=48) == 1 and call(ldx=3) == 1 and call(X=None) == 1
    assert call(img=C.c_void_p(p.value + 4)) == 1 and "16-byte" in message()
    assert call(dX=None) == 1 and "gp_fit_grad_inputs: null" in message()
    assert call(ztimg=None) == 1 and "null" in message()
    assert call(lddx=3) == 1 and "lddx" in message()
    assert call(ztimg=C.c_void_p(p.value + 4)) == 1 and "16-byte" in message()
    need = lib.cgat_gp_fit_grad_workspace_bytes(100, 8, 4, 32)
    assert call(ws_bytes=need - 1) == 3 and "workspace" in message()
    assert call(ws=None) == 3


def test_public_functions_are_exported_and_refuse_cpu_tensors():
    import inspect
    import cgat_amd as P
    inp = Gc.case("n150_m33_d5")["inp"]
    X, y, Z = inp["X"], inp["y_stat"], inp["Z"]
    for n in ("collapsed_bound", "deep_kernel_gradient"):
        assert getattr(P, n) is getattr(P.gp, n) and n in P.__all__
    assert inspect.signature(P.bound_and_gradient).parameters["wrt_embeddings"].default is False
    assert inspect.signature(P.gp._GradientPass.sums).parameters["input_grad"].default is False
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.bound_and_gradient(X, y, Z, 1.3, 2.0, wrt_embeddings=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.collapsed_bound(X, y, Z, 1.3, 2.0)
    with pytest.raises(TypeError, match="float32"):
        P.collapsed_bound(X.double(), y, Z, 1.3, 2.0)
