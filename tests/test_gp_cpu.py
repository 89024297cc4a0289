"""CPU-side checks of the sparse-GP head (cgat_amd/gp.py, csrc/gphead.hip): the arithmetic restated in fp64 in two forms,
the fp32 floor the GPU tolerance is held against, the ABI entries, and the host-side plumbing of GPHead.  No compute call
of the library is made here."""
import ctypes as C
import os
import re

import pytest
import torch

import gp_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(gp_cases.CASES))
def test_restatement_forms_agree(name):
    """Factor form and interp^T (S - I) interp agree to 1e-10 in fp64, on every case of the GPU parity test."""
    p, X, ref = gp_cases.case(name)
    direct = gp_cases.direct_form(p, X)
    for k in ("mean_f", "var_f", "pred", "lower", "upper"):
        assert float((ref[k] - direct[k]).abs().max()) <= 1e-10, k
    assert float(ref["var_f"].min()) > 0


@pytest.mark.parametrize("name", sorted(gp_cases.CASES))
def test_fp32_floor_of_the_cases(name):
    """An eager fp32 evaluation of the factor form stays below 2.5e-5 of the parity norms (a quarter of the 1e-4 bound):
    the inputs leave the tolerance its margin."""
    p, X, ref = gp_cases.case(name)
    got = gp_cases.factor_form(p, X, dtype=torch.float32)
    for k, (err, bound) in gp_cases.errors(got, ref, p).items():
        assert err <= 0.25 * bound, (k, err, bound)


def test_abi_declares_gp_entries():
    from cgat_amd import _lib
    src = open(os.path.join(ROOT, "include", "cgat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for n in ("cgat_gp_predict_workspace_bytes", "cgat_gp_predict"):
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert _lib.lib.cgat_abi_version() == 3
    assert _lib.lib.cgat_gp_predict_workspace_bytes(1000000, 1000, 384) == 0


def test_packed_image_layout():
    """gp._pack_image against the layout include/cgat_hip.h states."""
    from cgat_amd import gp
    R, Kd = 64, 24
    P = torch.arange(R * Kd, dtype=torch.float32).view(R, Kd)
    img = gp._pack_image(P)
    for c, k8, lane, q in ((0, 0, 0, 0), (1, 2, 37, 3), (0, 1, 63, 1), (1, 0, 31, 2)):
        assert img[((c * (Kd // 8) + k8) * 64 + lane) * 4 + q] == P[32 * c + (lane & 31), 8 * k8 + 2 * q + (lane >> 5)]


def test_factor_image_and_invalidation():
    """prepare() on host buffers: padded sizes, W1 lower triangular, a / |z|^2 against the restatement; the image is
    reused until a buffer changes in place."""
    import cgat_amd as P
    p, X, _ = gp_cases.case("g257_m37_d5")
    head = P.GPHead.from_tensors(p)
    im = head.prepare()
    M, D, Mp, Dp = 37, 5, 64, 64
    assert im["zimg"].numel() == Mp * Dp and im["factors"].numel() == Mp + 2 * Mp * Mp and im["znorm"].numel() == Mp
    _, _, a, W1, W2 = gp_cases._factors64(p, gp_cases.JITTER)
    assert torch.allclose(im["factors"][:M].double(), a, rtol=1e-6, atol=0)
    assert float(im["factors"][M:Mp].abs().max()) == 0
    # unpack the image: float4 (c, k8, lane), element q
    F = im["factors"][Mp:].view(2 * Mp // 32, Mp // 8, 2, 32, 4).permute(0, 3, 1, 4, 2).reshape(2 * Mp, Mp)
    assert torch.allclose(F[:M, :M].double(), W1, rtol=1e-6, atol=1e-12)
    assert torch.allclose(F[Mp:Mp + M, :M].double(), W2, rtol=1e-6, atol=1e-12)
    assert float(F[:Mp].triu(1).abs().max()) == 0 and float(F[M:Mp].abs().max()) == 0
    assert head.prepare() is im
    with torch.no_grad():
        head.variational_mean.mul_(2.0)
    im2 = head.prepare()
    assert im2 is not im and torch.allclose(im2["factors"][:M], 2 * im["factors"][:M], rtol=1e-6)


def test_head_refuses_cpu_and_wrong_dtype_and_keys():
    import cgat_amd as P
    p, X, _ = gp_cases.case("g64_m64_d16")
    head = P.GPHead.from_tensors(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        head.predict(X)
    with pytest.raises(KeyError):
        P.GPHead.from_tensors({k: v for k, v in p.items() if k != "std"})
    with pytest.raises(ValueError):
        P.GPHead(p["inducing_points"], p["variational_mean"][:-1], p["chol_variational_covar"])
