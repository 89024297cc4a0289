"""CPU-side checks of the gradient of the collapsed sparse-GP bound (cgat_amd/gp.py, csrc/gpgrad.hip): the
decomposition into device sums and a host part against torch autograd of the dense bound in fp64, the envelope argument
by central differences of the re-solved bound, the host functions of the package against the restatement, the fp32
floors the GPU tolerances are held against, the optimiser's case, the ABI entries and the refusals.  No compute call of
the library is made here.

The two tests of the fp32 floors check the restatement of tests/gp_grad_cases.py alone: they hold the recorded figures
the GPU bounds are derived from, and pass without the package.  Every other test runs the package's host functions, its
ABI or its refusals and fails where it lacks the gradient."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import gp_fit_cases as F
import gp_grad_cases as Gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(Gc.NAMES)


def _package_totals(c):
    """The three gradients with the host side of the package (collapsed_adjoints, whitening_pullback at the restated
    solution) around the fp64 blocks of the restatement."""
    from cgat_amd import gp
    fit, inp = c["fit"], c["inp"]
    adj = gp.collapsed_adjoints(fit["gram"], c["N"], c["s"], fit["sol"])
    pull = gp.whitening_pullback(inp["Z"], c["ell"], c["s"], Gc.JITTER, adj["dF_dW1"])
    host = {k: torch.as_tensor(pull[k], dtype=torch.float64).reshape(c["host"][k].shape) for k in Gc.GRADS}
    blk = Gc.blocks64(inp["X"], c["y_norm"], inp["Z"], c["s"], c["ell"], c["c"], adj["G_hat"], adj["g"])
    return Gc.totals(blk, inp["Z"], c["ell"], adj, host)


@pytest.mark.parametrize("name", NAMES)
def test_decomposition_equals_autograd(name):
    """Blocks + host part against autograd of the dense bound at fixed (c, v): 1e-9 of each gradient's max-norm, for the
    restatement and with the package's host functions in its place; the sum of colsum is the data part of dF/dlog s."""
    c = Gc.case(name)
    dev = Gc.deviations(c["grads"], c["autograd"])
    own = Gc.deviations(_package_totals(c), c["autograd"])
    print(f"[gp-grad] {name}: " + ", ".join(f"{k} {v:.2e} ({own[k]:.2e})" for k, v in dev.items()))
    assert all(v <= 1e-9 for v in dev.values()), dev
    assert all(v <= 1e-9 for v in own.values()), own
    assert abs(c["dense"] - c["fit"]["sol"]["elbo"]) <= 1e-10 * abs(c["dense"])
    data_s = c["adj"]["log_outputscale"] + c["N"] * c["s"] / (2 * c["v"])
    assert abs(float(c["blocks"]["colsum"].sum()) - data_s) <= 1e-10 * float(c["blocks"]["colsum"].abs().sum())


@pytest.mark.parametrize("name", NAMES)
def test_central_differences_of_the_resolved_bound(name):
    """F* with c and sigma^2 searched again at l e^{+-h} and s e^{+-h}, h = 1e-4: the envelope argument, 1e-6 relative."""
    c = Gc.case(name)
    inp, N, s, ell, h = c["inp"], c["N"], c["s"], c["ell"], 1e-4
    fd_l = (Gc.resolved_bound(inp, c["y_norm"], N, s, ell * math.exp(h))
            - Gc.resolved_bound(inp, c["y_norm"], N, s, ell * math.exp(-h))) / (2 * h)
    fd_s = (Gc.resolved_bound(inp, c["y_norm"], N, s * math.exp(h), ell)
            - Gc.resolved_bound(inp, c["y_norm"], N, s * math.exp(-h), ell)) / (2 * h)
    for grads in (c["grads"], _package_totals(c)):
        gl, gs = float(grads["log_lengthscale"]), float(grads["log_outputscale"])
        print(f"[gp-grad] {name}: dlog l {gl:.6e} (differences {fd_l:.6e}), dlog s {gs:.6e} (differences {fd_s:.6e})")
        assert abs(fd_l - gl) <= 1e-6 * abs(gl) and abs(fd_s - gs) <= 1e-6 * abs(gs)


@pytest.mark.parametrize("name", NAMES)
def test_host_functions_equal_the_restatement(name):
    from cgat_amd import gp
    c = Gc.case(name)
    fit, inp, adj = c["fit"], c["inp"], c["adj"]
    got = gp.collapsed_adjoints(fit["gram"], c["N"], c["s"], fit["sol"])
    assert set(got) == {"G_hat", "g", "dF_dW1", "log_outputscale"}
    for k, ref in (("G_hat", adj["G_hat"]), ("g", adj["g"]), ("dF_dW1", adj["T"])):
        assert got[k].dtype == torch.float64
        assert float((got[k] - ref).abs().max()) <= 1e-9 * float(ref.abs().max()), k
    assert abs(got["log_outputscale"] - adj["log_outputscale"]) <= 1e-9 * abs(adj["log_outputscale"])
    assert torch.equal(got["G_hat"], got["G_hat"].T)
    pull = gp.whitening_pullback(inp["Z"], c["ell"], c["s"], Gc.JITTER, adj["T"])
    assert set(pull) == set(Gc.GRADS)
    for k in Gc.GRADS:
        ref = c["host"][k]
        got_k = torch.as_tensor(pull[k], dtype=torch.float64).reshape(ref.shape)
        assert float((got_k - ref).abs().max()) <= 1e-9 * float(ref.abs().max()), k


@pytest.mark.parametrize("name", NAMES)
def test_fp32_floor_of_the_blocks(name):
    """The eager fp32 blocks against the fp64 blocks, each of its block's max-norm, with 1, 2 and 8 threads and chunks of
    1024 and 4096 rows: at or below the figure recorded in gp_grad_cases.BLOCK_FLOOR.  A block whose floor is at or below
    a quarter of PARITY is held to PARITY on the GPU, the others to four times their floor (block_bound)."""
    c = Gc.case(name)
    inp, adj = c["inp"], c["adj"]
    worst = {k: 0.0 for k in Gc.BLOCKS}
    threads = torch.get_num_threads()
    try:
        for th in (1, 2, 8):
            torch.set_num_threads(th)
            for chunk in (1024, 4096):
                b32 = Gc.blocks32(inp["X"], c["y_norm"], inp["Z"], c["s"], c["ell"], c["c"], adj["G_hat"], adj["g"], chunk=chunk)
                for k, v in Gc.deviations(b32, c["blocks"]).items():
                    worst[k] = max(worst[k], v)
    finally:
        torch.set_num_threads(threads)
    print(f"[gp-grad floor] {name}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k in Gc.BLOCKS:
        assert worst[k] <= Gc.BLOCK_FLOOR[k], (k, worst[k])
    assert Gc.BLOCK_FLOOR["P"] <= 0.25 * Gc.PARITY and Gc.block_bound("P") == Gc.PARITY
    for k in ("colsum", "d2sum"):                     # above a quarter of PARITY (n1100_m1024_d384): four times the floor
        assert Gc.BLOCK_FLOOR[k] > 0.25 * Gc.PARITY and Gc.block_bound(k) == 4 * Gc.BLOCK_FLOOR[k]


@pytest.mark.parametrize("name", NAMES)
def test_fp32_floor_of_the_total_gradients(name):
    """The three gradients of the eager fp32 arm (statistics and blocks in fp32, solve, adjoints and host part in fp64)
    against autograd in fp64: at or below gp_grad_cases.TOTAL_FLOOR, of which the GPU test allows four times."""
    c = Gc.case(name)
    worst = {k: 0.0 for k in Gc.GRADS}
    threads = torch.get_num_threads()
    try:
        for th in (1, 8):
            torch.set_num_threads(th)
            for chunk in (1024, 4096):
                for k, v in Gc.deviations(Gc.gradients32(c, chunk), c["autograd"]).items():
                    worst[k] = max(worst[k], v)
    finally:
        torch.set_num_threads(threads)
    print(f"[gp-grad floor] {name}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k in Gc.GRADS:
        assert worst[k] <= Gc.TOTAL_FLOOR[k], (k, worst[k])


def test_lbfgs_on_the_restatement_reaches_an_interior_optimum():
    """n600_m96_d5 from l = 2 sqrt(D), s = 1.3: fp64 L-BFGS over (log l, log s) ends above all three grid bounds, strictly
    inside the default box, at the figures recorded in gp_grad_cases.FIT_OPTIMUM."""
    from cgat_amd import gp
    f = Gc.fit_case()
    rec, D = Gc.FIT_OPTIMUM, Gc.FIT_CASE["D"]
    print(f"[gp-grad fit] grid {f['grid']}, optimum l {f['lengthscale']:.6f} (l / sqrt(D) {f['lengthscale'] / math.sqrt(D):.4f}), "
          f"s {f['outputscale']:.6f}, noise {f['noise']:.6f}, F* {f['elbo']:.5f}, {f['evaluations']} evaluations, "
          f"gradient norm {f['grad_norm']:.1e}, rel_l {f['rel_l']:.5f}, rel_s {f['rel_s']:.5f}")
    assert all(f["elbo"] > v + 10.0 for v in f["grid"].values())
    assert f["grad_norm"] <= 1e-3 and f["evaluations"] <= 40
    assert float(torch.linalg.eigvalsh(f["hessian"]).max()) < 0                      # a maximum
    assert gp.DEFAULT_BOUNDS == Gc.DEFAULT_BOX
    l0, s0 = f["inp"]["lengthscale"], f["inp"]["outputscale"]
    (ll, lh), (sl, sh) = Gc.DEFAULT_BOX["lengthscale"], Gc.DEFAULT_BOX["outputscale"]
    assert ll * l0 < f["lengthscale"] < lh * l0 and sl * s0 < f["outputscale"] < sh * s0
    for k in ("lengthscale", "outputscale", "noise", "elbo"):
        assert abs(f[k] - rec[k]) <= 1e-5 * abs(rec[k]), k
    for k in ("rel_l", "rel_s"):
        assert abs(f[k] - rec[k]) <= 1e-2 * rec[k], k


def test_abi_declares_gp_grad_entries():
    from cgat_amd import _lib
    src = open(os.path.join(ROOT, "include", "cgat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for n in ("cgat_gp_fit_grad_workspace_bytes", "cgat_gp_fit_grad"):
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in _lib.PROTOTYPES and hasattr(lib, n), n
    assert _lib.lib.cgat_abi_version() == 3


def test_workspace_query():
    from cgat_amd import _lib
    q = _lib.lib.cgat_gp_fit_grad_workspace_bytes
    for N, M, D in ((1000000, 1000, 384), (1100, 1024, 640), (70, 1, 1)):
        sizes = [q(N, M, D, ch) for ch in (32, 64, 1024, 1056, 4096, 32768, 65536)]
        assert all(v > 0 for v in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    # the chunk buffer [Ma_p][chunk] and the centred rows [D][chunk] are the floor of it; the partials of P stay small
    assert (1024 + 640) * 32768 * 4 <= q(1000000, 1024, 640, 32768) <= 512 * 2 ** 20
    assert q(100, 1025, 8, 32768) == 0 and q(100, 8, 8, 48) == 0 and q(0, 8, 8, 32) == 0      # what the entry refuses


# cgat_gp_fit_grad_workspace_bytes at the (N, M, D, chunk_rows) of every case of gp_fit_cases (None: the default of 32768)
WORKSPACE_BYTES = {"n70_m1_d1": 79360, "n150_m33_d5": 84224, "n300_m96_d65": 320256, "n1000_m129_d130": 1490944,
                   "n1100_m1000_d128": 6496256, "n1100_m1024_d384": 9883648, "n31_m30_d7": 71168}


def test_workspace_query_pinned():
    """The sizes the query has returned since the entry exists: the chunk plan it shares with the entry must not move them."""
    from cgat_amd import _lib
    q = _lib.lib.cgat_gp_fit_grad_workspace_bytes
    assert set(WORKSPACE_BYTES) == set(F.CASES)
    for name, kw in F.CASES.items():
        assert q(kw["N"], kw["M"], kw["D"], kw.get("chunk_rows") or 32768) == WORKSPACE_BYTES[name], name
    assert q(1000000, 1000, 384, 32768) == 243269632
    assert q(100, 1025, 8, 32768) == 0 and q(100, 8, 8, 48) == 0 and q(0, 8, 8, 32) == 0


def test_entry_refuses_bad_arguments_before_any_launch():
    """The sibling's codes and messages, from host memory that no kernel could read: every refusal precedes the launches."""
    from cgat_amd import _lib
    lib = _lib.lib
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(N=100, M=8, D=4, ldx=4, chunk=32, ws=p, ws_bytes=1 << 40, X=p, img=p):
        return lib.cgat_gp_fit_grad(X, ldx, p, N, D, img, M, p, p, p, p, p, p, 0.0, 1.0, 0.5, chunk, p, p, p, ws, ws_bytes, None)

    def message():
        return lib.cgat_last_error().decode(errors="replace")

    assert call(M=1025) == 4 and "M <= 1024" in message()
    assert call(N=0) == 1 and call(D=0) == 1 and call(M=0) == 1
    assert call(chunk=48) == 1 and "multiple of 32" in message()
    assert call(ldx=3) == 1 and "ldx" in message()
    assert call(X=None) == 1 and "null" in message()
    assert call(img=C.c_void_p(p.value + 4)) == 1 and "16-byte" in message()
    need = lib.cgat_gp_fit_grad_workspace_bytes(100, 8, 4, 32)
    assert call(ws_bytes=need - 1) == 3 and "workspace" in message()
    assert call(ws=None) == 3


def test_public_entry_points_refuse_cpu_dtype_and_arguments():
    import cgat_amd as P
    inp = F.case("n150_m33_d5")["inp"]
    X, y, Z = inp["X"], inp["y_stat"], inp["Z"]
    assert P.bound_and_gradient is P.gp.bound_and_gradient and "bound_and_gradient" in P.__all__
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.bound_and_gradient(X, y, Z, 1.3, 2.0)
    with pytest.raises(TypeError, match="float32"):
        P.bound_and_gradient(X.double(), y, Z, 1.3, 2.0)
    with pytest.raises(ValueError, match="width"):
        P.bound_and_gradient(X[:, :4], y, Z, 1.3, 2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.GPHead.fit(X, inp["y"], inducing_points=Z, lengthscale=2.0, learn=("lengthscale",))
