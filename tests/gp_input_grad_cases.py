"""Shared by tests/test_gp_input_grad_cpu.py and tests/test_gp_input_grad.py: an fp64 torch restatement of the gradient of
the collapsed sparse-GP bound in the embeddings X, on top of gp_grad_cases.py and gp_fit_cases.py (imported,
neither modified).

    reference      autograd of gp_grad_cases.dense_bound in X at the case's solved (c, v) (`autograd_input_gradient`)
    decomposition  r_nm = u_nm k_nm as in gp_grad_cases.blocks64 (`weights64`), rho_n = sum_m r_nm,
                   dF/dx_n = (sum_m r_nm zc_m - rho_n xc_n) / l^2 (`input_gradient64`); zc, xc centred at the centroid of Z
    fp32 arm       the same evaluated eagerly in fp32 (`input_gradient32`): centred as the kernel centres, W1, 2 G^ and g
                   rounded from fp64 as gp_grad_cases.blocks32 does, per chunk of rows; `input_gradient32_of_case` runs
                   it at the fp64 adjoints and again with the statistics in fp32 as well (what bound_and_gradient does)
    linear map     embeddings X0 @ W for a fixed W near the identity (`linear_case`): dF/dW by autograd, by the
                   decomposition (X0^T dX) and by the eager fp32 arm (`weight_gradient32`); the re-solved bound of
                   X0 @ (W + t dW) for central differences (`resolved_bound_through`)

k(x, x) = s does not depend on x, so X enters the bound through k_nm alone; with (c, v) at their maximisers the gradient
at fixed (c, v) is the gradient of the re-solved bound (the envelope theorem), which tests/test_gp_input_grad_cpu.py checks
by central differences through the linear map.

Nothing here touches the package under test or the GPU."""
import functools
import math

import torch

import gp_fit_cases as F
import gp_grad_cases as Gc

JITTER = Gc.JITTER
PARITY = Gc.PARITY
NAMES = Gc.NAMES
LINEAR_NAMES = ("n150_m33_d5", "n300_m96_d65", "n31_m30_d7")
f64 = torch.float64

# ---- recorded by tests/test_gp_input_grad_cpu.py (which re-measures them and holds them) --------------------------------
# Worst deviation of the eager fp32 dF/dX from fp64 autograd over the cases, of max |dF/dX|
# (test_fp32_floor_of_the_input_gradient: 1, 2 and 8 threads, chunks of 1024 and 4096 rows, at the case's fp64 adjoints as
# gp_grad_cases.BLOCK_FLOOR is).  Measured 1.09e-5, at n1100_m1024_d384 (the other cases stay at or below 4.1e-6); recorded
# a quarter above that.  Unlike colsum and d2sum this output is no sum over the rows that cancels: the floor lies below a
# quarter of PARITY, so the GPU bound is PARITY (input_bound).  With the statistics in fp32 as well, which is what
# bound_and_gradient does, the same test shows 1.84e-5 at that case and at most 7.1e-6 elsewhere: also below a quarter of
# PARITY.
INPUT_FLOOR = 1.36e-5
# Worst deviation of the eager fp32 dF/dW (embeddings X0 @ W in fp32, statistics, dF/dX and X0^T dX in fp32) from fp64
# autograd over LINEAR_NAMES, of max |dF/dW| (test_fp32_floor_of_the_weight_gradient, same threads and chunks).
# Measured 3.2e-6, 3.4e-6 and 5.44e-6 (n31_m30_d7); recorded a quarter above that.  The GPU test allows four times this
# figure.
WEIGHT_FLOOR = 6.8e-6


def input_bound():
    """The GPU bound of dF/dX, of its max-norm, by the rule of gp_grad_cases.block_bound: the project's PARITY where the
    fp32 floor is at or below a quarter of it, four times the floor otherwise."""
    return PARITY if INPUT_FLOOR <= 0.25 * PARITY else 4.0 * INPUT_FLOOR


def weight_bound():
    """The GPU bound of dF/dW through collapsed_bound, of its max-norm: four times what the eager fp32 arm shows."""
    return 4.0 * WEIGHT_FLOOR


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _logs(s, ell):
    return torch.tensor(math.log(ell), dtype=f64), torch.tensor(math.log(s), dtype=f64)


def autograd_input_gradient(X, y_norm, Z, s, ell, c, v, jitter=JITTER):
    """The reference: d dense_bound / dX [N, D] at fixed (c, v), fp64."""
    Xr = X.to(f64).clone().requires_grad_(True)
    ll, ls = _logs(s, ell)
    Fv = Gc.dense_bound(Xr, y_norm.to(f64), Z.to(f64), ll, ls, c, v, jitter)
    return torch.autograd.grad(Fv, Xr)[0]


def weights64(X, y_norm, Z, s, ell, c, G_hat, g, jitter=JITTER):
    """(R [M, N], Xc [N, D], Zc [M, D]) in fp64: r_nm = u_nm k_nm exactly as gp_grad_cases.blocks64 forms it."""
    X, Z, y = X.to(f64), Z.to(f64), y_norm.to(f64)
    cen = Z.mean(0)
    Xc, Zc = X - cen, Z - cen
    K = s * torch.exp(-0.5 * F._sqdist(Zc, Xc) / ell ** 2)
    L, _ = F.whitener(Z, s, ell, jitter)
    A = torch.linalg.solve_triangular(L, K, upper=False)
    Q = 2.0 * (G_hat @ A) + g[:, None] * (y - c)[None, :]
    return torch.linalg.solve_triangular(L.T, Q, upper=True) * K, Xc, Zc


def input_gradient64(X, y_norm, Z, s, ell, c, G_hat, g, jitter=JITTER):
    """dF/dX [N, D] by the decomposition, fp64."""
    R, Xc, Zc = weights64(X, y_norm, Z, s, ell, c, G_hat, g, jitter)
    return (R.T @ Zc - R.sum(0)[:, None] * Xc) / ell ** 2


def input_gradient32(X, y_norm, Z, s, ell, c, G_hat, g, jitter=JITTER, chunk=4096):
    """What an eager fp32 evaluation of dF/dX gives: centred as the kernel centres, W1, 2 G^ and g from fp64 rounded to
    fp32, the products per chunk of rows in fp32 (gp_grad_cases.blocks32 with one more product).  [N, D] fp32."""
    f32 = torch.float32
    _, W1 = F.whitener(Z, s, ell, jitter)
    cen = Z.to(f64).mean(0)
    Zc, W1, G2, g32 = (Z.to(f64) - cen).to(f32), W1.to(f32), (2.0 * G_hat).to(f32), g.to(f32)
    inv_l2 = torch.tensor(1.0 / ell ** 2, dtype=f32)
    out = []
    for i in range(0, X.shape[0], chunk):
        Xc = X[i:i + chunk].to(f32) - cen.to(f32)
        d2 = F._sqdist(Zc, Xc)
        K = torch.tensor(s, dtype=f32) * torch.exp(-0.5 * d2 / torch.tensor(ell, dtype=f32) ** 2)
        Q = G2 @ (W1 @ K) + g32[:, None] * (y_norm[i:i + chunk].to(f32) - torch.tensor(c, dtype=f32))[None, :]
        R = (W1.T @ Q) * K
        out.append((R.T @ Zc - R.sum(0)[:, None] * Xc) * inv_l2)
    return torch.cat(out)


def _adjoints32(X, y_norm, Z, N, s, ell, chunk):
    """(c, G^, g) as bound_and_gradient finds them: the statistics in fp32, solved and differentiated in fp64."""
    G32 = F.statistics_fp32(X, y_norm.float(), Z, s, ell, chunk=chunk)
    sol = F.solve(G32, N, s)
    adj = Gc.adjoints(G32, N, s, sol["constant"], sol["noise"])
    return sol["constant"], adj["G_hat"], adj["g"]


def input_gradient32_of_case(c, chunk=4096):
    """The two eager fp32 arms of a case: at the case's fp64 adjoints, and with the statistics in fp32 as well."""
    inp, adj = c["inp"], c["adj"]
    at64 = input_gradient32(inp["X"], c["y_norm"], inp["Z"], c["s"], c["ell"], c["c"], adj["G_hat"], adj["g"], chunk=chunk)
    const, G_hat, g = _adjoints32(inp["X"], c["y_norm"], inp["Z"], c["N"], c["s"], c["ell"], chunk)
    at32 = input_gradient32(inp["X"], c["y_norm"], inp["Z"], c["s"], c["ell"], const, G_hat, g, chunk=chunk)
    return at64, at32


def deviation(got, ref):
    """max |got - ref| / max |ref|."""
    return float((got.to(f64) - ref).abs().max()) / float(ref.abs().max())


@functools.lru_cache(maxsize=None)
def case(name):
    """gp_grad_cases.case(name) and, at its solved (c, v): dF/dX by autograd (`ref`) and by the decomposition (`dX`), and
    the data part of dF/dZ from the case's fp64 blocks (`dZ_data`); computed once, shared, never modified."""
    c = Gc.case(name)
    inp, adj = c["inp"], c["adj"]
    ref = autograd_input_gradient(inp["X"], c["y_norm"], inp["Z"], c["s"], c["ell"], c["c"], c["v"])
    dX = input_gradient64(inp["X"], c["y_norm"], inp["Z"], c["s"], c["ell"], c["c"], adj["G_hat"], adj["g"])
    Z = inp["Z"].to(f64)
    blk = c["blocks"]
    dZ_data = (blk["P"] - blk["colsum"][:, None] * (Z - Z.mean(0))) / c["ell"] ** 2
    return dict(c, ref=ref, dX=dX, dZ_data=dZ_data)


# ---- embeddings through a linear map ------------------------------------------------------------------------------------
def linear_weight(D):
    """W [D, D] fp32, fixed: the identity plus 0.1 randn / sqrt(D), so that X0 @ W stays where Z (rows of X0) lies."""
    g = torch.Generator().manual_seed(5000 + D)
    return torch.eye(D) + 0.1 * torch.randn(D, D, generator=g) / math.sqrt(D)


def resolved_bound_through(lc, W64):
    """F* of the embeddings X0 @ W64 (fp64): statistics and solver of gp_fit_cases, c and v searched again."""
    return F.solve(F.statistics(lc["X0"].to(f64) @ W64, lc["y_norm"], lc["Z"], lc["s"], lc["ell"]), lc["N"], lc["s"])["elbo"]


@functools.lru_cache(maxsize=None)
def linear_case(name):
    """The inputs of gp_grad_cases.case(name) with the embeddings X0 @ W: the fp64 fit of those embeddings, dF/dW at its
    (c, v) by autograd of dense_bound(X0 @ W) (`ref`) and as X0^T dX of the decomposition (`dW`)."""
    c = Gc.case(name)
    inp, N, s, ell = c["inp"], c["N"], c["s"], c["ell"]
    X0, Z, y_norm = inp["X"], inp["Z"], c["y_norm"]
    W = linear_weight(c["D"])
    E = X0.to(f64) @ W.to(f64)
    G = F.statistics(E, y_norm, Z, s, ell)
    sol = F.solve(G, N, s)
    const, v = sol["constant"], sol["noise"]
    adj = Gc.adjoints(G, N, s, const, v)
    Wr = W.to(f64).clone().requires_grad_(True)
    ll, ls = _logs(s, ell)
    Fv = Gc.dense_bound(X0.to(f64) @ Wr, y_norm.to(f64), Z.to(f64), ll, ls, const, v)
    ref = torch.autograd.grad(Fv, Wr)[0]
    dW = X0.to(f64).T @ input_gradient64(E, y_norm, Z, s, ell, const, adj["G_hat"], adj["g"])
    return dict(X0=X0, W=W, Z=Z, y_norm=y_norm, N=N, M=c["M"], D=c["D"], s=s, ell=ell, c=const, v=v, elbo=sol["elbo"],
                dense=float(Fv.detach()), ref=ref, dW=dW, chunk_rows=c["chunk_rows"])


def weight_gradient32(lc, chunk=4096):
    """The eager fp32 arm of collapsed_bound(X0 @ W).backward(): the embeddings, the statistics, dF/dX and X0^T dX in
    fp32, the solve and the adjoints in fp64 as the host does.  [D, D] fp32."""
    E32 = lc["X0"] @ lc["W"]
    const, G_hat, g = _adjoints32(E32, lc["y_norm"], lc["Z"], lc["N"], lc["s"], lc["ell"], chunk)
    dX = input_gradient32(E32, lc["y_norm"], lc["Z"], lc["s"], lc["ell"], const, G_hat, g, chunk=chunk)
    return lc["X0"].T @ dX
