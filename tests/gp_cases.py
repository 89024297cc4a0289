"""Shared by tests/test_gp_cpu.py and tests/test_gp_head.py: an fp64 torch restatement of the sparse variational GP's
prediction (reference CGAT/gaussian_process.py:45-66, 247-268) in two forms, and the input builder of the cases.

    k(x, z) = s exp(-|x - z|^2 / (2 l^2)),  L = chol(K_zz + jitter I)
    factor form : mean_f = c + k_x . a,  var_f = s - |W1 k_x|^2 + |W2 k_x|^2,  a = L^-T m, W1 = L^-1, W2 = L_S^T L^-1
    direct form : interp = L^-1 K_zx,  mean_f = c + interp^T m,  var_f = s + diag(interp^T (L_S L_S^T - I) interp)
    pred = mean_f std + mean,  lower / upper = (mean_f -+ 2 sqrt(var_f)) std + mean

Nothing here touches the package under test or the GPU."""
import functools
import math

import torch

JITTER = 1e-4
# (G, M, D) of the parity cases; `wide` doubles the lengthscale, `zero_mean` is the reference's --zero-mean, `ldx_pad`
# gives X a row stride larger than D
CASES = {
    "g257_m37_d5": dict(G=257, M=37, D=5),
    "g33_m1000_d128": dict(G=33, M=1000, D=128),
    "g300_m1024_d384": dict(G=300, M=1024, D=384, ldx_pad=3),
    "g65_m129_d640": dict(G=65, M=129, D=640, wide=True),
    "g1_m1_d1": dict(G=1, M=1, D=1),
    "g64_m64_d16": dict(G=64, M=64, D=16, zero_mean=True),
}


def build_inputs(G, M, D, seed=0, wide=False, zero_mean=False, ldx_pad=0):
    """fp32 tensors (what a user would hand to GPHead) on the CPU."""
    g = torch.Generator().manual_seed(1000 + seed + 7 * G + 13 * M + 17 * D)
    Z = 0.5 + torch.randn(M, D, generator=g)
    X = 0.5 + torch.randn(G, D, generator=g)
    m = torch.randn(M, generator=g)
    LS = 0.6 * torch.eye(M) + 0.3 / math.sqrt(M) * torch.tril(torch.randn(M, M, generator=g))
    ell = (2.0 if wide else 1.0) * math.sqrt(D)
    return dict(inducing_points=Z, variational_mean=m, chol_variational_covar=LS,
                constant=torch.tensor(0.0 if zero_mean else 0.2), outputscale=torch.tensor(1.7),
                lengthscale=torch.tensor(ell), mean=torch.tensor(-0.3), std=torch.tensor(2.5)), X


def _sqdist(X, Z):
    return torch.cdist(X, Z, compute_mode="donot_use_mm_for_euclid_dist") ** 2


def _scalars(p, dtype):
    return tuple(p[k].to(dtype) for k in ("constant", "outputscale", "lengthscale", "mean", "std"))


def _finish(mean_f, var_f, tm, ts):
    sd = var_f.clamp_min(0).sqrt()
    return dict(mean_f=mean_f, var_f=var_f, pred=mean_f * ts + tm, lower=(mean_f - 2 * sd) * ts + tm,
                upper=(mean_f + 2 * sd) * ts + tm)


def _factors64(p, jitter):
    dt = torch.float64
    Z, m, LS = (p[k].to(dt) for k in ("inducing_points", "variational_mean", "chol_variational_covar"))
    c, s, ell, tm, ts = _scalars(p, dt)
    M = Z.shape[0]
    Kzz = s * torch.exp(-0.5 * _sqdist(Z, Z) / ell ** 2) + jitter * torch.eye(M, dtype=dt)
    L = torch.linalg.cholesky(Kzz)
    a = torch.linalg.solve_triangular(L.T, m[:, None], upper=True)[:, 0]
    W1 = torch.linalg.solve_triangular(L, torch.eye(M, dtype=dt), upper=False)
    W2 = LS.tril().T @ W1
    return Kzz, L, a, W1, W2


def factor_form(p, X, jitter=JITTER, dtype=torch.float64):
    """The factor form.  The factors are always computed in fp64; `dtype` is the precision of the evaluation per row
    (torch.float32: what an eager fp32 evaluation of the same factors gives, the floor the tolerance is held against)."""
    _, _, a, W1, W2 = _factors64(p, jitter)
    c, s, ell, tm, ts = _scalars(p, dtype)
    Z, Xd = p["inducing_points"].to(dtype), X.to(dtype)
    if dtype != torch.float64:                       # the fp32 evaluation centres like the kernel does
        cen = p["inducing_points"].to(torch.float64).mean(0)
        Z, Xd = (p["inducing_points"].to(torch.float64) - cen).to(dtype), Xd - cen.to(dtype)
    kx = s * torch.exp(-0.5 * _sqdist(Xd, Z) / ell ** 2)
    mean_f = c + kx @ a.to(dtype)
    var_f = s - (kx @ W1.to(dtype).T).square().sum(1) + (kx @ W2.to(dtype).T).square().sum(1)
    return _finish(mean_f, var_f, tm, ts)


def direct_form(p, X, jitter=JITTER):
    """K_xx + interp^T (S - I) interp, the whitened strategy as gpytorch writes it, in fp64."""
    dt = torch.float64
    _, L, _, _, _ = _factors64(p, jitter)
    c, s, ell, tm, ts = _scalars(p, dt)
    Z, m = p["inducing_points"].to(dt), p["variational_mean"].to(dt)
    LS = p["chol_variational_covar"].to(dt).tril()
    kzx = s * torch.exp(-0.5 * _sqdist(Z, X.to(dt)) / ell ** 2)
    interp = torch.linalg.solve_triangular(L, kzx, upper=False)
    S = LS @ LS.T
    mean_f = c + interp.T @ m
    var_f = s + (interp * ((S - torch.eye(Z.shape[0], dtype=dt)) @ interp)).sum(0)
    return _finish(mean_f, var_f, tm, ts)


@functools.lru_cache(maxsize=None)
def case(name):
    """(params, X, fp64 reference) of a named case; computed once, shared, never modified."""
    kw = dict(CASES[name])
    pad = kw.pop("ldx_pad", 0)
    p, X = build_inputs(**kw)
    ref = factor_form(p, X)
    if pad:
        X = torch.cat([X, torch.full((X.shape[0], pad), 1e30)], dim=1)[:, :X.shape[1]]   # a view with ldx = D + pad
    return p, X, ref


def errors(got, ref, p):
    """The parity figures of the issue: each is (error, bound) with bound = 1e-4 of the named max-norm."""
    c, s = float(p["constant"]), float(p["outputscale"])
    out = {"mean_f": (float((got["mean_f"].double() - ref["mean_f"]).abs().max()),
                      1e-4 * float((ref["mean_f"] - c).abs().max())),
           "var_f": (float((got["var_f"].double() - ref["var_f"]).abs().max()), 1e-4 * s)}
    for k in ("pred", "lower", "upper"):
        if k in got:
            out[k] = (float((got[k].double() - ref[k]).abs().max()), 1e-4 * float(ref[k].abs().max()))
    return out
