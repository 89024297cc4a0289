"""Shared by tests/test_gp_predict_grad_cpu.py and tests/test_gp_predict_grad.py: an fp64 torch restatement of the derivative
of the sparse-GP head's prediction in its input, on top of gp_cases.py (imported, not modified).

    reference      autograd of sum_n gm_n mean_f(x_n) + gv_n var_f(x_n) in X through gp_cases.factor_form and through
                   gp_cases.direct_form (`autograd_gradient`); the two agree to 1e-10 of max |dX|
    decomposition  alpha = W1 k, q = gv 2 (S - I) alpha + gm m, u = W1^T q, r = u o k, rho = sum_m r_m,
                   dL/dx = (sum_m r_m zc_m - rho xc) / l^2 (`gradient64`); zc, xc centred at the centroid of Z
    fp32 arm       the same evaluated eagerly in fp32 (`gradient32`): centred as the kernel centres, W1, 2 (S - I) and m
                   rounded from fp64; without the G2 product where gv is None, as the kernel runs it
    upstreams      seeded gm, gv [G] in three arms (`upstream`): mean only, variance only, both
    linear map     embeddings X0 @ W for a fixed W near the identity (`nlpd_case`, g257_m37_d5): the mean negative log
                   predictive density of seeded targets, d/dW by fp64 autograd and by the eager fp32 arm

var_f is differentiated as s - |W1 k|^2 + |W2 k|^2 without its clamp at 0: no case has a row there (`case` asserts it).

Nothing here touches the package under test or the GPU."""
import functools
import math

import torch

import gp_cases as C

JITTER = C.JITTER
PARITY = 1e-4                      # the project's parity criterion (DESIGN), as gp_cases.errors applies it
NAMES = tuple(C.CASES)
ARMS = ("mean", "variance", "both")
NLPD_NAME = "g257_m37_d5"
NLPD_NOISE = 0.05
f64 = torch.float64

# ---- recorded by tests/test_gp_predict_grad_cpu.py (which re-measures them and holds them) ------------------------------
# Worst deviation of the eager fp32 dL/dX from fp64 autograd over the six cases, of max |dL/dX| of the arm
# (test_fp32_floor_of_the_gradient: 1, 2 and 8 threads).  Measured 3.20e-6 (mean only, g33_m1000_d128), 7.19e-6 (variance
# only, g65_m129_d640) and 3.09e-6 (both, g33_m1000_d128); recorded a quarter above that.  All lie below a quarter of PARITY,
# so the GPU bound of every arm is PARITY (`gradient_bound`).
GRADIENT_FLOOR = {"mean": 4.0e-6, "variance": 9.0e-6, "both": 3.9e-6}
# Worst deviation of the eager fp32 d mean(nlpd) / dW (embeddings X0 @ W, the prediction, its adjoints, dL/dX and X0^T dX in
# fp32) from fp64 autograd, of max |dL/dW| (test_fp32_floor_of_the_nlpd_weight_gradient, same threads).  Measured 8.88e-7;
# recorded a quarter above that.  The GPU test allows four times this figure.
NLPD_WEIGHT_FLOOR = 1.11e-6


def gradient_bound(arm):
    """The GPU bound of dL/dX of an arm, of its max-norm, by the rule of gp_grad_cases.block_bound: the project's PARITY
    where the fp32 floor is at or below a quarter of it, four times the floor otherwise."""
    return PARITY if GRADIENT_FLOOR[arm] <= 0.25 * PARITY else 4.0 * GRADIENT_FLOOR[arm]


def nlpd_weight_bound():
    """The GPU bound of d mean(nlpd) / dW, of its max-norm: four times what the eager fp32 arm shows."""
    return 4.0 * NLPD_WEIGHT_FLOOR


# ---- the restatement ----------------------------------------------------------------------------------------------------
def upstream(name, arm):
    """(gm, gv) [G] fp64 of a case and an arm, seeded; None for the side the arm leaves out."""
    G = C.CASES[name]["G"]
    g = torch.Generator().manual_seed(7000 + 31 * G + len(name))
    gm, gv = torch.randn(G, generator=g, dtype=f64), torch.randn(G, generator=g, dtype=f64)
    return (gm if arm != "variance" else None), (gv if arm != "mean" else None)


def autograd_gradient(form, p, X, gm, gv):
    """d (sum_n gm_n mean_f_n + gv_n var_f_n) / dX [G, D] through `form` (gp_cases.factor_form or direct_form), fp64."""
    Xr = X.to(f64).clone().requires_grad_(True)
    out = form(p, Xr)
    loss = 0.0
    if gm is not None:
        loss = loss + (gm * out["mean_f"]).sum()
    if gv is not None:
        loss = loss + (gv * out["var_f"]).sum()
    return torch.autograd.grad(loss, Xr)[0]


def _operands(p, X, dtype):
    """Zc [M, D], Xc [G, D], W1, G2 = 2 (S - I) [M, M], m [M], s, l: computed in fp64, centred there (Z) or in `dtype` (X, as
    the kernel does), rounded to `dtype`."""
    _, _, _, W1, _ = C._factors64(p, JITTER)
    Z, m = p["inducing_points"].to(f64), p["variational_mean"].to(f64)
    LS = p["chol_variational_covar"].to(f64).tril()
    cen = Z.mean(0)
    G2 = 2.0 * (LS @ LS.T - torch.eye(Z.shape[0], dtype=f64))
    _, s, ell, _, _ = C._scalars(p, dtype)
    return (Z - cen).to(dtype), X.to(dtype) - cen.to(dtype), W1.to(dtype), G2.to(dtype), m.to(dtype), s, ell


def _gradient(p, X, gm, gv, dtype):
    Zc, Xc, W1, G2, m, s, ell = _operands(p, X, dtype)
    K = s * torch.exp(-0.5 * C._sqdist(Xc, Zc) / ell ** 2)              # [G, M]
    Q = 0.0
    if gv is not None:
        Q = gv.to(dtype)[:, None] * ((K @ W1.T) @ G2)                    # G2 is symmetric
    if gm is not None:
        Q = Q + gm.to(dtype)[:, None] * m[None, :]
    R = (Q @ W1) * K
    return (R @ Zc - R.sum(1)[:, None] * Xc) / ell ** 2


def gradient64(p, X, gm, gv):
    """dL/dX [G, D] by the decomposition, fp64."""
    return _gradient(p, X, gm, gv, f64)


def gradient32(p, X, gm, gv):
    """What an eager fp32 evaluation of the decomposition gives.  [G, D] fp32."""
    return _gradient(p, X, gm, gv, torch.float32)


def deviation(got, ref):
    """max |got - ref| / max |ref|."""
    return float((got.to(f64) - ref).abs().max()) / float(ref.abs().max())


@functools.lru_cache(maxsize=None)
def case(name):
    """gp_cases.case(name) as a dict (p, X, forward) and, per arm, the upstreams (gm, gv), dL/dX by autograd through the
    factor form (`ref`) and through the direct form (`direct`) and by the decomposition (`dX`); computed once, shared,
    never modified."""
    p, X, forward = C.case(name)
    assert float(forward["var_f"].min()) > 0.0
    arms = {}
    for arm in ARMS:
        gm, gv = upstream(name, arm)
        arms[arm] = dict(gm=gm, gv=gv, ref=autograd_gradient(C.factor_form, p, X, gm, gv),
                         direct=autograd_gradient(C.direct_form, p, X, gm, gv), dX=gradient64(p, X, gm, gv))
    return dict(p=p, X=X, forward=forward, arms=arms, **{k: C.CASES[name][k] for k in ("G", "M", "D")})


# ---- the predictive density through a linear map ------------------------------------------------------------------------
def linear_weight(D):
    """W [D, D] fp32, fixed: the identity plus 0.1 randn / sqrt(D), so that X0 @ W stays where Z lies."""
    g = torch.Generator().manual_seed(9000 + D)
    return torch.eye(D) + 0.1 * torch.randn(D, D, generator=g) / math.sqrt(D)


def nlpd(mean_f, var_f, y, noise, tm, ts):
    """The negative log density of y under N(mean_f ts + tm, (var_f + noise) ts^2), per row."""
    var = (var_f + noise) * ts * ts
    resid = y - (mean_f * ts + tm)
    return 0.5 * (torch.log(2.0 * math.pi * var) + resid * resid / var)


@functools.lru_cache(maxsize=None)
def nlpd_case():
    """g257_m37_d5 with the embeddings X0 @ W and seeded targets in the targets' units: mean(nlpd) and its derivative in W
    by fp64 autograd through gp_cases.factor_form (`ref`)."""
    p, X0, _ = C.case(NLPD_NAME)
    W = linear_weight(X0.shape[1])
    g = torch.Generator().manual_seed(9100)
    y = float(p["mean"]) + float(p["std"]) * torch.randn(X0.shape[0], generator=g)
    Wr = W.to(f64).clone().requires_grad_(True)
    out = C.factor_form(p, X0.to(f64) @ Wr)
    assert float(out["var_f"].detach().min()) > 0.0
    loss = nlpd(out["mean_f"], out["var_f"], y.to(f64), NLPD_NOISE, p["mean"].to(f64), p["std"].to(f64)).mean()
    return dict(p=p, X0=X0, W=W, y=y, noise=NLPD_NOISE, loss=float(loss.detach()), ref=torch.autograd.grad(loss, Wr)[0])


def nlpd_weight_gradient32(nc):
    """The eager fp32 arm of head.nlpd(X0 @ W, y, noise).mean().backward(): the embeddings, the prediction (the factor form
    in fp32), its adjoints (torch autograd of the density in mean_f and var_f), dL/dX and X0^T dX in fp32.  [D, D] fp32."""
    p, X0 = nc["p"], nc["X0"]
    E = X0 @ nc["W"]
    out = C.factor_form(p, E, dtype=torch.float32)
    mean_f, var_f = out["mean_f"].detach().requires_grad_(True), out["var_f"].detach().requires_grad_(True)
    loss = nlpd(mean_f, var_f, nc["y"], nc["noise"], p["mean"], p["std"]).mean()
    gm, gv = torch.autograd.grad(loss, (mean_f, var_f))
    return X0.T @ gradient32(p, E, gm, gv)
