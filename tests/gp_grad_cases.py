"""Shared by tests/test_gp_grad_cpu.py and tests/test_gp_grad.py: an fp64 torch restatement of the gradient of the
collapsed sparse-GP bound in (Z, log l, log s), on top of the restatement of the fit in gp_fit_cases.py.

    reference      the dense bound F(Z, log l, log s) at fixed (c, v = sigma^2) under torch autograd (`dense_bound`)
    decomposition  G^ = dF/dPsi, g = dF/dbeta (`adjoints`); per row q_n = 2 G^ a_n + g (y~_n - c), u_n = W1^T q_n,
                   r_nm = u_nm k_nm; the blocks colsum = sum_n r_n, d2sum_m = sum_n r_nm |x_n - z_m|^2,
                   P = sum_n r_n (x_n - centroid)^T (`blocks64`); the part that passes through W1 = chol(K_zz + jitter I)^-1
                   (`host_part`); the three gradients from them (`totals`)
    fp32 arm       the blocks evaluated eagerly in fp32 (`blocks32`): centred as the kernel centres, W1, 2 G^ and g
                   rounded from fp64, summed per chunk of rows into fp64; and the whole evaluation with the statistics in
                   fp32 as well (`gradients32`), the floor of the total gradients

With (c, v) at their maximisers the gradient at fixed (c, v) is the gradient of the re-solved bound (the envelope
theorem), which tests/test_gp_grad_cpu.py checks by central differences.

Nothing here touches the package under test or the GPU."""
import functools
import math

import torch

import gp_fit_cases as F

JITTER = F.JITTER
PARITY = F.PARITY
ELBO_REL_BOUND = F.ELBO_REL_BOUND
NAMES = ("n70_m1_d1", "n150_m33_d5", "n300_m96_d65", "n1000_m129_d130", "n1100_m1024_d384", "n31_m30_d7")
CASES = {name: F.CASES[name] for name in NAMES}
BLOCKS = ("colsum", "d2sum", "P")
GRADS = ("log_lengthscale", "log_outputscale", "inducing_points")

# ---- recorded by tests/test_gp_grad_cpu.py (which re-measures them and holds them) -------------------------------------
# Worst deviation of the eager fp32 blocks from the fp64 blocks over the cases, of each block's max-norm
# (test_fp32_floor_of_the_blocks: 1 to 8 threads, chunks of 1024 and 4096 rows).  Measured 2.4e-4, 6.0e-4 and 1.8e-5, all
# three at n1100_m1024_d384 (the next case stays at 3.1e-5, 5.3e-5 and 5.8e-6): r_nm changes sign over the rows, and u =
# W1^T q carries W1's entries of up to 1 / sqrt(jitter), so colsum and d2sum are sums that cancel.  Recorded a quarter
# above what was measured, for the fp32 matrix products of another BLAS.  colsum and d2sum lie above a quarter of PARITY,
# so their GPU bound is four times these figures; P's is PARITY.
BLOCK_FLOOR = {"colsum": 3.0e-4, "d2sum": 7.5e-4, "P": 2.5e-5}
# Worst deviation of the three total gradients formed from the eager fp32 blocks (the host part added in fp64, where it
# partly cancels the data part; the statistics in fp32 as well, `gradients32`) from autograd in fp64, of each gradient's
# max-norm; test_fp32_floor_of_the_total_gradients.  Measured 3.3e-5 (n31_m30_d7), 7.5e-6 (n31_m30_d7) and 5.4e-5
# (n1100_m1024_d384), recorded a quarter above that.
TOTAL_FLOOR = {"log_lengthscale": 4.2e-5, "log_outputscale": 9.5e-6, "inducing_points": 6.8e-5}


def block_bound(k):
    """The GPU bound of a block, of its max-norm: the project's PARITY where the fp32 floor is at or below a quarter of
    it, four times the floor otherwise."""
    return PARITY if BLOCK_FLOOR[k] <= 0.25 * PARITY else 4.0 * BLOCK_FLOOR[k]


def total_bound(k):
    """The GPU bound of a total gradient, of its max-norm: four times what the eager fp32 arm shows for it."""
    return 4.0 * TOTAL_FLOOR[k]


# ---- the restatement ----------------------------------------------------------------------------------------------------
def _d2(A, B):
    """|a_i - b_j|^2 by expansion, differentiable; the callers centre A and B."""
    return (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * (A @ B.T)


def _factor(Z, log_l, log_s, jitter):
    """Differentiable: centred Z, L = chol(K_zz + jitter I) with the diagonal distances pinned to 0, the centroid."""
    M = Z.shape[0]
    eye = torch.eye(M, dtype=torch.float64)
    cen = Z.detach().mean(0)
    Zc = Z - cen
    Kzz = torch.exp(log_s - 0.5 * _d2(Zc, Zc).clamp_min(0.0) * (1.0 - eye) * torch.exp(-2.0 * log_l))
    return Zc, torch.linalg.cholesky(Kzz + jitter * eye), cen


def dense_bound(X, y_norm, Z, log_l, log_s, c, v, jitter=JITTER):
    """The collapsed bound at fixed (c, v) by dense algebra, fp64, differentiable in (Z, log_l, log_s)."""
    N, M = X.shape[0], Z.shape[0]
    Zc, L, cen = _factor(Z, log_l, log_s, jitter)
    Kzx = torch.exp(log_s - 0.5 * _d2(Zc, X - cen).clamp_min(0.0) * torch.exp(-2.0 * log_l))
    A = torch.linalg.solve_triangular(L, Kzx, upper=False)
    Psi, res = A @ A.T, y_norm - c
    beta = A @ res
    Lc = torch.linalg.cholesky(torch.eye(M, dtype=torch.float64) + Psi / v)
    sol = torch.cholesky_solve(beta[:, None], Lc)[:, 0]
    return (-0.5 * N * math.log(2 * math.pi * v) - torch.log(torch.diagonal(Lc)).sum() - (res @ res) / (2 * v)
            + (beta @ sol) / (2 * v * v) - (N * torch.exp(log_s) - torch.trace(Psi)) / (2 * v))


def autograd_gradients(X, y_norm, Z, s, ell, c, v, jitter=JITTER):
    """The reference: {log_lengthscale, log_outputscale, inducing_points} of dense_bound, and its value."""
    t = lambda x: torch.tensor(float(x), dtype=torch.float64, requires_grad=True)
    Zr, ll, ls = Z.to(torch.float64).clone().requires_grad_(True), t(math.log(ell)), t(math.log(s))
    Fv = dense_bound(X.to(torch.float64), y_norm.to(torch.float64), Zr, ll, ls, c, v, jitter)
    gZ, gl, gs = torch.autograd.grad(Fv, (Zr, ll, ls))
    return dict(log_lengthscale=gl.reshape(1), log_outputscale=gs.reshape(1), inducing_points=gZ), float(Fv.detach())


def adjoints(G, N, s, c, v):
    """From the statistics: G^ = dF/dPsi, g = dF/dbeta, T = 2 G^ Psi + g beta^T (dF/dW1 = T L^T), and dF/dlog s at fixed
    W1 = 2 tr(G^ Psi) + g.beta - N s / (2 v)."""
    b = F.blocks(G.to(torch.float64))
    M = b["Psi"].shape[0]
    eye = torch.eye(M, dtype=torch.float64)
    Li = torch.cholesky_inverse(torch.linalg.cholesky(eye + b["Psi"] / v))
    beta = b["Ay"] - c * b["A1"]
    w = Li @ beta
    G_hat = -Li / (2 * v) - torch.outer(w, w) / (2 * v ** 3) + eye / (2 * v)
    g = w / (v * v)
    GP = G_hat @ b["Psi"]
    return dict(G_hat=G_hat, g=g, T=2 * GP + torch.outer(g, beta), beta=beta,
                log_outputscale=2 * float(torch.trace(GP)) + float(g @ beta) - N * s / (2 * v))


def host_part(Z, s, ell, T, jitter=JITTER):
    """What reaches (Z, log l, log s) through W1 = L^-1: autograd of sum((T L^T) o W1) with T L^T held."""
    t = lambda x: torch.tensor(float(x), dtype=torch.float64, requires_grad=True)
    Zr, ll, ls = Z.to(torch.float64).clone().requires_grad_(True), t(math.log(ell)), t(math.log(s))
    _, L, _ = _factor(Zr, ll, ls, jitter)
    W1 = torch.linalg.solve_triangular(L, torch.eye(Z.shape[0], dtype=torch.float64), upper=False)
    gZ, gl, gs = torch.autograd.grad(((T @ L.detach().T) * W1).sum(), (Zr, ll, ls))
    return dict(log_lengthscale=gl.reshape(1), log_outputscale=gs.reshape(1), inducing_points=gZ)


def blocks64(X, y_norm, Z, s, ell, c, G_hat, g, jitter=JITTER):
    """colsum [M], d2sum [M], P [M, D] in fp64 (triangular solves, exact distances)."""
    X, Z, y = X.to(torch.float64), Z.to(torch.float64), y_norm.to(torch.float64)
    cen = Z.mean(0)
    Xc, Zc = X - cen, Z - cen
    d2 = F._sqdist(Zc, Xc)                                                   # [M, N]
    K = s * torch.exp(-0.5 * d2 / ell ** 2)
    L, _ = F.whitener(Z, s, ell, jitter)
    A = torch.linalg.solve_triangular(L, K, upper=False)
    Q = 2.0 * (G_hat @ A) + g[:, None] * (y - c)[None, :]
    R = torch.linalg.solve_triangular(L.T, Q, upper=True) * K
    return dict(colsum=R.sum(1), d2sum=(R * d2).sum(1), P=R @ Xc)


def blocks32(X, y_norm, Z, s, ell, c, G_hat, g, jitter=JITTER, chunk=4096):
    """What an eager fp32 evaluation of the blocks gives: centred as the kernel centres, W1, 2 G^ and g from fp64 rounded
    to fp32, three products per chunk of rows in fp32, the chunks added in fp64."""
    f32 = torch.float32
    _, W1 = F.whitener(Z, s, ell, jitter)
    cen = Z.to(torch.float64).mean(0)
    Zc, W1, G2, g32 = (Z.to(torch.float64) - cen).to(f32), W1.to(f32), (2.0 * G_hat).to(f32), g.to(f32)
    M, D = Z.shape
    out = dict(colsum=torch.zeros(M, dtype=torch.float64), d2sum=torch.zeros(M, dtype=torch.float64),
               P=torch.zeros(M, D, dtype=torch.float64))
    for i in range(0, X.shape[0], chunk):
        Xc = X[i:i + chunk].to(f32) - cen.to(f32)
        d2 = F._sqdist(Zc, Xc)
        K = torch.tensor(s, dtype=f32) * torch.exp(-0.5 * d2 / torch.tensor(ell, dtype=f32) ** 2)
        Q = G2 @ (W1 @ K) + g32[:, None] * (y_norm[i:i + chunk].to(f32) - torch.tensor(c, dtype=f32))[None, :]
        R = (W1.T @ Q) * K
        out["colsum"] += R.sum(1).to(torch.float64)
        out["d2sum"] += (R * d2).sum(1).to(torch.float64)
        out["P"] += (R @ Xc).to(torch.float64)
    return out


def totals(blk, Z, ell, adj, host):
    """The three gradients from the blocks (any precision, taken to fp64), the adjoints and the host part."""
    Z = Z.to(torch.float64)
    Zc = Z - Z.mean(0)
    b = {k: v.to(torch.float64) for k, v in blk.items()}
    return dict(log_lengthscale=b["d2sum"].sum().reshape(1) / ell ** 2 + host["log_lengthscale"],
                log_outputscale=torch.tensor([adj["log_outputscale"]], dtype=torch.float64) + host["log_outputscale"],
                inducing_points=(b["P"] - b["colsum"][:, None] * Zc) / ell ** 2 + host["inducing_points"])


def gradients32(c, chunk=4096):
    """The eager fp32 arm of bound_and_gradient for a case: the statistics in fp32 (gp_fit_cases.statistics_fp32), solved
    and differentiated in fp64 as the host does, the blocks in fp32 at those adjoints, the host part in fp64."""
    inp, N, s, ell = c["inp"], c["N"], c["s"], c["ell"]
    G32 = F.statistics_fp32(inp["X"], c["y_norm"].float(), inp["Z"], s, ell, chunk=chunk)
    sol = F.solve(G32, N, s)
    adj = adjoints(G32, N, s, sol["constant"], sol["noise"])
    blk = blocks32(inp["X"], c["y_norm"], inp["Z"], s, ell, sol["constant"], adj["G_hat"], adj["g"], chunk=chunk)
    return totals(blk, inp["Z"], ell, adj, host_part(inp["Z"], s, ell, adj["T"]))


def deviations(got, ref):
    """max |got - ref| / max |ref| per key of ref."""
    return {k: float((got[k].to(torch.float64) - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref}


@functools.lru_cache(maxsize=None)
def case(name):
    """gp_fit_cases.case(name) (inputs, targets normalised by the training rows, fp64 statistics and fit) and at its
    solved (c, v): the adjoints, the fp64 blocks, the host part, the decomposed and the autograd gradients; computed once,
    shared, never modified."""
    c = F.case(name)
    inp, sol, N = c["inp"], c["sol"], c["N"]
    s, ell, const, v = inp["outputscale"], inp["lengthscale"], sol["constant"], sol["noise"]
    adj = adjoints(c["gram"], N, s, const, v)
    blk = blocks64(inp["X"], c["y_norm"], inp["Z"], s, ell, const, adj["G_hat"], adj["g"])
    host = host_part(inp["Z"], s, ell, adj["T"])
    ref, Fv = autograd_gradients(inp["X"], c["y_norm"], inp["Z"], s, ell, const, v)
    return dict(fit=c, inp=inp, y_norm=c["y_norm"], N=N, M=c["M"], D=c["D"], s=s, ell=ell, c=const, v=v, adj=adj, blocks=blk,
                host=host, grads=totals(blk, inp["Z"], ell, adj, host), autograd=ref, dense=Fv,
                chunk_rows=c["chunk_rows"], ldx_pad=c["ldx_pad"])


def resolved_bound(inp, y_norm, N, s, ell):
    """F* at (l, s): the statistics and the solver of gp_fit_cases, c and v searched again."""
    return F.solve(F.statistics(inp["X"], y_norm, inp["Z"], s, ell), N, s)["elbo"]


# ---- the case of the optimiser ----------------------------------------------------------------------------------------
FIT_CASE = dict(N=600, M=96, D=5)
FIT_GRID = (0.5, 1.0, 2.0)                    # of sqrt(D); the ascent starts from the last
FIT_START = dict(lengthscale_factor=2.0, outputscale=1.3)
# the box GPHead.fit puts on l and s by default, as factors of the start (cgat_amd.gp.DEFAULT_BOUNDS; the CPU test
# compares the two)
DEFAULT_BOX = dict(lengthscale=(1.0 / 8.0, 8.0), outputscale=(1.0 / 16.0, 16.0))
# Recorded by test_gp_grad_cpu.py::test_lbfgs_on_the_restatement_reaches_an_interior_optimum, which re-derives them:
# the fp64 optimum of the re-solved bound over (log l, log s), and the relative distance in l and in s within which every
# point lies whose bound is within 2 ELBO_REL_BOUND |F*| of the optimum (the GPU test holds the reported bound, itself
# good to ELBO_REL_BOUND, within ELBO_REL_BOUND of F*), from the Hessian H of F* in (log l, log s) at the optimum:
# |dlog| <= sqrt(2 dF [(-H)^-1]_ii).
FIT_OPTIMUM = dict(lengthscale=1.561376, outputscale=0.631114, noise=0.333291, elbo=-649.09034, rel_l=0.01932, rel_s=0.07382)


def build_fit_inputs():
    """gp_fit_cases.build_inputs' recipe with another seed and a target the starting lengthscale cannot follow:
    3 + 2 sin(4 t) + 0.3 randn, no held-out rows in the draw (257 rows for predictions are drawn after everything else)."""
    N, M, D = (FIT_CASE[k] for k in "NMD")
    g = torch.Generator().manual_seed(4000 + 7 * N + 13 * M + 17 * D)
    X = 0.5 + torch.randn(N, D, generator=g)
    w = torch.randn(D, generator=g) / math.sqrt(D)
    t = (X - 0.5) @ w
    y = 3.0 + 2.0 * torch.sin(4.0 * t) + 0.3 * torch.randn(N, generator=g)
    Z = X[torch.randperm(N, generator=g)[:M]].clone()
    Xt = 0.5 + torch.randn(F.HELD_OUT, D, generator=g)
    return dict(X=X, y=y, Z=Z, Xt=Xt, outputscale=FIT_START["outputscale"],
                lengthscale=FIT_START["lengthscale_factor"] * math.sqrt(D))


def resolved_bound_and_gradient(inp, y_norm, N, s, ell):
    """(F*, [dF*/dlog l, dF*/dlog s], solution) of the restatement by the decomposition, fp64."""
    G = F.statistics(inp["X"], y_norm, inp["Z"], s, ell)
    sol = F.solve(G, N, s)
    adj = adjoints(G, N, s, sol["constant"], sol["noise"])
    blk = blocks64(inp["X"], y_norm, inp["Z"], s, ell, sol["constant"], adj["G_hat"], adj["g"])
    tot = totals(blk, inp["Z"], ell, adj, host_part(inp["Z"], s, ell, adj["T"]))
    return sol["elbo"], torch.cat([tot["log_lengthscale"], tot["log_outputscale"]]), sol


@functools.lru_cache(maxsize=None)
def fit_case():
    """The inputs, the restated bounds of the grid, and the fp64 optimum over (log l, log s) found by torch's L-BFGS
    (strong-Wolfe) on the restatement from (2 sqrt(D), 1.3): optimum (l, s, noise, elbo), the number of evaluations, the
    gradient norm at the end and the Hessian of F* in (log l, log s) there (central differences of the gradient)."""
    inp = build_fit_inputs()
    N, D = FIT_CASE["N"], FIT_CASE["D"]
    y_norm, tm, ts = F.normalise(inp["y"])
    grid = {f: resolved_bound(inp, y_norm, N, inp["outputscale"], f * math.sqrt(D)) for f in FIT_GRID}
    theta = torch.tensor([math.log(inp["lengthscale"]), math.log(inp["outputscale"])], dtype=torch.float64, requires_grad=True)
    count = [0]

    def closure():
        count[0] += 1
        ll, ls = theta.detach().tolist()
        Fv, grad, _ = resolved_bound_and_gradient(inp, y_norm, N, math.exp(ls), math.exp(ll))
        theta.grad = -grad
        return torch.tensor(-Fv, dtype=torch.float64)

    opt = torch.optim.LBFGS([theta], max_iter=100, tolerance_grad=1e-6, tolerance_change=1e-12, line_search_fn="strong_wolfe")
    opt.step(closure)
    ll, ls = theta.detach().tolist()
    Fv, grad, sol = resolved_bound_and_gradient(inp, y_norm, N, math.exp(ls), math.exp(ll))
    h, H = 1e-3, torch.zeros(2, 2, dtype=torch.float64)
    for j, (dl, ds) in enumerate(((h, 0.0), (0.0, h))):
        gp = resolved_bound_and_gradient(inp, y_norm, N, math.exp(ls + ds), math.exp(ll + dl))[1]
        gm = resolved_bound_and_gradient(inp, y_norm, N, math.exp(ls - ds), math.exp(ll - dl))[1]
        H[:, j] = (gp - gm) / (2 * h)
    H = 0.5 * (H + H.T)
    cov = torch.linalg.inv(-H)
    dF = 2.0 * ELBO_REL_BOUND * abs(Fv)
    return dict(inp=inp, y_norm=y_norm, mean=tm, std=ts, grid=grid, lengthscale=math.exp(ll), outputscale=math.exp(ls),
                noise=sol["noise"], elbo=Fv, evaluations=count[0], grad_norm=float(grad.norm()), hessian=H,
                rel_l=math.sqrt(2 * dF * float(cov[0, 0])), rel_s=math.sqrt(2 * dF * float(cov[1, 1])))
