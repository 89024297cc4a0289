"""Shared by tests/test_gp_fit_cpu.py and tests/test_gp_fit.py: an fp64 torch restatement of the collapsed sparse-GP fit
(the model of reference CGAT/gaussian_process.py:45-66, its bound at :233, target normalisation :200-204) and
the input builder of the cases.

    k(x, z) = s exp(-|x - z|^2 / (2 l^2)),  L = chol(K_zz + jitter I),  a_n = L^-1 k(Z, x_n),  a~_n = [a_n, y~_n, 1]
    statistics : G = sum_n a~_n a~_n^T
    solver     : Lambda = I + Psi / v,  S = Lambda^-1,  m = S beta / v,  beta = Ay - c A1,  c and v = sigma^2 maximise F
    explicit   : sum_n E_q[log N(y~_n | f_n, v)] - KL(N(m, L_S L_S^T) || N(0, I)),  f_n ~ N(c + a_n.m, s - |a_n|^2 + |L_S^T a_n|^2)

The statistics are compared block by block, each against its own max-norm.  With targets normalised by their own mean the
block sum_n y~_n is zero up to the rounding of that mean, and no fp32 evaluation can meet a relative bound on it; so the
statistics cases take y~ normalised by the mean / std of ALL generated targets (training and held-out rows: `y_stat`),
which leaves sum_n y~_n a statistic like the others.  The fit cases normalise as GPHead.fit does, by the training rows.

Nothing here touches the package under test or the GPU."""
import functools
import math

import torch

import gp_cases

JITTER = gp_cases.JITTER
HELD_OUT = 257
# (N, M, D) of the cases.  `chunk_rows`: what the GPU test passes (None: the default); `ldx_pad`: a row stride D + pad;
# `noise_sd`: standard deviation of the noise added to the targets (0.3 unless stated; the two cases with more of it had
# the most sensitive fitted noise at 0.3, 5.4e-6 to 5.8e-6 in the fp32 floor, which left that test no margin).
CASES = {
    "n70_m1_d1": dict(N=70, M=1, D=1),
    "n150_m33_d5": dict(N=150, M=33, D=5, chunk_rows=64),          # three chunks, the last partial; M + 2 crosses 32
    "n300_m96_d65": dict(N=300, M=96, D=65, ldx_pad=3),
    "n1000_m129_d130": dict(N=1000, M=129, D=130, noise_sd=0.02),   # low noise
    "n1100_m1000_d128": dict(N=1100, M=1000, D=128),
    "n1100_m1024_d384": dict(N=1100, M=1024, D=384, noise_sd=0.6),  # Ma_p = 1056
    "n31_m30_d7": dict(N=31, M=30, D=7, noise_sd=0.45),            # below one tile, M + 2 = 32
}
# Relative deviation of the fitted noise allowed on the GPU: four times the worst deviation of the eager fp32 evaluation
# of the statistics from the fp64 fit over the cases above, which tests/test_gp_fit_cpu.py::test_fp32_floor_of_the_cases
# measures: 4.0e-6 (case n1100_m1000_d128: 3.1e-6 to 4.0e-6 with 1 to 8 threads and 1024- or 4096-row chunks; every
# other case stays at or below 3.4e-6), taken as 5e-6 to leave the fp32 matrix products of another BLAS that spread
# again; the floor test holds the figure at a quarter of this bound.
NOISE_REL_BOUND = 4 * 5e-6
PARITY = 1e-4                                                       # the project's criterion, of each block's max-norm
ELBO_REL_BOUND = 1e-4
LOG_NOISE_BOUNDS = (math.log(1e-8), math.log(1e2))


def build_inputs(N, M, D, seed=0, noise_sd=0.3, **_):
    """fp32 tensors on the CPU: X [N, D], targets y [N] (a smooth function of a random projection plus noise, offset and
    scaled so that the normalisation matters), Z = M distinct rows of X, held-out rows Xt [257, D], s and l."""
    g = torch.Generator().manual_seed(2000 + seed + 7 * N + 13 * M + 17 * D)
    X = 0.5 + torch.randn(N + HELD_OUT, D, generator=g)
    w = torch.randn(D, generator=g) / math.sqrt(D)
    t = (X - 0.5) @ w
    y = 3.0 + 2.0 * (torch.sin(1.3 * t) + 0.5 * t) + 2.0 * noise_sd * torch.randn(N + HELD_OUT, generator=g)
    Z = X[torch.randperm(N, generator=g)[:M]].clone()
    y_all = y.to(torch.float64)
    y_stat = ((y_all - y_all.mean()) / y_all.std())[:N].to(torch.float32)
    return dict(X=X[:N].clone(), y=y[:N].clone(), y_stat=y_stat, Z=Z, Xt=X[N:].clone(), outputscale=1.3,
                lengthscale=math.sqrt(D))


def normalise(y):
    """(y~ in fp64, mean, std); mean and std are torch.mean / torch.std rounded to fp32, as a head stores them."""
    y64 = y.to(torch.float64)
    tm, ts = float(torch.mean(y64).float()), float(torch.std(y64).float())
    return (y64 - tm) / ts, tm, ts


def _sqdist(X, Z):
    return torch.cdist(X, Z, compute_mode="donot_use_mm_for_euclid_dist") ** 2


def whitener(Z, s, ell, jitter=JITTER):
    """L = chol(K_zz + jitter I) and W1 = L^-1, fp64."""
    Z = Z.to(torch.float64)
    M = Z.shape[0]
    L = torch.linalg.cholesky(s * torch.exp(-0.5 * _sqdist(Z, Z) / ell ** 2) + jitter * torch.eye(M, dtype=torch.float64))
    return L, torch.linalg.solve_triangular(L, torch.eye(M, dtype=torch.float64), upper=False)


def whitened_rows(X, Z, s, ell, jitter=JITTER):
    """a_n = L^-1 k(Z, x_n) as the columns of [M, N], fp64 (a triangular solve, not the product with W1)."""
    L, _ = whitener(Z, s, ell, jitter)
    Kzx = s * torch.exp(-0.5 * _sqdist(Z.to(torch.float64), X.to(torch.float64)) / ell ** 2)
    return torch.linalg.solve_triangular(L, Kzx, upper=False)


def statistics(X, y_norm, Z, s, ell, jitter=JITTER):
    """G [M+2, M+2] in fp64."""
    A = whitened_rows(X, Z, s, ell, jitter)
    At = torch.cat([A, y_norm.to(torch.float64)[None, :], torch.ones(1, A.shape[1], dtype=torch.float64)])
    return At @ At.T


def statistics_fp32(X, y_norm, Z, s, ell, jitter=JITTER, chunk=4096):
    """What an eager fp32 evaluation gives: centred as the kernel centres, W1 from fp64 rounded to fp32, the whitened rows
    and their Gram product in fp32 per chunk of rows, the chunks added in fp64."""
    f32 = torch.float32
    _, W1 = whitener(Z, s, ell, jitter)
    cen = Z.to(torch.float64).mean(0)
    Zc, W1 = (Z.to(torch.float64) - cen).to(f32), W1.to(f32)
    M = Z.shape[0]
    G = torch.zeros(M + 2, M + 2, dtype=torch.float64)
    for i in range(0, X.shape[0], chunk):
        Xc = X[i:i + chunk].to(f32) - cen.to(f32)
        K = torch.tensor(s, dtype=f32) * torch.exp(-0.5 * _sqdist(Xc, Zc) / torch.tensor(ell, dtype=f32) ** 2)
        At = torch.cat([W1 @ K.T, y_norm[i:i + chunk].to(f32)[None, :], torch.ones(1, Xc.shape[0], dtype=f32)])
        G += (At @ At.T).to(torch.float64)
    return G


def blocks(G):
    M = G.shape[0] - 2
    return {"Psi": G[:M, :M], "Ay": G[:M, M], "A1": G[:M, M + 1], "yy": G[M, M], "sum_y": G[M, M + 1]}


def collapsed(G, N, s, c, v):
    """F(c, v) by dense algebra on Lambda = I + Psi / v (a Cholesky factorisation), with S and m: fp64."""
    M = G.shape[0] - 2
    b = blocks(G.to(torch.float64))
    Lam = torch.eye(M, dtype=torch.float64) + b["Psi"] / v
    Lc = torch.linalg.cholesky(0.5 * (Lam + Lam.T))
    beta = b["Ay"] - c * b["A1"]
    rr = float(b["yy"]) - 2 * c * float(b["sum_y"]) + c * c * N
    sol = torch.cholesky_solve(beta[:, None], Lc)[:, 0]
    F = (-0.5 * N * math.log(2 * math.pi * v) - float(torch.log(torch.diagonal(Lc)).sum()) - rr / (2 * v)
         + float(beta @ sol) / (2 * v * v) - (N * s - float(torch.trace(b["Psi"]))) / (2 * v))
    S = torch.cholesky_inverse(Lc)
    return F, sol / v, torch.linalg.cholesky(0.5 * (S + S.T))


def solve(G, N, s, noise=None, zero_mean=False):
    """The restated solver: (m, L_S, c, v, F).  The search over v (and c's closed form) runs on the spectrum of Psi; the
    returned F, m and L_S come from `collapsed` at the found (c, v)."""
    G = G.to(torch.float64)
    M = G.shape[0] - 2
    b = blocks(G)
    lam, Q = torch.linalg.eigh(0.5 * (b["Psi"] + b["Psi"].T))
    lam = lam.clamp_min(0)
    by, b1 = Q.T @ b["Ay"], Q.T @ b["A1"]
    yy, sy, tr = float(b["yy"]), float(b["sum_y"]), float(torch.trace(b["Psi"]))

    def const(v):
        if zero_mean:
            return 0.0
        d = 1.0 / (v + lam)                              # Lambda^-1 / v on the spectrum
        return (sy - float((d * b1 * by).sum())) / (N - float((d * b1 * b1).sum()))

    def F(u):
        v = math.exp(u)
        c = const(v)
        beta = by - c * b1
        return (-0.5 * N * math.log(2 * math.pi * v) - 0.5 * float(torch.log1p(lam / v).sum())
                - (yy - 2 * c * sy + c * c * N) / (2 * v) + float((beta * beta / (v + lam)).sum()) / (2 * v)
                - (N * s - tr) / (2 * v))

    if noise is None:
        lo, hi = LOG_NOISE_BOUNDS
        us = torch.linspace(lo, hi, 400, dtype=torch.float64).tolist()
        k = max(range(len(us)), key=lambda i: F(us[i]))
        a, bb = us[max(k - 1, 0)], us[min(k + 1, len(us) - 1)]
        while bb - a > 1e-12:                            # ternary search on the bracket
            u1, u2 = a + (bb - a) / 3, bb - (bb - a) / 3
            if F(u1) < F(u2):
                a = u1
            else:
                bb = u2
        v = math.exp(0.5 * (a + bb))
    else:
        v = float(noise)
    c = const(v)
    Fv, m, LS = collapsed(G, N, s, c, v)
    return dict(variational_mean=m, chol_variational_covar=LS, constant=c, noise=v, elbo=Fv)


def explicit_elbo(A, y_norm, s, m, LS, c, v):
    """The bound as gpytorch states it (total nats), from the whitened rows A [M, N]; differentiable in m, LS, c."""
    M, N = A.shape
    LS = LS.tril()
    mu = c + A.T @ m
    var = s - (A * A).sum(0) + (LS.T @ A).square().sum(0)
    ell = (-0.5 * math.log(2 * math.pi * v) - ((y_norm - mu).square() + var) / (2 * v)).sum()
    kl = 0.5 * (LS.square().sum() + m @ m - M - 2 * torch.log(torch.diagonal(LS)).sum())
    return ell - kl


def head_params(inp, sol, tm, ts, ell=None):
    """The fp64 fit as the mapping gp_cases.direct_form evaluates."""
    t = lambda x: torch.tensor(float(x), dtype=torch.float64)
    return dict(inducing_points=inp["Z"].to(torch.float64), variational_mean=sol["variational_mean"],
                chol_variational_covar=sol["chol_variational_covar"], constant=t(sol["constant"]),
                outputscale=t(inp["outputscale"]), lengthscale=t(inp["lengthscale"] if ell is None else ell),
                mean=t(tm), std=t(ts))


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs, the fp64 statistics of (X, y_stat) (`gram_stat`), and with the targets normalised by the training rows the
    fp64 statistics (`gram`), fit and prediction on the held-out rows; computed once, shared, never modified."""
    kw = CASES[name]
    inp = build_inputs(**kw)
    y_norm, tm, ts = normalise(inp["y"])
    s, ell = inp["outputscale"], inp["lengthscale"]
    G = statistics(inp["X"], y_norm, inp["Z"], s, ell)
    G_stat = G.clone()
    M, ys = kw["M"], inp["y_stat"].to(torch.float64)
    G_stat[:M, M] = G_stat[M, :M] = whitened_rows(inp["X"], inp["Z"], s, ell) @ ys
    G_stat[M, M], G_stat[M, M + 1], G_stat[M + 1, M] = ys @ ys, ys.sum(), ys.sum()
    sol = solve(G, kw["N"], s)
    p = head_params(inp, sol, tm, ts)
    ref = gp_cases.direct_form(p, inp["Xt"])
    return dict(inp=inp, y_norm=y_norm, mean=tm, std=ts, gram=G, gram_stat=G_stat, sol=sol, params=p, ref=ref, N=kw["N"], M=kw["M"],
                D=kw["D"], chunk_rows=kw.get("chunk_rows"), ldx_pad=kw.get("ldx_pad", 0))


GRID_CASE = "n300_m96_d65"


@functools.lru_cache(maxsize=None)
def grid_elbos():
    """{lengthscale: restated bound} of GRID_CASE at l / 2, l, 2 l (targets normalised by the training rows)."""
    c = case(GRID_CASE)
    inp, s = c["inp"], c["inp"]["outputscale"]
    return {f * inp["lengthscale"]: solve(statistics(inp["X"], c["y_norm"], inp["Z"], s, f * inp["lengthscale"]), c["N"],
                                          s)["elbo"] for f in (0.5, 1.0, 2.0)}


def gram_errors(got, ref):
    """(error, bound) per block of the statistics, bound = 1e-4 of the block's max-norm in the restatement."""
    bg, br = blocks(got.to(torch.float64)), blocks(ref)
    return {k: (float((bg[k] - br[k]).abs().max()), PARITY * float(br[k].abs().max())) for k in br}
