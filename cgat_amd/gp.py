"""Prediction with uncertainty: a sparse variational Gaussian-process head on graph embeddings.

The reference's screening / active-learning flow continues past the graph embedding: `train-GP`
(CGAT/gaussian_process.py) fits a sparse variational GP on the embeddings and Utilities/gp_predict.py writes, per
candidate, `prediction` and `uncertainty = upper - prediction`.  This module is the prediction side of that GP, fused
into one HIP launch (csrc/gphead.hip), and a fit of the head on the device (`GPHead.fit`; below).
What the reference's AdamW loop learns by stochastic gradient -- the inducing points, the lengthscale, the outputscale --
`GPHead.fit(learn=...)` learns by a quasi-Newton ascent of the collapsed bound with its exact full-batch gradient.

Model (gaussian_process.py:45-66, evaluated at :247-268): ScaleKernel(RBFKernel) with one lengthscale l and outputscale
s, ConstantMean c (0 under --zero-mean), whitened VariationalStrategy with a CholeskyVariationalDistribution (mean m,
lower-triangular factor L_S), targets normalised by the scalars mean / std.  The latent distribution is returned, no
likelihood noise; the confidence region is mean +- 2 stddev.  With k(x, z) = s exp(-|x - z|^2 / (2 l^2)) and
L = chol(K_zz + jitter I):

    mean_f(x) = c + k_x . a                        a  = L^-T m
    var_f(x)  = s - |W1 k_x|^2 + |W2 k_x|^2        W1 = L^-1,   W2 = L_S^T L^-1
    pred  = mean_f std + mean,   lower / upper = (mean_f -+ 2 sqrt(var_f)) std + mean

which is the whitened formula K_xx + interp^T (S - I) interp with interp = L^-1 K_zx, as two sums of squares (the
indefinite form k^T B k loses the variance in fp32 when K_zz is poorly conditioned).

    head = GPHead.from_tensors({...}).to("cuda:0")
    pred, lower, upper = head.predict(embeddings)        # [G] each
    unc = head.uncertainty(embeddings)                   # upper - pred, gp_predict.py:29
    pred, lower, upper = head.predict_batch(model, batch, b_comp)

Fit (gaussian_process.py:59, :233: VariationalELBO under a GaussianLikelihood).  For a Gaussian likelihood the bound has
a closed-form maximiser in (m, L_S) for fixed (Z, l, s, noise sigma^2, c): Titsias' collapsed bound.  With
a_n = W1 k(Z, x_n), y~ = (y - mean) / std and the augmented row a~_n = [a_n, y~_n, 1] the data enter only through

    G = sum_n a~_n a~_n^T  [(M+2) x (M+2)]:   Psi = G[:M,:M],  Ay = G[:M,M],  A1 = G[:M,M+1],  y~.y~,  sum y~,  N

one streaming pass over the embeddings (`fit_statistics`: csrc/gpfit.hip, the whitened rows accumulated, fp32 products,
fp64 sums).  With beta = Ay - c A1, rr = y~.y~ - 2 c sum y~ + c^2 N and Lambda = I + Psi / sigma^2 (`solve_collapsed`,
host fp64):

    S = Lambda^-1,   m = Lambda^-1 beta / sigma^2,   L_S = chol(S)
    F = -N/2 log(2 pi sigma^2) - 1/2 log|Lambda| - rr / (2 sigma^2) + beta^T Lambda^-1 beta / (2 sigma^4)
        - (N s - tr Psi) / (2 sigma^2)

F is the bound sum_n E_q[log N(y~_n | f_n, sigma^2)] - KL(q(v) || N(0, I)) at that (m, L_S), in total nats.  c has a
closed form (F is quadratic in it), sigma^2 is found by a bounded 1-D search, l and s come from a caller's grid by the
larger F, Z is a fixed subset of the training rows (the reference's initialisation, :223-226) or the k-means centres
started from it (`init`, below).  gpytorch's
VariationalELBO is meant to be this bound divided by N (`elbo_per_point`); gpytorch is not installed where this package
is built, so that scaling is unconfirmed, like the default of `jitter`.

    head, report = GPHead.fit(embeddings, targets, inducing_points=1000, lengthscale="median")

Gradient.  With (m, L_S, c, sigma^2) at their maximisers, dF*/d(Z, log l, log s) is the partial derivative at
fixed (c, sigma^2) (the envelope theorem).  With G^ = dF/dPsi = (I - S - m m^T) / (2 sigma^2) and g = dF/dbeta = m / sigma^2
(`collapsed_adjoints`), per row q_n = 2 G^ a_n + g (y~_n - c), u_n = W1^T q_n = dF/dk_n, r_nm = u_nm k_nm, and a second
pass over the embeddings (csrc/gpgrad.hip) returns colsum = sum_n r_n, d2sum_m = sum_n r_nm |x_n - z_m|^2 and
P = sum_n r_n (x_n - centroid)^T in fp64:

    dF/dlog l = sum(d2sum) / l^2 + host      dF/dZ = (P - colsum o Zc) / l^2 + host      dF/dlog s = sum(colsum) - N s / (2 sigma^2) + host

`host` (`whitening_pullback`) is what reaches the parameters through W1 = chol(K_zz + jitter I)^-1: dF/dW1 =
(2 G^ Psi + g beta^T) L^T pulled back by torch autograd on the M x M host graph.  `bound_and_gradient` is the two passes
and the solve; `GPHead.fit(learn=("lengthscale", "outputscale", "inducing_points"))` ascends the bound with it.

Deep-kernel learning.  k(x, x) = s is constant, so the bound depends on the embeddings only through k_nm, and
the r of the second pass gives its derivative in them as well (same envelope argument):

    dF/dx_n = (sum_m r_nm (z_m - centroid) - rho_n (x_n - centroid)) / l^2,    rho_n = sum_m r_nm

one more product per tile of 32 rows in that pass (`cgat_gp_fit_grad_inputs`), [N, D] fp32 that stays on the device:
`bound_and_gradient(..., wrt_embeddings=True)`.  `collapsed_bound` is the bound as a tensor that is differentiable in the
embeddings, `deep_kernel_gradient` the exact full-batch gradient of -F / N in a network's parameters at the memory cost
of one batch.

Where Z starts.  The reference's only choice is that random batch of training rows.  `kmeans_step` is one
Lloyd step on the device (csrc/gpkmeans.hip: the distance tile of the passes above with an argmin, then the R^T X product
of the gradient pass with a one-hot R): assignment, counts, within-cluster sums of squares and sum_{a_n = m} (x_n -
centroid) in fp64.  `kmeans_inducing_points` iterates it from the subset `fit` would draw, moving the centres on the host
in fp64, and `GPHead.fit(init="kmeans")` or `init=("subset", "kmeans")` starts the fit there or from whichever of the two
has the larger bound: k-means is usually the better start, not always.

Differentiable predictions.  `latent`, `predict` and `uncertainty` are differentiable in the embeddings
where autograd records (grad mode on and `embeddings.requires_grad`); the head's own buffers are constants.  With
alpha = W1 k_x and S = L_S L_S^T the latent distribution reads mean_f = c + alpha . m, var_f = s + alpha^T (S - I) alpha, so
for upstream gradients gm = dL/dmean_f and gv = dL/dvar_f per row (`latent_adjoints` reduces those of the five outputs to
these two)

    u = dL/dk = W1^T (gv 2 (S - I) alpha + gm m),   r_m = u_m k_m,   dL/dx = (sum_m r_m (z_m - centroid) - rho (x - centroid)) / l^2

the chain of the bound's gradient without its row sums (`predictive_backward`: cgat_gp_predict_backward, csrc/gpback.hip).
`GPHead.nlpd` is the negative log predictive density of held-out targets on top of `latent`:

    head.nlpd(model(batch, b_comp, return_graph_embedding=True), y, report["noise"]).mean().backward()

Every other output carries no grad, with the exception of `collapsed_bound`; non-GPU and non-fp32 inputs are refused like
everywhere else in the package.
"""
import math

import torch
from torch import nn

from . import _lib
from .ops import _require_gpu, _ptr, _stream

_KEYS = ("inducing_points", "variational_mean", "chol_variational_covar", "constant", "outputscale", "lengthscale",
         "mean", "std")


def _pack_image(P):
    """Packed MFMA-operand image of P [R, Kd] (R % 32 == 0, Kd % 8 == 0), see include/cgat_hip.h:
    img[((c Kd/8 + k8) 64 + lane) 4 + q] = P[32 c + (lane & 31)][8 k8 + 2 q + (lane >> 5)]."""
    R, Kd = P.shape
    return P.view(R // 32, 32, Kd // 8, 4, 2).permute(0, 2, 4, 1, 3).contiguous().view(-1)


def _centred64(Z):
    """In fp64 on the host, from Z [M, D] (fp64, CPU): the centroid of Z, Zc = Z - centroid, |zc|^2."""
    cen = Z.mean(dim=0)
    Zc = Z - cen
    return cen, Zc, (Zc * Zc).sum(dim=1)


def _whitening64(Zc, zn, s, ell, jitter):
    """In fp64 on the host: L = chol(K_zz + jitter I) and W1 = L^-1 (exactly lower triangular)."""
    M = Zc.shape[0]
    d2 = (zn[:, None] + zn[None, :] - 2.0 * (Zc @ Zc.T)).clamp_min(0.0)
    d2.fill_diagonal_(0.0)
    Kzz = s * torch.exp(-0.5 * d2 / (ell * ell))
    L = torch.linalg.cholesky(Kzz + jitter * torch.eye(M, dtype=torch.float64))
    W1 = torch.linalg.solve_triangular(L, torch.eye(M, dtype=torch.float64), upper=False).tril()
    return L, W1


def _tile_operands(cen, Zc, zn, dev):
    """The fp32 operands of phase (a) of both kernels on `dev`: the packed image of Zc [Mp, Dp], the centroid, |zc|^2
    [Mp]; padding is zero."""
    M, D = Zc.shape
    Mp, Dp = (M + 31) // 32 * 32, (D + 63) // 64 * 64
    Zp = torch.zeros(Mp, Dp, dtype=torch.float32)
    Zp[:M, :D] = Zc
    znp = torch.zeros(Mp, dtype=torch.float32)
    znp[:M] = zn
    return dict(zimg=_pack_image(Zp).to(dev), centroid=cen.to(torch.float32).to(dev), znorm=znp.to(dev))


def _transposed_image(Zc, dev):
    """The fp32 factor of gp_input_rows on `dev`: the packed image of Zc^T [Dq, Mp], Dq = D rounded up to 32; padding is
    zero."""
    M, D = Zc.shape
    Mp, Dq = (M + 31) // 32 * 32, (D + 31) // 32 * 32
    Zt = torch.zeros(Dq, Mp, dtype=torch.float32)
    Zt[:D, :M] = Zc.T
    return _pack_image(Zt).to(dev)


def _square_image(P, dev):
    """The packed image of P [M, M] padded with zeros to [Mp, Mp], fp32 on `dev`."""
    M, Mp = P.shape[0], (P.shape[0] + 31) // 32 * 32
    Pp = torch.zeros(Mp, Mp, dtype=torch.float32)
    Pp[:M, :M] = P
    return _pack_image(Pp).to(dev)


def _check_embeddings(what, embeddings, D):
    """[N, D] fp32 on the GPU, unit column stride and a row stride of at least D (copied otherwise)."""
    if not isinstance(embeddings, torch.Tensor) or embeddings.dim() != 2:
        raise ValueError(f"{what}: embeddings must be a [N, D] tensor")
    if embeddings.dtype != torch.float32:
        raise TypeError(f"cgat_amd: expected float32, got {embeddings.dtype}")
    if embeddings.shape[1] != D:
        raise ValueError(f"{what}: embeddings have width {embeddings.shape[1]}, the inducing points {D}")
    _require_gpu(embeddings)
    x = embeddings.detach()
    if x.shape[0] and (x.stride(1) != 1 or x.stride(0) < D):
        x = x.contiguous()
    return x


DEFAULT_CHUNK_ROWS = 32768


class _StatisticsPass:
    """What a cgat_gp_fit_stats call needs and (l, s) do not change: the checked operands, the centred image of Z on the
    device, the workspace, the output.  factor(s, l, jitter) factors K_zz on the host in fp64 and uploads the image of
    W1; calling the object does that and enqueues the pass; a later call overwrites the same `gram`."""

    def __init__(self, what, embeddings, y_norm, inducing_points, chunk_rows, extra_workspace=None):
        Z = torch.as_tensor(inducing_points)
        if Z.dim() != 2 or Z.shape[0] < 1 or Z.shape[1] < 1:
            raise ValueError(f"{what}: inducing_points must be [M, D], got {tuple(Z.shape)}")
        self.M, self.D = Z.shape
        self.chunk = DEFAULT_CHUNK_ROWS if chunk_rows is None else int(chunk_rows)
        if self.chunk < 32 or self.chunk % 32:
            raise ValueError(f"{what}: chunk_rows = {self.chunk} is not a positive multiple of 32")
        self.what = what
        self.x = _check_embeddings(what, embeddings, self.D)
        self.N, dev = self.x.shape[0], self.x.device
        y = torch.as_tensor(y_norm)
        if y.numel() != self.N or self.N < 1:
            raise ValueError(f"{what}: {self.N} rows of embeddings, {y.numel()} targets (at least one row is needed)")
        self.y32 = y.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
        self.set_inducing_points(Z)
        self.gram = torch.empty(self.M + 2, self.M + 2, dtype=torch.float64, device=dev)
        self.ws_bytes = _lib.lib.cgat_gp_fit_stats_workspace_bytes(self.N, self.M, self.D, self.chunk)
        # one workspace serves the passes of a _GradientPass too: they follow each other on one stream
        also = 0 if extra_workspace is None else extra_workspace(self.N, self.M, self.D, self.chunk)
        self.ws = torch.empty(max(self.ws_bytes, also, 16), dtype=torch.uint8, device=dev)

    def set_inducing_points(self, Z):
        """Replaces Z (same shape): its fp64 centred form on the host and the fp32 operands of phase (a) on the device."""
        Z = torch.as_tensor(Z).detach().to("cpu", torch.float64)
        if tuple(Z.shape) != (self.M, self.D):
            raise ValueError(f"{self.what}: inducing_points must stay [{self.M}, {self.D}], got {tuple(Z.shape)}")
        self.Z = Z
        cen, self.Zc, self.zn = _centred64(Z)
        self.ops = _tile_operands(cen, self.Zc, self.zn, self.x.device)
        self.ops["ztimg"] = _transposed_image(self.Zc, self.x.device)
        self.W1 = self.w1img = None                         # of the Z before; factor() sets them

    def image(self, P):
        """The packed image of P [M, M] padded with zeros to [Mp, Mp], fp32 on the device."""
        return _square_image(P, self.x.device)

    _image = image

    def factor(self, outputscale, lengthscale, jitter):
        """W1 = chol(K_zz + jitter I)^-1 for (s, l) in fp64 on the host, as `W1`, and its image on the device, as `w1img`:
        what both passes whiten with until the next call."""
        _, self.W1 = _whitening64(self.Zc, self.zn, float(outputscale), float(lengthscale), float(jitter))
        self.w1img = self.image(self.W1)

    def __call__(self, outputscale, lengthscale, jitter):
        s, ell = float(outputscale), float(lengthscale)
        if not (s > 0.0 and ell > 0.0):
            raise ValueError(f"{self.what}: outputscale and lengthscale must be positive")
        M, x, ops, dev = self.M, self.x, self.ops, self.x.device
        self.factor(s, ell, jitter)
        with torch.cuda.device(dev):
            rc = _lib.lib.cgat_gp_fit_stats(_ptr(x), x.stride(0), _ptr(self.y32), self.N, self.D, _ptr(ops["zimg"]), M,
                                            _ptr(ops["centroid"]), _ptr(ops["znorm"]), _ptr(self.w1img), s,
                                            0.5 / (ell * ell), self.chunk, _ptr(self.gram), _ptr(self.ws), self.ws_bytes,
                                            _stream())
        _lib.check(rc, "cgat_gp_fit_stats")
        return self.gram


def fit_statistics(embeddings, y_norm, inducing_points, outputscale, lengthscale, jitter=1e-4, chunk_rows=None):
    """G = sum_n a~_n a~_n^T, a~_n = [W1 k(Z, x_n), y_norm[n], 1], as an fp64 [M+2, M+2] tensor on the device of
    `embeddings` (one cgat_gp_fit_stats call; layout in include/cgat_hip.h).  `embeddings` [N, D] fp32 on the GPU,
    `y_norm` [N] the normalised targets, `inducing_points` [M, D] (any device; its factors are computed on the host in
    fp64 exactly as GPHead.prepare() does and rounded to fp32).  `chunk_rows`: rows per chunk, a positive multiple of 32
    (default 32768)."""
    return _StatisticsPass("fit_statistics", embeddings, y_norm, inducing_points, chunk_rows)(outputscale, lengthscale,
                                                                                              jitter)


_LOG_NOISE_BOUNDS = (math.log(1e-8), math.log(1e2))     # of sigma^2, in units of the normalised targets' variance


def solve_collapsed(gram, N, outputscale, noise=None, zero_mean=False):
    """The maximiser of the bound from its statistics, on the host in fp64.  `gram` [M+2, M+2] as fit_statistics returns
    it, `N` the number of rows, `outputscale` the s it was computed with.  `noise`: the likelihood's sigma^2 (of the
    normalised targets), or None for a bounded search over log sigma^2 in [1e-8, 1e2] (a grid, then golden section).
    Returns a dict: variational_mean [M], chol_variational_covar [M, M] (lower), constant, noise, elbo (total nats).
    Eigenvalues of Psi are clamped at 0."""
    G = torch.as_tensor(gram).detach().to("cpu", torch.float64)
    if G.dim() != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 3:
        raise ValueError(f"solve_collapsed: gram must be [M+2, M+2], got {tuple(G.shape)}")
    M = G.shape[0] - 2
    N, s = int(N), float(outputscale)
    Psi = 0.5 * (G[:M, :M] + G[:M, :M].T)
    lam, Q = torch.linalg.eigh(Psi)
    lam = lam.clamp_min(0.0)
    by, b1 = Q.T @ G[:M, M], Q.T @ G[:M, M + 1]
    yy, sy, tr = float(G[M, M]), float(G[M, M + 1]), float(torch.trace(Psi))

    def at(v):
        d = v / (v + lam)                                   # eigenvalues of Lambda^-1
        c = 0.0
        if not zero_mean:
            c = (sy - float((d * b1 * by).sum()) / v) / (N - float((d * b1 * b1).sum()) / v)
        beta = by - c * b1
        rr = yy - 2.0 * c * sy + c * c * N
        F = (-0.5 * N * math.log(2.0 * math.pi * v) - 0.5 * float(torch.log1p(lam / v).sum()) - rr / (2.0 * v)
             + float((d * beta * beta).sum()) / (2.0 * v * v) - (N * s - tr) / (2.0 * v))
        return F, c, d, beta

    if noise is None:
        lo, hi = _LOG_NOISE_BOUNDS
        n_grid = 113
        grid = [lo + (hi - lo) * i / (n_grid - 1) for i in range(n_grid)]
        best = max(range(n_grid), key=lambda i: at(math.exp(grid[i]))[0])
        a, b = grid[max(best - 1, 0)], grid[min(best + 1, n_grid - 1)]
        g = (math.sqrt(5.0) - 1.0) / 2.0
        x1, x2 = b - g * (b - a), a + g * (b - a)
        f1, f2 = at(math.exp(x1))[0], at(math.exp(x2))[0]
        while b - a > 1e-12:
            if f1 < f2:
                a, x1, f1 = x1, x2, f2
                x2 = a + g * (b - a)
                f2 = at(math.exp(x2))[0]
            else:
                b, x2, f2 = x2, x1, f1
                x1 = b - g * (b - a)
                f1 = at(math.exp(x1))[0]
        v = math.exp(0.5 * (a + b))
    else:
        if not float(noise) > 0.0:
            raise ValueError("solve_collapsed: noise must be positive")
        v = float(noise)
    F, c, d, beta = at(v)
    S = (Q * d) @ Q.T
    return dict(variational_mean=Q @ (d * beta) / v, chol_variational_covar=torch.linalg.cholesky(0.5 * (S + S.T)),
                constant=c, noise=v, elbo=F)


def collapsed_adjoints(gram, N, outputscale, solution):
    """The adjoints of the statistics at a solution of the collapsed bound, on the host in fp64.  `gram`,
    `N`, `outputscale` as for solve_collapsed, `solution` what it returned for them.  With v = sigma^2,
    beta = Ay - c A1, S = Lambda^-1 = L_S L_S^T and m = S beta / v, returns a dict:

        G_hat            dF/dPsi  = (I - S - m m^T) / (2 v)                            [M, M], symmetric
        g                dF/dbeta = m / v                                              [M]
        dF_dW1           2 G_hat Psi + g beta^T: dF/dW1 = dF_dW1 L^T                   [M, M]
        log_outputscale  2 tr(G_hat Psi) + m.beta / v - N s / (2 v): dF/dlog s at fixed W1 (a float)

    c and sigma^2 are held fixed: at their maximisers that is the total derivative (the envelope theorem).  The
    eigenvalue clamp of solve_collapsed is not differentiated."""
    G = torch.as_tensor(gram).detach().to("cpu", torch.float64)
    if G.dim() != 2 or G.shape[0] != G.shape[1] or G.shape[0] < 3:
        raise ValueError(f"collapsed_adjoints: gram must be [M+2, M+2], got {tuple(G.shape)}")
    M = G.shape[0] - 2
    v, c, s = float(solution["noise"]), float(solution["constant"]), float(outputscale)
    m = solution["variational_mean"].to(torch.float64)
    LS = solution["chol_variational_covar"].to(torch.float64).tril()
    Psi = 0.5 * (G[:M, :M] + G[:M, :M].T)
    beta = G[:M, M] - c * G[:M, M + 1]
    G_hat = (torch.eye(M, dtype=torch.float64) - LS @ LS.T - torch.outer(m, m)) / (2.0 * v)
    G_hat = 0.5 * (G_hat + G_hat.T)
    g = m / v
    GP = G_hat @ Psi
    return dict(G_hat=G_hat, g=g, dF_dW1=2.0 * GP + torch.outer(g, beta),
                log_outputscale=2.0 * float(torch.trace(GP)) + float(m @ beta) / v - int(N) * s / (2.0 * v))


def whitening_pullback(Z, lengthscale, outputscale, jitter, dF_dW1):
    """The part of the gradient that reaches (Z, log l, log s) through W1 = chol(K_zz + jitter I)^-1, on the host in fp64:
    torch autograd through the Cholesky factorisation of the [M, M] matrix that _whitening64 builds (distances of the
    centred Z, the diagonal pinned to 0).  `dF_dW1` as collapsed_adjoints returns it.  Returns a dict: inducing_points
    [M, D], log_lengthscale, log_outputscale."""
    Z = torch.as_tensor(Z).detach().to("cpu", torch.float64).clone().requires_grad_(True)
    T = torch.as_tensor(dF_dW1).detach().to("cpu", torch.float64)
    M = Z.shape[0]
    log_l = torch.tensor(math.log(float(lengthscale)), dtype=torch.float64, requires_grad=True)
    log_s = torch.tensor(math.log(float(outputscale)), dtype=torch.float64, requires_grad=True)
    eye = torch.eye(M, dtype=torch.float64)
    Zc = Z - Z.detach().mean(dim=0)
    zn = (Zc * Zc).sum(dim=1)
    d2 = (zn[:, None] + zn[None, :] - 2.0 * (Zc @ Zc.T)).clamp_min(0.0) * (1.0 - eye)
    Kzz = torch.exp(log_s - 0.5 * d2 * torch.exp(-2.0 * log_l))
    L = torch.linalg.cholesky(Kzz + float(jitter) * eye)
    W1 = torch.linalg.solve_triangular(L, eye, upper=False)
    gZ, gl, gs = torch.autograd.grad(((T @ L.detach().T).tril() * W1).sum(), (Z, log_l, log_s))
    return dict(inducing_points=gZ, log_lengthscale=float(gl), log_outputscale=float(gs))


class _GradientPass:
    """What bound_and_gradient needs and (Z, l, s) do not change: a _StatisticsPass (the checked x, the targets, the one
    workspace both passes use) and the fp64 outputs of cgat_gp_fit_grad.  An optimiser calls it repeatedly, with
    set_inducing_points in between when Z moves."""

    def __init__(self, what, embeddings, y_norm, inducing_points, chunk_rows):
        self.stats = st = _StatisticsPass(what, embeddings, y_norm, inducing_points, chunk_rows,
                                          extra_workspace=_lib.lib.cgat_gp_fit_grad_workspace_bytes)
        dev = st.x.device
        self.ws_bytes = _lib.lib.cgat_gp_fit_grad_workspace_bytes(st.N, st.M, st.D, st.chunk)
        self.colsum = torch.empty(st.M, dtype=torch.float64, device=dev)
        self.d2sum = torch.empty(st.M, dtype=torch.float64, device=dev)
        self.P = torch.empty(st.M, st.D, dtype=torch.float64, device=dev)

    def set_inducing_points(self, Z):
        self.stats.set_inducing_points(Z)

    def sums(self, outputscale, lengthscale, two_G_hat, g, constant, input_grad=False):
        """Enqueues cgat_gp_fit_grad with the W1 of the last stats.factor() (a statistics pass makes one); (colsum, d2sum,
        P).  `input_grad`: cgat_gp_fit_grad_inputs in its place; (colsum, d2sum, P, dX), dX = dF/dX a new contiguous
        [N, D] fp32 tensor on the device."""
        st = self.stats
        if st.W1 is None:
            raise RuntimeError(f"{st.what}: no factorisation of K_zz yet; call stats.factor(outputscale, lengthscale, "
                               "jitter) or the statistics pass before sums()")
        s, ell = float(outputscale), float(lengthscale)
        x, ops, dev = st.x, st.ops, st.x.device
        w1timg = st.image(st.W1.T)
        g2img = st.image(torch.as_tensor(two_G_hat).to("cpu", torch.float64))
        g32 = torch.as_tensor(g).to("cpu", torch.float64).to(torch.float32).to(dev)
        common = (_ptr(x), x.stride(0), _ptr(st.y32), st.N, st.D, _ptr(ops["zimg"]), st.M, _ptr(ops["centroid"]),
                  _ptr(ops["znorm"]), _ptr(st.w1img), _ptr(w1timg), _ptr(g2img), _ptr(g32), float(constant), s,
                  0.5 / (ell * ell), st.chunk, _ptr(self.colsum), _ptr(self.d2sum), _ptr(self.P))
        if not input_grad:
            with torch.cuda.device(dev):
                rc = _lib.lib.cgat_gp_fit_grad(*common, _ptr(st.ws), self.ws_bytes, _stream())
            _lib.check(rc, "cgat_gp_fit_grad")
            return self.colsum, self.d2sum, self.P
        dX = torch.empty(st.N, st.D, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib.cgat_gp_fit_grad_inputs(*common, _ptr(ops["ztimg"]), _ptr(dX), dX.stride(0), _ptr(st.ws),
                                                  self.ws_bytes, _stream())
        _lib.check(rc, "cgat_gp_fit_grad_inputs")
        return self.colsum, self.d2sum, self.P, dX

    def __call__(self, outputscale, lengthscale, jitter, noise=None, zero_mean=False, wrt_embeddings=False):
        st = self.stats
        s, ell = float(outputscale), float(lengthscale)
        gram = st(s, ell, jitter)
        sol = solve_collapsed(gram, st.N, s, noise=noise, zero_mean=zero_mean)
        adj = collapsed_adjoints(gram, st.N, s, sol)
        out = self.sums(s, ell, 2.0 * adj["G_hat"], adj["g"], sol["constant"], input_grad=wrt_embeddings)
        colsum, d2sum, P = (t.cpu() for t in out[:3])
        host = whitening_pullback(st.Z, ell, s, jitter, adj["dF_dW1"])
        l2 = ell * ell
        grads = dict(log_lengthscale=float(d2sum.sum()) / l2 + host["log_lengthscale"],
                     log_outputscale=adj["log_outputscale"] + host["log_outputscale"],
                     inducing_points=(P - colsum[:, None] * st.Zc) / l2 + host["inducing_points"])
        if wrt_embeddings:
            grads["embeddings"] = out[3]
        return sol, grads


def fit_gradient_sums(embeddings, y_norm, inducing_points, outputscale, lengthscale, two_G_hat, g, constant, jitter=1e-4,
                      chunk_rows=None):
    """The three sums of one cgat_gp_fit_grad call (csrc/gpgrad.hip, layout in include/cgat_hip.h) as fp64 tensors on the
    device of `embeddings`: colsum [M], d2sum [M], P [M, D], for the adjoints `two_G_hat` [M, M] (= 2 dF/dPsi), `g` [M]
    and the constant c.  The other arguments as for fit_statistics; W1 is computed as there."""
    p = _GradientPass("fit_gradient_sums", embeddings, y_norm, inducing_points, chunk_rows)
    p.stats.factor(outputscale, lengthscale, jitter)
    return p.sums(outputscale, lengthscale, two_G_hat, g, constant)


def bound_and_gradient(embeddings, y_norm, inducing_points, outputscale, lengthscale, jitter=1e-4, noise=None,
                       zero_mean=False, chunk_rows=None, wrt_embeddings=False):
    """The collapsed bound at its maximiser in (m, L_S, c, sigma^2) and its exact full-batch gradient in the kernel's
    parameters: one statistics pass, one solve, one gradient pass.  Returns (solution, grads): `solution` as
    solve_collapsed returns it, `grads` a dict of fp64 host values: log_lengthscale, log_outputscale (floats) and
    inducing_points [M, D], the derivatives of solution["elbo"] (c and sigma^2 re-solved, or `noise` held).  With
    `wrt_embeddings` it also holds "embeddings": the derivative in the embeddings (Z an independent operand) as a
    contiguous [N, D] fp32 tensor on their device."""
    return _GradientPass("bound_and_gradient", embeddings, y_norm, inducing_points, chunk_rows)(
        outputscale, lengthscale, jitter, noise=noise, zero_mean=zero_mean, wrt_embeddings=wrt_embeddings)


class _BoundOfEmbeddings(torch.autograd.Function):
    """The bound as a function of the embeddings alone: the value and dF/dX of one bound_and_gradient call."""

    @staticmethod
    def forward(ctx, embeddings, elbo, dX):
        ctx.save_for_backward(dX)
        return torch.tensor(elbo, dtype=torch.float64, device=embeddings.device)

    @staticmethod
    def backward(ctx, grad_bound):
        dX, = ctx.saved_tensors
        return dX * grad_bound.to(torch.float32), None, None


def collapsed_bound(embeddings, y_norm, inducing_points, outputscale, lengthscale, jitter=1e-4, noise=None,
                    zero_mean=False, chunk_rows=None):
    """(bound, solution): the collapsed bound of bound_and_gradient as a 0-dim fp64 tensor on the device of `embeddings`,
    equal to solution["elbo"] and differentiable in `embeddings` (its backward is dF/dX of the same evaluation times the
    incoming scalar, in fp32).  The inducing points, the lengthscale and the outputscale are plain values here: their
    gradients are bound_and_gradient's."""
    sol, grads = _GradientPass("collapsed_bound", embeddings, y_norm, inducing_points, chunk_rows)(
        outputscale, lengthscale, jitter, noise=noise, zero_mean=zero_mean, wrt_embeddings=True)
    return _BoundOfEmbeddings.apply(embeddings, float(sol["elbo"]), grads["embeddings"]), sol


def deep_kernel_gradient(model, batches, y_norm, inducing_points, outputscale, lengthscale, jitter=1e-4, noise=None,
                         zero_mean=False, chunk_rows=None):
    """The exact full-batch gradient of the loss -F / N in the parameters of `model` (a CGAtNet), F the collapsed bound
    of the graph embeddings of all `batches`, at the memory cost of one batch.  `batches`: a sequence of
    (batch, b_comp) pairs as the model takes them; `y_norm` [N] the normalised targets in the graphs' order across the
    batches.  Three steps: the embeddings E [N, D] of every batch under eval() and no_grad; one bound_and_gradient(E, ...,
    wrt_embeddings=True); every batch forward again with grad (still eval()) and emb.backward(-dX[rows] / N), which
    accumulates into the parameters' .grad: the caller zeroes them and steps its optimiser.  The training flag is restored.
    Returns a dict: loss (= -elbo / N, a float), solution, grads (of F in Z, log l, log s, from the same evaluation, so
    the head's parameters can move too) and embeddings (E)."""
    # both sweeps read b_comp: a generator is materialised once
    batches = [(b, c if isinstance(c, (tuple, list, torch.Tensor)) else tuple(c)) for b, c in batches]
    if not batches:
        raise ValueError("deep_kernel_gradient: no batches")
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            E = torch.cat([model(b, c, return_graph_embedding=True) for b, c in batches])
        N = E.shape[0]
        sol, grads = bound_and_gradient(E, y_norm, inducing_points, outputscale, lengthscale, jitter=jitter, noise=noise,
                                        zero_mean=zero_mean, chunk_rows=chunk_rows, wrt_embeddings=True)
        seed = grads.pop("embeddings") * (-1.0 / N)
        row = 0
        for b, c in batches:
            emb = model(b, c, return_graph_embedding=True)
            emb.backward(seed[row:row + emb.shape[0]])
            row += emb.shape[0]
    finally:
        model.train(was_training)
    return dict(loss=-sol["elbo"] / N, solution=sol, grads=grads, embeddings=E)


LEARNABLE = ("lengthscale", "outputscale", "inducing_points")
# The box of GPHead.fit(learn=...) on l and on s, as factors of the values the ascent starts from.  On data the kernel
# cannot explain the bound rises all the way to s -> 0, on near-linear targets toward l, s -> infinity, where
# K_zz + jitter I leaves what the fp32 factors of the kernels resolve (W1 reaches 1 / sqrt(jitter)).  A start
# from a grid or the median distance is within a small factor of the optimum; 8 in l and 16 in s keep s / jitter below
# 2e5 for s = 1.
DEFAULT_BOUNDS = dict(lengthscale=(1.0 / 8.0, 8.0), outputscale=(1.0 / 16.0, 16.0))


def _ascend(evaluate, theta0, lo, hi, max_iter):
    """L-BFGS (torch.optim.LBFGS, strong-Wolfe line search) ascent of evaluate(theta) -> (F, dF/dtheta) over the fp64
    vector theta.  The box lo <= theta <= hi (+-inf where there is none) is enforced by composition: the objective is
    F(clamp(theta)), whose gradient is that of F with the clamped coordinates zeroed, so an iterate that leaves the box
    sees a function that is flat in that coordinate and the returned point is its projection.  Returns (theta, steps,
    evaluations): the last accepted iterate, the bound at each accepted iterate (non-decreasing: an L-BFGS step that
    does not raise the bound ends the ascent at the iterate before it), the number of evaluate calls."""
    x = theta0.clone().clamp(lo, hi).requires_grad_(True)
    seen, count = {}, [0]

    def at(t):
        t = t.detach().clamp(lo, hi)
        key = t.numpy().tobytes()
        if key not in seen:
            count[0] += 1
            F, grad = evaluate(t)
            inside = (t > lo) & (t < hi)
            seen[key] = (float(F), torch.where(inside, grad, torch.zeros_like(grad)))
        return seen[key]

    def closure():
        F, grad = at(x)
        x.grad = -grad.clone()
        return torch.tensor(-F, dtype=torch.float64)

    opt = torch.optim.LBFGS([x], lr=1.0, max_iter=1, max_eval=30, history_size=10, tolerance_grad=0.0,
                            tolerance_change=0.0, line_search_fn="strong_wolfe")
    steps = [at(x)[0]]
    for _ in range(int(max_iter)):
        before = x.detach().clone()
        opt.step(closure)
        F, grad = at(x)
        if not F >= steps[-1] or not bool(torch.isfinite(x).all()):
            with torch.no_grad():
                x.copy_(before)
            break
        gain = F - steps[-1]
        steps.append(F)
        if gain <= 1e-9 * abs(F) or float(grad.abs().max()) <= 1e-7 * max(abs(F), 1.0):
            break
    return x.detach().clamp(lo, hi), steps, count[0]


def median_lengthscale(Z):
    """sqrt of the median off-diagonal |z_i - z_j|^2, in fp64 on the host."""
    Z = torch.as_tensor(Z).detach().to("cpu", torch.float64)
    M = Z.shape[0]
    if M < 2:
        raise ValueError('GPHead.fit: lengthscale="median" needs at least two inducing points')
    Zc = Z - Z.mean(dim=0)
    zn = (Zc * Zc).sum(dim=1)
    d2 = (zn[:, None] + zn[None, :] - 2.0 * (Zc @ Zc.T)).clamp_min(0.0)
    i, j = torch.tril_indices(M, M, offset=-1)
    return math.sqrt(float(d2[i, j].median()))


def _subset_rows(x, M, seed):
    """M distinct rows of x [N, D] (device), drawn with a torch.Generator seeded by `seed`, on the host
    (the reference's initialisation, gaussian_process.py:223-226)."""
    perm = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(int(seed)))[:M]
    return x[perm.to(x.device)].to("cpu")


def _width_of(inducing_points, embeddings):
    """D as the caller states it: of a [M, D] start, else of the embeddings (None when neither is a matrix)."""
    if isinstance(inducing_points, torch.Tensor) and inducing_points.dim() == 2:
        return inducing_points.shape[1]
    return embeddings.shape[1] if isinstance(embeddings, torch.Tensor) and embeddings.dim() == 2 else None


class _KMeansPass:
    """What a cgat_gp_kmeans_step call needs and the centres do not change: the checked embeddings and the workspace.
    Calling it with centres [M, D] uploads their operands of phase (a) (_centred64 in fp64 on the host, rounded to fp32:
    _tile_operands) and enqueues one step; the outputs are new tensors."""

    def __init__(self, what, embeddings, M, D, chunk_rows):
        self.what, self.M, self.D = what, int(M), int(D)
        self.chunk = DEFAULT_CHUNK_ROWS if chunk_rows is None else int(chunk_rows)
        if self.chunk < 32 or self.chunk % 32:
            raise ValueError(f"{what}: chunk_rows = {self.chunk} is not a positive multiple of 32")
        self.x = _check_embeddings(what, embeddings, self.D)
        self.N = self.x.shape[0]
        if self.N < 1:
            raise ValueError(f"{what}: at least one row of embeddings is needed")
        self.ws_bytes = _lib.lib.cgat_gp_kmeans_step_workspace_bytes(self.N, self.M, self.D, self.chunk)
        self.ws = torch.empty(max(self.ws_bytes, 16), dtype=torch.uint8, device=self.x.device)

    def __call__(self, centres):
        Z = torch.as_tensor(centres).detach().to("cpu", torch.float64)
        if tuple(Z.shape) != (self.M, self.D):
            raise ValueError(f"{self.what}: centres must be [{self.M}, {self.D}], got {tuple(Z.shape)}")
        x, dev, M, D = self.x, self.x.device, self.M, self.D
        ops = _tile_operands(*_centred64(Z), dev)
        assign = torch.empty(self.N, dtype=torch.int32, device=dev)
        counts = torch.empty(M, dtype=torch.float64, device=dev)
        wss = torch.empty(M, dtype=torch.float64, device=dev)
        sums = torch.empty(M, D, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib.cgat_gp_kmeans_step(_ptr(x), x.stride(0), self.N, D, _ptr(ops["zimg"]), M, _ptr(ops["centroid"]),
                                              _ptr(ops["znorm"]), self.chunk, _ptr(assign), _ptr(counts), _ptr(wss),
                                              _ptr(sums), _ptr(self.ws), self.ws_bytes, _stream())
        _lib.check(rc, "cgat_gp_kmeans_step")
        return dict(assign=assign, counts=counts, wss=wss, sums=sums, centroid=ops["centroid"])


def _centres_of(what, centres):
    Z = torch.as_tensor(centres)
    if Z.dim() != 2 or Z.shape[0] < 1 or Z.shape[1] < 1:
        raise ValueError(f"{what}: the centres must be [M, D], got {tuple(Z.shape)}")
    return Z


def kmeans_step(embeddings, centres, chunk_rows=None):
    """One Lloyd step (one cgat_gp_kmeans_step call, csrc/gpkmeans.hip) of `embeddings` [N, D] (fp32, GPU)
    against `centres` [M, D] (any device, M <= 1024).  Returns a dict of tensors on the device of the embeddings:

        assign [N] int32    the nearest centre of each row, a tie to the smaller index
        counts [M] fp64     rows per centre (exact integers)
        wss [M] fp64        per centre, the sum of its rows' squared distances to it; wss.sum() is the inertia
        sums [M, D] fp64    per centre, the sum of (x_n - centroid) over its rows
        centroid [D] fp32   the mean of the centres the kernel centred with: the next centre m is
                            centroid + sums[m] / counts[m] where counts[m] > 0

    `chunk_rows` as for fit_statistics."""
    Z = _centres_of("kmeans_step", centres)
    return _KMeansPass("kmeans_step", embeddings, Z.shape[0], Z.shape[1], chunk_rows)(Z)


def kmeans_inducing_points(embeddings, inducing_points, iters=10, seed=0, chunk_rows=None):
    """Inducing points for GPHead.fit by Lloyd's k-means on `embeddings` [N, D] (fp32, GPU); returns (Z, report), Z
    [M, D] fp32 on the host.

    inducing_points   an int M: the start is the subset GPHead.fit draws for the same `seed` (so iters=0 returns exactly
                      that subset); or a start [M, D].  M <= 1024.
    iters             at most that many steps.  A step is one kmeans_step at the current Z, then, on the host in fp64,
                      Z_m <- centroid + sums_m / counts_m (a centre without rows stays where it is), rounded to fp32.
                      When a step finds the assignment of the step before it, the iteration has converged and stops
                      without that (repeated) update.

    report: iterations (updates of Z made), converged, inertia (sum_n min_m |x_n - z_m|^2 of every assignment
    evaluated, i.e. at the Z each step started from) and empty (per update, the number of centres without rows).
    Per step one upload of the centres' image and one read-back of (sums, counts, wss)."""
    what = "kmeans_inducing_points"
    iters = int(iters)
    if iters < 0:
        raise ValueError(f"{what}: iters = {iters} is negative")
    x = _check_embeddings(what, embeddings, _width_of(inducing_points, embeddings))
    if isinstance(inducing_points, torch.Tensor):
        Z = _centres_of(what, inducing_points).detach().to("cpu", torch.float32)
    else:
        M = int(inducing_points)
        if not 1 <= M <= x.shape[0]:
            raise ValueError(f"{what}: {M} inducing points from {x.shape[0]} rows")
        Z = _subset_rows(x, M, seed)
    report = dict(iterations=0, converged=False, inertia=[], empty=[])
    if iters == 0:
        return Z, report
    step = _KMeansPass(what, x, Z.shape[0], Z.shape[1], chunk_rows)
    before = None
    for _ in range(iters):
        out = step(Z)
        M, D = Z.shape
        back = torch.cat([out["sums"].reshape(-1), out["counts"], out["wss"]]).cpu()      # the one read-back
        sums, counts, wss = back[:M * D].reshape(M, D), back[M * D:M * D + M], back[M * D + M:]
        report["inertia"].append(float(wss.sum()))
        if before is not None and torch.equal(out["assign"], before):
            report["converged"] = True
            break
        before = out["assign"]
        filled = counts > 0
        centroid = _centred64(Z.to(torch.float64))[0].to(torch.float32)         # what the step centred with, out["centroid"]
        moved = centroid.to(torch.float64) + sums / counts.clamp_min(1.0)[:, None]
        Z = torch.where(filled[:, None], moved, Z.to(torch.float64)).to(torch.float32)
        report["empty"].append(int((~filled).sum()))
        report["iterations"] += 1
    return Z, report


INITS = ("subset", "kmeans")


class GPHead(nn.Module):
    """Sparse variational GP head.  Buffers (what each corresponds to in the reference's GLightningModel; no gpytorch
    checkpoint key names are claimed):

        inducing_points [M, D]          model.variational_strategy.inducing_points
        variational_mean [M]            the CholeskyVariationalDistribution's variational_mean
        chol_variational_covar [M, M]   its chol_variational_covar (the lower triangle is used)
        constant                        mean_module's constant (0 for ZeroMean)
        outputscale, lengthscale        covar_module's outputscale and its base kernel's single lengthscale (the
                                        constrained values, not the raw parameters)
        mean, std                       the target normalisation scalars of the LightningModule

    `jitter` is what is added to the diagonal of K_zz before its Cholesky factorisation.  The default 1e-4 is meant to
    be gpytorch's float32 default; gpytorch is not installed where this package is built, so that value could not be
    confirmed against it -- pass the value of your gpytorch version if it differs.
    """

    def __init__(self, inducing_points, variational_mean, chol_variational_covar, constant=0.0, outputscale=1.0,
                 lengthscale=1.0, mean=0.0, std=1.0, jitter=1e-4):
        super().__init__()
        Z = torch.as_tensor(inducing_points, dtype=torch.float32)
        m = torch.as_tensor(variational_mean, dtype=torch.float32).reshape(-1)
        LS = torch.as_tensor(chol_variational_covar, dtype=torch.float32)
        if Z.dim() != 2 or Z.shape[0] < 1 or Z.shape[1] < 1:
            raise ValueError(f"GPHead: inducing_points must be [M, D], got {tuple(Z.shape)}")
        M = Z.shape[0]
        if m.shape[0] != M or tuple(LS.shape) != (M, M):
            raise ValueError(f"GPHead: variational_mean must be [{M}] and chol_variational_covar [{M}, {M}], got "
                             f"{tuple(m.shape)} and {tuple(LS.shape)}")
        self.register_buffer("inducing_points", Z.clone())
        self.register_buffer("variational_mean", m.clone())
        self.register_buffer("chol_variational_covar", LS.clone())
        dev = Z.device
        for name, v in (("constant", constant), ("outputscale", outputscale), ("lengthscale", lengthscale),
                        ("mean", mean), ("std", std)):
            t = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
            if t.numel() != 1:
                raise ValueError(f"GPHead: {name} must be a scalar (one lengthscale, no ARD)")
            self.register_buffer(name, t.reshape(()).to(dev).clone())
        self.jitter = float(jitter)
        self._image = None
        self._image_key = None
        self._backward_image = None                         # of prepare_backward(), under the same key
        self._backward_key = None

    @classmethod
    def from_tensors(cls, mapping, jitter=1e-4):
        """From a plain dict with exactly the keys of the buffers above."""
        if set(mapping) != set(_KEYS):
            raise KeyError(f"GPHead.from_tensors: expected exactly the keys {sorted(_KEYS)}, got {sorted(mapping)}")
        return cls(*(mapping[k] for k in _KEYS), jitter=jitter)

    @classmethod
    def fit(cls, embeddings, targets, inducing_points=1000, lengthscale="median", outputscale=1.0, zero_mean=False,
            noise=None, jitter=1e-4, seed=0, chunk_rows=None, learn=(), max_iter=50, bounds=None, init=None,
            kmeans_iters=10):
        """Fits a head to `embeddings` [N, D] (fp32, GPU) and `targets` [N] at the optimum of the collapsed bound (module
        docstring); returns (head, report), the head on the device of the embeddings.

        inducing_points   an int M: that many distinct training rows, drawn with a torch.Generator seeded by `seed`
                          (the reference's initialisation, gaussian_process.py:223-226); or a [M, D] tensor.  M <= 1024.
        init              where an int M starts from (a [M, D] tensor is used as it is and reported as "given"):
                          "subset", those rows; "kmeans",
                          kmeans_inducing_points(embeddings, M, iters=kmeans_iters, seed=seed) from those rows
                          (DESIGN 10f); or a sequence of these: the (lengthscale, outputscale) grid then runs once per
                          start, "median" taken from each start's own Z, and the start of the largest bound wins
                          (k-means is usually the better start, not always).  None (the default) is "subset" with the
                          report as it was before there was a choice.  Otherwise every row of `candidates` gains the key
                          `init` and the report `init` (the winning start) and `kmeans` (the report of
                          kmeans_inducing_points, None where "kmeans" was not tried).  `learn` ascends from the winner.
        lengthscale,      a float or a sequence of floats each; a sequence runs one pass over the data per
        outputscale       (lengthscale, outputscale) pair and keeps the pair with the largest bound.  "median": the
                          square root of the median off-diagonal |z_i - z_j|^2.
        zero_mean         the reference's --zero-mean: constant = 0.  Otherwise the constant's closed form.
        noise             the likelihood's sigma^2 in units of the normalised targets, or None to search it.
        mean, std         torch.mean / torch.std of the targets (gaussian_process.py:200-204), hence N >= 2.

        report: noise, elbo (total nats), elbo_per_point (= elbo / N), lengthscale, outputscale, constant, and
        `candidates`, a list of dicts (lengthscale, outputscale, noise, constant, elbo), one per pair tried.

        learn             a subset of ("lengthscale", "outputscale", "inducing_points"); () (the default) stops at the
                          grid's best pair.  Otherwise the bound, re-solved in (m, L_S, c, sigma^2) at every point, is
                          ascended from that pair over (log l, log s, Z) by L-BFGS with a strong-Wolfe line search on
                          the host in fp64 with the exact full-batch gradient (bound_and_gradient: two passes over the
                          data per evaluation), at most `max_iter` iterations.
        bounds            {"lengthscale": (low, high), "outputscale": (low, high)}: the box of the ascent as factors of
                          the values it starts from, default DEFAULT_BOUNDS = (1/8, 8) and (1/16, 16).  The ascent
                          maximises the bound of the parameters projected onto the box.
        With `learn` the report gains: learned, steps (the bound at each accepted iterate, non-decreasing, steps[0] the
        grid's best), evaluations (of bound_and_gradient) and active_bounds (e.g. ["outputscale:lower"]; empty when the
        optimum is interior).  elbo, noise and constant are those of the returned head (Z rounded to fp32)."""
        Zin = inducing_points
        inits = ("subset",) if init is None else (init,) if isinstance(init, str) else tuple(init)
        if not inits or len(set(inits)) != len(inits) or not set(inits) <= set(INITS):
            raise ValueError(f"GPHead.fit: init must be one of {INITS} or a sequence of them, got {init!r}")
        if int(kmeans_iters) < 0:
            raise ValueError(f"GPHead.fit: kmeans_iters = {kmeans_iters} is negative")
        x = _check_embeddings("GPHead.fit", embeddings, _width_of(Zin, embeddings))
        N, dev = x.shape[0], x.device
        y = torch.as_tensor(targets).detach().reshape(-1)
        if y.numel() != N:
            raise ValueError(f"GPHead.fit: {N} rows of embeddings, {y.numel()} targets")
        if N < 2:
            raise ValueError("GPHead.fit: at least two rows are needed (the targets' standard deviation)")
        y64 = y.to("cpu", torch.float64)
        tm, ts = float(torch.mean(y64).float()), float(torch.std(y64).float())     # as the head stores them: fp32
        if not ts > 0.0:
            raise ValueError("GPHead.fit: the targets are constant")
        y_norm = ((y64 - tm) / ts).to(torch.float32).to(dev)
        kmeans_report = None
        if isinstance(Zin, torch.Tensor):
            starts = [("given", Zin.detach().to("cpu", torch.float32))]
        else:
            M = int(Zin)
            if not 1 <= M <= N:
                raise ValueError(f"GPHead.fit: {M} inducing points from {N} rows")
            starts = []
            for name in inits:
                if name == "kmeans":
                    Zk, kmeans_report = kmeans_inducing_points(x, M, iters=kmeans_iters, seed=seed, chunk_rows=chunk_rows)
                    starts.append((name, Zk))
                else:
                    starts.append((name, _subset_rows(x, M, seed)))
        as_list = lambda v: [float(t) for t in torch.as_tensor(v, dtype=torch.float64).reshape(-1)]
        learn = (learn,) if isinstance(learn, str) else tuple(learn)
        if len(set(learn)) != len(learn) or not set(learn) <= set(LEARNABLE):
            raise ValueError(f"GPHead.fit: learn must be a subset of {LEARNABLE}, got {learn}")
        box = dict(DEFAULT_BOUNDS)
        if bounds is not None:
            if not set(bounds) <= set(box):
                raise ValueError(f"GPHead.fit: bounds has the keys {sorted(box)}, got {sorted(bounds)}")
            box.update({k: (float(lo), float(hi)) for k, (lo, hi) in bounds.items()})
        if any(not 0.0 < lo <= 1.0 <= hi < math.inf for lo, hi in box.values()):
            raise ValueError("GPHead.fit: bounds are pairs of factors (low, high) with 0 < low <= 1 <= high < inf")
        # the workspace: once; Z's image: once per start
        Z = starts[0][1]
        gradient_pass = _GradientPass("GPHead.fit", x, y_norm, Z, chunk_rows) if learn else None
        data_pass = gradient_pass.stats if learn else _StatisticsPass("GPHead.fit", x, y_norm, Z, chunk_rows)
        candidates, best = [], None
        for name, Zs in starts:
            if Zs is not Z:
                data_pass.set_inducing_points(Zs)
            ells = ([median_lengthscale(Zs)] if isinstance(lengthscale, str) and lengthscale == "median"
                    else as_list(lengthscale))
            for ell in ells:
                for s in as_list(outputscale):
                    sol = solve_collapsed(data_pass(s, ell, jitter), N, s, noise=noise, zero_mean=zero_mean)
                    candidates.append(dict(lengthscale=ell, outputscale=s, noise=sol["noise"], constant=sol["constant"],
                                           elbo=sol["elbo"], **({} if init is None else {"init": name})))
                    if best is None or sol["elbo"] > best[1]["elbo"]:
                        best = (candidates[-1], sol, name, Zs)
        row, sol, start, Z = best
        learned = {} if init is None else dict(init=start, kmeans=kmeans_report)
        if learn:
            if Z is not starts[-1][1]:
                gradient_pass.set_inducing_points(Z)            # the ascent starts from the winner's Z
            row, sol, Z, ascent = cls._learn(gradient_pass, row, Z, learn, box, int(max_iter), jitter, noise, zero_mean)
            learned.update(ascent)
        head = cls(Z, sol["variational_mean"], sol["chol_variational_covar"], constant=sol["constant"],
                   outputscale=row["outputscale"], lengthscale=row["lengthscale"], mean=tm, std=ts, jitter=jitter).to(dev)
        report = dict(noise=sol["noise"], elbo=sol["elbo"], elbo_per_point=sol["elbo"] / N, constant=sol["constant"],
                      lengthscale=row["lengthscale"], outputscale=row["outputscale"], candidates=candidates, **learned)
        return head, report

    @staticmethod
    def _learn(gradient_pass, start, Z, learn, box, max_iter, jitter, noise, zero_mean):
        """The ascent of fit(learn=...) from the grid's best candidate `start`: theta = (log l, log s, Z) restricted to
        what `learn` names, in fp64 on the host; one evaluation is bound_and_gradient's two device passes.  Returns the
        final (row, solution, Z) and the report's extra entries."""
        l0, s0 = start["lengthscale"], start["outputscale"]
        Z0 = Z.to(torch.float64)
        M, D = Z0.shape
        parts, lo, hi = [], [], []
        for name, v0 in (("lengthscale", l0), ("outputscale", s0)):
            if name in learn:
                parts.append(torch.tensor([math.log(v0)], dtype=torch.float64))
                lo.append(torch.tensor([math.log(v0 * box[name][0])], dtype=torch.float64))
                hi.append(torch.tensor([math.log(v0 * box[name][1])], dtype=torch.float64))
        if "inducing_points" in learn:
            parts.append(Z0.reshape(-1))
            lo.append(torch.full((M * D,), -math.inf, dtype=torch.float64))
            hi.append(torch.full((M * D,), math.inf, dtype=torch.float64))
        lo, hi = torch.cat(lo), torch.cat(hi)

        def split(theta):
            i, ell, s, Zt = 0, l0, s0, Z0
            if "lengthscale" in learn:
                ell, i = math.exp(float(theta[i])), i + 1
            if "outputscale" in learn:
                s, i = math.exp(float(theta[i])), i + 1
            if "inducing_points" in learn:
                Zt = theta[i:].reshape(M, D)
            return ell, s, Zt

        def run(theta):
            ell, s, Zt = split(theta)
            if "inducing_points" in learn:
                gradient_pass.set_inducing_points(Zt)
            return (ell, s, Zt) + gradient_pass(s, ell, jitter, noise=noise, zero_mean=zero_mean)

        def evaluate(theta):
            _, _, _, sol, grads = run(theta)
            g = [torch.tensor([grads["log_" + k]], dtype=torch.float64) for k in ("lengthscale", "outputscale") if k in learn]
            if "inducing_points" in learn:
                g.append(grads["inducing_points"].reshape(-1))
            return sol["elbo"], torch.cat(g)

        theta, steps, evaluations = _ascend(evaluate, torch.cat(parts), lo, hi, max_iter)
        # the head holds Z in fp32: the final statistics pass and solve are made at the rounded Z
        ell, s, Zt = split(theta)
        Zt = Zt.to(torch.float32)
        gradient_pass.set_inducing_points(Zt)
        sol = solve_collapsed(gradient_pass.stats(s, ell, jitter), gradient_pass.stats.N, s, noise=noise, zero_mean=zero_mean)
        active = []
        for i, name in enumerate(k for k in ("lengthscale", "outputscale") if k in learn):
            active += [f"{name}:{side}" for side, edge in (("lower", lo[i]), ("upper", hi[i])) if float(theta[i]) == float(edge)]
        row = dict(lengthscale=ell, outputscale=s, noise=sol["noise"], constant=sol["constant"], elbo=sol["elbo"])
        return row, sol, Zt, dict(learned=tuple(learn), steps=steps, evaluations=evaluations, active_bounds=active)

    # --------------------------------------------------------------------------------------------------------------
    def _key(self):
        return (self.jitter,) + tuple((t.data_ptr(), t._version, t.device) for t in (getattr(self, k) for k in _KEYS))

    def _factors64(self):
        """c, s, l, mean, std as Python floats and, in fp64 on the host: the centroid of Z, Zc = Z - centroid, |zc|^2,
        a = L^-T m, W1 = L^-1 (exactly lower triangular), W2 = L_S^T L^-1, m and L_S (its lower triangle)."""
        Z = self.inducing_points.detach().to("cpu", torch.float64)
        m = self.variational_mean.detach().to("cpu", torch.float64)
        LS = self.chol_variational_covar.detach().to("cpu", torch.float64).tril()
        c, s, ell, tm, ts = (float(getattr(self, k)) for k in ("constant", "outputscale", "lengthscale", "mean", "std"))
        if not (s > 0.0 and ell > 0.0):
            raise ValueError("GPHead: outputscale and lengthscale must be positive")
        cen, Zc, zn = _centred64(Z)
        L, W1 = _whitening64(Zc, zn, s, ell, self.jitter)
        a = torch.linalg.solve_triangular(L.T, m[:, None], upper=True)[:, 0]
        return dict(c=c, s=s, inv_two_l2=0.5 / (ell * ell), mean=tm, std=ts, centroid=cen, Zc=Zc, znorm=zn, a=a, W1=W1,
                    W2=LS.T @ W1, m=m, LS=LS)

    def prepare(self):
        """Builds the fp32 factor image the kernel reads -- a, W1, W2, |z|^2 and the centroid of Z, computed once in
        fp64 with torch.linalg on the host and rounded to fp32 -- on the device of the buffers.  Called lazily by the
        first prediction and again after any buffer changed (in place or by .to())."""
        key = self._key()
        if self._image is not None and self._image_key == key:
            return self._image
        dev = self.inducing_points.device
        f = self._factors64()
        M, D = f["Zc"].shape
        Mp = (M + 31) // 32 * 32
        F = torch.zeros(2 * Mp, Mp, dtype=torch.float32)
        F[:M, :M] = f["W1"]
        F[Mp:Mp + M, :M] = f["W2"]
        factors = torch.zeros(Mp + 2 * Mp * Mp, dtype=torch.float32)
        factors[:M] = f["a"]
        factors[Mp:] = _pack_image(F)
        self._image = dict(M=M, D=D, c=f["c"], s=f["s"], inv_two_l2=f["inv_two_l2"], mean=f["mean"], std=f["std"],
                           factors=factors.to(dev), **_tile_operands(f["centroid"], f["Zc"], f["znorm"], dev))
        self._image_key = key
        return self._image

    def prepare_backward(self):
        """The fp32 images the backward of a prediction reads beside those of prepare(): W1, W1^T,
        G2 = 2 (L_S L_S^T - I), m and Zc^T, from the same fp64 host factors.  Built by the first backward and again after
        any buffer changed: a forward-only user never pays for them."""
        key = self._key()
        if self._backward_image is not None and self._backward_key == key:
            return self._backward_image
        dev = self.inducing_points.device
        f = self._factors64()
        M = f["Zc"].shape[0]
        G2 = 2.0 * (f["LS"] @ f["LS"].T - torch.eye(M, dtype=torch.float64))
        self._backward_image = dict(w1img=_square_image(f["W1"], dev), w1timg=_square_image(f["W1"].T, dev),
                                    g2img=_square_image(G2, dev), m=f["m"].to(torch.float32).to(dev),
                                    ztimg=_transposed_image(f["Zc"], dev))
        self._backward_key = key
        return self._backward_image

    # --------------------------------------------------------------------------------------------------------------
    def _run(self, embeddings, with_region):
        """The outputs of one cgat_gp_predict call: (mean_f, var_f) or all five.  Where autograd records (grad mode on and
        embeddings.requires_grad) they are differentiable in the embeddings (_Prediction); otherwise plain tensors."""
        if isinstance(embeddings, torch.Tensor) and embeddings.requires_grad and torch.is_grad_enabled():
            return list(_Prediction.apply(self, embeddings, with_region))
        return self._predict(embeddings, with_region)

    def _predict(self, embeddings, with_region):
        if not isinstance(embeddings, torch.Tensor) or embeddings.dim() != 2:
            raise ValueError("GPHead: embeddings must be a [G, D] tensor")
        _require_gpu(embeddings, self.inducing_points)
        if embeddings.dtype != torch.float32:
            raise TypeError(f"cgat_amd: expected float32, got {embeddings.dtype}")
        if embeddings.device != self.inducing_points.device:
            raise ValueError("GPHead: embeddings and the head must live on one device")
        im = self.prepare()
        G, D = embeddings.shape
        if D != im["D"]:
            raise ValueError(f"GPHead: embeddings have width {D}, the inducing points {im['D']}")
        x = embeddings.detach()
        if G and (x.stride(1) != 1 or x.stride(0) < D):
            x = x.contiguous()
        ldx = x.stride(0) if G else D
        dev = x.device
        n_out = 5 if with_region else 2
        outs = [torch.empty(G, dtype=torch.float32, device=dev) for _ in range(n_out)]
        ptrs = [_ptr(t) for t in outs] + [None] * (5 - n_out)
        with torch.cuda.device(dev):
            rc = _lib.lib.cgat_gp_predict(_ptr(x), ldx, G, D, _ptr(im["zimg"]), im["M"], _ptr(im["centroid"]),
                                          _ptr(im["znorm"]), _ptr(im["factors"]), im["c"], im["s"], im["inv_two_l2"],
                                          im["mean"], im["std"], *ptrs, None, 0, _stream())
        _lib.check(rc, "cgat_gp_predict")
        return outs

    def latent(self, embeddings):
        """(mean_f, var_f) of the latent distribution, [G] each; differentiable in `embeddings` where autograd records
        (module docstring), like `predict` and `uncertainty`."""
        mean_f, var_f = self._run(embeddings, False)
        return mean_f, var_f

    def predict(self, embeddings):
        """(pred, lower, upper), [G] each, as gaussian_process.py:265-268 returns them (denormalised)."""
        _, _, pred, lower, upper = self._run(embeddings, True)
        return pred, lower, upper

    def uncertainty(self, embeddings):
        """upper - pred, the `uncertainty` column of Utilities/gp_predict.py:29."""
        pred, _, upper = self.predict(embeddings)
        return upper - pred

    def nlpd(self, embeddings, targets, noise):
        """The negative log predictive density of `targets` [G] under the Gaussian likelihood, per row and in the targets'
        units: the density N(pred, (var_f + noise) std^2).  `noise` is the likelihood's sigma^2 in units of the normalised
        targets, the value the report of `fit` carries.  Plain torch on top of `latent`, hence differentiable in the
        embeddings like it."""
        noise = float(noise)
        if not noise > 0.0:
            raise ValueError("GPHead.nlpd: noise must be positive")
        mean_f, var_f = self.latent(embeddings)
        im = self.prepare()
        y = torch.as_tensor(targets).detach().reshape(-1).to(device=mean_f.device, dtype=torch.float32)
        if y.numel() != mean_f.numel():
            raise ValueError(f"GPHead.nlpd: {mean_f.numel()} rows of embeddings, {y.numel()} targets")
        var = (var_f + noise) * (im["std"] * im["std"])
        resid = y - (mean_f * im["std"] + im["mean"])
        return 0.5 * (torch.log(2.0 * math.pi * var) + resid * resid / var)

    def predict_batch(self, model, batch, b_comp):
        """The graph embedding of `model` (a CGAtNet) for this batch, under eval() and no_grad, then `predict`."""
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                emb = model(batch, b_comp, return_graph_embedding=True)
        finally:
            model.train(was_training)
        return self.predict(emb)


def latent_adjoints(grads, var_f, std):
    """Reduces the incoming gradients of the five outputs of a prediction to those of the latent pair.
    `grads`: (g_mean_f, g_var_f, g_pred, g_lower, g_upper), [G] each or None; `var_f` [G] as the forward returned it (clamped
    at 0); `std` the target normalisation scalar.  Returns (gm, gv) = (dL/dmean_f, dL/dvar_f), each [G] or None where no
    output reaches it:

        gm = g_mean_f + std (g_pred + g_lower + g_upper)        gv = g_var_f + std (g_upper - g_lower) / sqrt(var_f)

    Where var_f is 0 the forward clamped it and the whole gv of that row is 0 (the subgradient torch's clamp_min takes):
    no infinity leaves this function.  Plain torch on the device of its arguments."""
    g_mean, g_var, g_pred, g_lower, g_upper = grads
    std = float(std)
    gm = g_mean
    for g in (g_pred, g_lower, g_upper):
        if g is not None:
            gm = std * g if gm is None else gm + std * g
    gv = g_var
    if g_lower is not None or g_upper is not None:
        positive = var_f > 0
        spread = g_upper if g_lower is None else -g_lower if g_upper is None else g_upper - g_lower
        term = std * spread * torch.where(positive, var_f, torch.ones_like(var_f)).rsqrt()
        gv = term if gv is None else gv + term
    if gv is not None:
        gv = torch.where(var_f > 0, gv, torch.zeros_like(gv))
    return gm, gv


def predictive_backward(head, embeddings, grad_mean, grad_var, chunk_rows=None):
    """dL/d embeddings [G, D] (a new contiguous fp32 tensor on their device) of a loss L of the latent prediction of
    `head` (a GPHead), given grad_mean = dL/dmean_f and grad_var = dL/dvar_f, [G] each; either may be None (mean only,
    variance only).  One cgat_gp_predict_backward call (csrc/gpback.hip); the head's buffers are constants.
    The clamp of var_f at 0 is not seen here: `latent_adjoints` zeroes grad_var there.  `chunk_rows` as for
    fit_statistics."""
    what = "predictive_backward"
    if not isinstance(head, GPHead):
        raise TypeError(f"{what}: head must be a GPHead")
    _require_gpu(head.inducing_points)
    im = head.prepare()
    x = _check_embeddings(what, embeddings, im["D"])
    if x.device != head.inducing_points.device:
        raise ValueError(f"{what}: embeddings and the head must live on one device")
    chunk = DEFAULT_CHUNK_ROWS if chunk_rows is None else int(chunk_rows)
    if chunk < 32 or chunk % 32:
        raise ValueError(f"{what}: chunk_rows = {chunk} is not a positive multiple of 32")
    G, D, M, dev = x.shape[0], im["D"], im["M"], x.device
    ups = []
    for name, g in (("grad_mean", grad_mean), ("grad_var", grad_var)):
        if g is not None:
            if not isinstance(g, torch.Tensor) or g.numel() != G:
                raise ValueError(f"{what}: {name} must hold one value per row of the embeddings ({G})")
            g = g.detach().reshape(-1).to(device=dev, dtype=torch.float32).contiguous()
        ups.append(g)
    gm, gv = ups
    if G == 0 or (gm is None and gv is None):
        return torch.zeros(G, D, dtype=torch.float32, device=dev)
    back = head.prepare_backward()
    ws_bytes = _lib.lib.cgat_gp_predict_backward_workspace_bytes(G, M, D, chunk)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
    dX = torch.empty(G, D, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib.cgat_gp_predict_backward(
            _ptr(x), x.stride(0), G, D, _ptr(im["zimg"]), M, _ptr(im["centroid"]), _ptr(im["znorm"]), _ptr(back["w1img"]),
            _ptr(back["w1timg"]), _ptr(back["g2img"]), _ptr(back["m"]), None if gm is None else _ptr(gm),
            None if gv is None else _ptr(gv), im["s"], im["inv_two_l2"], chunk, _ptr(back["ztimg"]), _ptr(dX), dX.stride(0),
            _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "cgat_gp_predict_backward")
    return dX


class _Prediction(torch.autograd.Function):
    """cgat_gp_predict as a function of the embeddings: the forward is GPHead._predict, the backward reduces the incoming
    gradients to (gm, gv) (latent_adjoints) and runs predictive_backward.  Saves the embeddings, var_f and std."""

    @staticmethod
    def forward(ctx, head, embeddings, with_region):
        outs = head._predict(embeddings, with_region)
        ctx.head, ctx.key, ctx.std = head, head._key(), head.prepare()["std"]
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(embeddings, outs[1])
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        embeddings, var_f = ctx.saved_tensors
        if ctx.head._key() != ctx.key:
            raise RuntimeError("GPHead: a buffer of the head changed between a prediction and its backward")
        gm, gv = latent_adjoints(tuple(grads) + (None,) * (5 - len(grads)), var_f, ctx.std)
        return None, predictive_backward(ctx.head, embeddings, gm, gv), None
