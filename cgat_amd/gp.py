"""Prediction with uncertainty: a sparse variational Gaussian-process head on graph embeddings.

The reference's screening / active-learning flow continues past the graph embedding: `train-GP`
(CGAT/gaussian_process.py) fits a sparse variational GP on the embeddings and Utilities/gp_predict.py writes, per
candidate, `prediction` and `uncertainty = upper - prediction`.  This module is the PREDICTION side of that GP, fused
into one HIP launch (csrc/gphead.hip); training the GP (the ELBO) is out of scope.

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

Inference only: outputs carry no grad; non-GPU and non-fp32 inputs are refused like everywhere else in the package.
"""
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

    @classmethod
    def from_tensors(cls, mapping, jitter=1e-4):
        """From a plain dict with exactly the keys of the buffers above."""
        if set(mapping) != set(_KEYS):
            raise KeyError(f"GPHead.from_tensors: expected exactly the keys {sorted(_KEYS)}, got {sorted(mapping)}")
        return cls(*(mapping[k] for k in _KEYS), jitter=jitter)

    # --------------------------------------------------------------------------------------------------------------
    def _key(self):
        return (self.jitter,) + tuple((t.data_ptr(), t._version, t.device) for t in (getattr(self, k) for k in _KEYS))

    def _factors64(self):
        """c, s, l, mean, std as Python floats and, in fp64 on the host: the centroid of Z, Zc = Z - centroid, |zc|^2,
        a = L^-T m, W1 = L^-1 (exactly lower triangular), W2 = L_S^T L^-1."""
        Z = self.inducing_points.detach().to("cpu", torch.float64)
        m = self.variational_mean.detach().to("cpu", torch.float64)
        LS = self.chol_variational_covar.detach().to("cpu", torch.float64).tril()
        c, s, ell, tm, ts = (float(getattr(self, k)) for k in ("constant", "outputscale", "lengthscale", "mean", "std"))
        if not (s > 0.0 and ell > 0.0):
            raise ValueError("GPHead: outputscale and lengthscale must be positive")
        M = Z.shape[0]
        cen = Z.mean(dim=0)
        Zc = Z - cen
        zn = (Zc * Zc).sum(dim=1)
        d2 = (zn[:, None] + zn[None, :] - 2.0 * (Zc @ Zc.T)).clamp_min(0.0)
        d2.fill_diagonal_(0.0)
        Kzz = s * torch.exp(-0.5 * d2 / (ell * ell))
        L = torch.linalg.cholesky(Kzz + self.jitter * torch.eye(M, dtype=torch.float64))
        a = torch.linalg.solve_triangular(L.T, m[:, None], upper=True)[:, 0]
        W1 = torch.linalg.solve_triangular(L, torch.eye(M, dtype=torch.float64), upper=False).tril()
        return dict(c=c, s=s, inv_two_l2=0.5 / (ell * ell), mean=tm, std=ts, centroid=cen, Zc=Zc, znorm=zn, a=a, W1=W1,
                    W2=LS.T @ W1)

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
        Mp, Dp = (M + 31) // 32 * 32, (D + 63) // 64 * 64
        Zp = torch.zeros(Mp, Dp, dtype=torch.float32)
        Zp[:M, :D] = f["Zc"]
        F = torch.zeros(2 * Mp, Mp, dtype=torch.float32)
        F[:M, :M] = f["W1"]
        F[Mp:Mp + M, :M] = f["W2"]
        factors = torch.zeros(Mp + 2 * Mp * Mp, dtype=torch.float32)
        factors[:M] = f["a"]
        factors[Mp:] = _pack_image(F)
        znp = torch.zeros(Mp, dtype=torch.float32)
        znp[:M] = f["znorm"]
        self._image = dict(M=M, D=D, c=f["c"], s=f["s"], inv_two_l2=f["inv_two_l2"], mean=f["mean"], std=f["std"],
                           zimg=_pack_image(Zp).to(dev), centroid=f["centroid"].to(torch.float32).to(dev),
                           znorm=znp.to(dev), factors=factors.to(dev))
        self._image_key = key
        return self._image

    # --------------------------------------------------------------------------------------------------------------
    def _run(self, embeddings, with_region):
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
        """(mean_f, var_f) of the latent distribution, [G] each."""
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
