"""The gradient of the collapsed sparse-GP bound (cgat_amd.bound_and_gradient: cgat_gp_fit_stats, the host's fp64 solve
and adjoints, cgat_gp_fit_grad -- gp_whiten_rows, gp_apply_factor twice, gp_weight_rows, gp_centre_rows, gp_pair_slabs and
two reductions per chunk, csrc/gpgrad.hip) at training size: N = 1 000 000 embeddings, M = 1000 inducing points, D = 384
and 640.  Three arms, alternated in one process, device events around each call, warm-up; median / min / max:

    grad_pass_device_only   the C entry cgat_gp_fit_grad alone on prepared operands
    stats_pass_device_only  cgat_gp_fit_stats alone, the sibling the gradient pass is compared with
    bound_and_gradient      one evaluation as an optimiser makes it: both passes, the host's factorisation of K_zz, the
                            solve, the adjoints, the pull-back through the Cholesky factor, the uploads
    eager_fp32              an eager torch fp32 evaluation of the SAME three sums on the same box (same centring, W1, 2 G^
                            and g; the N x M matrices materialised chunk by chunk, the chunks added in fp64)

Beside the times: the FLOPs the algorithm needs (cross products twice, the triangle of W1 twice, the full product with
2 G^, R^T Xc), the gradient pass's share of the f32-input matrix peak (157.3 TF), the workspace, and the largest
difference between the fused and the eager sums, block by block, relative to the block's max-norm.  Writes one JSON
object to --out and prints it.

    python tools/gp_grad_bench.py [--reps 5] [--rows 1000000] [--out profiles/gp_grad_bench.json]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gp_predict_bench import F32_MATRIX_PEAK_TF, _time_alternating  # noqa: E402


class EagerSums:
    """colsum, d2sum, P in eager torch fp32 on the factors the fused pass uses (rounded to fp32 as its images are)."""

    def __init__(self, Z, s, ell, jitter, two_G_hat, g, c, chunk, dev):
        from cgat_amd import gp
        cen, Zc, zn = gp._centred64(Z.to("cpu", torch.float64))
        _, W1 = gp._whitening64(Zc, zn, s, ell, jitter)
        f32 = lambda t: t.to(torch.float32).to(dev).contiguous()
        self.Zc, self.zn, self.cen, self.W1, self.W1t = f32(Zc), f32(zn), f32(cen), f32(W1), f32(W1.t())
        self.G2, self.g = f32(two_G_hat), f32(g)
        self.s, self.inv_two_l2, self.c, self.chunk = s, 0.5 / (ell * ell), c, chunk

    def __call__(self, X, y):
        M, D = self.Zc.shape
        colsum = torch.zeros(M, dtype=torch.float64, device=X.device)
        d2sum = torch.zeros(M, dtype=torch.float64, device=X.device)
        P = torch.zeros(M, D, dtype=torch.float64, device=X.device)
        for i in range(0, X.shape[0], self.chunk):
            xc = X[i:i + self.chunk] - self.cen
            d2 = torch.addmm(self.zn[None, :] + xc.square().sum(1, keepdim=True), xc, self.Zc.t(), alpha=-2.0).clamp_min_(0)
            kx = d2.mul(-self.inv_two_l2).exp_().mul_(self.s)
            q = torch.addmm(torch.outer(y[i:i + self.chunk] - self.c, self.g), kx @ self.W1t, self.G2)   # G2 is symmetric
            r = (q @ self.W1).mul_(kx)
            colsum += r.sum(0).double()
            d2sum += (r * d2).sum(0).double()
            P += (r.t() @ xc).double()
        return colsum, d2sum, P


def needed_flops(N, M, D):
    """cross products (twice), W1 and W1^T (a triangle each), 2 G^ (full), R^T Xc."""
    return 2.0 * N * (2 * M * D + 2 * (M * (M + 1) / 2) + M * M + M * D)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--inducing", type=int, default=1000)
    ap.add_argument("--widths", type=int, nargs="+", default=[384, 640])
    ap.add_argument("--chunk", type=int, default=65536, help="rows per chunk of the eager arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_grad_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gp_grad_bench: no GPU visible; times are measured on the device or not at all")
    from cgat_amd import _lib, gp
    from cgat_amd.ops import _ptr, _stream
    dev = "cuda:0"
    N, M, s, jitter = args.rows, args.inducing, 1.3, 1e-4
    out = {"tool": "gp_grad_bench", "device": torch.cuda.get_device_name(0), "N": N, "M": M, "reps": args.reps,
           "chunk_rows": gp.DEFAULT_CHUNK_ROWS, "eager_chunk_rows": args.chunk, "f32_matrix_peak_tf": F32_MATRIX_PEAK_TF}
    for D in args.widths:
        g = torch.Generator(dev).manual_seed(D)
        X = 0.5 + torch.randn(N, D, device=dev, generator=g)
        w = torch.randn(D, device=dev, generator=g) / math.sqrt(D)
        y = torch.sin(1.3 * ((X - 0.5) @ w)) + 0.3 * torch.randn(N, device=dev, generator=g)
        y = (y - y.mean()) / y.std()
        Z, ell = X[:M].cpu(), math.sqrt(D)
        both = gp._GradientPass("gp_grad_bench", X, y, Z, None)
        st = both.stats
        sol, _ = both(s, ell, jitter)
        adj = gp.collapsed_adjoints(st.gram, N, s, sol)
        two_G_hat, c = 2.0 * adj["G_hat"], sol["constant"]
        eager = EagerSums(Z, s, ell, jitter, two_G_hat, adj["g"], c, args.chunk, dev)
        # the C entries alone, on operands prepared once
        ops, inv = st.ops, 0.5 / (ell * ell)
        st.factor(s, ell, jitter)
        w1img, w1timg, g2img = st.w1img, st.image(st.W1.T), st.image(two_G_hat)
        g32 = adj["g"].to(torch.float32).to(dev)
        grad_ws = _lib.lib.cgat_gp_fit_grad_workspace_bytes(N, M, D, st.chunk)

        def grad_only():
            _lib.check(_lib.lib.cgat_gp_fit_grad(_ptr(X), X.stride(0), _ptr(st.y32), N, D, _ptr(ops["zimg"]), M,
                                                 _ptr(ops["centroid"]), _ptr(ops["znorm"]), _ptr(w1img), _ptr(w1timg),
                                                 _ptr(g2img), _ptr(g32), c, s, inv, st.chunk, _ptr(both.colsum),
                                                 _ptr(both.d2sum), _ptr(both.P), _ptr(st.ws), grad_ws, _stream()),
                       "cgat_gp_fit_grad")

        def stats_only():
            _lib.check(_lib.lib.cgat_gp_fit_stats(_ptr(X), X.stride(0), _ptr(st.y32), N, D, _ptr(ops["zimg"]), M,
                                                  _ptr(ops["centroid"]), _ptr(ops["znorm"]), _ptr(w1img), s, inv, st.chunk,
                                                  _ptr(st.gram), _ptr(st.ws), st.ws_bytes, _stream()), "cgat_gp_fit_stats")

        times = _time_alternating({"grad_pass_device_only": grad_only, "stats_pass_device_only": stats_only,
                                   "bound_and_gradient": lambda: both(s, ell, jitter),
                                   "eager_fp32": lambda: eager(X, y)}, args.reps)
        grad_only()
        fused = [t.clone() for t in (both.colsum, both.d2sum, both.P)]
        ref32 = eager(X, y)
        diff = {k: float((a - b).abs().max() / b.abs().max()) for k, a, b in zip(("colsum", "d2sum", "P"), fused, ref32)}
        flops = needed_flops(N, M, D)
        ms = times["grad_pass_device_only"]["ms_median"]
        out[f"D{D}"] = {**times,
                        "eager_over_grad_pass": round(times["eager_fp32"]["ms_median"] / ms, 3),
                        "grad_pass_over_stats_pass": round(ms / times["stats_pass_device_only"]["ms_median"], 3),
                        "needed_tflop": round(flops / 1e12, 4), "grad_pass_tflops": round(flops / ms / 1e9, 2),
                        "grad_pass_share_of_f32_matrix_peak": round(flops / ms / 1e9 / F32_MATRIX_PEAK_TF, 4),
                        "workspace_mib": round(max(grad_ws, st.ws_bytes) / 2 ** 20, 1),
                        "max_rel_diff_fused_vs_eager_per_block": diff}
        del X, y, eager, fused, ref32, both, st
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
