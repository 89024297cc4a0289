"""The derivative of the sparse-GP head's prediction in its input (cgat_gp_predict_backward, csrc/gpback.hip) at
screening size: G = 1 000 000 embeddings, M = 1000 inducing points, D = 384 and 640.  The loss is
sum_n gm_n mean_f_n + gv_n var_f_n for seeded gm, gv, so both latent outputs carry a gradient.  Arms, alternated in one
process, device events around each call, warm-up; median / min / max:

    forward              head.latent(X) without grad: one cgat_gp_predict launch
    forward_backward     head.latent(X) with X.requires_grad, the loss, loss.backward(): the forward, the [G] torch
                         arithmetic of the loss and of latent_adjoints, one cgat_gp_predict_backward call
    backward             predictive_backward(head, X, gm, gv) alone (the workspace and dX come from torch's caching
                         allocator, as they do under autograd)
    backward_mean_only   the same with gv = None: alpha and the G2 product are not formed
    eager_fp32           torch fp32 autograd through the factor form on the head's own factors (tools/gp_predict_bench.py's
                         EagerFactorForm arithmetic, kept differentiable), forward and backward per chunk of rows

Beside the times: the FLOPs the backward needs (two cross products, the triangles of W1 and W1^T, G2, the product with
Zc^T), its rate against the f32-input matrix peak (157.3 TF), and the largest difference between the fused and the eager dX
relative to max |dX|.  Writes one JSON object to --out and prints it.

    python tools/gp_predict_grad_bench.py [--reps 7] [--rows 1000000] [--out profiles/gp_predict_grad_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gp_predict_bench import F32_MATRIX_PEAK_TF, _time_alternating  # noqa: E402


class EagerAutograd:
    """dL/dX of L = sum_n gm_n mean_f_n + gv_n var_f_n by torch autograd through the factor form in fp32, on the head's own
    factors, chunk by chunk (the G x M matrices of a chunk live until its backward has run)."""

    def __init__(self, head, chunk, dev):
        f = head._factors64()
        f32 = lambda t: t.to(torch.float32).to(dev).contiguous()
        self.Zc, self.a, self.zn, self.cen = f32(f["Zc"]), f32(f["a"]), f32(f["znorm"]), f32(f["centroid"])
        self.W1t, self.W2t = f32(f["W1"].t()), f32(f["W2"].t())
        self.im, self.chunk = f, chunk

    def __call__(self, X, gm, gv, dX):
        im = self.im
        for i in range(0, X.shape[0], self.chunk):
            sl = slice(i, i + self.chunk)
            x = X[sl].detach().requires_grad_(True)
            xc = x - self.cen
            d2 = torch.addmm(self.zn[None, :] + xc.square().sum(1, keepdim=True), xc, self.Zc.t(), alpha=-2.0)
            kx = d2.clamp_min(0).mul(-im["inv_two_l2"]).exp().mul(im["s"])
            mean_f = kx @ self.a + im["c"]
            var_f = im["s"] - (kx @ self.W1t).square().sum(1) + (kx @ self.W2t).square().sum(1)
            dX[sl] = torch.autograd.grad((gm[sl] * mean_f).sum() + (gv[sl] * var_f).sum(), x)[0]
        return dX


def needed_flops(G, M, D, variance=True):
    """Of one backward: the cross products of the recomputed distances, u = W1^T q and r^T Zc; with the variance also
    those of alpha (its distances, the triangle of W1) and G2 alpha."""
    flops = 2.0 * G * M * D + 2.0 * G * M * (M + 1) / 2 + 2.0 * G * M * D
    if variance:
        flops += 2.0 * G * M * D + 2.0 * G * M * (M + 1) / 2 + 2.0 * G * M * M
    return flops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--inducing", type=int, default=1000)
    ap.add_argument("--widths", type=int, nargs="+", default=[384, 640])
    ap.add_argument("--chunk", type=int, default=65536, help="rows per chunk of the eager arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_predict_grad_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gp_predict_grad_bench: no GPU visible; times are measured on the device or not at all")
    import cgat_amd as P
    import gp_cases
    dev = "cuda:0"
    G, M = args.rows, args.inducing
    out = {"tool": "gp_predict_grad_bench", "device": torch.cuda.get_device_name(0), "G": G, "M": M, "reps": args.reps,
           "chunk_rows": P.gp.DEFAULT_CHUNK_ROWS, "eager_chunk_rows": args.chunk, "f32_matrix_peak_tf": F32_MATRIX_PEAK_TF}
    for D in args.widths:
        p, _ = gp_cases.build_inputs(1, M, D)
        head = P.GPHead.from_tensors(p).to(dev)
        g = torch.Generator(dev).manual_seed(D)
        X = 0.5 + torch.randn(G, D, device=dev, generator=g)
        gm, gv = torch.randn(G, device=dev, generator=g), torch.randn(G, device=dev, generator=g)
        head.prepare()
        head.prepare_backward()
        eager = EagerAutograd(head, args.chunk, dev)
        dX_eager = torch.empty(G, D, device=dev)
        Xg = X.clone().requires_grad_(True)

        def forward():
            with torch.no_grad():
                return head.latent(X)

        def forward_backward():
            Xg.grad = None
            mean_f, var_f = head.latent(Xg)
            ((gm * mean_f).sum() + (gv * var_f).sum()).backward()

        times = _time_alternating({"forward": forward, "forward_backward": forward_backward,
                                   "backward": lambda: P.predictive_backward(head, X, gm, gv),
                                   "backward_mean_only": lambda: P.predictive_backward(head, X, gm, None),
                                   "eager_fp32": lambda: eager(X, gm, gv, dX_eager)}, args.reps)
        forward_backward()
        torch.cuda.synchronize()
        # the forward clamps var_f at 0 and latent_adjoints zeroes gv there; the eager arm differentiates the unclamped form
        clamped = int((head.latent(X)[1] == 0).sum())
        eager(X, gm, gv, dX_eager)
        diff = float((Xg.grad - dX_eager).abs().max() / dX_eager.abs().max())
        ms, ms_mean = times["backward"]["ms_median"], times["backward_mean_only"]["ms_median"]
        flops, flops_mean = needed_flops(G, M, D), needed_flops(G, M, D, variance=False)
        out[f"D{D}"] = {**times,
                        "forward_backward_minus_forward_ms": round(times["forward_backward"]["ms_median"]
                                                                   - times["forward"]["ms_median"], 3),
                        "eager_over_forward_backward": round(times["eager_fp32"]["ms_median"]
                                                             / times["forward_backward"]["ms_median"], 3),
                        "backward_needed_tflop": round(flops / 1e12, 4),
                        "backward_tflops": round(flops / ms / 1e9, 2),
                        "backward_share_of_f32_matrix_peak": round(flops / ms / 1e9 / F32_MATRIX_PEAK_TF, 4),
                        "backward_mean_only_tflops": round(flops_mean / ms_mean / 1e9, 2),
                        "dX_bytes_gib": round(G * D * 4 / 2 ** 30, 3),
                        "rows_with_clamped_variance": clamped,
                        "max_rel_diff_dX_fused_vs_eager": diff}
        del X, Xg, eager, dX_eager, gm, gv, head
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
