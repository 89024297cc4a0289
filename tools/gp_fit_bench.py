"""The data pass of the sparse-GP fit (cgat_amd.gp.fit_statistics, one cgat_gp_fit_stats call: gp_whiten_rows,
gp_gram_slabs and gp_gram_reduce per chunk, csrc/gpfit.hip) at training size: N = 1 000 000 embeddings, M = 1000 inducing
points, D = 384 and 640, against an eager torch fp32 evaluation of the SAME statistics on the same box (same centring,
same W1, the N x M whitened matrix materialised chunk by chunk, its Gram product in fp32 per chunk, the chunks added in
fp64).  Device events around each call, warm-up, the two arms alternated in one process; median / min / max.  Beside the
times: the FLOPs the algorithm needs (cross products, the triangle of W1, the lower triangle of the Gram product), the
pass's share of the f32-input matrix peak (157.3 TF), and the largest difference between the two arms' statistics, block
by block, relative to the block's max-norm.  The fused arm includes the host's fp64 factorisation of K_zz and the upload of
its image, as every call of fit_statistics does; `fused_device_only` times the C entry alone on prepared operands.
Writes one JSON object to --out and prints it.

    python tools/gp_fit_bench.py [--reps 7] [--rows 1000000] [--out profiles/gp_fit_bench.json]
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


class EagerStatistics:
    """The statistics in eager torch fp32 on the factors fit_statistics uses (rounded to fp32 as its images are)."""

    def __init__(self, Z, s, ell, jitter, chunk, dev):
        from cgat_amd import gp
        cen, Zc, zn = gp._centred64(Z.to("cpu", torch.float64))
        _, W1 = gp._whitening64(Zc, zn, s, ell, jitter)
        f32 = lambda t: t.to(torch.float32).to(dev).contiguous()
        self.Zc, self.zn, self.cen, self.W1t = f32(Zc), f32(zn), f32(cen), f32(W1.t())
        self.s, self.inv_two_l2, self.chunk = s, 0.5 / (ell * ell), chunk

    def __call__(self, X, y):
        M = self.Zc.shape[0]
        G = torch.zeros(M + 2, M + 2, dtype=torch.float64, device=X.device)
        for i in range(0, X.shape[0], self.chunk):
            xc = X[i:i + self.chunk] - self.cen
            d2 = torch.addmm(self.zn[None, :] + xc.square().sum(1, keepdim=True), xc, self.Zc.t(), alpha=-2.0)
            kx = d2.clamp_min_(0).mul_(-self.inv_two_l2).exp_().mul_(self.s)
            At = torch.empty(kx.shape[0], M + 2, dtype=torch.float32, device=X.device)
            torch.mm(kx, self.W1t, out=At[:, :M])
            At[:, M] = y[i:i + self.chunk]
            At[:, M + 1] = 1.0
            G += (At.t() @ At).double()
        return G


def needed_flops(N, M, D):
    return 2.0 * N * M * D + 2.0 * N * (M * (M + 1) / 2) + 2.0 * N * ((M + 2) * (M + 3) / 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--inducing", type=int, default=1000)
    ap.add_argument("--widths", type=int, nargs="+", default=[384, 640])
    ap.add_argument("--chunk", type=int, default=65536, help="rows per chunk of the eager arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_fit_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gp_fit_bench: no GPU visible; times are measured on the device or not at all")
    from cgat_amd import _lib, gp
    from cgat_amd.ops import _ptr, _stream
    dev = "cuda:0"
    N, M, s, jitter = args.rows, args.inducing, 1.3, 1e-4
    out = {"tool": "gp_fit_bench", "device": torch.cuda.get_device_name(0), "N": N, "M": M, "reps": args.reps,
           "chunk_rows": gp.DEFAULT_CHUNK_ROWS, "eager_chunk_rows": args.chunk, "f32_matrix_peak_tf": F32_MATRIX_PEAK_TF}
    for D in args.widths:
        g = torch.Generator(dev).manual_seed(D)
        X = 0.5 + torch.randn(N, D, device=dev, generator=g)
        y = torch.randn(N, device=dev, generator=g)
        Z, ell = X[:M].cpu(), math.sqrt(D)
        eager = EagerStatistics(Z, s, ell, jitter, args.chunk, dev)

        # the C entry alone, on operands prepared once
        cen, Zc, zn = gp._centred64(Z.to(torch.float64))
        _, W1 = gp._whitening64(Zc, zn, s, ell, jitter)
        ops = gp._tile_operands(cen, Zc, zn, dev)
        Mp = (M + 31) // 32 * 32
        W1p = torch.zeros(Mp, Mp)
        W1p[:M, :M] = W1
        w1img = gp._pack_image(W1p).to(dev)
        gram = torch.empty(M + 2, M + 2, dtype=torch.float64, device=dev)
        ws_bytes = _lib.lib.cgat_gp_fit_stats_workspace_bytes(N, M, D, gp.DEFAULT_CHUNK_ROWS)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

        def device_only():
            _lib.check(_lib.lib.cgat_gp_fit_stats(_ptr(X), X.stride(0), _ptr(y), N, D, _ptr(ops["zimg"]), M,
                                                  _ptr(ops["centroid"]), _ptr(ops["znorm"]), _ptr(w1img), s,
                                                  0.5 / (ell * ell), gp.DEFAULT_CHUNK_ROWS, _ptr(gram), _ptr(ws), ws_bytes,
                                                  _stream()), "cgat_gp_fit_stats")

        times = _time_alternating({"fused": lambda: gp.fit_statistics(X, y, Z, s, ell, jitter=jitter),
                                   "fused_device_only": device_only, "eager_fp32": lambda: eager(X, y)}, args.reps)
        fused, ref32 = gp.fit_statistics(X, y, Z, s, ell, jitter=jitter), eager(X, y)
        blocks = {"Psi": (slice(0, M), slice(0, M)), "Ay": (slice(0, M), M), "A1": (slice(0, M), M + 1), "yy": (M, M),
                  "sum_y": (M, M + 1)}
        diff = {k: float((fused[ix] - ref32[ix]).abs().max() / ref32[ix].abs().max()) for k, ix in blocks.items()}
        flops = needed_flops(N, M, D)
        ms = times["fused_device_only"]["ms_median"]
        out[f"D{D}"] = {**times, "eager_over_fused": round(times["eager_fp32"]["ms_median"] / times["fused"]["ms_median"], 3),
                        "eager_over_fused_device_only": round(times["eager_fp32"]["ms_median"] / ms, 3),
                        "needed_tflop": round(flops / 1e12, 4), "fused_device_only_tflops": round(flops / ms / 1e9, 2),
                        "fused_device_only_share_of_f32_matrix_peak": round(flops / ms / 1e9 / F32_MATRIX_PEAK_TF, 4),
                        "workspace_mib": round(ws_bytes / 2 ** 20, 1), "n_exact": float(fused[M + 1, M + 1]) == float(N),
                        "max_rel_diff_fused_vs_eager_per_block": diff}
        del X, y, eager, fused, ref32, ws
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
