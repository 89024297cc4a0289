"""The sparse-GP head (cgat_amd.GPHead.predict, one cgat_gp_predict launch, csrc/gphead.hip) at screening size:
G = 1 000 000 embeddings, M = 1000 inducing points, D = 384 and 640 (the reference's defaults: atom_fea_len x msg_heads),
against an eager torch fp32 evaluation of the SAME factors on the same box (same centring, same a / W1 / W2, the
G x M cross-kernel matrix materialised chunk by chunk so that it fits).  Device events around each call, warm-up, the two
arms alternated in one process; median / min / max.  Beside the times: the FLOPs the algorithm needs (cross products, the
triangle of W1, W2, the dot with a), the kernel's share of the f32-input matrix peak (157.3 TF), and the largest
difference between the two arms' outputs and of each from an fp64 restatement on a subsample.
Writes one JSON object to --out and prints it.

    python tools/gp_predict_bench.py [--reps 7] [--rows 1000000] [--out profiles/gp_predict_bench.json]
    python tools/gp_predict_bench.py --only-profile        # a few fused launches, for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

F32_MATRIX_PEAK_TF = 157.3


class EagerFactorForm:
    """The factor form in eager torch fp32 on the head's own factors (rounded to fp32 as the kernel's image is): what a
    user without the fused kernel would run."""

    def __init__(self, head, chunk, dev):
        f = head._factors64()
        f32 = lambda t: t.to(torch.float32).to(dev).contiguous()
        self.Zc, self.a, self.zn, self.cen = f32(f["Zc"]), f32(f["a"]), f32(f["znorm"]), f32(f["centroid"])
        self.W1t, self.W2t = f32(f["W1"].t()), f32(f["W2"].t())
        self.im, self.chunk = f, chunk

    def __call__(self, X):
        im = self.im
        outs = [torch.empty(X.shape[0], dtype=torch.float32, device=X.device) for _ in range(3)]
        for i in range(0, X.shape[0], self.chunk):
            xc = X[i:i + self.chunk] - self.cen
            d2 = torch.addmm(self.zn[None, :] + xc.square().sum(1, keepdim=True), xc, self.Zc.t(), alpha=-2.0)
            kx = d2.clamp_min_(0).mul_(-im["inv_two_l2"]).exp_().mul_(im["s"])
            mean_f = torch.addmv(torch.full((kx.shape[0],), im["c"], device=X.device), kx, self.a)
            var_f = (im["s"] - (kx @ self.W1t).square_().sum(1) + (kx @ self.W2t).square_().sum(1)).clamp_min_(0)
            two_sd = 2 * var_f.sqrt_()
            sl = slice(i, i + self.chunk)
            outs[0][sl] = mean_f * im["std"] + im["mean"]
            outs[1][sl] = (mean_f - two_sd) * im["std"] + im["mean"]
            outs[2][sl] = (mean_f + two_sd) * im["std"] + im["mean"]
        return tuple(outs)


def _time_alternating(fns, reps, warmup=2):
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            ts[k].append(a.elapsed_time(b))
    out = {}
    for k, v in ts.items():
        v.sort()
        out[k] = {"ms_median": round(v[len(v) // 2], 3), "ms_min": round(v[0], 3), "ms_max": round(v[-1], 3)}
    return out


def needed_flops(G, M, D):
    return 2.0 * G * M * D + 2.0 * G * (M * (M + 1) / 2 + M * M + M)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--inducing", type=int, default=1000)
    ap.add_argument("--widths", type=int, nargs="+", default=[384, 640])
    ap.add_argument("--chunk", type=int, default=65536, help="rows per chunk of the eager arm (K chunk = chunk x M x 4 B)")
    ap.add_argument("--subsample", type=int, default=512, help="rows checked against the fp64 restatement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_predict_bench.json"))
    ap.add_argument("--only-profile", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gp_predict_bench: no GPU visible; times are measured on the device or not at all")
    import cgat_amd as P
    import gp_cases
    dev = "cuda:0"
    G, M = args.rows, args.inducing
    out = {"tool": "gp_predict_bench", "device": torch.cuda.get_device_name(0), "G": G, "M": M, "reps": args.reps,
           "eager_chunk_rows": args.chunk, "f32_matrix_peak_tf": F32_MATRIX_PEAK_TF}
    for D in args.widths:
        p, _ = gp_cases.build_inputs(1, M, D)
        head = P.GPHead.from_tensors(p).to(dev)
        X = 0.5 + torch.randn(G, D, device=dev, generator=torch.Generator(dev).manual_seed(D))
        head.prepare()
        if args.only_profile:
            for _ in range(3):
                head.predict(X)
            torch.cuda.synchronize()
            continue
        eager = EagerFactorForm(head, args.chunk, dev)
        times = _time_alternating({"fused": lambda: head.predict(X), "eager_fp32": lambda: eager(X)}, args.reps)
        fused, ref32 = head.predict(X), eager(X)
        n = min(args.subsample, G)
        ref64 = gp_cases.factor_form(p, X[:n].cpu())
        norm = [float(ref64[k].abs().max()) for k in ("pred", "lower", "upper")]
        err = lambda got: max(float((g[:n].cpu().double() - ref64[k]).abs().max()) / nm
                              for g, k, nm in zip(got, ("pred", "lower", "upper"), norm))
        flops = needed_flops(G, M, D)
        ms = times["fused"]["ms_median"]
        out[f"D{D}"] = {"fused": times["fused"], "eager_fp32": times["eager_fp32"],
                        "eager_over_fused": round(times["eager_fp32"]["ms_median"] / ms, 3),
                        "needed_tflop": round(flops / 1e12, 4), "fused_tflops": round(flops / ms / 1e9, 2),
                        "fused_share_of_f32_matrix_peak": round(flops / ms / 1e9 / F32_MATRIX_PEAK_TF, 4),
                        "rows_per_s_fused": round(G / ms * 1e3, 1),
                        "max_rel_diff_fused_vs_eager": max(float((a - b).abs().max() / b.abs().max())
                                                           for a, b in zip(fused, ref32)),
                        "max_rel_err_vs_fp64_subsample": {"fused": err(fused), "eager_fp32": err(ref32)}}
        del X, eager, fused, ref32
        torch.cuda.empty_cache()
    if args.only_profile:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
