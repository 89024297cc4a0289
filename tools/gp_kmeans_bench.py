"""One Lloyd step of the k-means inducing points (cgat_amd.gp.kmeans_step, one cgat_gp_kmeans_step call: gp_assign_rows and
the row sums of the gradient pass per chunk, csrc/gpkmeans.hip) at training size: N = 1 000 000 embeddings,
M = 1000 centres, D = 384 and 640, against an eager torch fp32 step on the same box (same centring; per chunk of rows
|x|^2 + |z|^2 - 2 x z^T, argmin, index_add_ of the rows, the counts and the minima; the chunks added in fp64).  Device
events around each call, warm-up, the arms alternated in one process; median / min / max.  `fused` is the whole
kmeans_step (the host's fp64 centring of Z, the upload of its image, the allocation of the outputs), `fused_device_only`
the C entry alone on prepared operands.  Beside the times: the f32 matrix work the step executes (the distances and the
one-hot product, 2 N M D each) and what the algorithm needs (the distances and N D additions), the share of the f32-input
matrix peak (157.3 TF) the executed work reaches, the bytes of the one-hot chunk buffer written and read back, the share
of rows both arms assign alike and the largest difference of their sums relative to the max-norm.
Writes one JSON object to --out and prints it.

    python tools/gp_kmeans_bench.py [--reps 7] [--rows 1000000] [--out profiles/gp_kmeans_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gp_predict_bench import F32_MATRIX_PEAK_TF, _time_alternating  # noqa: E402


class EagerStep:
    """The step in eager torch fp32 on the operands kmeans_step uses (centred by the fp32 centroid of Z)."""

    def __init__(self, Z, chunk, dev):
        from cgat_amd import gp
        cen, Zc, zn = gp._centred64(Z.to("cpu", torch.float64))
        f32 = lambda t: t.to(torch.float32).to(dev).contiguous()
        self.Zct, self.zn, self.cen, self.chunk = f32(Zc.t()), f32(zn), f32(cen), chunk

    def __call__(self, X):
        M, D, dev = self.zn.shape[0], X.shape[1], X.device
        assign = torch.empty(X.shape[0], dtype=torch.int64, device=dev)
        counts, wss = torch.zeros(M, dtype=torch.float64, device=dev), torch.zeros(M, dtype=torch.float64, device=dev)
        sums = torch.zeros(M, D, dtype=torch.float64, device=dev)
        for i in range(0, X.shape[0], self.chunk):
            xc = X[i:i + self.chunk] - self.cen
            d2 = torch.addmm(self.zn[None, :] + xc.square().sum(1, keepdim=True), xc, self.Zct, alpha=-2.0)
            best, a = d2.clamp_min_(0).min(dim=1)
            assign[i:i + self.chunk] = a
            counts += torch.bincount(a, minlength=M).double()
            wss += torch.zeros(M, dtype=torch.float32, device=dev).index_add_(0, a, best).double()
            sums += torch.zeros(M, D, dtype=torch.float32, device=dev).index_add_(0, a, xc).double()
        return assign, counts, wss, sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--centres", type=int, default=1000)
    ap.add_argument("--widths", type=int, nargs="+", default=[384, 640])
    ap.add_argument("--chunk", type=int, default=65536, help="rows per chunk of the eager arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_kmeans_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gp_kmeans_bench: no GPU visible; times are measured on the device or not at all")
    from cgat_amd import _lib, gp
    from cgat_amd.ops import _ptr, _stream
    dev = "cuda:0"
    N, M = args.rows, args.centres
    out = {"tool": "gp_kmeans_bench", "device": torch.cuda.get_device_name(0), "N": N, "M": M, "reps": args.reps,
           "chunk_rows": gp.DEFAULT_CHUNK_ROWS, "eager_chunk_rows": args.chunk, "f32_matrix_peak_tf": F32_MATRIX_PEAK_TF}
    for D in args.widths:
        g = torch.Generator(dev).manual_seed(D)
        # a mixture of 16 clusters, offset so that the centring matters; the centres are rows of it
        means = 2.0 * torch.randn(16, D, device=dev, generator=g)
        X = 0.5 + means[torch.randint(0, 16, (N,), device=dev, generator=g)] + torch.randn(N, D, device=dev, generator=g)
        Z = X[:M].cpu()
        eager = EagerStep(Z, args.chunk, dev)

        # the C entry alone, on operands prepared once
        ops = gp._tile_operands(*gp._centred64(Z.to(torch.float64)), dev)
        assign = torch.empty(N, dtype=torch.int32, device=dev)
        counts, wss = (torch.empty(M, dtype=torch.float64, device=dev) for _ in range(2))
        sums = torch.empty(M, D, dtype=torch.float64, device=dev)
        ws_bytes = _lib.lib.cgat_gp_kmeans_step_workspace_bytes(N, M, D, gp.DEFAULT_CHUNK_ROWS)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

        def device_only():
            _lib.check(_lib.lib.cgat_gp_kmeans_step(_ptr(X), X.stride(0), N, D, _ptr(ops["zimg"]), M, _ptr(ops["centroid"]),
                                                    _ptr(ops["znorm"]), gp.DEFAULT_CHUNK_ROWS, _ptr(assign), _ptr(counts),
                                                    _ptr(wss), _ptr(sums), _ptr(ws), ws_bytes, _stream()),
                       "cgat_gp_kmeans_step")

        times = _time_alternating({"fused": lambda: gp.kmeans_step(X, Z), "fused_device_only": device_only,
                                   "eager_fp32": lambda: eager(X)}, args.reps)
        fused, (a32, c32, w32, s32) = gp.kmeans_step(X, Z), eager(X)
        same = float((fused["assign"].long() == a32).double().mean())
        diff = {"wss": float((fused["wss"] - w32).abs().max() / w32.abs().max()),
                "sums": float((fused["sums"] - s32).abs().max() / s32.abs().max())}
        executed, needed = 4.0 * N * M * D, 2.0 * N * M * D + 1.0 * N * D
        Mp = (M + 31) // 32 * 32
        ms = times["fused_device_only"]["ms_median"]
        out[f"D{D}"] = {**times, "eager_over_fused": round(times["eager_fp32"]["ms_median"] / times["fused"]["ms_median"], 3),
                        "eager_over_fused_device_only": round(times["eager_fp32"]["ms_median"] / ms, 3),
                        "executed_matrix_tflop": round(executed / 1e12, 4), "needed_tflop": round(needed / 1e12, 4),
                        "fused_device_only_executed_tflops": round(executed / ms / 1e9, 2),
                        "fused_device_only_share_of_f32_matrix_peak": round(executed / ms / 1e9 / F32_MATRIX_PEAK_TF, 4),
                        "one_hot_gib_written_and_read": round(2.0 * 4.0 * Mp * N / 2 ** 30, 2),
                        "workspace_mib": round(ws_bytes / 2 ** 20, 1),
                        "counts_exact": bool(float(fused["counts"].sum()) == float(N)
                                             and torch.equal(fused["counts"], torch.bincount(fused["assign"].long(), minlength=M).double())),
                        "rows_assigned_alike": round(same, 6), "max_rel_diff_fused_vs_eager": diff}
        del X, eager, fused, ws, a32, c32, w32, s32
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
