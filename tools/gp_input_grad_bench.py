"""The gradient of the collapsed sparse-GP bound in the embeddings (cgat_gp_fit_grad_inputs: the data pass of
cgat_gp_fit_grad with gp_input_rows after gp_weight_rows, csrc/gpgrad.hip) at training size: N = 1 000 000
embeddings, M = 1000 inducing points, D = 384 and 640.  Three arms, alternated in one process, device events around each
call, warm-up; median / min / max:

    grad_pass           (a) the C entry cgat_gp_fit_grad alone on prepared operands (what tools/gp_grad_bench.py calls
                        grad_pass_device_only: unchanged code, to be compared with that tool's figure on the same box)
    grad_pass_inputs    (b) cgat_gp_fit_grad_inputs on the same operands: the same three sums and dX [N, D]
    eager_fp32          (c) an eager torch fp32 evaluation of the same three sums plus dX on the same box (the factors of
                        gp_grad_bench.EagerSums; the N x M matrices materialised chunk by chunk)

Beside the times: the FLOPs the product of (b) adds (2 N Mp Dq) and the rate that is of the added time, the sums of (b)
against those of (a) (bit-equal or not), and the largest difference between the fused and the eager dX relative to
max |dX|.  Writes one JSON object to --out and prints it.

    python tools/gp_input_grad_bench.py [--reps 5] [--rows 1000000] [--out profiles/gp_input_grad_bench.json]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gp_grad_bench import EagerSums  # noqa: E402
from gp_predict_bench import F32_MATRIX_PEAK_TF, _time_alternating  # noqa: E402


class EagerSumsAndInputs(EagerSums):
    """colsum, d2sum, P and dX in eager torch fp32 on the factors the fused pass uses."""

    def __call__(self, X, y, dX):
        M, D = self.Zc.shape
        colsum = torch.zeros(M, dtype=torch.float64, device=X.device)
        d2sum = torch.zeros(M, dtype=torch.float64, device=X.device)
        P = torch.zeros(M, D, dtype=torch.float64, device=X.device)
        inv_l2 = 2.0 * self.inv_two_l2
        for i in range(0, X.shape[0], self.chunk):
            xc = X[i:i + self.chunk] - self.cen
            d2 = torch.addmm(self.zn[None, :] + xc.square().sum(1, keepdim=True), xc, self.Zc.t(), alpha=-2.0).clamp_min_(0)
            kx = d2.mul(-self.inv_two_l2).exp_().mul_(self.s)
            q = torch.addmm(torch.outer(y[i:i + self.chunk] - self.c, self.g), kx @ self.W1t, self.G2)   # G2 is symmetric
            r = (q @ self.W1).mul_(kx)
            colsum += r.sum(0).double()
            d2sum += (r * d2).sum(0).double()
            P += (r.t() @ xc).double()
            torch.addmm(xc.mul(r.sum(1, keepdim=True)), r, self.Zc, beta=-inv_l2, alpha=inv_l2, out=dX[i:i + self.chunk])
        return colsum, d2sum, P, dX


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--inducing", type=int, default=1000)
    ap.add_argument("--widths", type=int, nargs="+", default=[384, 640])
    ap.add_argument("--chunk", type=int, default=65536, help="rows per chunk of the eager arm")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gp_input_grad_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gp_input_grad_bench: no GPU visible; times are measured on the device or not at all")
    from cgat_amd import _lib, gp
    from cgat_amd.ops import _ptr, _stream
    dev = "cuda:0"
    N, M, s, jitter = args.rows, args.inducing, 1.3, 1e-4
    out = {"tool": "gp_input_grad_bench", "device": torch.cuda.get_device_name(0), "N": N, "M": M, "reps": args.reps,
           "chunk_rows": gp.DEFAULT_CHUNK_ROWS, "eager_chunk_rows": args.chunk, "f32_matrix_peak_tf": F32_MATRIX_PEAK_TF}
    for D in args.widths:
        g = torch.Generator(dev).manual_seed(D)
        X = 0.5 + torch.randn(N, D, device=dev, generator=g)
        w = torch.randn(D, device=dev, generator=g) / math.sqrt(D)
        y = torch.sin(1.3 * ((X - 0.5) @ w)) + 0.3 * torch.randn(N, device=dev, generator=g)
        y = (y - y.mean()) / y.std()
        Z, ell = X[:M].cpu(), math.sqrt(D)
        both = gp._GradientPass("gp_input_grad_bench", X, y, Z, None)
        st = both.stats
        sol, _ = both(s, ell, jitter)
        adj = gp.collapsed_adjoints(st.gram, N, s, sol)
        two_G_hat, c = 2.0 * adj["G_hat"], sol["constant"]
        eager = EagerSumsAndInputs(Z, s, ell, jitter, two_G_hat, adj["g"], c, args.chunk, dev)
        ops, inv = st.ops, 0.5 / (ell * ell)
        st.factor(s, ell, jitter)
        w1img, w1timg, g2img = st.w1img, st.image(st.W1.T), st.image(two_G_hat)
        g32 = adj["g"].to(torch.float32).to(dev)
        ws_bytes = _lib.lib.cgat_gp_fit_grad_workspace_bytes(N, M, D, st.chunk)
        dX = torch.empty(N, D, device=dev)
        dX_eager = torch.empty(N, D, device=dev)
        common = (_ptr(X), X.stride(0), _ptr(st.y32), N, D, _ptr(ops["zimg"]), M, _ptr(ops["centroid"]), _ptr(ops["znorm"]),
                  _ptr(w1img), _ptr(w1timg), _ptr(g2img), _ptr(g32), c, s, inv, st.chunk, _ptr(both.colsum), _ptr(both.d2sum),
                  _ptr(both.P))

        def plain():
            _lib.check(_lib.lib.cgat_gp_fit_grad(*common, _ptr(st.ws), ws_bytes, _stream()), "cgat_gp_fit_grad")

        def with_inputs():
            _lib.check(_lib.lib.cgat_gp_fit_grad_inputs(*common, _ptr(ops["ztimg"]), _ptr(dX), dX.stride(0), _ptr(st.ws),
                                                        ws_bytes, _stream()), "cgat_gp_fit_grad_inputs")

        times = _time_alternating({"grad_pass": plain, "grad_pass_inputs": with_inputs,
                                   "eager_fp32": lambda: eager(X, y, dX_eager)}, args.reps)
        plain()
        sums_plain = [t.clone() for t in (both.colsum, both.d2sum, both.P)]
        with_inputs()
        sums_equal = all(torch.equal(a, b) for a, b in zip(sums_plain, (both.colsum, both.d2sum, both.P)))
        eager(X, y, dX_eager)
        diff = float((dX - dX_eager).abs().max() / dX_eager.abs().max())
        Mp, Dq = (M + 31) // 32 * 32, (D + 31) // 32 * 32
        added_flops = 2.0 * N * Mp * Dq
        added_ms = times["grad_pass_inputs"]["ms_median"] - times["grad_pass"]["ms_median"]
        out[f"D{D}"] = {**times,
                        "inputs_minus_plain_ms": round(added_ms, 3),
                        "eager_over_grad_pass_inputs": round(times["eager_fp32"]["ms_median"]
                                                             / times["grad_pass_inputs"]["ms_median"], 3),
                        "added_tflop": round(added_flops / 1e12, 4),
                        "added_product_tflops": round(added_flops / added_ms / 1e9, 2) if added_ms > 0 else None,
                        "dX_bytes_gib": round(N * D * 4 / 2 ** 30, 3),
                        "workspace_mib": round(max(ws_bytes, st.ws_bytes) / 2 ** 20, 1),
                        "sums_bitwise_equal_to_plain_entry": sums_equal,
                        "max_rel_diff_dX_fused_vs_eager": diff}
        del X, y, eager, both, st, dX, dX_eager, sums_plain
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
