"""The head combination of GATConvEdges(no_hyper=False) alone: ops.EdgeHeadCombineFn (csrc/edgecomb.hip) against the
sequence of torch ops it replaces, forward + backward, alternated in one process and timed with HIP events, at the two
1M-edge shapes of the edge update (H = 3 scalar attention, H = 5 vector attention, Co = 128); the achieved fraction of
the HBM peak on the bytes the op cannot avoid; and the op-level error figures of tests/test_edge_head_combine.py
(fused and torch sequence against fp64, per case).  Writes one JSON file.

    python tools/edge_combine_bench.py [--reps 10] [--rounds 5] [--out profiles/edge_combine_bench.json] [--no-errors]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_BYTES_PER_S = 8.0e12
SHAPES = ((1000080, 3, 1, 128), (1000080, 5, 128, 128))          # (E, H, aF, Co)


def compulsory_bytes(E, H, aF, Co):
    """Forward reads sa, sm and perm and writes out; backward reads sa, sm, perm and g_out and writes g_sa and g_sm."""
    sa, sm, out, perm = 4 * E * H * aF, 4 * E * H * Co, 4 * E * Co, 4 * E
    return {"forward": sa + sm + perm + out, "backward": 2 * sa + 2 * sm + perm + out}


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def time_shape(E, H, aF, Co, reps, rounds):
    from cgat_amd import ops
    from test_edge_head_combine import eager_combine
    dev = "cuda:0"
    g = torch.Generator().manual_seed(11)
    sa = (2.0 * torch.randn(E, H, aF, generator=g)).to(dev).requires_grad_(True)
    sm = torch.randn(E, H, Co, generator=g).to(dev).requires_grad_(True)
    cot = torch.randn(E, Co, generator=g).to(dev)
    perm = torch.randperm(E, generator=g).to(torch.int32).to(dev)

    def step(fn):
        sa.grad = sm.grad = None
        fn(sa, sm, None, perm).backward(cot)
    fused = lambda: step(ops.EdgeHeadCombineFn.apply)
    eager = lambda: step(eager_combine)
    for fn in (fused, eager, fused, eager):                 # warm-up of both (code objects, allocator blocks)
        fn()
    torch.cuda.synchronize()
    ms = {"fused": [], "eager": []}
    for _ in range(rounds):                                 # alternated
        ms["fused"].append(_median_ms(fused, reps))
        ms["eager"].append(_median_ms(eager, reps))
    # the two launches alone (events on the launch stream around each kernel)
    ops.prof_reset()
    ops.prof_enable(True)
    for _ in range(reps):
        fused()
    torch.cuda.synchronize()
    ops.prof_enable(False)
    n, kernel_ms = ops.prof_get("edge_combine")
    ops.prof_reset()
    kernel_ms = kernel_ms / (n / 2)
    by = compulsory_bytes(E, H, aF, Co)
    total = by["forward"] + by["backward"]
    mid = lambda v: sorted(v)[len(v) // 2]
    res = {"E": E, "H": H, "aF": aF, "Co": Co, "reps": reps, "rounds": rounds,
           "fused_fwd_bwd_ms": round(mid(ms["fused"]), 4), "eager_fwd_bwd_ms": round(mid(ms["eager"]), 4),
           "fused_rounds_ms": [round(v, 4) for v in ms["fused"]], "eager_rounds_ms": [round(v, 4) for v in ms["eager"]],
           "fused_kernels_ms": round(kernel_ms, 4), "compulsory_bytes": by,
           "frac_of_8TBps_fwd_bwd_call": round(total / (mid(ms["fused"]) * 1e-3) / HBM_PEAK_BYTES_PER_S, 4),
           "frac_of_8TBps_kernels": round(total / (kernel_ms * 1e-3) / HBM_PEAK_BYTES_PER_S, 4)}
    res["speedup"] = round(res["eager_fwd_bwd_ms"] / res["fused_fwd_bwd_ms"], 3)
    return res


def error_figures():
    import test_edge_head_combine as T
    rows = []
    for E in T.E_SIZES:
        for H, aF, Co in T.SHAPES:
            for with_perm in (False, True):
                for with_keep in (False, True):
                    r = T.op_errors(E, H, aF, Co, with_perm, with_keep)
                    rows.append({"E": E, "H": H, "aF": aF, "Co": Co, "perm": with_perm, "keep": with_keep,
                                 "fused": r["fused"], "eager": r["eager"]})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_combine_bench.json"))
    ap.add_argument("--no-errors", action="store_true", help="timings only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edge_combine_bench.py needs an MI355X (cuda device); there is no CPU path to measure")
    out = {"tool": "edge_combine_bench", "device": torch.cuda.get_device_name(0),
           "unit": "ms per forward + backward of the op alone (median of medians, HIP events)",
           "shapes": [time_shape(*s, args.reps, args.rounds) for s in SHAPES]}
    if not args.no_errors:
        out["errors_vs_fp64"] = {"metric": "max-norm relative error against the torch expression in fp64, per tensor",
                                 "bound": "fused <= 2 x eager (tests/test_edge_head_combine.py)", "cases": error_figures()}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k != "errors_vs_fp64"}))


if __name__ == "__main__":
    main()
