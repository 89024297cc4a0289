"""One training-mode GATConvNodes layer with attention dropout (p = 0.1), forward + backward: the operand-split route
with the keep-mask pooling kernels (ops.set_fused_attention_dropout(True), the default) against the MessagePassing-style
route it replaces (switch off), alternated in one process and timed with HIP events, at the two 1M-edge shapes -- the
headline batch with H = 3 scalar attention and the harness-default batch with H = 5 vector attention.  Per route: the
step time of every round (their spread is the noise figure) and the peak allocation of one call.  Writes one JSON file.

    python tools/attn_dropout_bench.py [--reps 5] [--rounds 5] [--out profiles/attn_dropout_bench.json]

The two new kernels' own times come from a profiler run of their own,

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/attn_dropout_bench.py --only-profile
    python tools/attn_dropout_bench.py --kernel-stats DIR/.../*_kernel_stats.csv [--out ...]

the second call adding them, with their share of the 8 TB/s HBM peak on the bytes the shapes imply, to the JSON file.
"""
import argparse
import csv
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_BYTES_PER_S = 8.0e12
DROPOUT = 0.1
C = 128
# name, (crystals, atoms, neighbours), heads, vector attention
SHAPES = (("headline_h3_scalar", (4167, 20, 12), 3, False), ("harness_h5_vector", (2083, 20, 24), 5, True))


def kernel_bytes(N, E, H, vector):
    """What the two kernels cannot avoid moving (every operand once; the forward's second and third reading of the logits
    is left to the caches).  Forward reads logits, mask, keep_idx, messages and the row pointers and writes out, out_lo,
    mx and inv; backward reads all of those plus g_out and writes g_a and g_m."""
    aF, F = (H * C if vector else H), H * C
    a, m, idx, rp = 4 * E * aF, 4 * E * F, 4 * E, 4 * (N + 1)
    seg_f, seg_a = 4 * N * F, 4 * N * aF
    return {"forward": 2 * a + m + idx + rp + 2 * seg_f + 2 * seg_a,
            "backward": 2 * a + m + idx + rp + 3 * seg_f + 2 * seg_a + a + m}


def _setup(shape, H, vector):
    import cgat_amd as P
    dev = "cuda:0"
    b, _ = P.synthetic_batch(*shape, seed=0)
    g = torch.Generator().manual_seed(1)
    N, E = b.num_nodes, b.edge_index.shape[1]
    x = torch.randn(N, C, generator=g).to(dev).requires_grad_(True)
    e = torch.randn(E, C, generator=g).to(dev).requires_grad_(True)
    x0, cot = torch.randn(N, C, generator=g).to(dev), torch.randn(N, C, generator=g).to(dev)
    ei = b.edge_index.to(dev)
    torch.manual_seed(1)
    layer = P.GATConvNodes(C, C, C, H, concat=True, dropout=DROPOUT, vector_attention=vector).to(dev).train()

    def step():
        x.grad = e.grad = None
        for p in layer.parameters():
            p.grad = None
        layer(x, ei, e, x0).backward(cot)
    return step, N, E


def _ms(fn, reps):
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


def _peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def time_shape(name, shape, H, vector, reps, rounds):
    import cgat_amd as P
    step, N, E = _setup(shape, H, vector)
    routes = (("fused", True), ("switch_off", False))
    for _ in range(2):                                      # warm-up of both routes (code objects, allocator blocks)
        for _, on in routes:
            P.set_fused_attention_dropout(on)
            step()
    torch.cuda.synchronize()
    ms = {r: [] for r, _ in routes}
    for _ in range(rounds):                                 # alternated
        for r, on in routes:
            P.set_fused_attention_dropout(on)
            ms[r].append(_ms(step, reps))
    peak = {}
    for r, on in routes:
        P.set_fused_attention_dropout(on)
        peak[r] = round(_peak_mib(step), 1)
    P.set_fused_attention_dropout(True)
    mid = lambda v: sorted(v)[len(v) // 2]
    res = {"name": name, "crystals_atoms_neighbours": list(shape), "N": N, "E": E, "H": H, "vector_attention": vector,
           "dropout": DROPOUT, "reps": reps, "rounds": rounds}
    for r, _ in routes:
        res[r] = {"fwd_bwd_ms": round(mid(ms[r]), 3), "rounds_ms": [round(v, 3) for v in ms[r]],
                  "spread_ms": round(max(ms[r]) - min(ms[r]), 3), "peak_alloc_of_one_call_mib": peak[r]}
    res["speedup"] = round(res["switch_off"]["fwd_bwd_ms"] / res["fused"]["fwd_bwd_ms"], 3)
    res["gain_ms"] = round(res["switch_off"]["fwd_bwd_ms"] - res["fused"]["fwd_bwd_ms"], 3)
    res["accepted"] = bool(res["gain_ms"] > max(res["fused"]["spread_ms"], res["switch_off"]["spread_ms"]) and
                           peak["fused"] < peak["switch_off"])
    res["pool_kernel_bytes"] = kernel_bytes(N, E, H, vector)
    return res


def only_profile():
    """Three fused training steps per shape after one warm-up: the workload of the profiler run."""
    import cgat_amd as P
    P.set_fused_attention_dropout(True)
    for _, shape, H, vector in SHAPES:
        step, _, _ = _setup(shape, H, vector)
        for _ in range(4):
            step()
        torch.cuda.synchronize()


def add_kernel_stats(path, out_path):
    """Average times of the four instantiations from a rocprofv3 kernel-stats CSV; <false> is the scalar-attention shape
    (one logit per head), <true> the vector-attention one."""
    with open(out_path) as f:
        out = json.load(f)
    rows = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            for d in ("fwd", "bwd"):
                if f"seg_attnpool_drop_{d}_kernel<" in r["Name"]:
                    rows[(d, "<true>" in r["Name"])] = (int(r["Calls"]), float(r["AverageNs"]))
    for s in out["shapes"]:
        ks = {}
        for d, key in (("fwd", "forward"), ("bwd", "backward")):
            calls, ns = rows[(d, s["vector_attention"])]
            ks[f"seg_attnpool_drop_{d}"] = {"calls": calls, "average_us": round(ns / 1e3, 2),
                                            "frac_of_8TBps": round(s["pool_kernel_bytes"][key] / (ns * 1e-9) /
                                                                   HBM_PEAK_BYTES_PER_S, 4)}
        s["pool_kernels_rocprofv3"] = ks
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps([{s["name"]: s["pool_kernels_rocprofv3"]} for s in out["shapes"]]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_dropout_bench.json"))
    ap.add_argument("--only-profile", action="store_true", help="a few fused training steps per shape (for rocprofv3)")
    ap.add_argument("--kernel-stats", help="rocprofv3 kernel-stats CSV of an --only-profile run: add the kernels' times")
    args = ap.parse_args()
    if args.kernel_stats:
        return add_kernel_stats(args.kernel_stats, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("attn_dropout_bench.py needs an MI355X (cuda device); there is no CPU path to measure")
    if args.only_profile:
        return only_profile()
    import cgat_amd as P
    out = {"tool": "attn_dropout_bench", "device": torch.cuda.get_device_name(0), "mode": P.get_bilinear_mode(),
           "unit": "ms per forward + backward of one training-mode GATConvNodes layer (median over the rounds of the "
                   "median of `reps` calls, HIP events); spread = max - min over the rounds",
           "shapes": [time_shape(*s, args.reps, args.rounds) for s in SHAPES]}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
