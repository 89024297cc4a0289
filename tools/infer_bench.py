"""The forward without grad of the scalar-attention node layer against its opt-out (the training forward under no_grad),
alternated in one process: layer forward ms, CGAT_PROF tag times and the peak allocation of one call, at BASELINE
configs[1] (1 000 crystals, E = 240 000) and at the 1M-edge batch (4 167 crystals, E = 1 000 080), plus the
CGAtNet(200, 128, 4, msg_heads=3) eval forward on the 1M-edge batch; and the layer of the harness' scalar-attention
network (msg_heads = 5, 24 neighbours) at 64 crystals (E = 30 720), 1 000 crystals (E = 480 000) and the 1M-edge batch
at 24 neighbours (2 084 crystals, E = 1 000 320).  Prints one JSON line.

    python tools/infer_bench.py [--reps 10] [--h5-only]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAGS = ("edge_proj", "edge_logits", "seg_softmax", "edge_msg_wsum", "edge_z", "seg_wsum", "edge_ge", "linear128")


def _time(fn, reps):
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


def _tags(fn):
    from cgat_amd import ops
    ops.prof_reset()
    ops.prof_enable(True)
    fn()
    torch.cuda.synchronize()
    ops.prof_enable(False)
    out = {}
    for t in TAGS:
        n, ms = ops.prof_get(t)
        if n:
            out[t] = round(ms, 4)
    return out


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def layer_case(graphs, reps, H=3, K=12):
    import cgat_amd as P
    dev = "cuda:0"
    b, _ = P.synthetic_batch(graphs, 20, K, seed=0)
    g = torch.Generator().manual_seed(1)
    N, E = b.num_nodes, b.edge_index.shape[1]
    x, x0 = torch.randn(N, 128, generator=g).to(dev), torch.randn(N, 128, generator=g).to(dev)
    e = torch.randn(E, 128, generator=g).to(dev)
    ei = b.edge_index.to(dev)
    torch.manual_seed(1)
    layer = P.GATConvNodes(128, 128, 128, H, concat=True).to(dev)
    fn = lambda: layer(x, ei, e, x0)
    res = {"crystals": graphs, "N": N, "E": E, "H": H, "K": K}
    with torch.no_grad():
        for on in (True, False):             # warm-up of both routes (plans, workspaces)
            P.set_fused_inference(on)
            fn()
        ms = {True: [], False: []}
        for _ in range(3):                   # alternated
            for on in (True, False):
                P.set_fused_inference(on)
                ms[on].append(_time(fn, reps))
        for on, name in ((True, "infer"), (False, "opt_out")):
            P.set_fused_inference(on)
            res[name] = {"layer_fwd_ms": round(sorted(ms[on])[1], 4), "tags_ms": _tags(fn), "peak_alloc_bytes": _peak(fn)}
            fn()                              # the workspace of the other route is already there: peak of the call alone
    P.set_fused_inference(True)
    t = res["infer"]["tags_ms"]
    res["edge_logits+edge_msg_wsum+seg_softmax_ms"] = round(t.get("edge_logits", 0) + t.get("edge_msg_wsum", 0) +
                                                            t.get("seg_softmax", 0), 4)
    o = res["opt_out"]["tags_ms"]
    res["opt_out_edge_z+seg_wsum+seg_softmax_ms"] = round(o.get("edge_z", 0) + o.get("seg_wsum", 0) + o.get("seg_softmax", 0), 4)
    res["peak_alloc_saved_bytes"] = res["opt_out"]["peak_alloc_bytes"] - res["infer"]["peak_alloc_bytes"]
    return res


def net_case(graphs, reps):
    import cgat_amd as P
    dev = "cuda:0"
    b, roost = P.synthetic_batch(graphs, 20, 12, seed=0)
    b = b.to(dev)
    roost = tuple(t.to(dev) for t in roost)
    torch.manual_seed(1)
    net = P.CGAtNet(200, 128, 4, msg_heads=3, neighbor_number=12, update_edges=True).to(dev).eval()
    fn = lambda: net(b, roost)
    res = {"crystals": graphs, "E": int(b.edge_index.shape[1])}
    with torch.no_grad():
        for on in (True, False):
            P.set_fused_inference(on)
            fn()
        ms = {True: [], False: []}
        for _ in range(3):
            for on in (True, False):
                P.set_fused_inference(on)
                ms[on].append(_time(fn, reps))
    P.set_fused_inference(True)
    res["eval_fwd_ms"] = {"infer": round(sorted(ms[True])[1], 4), "opt_out": round(sorted(ms[False])[1], 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only-profile", action="store_true", help="a few inference-route layer forwards (for rocprofv3)")
    ap.add_argument("--h5-only", action="store_true", help="only the layer of the harness' scalar network (H = 5, K = 24)")
    args = ap.parse_args()
    import cgat_amd as P
    if args.only_profile:
        dev = "cuda:0"
        b, _ = P.synthetic_batch(4167, 20, 12, seed=0)
        g = torch.Generator().manual_seed(1)
        N, E = b.num_nodes, b.edge_index.shape[1]
        x, x0, e = torch.randn(N, 128, generator=g).to(dev), torch.randn(N, 128, generator=g).to(dev), \
            torch.randn(E, 128, generator=g).to(dev)
        ei = b.edge_index.to(dev)
        layer = P.GATConvNodes(128, 128, 128, 3, concat=True).to(dev)
        with torch.no_grad():
            for _ in range(6):
                layer(x, ei, e, x0)
        torch.cuda.synchronize()
        return
    out = {"tool": "infer_bench", "mode": P.get_bilinear_mode(), "device": torch.cuda.get_device_name(0)}
    if not args.h5_only:
        out.update({"baseline_configs1": layer_case(1000, args.reps), "batch_1m": layer_case(4167, args.reps),
                    "net_1m": net_case(4167, max(3, args.reps // 2))})
    out.update({"h5_k24_64": layer_case(64, args.reps, H=5, K=24), "h5_k24_1000": layer_case(1000, args.reps, H=5, K=24),
                "h5_k24_1m": layer_case(2084, args.reps, H=5, K=24)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
