"""The shell-indexed route of vector-attention node layers (cgat_amd.set_indexed_vector_attention) on against off,
alternated in one process: HIP events, warm-up, then medians of three samples of `--reps` calls each, with the spread
(min .. max of the samples' medians).  "off" is the parent route: the same IndexedEdgeAttr densified per layer.

  (a) one GATConvNodes(128, 128, 128, heads=5, vector_attention=True) layer, forward + backward, at 1 M edges (2 084
      crystals of 20 atoms, 24 neighbours), 240 000 edges (500 crystals) and 30 720 edges (64 crystals), with the CGAT_PROF
      tag times of one step
  (b) the harness-default network (CGAtNet(200, 128, 5, rezero, concat pooling, 24 neighbours, msg_heads=5, vector attention
      in both places) under set_indexed_edge_attr: training step (forward + backward) and eval forward, same sizes
  (c) the new launch alone (tag edge_idx_hidden of (a)): the bytes it has to move -- hidden stored, one Pj row gathered per
      slot, Pi once per atom, Te, the index arrays -- over its time
  (d) peak allocation of one step of (a)

Writes profiles/indexed_vector_bench.json (or --out) and prints the same JSON line.

    python tools/indexed_vector_bench.py [--reps 10] [--quick] [--out PATH]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/indexed_vector_bench.py --only-profile on|off
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
SIZES = (("1m", 2084), ("240k", 500), ("30k", 64))
TAGS = ("edge_idx_hidden", "edge_idx_class_sum", "edge_proj", "edge_z", "edge_ge", "edge_gw", "rows_ge", "rows_gw", "seg_wsum",
        "linear128")
HARNESS = dict(rezero=True, mean_pooling=False, neighbor_number=24, msg_heads=5, update_edges=True, vector_attention=True,
               global_vector_attention=True)


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


def _alternated(fn, reps, switch):
    """{'on': ..., 'off': ...}: median of three samples' medians and the spread, `switch(on)` before each sample."""
    for on in (True, False):
        switch(on)
        fn()
        fn()
    ms = {True: [], False: []}
    for _ in range(3):
        for on in (True, False):
            switch(on)
            ms[on].append(_median_ms(fn, reps))
    out = {}
    for on, name in ((True, "on"), (False, "off")):
        s = sorted(ms[on])
        out[name] = {"ms": round(s[1], 4), "min_ms": round(s[0], 4), "max_ms": round(s[2], 4)}
    out["on_over_off"] = round(out["on"]["ms"] / out["off"]["ms"], 4)
    return out


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
            out[t] = {"calls": n, "ms": round(ms, 4)}
    return out


def _peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def _layer(graphs):
    import cgat_amd as P
    b, _ = P.synthetic_batch(graphs, 20, 24, seed=0)
    g = torch.Generator().manual_seed(1)
    N, E = b.num_nodes, b.edge_index.shape[1]
    x = torch.randn(N, 128, generator=g).to(DEV).requires_grad_(True)
    x0 = torch.randn(N, 128, generator=g).to(DEV)
    table = torch.randn(25, 128, generator=g).to(DEV).requires_grad_(True)
    index = b.edge_attr.reshape(-1).long().to(DEV).clamp_(0, 24).contiguous()
    cot = torch.randn(N, 128, generator=g).to(DEV)
    ei = b.edge_index.to(DEV)
    torch.manual_seed(1)
    layer = P.GATConvNodes(128, 128, 128, heads=5, concat=True, vector_attention=True).to(DEV)
    leaves = [x, table] + list(layer.parameters())

    def step():
        y = layer(x, ei, P.IndexedEdgeAttr(table, index), x0)
        torch.autograd.grad((y * cot).sum(), leaves)
    return step, N, E


def layer_case(graphs, reps):
    import cgat_amd as P
    step, N, E = _layer(graphs)
    res = {"crystals": graphs, "N": N, "E": E, "H": 5, "K": 24, "R": 25}
    res["fwd_bwd"] = _alternated(step, reps, P.set_indexed_vector_attention)
    for on, name in ((True, "on"), (False, "off")):
        P.set_indexed_vector_attention(on)
        res["tags_" + name] = _tags(step)
        res["peak_alloc_bytes_" + name] = _peak(step)
    P.set_indexed_vector_attention(False)
    W2 = 2 * 5 * 256
    t = res["tags_on"].get("edge_idx_hidden")
    if t:
        nbytes = 4 * W2 * (2 * E + N + 25) + E * (8 + 4 + 4 + 4)
        res["edge_idx_hidden"] = {"bytes": nbytes, "ms": t["ms"], "GB_per_s": round(nbytes / t["ms"] / 1e6, 1)}
    return res


def _net(graphs):
    import cgat_amd as P
    b, roost = P.synthetic_batch(graphs, 20, 24, seed=0)
    b = b.to(DEV)
    roost = tuple(t.to(DEV) for t in roost)
    torch.manual_seed(1)
    net = P.CGAtNet(200, 128, 5, **HARNESS).to(DEV)
    return net, b, roost


def net_case(graphs, reps):
    import cgat_amd as P
    net, b, roost = _net(graphs)
    params = [p for p in net.parameters() if p.requires_grad]
    res = {"crystals": graphs, "E": int(b.edge_index.shape[1])}

    def train_step():
        y = net(b, roost)
        torch.autograd.grad(y.square().sum(), params, allow_unused=True)

    def eval_fwd():
        with torch.no_grad():
            net(b, roost)
    P.set_indexed_edge_attr(True)
    try:
        net.train()
        res["train_step"] = _alternated(train_step, reps, P.set_indexed_vector_attention)
        for on, name in ((True, "on"), (False, "off")):
            P.set_indexed_vector_attention(on)
            res["train_tags_" + name] = _tags(train_step)
        net.eval()
        res["eval_fwd"] = _alternated(eval_fwd, reps, P.set_indexed_vector_attention)
    finally:
        P.set_indexed_vector_attention(False)
        P.set_indexed_edge_attr(False)
    return res


def only_profile(which):
    """Three training steps of the harness-default network at 1 M edges with the switch `which` (for rocprofv3)."""
    import cgat_amd as P
    net, b, roost = _net(2084)
    params = [p for p in net.parameters() if p.requires_grad]
    P.set_indexed_edge_attr(True)
    P.set_indexed_vector_attention(which == "on")
    net.train()
    for _ in range(3):
        y = net(b, roost)
        torch.autograd.grad(y.square().sum(), params, allow_unused=True)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="the 30 720-edge size only")
    ap.add_argument("--only-profile", choices=("on", "off"), help="a few (b) training steps at 1 M edges (for rocprofv3)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "indexed_vector_bench.json"))
    args = ap.parse_args()
    import cgat_amd as P
    if args.only_profile:
        return only_profile(args.only_profile)
    out = {"tool": "indexed_vector_bench", "mode": P.get_bilinear_mode(), "device": torch.cuda.get_device_name(0),
           "reps": args.reps, "layer": {}, "net": {}}
    for name, graphs in SIZES:
        if args.quick and name != "30k":
            continue
        out["layer"][name] = layer_case(graphs, args.reps)
        torch.cuda.empty_cache()
        out["net"][name] = net_case(graphs, args.reps)
        torch.cuda.empty_cache()
    line = json.dumps(out)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
