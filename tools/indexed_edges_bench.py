"""Shell-indexed edge features (cgat_amd.set_indexed_edge_attr) on against off, alternated in one process, HIP events,
warm-up then `--reps` repetitions per sample, median and spread (min .. max of the samples' medians):

  (a) eval forward of CGAtNet(200, 128, 4, msg_heads=3) under no_grad at 1 M edges (4 167 crystals), 240 000 edges
      (1 000 crystals) and 64 crystals
  (b) the same for the harness-default network (vector attention: only the edge update collapses), 24 neighbours
  (c) one layer's per-edge phase by CGAT_PROF tag: edge_idx_logits + edge_idx_wsum against edge_logits + edge_msg_wsum
      (the layer called with an IndexedEdgeAttr and with the dense rows), with the bytes each indexed launch gathers
  (d) the 4-layer training step (forward + backward), on against off
  (e) peak allocation of one call of (a)

With --train-route, the training route (cgat_amd.set_indexed_edge_training) instead, three columns alternated in one
process: "indexed" (the route on), "densified" (the lookup densified per layer, as without the switch) and "dense" (a dense
edge_attr tensor / set_indexed_edge_attr off):

  (f) one layer forward + backward at 1 M edges, H = 3
  (g) the 4-layer training step at 1 M edges, 240 000 edges and 64 crystals
  (h) peak allocation of (g) at 1 M edges
  (i) per-kernel times of the new launches by CGAT_PROF tag next to edge_z, seg_wsum, edge_seg_bwd, edge_ge, edge_gw

Writes profiles/indexed_edges_bench.json (profiles/indexed_train_bench.json with --train-route; or --out) and prints the
same JSON line.

    python tools/indexed_edges_bench.py [--reps 10] [--quick] [--train-route] [--out PATH]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
TAGS = ("edge_idx_logits", "edge_idx_wsum", "edge_logits", "edge_msg_wsum", "seg_softmax", "edge_proj", "edge_ge",
        "linear128", "rowprog")


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


def _alternate(fn, reps, samples=3):
    """{on/off: {"median_ms", "min_ms", "max_ms"}} over `samples` alternated samples of `reps` timed calls each."""
    import cgat_amd as P
    ms = {True: [], False: []}
    try:
        for on in (True, False):                 # warm-up of both (plans, workspaces, index validation)
            P.set_indexed_edge_attr(on)
            fn()
            fn()
        for _ in range(samples):
            for on in (True, False):
                P.set_indexed_edge_attr(on)
                ms[on].append(_median_ms(fn, reps))
    finally:
        P.set_indexed_edge_attr(False)
    out = {}
    for on, name in ((True, "on"), (False, "off")):
        v = sorted(ms[on])
        out[name] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4)}
    out["on_over_off"] = round(out["on"]["median_ms"] / out["off"]["median_ms"], 4)
    return out


def _tags(fn):
    from cgat_amd import ops
    ops.prof_reset()
    ops.prof_enable(True)
    n0 = ops.prof_launches()
    fn()
    torch.cuda.synchronize()
    ops.prof_enable(False)
    out = {"launches": ops.prof_launches() - n0}
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


def _net(harness):
    import cgat_amd as P
    torch.manual_seed(1)
    if harness:
        return P.CGAtNet(200, 128, 5, rezero=True, mean_pooling=False, neighbor_number=24, msg_heads=5, update_edges=True,
                         vector_attention=True, global_vector_attention=True).to(DEV)
    return P.CGAtNet(200, 128, 4, msg_heads=3, neighbor_number=12, update_edges=True).to(DEV)


def _batch(crystals, K):
    import cgat_amd as P
    b, roost = P.synthetic_batch(crystals, 20, K, seed=0)
    return b.to(DEV), tuple(t.to(DEV) for t in roost)


def eval_case(crystals, reps, harness=False, peak=False):
    import cgat_amd as P
    K = 24 if harness else 12
    b, roost = _batch(crystals, K)
    net = _net(harness).eval()
    res = {"crystals": crystals, "N": b.num_nodes, "E": int(b.edge_index.shape[1]), "K": K}
    with torch.no_grad():
        fn = lambda: net(b, roost)
        res["eval_fwd"] = _alternate(fn, reps)
        for on, name in ((True, "on"), (False, "off")):
            P.set_indexed_edge_attr(on)
            res[name + "_tags_ms"] = _tags(fn)
            if peak:
                res[name + "_peak_alloc_bytes"] = _peak(fn)
        P.set_indexed_edge_attr(False)
    return res


def layer_case(crystals, reps, H=3, K=12):
    """(c): the node layer given an IndexedEdgeAttr against the same layer given the dense rows, by tag."""
    import cgat_amd as P
    b, _ = P.synthetic_batch(crystals, 20, K, seed=0)
    g = torch.Generator().manual_seed(1)
    N, E = b.num_nodes, b.edge_index.shape[1]
    x, x0 = torch.randn(N, 128, generator=g).to(DEV), torch.randn(N, 128, generator=g).to(DEV)
    table = torch.randn(K + 1, 128, generator=g).to(DEV)
    ea = P.IndexedEdgeAttr(table, b.edge_attr.to(DEV))
    ei = b.edge_index.to(DEV)
    torch.manual_seed(1)
    layer = P.GATConvNodes(128, 128, 128, H, concat=True).to(DEV)
    HHd = H * layer.MH_A.hidden_layer_dim
    res = {"crystals": crystals, "N": N, "E": E, "H": H, "K": K, "R": K + 1}
    with torch.no_grad():
        dense = ea.dense()
        f_on, f_off = (lambda: layer(x, ei, ea, x0)), (lambda: layer(x, ei, dense, x0))
        for f in (f_on, f_off, f_on, f_off):
            f()
        on, off = [], []
        for _ in range(3):
            on.append(_median_ms(f_on, reps))
            off.append(_median_ms(f_off, reps))
        res["layer_fwd_ms"] = {"indexed": round(sorted(on)[1], 4), "dense": round(sorted(off)[1], 4),
                               "indexed_min_max": [round(min(on), 4), round(max(on), 4)],
                               "dense_min_max": [round(min(off), 4), round(max(off), 4)]}
        t_on, t_off = [_tags(f_on) for _ in range(3)][-1], [_tags(f_off) for _ in range(3)][-1]
    res["indexed_tags_ms"], res["dense_tags_ms"] = t_on, t_off
    res["per_edge_phase_ms"] = {
        "indexed": round(t_on.get("edge_idx_logits", 0) + t_on.get("edge_idx_wsum", 0), 4),
        "dense": round(t_off.get("edge_logits", 0) + t_off.get("edge_msg_wsum", 0), 4)}
    # what each indexed launch gathers: per slot one half row of Pj and of Te (4 H Hd bytes each), per node one half row of Pi;
    # the logits write and the weighted sum reads 4 H bytes per slot, the weighted sum writes 4 H Hd per node
    half = 4 * HHd
    byt = {"edge_idx_logits": E * (2 * half + 4 * H + 12) + N * half,
           "edge_idx_wsum": E * (2 * half + 4 * H + 12) + 2 * N * half}
    res["gathered_bytes"] = byt
    res["gather_TB_per_s"] = {k: round(byt[k] / (t_on[k] * 1e-3) / 1e12, 3) for k in byt if t_on.get(k)}
    res["pj_from_memory_TB_per_s"] = {k: round(E * half / (t_on[k] * 1e-3) / 1e12, 3) for k in byt if t_on.get(k)}
    return res


def train_case(crystals, reps):
    """(d): forward + backward of the 4-layer network in train mode (no optimiser step), switch on against off."""
    b, roost = _batch(crystals, 12)
    net = _net(False).train()
    cot = torch.randn(crystals, 2, generator=torch.Generator().manual_seed(2)).to(DEV)

    def step():
        for p in net.parameters():
            p.grad = None
        (net(b, roost) * cot).sum().backward()
    return {"crystals": crystals, "E": int(b.edge_index.shape[1]), "train_step": _alternate(step, reps)}


TRAIN_TAGS = ("edge_idx_logits", "edge_idx_wsum", "edge_idx_bwd_msg", "edge_idx_bwd_soft", "edge_idx_bwd_att", "edge_gj",
              "edge_idx_class_sum", "edge_z", "seg_wsum", "edge_seg_bwd", "edge_ge", "edge_gw")


def _alternate3(fns, reps, samples=3):
    """{column: {"median_ms", "min_ms", "max_ms", "spread_ms"}} for {column: callable}, the columns alternated."""
    ms = {k: [] for k in fns}
    for f in fns.values():
        f()
        f()
    for _ in range(samples):
        for k, f in fns.items():
            ms[k].append(_median_ms(f, reps))
    out = {}
    for k, v in ms.items():
        v = sorted(v)
        out[k] = {"median_ms": round(v[len(v) // 2], 4), "min_ms": round(v[0], 4), "max_ms": round(v[-1], 4),
                  "spread_ms": round(v[-1] - v[0], 4)}
    return out


def _train_tags(fn):
    from cgat_amd import ops
    ops.prof_reset()
    ops.prof_enable(True)
    fn()
    torch.cuda.synchronize()
    ops.prof_enable(False)
    out = {}
    for t in TRAIN_TAGS:
        n, ms = ops.prof_get(t)
        if n:
            out[t] = {"launches": n, "ms": round(ms, 4)}
    return out


class _switches:
    def __init__(self, attr, train):
        self.v = (attr, train)

    def __enter__(self):
        import cgat_amd as P
        self.prev = (P.get_indexed_edge_attr(), P.get_indexed_edge_training())
        P.set_indexed_edge_attr(self.v[0])
        P.set_indexed_edge_training(self.v[1])

    def __exit__(self, *a):
        import cgat_amd as P
        P.set_indexed_edge_attr(self.prev[0])
        P.set_indexed_edge_training(self.prev[1])


def train_layer_case(crystals, reps, H=3, K=12):
    """(f), (i): one node layer forward + backward on the same lookup, three ways."""
    import cgat_amd as P
    b, _ = P.synthetic_batch(crystals, 20, K, seed=0)
    g = torch.Generator().manual_seed(1)
    N, E = b.num_nodes, b.edge_index.shape[1]
    x, x0 = torch.randn(N, 128, generator=g).to(DEV).requires_grad_(True), torch.randn(N, 128, generator=g).to(DEV)
    cot = torch.randn(N, 128, generator=g).to(DEV)
    table = torch.randn(K + 1, 128, generator=g).to(DEV).requires_grad_(True)
    index, ei = b.edge_attr.to(DEV), b.edge_index.to(DEV)
    dense = table.detach()[index].clone().requires_grad_(True)
    torch.manual_seed(1)
    layer = P.GATConvNodes(128, 128, 128, H, concat=True).to(DEV)
    leaves = [x, table] + list(layer.parameters())

    def run(ea, train):
        def f():
            with _switches(False, train):
                y = layer(x, ei, ea() if callable(ea) else ea, x0)
                torch.autograd.grad((y * cot).sum(), leaves + ([dense] if ea is dense else []), allow_unused=True)
        return f
    fns = {"indexed": run(lambda: P.IndexedEdgeAttr(table, index), True),
           "densified": run(lambda: P.IndexedEdgeAttr(table, index), False), "dense": run(dense, False)}
    res = {"crystals": crystals, "N": N, "E": E, "H": H, "R": K + 1, "layer_fwd_bwd": _alternate3(fns, reps)}
    res["tags"] = {k: _train_tags(f) for k, f in fns.items()}
    res["peak_alloc_bytes"] = {k: _peak(f) for k, f in fns.items()}
    return res


def train_net_case(crystals, reps, peak=False):
    """(g), (h): forward + backward of the 4-layer network in train mode (no optimiser step)."""
    b, roost = _batch(crystals, 12)
    net = _net(False).train()
    cot = torch.randn(crystals, 2, generator=torch.Generator().manual_seed(2)).to(DEV)

    def run(attr, train):
        def f():
            with _switches(attr, train):
                for p in net.parameters():
                    p.grad = None
                (net(b, roost) * cot).sum().backward()
        return f
    fns = {"indexed": run(True, True), "densified": run(True, False), "dense": run(False, False)}
    res = {"crystals": crystals, "E": int(b.edge_index.shape[1]), "train_step": _alternate3(fns, reps)}
    if peak:
        res["peak_alloc_bytes"] = {k: _peak(f) for k, f in fns.items()}
        res["tags"] = {k: _train_tags(f) for k, f in fns.items()}
    return res


def train_route_main(args, reps):
    import cgat_amd as P
    out = {"tool": "indexed_edges_bench --train-route", "mode": P.get_bilinear_mode(),
           "device": torch.cuda.get_device_name(0), "reps": reps, "samples": 3}
    big = 1000 if args.quick else 4167
    out["f_i_layer"] = {str(big): train_layer_case(big, reps)}
    torch.cuda.empty_cache()
    out["g_h_train"] = {}
    for c in ((1000, 64) if args.quick else (4167, 1000, 64)):
        out["g_h_train"][str(c)] = train_net_case(c, reps, peak=c == big)
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--quick", action="store_true", help="64 and 1 000 crystals only (a rehearsal of the tool)")
    ap.add_argument("--train-route", action="store_true", help="rows (f)-(i): the training route, three columns")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "indexed_train_bench.json" if args.train_route else "indexed_edges_bench.json")
    if not torch.cuda.is_available():
        sys.exit("indexed_edges_bench: needs an MI355X; nothing is measured without one")
    import cgat_amd as P
    reps = max(10, args.reps)
    sizes = (64, 1000) if args.quick else (4167, 1000, 64)
    if args.train_route:
        out = train_route_main(args, reps)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print(json.dumps(out))
        return
    out = {"tool": "indexed_edges_bench", "mode": P.get_bilinear_mode(), "device": torch.cuda.get_device_name(0),
           "reps": reps, "samples": 3}
    out["a_eval_scalar"] = {str(c): eval_case(c, reps, peak=True) for c in sizes}
    torch.cuda.empty_cache()
    out["b_eval_harness_default"] = {str(c): eval_case(c, reps, harness=True)
                                     for c in ((64, 500) if args.quick else (2084, 500, 64))}
    torch.cuda.empty_cache()
    out["c_layer"] = {str(c): layer_case(c, reps) for c in sizes}
    out["c_layer_h5_k24"] = {str(c): layer_case(c, reps, H=5, K=24) for c in ((64,) if args.quick else (2084, 64))}
    torch.cuda.empty_cache()
    out["d_train"] = {str(c): train_case(c, reps) for c in ((64,) if args.quick else (4167, 64))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
