"""From structures to a ready `PackedDataset` at the benchmark's size: 4 167 synthetic crystals of 20 atoms (the structures
of tools/neighbor_bench.py), K = 12 and 24 stored = packed columns.  Four builds on the host clock, each ending in a
synchronise, alternating in one process after a warm-up:

    from_structures            the dictionary and `from_dict`'s per-crystal loop (the route before csrc/pack.hip)
    from_structures_device     the same parse, then `from_tables`
    from_arrays_numpy          flat numpy arrays and a flat list of symbols
    from_arrays_device         device tensors and integer element rows

and, for attribution, the stages of the numpy build one by one (symbols to rows, upload, neighbour tables, `from_tables`),
each closed by a synchronise, the plan + write launches of csrc/pack.hip alone between device events, and the eval
forward's crystals/s on the same batch size (tools/infer_bench.py), the rate packing has to exceed.  Every figure
is a median with (min - max) over --reps repetitions; crystals/s are input crystals over the median.  Writes one JSON
object to --out and prints it.

    python tools/pack_bench.py [--reps 9] [--crystals 4167] [--out profiles/pack_bench.json]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _stat(ts, G=None):
    ts = sorted(ts)
    out = {"ms_median": round(ts[len(ts) // 2] * 1e3, 3), "ms_min": round(ts[0] * 1e3, 3), "ms_max": round(ts[-1] * 1e3, 3)}
    if G is not None:
        out["crystals_per_s"] = round(G / ts[len(ts) // 2], 1)
    return out


def _clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def _launches_ms(P, tabs, ptr, elem, tgt, K, n_elem, reps):
    """plan + write of csrc/pack.hip alone: outputs allocated beforehand from a first plan, device events around the two calls"""
    from cgat_amd import _lib
    G, (N, Ks), dev = ptr.shape[0] - 1, tabs.shell.shape, ptr.device
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    ws = torch.empty(_lib.lib.cgat_pack_dataset_workspace_bytes(G, N), dtype=torch.uint8, device=dev)
    totals = torch.empty(4, **i32)
    stream = torch.cuda.current_stream().cuda_stream
    plan = lambda: _lib.check(_lib.lib.cgat_pack_dataset_plan(ptr.data_ptr(), elem.data_ptr(), tabs.status.data_ptr(), G, N,
                                                              n_elem, totals.data_ptr(), ws.data_ptr(), ws.numel(), stream),
                              "cgat_pack_dataset_plan")
    plan()
    Gk, Nk, Uk, bad = totals.cpu().tolist()
    assert bad == 0
    outs = [torch.empty(Gk + 1, **i32), torch.empty(Nk, **i32), torch.empty(Nk, K, **i32), torch.empty(Nk, K, **i32),
            torch.empty(Nk, K, **i32), torch.empty(Gk + 1, **i32), torch.empty(Uk, **i32), torch.empty(Uk, **f32),
            torch.empty(Gk, **f32), torch.empty(Gk, **i32)]
    write = lambda: _lib.check(_lib.lib.cgat_pack_dataset_write(
        ptr.data_ptr(), elem.data_ptr(), tabs.shell.data_ptr(), tabs.self_idx.data_ptr(), tabs.nbr_idx.data_ptr(),
        tabs.status.data_ptr(), tgt.data_ptr(), G, N, Ks, K, n_elem, 0, totals.data_ptr(), ws.data_ptr(), ws.numel(), Gk, Nk,
        Uk, *[t.data_ptr() for t in outs], stream), "cgat_pack_dataset_write")
    ts = []
    for k in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        plan()
        write()
        b.record()
        torch.cuda.synchronize()
        if k >= 3:
            ts.append(a.elapsed_time(b) * 1e-3)
    moved = 4 * (3 * N * K * 2 + 3 * N + 2 * Nk + 3 * Uk) + 8 * G       # table rows in and out, ids read by both phases
    return dict(_stat(ts, G), bytes_moved=int(moved), kept=Gk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--crystals", type=int, default=4167)
    ap.add_argument("--atoms", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pack_bench.json"))
    ap.add_argument("--no-forward", action="store_true", help="skip the eval forward of tools/infer_bench.py")
    args = ap.parse_args()
    if args.reps < 7:
        raise SystemExit("pack_bench: at least 7 repetitions")
    import cgat_amd as P
    from cgat_amd.collate import _symbol_rows
    from cgat_amd.graph import ELEMENT_SYMBOLS
    from neighbor_bench import _embedding
    if not torch.cuda.is_available():
        raise SystemExit("pack_bench: no GPU visible; rates are measured on the device or not at all")
    warnings.simplefilter("ignore")
    dev = "cuda:0"
    emb = _embedding()
    structures = P.synthetic_structures(args.crystals, 0, atoms=args.atoms)
    G = len(structures)
    targets = {"e_above_hull": np.linspace(-1.0, 2.0, G)}
    lat = np.stack([s[0] for s in structures])
    frac = np.concatenate([s[1] for s in structures])
    ptr = np.zeros(G + 1, np.int32)
    ptr[1:] = np.cumsum([len(s[2]) for s in structures])
    syms = [el for s in structures for el in s[2]]
    rows = _symbol_rows(syms, list(ELEMENT_SYMBOLS))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_lat, d_frac, d_ptr, d_rows, d_tgt = up(lat), up(frac), up(ptr), up(rows), up(targets["e_above_hull"])
    out = {"tool": "pack_bench", "device": torch.cuda.get_device_name(0), "crystals": G, "atoms": int(ptr[-1]),
           "reps": args.reps, "radius": 18.0}
    for K in (12, 24):
        kw = dict(max_neighbor_number=K, stored_neighbors=K, device=dev)
        arms = {"from_structures": lambda: P.PackedDataset.from_structures(structures, targets, emb, **kw),
                "from_structures_device": lambda: P.PackedDataset.from_structures(structures, targets, emb, pack="device", **kw),
                "from_arrays_numpy": lambda: P.PackedDataset.from_arrays(lat, frac, ptr, syms, targets, emb, **kw),
                "from_arrays_device": lambda: P.PackedDataset.from_arrays(d_lat, d_frac, d_ptr, d_rows,
                                                                          {"e_above_hull": d_tgt}, emb, **kw)}
        times = {name: [] for name in arms}
        built = {}
        for rep in range(args.reps + 1):                     # repetition 0 warms every arm up and is not counted
            for name, fn in arms.items():
                dt, ds = _clock(fn)
                if rep:
                    times[name].append(dt)
                built[name] = ds
        same = all(all(torch.equal(ds.t[k], built["from_structures"].t[k]) for k in ds.t) for ds in built.values())
        res = {name: _stat(ts, G) for name, ts in times.items()}
        base = res["from_structures"]["ms_median"]
        for name in res:
            res[name]["speedup_vs_from_structures"] = round(base / res[name]["ms_median"], 2)
        # the numpy build, stage by stage
        stages = {k: [] for k in ("symbols_to_rows", "upload", "neighbor_tables", "from_tables")}
        for rep in range(args.reps + 1):
            t_sym, r = _clock(lambda: _symbol_rows(syms, list(ELEMENT_SYMBOLS)))
            t_up, dv = _clock(lambda: (up(lat), up(frac), up(ptr), up(r)))
            t_nb, tabs = _clock(lambda: P.neighbor_tables(dv[0], dv[1], dv[2], K))
            t_pk, _ = _clock(lambda: P.PackedDataset.from_tables(tabs, dv[2], dv[3], emb, targets, max_neighbor_number=K,
                                                                 device=dev))
            if rep:
                for k, v in zip(stages, (t_sym, t_up, t_nb, t_pk)):
                    stages[k].append(v)
        res["stages_of_from_arrays_numpy"] = {k: _stat(v) for k, v in stages.items()}
        res["plan_write_launches"] = _launches_ms(P, tabs, d_ptr, d_rows, d_tgt, K, len(ELEMENT_SYMBOLS), args.reps)
        res["all_builds_bit_identical"] = bool(same)
        out[f"K{K}"] = res
    if not args.no_forward:                                  # the stage after packing, same box, same process
        import infer_bench
        net = infer_bench.net_case(G, 3)
        ms = net["eval_fwd_ms"]["infer"]
        out["eval_forward"] = {"crystals": G, "E": net["E"], "eval_fwd_ms": ms, "crystals_per_s": round(G / ms * 1e3, 1)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
