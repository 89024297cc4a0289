"""Neighbour tables on the device (csrc/neighbors.hip) at the benchmark's size: 4 167 synthetic crystals of 20 atoms,
K = 12 and 24, radius 18 -- crystals/s and atoms/s of the kernel (device events around the launch pair, warm-up, median),
the share of atoms that needed a second working radius, the whole `PackedDataset.from_structures` call (host clock, ends in
a synchronise), and beside them on the same box the numpy restatement's rate (tests/neighbor_cases.py) on a subsample and
the eval forward's crystals/s (tools/infer_bench.py, CGAtNet(200, 128, 4, msg_heads=3) on the same 4 167 x 20 x 12 batch).
Writes one JSON object to --out and prints it.

    python tools/neighbor_bench.py [--reps 20] [--crystals 4167] [--out profiles/neighbor_bench.json]
    python tools/neighbor_bench.py --only-profile        # a few launches, for rocprofv3 --kernel-trace --stats
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def _device_inputs(structures, dev):
    lat = np.stack([s[0] for s in structures])
    frac = np.concatenate([s[1] for s in structures])
    ptr = np.zeros(len(structures) + 1, np.int32)
    ptr[1:] = np.cumsum([s[1].shape[0] for s in structures])
    return tuple(torch.from_numpy(a).to(dev) for a in (lat, frac, ptr))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--crystals", type=int, default=4167)
    ap.add_argument("--atoms", type=int, default=20)
    ap.add_argument("--subsample", type=int, default=24, help="crystals the numpy restatement is timed on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbor_bench.json"))
    ap.add_argument("--only-profile", action="store_true")
    ap.add_argument("--no-forward", action="store_true", help="skip the eval forward of tools/infer_bench.py")
    args = ap.parse_args()
    import cgat_amd as P
    from cgat_amd import neighbors
    if not torch.cuda.is_available():
        raise SystemExit("neighbor_bench: no GPU visible; rates are measured on the device or not at all")
    dev = "cuda:0"
    structures = P.synthetic_structures(args.crystals, 0, atoms=args.atoms)
    lat, frac, ptr = _device_inputs(structures, dev)
    G, N = lat.shape[0], frac.shape[0]
    if args.only_profile:
        for K in (12, 24):
            for _ in range(5):
                neighbors._run(lat, frac, ptr, K, 18.0, False, False)
        torch.cuda.synchronize()
        return
    out = {"tool": "neighbor_bench", "device": torch.cuda.get_device_name(0), "crystals": G, "atoms": N, "radius": 18.0,
           "reps": args.reps}
    for K in (12, 24):
        med, lo, hi = _median_ms(lambda: neighbors._run(lat, frac, ptr, K, 18.0, False, False), args.reps)
        res = P.neighbor_tables(lat, frac, ptr, K, return_passes=True)
        passes = res.passes.cpu().numpy()
        t0 = time.perf_counter()
        ds = P.PackedDataset.from_structures(structures, {"e_above_hull": np.zeros(G)}, _embedding(), max_neighbor_number=K,
                                             stored_neighbors=K, device=dev)
        torch.cuda.synchronize()
        whole = time.perf_counter() - t0
        out[f"K{K}"] = {"kernel_ms_median": round(med, 4), "kernel_ms_min": round(lo, 4), "kernel_ms_max": round(hi, 4),
                        "crystals_per_s": round(G / med * 1e3, 1), "atoms_per_s": round(N / med * 1e3, 1),
                        "built": int((res.status == 0).sum()), "share_atoms_second_radius": round(float((passes > 1).mean()), 5),
                        "max_passes": int(passes.max()), "from_structures_s": round(whole, 3),
                        "from_structures_crystals_per_s": round(len(ds) / whole, 1)}
    # the numpy restatement, same box, a subsample (it enumerates every image at the full radius)
    import neighbor_cases as NC
    sub = structures[:args.subsample]
    t0 = time.perf_counter()
    ref = [NC.reference_tables(s[0], s[1], 24) for s in sub]
    dt = time.perf_counter() - t0
    n_sub = sum(s[1].shape[0] for s in sub)
    got = P.neighbor_tables(*_device_inputs(sub, dev), 24)
    gs, gn = got.shell.cpu().numpy(), got.nbr_idx.cpu().numpy()
    a0, comparable, equal = 0, 0, 0
    for s, r in zip(sub, ref):
        n = s[1].shape[0]
        if NC.ambiguous_gaps(s[0], s[1], 24) == 0:
            comparable += 1
            equal += int(np.array_equal(gs[a0:a0 + n], r[1]) and np.array_equal(gn[a0:a0 + n], r[3]))
        a0 += n
    out["numpy_restatement_K24"] = {"crystals": len(sub), "seconds": round(dt, 3), "crystals_per_s": round(len(sub) / dt, 2),
                                    "atoms_per_s": round(n_sub / dt, 1), "comparable_crystals": comparable,
                                    "equal_to_kernel": equal}
    if not args.no_forward:
        import infer_bench
        net = infer_bench.net_case(G, max(3, args.reps // 4))
        ms = net["eval_fwd_ms"]["infer"]
        out["eval_forward"] = {"crystals": G, "E": net["E"], "eval_fwd_ms": ms, "crystals_per_s": round(G / ms * 1e3, 1)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def _embedding():
    from cgat_amd.graph import ELEMENT_SYMBOLS, element_table
    table = element_table().numpy()
    return {el: table[k].astype("float64").tolist() for k, el in enumerate(ELEMENT_SYMBOLS)}


if __name__ == "__main__":
    main()
