"""The optimiser and criterion choices of the reference's harness, fused against torch's own, interleaved
in one process: over the 307 tensors / 44.6 M parameters of CGAtNet(200, 128, 4, msg_heads=3) one step of FusedSGD
(momentum 0.9 and 0), FusedAdam and FusedAdamW (the yardstick) next to torch.optim.SGD / Adam / AdamW on the same
gradients; and loss + mae + rmse of a step at 64 and 4 167 crystals, `criterion_with_metrics` next to the torch
expression of CGAT/lightning_module.py:206-210, 240-243.  Per case: wall time per call (host clock around calls that
end in a device synchronise), the library's launches and its mean kernel time over 20 calls (ops.prof_launches, CGAT_PROF tags), achieved
bytes/s from the algorithmic bytes, and the number of GPU kernels torch.profiler sees in one call.  Writes one JSON
file and prints it.

    python tools/optim_bench.py [--reps 20] [--rounds 5] [--no-profiler] [--out profiles/optim_family.json]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
LR, WD = 1e-3, 1e-2
# algorithmic bytes per parameter: read p, g (, m (, v)); write p (, m (, v))
OPTIMISERS = {"sgd_m09": ("sgd", 20), "sgd_m0": ("sgd", 12), "adam": ("adam", 28), "adamw": ("adamw", 28)}


def _wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def _median(xs):
    return sorted(xs)[len(xs) // 2]


def _gpu_kernels(fn):
    """GPU kernels of one call as torch.profiler lists them (None where the profiler gives no device events)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception as exc:                                  # the measurement is optional; the timings are not
        print("torch.profiler:", repr(exc), file=sys.stderr)
        return None


def _library(fn, tag, calls=20):
    """(launches of the library per call, mean kernel ms under `tag` over `calls` calls)"""
    from cgat_amd import ops
    torch.cuda.synchronize()
    ops.prof_reset()
    ops.prof_enable(True)
    before = ops.prof_launches()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    launches = (ops.prof_launches() - before) / calls
    ops.prof_enable(False)
    n, ms = ops.prof_get(tag)
    if n == 0:
        raise SystemExit(f"optim_bench.py: no launch was recorded under the tag {tag!r}")
    return launches, ms / n


def _interleaved(cases, reps, rounds):
    for fn in cases.values():                                 # warm-up: state, plans, code objects
        for _ in range(3):
            fn()
    ms = {k: [] for k in cases}
    for _ in range(rounds):
        for k, fn in cases.items():
            ms[k].append(_wall_ms(fn, reps))
    return {k: round(_median(v), 4) for k, v in ms.items()}, {k: [round(x, 4) for x in v] for k, v in ms.items()}


def optimiser_cases(reps, rounds):
    import cgat_amd as P
    torch.manual_seed(1)
    net = P.CGAtNet(200, 128, 4, msg_heads=3, neighbor_number=12, update_edges=True).to(DEV)
    base = [p.detach() for p in net.parameters()]
    g = torch.Generator().manual_seed(2)
    grads = [torch.randn(p.shape, generator=g).to(DEV) for p in base]
    n_params = sum(p.numel() for p in base)

    def clone():
        ps = [torch.nn.Parameter(p.clone()) for p in base]
        for p, gr in zip(ps, grads):
            p.grad = gr                                       # the same gradients for every optimiser; none writes them
        return ps

    mk = {"fused.sgd_m09": lambda ps: P.FusedSGD(ps, lr=LR, weight_decay=WD, momentum=0.9),
          "fused.sgd_m0": lambda ps: P.FusedSGD(ps, lr=LR, weight_decay=WD, momentum=0),
          "fused.adam": lambda ps: P.FusedAdam(ps, lr=LR, weight_decay=WD),
          "fused.adamw": lambda ps: P.FusedAdamW(ps, lr=LR, weight_decay=WD),
          "torch.sgd_m09": lambda ps: torch.optim.SGD(ps, lr=LR, weight_decay=WD, momentum=0.9),
          "torch.sgd_m0": lambda ps: torch.optim.SGD(ps, lr=LR, weight_decay=WD, momentum=0),
          "torch.adam": lambda ps: torch.optim.Adam(ps, lr=LR, weight_decay=WD),
          "torch.adamw": lambda ps: torch.optim.AdamW(ps, lr=LR, weight_decay=WD)}
    cases = {k: f(clone()).step for k, f in mk.items()}
    wall, rounds_ms = _interleaved(cases, reps, rounds)
    out = {"tensors": len(base), "parameters": n_params, "reps": reps, "rounds": rounds, "step": {}}
    for k, fn in cases.items():
        side, name = k.split(".")
        tag, bytes_per = OPTIMISERS[name]
        res = {"wall_ms": wall[k], "wall_ms_rounds": rounds_ms[k]}
        if side == "fused":
            launches, kernel_ms = _library(fn, tag)
            res.update({"library_launches": launches, "kernel_ms": round(kernel_ms, 4),
                        "algorithmic_bytes": bytes_per * n_params,
                        "achieved_GBps": round(bytes_per * n_params / (kernel_ms * 1e-3) / 1e9, 1),
                        "frac_of_8TBps": round(bytes_per * n_params / (kernel_ms * 1e-3) / 8e12, 4)})
        out["step"][k] = res
    s = out["step"]
    out["ratios"] = {"fused.sgd_m09 / fused.adamw (kernel; 20/28 = 0.714 by bytes)":
                     round(s["fused.sgd_m09"]["kernel_ms"] / s["fused.adamw"]["kernel_ms"], 4),
                     "fused.adam / fused.adamw (kernel; 1 by bytes)":
                     round(s["fused.adam"]["kernel_ms"] / s["fused.adamw"]["kernel_ms"], 4),
                     **{f"fused / torch wall, {n}": round(s[f"fused.{n}"]["wall_ms"] / s[f"torch.{n}"]["wall_ms"], 4)
                        for n in OPTIMISERS}}
    return out, cases


def criterion_cases(n, reps, rounds):
    """One step's loss, mae and rmse with the gradient to `output`: the harness' default criterion (nn.L1Loss on the
    normalised target) and RobustL1, on the [n, 2] output of the network split as the harness splits it."""
    import cgat_amd as P
    mean, std = 0.3, 1.7
    g = torch.Generator().manual_seed(n)
    net_out = torch.randn(n, 2, generator=g).to(DEV).requires_grad_(True)
    y = torch.randn(n, generator=g).to(DEV)
    mae_fn, mse_fn = torch.nn.functional.l1_loss, torch.nn.functional.mse_loss
    sqrt2 = 2.0 ** 0.5

    def fused(kind):
        def fn():
            net_out.grad = None
            output, log_std = net_out.chunk(2, dim=1)
            loss, mae, rmse = P.criterion_with_metrics(kind, output, log_std, y.view(-1, 1), mean, std)
            loss.backward()
            return loss, mae, rmse
        return fn

    def plain(kind):
        def fn():
            net_out.grad = None
            output, log_std = net_out.chunk(2, dim=1)
            target = y.view(len(y), 1)
            target_norm = (target - mean) / std
            pred = output.data * std + mean
            if kind == "L1":
                loss = torch.nn.L1Loss()(output, target_norm)
            else:
                loss = torch.mean(sqrt2 * torch.abs(output - target_norm) * torch.exp(-log_std) + log_std)
            mae, rmse = mae_fn(pred, target), mse_fn(pred, target).sqrt_()
            loss.backward()
            return loss, mae, rmse
        return fn

    cases = {f"{side}.{kind}": f(kind) for kind in ("L1", "RobustL1") for side, f in (("fused", fused), ("torch", plain))}
    wall, rounds_ms = _interleaved(cases, reps, rounds)
    out = {"crystals": n, "what": "loss + mae + rmse + backward to the network output", "step": {}}
    for k, fn in cases.items():
        res = {"wall_ms": wall[k], "wall_ms_rounds": rounds_ms[k]}
        if k.startswith("fused"):
            launches, kernel_ms = _library(fn, "loss_metrics")
            res.update({"library_launches": launches, "kernel_ms": round(kernel_ms, 4)})
        out["step"][k] = res
    for kind in ("L1", "RobustL1"):
        a, b = (float(x) for x in cases[f"fused.{kind}"]()), (float(x) for x in cases[f"torch.{kind}"]())
        out["step"][f"fused.{kind}"]["max_rel_diff_to_torch"] = max(abs(x - y_) / max(abs(y_), 1e-30) for x, y_ in zip(a, b))
    return out, cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-profiler", action="store_true", help="skip the torch.profiler kernel counts")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_family.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench.py needs an MI355X (cuda device); there is no CPU path to measure")
    measured = [optimiser_cases(args.reps, args.rounds)] + [criterion_cases(n, 10 * args.reps, args.rounds) for n in (64, 4167)]
    out = {"tool": "optim_bench", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "optimisers": measured[0][0], "criterion": [m[0] for m in measured[1:]]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")

    write()                                                   # the timings are on disk before the profiler runs
    if not args.no_profiler:
        for res, cases in measured:
            for k, fn in cases.items():
                res["step"][k]["gpu_kernels"] = _gpu_kernels(fn)
        write()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
