"""Generates tests/golden/optim_family.npz (the criteria) and optim_family.<optimiser>.npz (one file per optimiser: the
snapshots are incompressible fp32 and together exceed the size cap on a committed file) from torch itself (CPU), which
is what the reference's harness calls for these choices: five steps of torch.optim.SGD (momentum 0.9 and 0) and torch.optim.Adam constructed as
CGAT/lightning_module.py:319-327 does, on the closed-form parameters / gradients of optim_recipe plus two tensors of
exactly one chunk and one chunk plus one element; and value, gradients, mae and rmse of the four criteria
(RobustL1 / RobustL2 of CGAT/utils.py:30-47, nn.L1Loss, nn.MSELoss) with the torch expressions of
lightning_module.py:153-159, 240-243.

    python tests/golden/make_optim_family_golden.py          (needs only torch)"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import optim_recipe as R

EXTRA_SHAPES = [(16384,), (16385,)]          # one chunk of the multi-tensor launch exactly, and one element more
MEAN, STD = 0.3, 1.7
OPTIMISERS = {"sgd_m09": lambda ps: torch.optim.SGD(ps, lr=R.LR, weight_decay=R.WD, momentum=0.9),
              "sgd_m0": lambda ps: torch.optim.SGD(ps, lr=R.LR, weight_decay=R.WD, momentum=0),
              "adam": lambda ps: torch.optim.Adam(ps, lr=R.LR, weight_decay=R.WD)}
CRITERIA = ("RobustL1", "RobustL2", "L1", "L2")


def params():
    out = R.params()
    for k, sh in enumerate(EXTRA_SHAPES, start=len(out)):
        out.append(R._sin(sh[0], 0.37 + 0.01 * k, 0.1 * k, 0.5).reshape(sh))
    return out


def loss_inputs():
    """(output, log_std, RAW target), each [257, 1]; row 5 has output == (target - MEAN) / STD exactly."""
    o, s, t = R.loss_inputs()
    o = o.clone()
    o[5] = ((t - MEAN) / STD)[5]
    return o, s, t


def criterion(kind, o, s, t, mean, std):
    """(loss, mae, rmse) as the reference's training_step forms them; works in the dtype of its inputs."""
    t_n = (t - mean) / std
    pred = o.detach() * std + mean
    if kind == "RobustL1":
        loss = torch.mean(np.sqrt(2.0) * torch.abs(o - t_n) * torch.exp(-s) + s)
    elif kind == "RobustL2":
        loss = torch.mean(0.5 * torch.pow(o - t_n, 2.0) * torch.exp(-2.0 * s) + s)
    elif kind == "L1":
        loss = torch.nn.L1Loss()(o, t_n)
    else:
        loss = torch.nn.MSELoss()(o, t_n)
    return loss, torch.nn.functional.l1_loss(pred, t), torch.nn.functional.mse_loss(pred, t).sqrt()


def compute():
    out = {}
    for name, mk in OPTIMISERS.items():
        ps = [torch.nn.Parameter(t.clone()) for t in params()]
        opt = mk(ps)
        for step in range(R.STEPS):
            for i, p in enumerate(ps):
                p.grad = R.grad(i, step, p.shape)
            opt.step()
            if step in (0, R.STEPS - 1):
                for i, p in enumerate(ps):
                    out[f"{name}.s{step}.p{i}"] = p.detach().numpy().copy()
        if name == "sgd_m09":
            for i, p in enumerate(ps):
                out[f"{name}.buf.p{i}"] = opt.state[p]["momentum_buffer"].numpy().copy()
    o, s, t = loss_inputs()
    for kind in CRITERIA:
        oo, ss = o.clone().requires_grad_(True), s.clone().requires_grad_(True)
        v, mae, rmse = criterion(kind, oo, ss, t, MEAN, STD)
        robust = kind.startswith("Robust")
        g = torch.autograd.grad(v, [oo, ss] if robust else [oo])
        out[f"{kind}.value"], out[f"{kind}.go"] = v.detach().numpy(), g[0].numpy()
        if robust:
            out[f"{kind}.gs"] = g[1].numpy()
        out[f"{kind}.mae"], out[f"{kind}.rmse"] = mae.numpy(), rmse.numpy()
    return out


def files(out):
    """file name -> its arrays: the criteria in optim_family.npz, each optimiser's snapshots in a file of its own"""
    split = {"optim_family.npz": {k: v for k, v in out.items() if k.split(".")[0] in CRITERIA}}
    for name in OPTIMISERS:
        split[f"optim_family.{name}.npz"] = {k: v for k, v in out.items() if k.split(".")[0] == name}
    return split


def load():
    """All arrays of the committed fixture files as one dict."""
    out = {}
    for fname in files({}):
        with np.load(os.path.join(HERE, fname)) as z:
            out.update({k: z[k] for k in z.files})
    return out


def main():
    for fname, arrays in files(compute()).items():
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **arrays)
        print("wrote", fname, len(arrays), "arrays", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
