"""Cases, seeded operands, the fp64 reference and the library runner of the hypernetwork route tests
(tests/test_hnet_routes.py; the route table itself is tests/test_hnet_routes_cpu.py).

The reference restates cgat_hnet_forward (include/cgat_hip.h; reference Hypernetworksmp.py:257-313) in fp64 torch on the
device: per predicted layer l, z_l = trunk_l(hin) (n_fc x [Linear + Tanh]), u_l = (vin (x) z_l) @ T_l + vin @ Bm_l^T +
z_l @ U_l^T + b0_l with T_l[i W + k, o] = head_w[(o W + i) W + k], and vin_(l+1) = tanh(LayerNorm(u_l)); its gradients are
autograd's.  The trilinear term is formed in row chunks as an outer product times a matrix, so no case needs the
[rows, W * W + W] predicted weights."""
import hashlib

import torch

MODES = ("f16x3c", "f16x3", "bf16x6", "f32")
# the launch-timer tags a hypernetwork pass can reach (CGAT_PROF in csrc), beside the process-wide launch counter
TAGS = ("mlp_chain", "linear128", "rowprog", "gemm_f32", "gemm_split", "bilinear_rows", "bilinear_dual", "bilinear_wgrad",
        "rows_dw")
LN_EPS = 1e-5
DAMPING = 0.3

# name: (W, n_fc, n_hyper, rows, damping, operands off the 16-byte grid)
CASES = {
    "small_rows": (128, 2, 2, 130, False, False),          # the small-row products (rowprog)
    "batched_chains": (128, 2, 4, 2100, False, False),     # above the small-row limit; the backward's chains in one launch
    "chain_per_layer": (128, 2, 4, 8200, False, False),    # more than 8192 rows: one chain launch per predicted layer
    "five_trunk_layers": (128, 5, 2, 2100, False, False),  # n_fc + 1 > CHAIN_MAX: no forward chain, a backward chain
    "eight_predicted": (128, 3, 8, 2100, False, False),    # 40 dense weight gradients > DW_BATCH_MAX: none waits
    "one_predicted": (128, 2, 1, 130, False, False),
    "width_64": (64, 2, 2, 130, False, False),             # every width-128 form off
    "early_prep": (128, 2, 2, 16400, False, False),        # >= 16384 rows: the overlapped backward prepares dT operands early
    "damping": (128, 2, 4, 2100, True, False),
    "off_grid": (128, 2, 2, 2100, False, True),            # h0 and one trunk weight 4 bytes off the 16-byte grid: fallbacks
}


def _off_grid(t):
    """The same values as a contiguous slice that starts at element 1 of a larger buffer."""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    out = buf[1:1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4
    return out


def make_operands(name, device):
    """{"h0", "v", "g_y", "damping" (or None), "flat"}: flat = per predicted layer n_fc trunk weights, n_fc trunk biases,
    head weight [W W + W, W], head bias [W W + W] (ops.HNetFn's order).  Seeded on the host; the same values every call."""
    W, n_fc, n_hyper, rows, damping, off = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    rn = lambda *s: torch.randn(*s, generator=g)
    ops = {"h0": rn(rows, W), "v": rn(rows, W), "g_y": rn(rows, W), "damping": torch.tensor([DAMPING]) if damping else None}
    flat = []
    for _ in range(n_hyper):
        flat += [rn(W, W) * (2.0 / W) ** 0.5 for _ in range(n_fc)]
        flat += [rn(W) * 0.1 for _ in range(n_fc)]
        flat += [rn(W * W + W, W) * 0.1 * (2.0 / W) ** 0.5, rn(W * W + W) * 0.05]
    ops = {k: (None if t is None else t.to(device)) for k, t in ops.items()}
    ops["flat"] = [t.to(device) for t in flat]
    if off:
        ops["h0"] = _off_grid(ops["h0"])
        ops["flat"][1] = _off_grid(ops["flat"][1])      # the second trunk weight of predicted layer 0
    return ops


def grad_names(name):
    W, n_fc, n_hyper, rows, damping, off = CASES[name]
    per = [f"fc_w{s}" for s in range(n_fc)] + [f"fc_b{s}" for s in range(n_fc)] + ["head_w", "head_b"]
    return ["g_h0", "g_v"] + (["g_damping"] if damping else []) + [f"layer{l}.{n}" for l in range(n_hyper) for n in per]


def reference(h0, v, damping, n_fc, n_hyper, flat, g_y, chunk=1024):
    """(y, [gradients in grad_names order]) in fp64 on the operands' device."""
    dd = lambda t: t.detach().double().requires_grad_(True)
    h0, v = dd(h0), dd(v)
    d = None if damping is None else dd(damping)
    flat = [dd(t) for t in flat]
    W = v.shape[1]
    hin = h0 if d is None else d * h0 + (1.0 - d) * v
    per = 2 * n_fc + 2
    vin = v
    for l in range(n_hyper):
        t = flat[l * per:(l + 1) * per]
        z = hin
        for s in range(n_fc):
            z = torch.tanh(z @ t[s].T + t[n_fc + s])
        head_w, head_b = t[2 * n_fc], t[2 * n_fc + 1]
        T = head_w[:W * W].view(W, W, W).permute(1, 2, 0).reshape(W * W, W)       # [i W + k, o]
        tri = torch.cat([(vin[a:a + chunk, :, None] * z[a:a + chunk, None, :]).reshape(-1, W * W) @ T
                         for a in range(0, vin.shape[0], chunk)])
        u = tri + vin @ head_b[:W * W].view(W, W).T + z @ head_w[W * W:].T + head_b[W * W:]
        vin = u if l == n_hyper - 1 else torch.tanh(torch.nn.functional.layer_norm(u, (W,), eps=LN_EPS))
    leaves = [h0, v] + ([d] if d is not None else []) + flat
    grads = torch.autograd.grad(vin, leaves, g_y.double())
    return vin.detach(), [g.detach() for g in grads]


def run_library(name, ops_, overlapped=False):
    """cgat_hnet_forward + cgat_hnet_backward (or _backward_overlapped, joined before returning) through cgat_amd.ops.
    Returns (y, [gradients in grad_names order], launches): launches = {tag: count} of the two calls, "all" = every kernel
    launch."""
    from cgat_amd import ops
    W, n_fc, n_hyper, rows, damping, off = CASES[name]
    dev = ops_["v"].device
    ops.prof_enable(True)
    ops.prof_reset()
    before = ops.prof_launches()
    try:
        y, saved, d, flat = ops._hnet_forward(ops_["h0"], ops_["v"], ops_["damping"], n_fc, n_hyper, ops_["flat"])
        assert [t.data_ptr() for t in flat] == [t.data_ptr() for t in ops_["flat"]] and saved.data_ptr() % 16 == 0
        main = torch.cuda.current_stream(dev)
        side = (main, ops.side_stream(dev)) if overlapped else None
        g_h0, g_v, g_d, grads, side_ws = ops._hnet_backward(ops_["h0"], ops_["v"], saved, d, flat, n_fc, n_hyper, ops_["g_y"],
                                                            side=side)
        if overlapped:
            main.wait_stream(side[1])
        torch.cuda.synchronize(dev)
        del side_ws
        launches = {t: ops.prof_get(t)[0] for t in TAGS}
        launches["all"] = ops.prof_launches() - before
    finally:
        ops.prof_enable(False)
    return y, [g_h0, g_v] + ([g_d] if g_d is not None else []) + list(grads), launches


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]
