"""Parity instrumentation (used by tests/, never on the hot path): records, per activation layer, the derivative
pattern the HIP backward will use -- `post-activation > 0` for every LeakyReLU(0.01) / ReLU of the path (reference
CGAT.py:95, message_changed.py:52,101, roost_message.py:340), keyed by the NAME of the layer's weight in the shared
state_dict layout.

Why: LeakyReLU' and ReLU' jump at 0.  Two correct fp32 evaluations of a pre-activation with |z| ~ 1e-7 max|z| can land
on different sides, and every gradient upstream then differs by a finite amount (the reference's own fp32 and fp64 runs
do).  With the oracle's derivative pattern forced to the recorded one (oracle.cgat_oracle.forced_masks) the comparison
needs no allowance for such flips.

    with cgat_amd.debug.record_masks(model) as masks:
        y = model(...)
    # masks: {"graphs.0.Node.MH_A.fc_in.weight": [bool tensor [rows, units] on the CPU, one per call], ...}
"""
import ctypes as C

import torch

from . import _lib
from ._lib import lib, check

last_hidden = None      # ops.EdgeHiddenHeadsFn leaves its hidden tensor here while a recorder is active
_active = None          # the recorder of the innermost `with`, or None (the normal state: every hook is one `is None` test)


class record_masks:
    def __init__(self, model):
        self.names = {p.data_ptr(): n for n, p in model.named_parameters()}
        self.masks = {}
        self.dropout = []      # keep-masks of the attention dropout (scaled by 1 / (1 - p)), original edge order, in call order

    def __enter__(self):
        global _active
        self.prev, _active = _active, self
        return self.masks

    def __exit__(self, *exc):
        global _active, last_hidden
        _active = self.prev
        last_hidden = None      # the [E, 2 H Hd] activation (GBs at 1 M edges) must not outlive the recorder


def recording():
    return _active is not None


def note(weight, mask):
    """`weight`: the layer's weight parameter (or any view sharing its first element); `mask`: bool [rows, units]."""
    if _active is None:
        return
    name = _active.names.get(weight.data_ptr())
    if name is not None:
        _active.masks.setdefault(name, []).append(mask.detach().to("cpu", torch.bool))


def expand_last(weights, index):
    """Shell-indexed edge features (ops.IndexedEdgeAttr): the layers with these weights have just run on the table's rows;
    the pattern each recorded last becomes that of the dense rows, mask[index] -- the reference's activation has one row
    per edge."""
    if _active is None:
        return
    idx = index.detach().to("cpu")
    for w in weights:
        lst = _active.masks.get(_active.names.get(w.data_ptr()))
        if lst:
            lst[-1] = lst[-1][idx]


def note_dropout(keep):
    if _active is not None:
        _active.dropout.append(keep.detach().to("cpu"))


def note_attention(a_in_w, m_in_w, plan, attn_params, saved, W2):
    """The fused scalar-attention layer: signs of the saved pre-activations of MH_A | MH_M through the C ABI
    (cgat_debug_nodes_attention_signs), original edge order."""
    if _active is None:
        return
    mask = torch.empty(plan.E, W2, dtype=torch.uint8, device=saved.device)
    with torch.cuda.device(saved.device):
        check(lib.cgat_debug_nodes_attention_signs(C.byref(plan.c), C.byref(attn_params), C.c_void_p(saved.data_ptr()),
                                                   C.c_void_p(mask.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "cgat_debug_nodes_attention_signs")
    half = W2 // 2
    note(a_in_w, mask[:, :half] != 0)
    note(m_in_w, mask[:, half:] != 0)


def note_attention_indexed(a_in_w, m_in_w, plan, attn_params, x, table, index):
    """The scalar-attention layer on the indexed training route (ops.NodesAttentionIndexedFn), which stores no
    pre-activations: their signs from x, table, index and the parameters through the forward's projections and the one
    function that forms z for the forward and the backward (cgat_debug_nodes_attention_signs_indexed), original edge
    order; noted as note_attention notes them."""
    if _active is None:
        return
    from . import ops
    R, W2 = int(table.shape[0]), 2 * attn_params.H * attn_params.Hd
    mask = torch.empty(plan.E, W2, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        ws = ops.workspace(lib.cgat_debug_nodes_attention_signs_indexed_workspace_bytes(C.byref(plan.c), C.byref(attn_params),
                                                                                        R), x.device)
        check(lib.cgat_debug_nodes_attention_signs_indexed(C.byref(plan.c), C.byref(attn_params), C.c_void_p(x.data_ptr()),
                                                           C.c_void_p(table.data_ptr()), R, C.c_void_p(index.data_ptr()),
                                                           C.c_void_p(mask.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(),
                                                           C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "cgat_debug_nodes_attention_signs_indexed")
    half = W2 // 2
    note(a_in_w, mask[:, :half] != 0)
    note(m_in_w, mask[:, half:] != 0)


def note_sorted_hidden(weights, plan, hidden):
    """EdgeHiddenFn's output (post-activation, destination-sorted slots) -> per-network masks in original edge order.
    `weights`: the first-layer weights of the stacked networks, equal column shares of `hidden`."""
    global last_hidden
    last_hidden = None          # consumed: drop the module-global reference (the caller's `hidden` argument keeps it for this call)
    if _active is None or hidden is None:
        return
    perm = plan.dst_perm.long()
    m = torch.empty(hidden.shape, dtype=torch.bool, device=hidden.device)
    m[perm] = hidden.detach() > 0
    share = hidden.shape[1] // len(weights)
    for k, w in enumerate(weights):
        note(w, m[:, k * share:(k + 1) * share])


# bit i of cgat_debug_nodes_attention_route's mask (include/cgat_hip.h; the route structs of csrc/layers.hip)
ROUTE_BITS = {
    "forward": ("fused_infer", "zx", "fused_z", "z_bf16", "proj_fast", "out_fast", "out_one"),
    "backward": ("rc", "vec", "have_scales", "z_bf16", "z_bf16_six", "out_fast", "out_heads_one", "node_ksplit",
                 "node_small_rows", "node_launches", "node_gemm", "node_scales", "ge_ksplit", "ge_launch", "ge_gemm",
                 "gw_launch", "gw_gemm"),
}


def nodes_attention_route(N, E, C_, Ce, H, Hd, backward=False):
    """The names of the routes the scalar-attention layer takes at these shapes in the current arithmetic and
    edge-storage modes, for 16-byte aligned operands (host only, no GPU needed)."""
    plan = _lib.Plan(N, E, None, None, None, None, None, None)
    p = _lib.AttnParams(C_, Ce, H, Hd, *([None] * 8))
    mask = lib.cgat_debug_nodes_attention_route(C.byref(plan), C.byref(p), 1 if backward else 0)
    return {n for i, n in enumerate(ROUTE_BITS["backward" if backward else "forward"]) if mask >> i & 1}


def nodes_attention_bit_form(N, E, C_, Ce, H, Hd):
    """Does the training forward of the scalar-attention layer keep its saved buffer in the bit form at these shapes, in
    the current arithmetic and edge-storage modes, for 16-byte aligned operands (cgat_nodes_attention_bit_form; host only):
    sign words and the two half projections in place of the attention pre-activations."""
    plan = _lib.Plan(N, E, None, None, None, None, None, None)
    p = _lib.AttnParams(C_, Ce, H, Hd, *([None] * 8))
    return bool(lib.cgat_nodes_attention_bit_form(C.byref(plan), C.byref(p)))


# bit i of cgat_debug_edge_hidden_route's mask (include/cgat_hip.h)
EDGE_HIDDEN_ROUTE_BITS = {
    "forward": ("fast",),
    "backward": ("have_scales", "node_ksplit", "node_small_rows", "node_launches", "node_gemm", "node_scales", "ge_ksplit",
                 "ge_launch", "ge_gemm", "gw_launch", "gw_gemm"),
}


def edge_hidden_route(N, E, C_, Ce, W2, backward=False, g_is_pre=False, has_absmax=False):
    """The names of the routes cgat_edge_hidden_forward / _backward (the operand-split first layer of the vector-attention
    variants) take at these shapes in the current arithmetic mode, for 16-byte aligned operands (host only, no GPU
    needed).  g_is_pre / has_absmax: the backward's arguments of those names."""
    plan = _lib.Plan(N, E, None, None, None, None, None, None)
    mask = lib.cgat_debug_edge_hidden_route(C.byref(plan), C_, Ce, W2, 1 if backward else 0, 1 if g_is_pre else 0,
                                            1 if has_absmax else 0)
    return {n for i, n in enumerate(EDGE_HIDDEN_ROUTE_BITS["backward" if backward else "forward"]) if mask >> i & 1}


# bit i of cgat_debug_hnet_route's mask (include/cgat_hip.h; HnetFwdRoute / HnetBwdRoute of csrc/hnet.hip)
HNET_ROUTE_BITS = {
    "forward": ("t_batched", "w_batched", "chained", "ln_fused"),
    "backward": ("t_batched", "w_batched", "dual", "chain", "chain_queued", "dw_deferred", "head_dw_queued",
                 "head_dw_rows", "dT_side", "early_prep", "dw_side", "dw_side_ws"),
}


def hnet_route(rows, W, n_fc, n_hyper, backward=False, overlapped=False):
    """The names of the routes cgat_hnet_forward / _backward (overlapped: _backward_overlapped) take at these shapes in the
    current arithmetic mode, for 16-byte aligned operands (host only, no GPU needed)."""
    p = _lib.HnetParams()
    p.W, p.n_fc, p.n_hyper = W, n_fc, n_hyper
    mask = lib.cgat_debug_hnet_route(rows, C.byref(p), 1 if backward else 0, 1 if overlapped else 0)
    return {n for i, n in enumerate(HNET_ROUTE_BITS["backward" if backward else "forward"]) if mask >> i & 1}


EDGE_Z_KERNELS = ("none", "rows128", "rows256", "msg_wsum")     # cgat_edge_z_form.kernel
EDGE_Z_LAUNCHES = ("edge_z", "edge_logits", "edge_msg_wsum")    # cgat_debug_edge_z_form's `launch`
EDGE_Z_STORES = ("f32", "bf16", "bits")


def edge_z_form(rows, W2, H=1, Hd=128, n_add_rows=0, ld_add=None, store="f32", adds=False, logits=False, omax=False, act=0,
                launch="edge_z"):
    """Which kernel a launch of the per-edge family (csrc/edgez.hip) runs at these dims in the current arithmetic mode, as
    a dict of cgat_edge_z_form's fields with `kernel` by name (host only, no GPU needed); None where the launch refuses the
    combination.  The defaults are the dense layer at width 128 with W2 outputs."""
    f = _lib.EdgeZForm()
    rc = lib.cgat_debug_edge_z_form(EDGE_Z_LAUNCHES.index(launch), rows, W2, H, Hd, n_add_rows, W2 if ld_add is None else ld_add,
                                    EDGE_Z_STORES.index(store), int(adds), int(logits), int(omax), act, C.byref(f))
    if rc != 0:
        return None
    d = {n: getattr(f, n) for n, _ in f._fields_}
    d["kernel"] = EDGE_Z_KERNELS[f.kernel]
    return d


EDGE_GE_LAUNCHES = ("plain", "ksplit", "prepared", "heads")      # cgat_debug_edge_bwd_form's `launch` for product "ge"
EDGE_GE_PREPS = ("none", "planes", "f16_tmax", "attn", "heads_f16")    # cgat_edge_bwd_form.prep


def edge_bwd_form(product, rows, W2, H=1, Hd=128, launch="plain", rebuilt=False, maxima=False, perm=False, force_six=False,
                  te=False):
    """Which form a launch of the backward per-edge family (csrc/edgebwd.hip) runs at these dims in the current arithmetic
    and edge-storage modes: product "ge" (rows @ W, K = W2 -> 128) or "gw" (rows^T @ e, K = rows), as a dict of the fields
    of cgat_edge_bwd_form that belong to the product, `prep` by name (host only, no GPU needed); None where the launch
    refuses the combination."""
    f = _lib.EdgeBwdForm()
    rc = lib.cgat_debug_edge_bwd_form(("ge", "gw").index(product), EDGE_GE_LAUNCHES.index(launch), rows, W2, H, Hd, int(rebuilt),
                                      int(maxima), int(perm), int(force_six), int(te), C.byref(f))
    if rc != 0:
        return None
    if product == "ge":
        d = {n: getattr(f, n) for n in ("passes", "rc", "bitplane", "prep", "grid_x", "groups", "blocks_per_group", "heads")}
        d["prep"] = EDGE_GE_PREPS[f.prep]
        return d
    return {n: getattr(f, n) for n in ("passes", "rc", "bitplane", "grid_x", "bit_shape", "te_only", "ranges", "SA", "SM",
                                       "message_pairs", "bit_grid_x", "ws_end", "ws_floats")}


def edge_ge_rebuilt(mask, ga, alpha, gS, wA, dst, We, H, Hd):
    """grad edge_attr's product alone on caller-supplied ingredients of the rebuilt rows (cgat_debug_edge_ge_rebuilt,
    include/cgat_hip.h): mask int32 [E, 2 H Hd / 32] bit words, ga / alpha [E, H], gS [N, H Hd], wA [H Hd], dst int32 [E],
    We [2 H Hd, 128]; returns [E, 128] in slot order."""
    E, dev = ga.shape[0], ga.device
    t = [mask.contiguous(), ga.contiguous(), alpha.contiguous(), gS.contiguous(), wA.contiguous(), dst.contiguous(),
         We.contiguous()]
    assert t[0].dtype == torch.int32 and t[5].dtype == torch.int32 and all(v.dtype == torch.float32 for v in t[1:5] + t[6:])
    out = torch.empty(E, 128, dtype=torch.float32, device=dev)
    from . import ops
    nbytes = lib.cgat_debug_edge_ge_rebuilt_workspace_bytes(E, H, Hd)
    ws = ops.workspace(nbytes, dev)
    with torch.cuda.device(dev):
        check(lib.cgat_debug_edge_ge_rebuilt(*[C.c_void_p(v.data_ptr()) for v in t], H, Hd, E, C.c_void_p(out.data_ptr()),
                                             C.c_void_p(ws.data_ptr()), ws.numel() * ws.element_size(),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "cgat_debug_edge_ge_rebuilt")
    return out


def edge_gw_rebuilt(mask, ga, alpha, gS, wA, e, perm, dst, H, Hd, force_six=False):
    """grad W_e's product alone on caller-supplied ingredients of the rebuilt rows (cgat_debug_edge_gw_rebuilt,
    include/cgat_hip.h): mask int32 [E, 2 H Hd / 32], ga / alpha [E, H], gS [N, H Hd], wA [H Hd], e [E, 128] in original
    edge order, perm int32 [E] (slot -> edge), dst int32 [E].  Returns (out [2 H Hd, 128], took_bitplane)."""
    E, dev = ga.shape[0], ga.device
    t = [mask.contiguous(), ga.contiguous(), alpha.contiguous(), gS.contiguous(), wA.contiguous(), e.contiguous(),
         perm.contiguous(), dst.contiguous()]
    assert all(v.dtype == torch.int32 for v in (t[0], t[6], t[7])) and all(v.dtype == torch.float32 for v in t[1:6])
    out = torch.empty(2 * H * Hd, 128, dtype=torch.float32, device=dev)
    from . import ops
    ws = ops.workspace(lib.cgat_debug_edge_gw_rebuilt_workspace_bytes(E, H, Hd), dev)
    took = C.c_int32(0)
    with torch.cuda.device(dev):
        check(lib.cgat_debug_edge_gw_rebuilt(*[C.c_void_p(v.data_ptr()) for v in t], H, Hd, E, 1 if force_six else 0,
                                             C.c_void_p(out.data_ptr()), C.byref(took), C.c_void_p(ws.data_ptr()),
                                             ws.numel() * ws.element_size(),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "cgat_debug_edge_gw_rebuilt")
    return out, bool(took.value)


def edge_gw_force_six(flag):
    """Process-wide: grad W_e keeps its six-pass form on every column (the A/B reference of the bit-plane route).  Returns
    the previous setting."""
    return bool(lib.cgat_debug_edge_gw_force_six(1 if flag else 0))


def neighbor_tables_with(lattice, frac_coords, atom_ptr, max_neighbor_number, radius, cap, first_radius=0.0):
    """neighbors.neighbor_tables with the candidate capacity (K .. 2048) and the first working radius (0 = from the number
    density) chosen by the caller (cgat_debug_neighbor_tables): drives the kernel's shrink / grow / does-not-fit paths.
    Returns the tables with distances and pass counts; status 2 is reported in `.status`, not raised."""
    from . import neighbors
    return neighbors._run(lattice, frac_coords, atom_ptr, max_neighbor_number, radius, True, True, cap=cap,
                          first_radius=first_radius)
