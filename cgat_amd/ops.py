"""torch.autograd wrappers over the C ABI.  PyTorch supplies device memory, the current
stream and the autograd tape; all arithmetic of the path runs in libcgat_hip kernels.
"""
import ctypes as C

import os

import torch

from . import _lib, debug, rowprog
from ._lib import lib, check


# ----------------------------------------------------------------------------------------
# plumbing
# ----------------------------------------------------------------------------------------
_NO_CPU = ("cgat_amd: the HIP path needs tensors on an MI355X device (cuda:N); "
           "there is no CPU fallback -- use oracle/ only for checking")


def _require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(_NO_CPU)


def _f32c(t):
    if t.dtype != torch.float32:
        raise TypeError(f"cgat_amd: expected float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_ws = {}


def workspace(nbytes, device):
    """Grow-only per-device scratch buffer.  All launches are ordered on the current stream, so
    one buffer serves every call (no allocation in the steady state)."""
    if torch.cuda.is_current_stream_capturing():
        # inside a hipGraph capture (cgat_amd.GraphedStep) the buffer must belong to THAT graph's memory pool: a cached
        # one would come from an earlier capture on the same capture stream, whose pool dies with its graph.  The pool
        # reuses the block as soon as the tensor is dropped, exactly as the caching allocator does in eager mode.
        return torch.empty(int(nbytes) + 4096, dtype=torch.uint8, device=device)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25) + 4096, dtype=torch.uint8, device=device)
        _ws[key] = buf
    return buf


def _scratch(numel, dtype, device):
    """A saved-for-backward / side buffer whose size the library dictates (only its pointer is used): the element count is
    rounded up to 1/16 of its octave.  Ragged batches change E by a few per cent from step to step; with exact sizes
    every new maximum made torch's caching allocator hipMalloc a fresh multi-GB block per layer (two 840-ms steps among
    121-ms ones in the training bench), with rounded sizes the cached blocks fit."""
    n = int(numel)
    if n > (1 << 20):
        step = 1 << (n.bit_length() - 5)
        n = (n + step - 1) // step * step
    return torch.empty(n, dtype=dtype, device=device)


# Destinations for parameter gradients (cgat_amd.dist.GradientAverager registers one): a backward pass that is about to
# allocate the gradient of a parameter asks the sinks first and writes straight into what they hand out -- the
# all-reduce bucket -- instead of into a fresh tensor that autograd then adds to (or the averager copies into) the bucket:
# 38 MB of gradients per layer step made 0.44 ms of fills, adds and copies at world size 1 (rocprofv3, round 6).
_grad_sinks = []


def register_grad_sink(fn):
    """fn(w) -> a writable tensor of w's shape that will BE the parameter's gradient, or None."""
    _grad_sinks.append(fn)
    return fn


def unregister_grad_sink(fn):
    if fn in _grad_sinks:
        _grad_sinks.remove(fn)


def _param_grad(w):
    for sink in _grad_sinks:
        t = sink(w)
        if t is not None:
            return t
    return torch.empty_like(w)


class _Switch:
    """One on/off switch of the package: its value, the env variable a fresh process reads it from ("0" / "1"; anything
    else leaves the default) and its default.  A default of None makes it a tri-state: None stays None until set."""

    def __init__(self, env, default):
        self.env, self.default = env, default
        self.value = {"0": False, "1": True}.get(os.environ.get(env), default)

    def set(self, flag):
        self.value = None if (flag is None and self.default is None) else bool(flag)


_validate_indices = os.environ.get("CGAT_VALIDATE_INDICES", "1") != "0"


def set_validate_indices(flag):
    """Index validation of the CSR plans (default on): an edge_index / segment index entry outside [0, N) raises
    IndexError, as the reference's index_select / scatter would.  It costs one host sync per plan build; a training
    loop that trusts its collation can switch it off."""
    global _validate_indices
    _validate_indices = bool(flag)


def _check_plan_complete(rowptr, n, what):
    # the plan builder drops out-of-range keys, so the last row pointer falls short of n exactly when one exists
    if _validate_indices and n > 0:
        got = int(rowptr[-1])
        if got != n:
            raise IndexError(f"cgat_amd: {n - got} of {n} entries of {what} are outside [0, {rowptr.numel() - 1})")


class EdgePlan:
    """CSR plan of a batch (C struct cgat_plan): built once per edge_index, shared by all layers,
    forward and backward."""

    def __init__(self, edge_index, num_nodes):
        _require_gpu(edge_index)
        if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise TypeError("edge_index must be int64 [2, E]")
        ei = edge_index.contiguous()
        E, N = int(ei.shape[1]), int(num_nodes)
        dev = ei.device
        i32 = dict(dtype=torch.int32, device=dev)
        self.N, self.E = N, E
        self.dst_rowptr = torch.empty(N + 1, **i32)
        self.dst_perm = torch.empty(E, **i32)
        self.dst_sorted = torch.empty(E, **i32)
        self.src_sorted = torch.empty(E, **i32)
        self.src_rowptr = torch.empty(N + 1, **i32)
        self.src_pos = torch.empty(E, **i32)
        nbytes = lib.cgat_plan_workspace_bytes(E, N)
        ws = workspace(nbytes, dev)
        with torch.cuda.device(dev):
            check(lib.cgat_plan_build(_ptr(ei), E, N, _ptr(self.dst_rowptr), _ptr(self.dst_perm),
                                      _ptr(self.dst_sorted), _ptr(self.src_sorted), _ptr(self.src_rowptr),
                                      _ptr(self.src_pos), _ptr(ws), ws.numel(), _stream()), "cgat_plan_build")
        _check_plan_complete(self.dst_rowptr, E, "edge_index[1]")
        _check_plan_complete(self.src_rowptr, E, "edge_index[0]")
        self.c = _lib.Plan(N, E, self.dst_rowptr.data_ptr(), self.dst_perm.data_ptr(), self.dst_sorted.data_ptr(),
                           self.src_sorted.data_ptr(), self.src_rowptr.data_ptr(), self.src_pos.data_ptr())


_plan_cache = {}


def get_plan(edge_index, num_nodes):
    """Small LRU keyed by the edge_index storage: every layer of a stack (and its backward)
    reuses the same plan."""
    key = (edge_index.data_ptr(), tuple(edge_index.shape), int(num_nodes), edge_index._version, edge_index.device.index)
    # a long-lived edge_index object carries its plan itself (the closed chunks of chunked.py: 8+ chunk tensors per 64 M
    # edges would evict each other from the 8-entry LRU and rebuild -- and re-validate, two host syncs -- their plan in
    # every forward, recomputation and backward)
    if hasattr(edge_index, "_cgat_plan"):                 # marked by its owner (chunked.closed_chunks): built on first use
        return attach_plan(edge_index, num_nodes)
    plan = _plan_cache.get(key)
    if plan is None:
        if len(_plan_cache) >= 8:
            _plan_cache.pop(next(iter(_plan_cache)))
        plan = EdgePlan(edge_index, num_nodes)
        plan._keepalive = edge_index
        _plan_cache[key] = plan
    return plan


def attach_plan(edge_index, num_nodes):
    """Build (and validate) the plan of `edge_index` once and keep it on the tensor object itself."""
    key = (edge_index.data_ptr(), tuple(edge_index.shape), int(num_nodes), edge_index._version, edge_index.device.index)
    own = getattr(edge_index, "_cgat_plan", None)
    if own is None or own[0] != key:
        edge_index._cgat_plan = (key, EdgePlan(edge_index, num_nodes))
    return edge_index._cgat_plan[1]


class SegmentPlan:
    """rowptr/perm for a generic int64 segment index (crystal index, Roost self index)."""

    def __init__(self, index, num_segments):
        _require_gpu(index)
        dev = index.device
        n, S = int(index.numel()), int(num_segments)
        keys = index.to(torch.int32).contiguous()
        self.n, self.S = n, S
        self.rowptr = torch.empty(S + 1, dtype=torch.int32, device=dev)
        self.perm = torch.empty(n, dtype=torch.int32, device=dev)
        ws = workspace(lib.cgat_csr_workspace_bytes(S), dev)
        with torch.cuda.device(dev):
            check(lib.cgat_csr_from_keys(_ptr(keys), n, S, _ptr(self.rowptr), _ptr(self.perm), _ptr(ws), ws.numel(),
                                         _stream()), "cgat_csr_from_keys")
        _check_plan_complete(self.rowptr, n, "the segment index")
        self.perm64 = self.perm.long()


_seg_plan_cache = {}


def get_segment_plan(index, num_segments):
    """SegmentPlan through a small LRU keyed by the index storage (as get_plan): the Roost branch and the crystal
    pooling of one batch build four plans per forward; a batch that is evaluated again (validation epochs, the
    hipGraph-captured step) builds -- and validates, one host synchronisation each -- none."""
    key = (index.data_ptr(), tuple(index.shape), int(num_segments), index._version, index.device.index)
    plan = _seg_plan_cache.get(key)
    if plan is None:
        if len(_seg_plan_cache) >= 16:
            _seg_plan_cache.pop(next(iter(_seg_plan_cache)))
        plan = SegmentPlan(index, num_segments)
        plan._keepalive = index
        _seg_plan_cache[key] = plan
    return plan


# ----------------------------------------------------------------------------------------
# GATConvNodes message + softmax + aggregate
# ----------------------------------------------------------------------------------------
def _attn_params(x, edge_attr, H, ws_):
    A_in_w = ws_[0]
    C_, Ce = x.shape[1], edge_attr.shape[1]
    D = 2 * C_ + Ce
    HHd = A_in_w.shape[0]
    assert A_in_w.numel() == HHd * D and HHd % H == 0
    Hd = HHd // H
    p = _lib.AttnParams(C_, Ce, H, Hd, *[t.data_ptr() for t in ws_])
    return p, Hd


def _require_scalar_attention(who, H, weights):
    """MH_A's second layers emit one logit per head (the fused attention entries take nothing else)."""
    A_in_w, A_out_w = weights[0], weights[2]
    if A_out_w.numel() != H * (A_in_w.shape[0] // H):
        raise ValueError(f"{who} handles scalar attention (MH_A output_dim == 1)")


def _attn_forward(x, edge_attr, plan, H, weights, *, save):
    """The scalar-attention forward behind NodesAttentionFn and NodeLayerFn (save=True: the training forward with its saved
    buffer) and nodes_attention_infer (save=False).  Returns (aggr, saved or None, the prepared weights)."""
    A_in_w, M_in_w = weights[0], weights[4]
    ws_ = [_f32c(w.detach()) for w in weights]
    _require_scalar_attention("_attn_forward", H, weights)
    N, E = plan.N, plan.E
    if x.shape[0] != N or edge_attr.shape[0] != E:
        raise ValueError(f"plan is for N={N}, E={E}; got x {tuple(x.shape)}, edge_attr {tuple(edge_attr.shape)}")
    p, Hd = _attn_params(x, edge_attr, H, ws_)
    dev = x.device
    saved = _scratch(lib.cgat_nodes_attention_saved_floats(N, E, H, Hd), torch.float32, dev) if save else None
    aggr = torch.empty(N, x.shape[1], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if save:
            ws = workspace(lib.cgat_nodes_attention_forward_workspace_bytes(C.byref(plan.c), C.byref(p)), dev)
            check(lib.cgat_nodes_attention_forward(C.byref(plan.c), C.byref(p), _ptr(x), _ptr(edge_attr), _ptr(aggr),
                                                   _ptr(saved), _ptr(ws), ws.numel(), _stream()),
                  "cgat_nodes_attention_forward")
        else:
            ws = workspace(lib.cgat_nodes_attention_infer_workspace_bytes(C.byref(plan.c), C.byref(p)), dev)
            check(lib.cgat_nodes_attention_infer(C.byref(plan.c), C.byref(p), _ptr(x), _ptr(edge_attr), _ptr(aggr), _ptr(ws),
                                                 ws.numel(), _stream()), "cgat_nodes_attention_infer")
    if save and debug.recording():
        debug.note_attention(A_in_w, M_in_w, plan, p, saved, 2 * H * Hd)
    return aggr, saved, ws_


def _attn_backward(x, edge_attr, plan, H, weights, saved, g_aggr, storage, stream):
    """cgat_nodes_attention_backward on `stream` (a raw handle) under the forward's edge-storage mode; the workspace is
    taken here, after whatever the caller has issued before.  Returns (g_x, g_e, parameter grads)."""
    g_aggr = _f32c(g_aggr)
    p, _ = _attn_params(x, edge_attr, H, weights)
    dev = x.device
    g_x, g_e = torch.empty_like(x), torch.empty_like(edge_attr)
    grads = [_param_grad(w) for w in weights]
    g = _lib.AttnGrads(*[t.data_ptr() for t in grads])
    with torch.cuda.device(dev):
        ws = workspace(lib.cgat_nodes_attention_backward_workspace_bytes(C.byref(plan.c), C.byref(p)), dev)
        with _storage_of(storage):
            check(lib.cgat_nodes_attention_backward(C.byref(plan.c), C.byref(p), _ptr(x), _ptr(edge_attr), _ptr(saved),
                                                    _ptr(g_aggr), _ptr(g_x), _ptr(g_e), C.byref(g), _ptr(ws), ws.numel(),
                                                    stream), "cgat_nodes_attention_backward")
    return g_x, g_e, grads


class NodesAttentionFn(torch.autograd.Function):
    """aggr[n] = mean_h sum_{e: dst(e)=n} softmax_dst(MH_A(m_e))[h] * MH_M(m_e)[h]
    (reference CGAT.py:319-329 + PyG aggregate), scalar attention."""

    @staticmethod
    def forward(ctx, x, edge_attr, plan, H, A_in_w, A_in_b, A_out_w, A_out_b, M_in_w, M_in_b, M_out_w, M_out_b):
        weights = [A_in_w, A_in_b, A_out_w, A_out_b, M_in_w, M_in_b, M_out_w, M_out_b]
        _require_gpu(x, edge_attr, *weights)
        x, edge_attr = _f32c(x), _f32c(edge_attr)
        aggr, saved, weights = _attn_forward(x, edge_attr, plan, H, weights, save=True)
        ctx.plan, ctx.H, ctx.storage = plan, H, lib.cgat_get_edge_storage()
        ctx.save_for_backward(x, edge_attr, saved, *weights)
        return aggr

    @staticmethod
    def backward(ctx, g_aggr):
        x, edge_attr, saved, *weights = ctx.saved_tensors
        g_x, g_e, grads = _attn_backward(x, edge_attr, ctx.plan, ctx.H, weights, saved, g_aggr, ctx.storage, _stream())
        return (g_x, g_e, None, None, *grads)


_fused_infer = _Switch("CGAT_FUSED_INFER", True)


def set_fused_inference(flag):
    """The forward-without-grad route of the scalar-attention node layer (default on; env CGAT_FUSED_INFER=0 starts it
    off): under torch.no_grad() / inference_mode(), or when nothing of a layer requires grad, GATConvNodes runs
    nodes_attention_infer instead of the autograd node -- same results bit for bit, no saved buffer, and at the
    benchmark widths no per-edge activations at all.  Off: the training forward runs (the A/B reference)."""
    _fused_infer.set(flag)


def get_fused_inference():
    return _fused_infer.value


def nodes_attention_infer(x, edge_attr, plan, H, A_in_w, A_in_b, A_out_w, A_out_b, M_in_w, M_in_b, M_out_w, M_out_b):
    """NodesAttentionFn's forward without the autograd node and without a saved buffer (cgat_nodes_attention_infer):
    buffers from workspace(), nothing allocated but the result.  Never records a backward."""
    weights = [A_in_w, A_in_b, A_out_w, A_out_b, M_in_w, M_in_b, M_out_w, M_out_b]
    _require_gpu(x, edge_attr, *weights)
    return _attn_forward(_f32c(x.detach()), _f32c(edge_attr.detach()), plan, H, weights, save=False)[0]


# ----------------------------------------------------------------------------------------
# shell-indexed edge features: edge_attr[e] = table[index[e]]
# ----------------------------------------------------------------------------------------
_indexed_edge_attr = _Switch("CGAT_INDEXED_EDGE_ATTR", False)


def set_indexed_edge_attr(flag):
    """CGAtNet carries its edge features as an IndexedEdgeAttr (default off; env CGAT_INDEXED_EDGE_ATTR=1 starts it on)
    where that is exact: every Edge layer is the shipped no_hyper form and batch.edge_attr holds integer shell ids.  The
    edge update then runs on the table's rows, and scalar-attention node layers without grad take
    nodes_attention_infer_indexed.  Off: the dense edge features of every earlier release, bit for bit."""
    _indexed_edge_attr.set(flag)


def get_indexed_edge_attr():
    return _indexed_edge_attr.value


_index_checked = {}


class IndexedEdgeAttr:
    """Edge features as a lookup: edge_attr[e] = table[index[e]].

    table  [R, Ce] float32 on the GPU; may require grad
    index  [E] int64 in original edge order, values in [0, R)

    In the shipped network nbr_embedding's lookup and every row-wise edge update keep the edge features in this form
    with R = neighbor_number + 1.  `dense()` returns small_embedding(index, table), cached on the
    object: the gradient reaches `table` through the deterministic per-class row sum of that op, which it has while
    R * Ce <= 8192 (small_embedding's limit; beyond it torch's embedding backward runs, which is not deterministic).
    The index values are validated once per index tensor (one host round trip, under ops.set_validate_indices like the
    plans; skipped during a hipGraph capture): `with_table` keeps the index and its validation."""

    def __init__(self, table, index, _checked=False):
        if not torch.is_tensor(table) or not torch.is_tensor(index):
            raise TypeError("IndexedEdgeAttr(table, index) takes two tensors")
        _require_gpu(table, index)
        if table.dtype != torch.float32 or table.dim() != 2:
            raise TypeError(f"IndexedEdgeAttr: table must be float32 [R, Ce], got {table.dtype} {tuple(table.shape)}")
        if index.dtype != torch.int64 or index.dim() != 1:
            raise TypeError(f"IndexedEdgeAttr: index must be int64 [E], got {index.dtype} {tuple(index.shape)}")
        if table.shape[0] < 1:
            raise ValueError("IndexedEdgeAttr: the table has no rows")
        self.table, self.index = table, index
        self._dense = None
        if not _checked:
            self._validate()

    def _validate(self):
        idx, R = self.index, int(self.table.shape[0])
        if not _validate_indices or idx.numel() == 0 or torch.cuda.is_current_stream_capturing():
            return
        key = (idx.data_ptr(), idx.numel(), idx._version, idx.device.index)
        if _index_checked.get(key, (1 << 62, None))[0] <= R:   # this index has passed for a table of no more rows
            return
        lo, hi = (int(v) for v in torch.aminmax(idx))
        if lo < 0 or hi >= R:
            raise IndexError(f"cgat_amd: IndexedEdgeAttr index values span [{lo}, {hi}], outside [0, {R})")
        if len(_index_checked) >= 16:
            _index_checked.pop(next(iter(_index_checked)))
        _index_checked[key] = (hi + 1, idx)              # (the tensor is kept alive: its address is the key)

    @property
    def shape(self):
        return (self.index.shape[0], self.table.shape[1])

    def with_table(self, table):
        """The same lookup over another table of as many rows (a row-wise function of this one's)."""
        if table.shape[0] != self.table.shape[0]:
            raise ValueError("IndexedEdgeAttr.with_table: the row count must not change")
        return IndexedEdgeAttr(table, self.index, _checked=True)

    def dense(self):
        if self._dense is None:
            self._dense = small_embedding(self.index, self.table)
        return self._dense


def _attn_indexed_ok(entry, plan_c, C_, Ce, H, Hd, R):
    p = _lib.AttnParams(int(C_), int(Ce), int(H), int(Hd), *([None] * 8))
    return bool(entry(C.byref(plan_c), C.byref(p), int(R)))


def infer_indexed_ok(plan_c, C_, Ce, H, Hd, R):
    """cgat_nodes_attention_infer_indexed_ok for a layer of these dims (host only; plan_c: the C struct of a plan)."""
    return _attn_indexed_ok(lib.cgat_nodes_attention_infer_indexed_ok, plan_c, C_, Ce, H, Hd, R)


def nodes_attention_infer_indexed(x, edge_attr, plan, H, A_in_w, A_in_b, A_out_w, A_out_b, M_in_w, M_in_b, M_out_w, M_out_b):
    """nodes_attention_infer for an IndexedEdgeAttr (or a (table, index) pair) without forming table[index]
    (cgat_nodes_attention_infer_indexed): Te = table W_e^T once, the per-edge phase a gather of three rows.  Equal to the
    dense call up to fp32 summation order.  Raises where the library does not take the shape (infer_indexed_ok)."""
    if not isinstance(edge_attr, IndexedEdgeAttr):
        edge_attr = IndexedEdgeAttr(*edge_attr)
    weights = [A_in_w, A_in_b, A_out_w, A_out_b, M_in_w, M_in_b, M_out_w, M_out_b]
    table, index = edge_attr.table, edge_attr.index
    _require_gpu(x, *weights)
    x, table, index = _f32c(x.detach()), _f32c(table.detach()), index.contiguous()
    ws_ = [_f32c(w.detach()) for w in weights]
    _require_scalar_attention("nodes_attention_infer_indexed", H, weights)
    N, E, R = plan.N, plan.E, int(table.shape[0])
    if x.shape[0] != N or index.shape[0] != E:
        raise ValueError(f"plan is for N={N}, E={E}; got x {tuple(x.shape)}, index {tuple(index.shape)}")
    p, Hd = _attn_params(x, table, H, ws_)
    dev = x.device
    aggr = torch.empty(N, x.shape[1], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws = workspace(lib.cgat_nodes_attention_infer_indexed_workspace_bytes(C.byref(plan.c), C.byref(p), R), dev)
        check(lib.cgat_nodes_attention_infer_indexed(C.byref(plan.c), C.byref(p), _ptr(x), _ptr(table), R, _ptr(index),
                                                     _ptr(aggr), _ptr(ws), ws.numel(), _stream()),
              "cgat_nodes_attention_infer_indexed")
    return aggr


_indexed_edge_training = _Switch("CGAT_INDEXED_EDGE_TRAIN", False)


def set_indexed_edge_training(flag):
    """The training route of shell-indexed edge features (default off; env CGAT_INDEXED_EDGE_TRAIN=1 starts it on): a
    scalar-attention node layer given an IndexedEdgeAttr WITH a backward to follow runs NodesAttentionIndexedFn -- no
    [E, Ce] edge features, no stored pre-activations, grad table and grad W_e from a per-class sum -- where the library
    takes the shape (train_indexed_ok).  It matters only where an IndexedEdgeAttr reaches the layer: through CGAtNet that
    needs set_indexed_edge_attr(True) too.  Off: such a layer densifies and runs the dense training launches, bit for bit."""
    _indexed_edge_training.set(flag)


def get_indexed_edge_training():
    return _indexed_edge_training.value


def train_indexed_ok(plan_c, C_, Ce, H, Hd, R):
    """cgat_nodes_attention_train_indexed_ok for a layer of these dims in the current arithmetic and edge-storage modes
    (host only; plan_c: the C struct of a plan)."""
    return _attn_indexed_ok(lib.cgat_nodes_attention_train_indexed_ok, plan_c, C_, Ce, H, Hd, R)


def _indexed_operands_error(x, table, index, N, E):
    """What the indexed autograd functions demand of x, table and index for a plan of N nodes and E edges: None, or the
    exception that names the first operand that fails.  The layers' route facts read it too: what these functions would
    refuse densifies instead, like every other ineligible call."""
    if not (torch.is_tensor(x) and torch.is_tensor(table) and torch.is_tensor(index)):
        return TypeError("indexed edge features: x, table and index must be tensors")
    if not (x.is_cuda and table.is_cuda and index.is_cuda):
        return RuntimeError(_NO_CPU)
    if x.dtype != torch.float32 or x.dim() != 2:
        return TypeError(f"indexed edge features: x must be float32 [N, C], got {x.dtype} {tuple(x.shape)}")
    if table.dtype != torch.float32 or table.dim() != 2:
        return TypeError(f"indexed edge features: table must be float32 [R, Ce], got {table.dtype} {tuple(table.shape)}")
    if index.dtype != torch.int64 or index.dim() != 1:
        return TypeError(f"indexed edge features: index must be int64 [E], got {index.dtype} {tuple(index.shape)}")
    if x.shape[0] != N or index.shape[0] != E:
        return ValueError(f"plan is for N={N}, E={E}; got x {tuple(x.shape)}, index {tuple(index.shape)}")
    if not index.is_contiguous():                         # (a copy per call would never find its class plan again)
        return ValueError("indexed edge features: index must be contiguous")
    return None


def _indexed_operands_ok(x, table, index, N, E):
    return _indexed_operands_error(x, table, index, N, E) is None


def _class_plan(index, plan, R):
    """The grouping of a plan's destination-sorted slots by class for the class sum of the indexed backward: (cls_pos [E],
    piece_rowptr, piece_start [R + 1]) -- a stable counting sort of the slots by index[dst_perm] (clamped as the kernels
    clamp) and the fixed 256-row pieces of every class (cgat_indexed_class_plan).  Built once per (index, plan), in a forward outside any capture; shared by all
    layers and by IndexedEdgeAttr.with_table copies (the key is the index tensor)."""
    cache = plan.__dict__.setdefault("_class_plans", {})
    key = (index.data_ptr(), index._version, int(index.numel()), int(R))
    cp = cache.get(key)
    if cp is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("cgat_amd: the class plan of an IndexedEdgeAttr must be built before a capture "
                               "(run one eager forward of the layer first)")
        dev, E = index.device, plan.E
        i32 = dict(dtype=torch.int32, device=dev)
        cls_pos = torch.empty(E, **i32)
        n_pieces = lib.cgat_indexed_class_pieces(E, R)
        piece_start, piece_rowptr = torch.empty(R + 1, **i32), torch.empty(n_pieces + 1, **i32)
        with torch.cuda.device(dev):
            ws = workspace(lib.cgat_indexed_class_plan_workspace_bytes(E, R), dev)
            check(lib.cgat_indexed_class_plan(C.byref(plan.c), _ptr(index), R, _ptr(cls_pos), _ptr(piece_start),
                                              _ptr(piece_rowptr), _ptr(ws), ws.numel(), _stream()), "cgat_indexed_class_plan")
        cp = (cls_pos, piece_rowptr, piece_start, index)          # (the index is kept alive: its address is the key)
        if len(cache) >= 4:
            cache.pop(next(iter(cache)))
        cache[key] = cp
    return cp[:3]


def _attn_forward_indexed(x, table, index, plan, H, weights):
    """cgat_nodes_attention_forward_indexed behind NodesAttentionIndexedFn and NodeLayerIndexedFn.  Everything is checked
    before the first launch.  Returns (aggr, saved, the prepared operands x, table, index, weights, the class plan)."""
    N, E = plan.N, plan.E
    err = _indexed_operands_error(x, table, index, N, E)
    if err is not None:
        raise err
    _require_gpu(*weights)
    A_in_w, M_in_w = weights[0], weights[4]
    _require_scalar_attention("NodesAttentionIndexedFn", H, weights)
    R = int(table.shape[0])
    x, table = _f32c(x.detach()), _f32c(table.detach())
    ws_ = [_f32c(w.detach()) for w in weights]
    p, Hd = _attn_params(x, table, H, ws_)
    if not lib.cgat_nodes_attention_train_indexed_ok(C.byref(plan.c), C.byref(p), R):
        raise ValueError(f"NodesAttentionIndexedFn: H {H}, Hd {Hd}, R {R} is not taken in the current arithmetic / "
                         "edge-storage modes (ops.train_indexed_ok); densify")
    dev = x.device
    cls = _class_plan(index, plan, R)
    # (its exact size: E * H + N * H floats and padding -- alpha and ssum, all a layer keeps for its backward)
    saved = torch.empty(lib.cgat_nodes_attention_indexed_saved_floats(N, E, H, Hd), dtype=torch.float32, device=dev)
    aggr = torch.empty(N, x.shape[1], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws = workspace(lib.cgat_nodes_attention_forward_indexed_workspace_bytes(C.byref(plan.c), C.byref(p), R), dev)
        check(lib.cgat_nodes_attention_forward_indexed(C.byref(plan.c), C.byref(p), _ptr(x), _ptr(table), R, _ptr(index),
                                                       _ptr(aggr), _ptr(saved), _ptr(ws), ws.numel(), _stream()),
              "cgat_nodes_attention_forward_indexed")
    if debug.recording():
        debug.note_attention_indexed(A_in_w, M_in_w, plan, p, x, table, index)
    return aggr, saved, x, table, index, ws_, cls


def _attn_backward_indexed(x, table, index, cls, plan, H, weights, saved, g_aggr, stream):
    """cgat_nodes_attention_backward_indexed on `stream` (a raw handle).  Builds and validates nothing.  Returns (g_x,
    g_table, parameter grads)."""
    g_aggr = _f32c(g_aggr)
    p, _ = _attn_params(x, table, H, weights)
    dev, R = x.device, int(table.shape[0])
    g_x, g_t = torch.empty_like(x), torch.empty_like(table)
    grads = [_param_grad(w) for w in weights]
    g = _lib.AttnGrads(*[t.data_ptr() for t in grads])
    cls_pos, piece_rowptr, piece_start = cls
    with torch.cuda.device(dev):
        ws = workspace(lib.cgat_nodes_attention_backward_indexed_workspace_bytes(C.byref(plan.c), C.byref(p), R), dev)
        check(lib.cgat_nodes_attention_backward_indexed(C.byref(plan.c), C.byref(p), _ptr(x), _ptr(table), R, _ptr(index),
                                                        _ptr(cls_pos), _ptr(piece_rowptr), _ptr(piece_start), _ptr(saved),
                                                        _ptr(g_aggr), _ptr(g_x), _ptr(g_t), C.byref(g), _ptr(ws), ws.numel(),
                                                        stream), "cgat_nodes_attention_backward_indexed")
    return g_x, g_t, grads


class NodesAttentionIndexedFn(torch.autograd.Function):
    """NodesAttentionFn for edge_attr = table[index] (reference CGAT.py:319-329 on the lookup of 569 / 583) without the
    [E, Ce] edge features and without stored pre-activations: the forward is nodes_attention_infer_indexed's, bit for bit,
    keeping alpha and ssum; the backward forms S and z again from three gathered rows and returns g_x, g_table (the embedding
    backward included) and the eight parameter gradients."""

    @staticmethod
    def forward(ctx, x, table, index, plan, H, A_in_w, A_in_b, A_out_w, A_out_b, M_in_w, M_in_b, M_out_w, M_out_b):
        weights = [A_in_w, A_in_b, A_out_w, A_out_b, M_in_w, M_in_b, M_out_w, M_out_b]
        aggr, saved, x, table, index, weights, cls = _attn_forward_indexed(x, table, index, plan, H, weights)
        ctx.plan, ctx.H, ctx.cls = plan, H, cls
        ctx.save_for_backward(x, table, index, saved, *weights)
        return aggr

    @staticmethod
    def backward(ctx, g_aggr):
        x, table, index, saved, *weights = ctx.saved_tensors
        g_x, g_t, grads = _attn_backward_indexed(x, table, index, ctx.cls, ctx.plan, ctx.H, weights, saved, g_aggr, _stream())
        return (g_x, g_t, None, None, None, *grads)


def _edge_hidden_forward(who, x, edge_attr, plan, w_in, b_in):
    """cgat_edge_hidden_forward behind EdgeHiddenFn and EdgeHiddenHeadsFn.  Returns the prepared operands, hidden and
    hmax = max |hidden| (the fp16 scale of the second layers)."""
    x, edge_attr, w_in, b_in = _f32c(x), _f32c(edge_attr), _f32c(w_in.detach()), _f32c(b_in.detach())
    N, E = plan.N, plan.E
    Cn, Ce, W2 = x.shape[1], edge_attr.shape[1], w_in.shape[0]
    if x.shape[0] != N or edge_attr.shape[0] != E or w_in.shape[1] != 2 * Cn + Ce or b_in.numel() != W2:
        raise ValueError(f"{who}: shapes do not match the plan / the stacked first-layer weight")
    dev = x.device
    hidden = torch.empty(E, W2, dtype=torch.float32, device=dev)
    hmax = torch.empty(1, dtype=torch.float32, device=dev)
    ws = workspace(lib.cgat_edge_hidden_forward_workspace_bytes(C.byref(plan.c), Cn, Ce, W2), dev)
    with torch.cuda.device(dev):
        check(lib.cgat_edge_hidden_forward(C.byref(plan.c), Cn, Ce, W2, _ptr(w_in), _ptr(b_in), _ptr(x),
                                           _ptr(edge_attr), _ptr(hidden), _ptr(hmax), _ptr(ws), ws.numel(), _stream()),
              "cgat_edge_hidden_forward")
    return x, edge_attr, w_in, hidden, hmax


def _edge_hidden_backward(x, edge_attr, plan, w_in, hidden, g, g_is_pre, gmax):
    """cgat_edge_hidden_backward behind EdgeHiddenFn (g: the gradient of hidden) and EdgeHiddenHeadsFn (g_is_pre = 1: of
    the pre-activations, gmax its maximum).  Returns g_x, g_edge_attr, g_w_in, g_b_in."""
    Cn, Ce, W2 = x.shape[1], edge_attr.shape[1], w_in.shape[0]
    dev = x.device
    g_x, g_e = torch.empty_like(x), torch.empty_like(edge_attr)
    g_w, g_b = torch.empty_like(w_in), torch.empty(W2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws = workspace(lib.cgat_edge_hidden_backward_workspace_bytes(C.byref(plan.c), Cn, Ce, W2), dev)
        check(lib.cgat_edge_hidden_backward(C.byref(plan.c), Cn, Ce, W2, _ptr(w_in), _ptr(x), _ptr(edge_attr),
                                            _ptr(hidden), _ptr(g), g_is_pre, _ptr(gmax), _ptr(g_x), _ptr(g_e), _ptr(g_w),
                                            _ptr(g_b), _ptr(ws), ws.numel(), _stream()), "cgat_edge_hidden_backward")
    return g_x, g_e, g_w, g_b


class EdgeHiddenFn(torch.autograd.Function):
    """hidden[t] = LeakyReLU(w_in [x_i ; edge_attr ; x_j] + b_in) in destination-sorted slot order t (plan.dst_perm):
    the first layer of both message networks (reference CGAT.py:96,105-108 on the concatenated message of 316-318)
    with the operand split, for the vector-attention variants whose second layers need every hidden row."""

    @staticmethod
    def forward(ctx, x, edge_attr, plan, w_in, b_in):
        _require_gpu(x, edge_attr, w_in, b_in)
        x, edge_attr, w_in, hidden, hmax = _edge_hidden_forward("EdgeHiddenFn", x, edge_attr, plan, w_in, b_in)
        ctx.plan = plan
        ctx.save_for_backward(x, edge_attr, w_in, hidden)
        ctx.mark_non_differentiable(hmax)
        return hidden, hmax

    @staticmethod
    def backward(ctx, g_hidden, _g_hmax=None):
        x, edge_attr, w_in, hidden = ctx.saved_tensors
        g_x, g_e, g_w, g_b = _edge_hidden_backward(x, edge_attr, ctx.plan, w_in, hidden, _f32c(g_hidden), 0, None)
        return g_x, g_e, None, g_w, g_b


# ---- the same first layer on shell-indexed edge features (cgat_edge_hidden_forward_indexed / _backward_indexed) ----
_indexed_vector_attention = _Switch("CGAT_INDEXED_VECTOR_ATTN", False)


def set_indexed_vector_attention(flag):
    """The shell-indexed route of VECTOR-attention node layers (default off; env CGAT_INDEXED_VECTOR_ATTN=1 starts it on):
    such a layer given an IndexedEdgeAttr keeps it, with grad and without, and runs EdgeHiddenIndexedFn /
    EdgeHiddenHeadsIndexedFn -- Te = table W_e^T over R rows and a three-row gather in place of the per-edge K = Ce
    product, no [E, Ce] edge features (none saved either), grad table and grad W_e from a per-class row sum -- where the
    library takes the shape (edge_hidden_indexed_ok).  `hidden` [E, 2 H Hd] and everything behind it are unchanged.  It
    matters only where an IndexedEdgeAttr reaches the layer: through CGAtNet that needs set_indexed_edge_attr(True) too.
    Off: such a layer densifies and runs the dense launches, bit for bit."""
    _indexed_vector_attention.set(flag)


def get_indexed_vector_attention():
    return _indexed_vector_attention.value


def edge_hidden_indexed_ok(plan_c, C_, Ce, W2, R):
    """cgat_edge_hidden_indexed_ok for a first layer of these dims in the current edge-storage mode (host only; plan_c:
    the C struct of a plan)."""
    return bool(lib.cgat_edge_hidden_indexed_ok(C.byref(plan_c), int(C_), int(Ce), int(W2), int(R)))


def _edge_hidden_forward_indexed(who, x, table, index, plan, w_in, b_in):
    """cgat_edge_hidden_forward_indexed behind EdgeHiddenIndexedFn and EdgeHiddenHeadsIndexedFn.  Everything is checked
    before the first launch.  Returns the prepared operands, hidden, hmax and the class plan of the backward."""
    err = _indexed_operands_error(x, table, index, plan.N, plan.E)
    if err is not None:
        raise err
    _require_gpu(w_in, b_in)
    x, table, w_in, b_in = _f32c(x), _f32c(table), _f32c(w_in.detach()), _f32c(b_in.detach())
    N, E, R = plan.N, plan.E, int(table.shape[0])
    Cn, Ce, W2 = x.shape[1], table.shape[1], w_in.shape[0]
    if w_in.shape[1] != 2 * Cn + Ce or b_in.numel() != W2:
        raise ValueError(f"{who}: shapes do not match the stacked first-layer weight")
    if not edge_hidden_indexed_ok(plan.c, Cn, Ce, W2, R):
        raise ValueError(f"{who}: N {N}, E {E}, W2 {W2}, R {R} is not taken in the current edge-storage mode "
                         "(ops.edge_hidden_indexed_ok); densify")
    dev = x.device
    cls = _class_plan(index, plan, R)
    hidden = torch.empty(E, W2, dtype=torch.float32, device=dev)
    hmax = torch.empty(1, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws = workspace(lib.cgat_edge_hidden_forward_indexed_workspace_bytes(C.byref(plan.c), Cn, Ce, W2, R), dev)
        check(lib.cgat_edge_hidden_forward_indexed(C.byref(plan.c), Cn, Ce, W2, _ptr(w_in), _ptr(b_in), _ptr(x), _ptr(table),
                                                   R, _ptr(index), _ptr(hidden), _ptr(hmax), _ptr(ws), ws.numel(),
                                                   _stream()), "cgat_edge_hidden_forward_indexed")
    return x, table, w_in, hidden, hmax, cls


def _edge_hidden_backward_indexed(x, table, index, cls, plan, w_in, hidden, g, g_is_pre, gmax):
    """cgat_edge_hidden_backward_indexed.  Builds and validates nothing.  Returns g_x, g_table, g_w_in, g_b_in."""
    Cn, Ce, W2, R = x.shape[1], table.shape[1], w_in.shape[0], int(table.shape[0])
    dev = x.device
    g_x, g_t = torch.empty_like(x), torch.empty_like(table)
    g_w, g_b = torch.empty_like(w_in), torch.empty(W2, dtype=torch.float32, device=dev)
    cls_pos, piece_rowptr, piece_start = cls
    with torch.cuda.device(dev):
        ws = workspace(lib.cgat_edge_hidden_backward_indexed_workspace_bytes(C.byref(plan.c), Cn, Ce, W2, R), dev)
        check(lib.cgat_edge_hidden_backward_indexed(C.byref(plan.c), Cn, Ce, W2, _ptr(w_in), _ptr(x), _ptr(table), R,
                                                    _ptr(index), _ptr(cls_pos), _ptr(piece_rowptr), _ptr(piece_start),
                                                    _ptr(hidden), _ptr(g), g_is_pre, _ptr(gmax), _ptr(g_x), _ptr(g_t),
                                                    _ptr(g_w), _ptr(g_b), _ptr(ws), ws.numel(), _stream()),
              "cgat_edge_hidden_backward_indexed")
    return g_x, g_t, g_w, g_b


class EdgeHiddenIndexedFn(torch.autograd.Function):
    """EdgeHiddenFn for edge_attr = table[index] (reference CGAT.py:96,105-108 on the message of 316-318 with the lookups
    of 569 / 583) without the [E, Ce] edge features: hidden from three gathered rows, and a backward that returns g_x,
    g_table (the embedding backward included), g_w_in and g_b_in from segment sums and a per-class row sum.  Saves x, table,
    index, w_in and hidden."""

    @staticmethod
    def forward(ctx, x, table, index, plan, w_in, b_in):
        x, table, w_in, hidden, hmax, cls = _edge_hidden_forward_indexed("EdgeHiddenIndexedFn", x, table, index, plan,
                                                                         w_in, b_in)
        ctx.plan, ctx.cls = plan, cls
        ctx.save_for_backward(x, table, index, w_in, hidden)
        ctx.mark_non_differentiable(hmax)
        return hidden, hmax

    @staticmethod
    def backward(ctx, g_hidden, _g_hmax=None):
        x, table, index, w_in, hidden = ctx.saved_tensors
        g_x, g_t, g_w, g_b = _edge_hidden_backward_indexed(x, table, index, ctx.cls, ctx.plan, w_in, hidden,
                                                           _f32c(g_hidden), 0, None)
        return g_x, g_t, None, None, g_w, g_b


# ----------------------------------------------------------------------------------------
# hypernetwork Pooling_NN
# ----------------------------------------------------------------------------------------
def _hnet_struct(cls, W, n_fc, n_hyper, flat, damping):
    s = cls()
    if cls is _lib.HnetParams:
        s.W, s.n_fc, s.n_hyper = W, n_fc, n_hyper
    per = 2 * n_fc + 2
    for l in range(n_hyper):
        t = flat[l * per:(l + 1) * per]
        for k in range(n_fc):
            s.layer[l].fc_w[k] = t[k].data_ptr()
            s.layer[l].fc_b[k] = t[n_fc + k].data_ptr()
        s.layer[l].head_w = t[2 * n_fc].data_ptr()
        s.layer[l].head_b = t[2 * n_fc + 1].data_ptr()
    s.damping = None if damping is None else damping.data_ptr()
    return s


# Side stream for the hypernetwork's weight-gradient contractions (cgat_hnet_backward_overlapped, used by NodeLayerFn):
# they are off the critical path of the backward pass and matrix-core bound, the attention backward is HBM bound.
# Decided by same-box A/Bs per arithmetic mode: in the 22-bit "f16x3" mode the overlap is worth 0.5 ms of a 23.9 ms step
# (the batched dT launch on half of the chip beside the HBM-bound attention backward) and is the default.  In the default
# 24-bit "f16x3c" mode, since its dT is ONE batched launch (round 5), it is worth 0.5-0.9 ms of 30.0 (29.0-29.5 vs
# 29.9-30.0 ms: the HBM-bound segment backward, source-side sums and dense weight gradients lose little on the other half
# of the chip; profiles/r05_side_stream_sweep.txt) -- opt-in there (CGAT_OVERLAP_WGRAD=1 / set_overlap_wgrad(True)): on
# half of the chip the dominant kernel's launch takes 8.2-8.8 ms instead of 4.6, and the step's per-kernel durations --
# the bench line's roofline, the rocprof statistics -- stop being statements about the kernels; the default keeps every
# kernel alone on the chip.  "bf16x6" (four six-pass dT launches, two to four times as long as the kernels they would
# run beside) gains nothing: 33.13 / 33.12 ms with, 33.04 / 33.08 without.
_side_streams = {}
_overlap_wgrad = _Switch("CGAT_OVERLAP_WGRAD", None)


def set_overlap_wgrad(flag):
    _overlap_wgrad.set(flag)


def get_overlap_wgrad():
    """The raw setting (None = decided per arithmetic mode): what a caller that changes it temporarily must restore."""
    return _overlap_wgrad.value


def overlap_enabled():
    if _overlap_wgrad.value is None:
        return get_bilinear_mode() == "f16x3"
    return _overlap_wgrad.value


def side_stream(device, create=True):
    """The per-device side stream (None if it has never been used and create is False)."""
    dev = torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    if key not in _side_streams and create:
        _side_streams[key] = torch.cuda.Stream(device=dev)
    return _side_streams.get(key)


_branch_streams = {}
_BRANCH_MAX_EDGES = 262144


def branch_stream(device, n_edges, which=0):
    """The stream independent sub-networks run on beside the main stream at SMALL batches (CGAtNet: the composition
    branch beside the graph layers) -- or None when the batch is large enough for every kernel to fill the chip by
    itself.  At the harness' shipped batch (64 crystals) a kernel occupies 5-40 of the 256 CUs for as long as one
    workgroup needs for its serial chain, so two independent chains side by side cost the longer one, not the sum
    (SURVEY 8 f3).  Works eagerly and under hipGraph capture (fork / join by events); autograd runs each node's backward
    on its forward's stream, so the backward overlaps the same way."""
    if n_edges > _BRANCH_MAX_EDGES:
        return None
    dev = torch.device(device)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), which)
    if key not in _branch_streams:
        _branch_streams[key] = torch.cuda.Stream(device=dev)
    return _branch_streams[key]


def aux_streams():
    """Every stream this package may have issued gradient-producing work on besides the caller's (dist.py makes a
    collective wait for them)."""
    return list(_branch_streams.values()) + list(_side_streams.values())


def _hnet_forward(h0, v, damping, n_fc, n_hyper, flat):
    """cgat_hnet_forward behind HNetFn and NodeLayerFn.  Returns (y, saved, prepared damping or None, prepared flat)."""
    _require_gpu(h0, v, *flat)
    flat = [_f32c(t.detach()) for t in flat]
    d = None if damping is None else _f32c(damping.detach())
    rows, W = v.shape
    if h0.shape != v.shape:
        raise ValueError("hypernetwork: h0 and v must both be [rows, W]")
    for l in range(n_hyper):
        hw = flat[l * (2 * n_fc + 2) + 2 * n_fc]
        if tuple(hw.shape) != (W * W + W, W):
            raise ValueError(f"hypernetwork head weight must be [{W * W + W}, {W}] (all widths equal), got {tuple(hw.shape)}")
    p = _hnet_struct(_lib.HnetParams, W, n_fc, n_hyper, flat, d)
    dev = v.device
    saved = _scratch(lib.cgat_hnet_saved_floats(rows, C.byref(p)), torch.float32, dev)
    y = torch.empty_like(v)
    with torch.cuda.device(dev):
        ws = workspace(lib.cgat_hnet_forward_workspace_bytes(rows, C.byref(p)), dev)
        check(lib.cgat_hnet_forward(rows, C.byref(p), _ptr(h0), _ptr(v), _ptr(y), _ptr(saved), _ptr(ws), ws.numel(),
                                    _stream()), "cgat_hnet_forward")
    return y, saved, d, flat


def _hnet_backward(h0, v, saved, d, flat, n_fc, n_hyper, g_y, side=None):
    """cgat_hnet_backward, or -- side = (main stream, side stream) -- cgat_hnet_backward_overlapped, which leaves the
    weight-gradient contractions on the side stream for the caller to join.  Returns (g_h0, g_v, g_d or None, grads,
    side_ws): the caller MUST keep side_ws alive until the main stream has waited for the side stream."""
    rows, W = v.shape
    g_y = _f32c(g_y)
    p = _hnet_struct(_lib.HnetParams, W, n_fc, n_hyper, flat, d)
    grads = [_param_grad(t) for t in flat]
    g_d = torch.empty_like(d) if d is not None else None
    g = _hnet_struct(_lib.HnetGrads, W, n_fc, n_hyper, grads, g_d)
    g_h0, g_v = torch.empty_like(h0), torch.empty_like(v)
    dev = v.device
    side_ws = None
    with torch.cuda.device(dev):
        ws = workspace(lib.cgat_hnet_backward_workspace_bytes(rows, C.byref(p)), dev)
        if side is None:
            check(lib.cgat_hnet_backward(rows, C.byref(p), _ptr(h0), _ptr(v), _ptr(saved), _ptr(g_y), _ptr(g_h0),
                                         _ptr(g_v), C.byref(g), _ptr(ws), ws.numel(), _stream()), "cgat_hnet_backward")
        else:
            main, s2 = side
            # side_ws (the side stream's inputs and scratch: g_u, g_pre, the dw slabs, the dT workspace) is its own
            # allocation: the attention backward reuses the cached main workspace while the side stream is still running.
            # It is allocated on the main stream and read and written on the side stream, so it has to outlive the join:
            # dropped earlier, the allocator hands its block to the next main-stream allocation
            side_ws = _scratch(lib.cgat_hnet_backward_side_workspace_bytes(rows, C.byref(p)), torch.uint8, dev)
            check(lib.cgat_hnet_backward_overlapped(rows, C.byref(p), _ptr(h0), _ptr(v), _ptr(saved), _ptr(g_y),
                                                    _ptr(g_h0), _ptr(g_v), C.byref(g), _ptr(ws), ws.numel(),
                                                    main.cuda_stream, _ptr(side_ws), side_ws.numel(), s2.cuda_stream),
                  "cgat_hnet_backward_overlapped")
    return g_h0, g_v, g_d, grads, side_ws


class HNetFn(torch.autograd.Function):
    """y = HyperFC(hyper_input)(v)  with hyper_input = h0 (H_Net_0) or d*h0 + (1-d)*v (H_Net);
    reference Hypernetworksmp.py:257-313.  `flat` = per predicted layer: n_fc trunk weights,
    n_fc trunk biases, head weight [W*W+W, W], head bias [W*W+W]."""

    @staticmethod
    def forward(ctx, h0, v, damping, n_fc, n_hyper, *flat):
        h0, v = _f32c(h0), _f32c(v)
        y, saved, d, flat = _hnet_forward(h0, v, damping, n_fc, n_hyper, flat)
        ctx.n_fc, ctx.n_hyper, ctx.has_d = n_fc, n_hyper, d is not None
        ctx.save_for_backward(h0, v, saved, *([d] if d is not None else []), *flat)
        return y

    @staticmethod
    def backward(ctx, g_y):
        h0, v, saved, *rest = ctx.saved_tensors
        d = rest.pop(0) if ctx.has_d else None
        g_h0, g_v, g_d, grads, _ = _hnet_backward(h0, v, saved, d, rest, ctx.n_fc, ctx.n_hyper, g_y)
        return (g_h0, g_v, g_d, None, None, *grads)


def _layer_backward(ctx, h0, aggr, saved_h, d, flat, g_y, attn_backward, overlap):
    """The backward schedule of a whole-layer node (NodeLayerFn, NodeLayerIndexedFn): the hypernetwork backward first --
    overlap: cgat_hnet_backward_overlapped, its weight-gradient contractions left on the side stream --, then
    `attn_backward(g_aggr, raw main stream)` on the main stream, then the join.  Returns (g_h0, g_d, the hypernetwork's
    parameter grads, what attn_backward returned)."""
    dev = aggr.device
    main = torch.cuda.current_stream(dev)
    side = (main, side_stream(dev)) if overlap else None
    # the hypernetwork's workspace is taken and its call issued first, then the attention backward takes its workspace
    # from the same cache (main-stream order; what the side stream reads is its own allocation)
    g_h0, g_aggr, g_d, g_flat, side_ws = _hnet_backward(h0, aggr, saved_h, d, flat, ctx.n_fc, ctx.n_hyper, g_y, side=side)
    g_attn = attn_backward(g_aggr, main.cuda_stream)
    if overlap:
        with torch.cuda.device(dev):
            main.wait_stream(side[1])    # every gradient is complete, in stream order, when this node returns
    del side_ws                          # (held until here: the side stream was using it)
    return g_h0, g_d, g_flat, g_attn


class NodeLayerFn(torch.autograd.Function):
    """One whole GATConvNodes layer: aggr = attention(x, edge_attr) (NodesAttentionFn), y = HyperFC(h0)(aggr) (HNetFn) --
    reference CGAT.py:307-340 -- as ONE autograd node, so that its backward can run the hypernetwork's four
    weight-gradient contractions (matrix-core bound, feeding nothing else) on a side stream BESIDE the attention
    backward (HBM bound) and join the two streams before returning.  Same kernels, same results as the two separate
    nodes; only the schedule differs."""

    @staticmethod
    def forward(ctx, x, edge_attr, h0, plan, H, damping, n_fc, n_hyper, *params):
        _require_gpu(x, edge_attr, h0, *params)
        x, edge_attr, h0 = _f32c(x), _f32c(edge_attr), _f32c(h0)
        if x.shape[0] != plan.N or edge_attr.shape[0] != plan.E or h0.shape != x.shape:
            raise ValueError("NodeLayerFn: shapes do not match the plan")
        aggr, saved_a, attn_w = _attn_forward(x, edge_attr, plan, H, params[:8], save=True)
        y, saved_h, d, flat = _hnet_forward(h0, aggr, damping, n_fc, n_hyper, params[8:])
        ctx.plan, ctx.H, ctx.n_fc, ctx.n_hyper, ctx.has_d = plan, H, n_fc, n_hyper, d is not None
        ctx.storage = lib.cgat_get_edge_storage()
        ctx.save_for_backward(x, edge_attr, h0, aggr, saved_a, saved_h, *([d] if d is not None else []), *attn_w, *flat)
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, edge_attr, h0, aggr, saved_a, saved_h, *rest = ctx.saved_tensors
        d = rest.pop(0) if ctx.has_d else None
        attn_w, flat = rest[:8], rest[8:]
        attn = lambda g_aggr, stream: _attn_backward(x, edge_attr, ctx.plan, ctx.H, attn_w, saved_a, g_aggr, ctx.storage,
                                                     stream)
        g_h0, g_d, g_flat, (g_x, g_e, g_attn) = _layer_backward(ctx, h0, aggr, saved_h, d, flat, g_y, attn, overlap=True)
        return (g_x, g_e, g_h0, None, None, g_d, None, None, *g_attn, *g_flat)


def _overlapped_hnet_keeps_bits(v):
    """True where cgat_hnet_backward_overlapped gives the bits of cgat_hnet_backward: the batched fp16 forms of the
    weight-gradient contraction ("f16x3", "f16x3c" at width 128), whose row split does not follow the grid.  Under the
    six-pass plane forms ("bf16x6", "bf16x3") the side stream's half-chip grid halves the split and the sums differ in the
    last bits (test_hip_golden.py::test_side_stream_equals_serial holds NodeLayerFn to 1e-5 there)."""
    return get_bilinear_mode() in ("f16x3", "f16x3c") and v.shape[1] == 128


class NodeLayerIndexedFn(torch.autograd.Function):
    """NodeLayerFn for edge_attr = table[index]: aggr = NodesAttentionIndexedFn, y = HyperFC(h0)(aggr) as ONE autograd node
    with the same schedule -- the hypernetwork's weight-gradient contractions on the side stream beside the attention
    backward, joined before returning -- wherever that schedule keeps the bits of the two separate nodes
    (_overlapped_hnet_keeps_bits); elsewhere the two backward calls run one after the other.  Bit-equal to
    NodesAttentionIndexedFn + HNetFn in every arithmetic mode."""

    @staticmethod
    def forward(ctx, x, table, index, h0, plan, H, damping, n_fc, n_hyper, *params):
        _require_gpu(h0)
        h0 = _f32c(h0)
        if h0.shape != x.shape:
            raise ValueError("NodeLayerIndexedFn: shapes do not match the plan")
        aggr, saved_a, x, table, index, attn_w, cls = _attn_forward_indexed(x, table, index, plan, H, list(params[:8]))
        y, saved_h, d, flat = _hnet_forward(h0, aggr, damping, n_fc, n_hyper, params[8:])
        ctx.plan, ctx.H, ctx.n_fc, ctx.n_hyper, ctx.has_d, ctx.cls = plan, H, n_fc, n_hyper, d is not None, cls
        ctx.save_for_backward(x, table, index, h0, aggr, saved_a, saved_h, *([d] if d is not None else []), *attn_w, *flat)
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, table, index, h0, aggr, saved_a, saved_h, *rest = ctx.saved_tensors
        d = rest.pop(0) if ctx.has_d else None
        attn_w, flat = rest[:8], rest[8:]
        attn = lambda g_aggr, stream: _attn_backward_indexed(x, table, index, ctx.cls, ctx.plan, ctx.H, attn_w, saved_a,
                                                             g_aggr, stream)
        # the overlapped hypernetwork backward caps the grid of its weight-gradient launches; where that cap moves the row
        # split of their sums (the six-pass plane forms, other widths) the serial call runs: HNetFn's bits
        g_h0, g_d, g_flat, (g_x, g_t, g_attn) = _layer_backward(ctx, h0, aggr, saved_h, d, flat, g_y, attn,
                                                                overlap=_overlapped_hnet_keeps_bits(aggr))
        return (g_x, g_t, None, g_h0, None, None, g_d, None, None, *g_attn, *g_flat)


# ----------------------------------------------------------------------------------------
# dense layer, segment ops
# ----------------------------------------------------------------------------------------
class LinearFn(torch.autograd.Function):
    """y = act(x W^T + b); x [M,K], W [N,K] (any leading stride), act in {none,tanh,leaky,relu}."""

    @staticmethod
    def forward(ctx, x, w, b, act):
        _require_gpu(x, w, b)
        # a column slice of a wider matrix (one head's hidden block) is passed with its row stride, not copied
        if not (x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and
                x.data_ptr() % 16 == 0):
            x = _f32c(x)
        w2 = w.detach().reshape(w.shape[0], -1)
        if w2.stride(1) != 1:
            w2 = w2.contiguous()
        if w2.dtype != torch.float32:
            raise TypeError("weights must be float32")
        bb = None if b is None else _f32c(b.detach())
        M, K = x.shape
        N = w2.shape[0]
        y = torch.empty(M, N, dtype=torch.float32, device=x.device)
        ws = workspace(lib.cgat_linear_forward_workspace_bytes(M, K, N), x.device)
        with torch.cuda.device(x.device):
            check(lib.cgat_linear_forward(_ptr(x), x.stride(0), _ptr(w2), w2.stride(0), _ptr(bb), _ptr(y), N, M, K, N, act,
                                          None, _ptr(ws), ws.numel(), _stream()), "cgat_linear_forward")
        ctx.act, ctx.has_b, ctx.wshape = act, b is not None, w.shape
        ctx.save_for_backward(x, w2, y)
        if act in (_lib.ACT_LEAKY, _lib.ACT_RELU) and debug.recording():
            debug.note(w, y > 0)
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, w2, y = ctx.saved_tensors
        g_y = _f32c(g_y)
        M, K = x.shape
        N = w2.shape[0]
        dev = x.device
        gpre = torch.empty_like(y) if ctx.act != _lib.ACT_NONE else None
        g_x = torch.empty(M, K, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        g_w = torch.empty(N, K, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        g_b = torch.empty(N, dtype=torch.float32, device=dev) if (ctx.has_b and ctx.needs_input_grad[2]) else None
        ws = workspace(lib.cgat_linear_backward_workspace_bytes(M, K, N), dev)
        with torch.cuda.device(dev):
            check(lib.cgat_linear_backward(_ptr(x), x.stride(0), _ptr(w2), w2.stride(0), _ptr(y), N, _ptr(g_y), N, _ptr(gpre),
                                           _ptr(g_x), K, 0, _ptr(g_w), K, _ptr(g_b), M, K, N, ctx.act, _ptr(ws),
                                           ws.numel(), _stream()), "cgat_linear_backward")
        return g_x, (None if g_w is None else g_w.reshape(ctx.wshape)), g_b, None


def _cos(Co, n):
    """Output width per network: one int for all, or one per network (scalar attention: 1 for MH_A, C for MH_M)."""
    return tuple(Co) if isinstance(Co, (tuple, list)) else (Co,) * n


def _heads_forward(hid, nets, H, Hd, Co, hmax=None):
    """nets: list of (weight [H*Co, Hd], bias [H*Co] or None); network i reads columns [i*H*Hd, (i+1)*H*Hd) of hid.
    hmax: device scalar max |hid| (EdgeHiddenFn's second output), which lets the Hd > 128 products run in the f16x3 form."""
    E, W2 = hid.shape
    cos = _cos(Co, len(nets))
    outs = [torch.empty(E, H * co, dtype=torch.float32, device=hid.device) for co in cos]
    ws = workspace(max(lib.cgat_heads_linear_forward_workspace_bytes(E, Hd, co, H) for co in cos), hid.device)
    with torch.cuda.device(hid.device):
        for net, (w, b) in enumerate(nets):
            Co = cos[net]
            # the H heads of a network as ONE call: head h reads the column block (net * H + h) * Hd of hid, rows
            # [h * Co, (h + 1) * Co) of the weight / bias, and writes columns [h * Co, (h + 1) * Co) of the output
            check(lib.cgat_heads_linear_forward(_ptr(hid[:, net * H * Hd:]), W2, Hd, _ptr(w), Hd, Co * Hd, _ptr(b), Co,
                                                _ptr(outs[net]), H * Co, Co, E, Hd, Co, H, _ptr(hmax), _ptr(ws), ws.numel(),
                                                _stream()), "cgat_heads_linear_forward")
    return outs


def _heads_backward(hid, weights, has_b, grads, H, Hd, Co, need_hid):
    E, W2 = hid.shape
    dev = hid.device
    cos = _cos(Co, len(weights))
    gs = [_f32c(g.reshape(E, H * co)) for g, co in zip(grads, cos)]
    g_hid = torch.empty_like(hid) if need_hid else None
    g_w = [torch.empty(H * co, Hd, dtype=torch.float32, device=dev) for co in cos]
    g_b = [torch.empty(H * co, dtype=torch.float32, device=dev) if hb else None for hb, co in zip(has_b, cos)]
    ws = workspace(max(lib.cgat_linear_backward_workspace_bytes(E, Hd, co) for co in cos), dev)
    with torch.cuda.device(dev):
        for net, w in enumerate(weights):
            Co = cos[net]
            for h in range(H):
                col = (net * H + h) * Hd
                check(lib.cgat_linear_backward(_ptr(hid[:, col:col + Hd]), W2, _ptr(w[h * Co:(h + 1) * Co]), Hd, None, Co,
                                               _ptr(gs[net][:, h * Co:(h + 1) * Co]), H * Co, None,
                                               None if g_hid is None else _ptr(g_hid[:, col:col + Hd]), W2, 0,
                                               _ptr(g_w[net][h * Co:(h + 1) * Co]), Hd,
                                               None if g_b[net] is None else _ptr(g_b[net][h * Co:(h + 1) * Co]),
                                               E, Hd, Co, _lib.ACT_NONE, _ptr(ws), ws.numel(), _stream()),
                      "cgat_linear_backward")
    return g_hid, g_w, g_b


class HeadsLinearFn(torch.autograd.Function):
    """Second layers of two multi-head networks on one hidden matrix (vector attention, reference CGAT.py:97-98,
    103-109 applied per head): out_A[:, h, :] = hid[:, h*Hd:(h+1)*Hd] W_A[h]^T + b_A[h], out_M the same on the second
    half of the columns.  One autograd node for all 2H slices: the backward writes every head's input gradient
    straight into its column block of ONE [E, 2*H*Hd] buffer -- per-slice autograd nodes made torch zero-fill and add
    a full-size 6 GB gradient per head (21 ms of a 75 ms step at E = 1M)."""

    @staticmethod
    def forward(ctx, hid, wa, ba, wm, bm, H, Hd, Co, hmax=None):
        _require_gpu(hid, wa, wm)
        hid = _f32c(hid)
        E = hid.shape[0]
        cos = _cos(Co, 2)                   # (Co may be a pair: scalar attention's MH_A emits one logit per head)
        ws_ = [_f32c(w.detach().reshape(H * co, Hd)) for w, co in zip((wa, wm), cos)]
        bs_ = [None if b is None else _f32c(b.detach()) for b in (ba, bm)]
        outs = _heads_forward(hid, list(zip(ws_, bs_)), H, Hd, cos, hmax)
        ctx.dims = (H, Hd, cos)
        ctx.shapes = (wa.shape, wm.shape)
        ctx.has_b = (ba is not None, bm is not None)
        ctx.save_for_backward(hid, ws_[0], ws_[1])
        return outs[0].reshape(E, H, cos[0]), outs[1].reshape(E, H, cos[1])

    @staticmethod
    def backward(ctx, g_a, g_m):
        hid, w0, w1 = ctx.saved_tensors
        H, Hd, Co = ctx.dims
        g_hid, g_w, g_b = _heads_backward(hid, (w0, w1), ctx.has_b, (g_a, g_m), H, Hd, Co, ctx.needs_input_grad[0])
        return (g_hid, g_w[0].reshape(ctx.shapes[0]), g_b[0], g_w[1].reshape(ctx.shapes[1]), g_b[1], None, None, None, None)


def _hidden_heads_forward(ctx, hidden, hmax, wa, ba, wm, bm, H, Hd, Co):
    """The second-layer half of EdgeHiddenHeadsFn / EdgeHiddenHeadsIndexedFn's forward on a fresh `hidden`: sets ctx.dims,
    .shapes, .has_b and returns (out_A [E, H, Co_A], out_M [E, H, Co_M], the two prepared head weights to save)."""
    E = hidden.shape[0]
    cos = _cos(Co, 2)
    ws_ = [_f32c(w.detach().reshape(H * co, Hd)) for w, co in zip((wa, wm), cos)]
    bs_ = [None if b is None else _f32c(b.detach()) for b in (ba, bm)]
    outs = _heads_forward(hidden, list(zip(ws_, bs_)), H, Hd, cos, hmax)
    ctx.dims = (H, Hd, cos)
    ctx.shapes = (wa.shape, wm.shape)
    ctx.has_b = (ba is not None, bm is not None)
    if debug.recording():
        debug.last_hidden = hidden             # the calling module records the derivative pattern under its weights' names
    return outs[0].reshape(E, H, cos[0]), outs[1].reshape(E, H, cos[1]), ws_[0], ws_[1]


def _hidden_heads_backward(ctx, hidden, w0, w1, g_a, g_m):
    """The second layers' backward with LeakyReLU' folded in (cgat_heads_linear_backward_dact): returns gpre (the gradient of
    the PRE-activations, written head by head), its device maximum and the head weights' / biases' gradients."""
    H, Hd, cos = ctx.dims
    E, W2 = hidden.shape
    dev = hidden.device
    gs = [_f32c(g.reshape(E, H * co)) for g, co in zip((g_a, g_m), cos)]
    gpre = torch.empty_like(hidden)
    gmax = torch.zeros(1, dtype=torch.float32, device=dev)
    g_w = [torch.empty(H * co, Hd, dtype=torch.float32, device=dev) for co in cos]
    g_b = [torch.empty(H * co, dtype=torch.float32, device=dev) if hb else None for hb, co in zip(ctx.has_b, cos)]
    ws = workspace(max(lib.cgat_heads_linear_backward_dact_workspace_bytes(E, Hd, co, H) for co in cos), dev)
    with torch.cuda.device(dev):
        for net, w in enumerate((w0, w1)):
            Co = cos[net]
            col = net * H * Hd
            check(lib.cgat_heads_linear_backward_dact(
                _ptr(hidden[:, col:]), W2, Hd, _ptr(w), Hd, Co * Hd, _ptr(gs[net]), H * Co, Co,
                _ptr(gpre[:, col:]), W2, Hd, _ptr(hidden[:, col:]), W2, Hd, _ptr(gmax), _ptr(g_w[net]), Hd, Co * Hd,
                _ptr(g_b[net]), Co, E, Hd, Co, H, _ptr(ws), ws.numel(), _stream()), "cgat_heads_linear_backward_dact")
    return gpre, gmax, g_w, g_b


class EdgeHiddenHeadsFn(torch.autograd.Function):
    """EdgeHiddenFn followed by HeadsLinearFn as ONE autograd node (vector attention: both networks' first layers on
    [x_i; edge_attr; x_j], then the 2H per-head second layers; reference CGAT.py:96-109 on the message of 316-318).
    Same forward kernels; the point is the backward: the second layers' input gradient g_hid = g W is the gradient of a
    LeakyReLU OUTPUT, and autograd turns it into the pre-activation gradient with an elementwise pass over [E, 2 H Hd]
    (30 GB per layer at the harness-default shape: 12 % of its step).  Here the product's epilogue multiplies by
    LeakyReLU'(sign of hidden) and takes the tensor maximum on the way (cgat_linear_backward_dact), and the first
    layers' backward consumes the result as it is (cgat_edge_hidden_backward, g_is_pre = 1)."""

    @staticmethod
    def eligible(hid_width, H, Hd, cos):
        return (get_bilinear_mode() != "f32" and Hd % 128 == 0 and all(co == 128 for co in cos) and
                hid_width == 2 * H * Hd)

    @staticmethod
    def forward(ctx, x, edge_attr, plan, w_in, b_in, wa, ba, wm, bm, H, Hd, Co):
        _require_gpu(x, edge_attr, w_in, b_in, wa, wm)
        x, edge_attr, w_in, hidden, hmax = _edge_hidden_forward("EdgeHiddenHeadsFn", x, edge_attr, plan, w_in, b_in)
        ctx.plan = plan
        sa, sm, w0, w1 = _hidden_heads_forward(ctx, hidden, hmax, wa, ba, wm, bm, H, Hd, Co)
        ctx.save_for_backward(x, edge_attr, w_in, hidden, w0, w1)
        return sa, sm

    @staticmethod
    def backward(ctx, g_a, g_m):
        x, edge_attr, w_in, hidden, w0, w1 = ctx.saved_tensors
        gpre, gmax, g_w, g_b = _hidden_heads_backward(ctx, hidden, w0, w1, g_a, g_m)
        g_x, g_e, g_win, g_bin = _edge_hidden_backward(x, edge_attr, ctx.plan, w_in, hidden, gpre, 1, gmax)
        return (g_x, g_e, None, g_win, g_bin, g_w[0].reshape(ctx.shapes[0]), g_b[0], g_w[1].reshape(ctx.shapes[1]), g_b[1],
                None, None, None)


class EdgeHiddenHeadsIndexedFn(torch.autograd.Function):
    """EdgeHiddenHeadsFn for edge_attr = table[index]: EdgeHiddenIndexedFn's first layer, the same second layers, and the
    backward's g_is_pre = 1 form (cgat_heads_linear_backward_dact, then cgat_edge_hidden_backward_indexed) -- the form the
    harness-default shape takes.  Saves x, table, index, w_in, hidden and the head weights: no [E, Ce] tensor."""

    eligible = staticmethod(EdgeHiddenHeadsFn.eligible)

    @staticmethod
    def forward(ctx, x, table, index, plan, w_in, b_in, wa, ba, wm, bm, H, Hd, Co):
        _require_gpu(wa, wm)
        x, table, w_in, hidden, hmax, cls = _edge_hidden_forward_indexed("EdgeHiddenHeadsIndexedFn", x, table, index,
                                                                         plan, w_in, b_in)
        ctx.plan, ctx.cls = plan, cls
        sa, sm, w0, w1 = _hidden_heads_forward(ctx, hidden, hmax, wa, ba, wm, bm, H, Hd, Co)
        ctx.save_for_backward(x, table, index, w_in, hidden, w0, w1)
        return sa, sm

    @staticmethod
    def backward(ctx, g_a, g_m):
        x, table, index, w_in, hidden, w0, w1 = ctx.saved_tensors
        gpre, gmax, g_w, g_b = _hidden_heads_backward(ctx, hidden, w0, w1, g_a, g_m)
        g_x, g_t, g_win, g_bin = _edge_hidden_backward_indexed(x, table, index, ctx.cls, ctx.plan, w_in, hidden, gpre, 1,
                                                               gmax)
        return (g_x, g_t, None, None, g_win, g_bin, g_w[0].reshape(ctx.shapes[0]), g_b[0], g_w[1].reshape(ctx.shapes[1]),
                g_b[1], None, None, None)


class HeadsLinear1Fn(torch.autograd.Function):
    """The same for one network: out[:, h, :] = hid[:, h*Hd:(h+1)*Hd] W[h]^T + b[h] (MultiHeadNetwork.fc_out)."""

    @staticmethod
    def forward(ctx, hid, w, b, H, Hd, Co):
        _require_gpu(hid, w)
        hid = _f32c(hid)
        E = hid.shape[0]
        w2 = _f32c(w.detach().reshape(H * Co, Hd))
        bb = None if b is None else _f32c(b.detach())
        out = _heads_forward(hid, [(w2, bb)], H, Hd, Co)[0]
        ctx.dims = (H, Hd, Co)
        ctx.wshape = w.shape
        ctx.has_b = b is not None
        ctx.save_for_backward(hid, w2)
        return out.reshape(E, H, Co)

    @staticmethod
    def backward(ctx, g):
        hid, w2 = ctx.saved_tensors
        H, Hd, Co = ctx.dims
        g_hid, g_w, g_b = _heads_backward(hid, (w2,), (ctx.has_b,), (g,), H, Hd, Co, ctx.needs_input_grad[0])
        return g_hid, g_w[0].reshape(ctx.wshape), g_b[0], None, None, None


class SmallEmbeddingFn(torch.autograd.Function):
    """table[idx] for a small table looked up once per edge (nn.Embedding(neighbor_number + 1, Ce) in CGAtNet): the
    forward is a row gather, the backward a deterministic per-class row sum (cgat_embedding_backward) instead of
    torch's sort + atomic scatter."""

    @staticmethod
    def forward(ctx, idx, table):
        _require_gpu(idx, table)
        ctx.save_for_backward(idx)
        ctx.tshape = table.shape
        return table.detach().index_select(0, idx.reshape(-1)).reshape(*idx.shape, table.shape[1])

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        K, Cc = ctx.tshape
        g2 = _f32c(g.reshape(-1, Cc))
        ii = idx.reshape(-1).contiguous()
        out = torch.empty(K, Cc, dtype=torch.float32, device=g2.device)
        ws = workspace(lib.cgat_embedding_backward_workspace_bytes(K, Cc), g2.device)
        with torch.cuda.device(g2.device):
            check(lib.cgat_embedding_backward(_ptr(g2), Cc, _ptr(ii), g2.shape[0], K, Cc, _ptr(out), _ptr(ws), ws.numel(),
                                              _stream()), "cgat_embedding_backward")
        return None, out


def small_embedding(idx, table):
    """nn.Embedding lookup with the deterministic backward when the table is small enough, F.embedding otherwise."""
    if (table.is_cuda and idx.dtype == torch.int64 and table.dtype == torch.float32 and table.shape[1] <= 128 and
            table.shape[0] * table.shape[1] <= 8192):
        return SmallEmbeddingFn.apply(idx, table)
    return torch.nn.functional.embedding(idx, table)


def linear(x, w, b=None, act=_lib.ACT_NONE):
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1])
    if rowprog.eligible(x2):
        # a few hundred rows: one wave per 16 x 16 output tile (csrc/rowprog.hip), one launch per direction
        (y,) = rowprog.RowNetsFn.apply(x2, None, (((act, 0, b is not None),),), w, b, None)
        return y.reshape(*lead, y.shape[-1])
    y = LinearFn.apply(x.reshape(-1, x.shape[-1]), w, b, act)
    return y.reshape(*lead, y.shape[-1])


class SegmentSoftmaxFn(torch.autograd.Function):
    """alpha = mult * exp(a - segmax) / (segsum + eps) over CSR-ordered rows [R, F]."""

    @staticmethod
    def forward(ctx, a, mult, rowptr, eps):
        _require_gpu(a, mult, rowptr)
        a = _f32c(a)
        m = None if mult is None else _f32c(mult)
        R, F = a.shape
        S = rowptr.numel() - 1
        alpha = torch.empty_like(a)
        with torch.cuda.device(a.device):
            check(lib.cgat_segment_softmax_forward(_ptr(a), _ptr(m), _ptr(rowptr), S, F, eps, _ptr(alpha), _stream()),
                  "cgat_segment_softmax_forward")
        ctx.has_m = m is not None
        ctx.save_for_backward(alpha, rowptr, *([m] if m is not None else []))
        return alpha

    @staticmethod
    def backward(ctx, g_alpha):
        alpha, rowptr, *rest = ctx.saved_tensors
        m = rest[0] if ctx.has_m else None
        g_alpha = _f32c(g_alpha)
        R, F = alpha.shape
        S = rowptr.numel() - 1
        g_a = torch.empty_like(alpha)
        g_m = torch.empty_like(m) if (m is not None and ctx.needs_input_grad[1]) else None
        with torch.cuda.device(alpha.device):
            check(lib.cgat_segment_softmax_backward(_ptr(alpha), _ptr(g_alpha), _ptr(m), _ptr(rowptr), S, F, _ptr(g_a),
                                                    _ptr(g_m), _stream()), "cgat_segment_softmax_backward")
        return g_a, g_m, None, None


class SegmentSumFn(torch.autograd.Function):
    """out[s] = sum of the CSR-ordered rows of segment s; backward = broadcast."""

    @staticmethod
    def forward(ctx, x, rowptr, seg_of_row):
        _require_gpu(x, rowptr)
        x = _f32c(x)
        R, F = x.shape
        S = rowptr.numel() - 1
        out = torch.empty(S, F, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            check(lib.cgat_segment_sum(_ptr(x), F, None, _ptr(rowptr), S, F, _ptr(out), F, _stream()), "cgat_segment_sum")
        ctx.save_for_backward(seg_of_row)
        return out

    @staticmethod
    def backward(ctx, g):
        (seg_of_row,) = ctx.saved_tensors
        return g.index_select(0, seg_of_row), None, None


def _chain_desc(rows, x, layers, in_dact=None, in_dact_type=0, in_store=None):
    """cgat_chain_desc from python values; `layers` = dicts with W, transposed, bias, act, dact, dact_type, resid, out,
    accumulate (tensors are 2-D row-major [rows,128] / [128,128])."""
    d = _lib.ChainDesc()
    d.n_layers, d.rows = len(layers), rows
    d.x, d.ldx = x.data_ptr(), x.stride(0)
    if in_dact is not None:
        d.in_dact, d.ld_in_dact, d.in_dact_type = in_dact.data_ptr(), in_dact.stride(0), in_dact_type
    if in_store is not None:
        d.in_store, d.ld_in_store = in_store.data_ptr(), in_store.stride(0)
    for i, L in enumerate(layers):
        c = d.layer[i]
        W = L["W"]
        c.W = W.data_ptr()
        c.w_so, c.w_sk = (1, W.stride(0)) if L.get("transposed") else (W.stride(0), 1)
        for k in ("dact", "resid", "out"):
            if L.get(k) is not None:
                setattr(c, k, L[k].data_ptr())
                setattr(c, "ld_" + k, L[k].stride(0))
        if L.get("bias") is not None:
            c.bias = L["bias"].data_ptr()
        c.act, c.dact_type, c.accumulate = L.get("act", 0), L.get("dact_type", 0), int(L.get("accumulate", False))
    return d


def _run_chain(d, device):
    ws = workspace(lib.cgat_mlp_chain_workspace_bytes(d.n_layers), device)
    with torch.cuda.device(device):
        check(lib.cgat_mlp_chain(C.byref(d), _ptr(ws), ws.numel(), _stream()), "cgat_mlp_chain")


class ChainMLPFn(torch.autograd.Function):
    """out = resid + W_n act(... act(W_1 x + b_1) ...) + b_n for width-128 layers in ONE launch per direction
    (csrc/chain.hip): SimpleNetwork (message_changed.py:36-63) on [rows,128] inputs, with the residual of CGAtNet's
    `edge_attr + Edge(...)` (CGAT.py:580-585) folded in.  Hidden activations are kept for backward; the backward chain
    runs on the transposed weights with the activation derivatives folded in and leaves every pre-activation gradient
    for the one-pass weight + bias gradient kernel."""

    @staticmethod
    def eligible(x, weights, resid=None):
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == 128 and x.shape[0] > 0):
            return False
        if get_bilinear_mode() not in ("f16x3", "f16x3c", "bf16x6") or not (1 <= len(weights) <= 5):
            return False
        if resid is not None and (resid.shape != x.shape or resid.dtype != torch.float32):
            return False
        return all(tuple(w.shape) == (128, 128) and w.dtype == torch.float32 for w in weights)

    @staticmethod
    def forward(ctx, x, resid, act, *wb):
        n = len(wb) // 2
        ws_, bs_ = [_f32c(w.detach()) for w in wb[:n]], [_f32c(b.detach()) for b in wb[n:]]
        # x + f(x): the backward chain then adds g_out in its last layer.  Callers pass two separate reshape() results
        # of one tensor (SimpleNetwork.forward), so identity is decided on storage, shape and strides
        ctx.same = resid is not None and (resid is x or (resid.data_ptr() == x.data_ptr() and resid.shape == x.shape and
                                                         resid.stride() == x.stride() and resid.dtype == x.dtype))
        x = _f32c(x)
        r = None if resid is None else (x if ctx.same else _f32c(resid))
        rows, dev = x.shape[0], x.device
        hid = [torch.empty(rows, 128, dtype=torch.float32, device=dev) for _ in range(n - 1)]
        out = torch.empty(rows, 128, dtype=torch.float32, device=dev)
        layers = [dict(W=ws_[i], bias=bs_[i], act=act, out=hid[i]) for i in range(n - 1)]
        layers.append(dict(W=ws_[-1], bias=bs_[-1], act=_lib.ACT_NONE, resid=r, out=out))
        _run_chain(_chain_desc(rows, x, layers), dev)
        if act in (_lib.ACT_LEAKY, _lib.ACT_RELU) and debug.recording():
            for i in range(n - 1):
                debug.note(wb[i], hid[i] > 0)
        ctx.act, ctx.n, ctx.has_r = act, n, resid is not None
        ctx.save_for_backward(x, *hid, *ws_)
        return out

    @staticmethod
    def backward(ctx, g_out):
        n, act = ctx.n, ctx.act
        x, *rest = ctx.saved_tensors
        hid, ws_ = rest[:n - 1], rest[n - 1:]
        g_out = _f32c(g_out)
        rows, dev = x.shape[0], x.device
        gpre = [torch.empty(rows, 128, dtype=torch.float32, device=dev) for _ in range(n - 1)] + [g_out]
        g_x = torch.empty(rows, 128, dtype=torch.float32, device=dev)
        layers = []
        for i in range(n):                               # chain layer i multiplies by W_(n-1-i)
            sl = n - 1 - i
            L = dict(W=ws_[sl], transposed=True)
            if sl > 0:
                L.update(dact=hid[sl - 1], dact_type=act, out=gpre[sl - 1])
            else:
                L.update(out=g_x, resid=g_out if ctx.same else None)
            layers.append(L)
        _run_chain(_chain_desc(rows, g_out, layers), dev)
        g_w, g_b = [], []
        wsz = workspace(lib.cgat_linear_backward_workspace_bytes(rows, 128, 128), dev)
        with torch.cuda.device(dev):
            for sl in range(n):                          # dW_sl = gpre_sl^T input_sl, db_sl = column sums of gpre_sl
                xin = x if sl == 0 else hid[sl - 1]
                gw = torch.empty(128, 128, dtype=torch.float32, device=dev)
                gb = torch.empty(128, dtype=torch.float32, device=dev)
                check(lib.cgat_linear_backward(_ptr(xin), 128, _ptr(ws_[sl]), 128, None, 128, _ptr(gpre[sl]), 128, None,
                                               None, 128, 0, _ptr(gw), 128, _ptr(gb), rows, 128, 128, _lib.ACT_NONE,
                                               _ptr(wsz), wsz.numel(), _stream()), "cgat_linear_backward")
                g_w.append(gw); g_b.append(gb)
        return (g_x, g_out if (ctx.has_r and not ctx.same) else None, None, *g_w, *g_b)


class AttentionPoolFn(torch.autograd.Function):
    """out[s, f] = sum_{r in seg s} alpha[r, f // fw] * m[r, f] with alpha = mult * exp(a - segmax) / (segsum + eps) -- the
    reference's softmax -> multiply -> scatter_add (CGAT.py:323-329, 59-61; roost_message.py:305-317) as one kernel per
    direction.  `a` [R, aF], `m` [R, F] (fw = F // aF), `mult` [R] or None; `perm` = rows of each segment in CSR order
    (None: the rows already are), so nothing is gathered or permuted.

    apply(a, mult, m, rowptr, perm, eps, keep, keep_idx) is the same with training-mode attention dropout between the
    softmax and the product (CGAT.py:325): out = sum_r keep * alpha * m.  `keep` [R, aF] is the keep-mask scaled by
    1 / (1 - p); the keep row of CSR position t is keep_idx[t] (int32 [R]) or, with keep_idx None, the operand row.  The
    mask gets no gradient, and a mask together with `mult` is refused (no layer combines them; it is not built)."""

    @staticmethod
    def supported(a, m):
        aF, F = a.shape[1], m.shape[1]
        if F % 4 or F % aF or not (a.is_cuda and a.dtype == torch.float32 and m.dtype == torch.float32):
            return False
        fw = F // aF
        return (fw == 1 and aF % 4 == 0) or (fw % 4 == 0 and fw // 4 <= 64 and (fw // 4) & (fw // 4 - 1) == 0)

    @staticmethod
    def forward(ctx, a, mult, m, rowptr, perm, eps, *drop):
        keep, keep_idx = drop if drop else (None, None)
        _require_gpu(a, m, rowptr, keep, keep_idx)
        a, m = _f32c(a), _f32c(m)
        mu = None if mult is None else _f32c(mult.reshape(-1))
        R, aF = a.shape
        F = m.shape[1]
        S = rowptr.numel() - 1
        dev = a.device
        if keep is not None:
            if mu is not None:
                raise ValueError("AttentionPoolFn: a keep-mask together with a multiplier is not supported")
            if keep.shape != a.shape:
                raise ValueError("AttentionPoolFn: the keep-mask must have the logits' shape")
            keep = _f32c(keep)
            if keep_idx is not None:
                if keep_idx.dtype != torch.int32 or keep_idx.numel() != R:
                    raise TypeError("AttentionPoolFn: keep_idx must be int32 [R]")
                keep_idx = keep_idx.contiguous()
        elif keep_idx is not None:
            raise ValueError("AttentionPoolFn: keep_idx without a keep-mask")
        out = torch.empty(S, F, dtype=torch.float32, device=dev)
        mx = torch.empty(S, aF, dtype=torch.float32, device=dev)
        inv = torch.empty(S, aF, dtype=torch.float32, device=dev)
        # low part of the fp64 sum: backward centres on out + out_lo (not needed, hence not computed, without a backward)
        need_lo = any(ctx.needs_input_grad[:3])
        out_lo = torch.empty(S, F, dtype=torch.float32, device=dev) if need_lo else None
        with torch.cuda.device(dev):
            if keep is not None:
                check(lib.cgat_segment_attention_pool_dropout_forward(
                    _ptr(a), aF, _ptr(keep), _ptr(keep_idx), _ptr(m), F, _ptr(rowptr), _ptr(perm), S, F, eps, _ptr(out),
                    _ptr(mx), _ptr(inv), _ptr(out_lo), _stream()), "cgat_segment_attention_pool_dropout_forward")
            else:
                check(lib.cgat_segment_attention_pool_forward(_ptr(a), aF, _ptr(mu), _ptr(m), F, _ptr(rowptr), _ptr(perm), S, F,
                                                              eps, _ptr(out), _ptr(mx), _ptr(inv), _ptr(out_lo), _stream()),
                      "cgat_segment_attention_pool_forward")
        ctx.has_mu, ctx.has_perm, ctx.mshape = mu is not None, perm is not None, None if mult is None else mult.shape
        ctx.has_keep, ctx.has_kidx, ctx.n_drop = keep is not None, keep_idx is not None, len(drop)
        ctx.save_for_backward(a, m, out, mx, inv, out_lo, rowptr, *([mu] if mu is not None else []),
                              *([perm] if perm is not None else []), *([keep] if keep is not None else []),
                              *([keep_idx] if keep_idx is not None else []))
        return out

    @staticmethod
    def backward(ctx, g_out):
        a, m, out, mx, inv, out_lo, rowptr, *rest = ctx.saved_tensors
        mu = rest.pop(0) if ctx.has_mu else None
        perm = rest.pop(0) if ctx.has_perm else None
        keep = rest.pop(0) if ctx.has_keep else None
        keep_idx = rest.pop(0) if ctx.has_kidx else None
        g_out = _f32c(g_out)
        R, aF = a.shape
        F = m.shape[1]
        S = rowptr.numel() - 1
        g_a = torch.empty_like(a)
        g_m = torch.empty_like(m) if ctx.needs_input_grad[2] else None
        g_mu = torch.empty_like(mu) if (mu is not None and ctx.needs_input_grad[1]) else None
        with torch.cuda.device(a.device):
            if keep is not None:
                check(lib.cgat_segment_attention_pool_dropout_backward(
                    _ptr(a), aF, _ptr(keep), _ptr(keep_idx), _ptr(m), F, _ptr(rowptr), _ptr(perm), S, F, _ptr(out), _ptr(mx),
                    _ptr(inv), _ptr(out_lo), _ptr(g_out), _ptr(g_a), _ptr(g_m), F, _stream()),
                    "cgat_segment_attention_pool_dropout_backward")
            else:
                check(lib.cgat_segment_attention_pool_backward(_ptr(a), aF, _ptr(mu), _ptr(m), F, _ptr(rowptr), _ptr(perm), S, F,
                                                               _ptr(out), _ptr(mx), _ptr(inv), _ptr(out_lo), _ptr(g_out), _ptr(g_a),
                                                               _ptr(g_m), F, _ptr(g_mu), _stream()),
                      "cgat_segment_attention_pool_backward")
        return (g_a, (None if g_mu is None else g_mu.reshape(ctx.mshape)), g_m, None, None, None) + (None,) * ctx.n_drop


def attention_pool(a, m, index_plan, index, mult=None, eps=1e-16):
    """softmax(a over the segments of index) * m, summed per segment: rows in their ORIGINAL order, `index_plan` the
    SegmentPlan of `index`.  One launch per direction when the shape allows, the generic three-step path otherwise."""
    n = a.shape[0]
    a2, m2 = a.reshape(n, -1), m.reshape(n, -1)
    if n > 0 and AttentionPoolFn.supported(a2, m2) and (mult is None or a2.shape[1] == 1):
        return AttentionPoolFn.apply(a2, mult, m2, index_plan.rowptr, index_plan.perm, eps)
    alpha = segment_softmax(a2, index_plan, mult=mult, eps=eps)
    fw = m2.shape[1] // a2.shape[1]
    w = alpha if fw == 1 else alpha.repeat_interleave(fw, dim=1)
    return segment_sum(w * m2, index_plan, index)


_fused_edge_combine = _Switch("CGAT_FUSED_EDGE_COMBINE", True)


def set_fused_edge_combine(flag):
    """The one-kernel head combination of GATConvEdges(no_hyper=False) (default on; env CGAT_FUSED_EDGE_COMBINE=0 starts
    it off): EdgeHeadCombineFn instead of the exp / sum / division / dropout / product / mean / index_copy sequence of
    torch ops on [E, H, Co] tensors.  Off: that sequence runs (the A/B reference)."""
    _fused_edge_combine.set(flag)


def get_fused_edge_combine():
    return _fused_edge_combine.value


_fused_attn_dropout = _Switch("CGAT_FUSED_ATTN_DROPOUT", True)


def set_fused_attention_dropout(flag):
    """Training-mode attention dropout of GATConvNodes on the operand-split first layer and the keep-mask attention-pool
    kernels (default on; env CGAT_FUSED_ATTN_DROPOUT=0 starts it off).  Off: the MessagePassing-style route runs --
    concatenated [E, 2C+Ce] rows, generic networks, segment softmax, mask, product, segment sum (the A/B reference).
    The mask is drawn the same way on both routes: one seed gives one mask per edge."""
    _fused_attn_dropout.set(flag)


def get_fused_attention_dropout():
    return _fused_attn_dropout.value


class EdgeHeadCombineFn(torch.autograd.Function):
    """out[perm[t]] = mean_h softmax over the heads(sa[t])[h] * keep[t, h] * sm[t, h] -- the reference's exp -> sum over
    heads -> division -> dropout -> times the message -> mean (CGAT.py:214-223; no max-subtraction) as one kernel per
    direction (csrc/edgecomb.hip).  `sa` [E, H, 1 | Co], `sm` [E, H, Co], `keep` the dropout keep-mask of sa's shape or
    None, `perm` int32 [E] (rows are destination-sorted slots: plan.dst_perm) or None.  Backward recomputes the softmax
    from sa: nothing but the inputs is saved."""

    @staticmethod
    def supported(sa, sm):
        if sa.dim() != 3 or sm.dim() != 3 or sa.shape[:2] != sm.shape[:2]:
            return False
        if sa.dtype != torch.float32 or sm.dtype != torch.float32:
            return False
        H, aF, Co = sm.shape[1], sa.shape[2], sm.shape[2]
        return Co % 4 == 0 and 0 < Co <= 256 and 1 <= H <= 8 and aF in (1, Co)

    @staticmethod
    def forward(ctx, sa, sm, keep, perm):
        _require_gpu(sa, sm, keep, perm)
        if not EdgeHeadCombineFn.supported(sa, sm):
            raise ValueError(f"EdgeHeadCombineFn: unsupported shapes {tuple(sa.shape)}, {tuple(sm.shape)}")
        sa, sm = _f32c(sa), _f32c(sm)
        E, H, Co = sm.shape
        aF = sa.shape[2]
        if keep is not None:
            if keep.shape != sa.shape:
                raise ValueError("EdgeHeadCombineFn: the keep-mask must have the logits' shape")
            keep = _f32c(keep)
        if perm is not None:
            if perm.dtype != torch.int32 or perm.numel() != E:
                raise TypeError("EdgeHeadCombineFn: perm must be int32 [E]")
            perm = perm.contiguous()
        out = torch.empty(E, Co, dtype=torch.float32, device=sm.device)
        with torch.cuda.device(sm.device):
            check(lib.cgat_edge_head_combine_forward(_ptr(sa), aF, _ptr(sm), _ptr(keep), _ptr(perm), E, H, Co, _ptr(out),
                                                     _stream()), "cgat_edge_head_combine_forward")
        ctx.has_keep, ctx.has_perm = keep is not None, perm is not None
        ctx.save_for_backward(sa, sm, *([keep] if keep is not None else []), *([perm] if perm is not None else []))
        return out

    @staticmethod
    def backward(ctx, g_out):
        sa, sm, *rest = ctx.saved_tensors
        keep = rest.pop(0) if ctx.has_keep else None
        perm = rest.pop(0) if ctx.has_perm else None
        g_out = _f32c(g_out)
        E, H, Co = sm.shape
        g_sa = torch.empty_like(sa) if ctx.needs_input_grad[0] else None
        g_sm = torch.empty_like(sm) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(sm.device):
            check(lib.cgat_edge_head_combine_backward(_ptr(sa), sa.shape[2], _ptr(sm), _ptr(keep), _ptr(perm), _ptr(g_out),
                                                      E, H, Co, _ptr(g_sa), _ptr(g_sm), _stream()),
                  "cgat_edge_head_combine_backward")
        return g_sa, g_sm, None, None


def edge_combine_route(sa, sm):
    """True when GATConvEdges hands its head combination to EdgeHeadCombineFn: the switch is on, the tensors are on the
    GPU and the shape is one the kernels take.  Everything else keeps the sequence of torch ops."""
    return _fused_edge_combine.value and sa.is_cuda and sm.is_cuda and EdgeHeadCombineFn.supported(sa, sm)


class GatherRowsFn(torch.autograd.Function):
    """x[index] whose backward is an atomics-free segment sum over the index's CSR plan
    (deterministic, unlike index_add)."""

    @staticmethod
    def forward(ctx, x, index, plan):
        _require_gpu(x, index)
        ctx.plan, ctx.rows = plan, x.shape[0]
        return x.index_select(0, index)

    @staticmethod
    def backward(ctx, g):
        plan = ctx.plan
        g = _f32c(g)
        F = g.shape[1]
        out = torch.empty(ctx.rows, F, dtype=torch.float32, device=g.device)
        with torch.cuda.device(g.device):
            check(lib.cgat_segment_sum(_ptr(g), F, _ptr(plan.perm), _ptr(plan.rowptr), plan.S, F, _ptr(out), F,
                                       _stream()), "cgat_segment_sum")
        return out, None, None


def gather_rows(x, index, plan):
    return GatherRowsFn.apply(x, index, plan)


def segment_softmax(a, index_plan, mult=None, eps=1e-16):
    """softmax over the segments of `index_plan` for rows in their ORIGINAL order [R, F]."""
    perm = index_plan.perm64
    a_s = a.index_select(0, perm)
    m_s = None if mult is None else mult.reshape(-1).index_select(0, perm)
    al_s = SegmentSoftmaxFn.apply(a_s, m_s, index_plan.rowptr, eps)
    out = torch.empty_like(al_s)
    return out.index_copy(0, perm, al_s)


def segment_sum(x, index_plan, index):
    """scatter_add(x, index, dim=0, dim_size=S) for rows in their original order."""
    perm = index_plan.perm64
    return SegmentSumFn.apply(x.index_select(0, perm), index_plan.rowptr, index.index_select(0, perm))


_MODES = {"f32": 0, "bf16x6": 6, "bf16x3": 3, "f16x3": 2, "f16x3c": 4}
# the mode a fresh process starts in (env CGAT_BILINEAR_MODE overrides the built-in default)
DEFAULT_MODE = os.environ.get("CGAT_BILINEAR_MODE", "f16x3c")
if DEFAULT_MODE not in _MODES:
    DEFAULT_MODE = "f16x3c"


def set_bilinear_mode(mode):
    """Arithmetic of the width-128 matrix-core kernels.
    "f16x3c" (default, round 4): 24-bit operands.  Every fp32 operand is scaled by a power of two and split EXACTLY into
    three pieces x = h + l + t (two fp16 pieces and the 24th bit); a product is hh + hl + lh on three fp16-MFMA passes
    (exact) plus ll + ht + th (weight <= 2^-22) on three 6-bit MFMA passes of K = 128 (csrc/mfma_bf16.h), fp32 accumulate:
    1.25 x the matrix time of "f16x3" where "bf16x6" needs 2 x.  Kernels without that form run their "bf16x6" form.
    "bf16x6": three bf16 pieces (24 bits), six bf16-MFMA passes.  "f16x3": two fp16 pieces = 22-bit operands, three passes
    (the fastest; not the default because its operands are narrower than fp32's).  "f32": f32-input MFMA, exact fp32
    fmaf chains.  "bf16x3": three bf16 passes, ~4e-6 relative; fails the parity tests (diagnostic)."""
    lib.cgat_set_bilinear_mode(_MODES[mode])


def get_bilinear_mode():
    m = lib.cgat_get_bilinear_mode()
    return {v: k for k, v in _MODES.items()}[m]


# launch-timer tags of the contraction kernels that have the 3.75-pass h + l + t form in the f16x3c mode (bench.py prices a
# kernel against 2500 / 3.75 TFLOP/s only if it is listed here, against 2500 / 6 otherwise)
F16C_KERNELS = ("bilinear_rows", "bilinear_dual", "bilinear_wgrad")


def set_edge_storage(mode):
    """Storage of the per-edge intermediates Z / gZ of the fused scalar-attention path: "f32" (default) or "bf16"
    (BASELINE configs[4]'s "bf16 activations": half the HBM bytes of the edge phase, tolerance 1e-2; logits, softmax
    statistics and all products unchanged).  Exists at C = Ce = 128 in every split arithmetic mode (f16x3c, bf16x6, f16x3);
    a scalar-attention layer without a bf16 form (other widths, the f32 mode) raises instead of silently running in fp32
    storage.  "bf16-mma" (round 6, the 24-bit modes): bf16 storage AND bf16 OPERANDS in the two per-edge
    BACKWARD products (grad edge_attr, grad W_e: ONE matrix pass on round-to-nearest bf16 images of the rebuilt gZ rows
    and of the weight / edge rows, fp32 accumulation) -- BASELINE configs[4]'s "bf16 activations with MFMA edge-MLP",
    tolerance 1e-2.  The forward product keeps its six passes: on bf16 operands the pre-activations move by ~3e-3 of
    their scale, 0.3 % of the LeakyReLU derivatives land on the other side, and the gradients of edge_attr and of the
    attention network's first layer came out 1.6 % ... 5.7 % off (tools/bf16mma_probe.py; measured 775 ms instead of 830
    per 64 M-edge step) -- outside the mode's stated tolerance.
    "f32+gz" / "f32+za": fp32 with the backward's gZ stored / with the attention pre-activations stored at every shape --
    the A/B references of the rebuilt-gZ route and of the bit form of the saved buffer (debug.nodes_attention_bit_form)."""
    lib.cgat_set_edge_storage({"f32": 0, "bf16": 1, "f32+gz": 2, "bf16-mma": 3, "f32+za": 4}[mode])


def get_edge_storage():
    return {0: "f32", 1: "bf16", 2: "f32+gz", 3: "bf16-mma", 4: "f32+za"}[lib.cgat_get_edge_storage()]


class _storage_of:
    """Run a backward under the edge-storage mode its forward ran under."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = lib.cgat_get_edge_storage()
        lib.cgat_set_edge_storage(self.mode)

    def __exit__(self, *a):
        lib.cgat_set_edge_storage(self.prev)


def prof_enable(on=True):
    lib.cgat_prof_enable(1 if on else 0)


def prof_reset():
    lib.cgat_prof_reset()


def prof_launches():
    """Kernel launches the library has issued so far in this process (all streams)."""
    return int(lib.cgat_prof_launches())


def prof_get(tag):
    n, ms = C.c_int(0), C.c_float(0.0)
    lib.cgat_prof_get(tag.encode(), C.byref(n), C.byref(ms))
    return n.value, ms.value
