"""CGAtNet and its attention layers behind the reference's constructor / forward API and
state_dict layout (reference CGAT/CGAT.py:14-613), executing on libcgat_hip.

Drop-in: `importlib.import_module("cgat_amd").CGAtNet(200, elem_fea_len=..., ...)` is what
lightning_module.py:165-176 does with `--version cgat_amd`.

torch_geometric is not required: `GATConvNodes` keeps the MessagePassing-style surface
(`forward(x, edge_index, edge_attr, x_0, size=None)`, `message`, `update`), and PyG's gather
convention is applied through the batch's CSR plan: x_j = x[edge_index[0]], x_i =
x[edge_index[1]], softmax and aggregation keyed by edge_index[1].
"""
import itertools
import os
from typing import Callable, NamedTuple, Union

import torch
import torch.nn as nn

from . import _lib, chunked, debug, rowprog
from .hypernet import H_Net, H_Net_0
from .mlp import ResidualNetwork, SimpleNetwork
from .ops import (AttentionPoolFn, attention_pool, get_fused_attention_dropout, EdgeHiddenFn, EdgeHiddenHeadsFn, HeadsLinear1Fn, HeadsLinearFn, NodeLayerFn, NodesAttentionFn, SegmentPlan, SegmentSoftmaxFn, SegmentSumFn, gather_rows, get_plan, get_segment_plan, linear, small_embedding,
                  segment_softmax, segment_sum)
from .ops import overlap_enabled as ops_overlap_enabled
from .ops import HNetFn, get_fused_inference, nodes_attention_infer
from .ops import IndexedEdgeAttr, get_indexed_edge_attr, infer_indexed_ok, nodes_attention_infer_indexed
from .ops import NodesAttentionIndexedFn, NodeLayerIndexedFn, get_indexed_edge_training, train_indexed_ok
from .ops import EdgeHiddenIndexedFn, EdgeHiddenHeadsIndexedFn, edge_hidden_indexed_ok, get_indexed_vector_attention
from .ops import EdgeHeadCombineFn, edge_combine_route, _indexed_operands_ok
from .ops import branch_stream
from .roost import Roost


# ----------------------------------------------------------------------------------------
# routes: which of the library's entries a layer call reaches, decided once per call
# ----------------------------------------------------------------------------------------
class Route(NamedTuple):
    """What one layer call runs.  `kind`: GATConvNodes -- pair, layer_fused, scalar, vector, vector_dropout, message;
    GATConvEdges -- rowwise, fast, generic.  `indexed`: an IndexedEdgeAttr is kept (False: forward densifies one that
    arrives).  `no_grad`: the scalar attention half runs nodes_attention_infer[_indexed] (kinds scalar, layer_fused)."""
    kind: str
    indexed: bool = False
    no_grad: bool = False


_Lazy = Union[bool, Callable[[], bool]]     # an answer that costs a call: asked only by the route that depends on it


def _ask(answer):
    return answer() if callable(answer) else answer


class NodeFacts(NamedTuple):
    """Everything nodes_route reads of one GATConvNodes call (GATConvNodes._facts gathers it)."""
    x_is_tensor: bool = True
    x_cuda: bool = True
    x_f32: bool = True
    x_2d: bool = True
    edge_attr_cuda: bool = True
    N: int = 0
    E: int = 0
    C: int = 0
    Ce: int = 0
    H: int = 0
    Hd: int = 0
    R: int = 0                          # rows of the table of an IndexedEdgeAttr (0: a dense tensor arrived)
    vector: bool = False
    final: bool = False
    first: bool = False
    pooling: type = type(None)          # type(Pooling_NN)
    message_own: bool = True            # type(layer).message is GATConvNodes.message
    update_own: bool = True
    drop: bool = False                  # dropout and training
    grad_enabled: bool = True
    requires_grad: bool = True          # any of x, edge_attr (its table) and the attention parameters
    recording: bool = False             # debug.recording()
    over_budget: bool = False           # E > chunked.max_edges_per_pass()
    inner_pass: bool = False            # one chunk of a chunked pass
    overlap: bool = False               # ops.overlap_enabled()
    fused_infer: bool = True            # the switches
    fused_dropout: bool = True
    indexed_training: bool = False
    indexed_vector: bool = False
    indexed_input: bool = False         # an IndexedEdgeAttr arrived
    operands_ok: bool = False           # ops._indexed_operands_ok of x, table, index
    pool_supported: _Lazy = False       # AttentionPoolFn.supported at the layer's widths
    infer_indexed_ok: _Lazy = False     # the library's answers at (N, E) and the layer's dims
    train_indexed_ok: _Lazy = False
    edge_hidden_indexed_ok: _Lazy = False


def nodes_route(f):
    """The route of a GATConvNodes call from its facts alone: no tensor, plan, library call or global is touched here
    (the lazy answers are asked last, and only where everything else already holds)."""
    if not f.x_is_tensor:
        return Route("pair")
    own = f.message_own and f.update_own
    # no backward can follow (grad mode off, or nothing involved requires grad) and no debug recording wants the saved buffer
    no_grad = f.fused_infer and not f.recording and (not f.grad_enabled or not f.requires_grad)
    if f.overlap and not f.vector and not f.final and not f.drop and own and f.pooling in (H_Net, H_Net_0):
        kind = "layer_fused"
    elif not f.vector and f.message_own and not f.drop:
        kind = "scalar"
    elif f.vector and f.message_own and not f.drop:
        kind = "vector"
    elif (f.drop and not f.inner_pass and f.fused_dropout and f.message_own and f.x_cuda and f.edge_attr_cuda and f.x_f32
          and f.E > 0 and _ask(f.pool_supported)):
        kind = "vector_dropout"
    else:
        # subclasses overriding message(), and training-mode attention dropout where vector_dropout does not apply
        # (switched off, CPU tensors, a shape the pooling kernels do not take, chunks)
        kind = "message"
    # an IndexedEdgeAttr survives one unchunked pass without training-mode dropout through the layer's own message / update
    indexed = f.indexed_input and f.x_cuda and not f.drop and own and not f.over_budget
    if indexed and f.vector:
        # with grad and without; a debug recording stays (debug.note_sorted_hidden needs `hidden` alone)
        indexed = f.indexed_vector and f.operands_ok and _ask(f.edge_hidden_indexed_ok)
    elif indexed:
        x_ok = f.x_f32 and f.x_2d
        # either nodes_attention_infer_indexed, or -- a backward follows, under the training switch; a debug recording
        # does not leave it (debug.note_attention_indexed) -- NodesAttentionIndexedFn / NodeLayerIndexedFn
        indexed = ((x_ok and no_grad and _ask(f.infer_indexed_ok)) or
                   (f.indexed_training and f.grad_enabled and x_ok and f.operands_ok and f.requires_grad and
                    _ask(f.train_indexed_ok)))
    return Route(kind, bool(indexed), no_grad and kind in ("scalar", "layer_fused"))


class EdgeFacts(NamedTuple):
    """Everything edges_route reads of one GATConvEdges call."""
    indexed_input: bool = False
    no_hyper: bool = True
    x_cuda: bool = True
    networks_own: bool = True           # MH_A and MH_M are MultiHeadNetwork itself


def edges_route(f):
    if f.no_hyper:
        # the shipped form is row-wise: on an IndexedEdgeAttr it runs on the table's rows and the result is a lookup again
        return Route("rowwise", f.indexed_input)
    return Route("fast" if f.x_cuda and f.networks_own else "generic")     # (the per-edge form needs the rows themselves)


class MultiHeadNetwork(nn.Module):
    """nb_heads independent input_dim -> hidden -> output_dim MLPs with LeakyReLU(0.01), stored as
    the reference's grouped 1x1 Conv1d parameters (CGAT.py:65-112).  The head replication
    (`repeat`) of the reference never happens: all heads' first layers are one GEMM, each
    head's second layer one GEMM on its slice."""

    def __init__(self, input_dim, output_dim, hidden_layer_dim, nb_heads, view=True):
        super().__init__()
        self.input_dim = input_dim
        self.nb_heads = nb_heads
        self.output_dim = output_dim
        self.hidden_layer_dim = hidden_layer_dim
        self.fc_in = nn.Conv1d(in_channels=input_dim * nb_heads, out_channels=hidden_layer_dim * nb_heads,
                               kernel_size=1, groups=nb_heads)
        self.acts = nn.LeakyReLU()
        self.fc_out = nn.Conv1d(in_channels=hidden_layer_dim * nb_heads, out_channels=output_dim * nb_heads,
                                kernel_size=1, groups=nb_heads)
        self.view = view

    def forward(self, fea):
        fea = fea.reshape(-1, self.input_dim)
        H, Hd, O = self.nb_heads, self.hidden_layer_dim, self.output_dim
        if rowprog.eligible(fea) and 2 * H + 2 <= _lib.ROWPROG_MAX_OPS:
            # a few hundred rows (the crystal pooling at the harness' batch): both layers of all heads in one launch
            return rowprog.RowMultiHeadFn.apply(fea, self.fc_in.weight, self.fc_in.bias, self.fc_out.weight,
                                                self.fc_out.bias, H, Hd, O)
        hid = linear(fea, self.fc_in.weight, self.fc_in.bias, _lib.ACT_LEAKY)            # [M, H*Hd]
        # all heads' second layers as one autograd node (no per-slice zero-filled gradients of hid)
        return HeadsLinear1Fn.apply(hid, self.fc_out.weight, self.fc_out.bias, H, Hd, O)  # [M, H, O]

    def __repr__(self):
        return self.__class__.__name__


class MHAttention(nn.Module):
    """Per-crystal multi-head attention pooling of node features with the composition
    embedding as context (CGAT.py:14-62)."""

    def __init__(self, in_channels, out_channels, heads=1, vector_attention=False):
        super().__init__()
        self.heads = heads
        self.out_channels = out_channels
        self.MH_A = MultiHeadNetwork(2 * in_channels, out_channels if vector_attention else 1, in_channels, heads,
                                     view=False)
        self.MH_M = MultiHeadNetwork(in_channels, out_channels, in_channels, heads)

    def forward(self, fea, cry_fea, index, size=None):
        size = int(index[-1]) + 1 if size is None else size
        plan = get_segment_plan(index, size)
        m = self.MH_M(fea)                                                         # [N,H,C]
        pair = torch.cat([fea, gather_rows(cry_fea, index, plan)], dim=1)          # == stack+transpose+reshape, 55-58
        alpha = self.MH_A(pair)                                                    # [N,H,1|C]
        return attention_pool(alpha, m, plan, index, eps=1e-16)                    # softmax over the crystal, x m, summed


def _dropout_keep(like, p):
    """Keep-mask of F.dropout(alpha, p, training=True) (reference CGAT.py:221, 325) as an explicit tensor: Bernoulli(1 - p)
    scaled by 1 / (1 - p), drawn from torch's Philox generator of the device (seeded by torch.manual_seed, as the
    reference's own mask is)."""
    if p >= 1.0:
        return torch.zeros_like(like)
    return torch.empty_like(like).bernoulli_(1.0 - p).mul_(1.0 / (1.0 - p))


def _edge_hidden(in_channels, nbr_channels):
    return int((2 * in_channels + nbr_channels) / 1.5)


class GATConvEdges(nn.Module):
    """Edge update (CGAT.py:115-230).  With the shipped no_hyper=True the reference computes the
    attention and then discards it (224-225): the result is Pooling_NN(edge_attr) alone, and
    MH_A / MH_M never receive a gradient.  That dead compute is skipped here -- outputs and
    gradients are identical."""

    def __init__(self, in_channels, out_channels, nbr_channels, heads=1, concat=True, negative_slope=0.2, dropout=0,
                 bias=True, vector_attention=False, first=False, no_hyper=True, **kwargs):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.nbr_channels = nbr_channels
        self.heads = heads
        self.concat = concat
        self.negative_slope = negative_slope
        self.dropout = dropout
        self.vector_attention = vector_attention
        D, Hd = 2 * in_channels + nbr_channels, _edge_hidden(in_channels, nbr_channels)
        self.MH_A = MultiHeadNetwork(D, out_channels if vector_attention else 1, Hd, heads)
        self.MH_M = MultiHeadNetwork(D, out_channels, Hd, heads)
        if no_hyper:
            self.Pooling_NN = SimpleNetwork(out_channels, out_channels, [out_channels])
        elif first:
            self.Pooling_NN = H_Net_0(out_channels, 3, out_channels, out_channels, 2, out_channels, out_channels)
        else:
            self.Pooling_NN = H_Net(out_channels, 3, out_channels, out_channels, 2, out_channels, out_channels)
        self.first = first
        self.no_hyper = no_hyper

    def _facts(self, x, edge_attr):
        return EdgeFacts(indexed_input=isinstance(edge_attr, IndexedEdgeAttr), no_hyper=self.no_hyper,
                         x_cuda=torch.is_tensor(x) and x.is_cuda,
                         networks_own=type(self.MH_A) is MultiHeadNetwork and type(self.MH_M) is MultiHeadNetwork)

    def route(self, x, edge_index, edge_attr):
        """The Route `forward` takes for these arguments, without running anything."""
        return edges_route(self._facts(x, edge_attr))

    def forward(self, x, edge_index, edge_attr, x_0, size=None):
        route = self.route(x, edge_index, edge_attr)
        if isinstance(edge_attr, IndexedEdgeAttr) and not route.indexed:
            edge_attr = edge_attr.dense()
        if route.kind == "rowwise":           # (the discarded attention's dropout mask is discarded with it)
            if route.indexed:
                return edge_attr.with_table(self.Pooling_NN(edge_attr.table))
            return self.Pooling_NN(edge_attr)
        drop = self.dropout if (self.dropout and self.training) else 0.0
        plan = get_plan(edge_index, x.shape[0])
        if route.kind == "fast":
            aggr_out = self._message_fast(x, edge_attr, plan, drop)
        else:
            splan0, splan1 = _endpoint_plans(plan, edge_index)
            x_i = gather_rows(x, edge_index[0], splan0)           # note: opposite naming to GATConvNodes (209-210)
            x_j = gather_rows(x, edge_index[1], splan1)
            m = torch.cat([x_i, edge_attr, x_j], dim=-1)
            # logits and messages [E, H, .] in the caller's edge order -> [E, Co] (CGAT.py:214-223)
            aggr_out = _head_softmax_mean(self.MH_A(m), self.MH_M(m), drop)
        if self.first:
            return self.Pooling_NN(edge_attr, aggr_out)
        return self.Pooling_NN(x_0, edge_attr, aggr_out)

    def _message_fast(self, x, edge_attr, plan, drop=0.0):
        """The attention / message networks of the edge update without the concatenated [E, 2C+Ce] rows: first layers of
        both networks as ONE operand-split op in destination-sorted slot order (EdgeHiddenFn, the op of the
        vector-attention node layer), the 2H second layers as one autograd node, the head softmax and mean on [E, H, .]
        tensors, and one permutation back to the caller's edge order at the end."""
        a, m = self.MH_A, self.MH_M
        H, Hd, D, C, Ce = self.heads, a.hidden_layer_dim, a.input_dim, self.in_channels, self.nbr_channels
        w = torch.cat([a.fc_in.weight.reshape(H * Hd, D), m.fc_in.weight.reshape(H * Hd, D)], dim=0)
        # the edge update names the endpoints the other way round (CGAT.py:209-210: x_i = x[edge_index[0]]); the op
        # multiplies its first column block with x[edge_index[1]] and its last with x[edge_index[0]]: swap the blocks
        w = torch.cat([w[:, C + Ce:], w[:, C:C + Ce], w[:, :C]], dim=1)
        sa, sm = _two_layers(a, m, x, edge_attr, plan, w, torch.cat([a.fc_in.bias, m.fc_in.bias]))
        return _head_softmax_mean(sa, sm, drop, plan.dst_perm)


def _two_layers(a, m, x, edge_attr, plan, w_in, b_in, indexed=False):
    """First layers of both networks of a layer (MH_A, MH_M; w_in, b_in their stacked first-layer parameters) on the
    operand split, then the 2H second layers: logits and messages [E, H, .] in destination-sorted slot order.  On a
    dense edge_attr or (indexed) on a lookup: the same two forms, no [E, Ce] tensor."""
    H, Hd = a.nb_heads, a.hidden_layer_dim
    first = (edge_attr.table, edge_attr.index) if indexed else (edge_attr,)
    second = (a.fc_out.weight, a.fc_out.bias, m.fc_out.weight, m.fc_out.bias, H, Hd, (a.output_dim, m.output_dim))
    if EdgeHiddenHeadsFn.eligible(w_in.shape[0], H, Hd, (a.output_dim, m.output_dim)):
        # first layers + the 2H second layers as ONE autograd node: its backward folds LeakyReLU' into the second
        # layers' input-gradient products instead of an elementwise pass over [E, 2 H Hd] (ops.EdgeHiddenHeadsFn)
        heads_fn = EdgeHiddenHeadsIndexedFn if indexed else EdgeHiddenHeadsFn
        sa, sm = heads_fn.apply(x, *first, plan, w_in, b_in, *second)
        hid = debug.last_hidden
    else:
        hidden_fn = EdgeHiddenIndexedFn if indexed else EdgeHiddenFn
        hid, hmax = hidden_fn.apply(x, *first, plan, w_in, b_in)                         # [E, 2*H*Hd], sorted slots
        # second layers of all 2H heads as one autograd node (ops.HeadsLinearFn): [E,H,Co] each
        sa, sm = HeadsLinearFn.apply(hid, *second, hmax)
    if debug.recording():
        debug.note_sorted_hidden((a.fc_in.weight, m.fc_in.weight), plan, hid)
    return sa, sm


def _head_softmax_mean(sa, sm, drop, perm=None):
    """Softmax over the heads (no max-subtraction), dropout, times the message, head mean (CGAT.py:214-223): logits and
    messages [E, H, .] -> [E, Co].  `perm` (plan.dst_perm): the rows are destination-sorted slots and the result goes
    back to the caller's edge order; None: they are in that order already."""
    keep = None
    if drop:
        keep = _dropout_keep(sa, drop)                        # CGAT.py:221
        if debug.recording():                                 # (recorded in the caller's edge order)
            debug.note_dropout(keep if perm is None else torch.empty_like(keep).index_copy(0, perm.long(), keep))
    if edge_combine_route(sa, sm):
        # exp, head sum, division, dropout, product, head mean and the permutation back as one kernel per direction
        return EdgeHeadCombineFn.apply(sa, sm, keep, perm)
    alpha = sa.exp()
    alpha = alpha / alpha.sum(dim=1, keepdim=True)
    if keep is not None:
        alpha = alpha * keep
    out = (sm * alpha).mean(dim=1)
    return out if perm is None else torch.empty_like(out).index_copy(0, perm.long(), out)


class _RowPlan:
    """Adapter: the rows-grouped-by-endpoint view GatherRowsFn needs, taken from an EdgePlan."""

    def __init__(self, rowptr, perm, S):
        self.rowptr, self.perm, self.S = rowptr, perm, S


def _endpoint_plans(plan, edge_index):
    """(plan over edge_index[0], plan over edge_index[1]) in ORIGINAL edge order."""
    if not hasattr(plan, "_orig_plans"):
        plan._orig_plans = (SegmentPlan(edge_index[0], plan.N), _RowPlan(plan.dst_rowptr, plan.dst_perm, plan.N))
    return plan._orig_plans


class GATConvNodes(nn.Module):
    """Node update: per-edge multi-head MLPs -> softmax over each atom's incoming edges ->
    scatter-add -> head mean -> hypernetwork (CGAT.py:233-340)."""

    def __init__(self, in_channels, out_channels, nbr_channels, heads=1, concat=False, negative_slope=0.2, dropout=0,
                 bias=True, final=False, vector_attention=False, first=False, **kwargs):
        super().__init__()
        self.aggr, self.flow, self.node_dim = 'add', 'source_to_target', 0
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.nbr_channels = nbr_channels
        self.heads = heads
        self.concat = concat
        self.negative_slope = negative_slope       # stored, never used: the MLPs use nn.LeakyReLU() = 0.01
        self.dropout = dropout
        self.final = final
        self.first = first
        self.vector_attention = vector_attention
        D, Hd = 2 * in_channels + nbr_channels, _edge_hidden(in_channels, nbr_channels)
        self.MH_A = MultiHeadNetwork(D, out_channels if vector_attention else 1, Hd, heads)
        self.MH_M = MultiHeadNetwork(D, out_channels, Hd, heads)
        if not final and first:
            self.Pooling_NN = H_Net_0(out_channels, 3, out_channels, out_channels, 2, out_channels, out_channels)
        elif not final:
            self.Pooling_NN = H_Net(out_channels, 3, out_channels, out_channels, 2, out_channels, out_channels)

    # -- the route of one call: gathered facts -> nodes_route.  `forward` asks once; the runners below receive the answer
    #    and decide nothing (handed a combination they cannot run, they raise) ----------------------------------------
    def _facts(self, x, edge_index, edge_attr, inner_pass=False):
        if not torch.is_tensor(x):
            return NodeFacts(x_is_tensor=False)
        indexed = isinstance(edge_attr, IndexedEdgeAttr)
        ea = edge_attr.table if indexed else edge_attr
        N, E, H, Hd = x.shape[0], edge_index.shape[1], self.heads, self.MH_A.hidden_layer_dim
        C, Ce, R = (x.shape[1] if x.dim() == 2 else 0), edge_attr.shape[1], (ea.shape[0] if indexed else 0)
        plan_c = lambda: _lib.Plan(N, E, 0, 0, 0, 0, 0, 0)           # (the library's answers read N and E of a plan)
        return NodeFacts(
            x_cuda=x.is_cuda, x_f32=x.dtype == torch.float32, x_2d=x.dim() == 2, edge_attr_cuda=ea.is_cuda,
            N=N, E=E, C=C, Ce=Ce, H=H, Hd=Hd, R=R, vector=bool(self.vector_attention), final=bool(self.final),
            first=bool(self.first), pooling=type(getattr(self, "Pooling_NN", None)),
            message_own=type(self).message is GATConvNodes.message, update_own=type(self).update is GATConvNodes.update,
            drop=bool(self.dropout and self.training),      # F.dropout(..., training=self.training): identity in eval mode
            grad_enabled=torch.is_grad_enabled(),
            requires_grad=x.requires_grad or ea.requires_grad or any(t is not None and t.requires_grad
                                                                   for t in self._attn_params()),
            recording=debug.recording(), over_budget=E > chunked.max_edges_per_pass(), inner_pass=inner_pass,
            overlap=ops_overlap_enabled(), fused_infer=get_fused_inference(), fused_dropout=get_fused_attention_dropout(),
            indexed_training=get_indexed_edge_training(), indexed_vector=get_indexed_vector_attention(),
            indexed_input=indexed, operands_ok=indexed and _indexed_operands_ok(x, ea, edge_attr.index, N, E),
            pool_supported=lambda: AttentionPoolFn.supported(x.new_empty(0, H * self.MH_A.output_dim),
                                                             x.new_empty(0, H * self.out_channels)),
            infer_indexed_ok=lambda: infer_indexed_ok(plan_c(), C, Ce, H, Hd, R),
            train_indexed_ok=lambda: train_indexed_ok(plan_c(), C, Ce, H, Hd, R),
            edge_hidden_indexed_ok=lambda: edge_hidden_indexed_ok(plan_c(), C, Ce, 2 * H * Hd, R))

    def route(self, x, edge_index, edge_attr, inner_pass=False):
        """The Route of one pass of `forward` over these arguments, without running anything (no launch, no plan).
        inner_pass: as one chunk of a chunked pass (E beyond chunked.max_edges_per_pass()) is routed."""
        return nodes_route(self._facts(x, edge_index, edge_attr, inner_pass))

    def _attn_params(self):
        a, m = self.MH_A, self.MH_M
        return (a.fc_in.weight, a.fc_in.bias, a.fc_out.weight, a.fc_out.bias, m.fc_in.weight, m.fc_in.bias,
                m.fc_out.weight, m.fc_out.bias)

    # -- fused scalar-attention path: one call into cgat_nodes_attention_forward, or -- route.no_grad: no backward can
    #    follow -- the forward without grad (ops.nodes_attention_infer: same results, no saved buffer, no per-edge
    #    activations at the benchmark widths); route.indexed: the same two on the lookup -----------------------------
    def _aggregate_fused(self, x, edge_attr, plan, route):
        if route.kind not in ("scalar", "layer_fused"):
            raise ValueError(f"GATConvNodes: the fused scalar-attention path cannot run {route}")
        params = self._attn_params()
        if route.indexed and route.no_grad:
            return nodes_attention_infer_indexed(x, edge_attr, plan, self.heads, *params)
        if route.indexed:
            return NodesAttentionIndexedFn.apply(x, edge_attr.table, edge_attr.index, plan, self.heads, *params)
        if route.no_grad:
            return nodes_attention_infer(x, edge_attr, plan, self.heads, *params)
        return NodesAttentionFn.apply(x, edge_attr, plan, self.heads, *params)

    # -- vector attention (CGAT.py:286-290: MH_A emits one logit per head AND channel): the shared first layer of both
    #    networks runs as one operand-split op in destination-sorted order, so the concatenated message [E, 2C+Ce],
    #    its K = 2C+Ce products and the two permutations of the generic path disappear.  With training-mode attention
    #    dropout (route vector_dropout; CGAT.py:325: a keep-mask of the coefficients, [E, H, Co | 1] in ORIGINAL edge order)
    #    also the scalar-attention layer runs here, MH_A's second layers emitting one logit per head: the pooling kernels
    #    take the mask as an operand and reach its rows through plan.dst_perm ----------------------------------------
    def _aggregate_vector(self, x, edge_attr, plan, route):
        if route.kind not in ("vector", "vector_dropout"):
            raise ValueError(f"GATConvNodes: the operand-split path cannot run {route}")
        a, m = self.MH_A, self.MH_M
        H, Hd, Co, D, E = self.heads, a.hidden_layer_dim, self.out_channels, a.input_dim, plan.E
        keep = None
        if route.kind == "vector_dropout":
            # drawn on the shape and in the edge order of the MessagePassing-style route's alpha: one seed, one mask
            keep = _dropout_keep(x.new_empty(E, H, a.output_dim), self.dropout)                      # CGAT.py:325
            debug.note_dropout(keep)
        w_in = torch.cat([a.fc_in.weight.reshape(H * Hd, D), m.fc_in.weight.reshape(H * Hd, D)], dim=0)
        sa, sm = _two_layers(a, m, x, edge_attr, plan, w_in, torch.cat([a.fc_in.bias, m.fc_in.bias]), route.indexed)
        sa2, sm2 = sa.reshape(E, -1), sm.reshape(E, -1)
        if keep is not None:
            # (the route has checked the shape) softmax, mask, product and sum as one kernel per direction
            agg = AttentionPoolFn.apply(sa2, None, sm2, plan.dst_rowptr, None, 1e-16, keep.reshape(E, -1), plan.dst_perm)
        elif E > 0 and AttentionPoolFn.supported(sa2, sm2):
            # channel-wise softmax over each atom's incoming edges, times the message, summed per atom: one kernel per
            # direction (csrc/segment.hip), no alpha / alpha*message tensors of [E, H*C]
            agg = AttentionPoolFn.apply(sa2, None, sm2, plan.dst_rowptr, None, 1e-16)
        else:
            alpha = SegmentSoftmaxFn.apply(sa2, None, plan.dst_rowptr, 1e-16)
            agg = SegmentSumFn.apply(sm2 * alpha, plan.dst_rowptr, plan.dst_sorted.long())
        return agg.reshape(plan.N, H, Co).mean(dim=1)

    # -- MessagePassing-style surface (subclasses overriding message) --
    def message(self, x_i, x_j, edge_attr, edge_index_i, plan=None):
        m = torch.cat([x_i, edge_attr, x_j], dim=-1)
        alpha = self.MH_A(m)
        m = self.MH_M(m)
        E = alpha.shape[0]
        perm = plan.dst_perm.long()
        al = SegmentSoftmaxFn.apply(alpha.reshape(E, -1).index_select(0, perm), None, plan.dst_rowptr, 1e-16)
        alpha = torch.empty_like(al).index_copy(0, perm, al).reshape(alpha.shape)
        if self.dropout and self.training:
            keep = _dropout_keep(alpha, self.dropout)         # CGAT.py:325: sample attention coefficients stochastically
            debug.note_dropout(keep)
            alpha = alpha * keep
        return m * alpha

    def _aggregate_message(self, x_src, x_dst, edge_index, edge_attr, plan, splans):
        """The MessagePassing-style route: gather both endpoints (x_j from x_src with edge_index[0], x_i from x_dst with
        edge_index[1]; splans: their row plans), message(), sum per destination, head mean -> [plan.N, Co]."""
        x_j = gather_rows(x_src, edge_index[0], splans[0])
        x_i = gather_rows(x_dst, edge_index[1], splans[1])
        msg = self.message(x_i, x_j, edge_attr, edge_index[1], plan=plan)                 # [E,H,C]
        E = msg.shape[0]
        perm = plan.dst_perm.long()
        agg = SegmentSumFn.apply(msg.reshape(E, -1).index_select(0, perm), plan.dst_rowptr,
                                 edge_index[1].index_select(0, perm))
        return agg.reshape(plan.N, self.heads, self.out_channels).mean(dim=1)

    # -- whole layer as one autograd node (scalar attention + H_Net update): lets the backward overlap the
    #    hypernetwork's weight-gradient contractions with the attention backward (ops.NodeLayerFn) -----------------
    def _layer_fused(self, x, edge_attr, x_0, plan, route):
        if route.kind != "layer_fused":
            raise ValueError(f"GATConvNodes: the whole-layer node cannot run {route}")
        pool = self.Pooling_NN
        hyper = pool.Hyper
        flat = []
        for layer in hyper.layers:
            hl = layer.hyper_linear if hasattr(layer, "hyper_linear") else layer
            flat += hl.flat_params()
        if self.first:
            h0, damping = x, None
        else:
            with torch.no_grad():
                pool.damping.data = pool.damping.data.clamp(0.0, 1.0)      # Hypernetworksmp.py:307, as H_Net.forward
            h0, damping = x_0, pool.damping
        if route.no_grad:
            # the attention half without grad; the hypernetwork as its own node (NodeLayerFn's forward runs the same call)
            aggr = self._aggregate_fused(x, edge_attr, plan, route)
            return HNetFn.apply(h0, aggr, damping, hyper.n_fc, len(hyper.layers), *flat)
        if route.indexed:
            return NodeLayerIndexedFn.apply(x, edge_attr.table, edge_attr.index, h0, plan, self.heads, damping, hyper.n_fc,
                                            len(hyper.layers), *self._attn_params(), *flat)
        return NodeLayerFn.apply(x, edge_attr, h0, plan, self.heads, damping, hyper.n_fc, len(hyper.layers),
                                 *self._attn_params(), *flat)

    def propagate(self, edge_index, x, edge_attr, x_0, route=None):
        """One pass on `route` (None: asked here), or -- beyond the per-pass budget -- chunk by chunk, each chunk's inner
        pass on its own route."""
        if edge_index.shape[1] > chunked.max_edges_per_pass():
            # beyond the per-pass budget (BASELINE configs[4]: 64 M edges): closed chunks of the graph, one at a time
            chunks = chunked.closed_chunks(edge_index, x.shape[0], chunked.max_edges_per_pass())
            if len(chunks) > 1:
                drop = bool(self.dropout and self.training)
                if (not self.vector_attention and not drop and not ops_overlap_enabled() and
                        type(self).message is GATConvNodes.message and type(self).update is GATConvNodes.update and
                        os.environ.get("CGAT_CHUNK_SPLIT", "1") != "0"):
                    # aggregate (6 KB of saved state per edge) is recomputed per chunk in backward, update (the
                    # hypernetwork: small state) is not: 2 + 1 passes instead of 2 + 2
                    agg = lambda xs, ei, es: self._aggregate_fused(xs, es, get_plan(ei, xs.shape[0]),
                                                                   self.route(xs, ei, es, inner_pass=True))
                    upd = lambda aggr, x0s, xs: self.update(aggr, x_0=x0s, x=xs, _mean_done=True)
                    return chunked.ChunkedSplitLayerFn.apply(agg, upd, chunks, x, edge_attr, x_0, *self.parameters())
                run = lambda xs, ei, es, x0s: self._propagate_one(ei, xs, es, x0s, self.route(xs, ei, es, inner_pass=True))
                return chunked.ChunkedLayerFn.apply(run, chunks, x, edge_attr, x_0, *self.parameters())
        return self._propagate_one(edge_index, x, edge_attr, x_0, route or self.route(x, edge_index, edge_attr))

    def _propagate_one(self, edge_index, x, edge_attr, x_0, route):
        plan = get_plan(edge_index, x.shape[0])
        if route.kind == "layer_fused":
            return self._layer_fused(x, edge_attr, x_0, plan, route)
        if route.kind == "scalar":
            aggr = self._aggregate_fused(x, edge_attr, plan, route)
        elif route.kind in ("vector", "vector_dropout"):
            aggr = self._aggregate_vector(x, edge_attr, plan, route)
        elif route.kind == "message" and not route.indexed:
            aggr = self._aggregate_message(x, x, edge_index, edge_attr, plan, _endpoint_plans(plan, edge_index))
        else:
            raise ValueError(f"GATConvNodes: one pass over a node tensor cannot run {route}")
        return self.update(aggr, x_0=x_0, x=x, _mean_done=True)

    def update(self, aggr_out, x_0, x, _mean_done=False):
        if not _mean_done:
            aggr_out = aggr_out.mean(dim=1)
        if not self.final and self.first:
            return self.Pooling_NN(x, aggr_out)
        elif not self.final:
            return self.Pooling_NN(x_0, x, aggr_out)
        return aggr_out

    def _propagate_pair(self, edge_index, x_src, x_dst, edge_attr):
        """x = (x_source, x_target) (CGAT.py:308-312): PyG gathers x_j from the first entry with edge_index[0], x_i from
        the second with edge_index[1] and aggregates over the second's rows."""
        n_src, n_dst = x_src.shape[0], x_dst.shape[0]
        plan = get_plan(edge_index, max(n_src, n_dst))
        if not hasattr(plan, "_pair_plans"):
            plan._pair_plans = {}
        key = (n_src, n_dst)
        if key not in plan._pair_plans:
            if edge_index.shape[1] and int(edge_index[1].max()) >= n_dst:
                raise IndexError(f"cgat_amd: edge_index[1] reaches beyond the {n_dst} target rows")
            plan._pair_plans[key] = (SegmentPlan(edge_index[0], n_src), _RowPlan(plan.dst_rowptr, plan.dst_perm, n_dst))
        return self._aggregate_message(x_src, x_dst, edge_index, edge_attr, plan, plan._pair_plans[key])[:n_dst]

    def forward(self, x, edge_index, edge_attr, x_0, size=None):
        route = self.route(x, edge_index, edge_attr)
        if isinstance(edge_attr, IndexedEdgeAttr) and not route.indexed:
            edge_attr = edge_attr.dense()
        if route.kind == "pair":
            x_src, x_dst = x[0], x[1]
            if x_src is None or x_dst is None or not self.final:
                # the reference's update() hands `x` to the hypernetwork (CGAT.py:328-335), which needs a tensor, and its
                # message() concatenates both entries: a pair works there with final=True and two tensors only
                raise TypeError("GATConvNodes: x = (x_source, x_target) needs two tensors and final=True "
                                "(the hypernetwork update takes a single node tensor, as in the reference)")
            return self._propagate_pair(edge_index, x_src, x_dst, edge_attr)
        return self.propagate(edge_index, x, edge_attr, x_0, route)

    def __repr__(self):
        return '{}({}, {}, heads={})'.format(self.__class__.__name__, self.in_channels, self.out_channels, self.heads)


class CGAtNet(nn.Module):
    """The stack driver (CGAT.py:343-613).  Only update_edges=True exists: the reference's
    update_edges=False branch raises at forward (positional-argument bug at CGAT.py:408-421)."""

    def __init__(self, orig_elem_fea_len, elem_fea_len, n_graph, nbr_embedding_size=128, neighbor_number=12,
                 mean_pooling=True, rezero=False, msg_heads=3, update_edges=False, vector_attention=False,
                 global_vector_attention=False, n_graph_roost=3, no_hyper=True):
        super().__init__()
        if not update_edges:
            raise NotImplementedError("CGAtNet(update_edges=False) is broken in the reference "
                                      "(CGAT.py:408-421 raises at forward); use update_edges=True")
        self.mean_pooling = mean_pooling
        self.update_edges = update_edges
        self.embedding = nn.Linear(orig_elem_fea_len, elem_fea_len, bias=False)
        self.nbr_embedding = nn.Embedding(num_embeddings=neighbor_number + 1, embedding_dim=nbr_embedding_size)
        self.no_hyper = no_hyper
        self.graphs = nn.ModuleList([
            nn.ModuleDict({
                'Node': GATConvNodes(elem_fea_len, elem_fea_len, nbr_embedding_size, msg_heads, concat=True,
                                     vector_attention=vector_attention, first=(k == 0)),
                'Edge': GATConvEdges(elem_fea_len, nbr_embedding_size, nbr_embedding_size, msg_heads, concat=True,
                                     vector_attention=vector_attention, first=(k == 0), no_hyper=no_hyper)})
            for k in range(n_graph)])
        self.roost = Roost(orig_elem_fea_len, elem_fea_len, n_graph_roost)
        self.cry_pool = MHAttention(in_channels=elem_fea_len, out_channels=elem_fea_len, heads=msg_heads,
                                    vector_attention=global_vector_attention)
        self.msg_heads = msg_heads
        self.elem_fea_len = elem_fea_len
        out_hidden = [1024, 1024, 512, 512, 256, 256, 128]
        self.output_nn = ResidualNetwork(elem_fea_len if mean_pooling else elem_fea_len * msg_heads, 2, out_hidden,
                                         if_rezero=rezero)

    def forward(self, batch, roost, *, last_layer=True, return_graph_embedding=False):
        edge_index = batch.edge_index
        crystal_elem_idx = batch.batch
        G = getattr(batch, "num_graphs", None)
        if G is None:
            G = int(crystal_elem_idx[-1]) + 1                                   # one host sync per batch
        # The composition branch (reference CGAT.py:593: computed AFTER the graph layers, which it does not depend on) is
        # issued first, on a branch stream at small batches: it then runs beside the graph layers instead of after them
        roost = tuple(roost)                                                    # the harness passes a generator
        main = branch = None
        if batch.x.is_cuda:
            branch = branch_stream(batch.x.device, edge_index.shape[1])
        if branch is not None:
            main = torch.cuda.current_stream(batch.x.device)
            branch.wait_stream(main)
            with torch.cuda.stream(branch):
                crys_comp = self.roost(*roost, num_crystals=G)
        indexed = self._indexed_edges(batch)                                    # (opt-in: ops.set_indexed_edge_attr)
        if not indexed:
            edge_attr = small_embedding(batch.edge_attr, self.nbr_embedding.weight)  # [E] int64 -> [E,Ce]
        elem_fea = linear(batch.x, self.embedding.weight, None)                 # [N,200] -> [N,C]
        elem_fea_0 = elem_fea
        if indexed:
            elem_fea = self._graphs_indexed(batch, elem_fea)
            return self._readout(batch, roost, elem_fea, G, main, branch, crys_comp if branch is not None else None,
                                 last_layer, return_graph_embedding)
        edge_attr_0 = edge_attr
        # (per-layer fork / join: worth it inside a hipGraph, where it is a graph edge -- 13.76 -> 13.45 ms per replayed
        # 64-crystal step; in eager mode the eight extra stream switches cost more host time than the overlap returns)
        ebranch = (branch_stream(batch.x.device, edge_index.shape[1], which=1)
                   if branch is not None and torch.cuda.is_current_stream_capturing() else None)
        for graph_func in self.graphs:
            edge = graph_func['Edge']
            shipped = edge.no_hyper and type(edge).forward is GATConvEdges.forward
            # shipped form: Edge(...) = Pooling_NN(edge_attr) (its attention is dead code, CGAT.py:224-225); the residual
            # add of CGAT.py:582 rides in the same launch.  It is issued BEFORE the node update in every execution mode --
            # on the edge branch stream where there is one -- so that the autograd nodes are created in the same order
            # eagerly and under capture: edge_attr receives three gradient contributions, and the order in which the
            # engine adds them follows the nodes' sequence numbers (a replayed graph is bit-equal to the eager step)
            if shipped and ebranch is not None:
                ebranch.wait_stream(main)
                with torch.cuda.stream(ebranch):
                    new_edge_attr = edge.Pooling_NN(edge_attr, residual=edge_attr)
            elif shipped:
                new_edge_attr = edge.Pooling_NN(edge_attr, residual=edge_attr)
            node_update = graph_func['Node'](elem_fea, edge_index, edge_attr, elem_fea_0)
            if shipped and ebranch is not None:
                main.wait_stream(ebranch)
                new_edge_attr.record_stream(main)
                edge_attr.record_stream(ebranch)
            if shipped:
                edge_attr = new_edge_attr
            else:
                edge_attr = edge_attr + edge(elem_fea, edge_index, edge_attr, edge_attr_0)
            elem_fea = elem_fea + node_update
        return self._readout(batch, roost, elem_fea, G, main, branch, crys_comp if branch is not None else None,
                             last_layer, return_graph_embedding)

    def _indexed_edges(self, batch):
        """The shell-indexed form of the edge features applies (ops.set_indexed_edge_attr): the switch is on, every Edge
        layer is the shipped row-wise form, and batch.edge_attr holds integer ids on the GPU.  One layer that fails
        sends the whole forward down the dense path."""
        ea = batch.edge_attr
        return (get_indexed_edge_attr() and torch.is_tensor(ea) and ea.is_cuda and ea.dim() == 1 and
                not ea.is_floating_point() and not ea.is_complex() and ea.dtype != torch.bool and
                self.nbr_embedding.weight.is_cuda and self.nbr_embedding.weight.dtype == torch.float32 and
                all(g['Edge'].no_hyper and type(g['Edge']).forward is GATConvEdges.forward for g in self.graphs))

    def _graphs_indexed(self, batch, elem_fea):
        """The graph layers on edge_attr_l[e] = T_l[shell[e]]: the edge update and its residual run
        on the R = neighbor_number + 1 rows of the table -- a small-row program on the main stream, no edge branch -- and
        the node layers take the lookup (without grad: no per-edge product; with grad: one gather per layer, whose
        backward is the deterministic per-class row sum)."""
        elem_fea_0 = elem_fea
        index = batch.edge_attr if batch.edge_attr.dtype == torch.int64 else batch.edge_attr.long()
        ea = IndexedEdgeAttr(self.nbr_embedding.weight, index)
        if self._edge_tables_ahead(ea.table):
            # no grad: T_l depends on the edge networks alone, so every layer's table comes from ONE small-row launch
            # issued ahead of the node layers (the same products as below, bit for bit; the last update feeds nothing)
            tables = self._edge_tables(ea.table)
            for graph_func, table in zip(self.graphs, tables):
                elem_fea = elem_fea + graph_func['Node'](elem_fea, batch.edge_index, ea.with_table(table), elem_fea_0)
            return elem_fea
        for graph_func in self.graphs:
            node_update = graph_func['Node'](elem_fea, batch.edge_index, ea, elem_fea_0)
            pool = graph_func['Edge'].Pooling_NN
            ea = ea.with_table(pool(ea.table, residual=ea.table))
            if debug.recording():
                debug.expand_last([fc.weight for fc in pool.fcs], ea.index)
            elem_fea = elem_fea + node_update
        return elem_fea

    def _edge_tables_ahead(self, table):
        pools = [g['Edge'].Pooling_NN for g in self.graphs]
        return (not torch.is_grad_enabled() and not debug.recording() and rowprog.eligible(table) and
                2 * (len(pools) - 1) <= _lib.ROWPROG_MAX_OPS and
                all(type(p) is SimpleNetwork and len(p.fcs) == 1 and p.fcs[0].bias is not None and
                    p.fc_out.bias is not None and p.fc_out.weight.shape[0] == table.shape[1] and
                    p.fcs[0].weight.shape[1] == table.shape[1] for p in pools))

    def _edge_tables(self, table):
        """[T_0, ..., T_{L-1}] with T_{l+1} = T_l + Edge_l.Pooling_NN(T_l) as one small-row program: per layer the two
        ops SimpleNetwork.forward(T_l, residual=T_l) runs, phases in sequence."""
        R, dev = table.shape[0], table.device
        cur = table.detach()
        tables, prog = [cur], []
        for g in list(self.graphs)[:-1]:
            pool = g['Edge'].Pooling_NN
            w1, wo = pool.fcs[0].weight.detach(), pool.fc_out.weight.detach()
            hid = torch.empty(R, w1.shape[0], dtype=torch.float32, device=dev)
            out = torch.empty(R, wo.shape[0], dtype=torch.float32, device=dev)
            prog.append(rowprog.op(len(prog), R, w1.shape[0], w1.shape[1], cur, w1, hid, bias=pool.fcs[0].bias.detach(),
                                   act=_lib.ACT_LEAKY))
            prog.append(rowprog.op(len(prog), R, wo.shape[0], wo.shape[1], hid, wo, out, bias=pool.fc_out.bias.detach(),
                                   resid=cur))
            tables.append(out)
            cur = out
        if prog:
            rowprog.run(prog, dev)
        return tables

    def _readout(self, batch, roost, elem_fea, G, main, branch, crys_comp, last_layer, return_graph_embedding):
        crystal_elem_idx = batch.batch
        if branch is not None:
            main.wait_stream(branch)
            crys_comp.record_stream(main)
        else:
            crys_comp = self.roost(*roost, num_crystals=G)
        crys_fea = self.cry_pool(elem_fea, crys_comp, crystal_elem_idx, size=G)
        if self.mean_pooling:
            crys_fea = crys_fea.view(-1, self.msg_heads, self.elem_fea_len).mean(dim=1)
        if return_graph_embedding:
            return crys_fea
        return self.output_nn(crys_fea, last_layer=last_layer)

    def __repr__(self):
        return self.__class__.__name__

    def get_output_parameters(self):
        return self.output_nn.parameters()

    def get_hidden_parameters(self):
        return itertools.chain(self.embedding.parameters(), self.nbr_embedding.parameters(),
                               self.graphs.parameters(), self.roost.parameters(), self.cry_pool.parameters())
