"""The shell-indexed edge route (csrc/edgeidx.hip) at the shapes its other tests do not launch: the class plan bit for bit
against numpy, and layer parity on one small graph that takes every segment path, for every instantiation KQ =
ceil(H * Hd / 256) that tests/test_indexed_edge_attr.py::OP_CASES leaves out, long segments under every waves-per-workgroup
pair, heads that straddle a wave pass, and dead lanes (DESIGN.md section 10a has the map of cases).

Tolerances, both the project's own and unchanged (tests/test_indexed_edge_attr.py, tests/test_indexed_edge_training.py):
  flat   1e-4 of the largest reference entry per tensor, through test_hip_golden.py::_compare_with_oracle with the
         route's own derivative pattern forced on the oracle
  ratio  against the oracle in fp64 on the same inputs, the indexed route's largest error is at most 2 x the dense
         route's
The class plan is integers: np.array_equal.  Every figure is printed before it is asserted."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from indexed_cases import PLAN_CASES, class_index, class_plan_reference
from test_fused_inference import DEV, _mode
from test_indexed_edge_attr import FLAT, RATIO, _check_both, _index, _maxerr, _oracle_refs
from test_indexed_edge_attr import _tags as _infer_tags
from test_indexed_edge_training import (GRAD_NAMES, _assert_dense_tags, _assert_indexed_tags, _final_layer, _step, _tags,
                                        _train)

pytestmark = pytest.mark.gpu
SENTINEL = -7


# ---------------------------------------------------------------------------------------------------------------------
# 1. the class plan, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _run_class_plan(plan, index, R):
    """cgat_indexed_class_plan through the C ABI into arrays filled with a sentinel: (cls_pos, piece_start, piece_rowptr)
    as numpy."""
    from cgat_amd import _lib
    lib = _lib.lib
    E = plan.E
    n_max = lib.cgat_indexed_class_pieces(E, R)
    i32 = dict(dtype=torch.int32, device=DEV)
    cls_pos, piece_start = torch.full((E,), SENTINEL, **i32), torch.full((R + 1,), SENTINEL, **i32)
    piece_rowptr = torch.full((n_max + 1,), SENTINEL, **i32)
    nbytes = lib.cgat_indexed_class_plan_workspace_bytes(E, R)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    vp = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    rc = lib.cgat_indexed_class_plan(C.byref(plan.c), vp(index), R, vp(cls_pos), vp(piece_start), vp(piece_rowptr), vp(ws),
                                     nbytes, None)
    torch.cuda.synchronize()
    assert rc == 0, (rc, lib.cgat_last_error())
    return cls_pos.cpu().numpy(), piece_start.cpu().numpy(), piece_rowptr.cpu().numpy()


@pytest.mark.parametrize("E,R,dist", PLAN_CASES, ids=lambda v: str(v))
def test_class_plan_bit_exact(E, R, dist):
    """All of cls_pos [E], piece_start [R + 1] and piece_rowptr [cgat_indexed_class_pieces(E, R) + 1] against
    indexed_cases.class_plan_reference, the filled tail and the clamp of out-of-range values included; twice (the count
    kernel's LDS atomics are integer adds: order-free)."""
    from cgat_amd import _lib, ops
    N = 500
    g = torch.Generator().manual_seed(17 + E)
    ei = torch.randint(0, N, (2, E), generator=g).to(DEV)               # random destinations, in random order
    plan = ops.get_plan(ei, N)
    dst_perm = plan.dst_perm.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(dst_perm), np.arange(E))
    assert E < 255 or not np.array_equal(dst_perm, np.arange(E)), "dst_perm is the identity"
    index = class_index(E, R, dist)
    want = class_plan_reference(index, dst_perm, R, _lib.lib.cgat_indexed_class_pieces(E, R))
    index_gpu = torch.from_numpy(index).to(DEV)
    got = _run_class_plan(plan, index_gpu, R)
    again = _run_class_plan(plan, index_gpu, R)
    total = int(want[1][R])
    for name, a, b, w in zip(("cls_pos", "piece_start", "piece_rowptr"), got, again, want):
        bad = int((a != w).sum()) if a.shape == w.shape else -1
        print(f"[indexed-shapes] plan ({E}, {R}, {dist}) {name} [{a.shape[0]}]: {bad} entries differ from numpy, "
              f"{int((a == SENTINEL).sum())} unwritten; pieces {total} of {want[2].shape[0] - 1}")
    for name, a, b, w in zip(("cls_pos", "piece_start", "piece_rowptr"), got, again, want):
        assert np.array_equal(a, w), name
        assert np.array_equal(a, b), name + " (second call)"


# ---------------------------------------------------------------------------------------------------------------------
# 2. one small graph that takes every segment path
# ---------------------------------------------------------------------------------------------------------------------
HUB_DEG = {60: 1000, 9: 300, 7: 257, 8: 256, 0: 0, 30: 0, 59: 0}


@functools.lru_cache(maxsize=None)
def _hub61(odd=False):
    """N = 61 (no multiple of the 4, 8 or 16 segments of a workgroup): the last node with 1 000 incoming edges, node 9 with
    300, node 7 with 257 (the shortest long segment), node 8 with 256 (the longest ordinary one), nodes 0, 30 and 59 with
    none, the others with 1 - 23; three long segments in the one list of the workgroups behind.  Sources uniform, edges in
    random order, E % 4 == 0; odd: one edge more."""
    rs = np.random.RandomState(61)
    N = 61
    deg = rs.randint(1, 24, size=N).astype(np.int64)
    for n, d in HUB_DEG.items():
        deg[n] = d
    deg[1] += (4 - int(deg.sum()) % 4) % 4 + (1 if odd else 0)
    E = int(deg.sum())
    dst = np.repeat(np.arange(N), deg)
    src = rs.randint(0, N, size=E)
    order = rs.permutation(E)
    ei = torch.from_numpy(np.stack([src[order], dst[order]])).long()
    got = np.bincount(ei[1].numpy(), minlength=N)
    assert all(got[n] == d for n, d in HUB_DEG.items()), got
    ordinary = np.array([n for n in range(N) if n not in HUB_DEG])
    assert got[ordinary].min() >= 1 and got[ordinary].max() <= 27
    assert E % 4 == (1 if odd else 0) and int((got > 256).sum()) == 3 and N % 4 != 0
    assert int(ei[0].min()) >= 0 and int(ei[0].max()) < N and not bool((np.diff(ei[1].numpy()) >= 0).all())
    return N, ei


SKEW_R = 256
SKEW_CLASSES = {0: 1, 3: 256, 4: 257, 200: 513}          # class 255 takes the rest; every other class is empty


def _skew_index(E):
    """Classes over a random permutation of the edges, so that every class is spread over many destinations: the class
    sum at its piece boundaries (1, 256, 257 and 2 x 256 + 1 rows), beside one class of five pieces."""
    rest = E - sum(SKEW_CLASSES.values())
    assert rest > 1024
    cls = np.concatenate([np.full(n, r, dtype=np.int64) for r, n in SKEW_CLASSES.items()] + [np.full(rest, 255, dtype=np.int64)])
    idx = np.empty(E, dtype=np.int64)
    idx[np.random.RandomState(7).permutation(E)] = cls
    n = np.bincount(idx, minlength=SKEW_R)
    assert all(n[r] == c for r, c in SKEW_CLASSES.items()) and n[255] == rest and int((n > 0).sum()) == 5
    return torch.from_numpy(idx)


# (C, H, R, index kind, arithmetic mode, odd graph); Hd = 2 C, KQ = ceil(H * Hd / 256)
SHAPE_CASES = (
    (128, 2, 13, "even", "f16x3c", False),     # KQ 2: bwd_msg's 16-wave split on long segments
    (128, 4, 256, "skew", "f16x3c", False),    # KQ 4: logits 16 waves / bwd_msg 8; the class sum at piece boundaries
    (128, 4, 256, "skew", "f16x3c", True),     #       E % 4 == 1
    (128, 6, 13, "even", "f16x3c", False),     # KQ 6: logits 8 / bwd_msg 4
    (128, 6, 13, "even", "f32", False),
    (128, 7, 1, "even", "f16x3c", False),      # KQ 7
    (64, 8, 25, "even", "f16x3c", False),      # KQ 4, Hd = 128: two heads per wave pass
    (96, 3, 13, "even", "f16x3c", False),      # KQ 3, Hd = 192: heads straddle passes, dead lanes in the last pass
    (96, 3, 13, "even", "f32", False),
    (40, 2, 13, "even", "f16x3c", False),      # KQ 1, Hd = 80: 24 dead lanes
)
_ids = lambda c: f"C{c[0]}-H{c[1]}-R{c[2]}-{c[3]}-{c[4]}" + ("-odd" if c[5] else "")


def _shape_inputs(C_, R, kind, odd):
    N, ei = _hub61(odd)
    E = ei.shape[1]
    g = torch.Generator().manual_seed(6)
    x, table = torch.randn(N, C_, generator=g), torch.randn(R, C_, generator=g)
    index = _skew_index(E) if kind == "skew" else _index(E, R)
    return N, ei, x, table, index


def _cot(N, C_):
    return torch.randn(N, C_, generator=torch.Generator().manual_seed(9))


def _call(m, i):
    import cgat_amd as P
    if isinstance(m, P.GATConvNodes):
        return m(i["x"], i["edge_index"], P.IndexedEdgeAttr(i["table"], i["index"]), None)
    return m(i["x"], i["edge_index"], torch.nn.functional.embedding(i["index"], i["table"]), None)


def _table_rows(label, gt, index, R):
    """Unused rows of table.grad exactly zero, used rows non-zero."""
    used = torch.zeros(R, dtype=torch.bool)
    used[index.unique()] = True
    row_max = gt.abs().amax(dim=1).cpu()
    print(f"[indexed-shapes] {label} table.grad row maxima: used min {float(row_max[used].min()):.3e}, unused max "
          f"{float(row_max[~used].max()) if (~used).any() else 0.0:.3e}")
    assert bool((row_max[~used] == 0).all()) and bool((row_max[used] > 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 3. the training route
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SHAPE_CASES, ids=_ids)
def test_training_gradients_vs_oracle(case):
    """test_indexed_edge_training.py::test_layer_gradients_vs_oracle on _hub61: every tensor of the step (the output and
    the gradients of x, table and the eight parameters) flat against the oracle, the indexed launches and none of the
    dense per-edge ones, the unused rows of table.grad exactly zero."""
    import cgat_amd as P
    from cgat_amd import ops
    from oracle import cgat_oracle as O
    from test_hip_golden import _compare_with_oracle
    C_, H, R, kind, mode, odd = case
    N, ei, x, table, index = _shape_inputs(C_, R, kind, odd)
    inputs = {"x": x, "edge_index": ei, "table": table, "index": index}
    mk = lambda ns: (lambda: ns.GATConvNodes(C_, C_, C_, H, concat=True, final=True))
    with _mode(mode), _train(True):
        assert ops.train_indexed_ok(ops.get_plan(ei.to(DEV), N).c, C_, C_, H, 2 * C_, R)
        worst = _compare_with_oracle(mk(P), mk(O), inputs, _call, tol=FLAT, label=f"indexed_shapes {_ids(case)}")
        _, pm = _final_layer(C_, H)
        (y, g), t = _tags(lambda: _step(pm, x.to(DEV), ei.to(DEV), table.to(DEV), index.to(DEV), _cot(N, C_).to(DEV)))
    # (err/|ref| per tensor: the table _compare_with_oracle prints.  Its `worst` counts MH_A.fc_out.bias, whose gradient is
    # zero in exact arithmetic -- |ref| ~ 1e-16 -- and which it holds to the zero-gradient floor)
    print(f"[indexed-shapes] train {_ids(case)}: KQ {-(-H * 2 * C_ // 256)}, worst err/|ref| with the zero gradient "
          f"{worst:.3e}; tags {t}")
    _assert_indexed_tags(t)       # (_compare_with_oracle has asserted every tensor, GRAD_NAMES among them)
    assert set(GRAD_NAMES) <= set(g) and all(g[k] is not None and bool(torch.isfinite(g[k]).all()) for k in GRAD_NAMES)
    _table_rows(_ids(case), g["table"], index, R)


@pytest.mark.parametrize("case", SHAPE_CASES, ids=_ids)
def test_forward_bits_and_repeatability(case):
    """The training forward's bits are the no-grad forward's, and a second training step is the first bit for bit: the
    order of the long-segment list (an LDS atomic counter) reaches no result."""
    import cgat_amd as P
    C_, H, R, kind, mode, odd = case
    N, ei, x, table, index = _shape_inputs(C_, R, kind, odd)
    _, pm = _final_layer(C_, H)
    x, ei, table, index, cot = x.to(DEV), ei.to(DEV), table.to(DEV), index.to(DEV), _cot(N, C_).to(DEV)
    with _mode(mode), _train(True):
        (y1, g1), t = _tags(lambda: _step(pm, x, ei, table, index, cot))
        y2, g2 = _step(pm, x, ei, table, index, cot)
        with torch.no_grad():
            y0, t0 = _tags(lambda: pm(x, ei, P.IndexedEdgeAttr(table, index), None))
    _assert_indexed_tags(t)
    assert t0["edge_idx_logits"] > 0 and t0["edge_idx_wsum"] > 0 and t0["seg_wsum"] == 0 and t0["edge_z"] == 0, t0
    diff = {k: _maxerr(g1[k], g2[k]) for k in GRAD_NAMES}
    print(f"[indexed-shapes] bits {_ids(case)}: training - no-grad forward {_maxerr(y1, y0):.3e}; second step - first: "
          f"out {_maxerr(y1, y2):.3e}, gradients {max(diff.values()):.3e}")
    assert torch.equal(y1, y0)
    assert torch.equal(y1, y2)
    for k in GRAD_NAMES:
        assert torch.equal(g1[k], g2[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 4. the route without grad
# ---------------------------------------------------------------------------------------------------------------------
def _no_grad_case(label, C_, H, R, kind, mode, odd):
    """The layer under torch.no_grad() on the indexed launches: flat against the fp32 oracle, and the ratio rule against
    the dense no-grad route on table[index] against the fp64 oracle."""
    import cgat_amd as P
    from cgat_amd import ops
    N, ei, x, table, index = _shape_inputs(C_, R, kind, odd)
    om, pm = _final_layer(C_, H)
    want32, want64 = _oracle_refs(("hub61", C_, H, R, kind, odd), om, x, ei, table[index], None)
    x, ei, table, index = x.to(DEV), ei.to(DEV), table.to(DEV), index.to(DEV)
    with _mode(mode), torch.no_grad():
        assert ops.infer_indexed_ok(ops.get_plan(ei, N).c, C_, C_, H, pm.MH_A.hidden_layer_dim, R)
        got, t = _infer_tags(lambda: pm(x, ei, P.IndexedEdgeAttr(table, index), None))
        dense, td = _infer_tags(lambda: pm(x, ei, table[index], None))
    print(f"[indexed-shapes] no-grad {label}: tags {t}")
    assert t["edge_idx_logits"] > 0 and t["edge_idx_wsum"] > 0, t
    assert all(t[k] == 0 for k in ("edge_logits", "edge_msg_wsum", "edge_z", "seg_wsum")), t
    assert td["edge_idx_logits"] == 0 and td["edge_idx_wsum"] == 0, td
    _check_both(f"shapes no-grad {label}", got, dense, want32, want64)


@pytest.mark.parametrize("case", SHAPE_CASES, ids=_ids)
def test_no_grad_vs_dense_and_fp64(case):
    _no_grad_case(_ids(case), *case)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the class sum at piece boundaries, row by row
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odd", [False, True], ids=["even", "odd"])
def test_skew_table_grad_row_by_row(odd):
    """C = 128, H = 4, R = 256 with classes of exactly 1, 256, 257 and 513 edges beside one of five pieces: every used row
    of table.grad within FLAT of ITS OWN largest reference entry (the oracle in fp64 with the pattern this run recorded
    forced on it) -- a dropped or doubled row of the 1-edge class would vanish in the max-norm of the tensor."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    C_, H, R = 128, 4, SKEW_R
    N, ei_cpu, x_cpu, table_cpu, index_cpu = _shape_inputs(C_, R, "skew", odd)
    om, pm = _final_layer(C_, H)
    om64 = copy.deepcopy(om).double()
    cot_cpu = _cot(N, C_)
    rec = P.debug.record_masks(pm)
    with _mode("f16x3c"), _train(True), rec as masks:
        (_, g), t = _tags(lambda: _step(pm, x_cpu.to(DEV), ei_cpu.to(DEV), table_cpu.to(DEV), index_cpu.to(DEV),
                                        cot_cpu.to(DEV)))
    _assert_indexed_tags(t)
    xr, tr = x_cpu.double().requires_grad_(True), table_cpu.double().requires_grad_(True)
    with O.forced_masks(om64, masks):
        y = om64(xr, ei_cpu, torch.nn.functional.embedding(index_cpu, tr), None)
        (ref,) = torch.autograd.grad((y * cot_cpu.double()).sum(), [tr])
    got = g["table"].double().cpu()
    n = np.bincount(index_cpu.numpy(), minlength=R)
    worst = 0.0
    for r in range(R):
        if n[r] == 0:
            continue
        err, ref_max = float((got[r] - ref[r]).abs().max()), float(ref[r].abs().max())
        worst = max(worst, err / ref_max)
        print(f"[indexed-shapes] skew odd={odd} table.grad row {r} ({n[r]} edges): err {err:.3e} |ref| {ref_max:.3e} "
              f"err/|ref| {err / ref_max:.3e}")
    unused = torch.from_numpy(n == 0)
    assert bool((got[unused] == 0).all()) and bool((ref[unused] == 0).all())
    for r in range(R):
        if n[r]:
            assert float((got[r] - ref[r]).abs().max()) <= FLAT * float(ref[r].abs().max()), (r, int(n[r]))


# ---------------------------------------------------------------------------------------------------------------------
# 6. H * Hd = 240: the route without grad takes it, the training route densifies
# ---------------------------------------------------------------------------------------------------------------------
def test_c40_h3_no_grad_indexed_training_dense():
    """C = 40, H = 3: Hd = 80, H * Hd = 240 is no multiple of the 32 columns of a sign word.  infer_indexed_ok holds and
    train_indexed_ok does not: without grad the layer runs the indexed launches, a training step under the switch runs
    the dense ones, and both meet the flat bound."""
    import cgat_amd as P
    from cgat_amd import ops
    from oracle import cgat_oracle as O
    from test_hip_golden import _compare_with_oracle
    C_, H, R = 40, 3, 13
    N, ei, x, table, index = _shape_inputs(C_, R, "even", False)
    plan = ops.get_plan(ei.to(DEV), N)
    assert ops.infer_indexed_ok(plan.c, C_, C_, H, 2 * C_, R) and not ops.train_indexed_ok(plan.c, C_, C_, H, 2 * C_, R)
    _no_grad_case("C40-H3-R13", C_, H, R, "even", "f16x3c", False)
    inputs = {"x": x, "edge_index": ei, "table": table, "index": index}
    mk = lambda ns: (lambda: ns.GATConvNodes(C_, C_, C_, H, concat=True, final=True))
    with _mode("f16x3c"), _train(True):
        worst = _compare_with_oracle(mk(P), mk(O), inputs, _call, tol=FLAT, label="indexed_shapes C40-H3 (dense)")
        _, pm = _final_layer(C_, H)
        (y, g), t = _tags(lambda: _step(pm, x.to(DEV), ei.to(DEV), table.to(DEV), index.to(DEV), _cot(N, C_).to(DEV)))
    print(f"[indexed-shapes] train C40-H3-R13 (densified): worst err/|ref| with the zero gradient {worst:.3e}; tags {t}")
    _assert_dense_tags(t)
    _table_rows("C40-H3-R13", g["table"], index, R)
