"""The HBM-bound helper kernels of the backward (csrc/rowops.hip) -- column sums, the LayerNorm+tanh backward, the damping
mix backward and its partial sum -- at the shapes where the way threads map to their work can go wrong.  Their summation
orders and roundings are a contract (written above each kernel); the kernels were re-mapped for bandwidth under it.

Checks per case:
 * the bits of the parent build: tests/golden/row_helpers_parent.json holds, per case, the SHA-256 of the output bytes and four
   sampled words (uint32), recorded with the build of the commit named in the file by
       python tests/test_row_helpers.py --record FILE --tree CHECKOUT
   Equality is exact.
 * parity with the float64 result over the same inputs: column sums at the TOL of tests/test_hip_kernels.py, the LayerNorm
   backward at that file's 5e-5; the hypernetwork and attention backward, which tests/test_hip_kernels.py does not run, at
   the criterion of their own parity tests (tests/test_hnet_routes.py: TOL of tests/oracle_cases.py, and the floor for
   gradients that are zero in exact arithmetic, such as the attention logit bias by the softmax's shift invariance).
 * column sums also against a numpy float32 emulation of the documented order (pure additions, then one multiplication by
   alpha: the emulation is exact, so is the comparison), alpha = 0.5 included -- that one through cgat_debug_colsum, since
   every bias gradient passes alpha = 1.  The emulation itself is compared with the float64 sum on the CPU.

Every operand buffer is NaN outside [rows, cols], 64 rows past the end included.

Column sums through cgat_linear_backward's bias gradient: rows {1, 3, 4, 5, 127, 128, 129, 513, 16 385} (16 385: three
levels, 129 chunks -> 2 -> 1) x cols {1, 3, 5 (narrow form), 63, 65 (generic), 64, 128, 132, 1536 (wide form)} x leading
dimension {tight, cols + 4 with the base four bytes off the 16-byte grid: the wide form's fallback}.
LayerNorm backward: rows {1, 3, 4, 5, 257, 1023} at W = 128; W = 64 and W = 200 (the kept kernel); a row of equal values;
|u| up to 2^10.  Hypernetwork backward with damping: rows {1, 65, 300, 2049} (2049 x 128 elements pass mix_bwd's cap of 1024
workgroups) x {2, 4} predicted layers.  Attention backward, H = 3, Hd = 256, C = Ce = 128: N = 40 and N = 1400 with K = 12
incoming edges each (E = 16 800: three column-sum levels over ga) plus one node without an incoming edge; inputs and
first-layer weights on a dyadic grid with odd biases, so that every pre-activation is exact and non-zero in fp32 and fp64
alike and both take the same LeakyReLU derivative.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "row_helpers_parent.json")
TOL = 2e-5                    # tests/test_hip_kernels.py
LN_TOL = 5e-5                 # tests/test_hip_kernels.py, test_layernorm_tanh
PAR_TOL, ZERO_FLOOR, NUM_ZERO = 1e-4, 1e-6, 1e-7   # tests/oracle_cases.py, as tests/test_hnet_routes.py applies them
SAMPLES = 4
CS_ROWS = [1, 3, 4, 5, 127, 128, 129, 513, 16385]
CS_COLS = [1, 3, 5, 63, 64, 65, 128, 132, 1536]
CS_LDS = ["tight", "padded"]
COLSUM = [(r, c, ld) for r in CS_ROWS for c in CS_COLS for ld in CS_LDS]
LN = [("rows", 1, 128), ("rows", 3, 128), ("rows", 4, 128), ("rows", 5, 128), ("rows", 257, 128), ("rows", 1023, 128),
      ("rows", 257, 64), ("rows", 5, 200), ("equal", 5, 128), ("wide", 257, 128)]
HNET = [(n_hyper, rows) for n_hyper in (2, 4) for rows in (1, 65, 300, 2049)]
ATTN = [40, 1400]
gpu = pytest.mark.gpu


def case_id(c):
    return "-".join(map(str, c)) if isinstance(c, tuple) else str(c)


def fingerprint(ts):
    """{"sha256", "samples"} of the tensors' bytes, in order."""
    h = hashlib.sha256()
    samples = []
    for t in ts:
        flat = t.detach().contiguous().view(-1).cpu()
        h.update(flat.numpy().tobytes())
        idx = torch.linspace(0, flat.numel() - 1, SAMPLES).long()
        samples += [int(x) for x in flat[idx].view(torch.int32).tolist()]
    return {"sha256": h.hexdigest(), "samples": [x & 0xFFFFFFFF for x in samples]}


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    d = b.abs().max().item()
    return (a - b).abs().max().item() / (d if d > 0 else 1.0)


def _place(t, ld, off):
    """t's values at leading dimension ld, `off` floats into a NaN buffer that extends 64 rows past the end."""
    rows, cols = t.shape
    buf = torch.full(((rows + 64) * ld + 8,), float("nan"), dtype=torch.float32, device=t.device)
    view = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t)
    return buf, view


def _mode():
    from cgat_amd import ops

    class M:
        def __enter__(self):
            self.was = ops.get_bilinear_mode()
            ops.set_bilinear_mode("f16x3c")

        def __exit__(self, *exc):
            ops.set_bilinear_mode(self.was)
    return M()


# ---- column sums ----
def colsum_values(case):
    rows, cols, ld = case
    g = torch.Generator().manual_seed(104729 * rows + 131 * cols + len(ld))
    return torch.randn(rows, cols, generator=g)


def make_colsum(case, dev):
    rows, cols, ld = case
    pad = ld == "padded"
    buf, x = _place(colsum_values(case).to(dev), cols + 4 if pad else cols, 1 if pad else 0)
    assert x.data_ptr() % 16 == (4 if pad else 0)
    return buf, x


def run_colsum_bias(x):
    """The bias gradient of cgat_linear_backward alone (no input or weight gradient, no activation): column sums of g_y."""
    from cgat_amd import _lib
    rows, cols = x.shape
    out = torch.full((cols,), float("nan"), device=x.device)
    ws = torch.full((_lib.lib.cgat_linear_backward_workspace_bytes(rows, 128, cols),), 0xFF, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib.cgat_linear_backward(None, 128, None, 128, None, cols, x.data_ptr(), x.stride(0), None, None, 128, 0,
                                             None, 128, out.data_ptr(), rows, 128, cols, 0, ws.data_ptr(), ws.numel(), None),
               "cgat_linear_backward")
    torch.cuda.synchronize()
    return out


def run_colsum_debug(x, alpha):
    from cgat_amd import _lib
    rows, cols = x.shape
    out = torch.full((cols,), float("nan"), device=x.device)
    ws = torch.full((_lib.lib.cgat_debug_colsum_workspace_bytes(rows, cols),), 0xFF, dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib.cgat_debug_colsum(x.data_ptr(), x.stride(0), rows, cols, out.data_ptr(), alpha, ws.data_ptr(), ws.numel(),
                                          None), "cgat_debug_colsum")
    torch.cuda.synchronize()
    return out


def emulate_colsum(x, alpha):
    """The documented order in numpy float32: per 128-row chunk four lane sums over rows r0 + rl, r0 + rl + 4, ... ascending,
    from 0.f (rows past the end add +0.f, which changes nothing); (red0 + red1) + red2) + red3, times alpha; the same over
    the partials (alpha 1) until one chunk is left."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    a = np.float32(alpha)
    while True:
        rows, cols = x.shape
        chunks = max(1, -(-rows // 128))
        p = np.zeros((chunks * 128, cols), dtype=np.float32)
        p[:rows] = x
        p = p.reshape(chunks, 32, 4, cols)
        s = np.zeros((chunks, 4, cols), dtype=np.float32)
        for j in range(32):
            s = s + p[:, j]
        x = a * (((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3])
        a = np.float32(1.0)
        if chunks == 1:
            return x[0]


@pytest.mark.parametrize("rows", CS_ROWS)
def test_colsum_emulation_matches_float64(rows):
    """No GPU: the emulated order against the float64 sum, every column count, both alphas."""
    for cols in CS_COLS:
        v = colsum_values((rows, cols, "tight"))
        for alpha in (1.0, 0.5):
            got = torch.from_numpy(emulate_colsum(v.numpy(), alpha))
            assert rel(got, alpha * v.double().sum(0)) <= TOL, (rows, cols, alpha)


@gpu
@pytest.mark.parametrize("case", COLSUM, ids=case_id)
def test_colsum(case, golden):
    dev = torch.device("cuda:0")
    buf, x = make_colsum(case, dev)
    v = x.cpu()
    out = run_colsum_bias(x)
    half = run_colsum_debug(x, 0.5)
    err, err_half = rel(out, v.double().sum(0)), rel(half, 0.5 * v.double().sum(0))
    print(f"  {case_id(case)} err/|ref| {err:.2e} (alpha 0.5: {err_half:.2e})")
    assert torch.isfinite(out).all() and torch.isfinite(half).all()
    assert err <= TOL and err_half <= TOL
    assert np.array_equal(out.cpu().numpy().view(np.uint32), emulate_colsum(v.numpy(), 1.0).view(np.uint32))
    assert np.array_equal(half.cpu().numpy().view(np.uint32), emulate_colsum(v.numpy(), 0.5).view(np.uint32))
    assert torch.equal(run_colsum_debug(x, 1.0), out)
    got, want = fingerprint([out]), golden["colsum/" + case_id(case)]
    assert got["samples"] == want["samples"]
    assert got["sha256"] == want["sha256"]


# ---- LayerNorm + tanh backward ----
def make_ln(case, dev):
    kind, rows, W = case
    g = torch.Generator().manual_seed(7 * rows + W + 1000 * ["rows", "equal", "wide"].index(kind))
    u, gy = torch.randn(rows, W, generator=g), torch.randn(rows, W, generator=g)
    if kind == "equal":
        u[2] = 0.75
    if kind == "wide":
        u.mul_(torch.exp2(torch.randint(-4, 11, u.shape, generator=g).float()) / 4.0)   # |u| up to about 2^10
    return [_place(t.to(dev), W, 0) for t in (u, gy)]


def run_ln(case, o):
    """(y, gu): y from the library's forward (not touched by the change), so that both builds see the same bits."""
    from cgat_amd import _lib
    kind, rows, W = case
    (_, u), (_, gy) = o
    ybuf, y = _place(torch.zeros(rows, W, device=u.device), W, 0)
    gu = torch.full((rows, W), float("nan"), device=u.device)
    _lib.check(_lib.lib.cgat_layernorm_tanh_forward(u.data_ptr(), y.data_ptr(), rows, W, 1e-5, None), "ln fwd")
    _lib.check(_lib.lib.cgat_layernorm_tanh_backward(u.data_ptr(), y.data_ptr(), gy.data_ptr(), gu.data_ptr(), rows, W, 1e-5,
                                                     None), "ln bwd")
    torch.cuda.synchronize()
    return y, gu


@gpu
@pytest.mark.parametrize("case", LN, ids=case_id)
def test_layernorm_tanh_backward(case, golden):
    kind, rows, W = case
    o = make_ln(case, torch.device("cuda:0"))
    y, gu = run_ln(case, o)
    ud = o[0][1].double().cpu().requires_grad_(True)
    yr = torch.tanh(torch.nn.functional.layer_norm(ud, [W], eps=1e-5))
    (gur,) = torch.autograd.grad(yr, ud, o[1][1].double().cpu())
    err = rel(gu, gur)
    print(f"  {case_id(case)} err/|ref| {err:.2e}")
    assert torch.isfinite(gu).all()
    assert err <= LN_TOL
    got, want = fingerprint([gu]), golden["ln/" + case_id(case)]
    assert got["samples"] == want["samples"]
    assert got["sha256"] == want["sha256"]


# ---- hypernetwork backward with damping ----
def make_hnet(n_hyper, rows, dev):
    W, n_fc = 128, 2
    g = torch.Generator().manual_seed(9000 + 10 * rows + n_hyper)
    rn = lambda *s: torch.randn(*s, generator=g)
    o = {"h0": rn(rows, W), "v": rn(rows, W), "g_y": rn(rows, W), "damping": torch.tensor([0.3])}
    flat = []
    for _ in range(n_hyper):
        flat += [rn(W, W) * (2.0 / W) ** 0.5 for _ in range(n_fc)]
        flat += [rn(W) * 0.1 for _ in range(n_fc)]
        flat += [rn(W * W + W, W) * 0.1 * (2.0 / W) ** 0.5, rn(W * W + W) * 0.05]
    o = {k: t.to(dev) for k, t in o.items()}
    o["flat"] = [t.to(dev) for t in flat]
    return o


def run_hnet(n_hyper, o):
    """[g_h0, g_v, g_damping, head weight gradient of every predicted layer] of the serial backward."""
    from cgat_amd import ops
    y, saved, d, flat = ops._hnet_forward(o["h0"], o["v"], o["damping"], 2, n_hyper, o["flat"])
    g_h0, g_v, g_d, grads, _ = ops._hnet_backward(o["h0"], o["v"], saved, d, flat, 2, n_hyper, o["g_y"])
    torch.cuda.synchronize()
    return [g_h0, g_v, g_d] + [grads[l * 6 + 4] for l in range(n_hyper)]


def _within(names, got, ref, case_scale):
    bad = []
    for name, a, r in zip(names, got, ref):
        ref_max = float(r.abs().max())
        err = float((a.detach().double() - r).abs().max())
        floor = ZERO_FLOOR * case_scale if ref_max <= NUM_ZERO * case_scale else 0.0
        print(f"  {name:12s} err {err:.3e} |ref| {ref_max:.3e}")
        if not err <= max(PAR_TOL * ref_max, floor):
            bad.append((name, err, ref_max))
    return bad


@gpu
@pytest.mark.parametrize("n_hyper,rows", HNET)
def test_hnet_backward_with_damping(n_hyper, rows, golden):
    import hnet_cases as H
    o = make_hnet(n_hyper, rows, torch.device("cuda:0"))
    with _mode():
        got = run_hnet(n_hyper, o)
    _, grads = H.reference(o["h0"], o["v"], o["damping"], 2, n_hyper, o["flat"], o["g_y"])
    ref = grads[:3] + [grads[3 + l * 6 + 4] for l in range(n_hyper)]
    names = ["g_h0", "g_v", "g_damping"] + [f"head_w{l}" for l in range(n_hyper)]
    assert all(torch.isfinite(t).all() for t in got)
    assert not _within(names, got, ref, max(float(r.abs().max()) for r in grads))
    fp, want = fingerprint(got), golden[f"hnet/{n_hyper}-{rows}"]
    assert fp["samples"] == want["samples"]
    assert fp["sha256"] == want["sha256"]


# ---- attention backward ----
H_, HD, C_ = 3, 256, 128


def make_attn(N, dev):
    """N nodes with 12 incoming edges each and one more without any.  x, e and the first-layer weights are multiples of
    1/8 and 1/64, the first-layer biases odd multiples of 1/1024: every pre-activation is an exact, non-zero multiple of
    1/1024 below 2^24 of them, in fp32 (whole or split) and in fp64."""
    g = torch.Generator().manual_seed(500 + N)
    Nn, K, D = N + 1, 12, 3 * C_
    dst = torch.arange(N).repeat_interleave(K)
    src = torch.randint(0, Nn, (N * K,), generator=g)
    perm = torch.randperm(N * K, generator=g)
    ei = torch.stack([src[perm], dst[perm]])
    dy = lambda shape, den: torch.randint(-8, 9, shape, generator=g).float() / den
    odd = lambda n: (2 * torch.randint(-8, 8, (n,), generator=g) + 1).float() / 1024
    o = {"x": dy((Nn, C_), 8), "e": dy((N * K, C_), 8), "g_aggr": torch.randn(Nn, C_, generator=g)}
    ws = [dy((H_ * HD, D), 64), odd(H_ * HD), torch.randn(H_, HD, generator=g) * 0.05, torch.randn(H_, generator=g) * 0.1,
          dy((H_ * HD, D), 64), odd(H_ * HD), torch.randn(H_ * C_, HD, generator=g) * 0.05, torch.randn(H_ * C_, generator=g) * 0.1]
    o = {k: t.to(dev) for k, t in o.items()}
    o["ei"], o["ws"], o["Nn"] = ei.to(dev), [t.to(dev) for t in ws], Nn
    return o


def run_attn(o):
    """[grad A_out_b, grad A_out_w, grad (A_in_b | M_in_b)] of cgat_nodes_attention_backward."""
    from cgat_amd import _lib, ops
    plan = ops.EdgePlan(o["ei"], o["Nn"])
    aggr, saved, ws_ = ops._attn_forward(o["x"], o["e"], plan, H_, o["ws"], save=True)
    _, _, grads = ops._attn_backward(o["x"], o["e"], plan, H_, ws_, saved, o["g_aggr"], _lib.lib.cgat_get_edge_storage(),
                                     ops._stream())
    torch.cuda.synchronize()
    return [grads[3], grads[2], torch.cat([grads[1], grads[5]])]


def attn_reference(o):
    """The same gradients, and the largest gradient of all eight parameters, by fp64 autograd (oracle GATConvNodes.message:
    m = [x_i, e, x_j], softmax by destination exp(a - max) / (sum + 1e-16), mean over heads)."""
    dd = lambda t: t.detach().double().requires_grad_(True)
    x, e, ws = o["x"].double(), o["e"].double(), [dd(t) for t in o["ws"]]
    src, dst = o["ei"]
    E, Nn = e.shape[0], o["Nn"]
    lk = torch.nn.functional.leaky_relu
    m = torch.cat([x[dst], e, x[src]], 1)
    a = torch.einsum("ehk,hk->eh", lk(m @ ws[0].T + ws[1], 0.01).view(E, H_, HD), ws[2].view(H_, HD)) + ws[3]
    amax = torch.full((Nn, H_), -float("inf"), dtype=a.dtype, device=a.device).index_reduce_(0, dst, a.detach(), "amax")
    ex = torch.exp(a - amax[dst])
    alpha = ex / (torch.zeros(Nn, H_, dtype=a.dtype, device=a.device).index_add_(0, dst, ex)[dst] + 1e-16)
    msg = torch.einsum("ehk,hck->ehc", lk(m @ ws[4].T + ws[5], 0.01).view(E, H_, HD), ws[6].view(H_, C_, HD)) + ws[7].view(H_, C_)
    out = torch.zeros(Nn, H_, C_, dtype=a.dtype, device=a.device).index_add_(0, dst, msg * alpha[:, :, None]).mean(1)
    gr = torch.autograd.grad(out, ws, o["g_aggr"].double())
    return [gr[3], gr[2].reshape(-1), torch.cat([gr[1], gr[5]])], max(float(t.abs().max()) for t in gr)


@gpu
@pytest.mark.parametrize("N", ATTN)
def test_attention_backward(N, golden):
    o = make_attn(N, torch.device("cuda:0"))
    with _mode():
        got = run_attn(o)
    ref, scale = attn_reference(o)
    assert all(torch.isfinite(t).all() for t in got)
    assert not _within(["A_out_b", "A_out_w", "in_bias"], [t.reshape(-1) for t in got], ref, scale)
    fp, want = fingerprint(got), golden[f"attn/{N}"]
    assert fp["samples"] == want["samples"]
    assert fp["sha256"] == want["sha256"]


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))["cases"]


if __name__ == "__main__":      # python tests/test_row_helpers.py --record FILE --tree CHECKOUT   (on an MI355X)
    out_path = sys.argv[sys.argv.index("--record") + 1]
    tree = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
    sys.path.insert(0, tree)
    import subprocess
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else \
        subprocess.check_output(["git", "-C", tree, "rev-parse", "HEAD"], text=True).strip()
    import cgat_amd
    assert os.path.dirname(os.path.abspath(cgat_amd.__file__)) == os.path.join(tree, "cgat_amd"), cgat_amd.__file__
    dev = torch.device("cuda:0")
    cases = {}
    for c in COLSUM:
        cases["colsum/" + case_id(c)] = fingerprint([run_colsum_bias(make_colsum(c, dev)[1])])
    for c in LN:
        cases["ln/" + case_id(c)] = fingerprint([run_ln(c, make_ln(c, dev))[1]])
    with _mode():
        for n_hyper, rows in HNET:
            cases[f"hnet/{n_hyper}-{rows}"] = fingerprint(run_hnet(n_hyper, make_hnet(n_hyper, rows, dev)))
        for N in ATTN:
            cases[f"attn/{N}"] = fingerprint(run_attn(make_attn(N, dev)))
    doc = {"what": "row helper kernels: SHA-256 of the output bytes and %d sampled words (uint32, evenly spaced over the flat "
                   "output) per case of tests/test_row_helpers.py" % SAMPLES,
           "commit": commit,
           "command": "python tests/test_row_helpers.py --record FILE --tree CHECKOUT  (MI355X, the build of `commit`)",
           "cases": cases}
    json.dump(doc, open(out_path, "w"), indent=0, separators=(",", ":"))
    print(len(cases), "cases recorded with", tree)
