"""The f16x3c weight gradient  out[a,b,c] = sum_n p[n,a] q[n,b] r[n,c]  (csrc/wgradc.hip) at the shapes where the way it
fetches its operands can go wrong, now that the kernel reads p from the row-major tensor itself (dword LDS-DMA, lane = row)
and the product's power-of-two scale and the sign of the 512-row groups ride on the q image.

Two checks per case:
 * parity with the float64 sum over the kernel's own inputs, max-norm relative TOL of tests/test_hip_kernels.py;
 * the bits of the parent build: tests/golden/wgrad_operands_parent.json holds, per case, the SHA-256 of the output bytes and
   four sampled entries (as uint32), recorded with the build of the commit named in the file by
       python tests/test_wgrad_operands.py --record FILE --tree CHECKOUT
   The change moves exact multipliers and copies between kernels; the same scaled values reach the same instructions in the
   same order, so equality is exact.

Cases.  One layer through cgat_bilinear_wgrad (row splits + slab sum): rows in {1, 63, 64, 65, 511, 512, 513, 1025, 1537}
(chunk padding, row clamping, the sign flip of odd 512-row groups) x NA in {128, 127, 2, 1} (odd pair count, columns past NA)
x leading dimensions {tight, 132 with p four bytes off the 16-byte grid}; at 513 rows, NA = 127, padded: each operand all
zero, and each operand with magnitudes from 2^-30 to 2^10.  Every operand buffer is NaN outside [rows, columns] -- 64 rows
past the end included -- so a read that is not clamped shows.  Two and four predicted layers (one unit per (layer, a pair))
through the hypernetwork backward, serial and overlapped, head weight gradients against hnet_cases.reference.
"""
import hashlib
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "wgrad_operands_parent.json")
TOL = 2e-5                                                 # tests/test_hip_kernels.py
ROWS = [1, 63, 64, 65, 511, 512, 513, 1025, 1537]
NAS = [128, 127, 2, 1]
LDS = ["tight", "padded"]
KINDS = ["zero_p", "zero_q", "zero_r", "wide_p", "wide_q", "wide_r"]
ONE_LAYER = [(rows, NA, ld, "randn") for rows in ROWS for NA in NAS for ld in LDS] + [(513, 127, "padded", k) for k in KINDS]
HNET = [(2, 300), (4, 300), (4, 65), (4, 513), (4, 1537)]  # (predicted layers, rows); width 128, two trunk layers
SAMPLES = 4

pytestmark = pytest.mark.gpu


def case_id(c):
    return "-".join(map(str, c))


def _place(t, ld, off):
    """t's values at leading dimension ld, `off` floats into a NaN buffer that extends 64 rows past the end."""
    rows, cols = t.shape
    buf = torch.full(((rows + 64) * ld + 8,), float("nan"), dtype=torch.float32, device=t.device)
    view = buf[off:off + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(t)
    return buf, view


def make_one_layer(case, dev):
    rows, NA, ld, kind = case
    g = torch.Generator().manual_seed(7919 * rows + 31 * NA + len(ld) + 101 * (["randn"] + KINDS).index(kind))
    t = {"p": torch.randn(rows, NA, generator=g), "q": torch.randn(rows, 128, generator=g), "r": torch.randn(rows, 128, generator=g)}
    if kind.startswith("zero_"):
        t[kind[-1]].zero_()
    if kind.startswith("wide_"):
        x = t[kind[-1]]
        x.mul_(torch.exp2(torch.randint(-30, 11, x.shape, generator=g).float()))
    pad = ld == "padded"
    out = {}
    for k, cols in (("p", NA), ("q", 128), ("r", 128)):
        out[k] = _place(t[k].to(dev), 132 if pad else cols, 1 if (pad and k == "p") else 0)
    assert out["q"][1].data_ptr() % 16 == 0 and out["r"][1].data_ptr() % 16 == 0
    assert not pad or out["p"][1].data_ptr() % 16 == 4
    return out


def run_one_layer(case, o):
    from cgat_amd import _lib
    rows, NA, ld, kind = case
    (_, p), (_, q), (_, r) = o["p"], o["q"], o["r"]
    dev = p.device
    out = torch.full((NA, 128, 128), float("nan"), device=dev)
    ws = torch.full((max(_lib.lib.cgat_bilinear_wgrad_workspace_bytes(rows, NA, 128, 128), 256),), 0xFF, dtype=torch.uint8, device=dev)
    _lib.check(_lib.lib.cgat_bilinear_wgrad(p.data_ptr(), p.stride(0), q.data_ptr(), q.stride(0), r.data_ptr(), r.stride(0),
                                            out.data_ptr(), rows, NA, 128, 128, ws.data_ptr(), ws.numel(), None), "bilinear_wgrad")
    torch.cuda.synchronize()
    return out


def make_hnet(n_hyper, rows, dev):
    W, n_fc = 128, 2
    g = torch.Generator().manual_seed(4000 + 10 * rows + n_hyper)
    rn = lambda *s: torch.randn(*s, generator=g)
    o = {"h0": rn(rows, W), "v": rn(rows, W), "g_y": rn(rows, W)}
    flat = []
    for _ in range(n_hyper):
        flat += [rn(W, W) * (2.0 / W) ** 0.5 for _ in range(n_fc)]
        flat += [rn(W) * 0.1 for _ in range(n_fc)]
        flat += [rn(W * W + W, W) * 0.1 * (2.0 / W) ** 0.5, rn(W * W + W) * 0.05]
    o = {k: t.to(dev) for k, t in o.items()}
    o["flat"] = [t.to(dev) for t in flat]
    return o


def run_hnet(n_hyper, o, overlapped):
    """The head weight gradients [W W + W, W] of every predicted layer (rows < W W: the weight-gradient contraction)."""
    from cgat_amd import ops
    dev = o["v"].device
    y, saved, d, flat = ops._hnet_forward(o["h0"], o["v"], None, 2, n_hyper, o["flat"])
    main = torch.cuda.current_stream(dev)
    side = (main, ops.side_stream(dev)) if overlapped else None
    g_h0, g_v, g_d, grads, side_ws = ops._hnet_backward(o["h0"], o["v"], saved, d, flat, 2, n_hyper, o["g_y"], side=side)
    if overlapped:
        main.wait_stream(side[1])
    torch.cuda.synchronize(dev)
    del side_ws
    return [grads[l * 6 + 4] for l in range(n_hyper)]


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


def _mode():
    from cgat_amd import ops

    class M:
        def __enter__(self):
            self.was = ops.get_bilinear_mode()
            ops.set_bilinear_mode("f16x3c")

        def __exit__(self, *exc):
            ops.set_bilinear_mode(self.was)
    return M()


def rel(a, b):
    a, b = a.double(), b.double()
    d = b.abs().max().item()
    return (a - b).abs().max().item() / (d if d > 0 else 1.0)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))["cases"]


@pytest.mark.parametrize("case", ONE_LAYER, ids=case_id)
def test_one_layer(case, golden):
    dev = torch.device("cuda:0")
    o = make_one_layer(case, dev)
    with _mode():
        out = run_one_layer(case, o)
    ref = torch.einsum("na,nb,nc->abc", o["p"][1].double(), o["q"][1].double(), o["r"][1].double())
    err = rel(out, ref)
    print(f"  {case_id(case)} err/|ref| {err:.2e}")
    assert torch.isfinite(out).all()
    assert err <= TOL
    got, want = fingerprint([out]), golden["one/" + case_id(case)]
    assert got["samples"] == want["samples"]
    assert got["sha256"] == want["sha256"]


_hnet_ref = {}


def _hnet_reference(n_hyper, rows):
    """(operands, fp64 head weight gradients): computed once, shared, never written to."""
    import hnet_cases as H
    if (n_hyper, rows) not in _hnet_ref:
        o = make_hnet(n_hyper, rows, torch.device("cuda:0"))
        _, grads = H.reference(o["h0"], o["v"], None, 2, n_hyper, o["flat"], o["g_y"])
        _hnet_ref[(n_hyper, rows)] = (o, [grads[2 + l * 6 + 4] for l in range(n_hyper)])
    return _hnet_ref[(n_hyper, rows)]


@pytest.mark.parametrize("n_hyper,rows", HNET)
def test_predicted_layers(n_hyper, rows, golden):
    from cgat_amd import ops
    o, ref = _hnet_reference(n_hyper, rows)
    with _mode():
        serial = run_hnet(n_hyper, o, False)
        over = run_hnet(n_hyper, o, True)
        keeps_bits = ops._overlapped_hnet_keeps_bits(o["v"])
    for l, (a, b, r) in enumerate(zip(serial, over, ref)):
        ea, eb = rel(a, r), rel(b, r)
        print(f"  layer {l}: err/|ref| serial {ea:.2e} overlapped {eb:.2e}")
        assert ea <= TOL and eb <= TOL
        if keeps_bits:
            assert torch.equal(a, b), f"layer {l}: the overlapped backward gives other bits than the serial one"
    got, want = fingerprint(serial), golden[f"hnet/{n_hyper}-{rows}"]
    assert got["samples"] == want["samples"]
    assert got["sha256"] == want["sha256"]


if __name__ == "__main__":      # python tests/test_wgrad_operands.py --record FILE --tree CHECKOUT   (on an MI355X)
    out_path = sys.argv[sys.argv.index("--record") + 1]
    tree = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
    sys.path.insert(0, tree)
    import subprocess
    commit = sys.argv[sys.argv.index("--commit") + 1] if "--commit" in sys.argv else \
        subprocess.check_output(["git", "-C", tree, "rev-parse", "HEAD"], text=True).strip()
    dev = torch.device("cuda:0")
    cases = {}
    with _mode():
        for c in ONE_LAYER:
            cases["one/" + case_id(c)] = fingerprint([run_one_layer(c, make_one_layer(c, dev))])
        for n_hyper, rows in HNET:
            cases[f"hnet/{n_hyper}-{rows}"] = fingerprint(run_hnet(n_hyper, make_hnet(n_hyper, rows, dev), False))
    doc = {"what": "f16x3c weight gradient: SHA-256 of the output bytes and %d sampled entries (uint32, evenly spaced over "
                   "the flat output) per case of tests/test_wgrad_operands.py" % SAMPLES,
           "commit": commit,
           "command": "python tests/test_wgrad_operands.py --record FILE --tree CHECKOUT  (MI355X, the build of `commit`)",
           "cases": cases}
    json.dump(doc, open(out_path, "w"), indent=0, separators=(",", ":"))
    print(len(cases), "cases recorded with", tree)
