"""The hypernetwork orchestrators (csrc/hnet.hip) on every route of tests/test_hnet_routes_cpu.py's table that a small
shape reaches: parity with an fp64 restatement, identical bits on a repeated call, the overlapped backward against the
serial one, and the launches each route makes.

Reference: tests/hnet_cases.py restates the layer in fp64 torch on the device; test_reference_is_the_oracle holds that
restatement to the oracle's H_Net.  Criterion, here as there, is test_hip_golden.py's (_compare_with_oracle):
    ||got - ref||_inf <= max(TOL * ||ref64||_inf, ZERO_FLOOR * largest gradient of the case where the floor is open)
per tensor, flat.

Launches: tests/golden/hnet_launches.json holds, per mode / case / serial or overlapped, the launch count of every
launch-timer tag a hypernetwork pass can reach and of all kernels, recorded on an MI355X with the build of the commit
before the orchestrators moved to csrc/hnet.hip (forward + backward of hnet_cases.run_library)."""
import copy
import json
import os

import pytest
import torch

import hnet_cases as H
from golden_util import floor_open
from test_hip_golden import TOL, ZERO_FLOOR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAUNCHES = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hnet_launches.json")))["launches"]

_ref = {}


def _reference(name):
    """(operands, y, gradients) of a case: computed once, shared by the modes, never written to."""
    if name not in _ref:
        W, n_fc, n_hyper, rows, damping, off = H.CASES[name]
        o = H.make_operands(name, torch.device(DEV))
        y, grads = H.reference(o["h0"], o["v"], o["damping"], n_fc, n_hyper, o["flat"], o["g_y"])
        _ref[name] = (o, y, grads)
    return _ref[name]


def _failures(names, got, ref):
    """The tensors of `got` outside the criterion against the fp64 `ref` (item 0: the output), with every figure."""
    case_scale = max(float(r.abs().max()) for r in ref[1:])
    bad = []
    for name, a, r in zip(names, got, ref):
        ref_max = float(r.abs().max())
        err = float((a.detach().double() - r).abs().max())
        floor = ZERO_FLOOR * case_scale if name != "out" and floor_open(ref_max, case_scale) else 0.0
        print(f"  {name:22s} err/|ref| {err / max(ref_max, 1e-300):.2e}")
        if err > max(TOL * ref_max, floor):
            bad.append(f"{name}: err {err:.3e} allowed {max(TOL * ref_max, floor):.3e} |ref| {ref_max:.3e}")
    return bad


def test_reference_is_the_oracle():
    """hnet_cases.reference against the oracle's H_Net (damping included) at the shape of case `small_rows`: oracle fp32
    and fp64 runs as in _compare_with_oracle, the restatement in the place of the HIP run."""
    import cgat_amd as P
    from oracle import cgat_oracle as O
    W, n_fc, n_hyper, rows, _, _ = H.CASES["small_rows"]
    torch.manual_seed(1)
    om = O.H_Net(W, n_fc - 1, W, W, n_hyper - 2, W, W)
    pm = P.H_Net(W, n_fc - 1, W, W, n_hyper - 2, W, W)
    pm.load_state_dict(om.state_dict())
    flat = []
    for layer in pm.Hyper.layers:
        flat += (layer.hyper_linear if hasattr(layer, "hyper_linear") else layer).flat_params()
    pname = {id(p): n for n, p in pm.named_parameters()}
    order = ["damping"] + [pname[id(t)] for t in flat]
    g = torch.Generator().manual_seed(31)
    h0, v, g_y = (torch.randn(rows, W, generator=g) for _ in range(3))

    def run(m, dt):
        a, b = h0.to(dt).requires_grad_(True), v.to(dt).requires_grad_(True)
        params = dict(m.named_parameters())
        y = m(a, None, b)
        gr = torch.autograd.grad(y, [a, b] + [params[n] for n in order], g_y.to(dt))
        return [y.detach()] + [t.detach() for t in gr]
    o32, o64 = run(om, torch.float32), run(copy.deepcopy(om).double(), torch.float64)
    dev = torch.device(DEV)
    y, grads = H.reference(h0.to(dev), v.to(dev), pm.damping.detach().to(dev), n_fc, n_hyper, [t.detach().to(dev) for t in flat],
                           g_y.to(dev))
    case_scale = max(float(t.abs().max()) for t in o64[1:])
    for name, a, b32, b64 in zip(["out", "g_h0", "g_v"] + order, [y] + grads, o32, o64):
        ref_max = float(b64.abs().max())
        err = float((a.cpu() - b32.double()).abs().max())
        floor = ZERO_FLOOR * case_scale if name != "out" and floor_open(ref_max, case_scale) else 0.0
        assert err <= max(TOL * ref_max, floor), (name, err, ref_max)


@pytest.mark.parametrize("name", list(H.CASES))
@pytest.mark.parametrize("mode", H.MODES)
def test_case(mode, name):
    from cgat_amd import ops
    o, y_ref, g_ref = _reference(name)
    names = ["out"] + H.grad_names(name)
    was = ops.get_bilinear_mode()
    ops.set_bilinear_mode(mode)
    try:
        y, grads, launches = H.run_library(name, o)
        y2, grads2, launches2 = H.run_library(name, o)
        yo, gradso, launches_o = H.run_library(name, o, overlapped=True)
        keeps_bits = ops._overlapped_hnet_keeps_bits(o["v"])
    finally:
        ops.set_bilinear_mode(was)
    assert len(names) == 1 + len(grads) == 1 + len(g_ref)
    bad = _failures(names, [y] + grads, [y_ref] + g_ref)
    assert not bad, "\n".join(bad)
    bad = _failures(names, [yo] + gradso, [y_ref] + g_ref)
    assert not bad, "overlapped:\n" + "\n".join(bad)
    for n, a, b in zip(names, [y] + grads, [y2] + grads2):
        assert torch.equal(a, b), f"{n}: a repeated call gives other bits"
    if keeps_bits:
        for n, a, b in zip(names, [y] + grads, [yo] + gradso):
            assert torch.equal(a, b), f"{n}: the overlapped backward gives other bits than the serial one"
    print("  launches", launches, launches_o)
    assert launches == launches2 == LAUNCHES[f"{mode}/{name}/serial"]
    assert launches_o == LAUNCHES[f"{mode}/{name}/overlapped"]
