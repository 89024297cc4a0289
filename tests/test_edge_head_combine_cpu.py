"""CPU-side checks of the edge update's head-combination op: the library exports its two entry points, the binding
lists them, the shape predicate's truth table, and the environment switch.  No compute call is made here."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cgat_edge_head_combine_forward", "cgat_edge_head_combine_backward")


def test_library_exports_and_binding_lists_the_entry_points():
    from cgat_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    assert _lib.lib.cgat_abi_version() == 3                # no existing signature changed


# (H, aF, Co) -> supported
TRUTH = [((3, 1, 128), True), ((5, 128, 128), True), ((1, 1, 40), True), ((8, 1, 64), True), ((3, 16, 16), True),
         ((2, 1, 256), True), ((1, 1, 4), True),
         ((3, 1, 30), False),                              # Co % 4 != 0
         ((9, 1, 128), False), ((9, 128, 128), False),     # more than 8 heads
         ((3, 1, 260), False),                             # Co > 256
         ((3, 2, 128), False), ((3, 64, 128), False)]      # neither one logit per head nor one per channel


@pytest.mark.parametrize("device", ["meta", "cpu"])
@pytest.mark.parametrize("shape,want", TRUTH, ids=lambda v: str(v))
def test_supported_truth_table(shape, want, device):
    from cgat_amd import ops
    H, aF, Co = shape
    sa, sm = torch.empty(5, H, aF, device=device), torch.empty(5, H, Co, device=device)
    assert ops.EdgeHeadCombineFn.supported(sa, sm) is want
    # never on anything but fp32, never for mismatched row / head counts
    assert not ops.EdgeHeadCombineFn.supported(sa.double(), sm.double())
    assert not ops.EdgeHeadCombineFn.supported(sa, torch.empty(5, H + 1, Co, device=device))
    assert not ops.EdgeHeadCombineFn.supported(sa, torch.empty(6, H, Co, device=device))
    # the layers only route GPU tensors to the kernels
    assert not ops.edge_combine_route(sa, sm)


def test_no_cpu_fallback():
    from cgat_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.EdgeHeadCombineFn.apply(torch.zeros(4, 3, 1), torch.zeros(4, 3, 128), None, None)


def test_switch_round_trip_and_reexport():
    import cgat_amd as P
    from cgat_amd import ops
    assert P.set_fused_edge_combine is ops.set_fused_edge_combine
    assert P.get_fused_edge_combine is ops.get_fused_edge_combine
    was = P.get_fused_edge_combine()
    try:
        P.set_fused_edge_combine(False)
        assert P.get_fused_edge_combine() is False
        P.set_fused_edge_combine(True)
        assert P.get_fused_edge_combine() is True
    finally:
        P.set_fused_edge_combine(was)


@pytest.mark.parametrize("value,want", [("0", False), (None, True)])
def test_environment_switch_in_a_child_process(value, want):
    env = {k: v for k, v in os.environ.items() if k != "CGAT_FUSED_EDGE_COMBINE"}
    if value is not None:
        env["CGAT_FUSED_EDGE_COMBINE"] = value
    out = subprocess.run([sys.executable, "-c", "import cgat_amd; print(cgat_amd.get_fused_edge_combine())"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == str(want)
