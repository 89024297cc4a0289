"""CPU-side checks of attention pooling with a dropout keep-mask: the library exports its two entry points, the binding
lists them, the shape predicate's truth table, the switch -- and, in fp64, the identity the kernels rest on.  No compute
call into the library is made here."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cgat_segment_attention_pool_dropout_forward", "cgat_segment_attention_pool_dropout_backward")


def test_library_exports_and_binding_lists_the_entry_points():
    from cgat_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.PROTOTYPES, name
    # keep, keep_idx in the place of mult; backward without g_mult
    plain_f = _lib.PROTOTYPES["cgat_segment_attention_pool_forward"][1]
    plain_b = _lib.PROTOTYPES["cgat_segment_attention_pool_backward"][1]
    assert len(_lib.PROTOTYPES[SYMBOLS[0]][1]) == len(plain_f) + 1
    assert len(_lib.PROTOTYPES[SYMBOLS[1]][1]) == len(plain_b)
    assert _lib.lib.cgat_abi_version() == 3                # no existing signature changed


# (aF, F) -> supported (on the GPU; never elsewhere)
TRUTH = [((384, 384), True), ((640, 640), True), ((3, 384), True), ((5, 640), True), ((3, 48), True), ((1, 16), True),
         ((1, 256), True),
         ((3, 36), False),                                 # F / aF = 12: no power of two times four
         ((1, 512), False),                                # more than 64 lanes per logit column
         ((6, 6), False), ((2, 2), False),                 # one logit per feature needs aF % 4 == 0
         ((5, 384), False),                                # F % aF != 0
         ((3, 6), False)]                                  # F % 4 != 0


@pytest.mark.parametrize("device", ["meta", "cpu"])
@pytest.mark.parametrize("shape,want", TRUTH, ids=lambda v: str(v))
def test_supported_truth_table(shape, want, device):
    """The mask does not enter the predicate: AttentionPoolFn.supported(a, m) decides for both paths.  On `meta` and
    `cpu` tensors it is False throughout (the layers only route GPU tensors to the kernels); the shape rule itself is
    read off with is_cuda patched in."""
    from cgat_amd import ops
    aF, F = shape
    a, m = torch.empty(5, aF, device=device), torch.empty(5, F, device=device)
    assert ops.AttentionPoolFn.supported(a, m) is False

    class OnGpu:
        is_cuda = True

        def __init__(self, t):
            self.shape, self.dtype = t.shape, t.dtype
    assert ops.AttentionPoolFn.supported(OnGpu(a), OnGpu(m)) is want
    assert ops.AttentionPoolFn.supported(OnGpu(a.double()), OnGpu(m.double())) is False


def test_no_cpu_fallback():
    from cgat_amd import ops
    R, S = 6, 2
    rowptr = torch.tensor([0, 3, 6], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.AttentionPoolFn.apply(torch.zeros(R, 3), None, torch.zeros(R, 48), rowptr, None, 1e-16, torch.ones(R, 3), None)
    import cgat_amd as P
    layer = P.GATConvNodes(16, 16, 16, 3, concat=True, dropout=0.3)           # CPU tensors keep the MessagePassing route,
    assert layer.route(torch.zeros(4, 16), torch.zeros(2, 8, dtype=torch.long), torch.zeros(8, 16)).kind == "message"


def test_switch_round_trip_and_reexport():
    import cgat_amd as P
    from cgat_amd import ops
    assert P.set_fused_attention_dropout is ops.set_fused_attention_dropout
    assert P.get_fused_attention_dropout is ops.get_fused_attention_dropout
    assert "set_fused_attention_dropout" in P.__all__ and "get_fused_attention_dropout" in P.__all__
    was = P.get_fused_attention_dropout()
    try:
        P.set_fused_attention_dropout(False)
        assert P.get_fused_attention_dropout() is False
        P.set_fused_attention_dropout(True)
        assert P.get_fused_attention_dropout() is True
    finally:
        P.set_fused_attention_dropout(was)


@pytest.mark.parametrize("value,want", [("0", False), (None, True)])
def test_environment_switch_in_a_child_process(value, want):
    env = {k: v for k, v in os.environ.items() if k != "CGAT_FUSED_ATTN_DROPOUT"}
    if value is not None:
        env["CGAT_FUSED_ATTN_DROPOUT"] = value
    out = subprocess.run([sys.executable, "-c", "import cgat_amd; print(cgat_amd.get_fused_attention_dropout())"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == str(want)


@pytest.mark.parametrize("aF,F", [(3, 48), (16, 16)])
def test_identity_the_kernels_rest_on(aF, F):
    """fp64, ragged 37 segments: softmax -> dropout -> multiply -> scatter-add (the reference's sequence) equals the
    plain pooling of the masked message keep * m -- forward, the gradient of the logits, and the gradient of the message
    once the pooling's own (alpha * g_out) is scaled by keep -- to 1e-12."""
    g = torch.Generator().manual_seed(aF)
    S, eps, fw = 37, 1e-16, F // aF
    counts = torch.randint(0, 30, (S,), generator=g)
    counts[5] = 0
    seg = torch.repeat_interleave(torch.arange(S), counts)[torch.randperm(int(counts.sum()), generator=g)]
    R = seg.numel()
    keep = (torch.rand(R, aF, generator=g, dtype=torch.float64) >= 0.3).double() / 0.7
    keep[seg == 11] = 0.0                                   # a segment whose rows are all dropped
    cot = torch.randn(S, F, generator=g, dtype=torch.float64)

    def softmax(a):
        mx = torch.full((S, aF), -float("inf"), dtype=torch.float64).scatter_reduce(0, seg.view(-1, 1).expand(R, aF),
                                                                                      a.detach(), "amax")
        ex = (a - mx[seg]).exp()
        return ex / (torch.zeros(S, aF, dtype=torch.float64).index_add(0, seg, ex) + eps)[seg]

    def pool(alpha, msg):
        return torch.zeros(S, F, dtype=torch.float64).index_add(0, seg, alpha.repeat_interleave(fw, dim=1) * msg)
    a0 = 3 * torch.randn(R, aF, generator=g, dtype=torch.float64)
    m0 = torch.randn(R, F, generator=g, dtype=torch.float64)
    # the reference's sequence
    a, m = a0.clone().requires_grad_(True), m0.clone().requires_grad_(True)
    out_ref = pool(softmax(a) * keep, m)
    ga_ref, gm_ref = torch.autograd.grad((out_ref * cot).sum(), [a, m])
    # pooling of the masked message; its message gradient is taken wrt m' = keep * m and scaled by keep afterwards
    a2 = a0.clone().requires_grad_(True)
    mk = (keep.repeat_interleave(fw, dim=1) * m0).requires_grad_(True)
    out = pool(softmax(a2), mk)
    ga, gmk = torch.autograd.grad((out * cot).sum(), [a2, mk])
    gm = keep.repeat_interleave(fw, dim=1) * gmk

    def rel(x, y):
        return float((x - y).abs().max() / y.abs().max())
    assert rel(out.detach(), out_ref.detach()) <= 1e-12
    assert rel(ga, ga_ref) <= 1e-12
    assert rel(gm, gm_ref) <= 1e-12
    # and g_a in the kernel's own form: sum over the column's features of alpha g_out (keep m - out)
    alpha = softmax(a0).repeat_interleave(fw, dim=1)
    ga_kernel = (alpha * cot[seg] * (keep.repeat_interleave(fw, dim=1) * m0 - out.detach()[seg])).reshape(R, aF, fw).sum(-1)
    assert rel(ga_kernel, ga_ref) <= 1e-12
