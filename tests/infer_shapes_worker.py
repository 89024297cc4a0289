"""Child process of tests/test_fused_inference_shapes.py (a crash inside the HIP graph runtime must fail ONE test, not
take the pytest process down; CGAT_Z_COL_GROUPS is read once per process).
  capture: the harness' scalar-attention network (msg_heads = 5, 24 neighbours) on 64 crystals, eval() under no_grad,
           captured with torch.cuda.graph, replays to the eager bits, also after its static input was overwritten.
  layer OUT: the H = 5 no_grad layer outputs on the few-row graphs of the test, checked against the training forward,
           saved to OUT for the parent to compare (run with CGAT_Z_COL_GROUPS=0)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def capture():
    import cgat_amd as P
    from test_fused_inference_shapes import _harness_net
    dev = "cuda:0"
    b, roost = P.synthetic_batch(64, 20, 24, seed=8)
    b = b.to(dev)
    roost = tuple(t.to(dev) for t in roost)
    net = _harness_net()
    x0 = b.x.clone()
    x_other = b.x[torch.randperm(b.x.shape[0], generator=torch.Generator().manual_seed(3)).to(dev)].clone()
    x_static = b.x.clone()
    b.x = x_static
    with torch.no_grad():
        want = net(b, roost).clone()
        x_static.copy_(x_other)
        want2 = net(b, roost).clone()
        x_static.copy_(x0)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net(b, roost)                       # warm-up on the capture stream (plans, workspaces)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = net(b, roost)
        for xv, w in ((x0, want), (x_other, want2), (x0, want)):
            x_static.copy_(xv)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, w), float((out - w).abs().max())
    print("INFER_SHAPES_CAPTURE_OK")


def layer(path):
    from test_fused_inference_shapes import _graph, _inputs, _layer, _tags
    res = {}
    for kind in ("ragged_few", "c64k24"):
        N, ei = _graph(kind)
        x, ei, e, x0 = _inputs(N, ei)
        lay = _layer(False)
        want = lay(x.clone().requires_grad_(True), ei, e.clone().requires_grad_(True), x0).detach()
        with torch.no_grad():
            got, t = _tags(lambda: lay(x, ei, e, x0))
        assert t["edge_msg_wsum"] > 0 and t["edge_z"] == 0, t
        assert torch.equal(got, want), (kind, float((got - want).abs().max()))
        res[kind] = got.cpu()
    torch.save(res, path)
    print("INFER_SHAPES_LAYER_OK")


if __name__ == "__main__":
    if sys.argv[1] == "capture":
        capture()
    else:
        layer(sys.argv[2])
