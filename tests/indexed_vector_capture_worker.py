"""Child process of tests/test_indexed_vector_layer.py (a crash inside the HIP graph runtime must fail ONE test, not take
the pytest process down): with cgat_amd.set_indexed_vector_attention(True), one forward + backward of a vector-attention
node layer on an IndexedEdgeAttr -- cgat_edge_hidden_forward_indexed / _backward_indexed -- is run eagerly (which builds the
class plan), then captured with torch.cuda.graph after two warm-up steps on the capture stream; the captured step replays
twice, after its static inputs were overwritten, to the eager step's output and gradients bit for bit."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import cgat_amd as P
    from cgat_amd import ops
    dev = "cuda:0"
    P.set_indexed_vector_attention(True)
    b, _ = P.synthetic_batch(150, 20, 12, seed=5)
    N, ei = b.num_nodes, b.edge_index.to(dev)
    E = ei.shape[1]
    g = torch.Generator().manual_seed(6)
    x0, x1 = torch.randn(N, 128, generator=g).to(dev), torch.randn(N, 128, generator=g).to(dev)
    t0, t1 = torch.randn(13, 128, generator=g).to(dev), torch.randn(13, 128, generator=g).to(dev)
    cot = torch.randn(N, 128, generator=g).to(dev)
    index = (torch.arange(0, 12, 2)[torch.randint(0, 6, (E,), generator=g)]).to(dev)
    torch.manual_seed(1)
    layer = P.GATConvNodes(128, 128, 128, 3, concat=True, final=True, vector_attention=True).to(dev)
    params = list(layer.parameters())
    x_s, t_s = x0.clone().requires_grad_(True), t0.clone().requires_grad_(True)

    def step():
        y = layer(x_s, ei, P.IndexedEdgeAttr(t_s, index), None)
        return (y, *torch.autograd.grad((y * cot).sum(), [x_s, t_s] + params))

    def eager(xv, tv):
        with torch.no_grad():
            x_s.copy_(xv)
            t_s.copy_(tv)
        return [v.detach().clone() for v in step()]

    ops.prof_reset()
    ops.prof_enable(True)
    want0 = eager(x0, t0)                       # the eager step: builds the class plan
    torch.cuda.synchronize()
    ops.prof_enable(False)
    assert ops.prof_get("edge_idx_hidden")[0] == 1 and ops.prof_get("edge_idx_class_sum")[0] == 1
    assert ops.prof_get("edge_z")[0] == 0 and ops.prof_get("edge_ge")[0] == 0 and ops.prof_get("edge_gw")[0] == 0
    want1 = eager(x1, t1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                  # two eager warm-up steps on the capture stream (plans, workspaces)
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    for (xv, tv), want in (((x1, t1), want1), ((x0, t0), want0)):
        with torch.no_grad():
            x_s.copy_(xv)
            t_s.copy_(tv)
        graph.replay()
        torch.cuda.synchronize()
        for a, w in zip(out, want):
            assert torch.equal(a, w), float((a - w).abs().max())
    print("INDEXED_VECTOR_CAPTURE_OK")


if __name__ == "__main__":
    main()
