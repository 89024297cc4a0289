"""Child process of tests/test_indexed_edge_attr.py (a crash inside the HIP graph runtime must fail ONE test, not take the
pytest process down): with cgat_amd.set_indexed_edge_attr(True) an eval forward of CGAtNet under no_grad -- the node layers
on cgat_nodes_attention_infer_indexed, the edge update on the table's rows -- captured with torch.cuda.graph replays to the
bits of the eager forward, also after its static input was overwritten."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import cgat_amd as P
    from cgat_amd import ops
    dev = "cuda:0"
    P.set_indexed_edge_attr(True)
    b, roost = P.synthetic_batch(150, 20, 12, seed=8)
    b = b.to(dev)
    roost = tuple(t.to(dev) for t in roost)
    torch.manual_seed(1)
    net = P.CGAtNet(200, 128, 4, msg_heads=3, neighbor_number=12, update_edges=True).to(dev).eval()
    x0 = b.x.clone()
    x_other = b.x[torch.randperm(b.x.shape[0], generator=torch.Generator().manual_seed(3)).to(dev)].clone()
    x_static = b.x.clone()
    b.x = x_static

    with torch.no_grad():
        ops.prof_reset()
        ops.prof_enable(True)
        want = net(b, roost).clone()
        torch.cuda.synchronize()
        ops.prof_enable(False)
        assert ops.prof_get("edge_idx_wsum")[0] == 4 and ops.prof_get("edge_msg_wsum")[0] == 0
        x_static.copy_(x_other)
        want2 = net(b, roost).clone()
        x_static.copy_(x0)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            net(b, roost)                       # warm-up on the capture stream (plans, workspaces, index validation)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = net(b, roost)
        for xv, w in ((x0, want), (x_other, want2), (x0, want)):
            x_static.copy_(xv)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, w), float((out - w).abs().max())
    print("INDEXED_CAPTURE_OK")


if __name__ == "__main__":
    main()
