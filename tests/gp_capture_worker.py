"""Child process of tests/test_gp_head.py (a crash inside the HIP graph runtime must fail ONE test, not take the pytest
process down): GPHead.predict -- one cgat_gp_predict launch, no workspace, no host synchronisation -- captured with
torch.cuda.graph replays to the bits of the eager call, also after its static input was overwritten."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import cgat_amd as P
    import gp_cases
    dev = "cuda:0"
    p, X, _ = gp_cases.case("g257_m37_d5")
    head = P.GPHead.from_tensors(p).to(dev)
    x0 = X.to(dev)
    x_other = x0.flip(0).contiguous() * 0.5
    x_static = x0.clone()
    want = [t.clone() for t in head.predict(x_static)]       # also builds the factor image, outside the capture
    want2 = [t.clone() for t in head.predict(x_other)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        head.predict(x_static)                               # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = head.predict(x_static)
    for xv, w in ((x0, want), (x_other, want2), (x0, want)):
        x_static.copy_(xv)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(o, v) for o, v in zip(out, w))
    print("GP_CAPTURE_OK")


if __name__ == "__main__":
    main()
