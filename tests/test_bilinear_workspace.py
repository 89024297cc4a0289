"""What the split of csrc/bilinear.hip into contractions (bilinear.hip), operand images (opimage.hip) and the weight
gradient (bilwgrad.hip) must not move: every workspace size.

The size queries of the three contraction entry points and of the hypernetwork layer are host arithmetic on the dims (the
hypernetwork's are dry passes over null operands): no device call, so this file needs no GPU.  The hypernetwork queries
are here because they reach bilinear_wgrad_batch_ws_bytes and bilinear_T_floats_max.
tests/golden/bilinear_workspace_bytes.json holds the values over a grid of row counts, operand widths and arithmetic
modes, recorded by `python tests/test_bilinear_workspace.py --record FILE` with the build of the commit BEFORE the split;
the comparison is exact (integers).

Zero rows are asked of the weight-gradient query alone: at that commit, as now, the other queries divide by the number of
row tiles (rows_asplit, bilinear.hip) and end the process on zero rows, so there is no value to record.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
GOLDEN = os.path.join(HERE, "golden", "bilinear_workspace_bytes.json")

ROWS = [1, 127, 128, 300, 1280, 2049, 8192, 8193, 16400, 83340]
DIMS = [(128, 128, 128), (1, 128, 128), (2, 128, 128), (37, 128, 128), (130, 128, 128), (64, 64, 64), (22, 22, 22),
        (256, 256, 256)]
HNETS = [(128, 2, 1), (128, 2, 2), (128, 2, 4), (64, 2, 4)]     # (width, dense layers per predicted layer, predicted layers)
MODES = ["f32", "bf16x6", "bf16x3", "f16x3", "f16x3c"]
WGRAD_ROWS = [0] + ROWS


def _hnet_sizes(rows, W, n_fc, n_hyper):
    from cgat_amd import _lib
    p = _lib.HnetParams()
    p.W, p.n_fc, p.n_hyper = W, n_fc, n_hyper
    lib = _lib.lib
    return [lib.cgat_hnet_forward_workspace_bytes(rows, C.byref(p)), lib.cgat_hnet_backward_workspace_bytes(rows, C.byref(p)),
            lib.cgat_hnet_backward_side_workspace_bytes(rows, C.byref(p)), lib.cgat_hnet_saved_floats(rows, C.byref(p))]


class _mode:
    """Arithmetic mode for the block, restored afterwards."""

    def __init__(self, mode):
        self.want = mode

    def __enter__(self):
        from cgat_amd import ops
        self.was = ops.get_bilinear_mode()
        ops.set_bilinear_mode(self.want)

    def __exit__(self, *exc):
        from cgat_amd import ops
        ops.set_bilinear_mode(self.was)


def measure():
    """{mode: {"rows": {"rows,NA,NB,NC": bytes}, "dual": {"rows": bytes}, "wgrad": {"rows,NA,NB,NC": bytes},
               "hnet": {"rows,W,n_fc,n_hyper": [forward, backward, backward side, saved floats]}}}"""
    from cgat_amd import _lib
    lib = _lib.lib
    doc = {}
    for mode in MODES:
        with _mode(mode):
            doc[mode] = {
                "rows": {",".join(map(str, (n,) + d)): lib.cgat_bilinear_rows_workspace_bytes(n, *d) for n in ROWS for d in DIMS},
                "dual": {str(n): lib.cgat_bilinear_dual_workspace_bytes(n) for n in ROWS},
                "wgrad": {",".join(map(str, (n,) + d)): lib.cgat_bilinear_wgrad_workspace_bytes(n, *d) for n in WGRAD_ROWS
                          for d in DIMS},
                "hnet": {",".join(map(str, (n,) + h)): _hnet_sizes(n, *h) for n in ROWS for h in HNETS},
            }
    return doc


def test_workspace_sizes_are_the_recorded_ones():
    want = json.load(open(GOLDEN))["sizes"]
    got = measure()
    assert sorted(got) == sorted(want) == sorted(MODES)
    for mode in want:
        assert sorted(got[mode]) == sorted(want[mode]), mode
        for op, sizes in want[mode].items():
            assert sorted(got[mode][op]) == sorted(sizes), (mode, op)
            for shape, size in sizes.items():
                assert got[mode][op][shape] == size, (mode, op, shape, got[mode][op][shape], size)
        assert len(want[mode]["rows"]) == len(ROWS) * len(DIMS) and len(want[mode]["wgrad"]) == len(WGRAD_ROWS) * len(DIMS)
        assert len(want[mode]["dual"]) == len(ROWS) and len(want[mode]["hnet"]) == len(ROWS) * len(HNETS)


def test_mode_is_restored():
    from cgat_amd import ops
    was = ops.get_bilinear_mode()
    measure()
    assert ops.get_bilinear_mode() == was


if __name__ == "__main__":      # python tests/test_bilinear_workspace.py --record FILE
    out_path = sys.argv[sys.argv.index("--record") + 1]
    doc = {"what": "bytes returned by cgat_bilinear_{rows,dual,wgrad}_workspace_bytes and by "
                   "cgat_hnet_{forward,backward,backward_side}_workspace_bytes, floats by cgat_hnet_saved_floats",
           "command": "python tests/test_bilinear_workspace.py --record FILE   (build of the commit before bilinear.hip "
                      "was split into bilinear.hip, opimage.hip and bilwgrad.hip; no GPU needed)",
           "sizes": measure()}
    json.dump(doc, open(out_path, "w"), indent=0, separators=(",", ":"))
    print(sum(len(t) for v in doc["sizes"].values() for t in v.values()), "sizes recorded")
