"""Which kernel a launch of the per-edge family (csrc/edgez.hip) runs.  The forms of one launch are bit-identical by design,
so a launch that quietly changed form would pass every parity test; cgat_debug_edge_z_form names the form, and the table
below pins it.  Host arithmetic only: no GPU.

The table was written from the conditions of the launchers as they stood before the form became a named value (commit
923502f; csrc/edgez.hip and csrc/kernels.h of that commit, cited per condition), not from the query's output:
  z_col_groups(tiles, ncb, unit)   1 at tiles >= 512; else the divisors g of ncb with (ncb / g) % unit == 0 in ascending
                                   order, stopping at the first with tiles * g >= 512 (the largest if none) (kernels.h:209-215)
  256-row kernel (edge_z6w)        a 24-bit mode; not [fp32 store, ceil(E / 256) < 128 and z_col_groups(ceil(E / 128), ncb,
                                   unit) > 1]; H * Hd of the logits <= 2048; n_add_rows > 0; n_add_rows * 4 * ld_add < 2^32
                                   (edgez.hip:1095-1099) -- and gathered addends, a permutation, act none / LeakyReLU, not
                                   omax together with logits (:1131-1132)
  128-row kernel otherwise         passes 2 in f16x3, 3 in bf16x3, else 6 (:1164-1170); column groups z_col_groups(ceil(E /
                                   128), ncb, unit) in a 24-bit mode under fp32 store, else 1 (:1155-1156); unit = Hd / 128
                                   with logits, else 1 (:1127, :1156)
  bf16 store                       refused without addends, a 24-bit mode, act none, no omax (:1117-1118)
  bit form                         refused unless the 256-row kernel runs it, with logits, and 2 n_add_rows + ceil(E / 32)
                                   <= E (:1128-1130)
  logits launch                    256-row kernel, mode 1; groups z_col_groups(ceil(E / 256), H Hd / 128, Hd / 128) below
                                   128 tiles of 256, else 1 (:1196, :1205-1209)
  message / weighted-sum launch    R = 128 at mean in-degree >= 128, else 256 - 16 ceil(deg / 16); groups
                                   z_col_groups(ceil(E / R), H Hd / 128) below 128 tiles of 256, else 1, then raised until
                                   they divide the blocks and (1024 / min(H Hd / 4, 256)) * blocks per group * 128 <= 4096
                                   (:1224-1230)
  dense layer at width 128         the 128-row kernel without addends; groups z_col_groups(ceil(rows / 128), n_out / 128) in a
                                   24-bit mode (:1265-1268)
The first layer of the vector-attention variants calls the per-edge launch WITHOUT n_add_rows (layers.hip:1017 of that
commit stops at omax), so it never runs the 256-row kernel; the rows marked `hidden` pin that as it is."""
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from test_attn_workspace import _modes   # noqa: E402

BIT24 = ("f16x3c", "bf16x6")
LEAKY = 2


def R128(passes, groups, per_group, tiles, adds=1, zb=0):
    return dict(kernel="rows128", passes=passes, adds=adds, z_bf16=zb, wide_mode=0, groups=groups, blocks_per_group=per_group,
                grid_x=tiles, tile_rows=128)


def R256(mode, groups, per_group, tiles, zb=0, passes=6, adds=1):
    return dict(kernel="rows256", passes=passes, adds=adds, z_bf16=zb, wide_mode=mode, groups=groups,
                blocks_per_group=per_group, grid_x=tiles, tile_rows=256)


def WSUM(R, groups, per_group, tiles, zb=0):
    return dict(kernel="msg_wsum", passes=6, adds=1, z_bf16=zb, wide_mode=0, groups=groups, blocks_per_group=per_group,
                grid_x=tiles, tile_rows=R)


def cdiv(a, b):
    return -(-a // b)


# the per-edge launch of a scalar-attention layer, H 3, Hd 256: W2 = 1536 = 12 column blocks, a head = 2 blocks
def edge(E, N=None, H=3, Hd=256, **kw):
    W2 = 2 * H * Hd
    return dict(rows=E, W2=W2, H=H, Hd=Hd, n_add_rows=E // 12 if N is None else N, ld_add=W2, adds=True, logits=True, **kw)


def proj(N, W2=1536):      # node_projections: no addends, no logits, ld_add 0
    return dict(rows=N, W2=W2, H=3, Hd=W2 // 6, n_add_rows=0, ld_add=0)


def hidden(E, W2=1536, n_add_rows=0):     # edge_hidden_forward_impl: LeakyReLU, omax, one "head" of W2 / 2 columns
    return dict(rows=E, W2=W2, H=1, Hd=W2 // 2, n_add_rows=n_add_rows, ld_add=W2, adds=True, omax=True, act=LEAKY)


def dense(rows, n_out):
    return dict(rows=rows, W2=n_out, ld_add=0)


NMAX = 699050       # the largest n with n * 4 * 1536 < 2^32
# (what, modes, arguments of debug.edge_z_form, form or None = refused)
TABLE = [
    # 32 513 edges: the first count with 128 row tiles of 256 -> the 256-row kernel; one fewer: 254 tiles of 128, groups 2
    # (508 < 512) then 3; edgez_worker's 14 640: 115 tiles, groups 2, 3, (4: 3 blocks split a head) 6
    ("edge 32513", BIT24, edge(32513), R256(0, 1, 12, 128)),
    ("edge 32512", BIT24, edge(32512), R128(6, 3, 4, 254)),
    ("edge 14640", BIT24, edge(14640), R128(6, 6, 2, 115)),
    # f16x3: two planes, never groups; bf16x3: three passes; neither has the 256-row kernel
    ("edge 32513", ("f16x3",), edge(32513), R128(2, 1, 12, 255)),
    ("edge 14640", ("f16x3",), edge(14640), R128(2, 1, 12, 115)),
    ("edge 32513", ("bf16x3",), edge(32513), R128(3, 1, 12, 255)),
    ("edge 14640", ("bf16x3",), edge(14640), R128(3, 1, 12, 115)),
    ("edge 14640", ("f32",), edge(14640), R128(6, 1, 12, 115)),       # (no caller launches it in f32: edge_z_dims)
    # bf16 store: the 256-row kernel at any E; refused outside the 24-bit modes
    ("bf16 14640", BIT24, edge(14640, store="bf16"), R256(0, 1, 12, 58, zb=1)),
    ("bf16 32513", BIT24, edge(32513, store="bf16"), R256(0, 1, 12, 128, zb=1)),
    ("bf16 240", BIT24, edge(240, store="bf16"), R256(0, 1, 12, 1, zb=1)),
    ("bf16 14640", ("f16x3", "bf16x3", "f32"), edge(14640, store="bf16"), None),
    # the bit form at its own limit: E 32 640, 2 N + 1 020 <= 32 640 <=> N <= 15 810; and never on the few-row form
    ("bits N 15810", BIT24, edge(32640, N=15810, store="bits"), R256(3, 1, 12, 128)),
    ("bits N 15811", BIT24, edge(32640, N=15811, store="bits"), None),
    ("bits 32512", BIT24, edge(32512, store="bits"), None),
    ("bits 32640", ("f16x3", "bf16x3"), edge(32640, store="bits"), None),
    # the projections: 24 tiles at 3 000 rows, groups 2, 3, 4, 6, 12 (288 < 512: the largest); 512 tiles at 65 536
    ("proj 3000", BIT24, proj(3000), R128(6, 12, 1, 24, adds=0)),
    ("proj 65536", BIT24, proj(65536), R128(6, 1, 12, 512, adds=0)),
    ("proj 65408", BIT24, proj(65408), R128(6, 2, 6, 511, adds=0)),
    ("proj 3000", ("f16x3",), proj(3000), R128(2, 1, 12, 24, adds=0)),
    ("proj 3000", ("bf16x3",), proj(3000), R128(3, 1, 12, 24, adds=0)),
    # hidden: n_add_rows 0 -> the 128-row kernel whatever E; with the rows given it WOULD be the 256-row kernel
    ("hidden 14640", BIT24, hidden(14640), R128(6, 6, 2, 115)),
    ("hidden 32640", BIT24, hidden(32640), R128(6, 3, 4, 255)),
    ("hidden 65536", BIT24, hidden(65536), R128(6, 1, 12, 512)),
    ("hidden 1000080", BIT24, hidden(1000080), R128(6, 1, 12, 7814)),
    ("hidden 65536 given rows", BIT24, hidden(65536, n_add_rows=5461), R256(0, 1, 12, 256)),
    ("hidden 14640", ("f16x3",), hidden(14640), R128(2, 1, 12, 115)),
    # omax together with logits: the running maximum shares a register with the logits -> 128-row kernel, 255 tiles, groups 3
    ("omax+logits", BIT24, edge(32640, omax=True), R128(6, 3, 4, 255)),
    ("tanh", BIT24, edge(32640, act=1), R128(6, 3, 4, 255)),
    # fc_out_A's weight in the 256-row kernel's LDS: H Hd 2 048 fits, 2 304 (36 blocks, groups 2, 3) does not
    ("hhd 2048", BIT24, edge(32640, H=8), R256(0, 1, 32, 128)),
    ("hhd 2304", BIT24, edge(32640, H=9), R128(6, 3, 12, 255)),
    # 32-bit gather offsets
    ("gather bound", BIT24, edge(12 * NMAX, N=NMAX), R256(0, 1, 12, cdiv(12 * NMAX, 256))),
    ("gather bound + 1", BIT24, edge(12 * NMAX, N=NMAX + 1), R128(6, 1, 12, cdiv(12 * NMAX, 128))),
    ("no rows", BIT24, edge(0), dict(kernel="none", passes=0, adds=0, z_bf16=0, wide_mode=0, groups=0, blocks_per_group=0,
                                     grid_x=0, tile_rows=0)),
    # the forward without grad on both sides of 128 row tiles of 256 (32 508 = 2 709 x 12: 127 tiles; 32 520: 128).
    # logits: 6 attention blocks in whole heads, groups (2: 3 blocks split a head) 3.  message: R 240 at in-degree 12, 136
    # tiles, groups 2, 3, 6 (816 >= 512); carry 5 x blocks x 128 <= 4 096
    ("logits few", BIT24, dict(edge(32508), launch="edge_logits"), R256(1, 3, 2, 127)),
    ("logits", BIT24, dict(edge(32520), launch="edge_logits"), R256(1, 1, 6, 128)),
    ("wsum few", BIT24, dict(edge(32508), launch="edge_msg_wsum"), WSUM(240, 6, 1, 136)),
    ("wsum", BIT24, dict(edge(32520), launch="edge_msg_wsum"), WSUM(240, 1, 6, 136)),
    ("wsum bf16", BIT24, dict(edge(32520, store="bf16"), launch="edge_msg_wsum"), WSUM(240, 1, 6, 136, zb=1)),
    ("wsum hhd 2048", BIT24, dict(edge(65280, H=8), launch="edge_msg_wsum"), WSUM(240, 2, 8, 272)),     # 4 x 16 x 128 > 4 096
    ("wsum hhd 2304", BIT24, dict(edge(65280, H=9), launch="edge_msg_wsum"), None),
    # the dense layer: one block has nothing to deal; 4 blocks over 2 tiles: groups 2, 4; 547 tiles: none
    ("dense 128 x 130", BIT24, dense(130, 128), R128(6, 1, 1, 2, adds=0)),
    ("dense 128 x 70000", BIT24, dense(70000, 128), R128(6, 1, 1, 547, adds=0)),
    ("dense 512 x 130", BIT24, dense(130, 512), R128(6, 4, 1, 2, adds=0)),
    ("dense 512 x 70000", BIT24, dense(70000, 512), R128(6, 1, 4, 547, adds=0)),
    ("dense 512 x 130", ("f16x3",), dense(130, 512), R128(2, 1, 4, 2, adds=0)),
    ("dense 512 x 130", ("bf16x3",), dense(130, 512), R128(3, 1, 4, 2, adds=0)),
]
CASES = [(what, mode, args, want) for what, modes, args, want in TABLE for mode in modes]


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"{c[0]} {c[1]}".replace(" ", "_") for c in CASES])
def test_form_table(case):
    from cgat_amd import debug
    what, mode, args, want = CASES[case]
    with _modes(mode, "f32"):
        got = debug.edge_z_form(**args)
    assert got == want, (what, mode, got, want)


def test_hidden_layer_never_runs_the_256_row_kernel():
    from cgat_amd import debug
    for mode in BIT24:
        with _modes(mode, "f32"):
            for E in (240, 14640, 32512, 32513, 32640, 65536, 1000080):
                for W2 in (512, 1536, 2560):
                    assert debug.edge_z_form(**hidden(E, W2))["kernel"] == "rows128", (mode, E, W2)


# (N, E) of 61 / 136 / 272 crystals of 20 atoms with 12 neighbours, the benchmark's large batch, and two around the bit
# form's own limit; layers H x Hd
SHAPES = [(1220, 14640), (2720, 32640), (5440, 65280), (83340, 1000080), (15810, 32640), (15811, 32640), (2709, 32508)]
LAYERS = [(3, 256), (1, 256), (5, 256), (8, 256), (9, 256), (3, 128)]


@pytest.mark.parametrize("mode", ["f16x3c", "bf16x6", "f16x3", "bf16x3"])
def test_layer_queries_agree_with_the_form(mode):
    """What the backward reads out of the saved buffer is decided by the layer's own predicates (layers.hip: attn_z_form,
    attn_bit_form_dims, attn_infer_fused); each must say what the launch's form says."""
    import ctypes as C
    from cgat_amd import _lib, debug
    for N, E in SHAPES:
        for H, Hd in LAYERS:
            plan, p = _lib.Plan(N, E, None, None, None, None, None, None), _lib.AttnParams(128, 128, H, Hd, *([None] * 8))
            with _modes(mode, "f32"):
                bits = debug.edge_z_form(**edge(E, N, H, Hd, store="bits"))
                assert bits is None or (bits["kernel"], bits["wide_mode"]) == ("rows256", 3)
                if debug.nodes_attention_bit_form(N, E, 128, 128, H, Hd):
                    assert bits is not None, (mode, N, E, H, Hd)
                if Hd == 256 and H in (1, 3, 5):     # where the backward has its bit-plane form, the two are one statement
                    assert debug.nodes_attention_bit_form(N, E, 128, 128, H, Hd) == (bits is not None), (mode, N, E, H, Hd)
                fused = _lib.lib.cgat_nodes_attention_infer_fused(C.byref(plan), C.byref(p))
                assert fused == int("fused_infer" in debug.nodes_attention_route(N, E, 128, 128, H, Hd))
                wsum = debug.edge_z_form(**dict(edge(E, N, H, Hd), launch="edge_msg_wsum"))
                if fused:
                    logits = debug.edge_z_form(**dict(edge(E, N, H, Hd), launch="edge_logits"))
                    assert (logits["kernel"], logits["wide_mode"]) == ("rows256", 1) and wsum["kernel"] == "msg_wsum"
                    few = cdiv(E, 256) < 128
                    assert (logits["groups"] > 1) == (few and H > 1), (mode, N, E, H, Hd, logits)
                # edgez.hip:1185-1193 of that commit
                assert fused == int(mode in BIT24 and Hd % 128 == 0 and H * Hd <= 2048 and H <= 8 and (E * H) % 4 == 0 and
                                    N * 4 * 2 * H * Hd < 2 ** 32), (mode, N, E, H, Hd)
            with _modes(mode, "bf16"):
                bwd = debug.nodes_attention_route(N, E, 128, 128, H, Hd, backward=True)
                fwd = debug.nodes_attention_route(N, E, 128, 128, H, Hd)
                if "z_bf16_six" in bwd:        # the backward will read bf16 rows written by the six-pass per-edge launch
                    f = debug.edge_z_form(**edge(E, N, H, Hd, store="bf16"))
                    assert "z_bf16" in fwd and f is not None and f["z_bf16"] == 1 and f["passes"] == 6, (mode, N, E, H, Hd, f)
                    assert f["kernel"] == ("rows256" if H * Hd <= 2048 else "rows128")


_CHILD = """
import sys
sys.path[:0] = [%r, %r]
from test_edgez_forms_cpu import *
from test_attn_workspace import _modes
from cgat_amd import debug
with _modes("f16x3c", "f32"):
    print(([debug.edge_z_form(**a) for a in (edge(32513), edge(14640), proj(3000), dense(130, 512),
                                             dict(edge(32508), launch="edge_logits"), dict(edge(32508), launch="edge_msg_wsum"))],
           debug.nodes_attention_bit_form(2720, 32640, 128, 128, 3, 256),
           "fused_infer" in debug.nodes_attention_route(2720, 32640, 128, 128, 3, 256)))
"""


def _child(env):
    out = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, HERE)], env=dict(os.environ, **env), capture_output=True,
                         text=True, check=True).stdout
    return eval(out.strip().splitlines()[-1])


def test_switch_edge_z6w_off():
    """CGAT_EDGE_Z6W=0 (edgez.hip:1080-1083, :1097, :1187): no 256-row kernel -- the 128-row kernel with its groups (255
    tiles: 2, 3) -- and with it neither the bit form nor the fused inference; nothing else moves."""
    forms, bit_form, fused = _child({"CGAT_EDGE_Z6W": "0"})
    assert forms[:4] == [R128(6, 3, 4, 255), R128(6, 6, 2, 115), R128(6, 12, 1, 24, adds=0), R128(6, 4, 1, 2, adds=0)]
    assert not bit_form and not fused


def test_switch_col_groups_off():
    """CGAT_Z_COL_GROUPS=0 (edgez.hip:1085-1088): no groups anywhere, so no few-row form: the 256-row kernel at any E.  The
    bit form keeps asking for 128 row tiles (edgez.hip:1104)."""
    forms, bit_form, fused = _child({"CGAT_Z_COL_GROUPS": "0"})
    assert forms == [R256(0, 1, 12, 128), R256(0, 1, 12, 58), R128(6, 1, 12, 24, adds=0), R128(6, 1, 4, 2, adds=0),
                     R256(1, 1, 6, 127), WSUM(240, 1, 6, 136)]
    assert bit_form and fused
    with_groups = _child({})
    assert with_groups[0][1] == R128(6, 6, 2, 115) and with_groups[1:] == (True, True)
