"""Which form a launch of the backward per-edge family (csrc/edgebwd.hip: edge_ge_kernel, edge_gw_kernel) runs.  The forms
of one launch agree within tolerance -- the bit-plane and K-split forms re-round -- so a launch that quietly fell back to
six passes, or took another group count, would pass every parity test and only cost speed; cgat_debug_edge_bwd_form names
the form, and the table below pins it.  Host arithmetic only: no GPU.

The table was written from the conditions of the launchers as they stood before the form became a named value (commit
6796ce7; csrc/edgebwd.hip of that commit unless another file is named, cited per condition), not from the query's output:
  grad edge_attr (edge_ge), the plain launch
    fp16 form            f16x3 with max |rows| given, a weight with 128 contiguous outputs (:897-898): two planes scaled by
                         the weight's maximum (:903-909)
    bit-plane body       not the fp16 form; rebuilt rows, a 24-bit mode, not "bf16-mma", 1 <= H <= 8, Hd % 128 == 0, W2 / 32
                         mask words, and the launch group's columns a multiple of Hd (:878-881, :900): the attention-scaled
                         image with column sums (:910-912)
    one pass             rebuilt rows, not the fp16 form, "bf16-mma", not bf16x3 (:922)
    else                 six passes, three in bf16x3 (:927-928); three bf16 planes (:914); row tiles of 256 (:917)
  K-split groups         1 outside the 24-bit modes, below 1 024 rows, from 192 row tiles of 256; else the divisors S >= 2 of
                         the column blocks with an even quotient in ascending order, stopping at the first with tiles * S >=
                         192 (the largest if none) (:941-949); never for rebuilt rows under "bf16-mma" (layers.hip:573).  The
                         launch refuses other modes (:954); its bodies are the bit-plane body where it holds for a GROUP's
                         blocks, else six passes (:957, :967-976)
  prepared image         six passes on the caller's image, whatever the mode (:984-994)
  heads                  f16x3: two fp16 planes by the batched preparation (:1027-1036); else the six-pass image (:1018-1025);
                         grid.y = head
  grad W_e (edge_gw)
    plain form           256 / (W2 / 256) k-ranges per column-block pair (:1045-1049, :1156, :1198); fp16 planes with both
                         maxima given in f16x3 (:1160); one pass for rebuilt rows under "bf16-mma" outside bf16x3 (:1201);
                         else six passes, three in bf16x3 (:1203-1204)
    bit-plane shape      f16x3c / bf16x6, not "bf16-mma", Hd == 256, W2 - H Hd a positive multiple of 256 (:1061-1062); SA =
                         768 / (3 H + 4 npm) >= 1, SM = (256 - H SA) / npm >= 1 (:1063-1069)
    bit-plane form       that shape, not the fp16 form, rebuilt rows, a permutation, no force_six (:1071-1073, :1164);
                         SM npm + SA H workgroups (:1181)
    te                   with the bit-plane form off: that form first, for te alone (:1171, :1175-1192); refused without its
                         shape (:1172-1174)
    workspace            slabs behind the planes of e rounded up to 16 floats (:1158); attention slabs behind SM message
                         slabs, column sums behind SA attention slabs (:1177-1178), SA H 8 rows of 128 (:1119-1120); the size
                         query: planes + max(plain slabs, 256 x 256 x 128 + 256 x 8 x 128) + 64 (:1087-1091)"""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from test_attn_workspace import _modes   # noqa: E402

BIT24 = ("f16x3c", "bf16x6")
ALL = ("f16x3c", "bf16x6", "f16x3", "bf16x3", "f32")
F32, MMA = ("f32",), ("bf16-mma",)
BOTH = F32 + MMA


def cdiv(a, b):
    return -(-a // b)


def GE(passes, rc, bitplane, prep, tiles, groups=1, per_group=12, heads=0):
    return dict(passes=passes, rc=rc, bitplane=bitplane, prep=prep, grid_x=tiles, groups=groups, blocks_per_group=per_group,
                heads=heads)


# the per-edge launch of a scalar-attention layer over rebuilt rows, H 3, Hd 256: W2 = 1536 = 12 column blocks
def ge(rows, H=3, Hd=256, W2=None, rebuilt=True, **kw):
    return dict(product="ge", rows=rows, W2=2 * H * Hd if W2 is None else W2, H=H, Hd=Hd, rebuilt=rebuilt, perm=rebuilt, **kw)


def gw_ws(E, W2, H=0, SA=0, SM=0, S=None):
    """(ws_end, ws_floats) by the parent's carve (:1158, :1177-1178, :1119-1120, :1087-1091)"""
    S = 256 // (W2 // 256) if S is None else S
    planes = (cdiv(E, 128) * 128 * 128 * 3 + 1) // 2
    slab = cdiv(planes, 16) * 16
    end = slab + S * W2 * 128
    if SA:
        end = max(end, slab + SM * (W2 - H * 256) * 128 + SA * H * 256 * 128 + SA * H * 8 * 128)
    return end, planes + max(S * W2 * 128, 256 * 256 * 128 + 256 * 8 * 128) + 64


def GW(E, W2, passes, rc, bitplane=0, bit_shape=0, te_only=0, H=0, SA=0, SM=0):
    S = 256 // (W2 // 256)
    npm = (W2 - H * 256) // 256 if SA else 0
    end, floats = gw_ws(E, W2, H, SA, SM)
    return dict(passes=passes, rc=rc, bitplane=bitplane, grid_x=S * (W2 // 256), bit_shape=bit_shape, te_only=te_only, ranges=S,
                SA=SA, SM=SM, message_pairs=npm, bit_grid_x=SM * npm + SA * H, ws_end=end, ws_floats=floats)


def gw(E, H=3, Hd=256, W2=None, rebuilt=True, perm=True, **kw):
    return dict(product="gw", rows=E, W2=2 * H * Hd if W2 is None else W2, H=H, Hd=Hd, rebuilt=rebuilt, perm=perm, **kw)


E = 65280      # 272 crystals of 20 atoms with 12 neighbours: 255 row tiles of 256
# (what, arithmetic modes, edge storages, arguments of debug.edge_bwd_form, form or None = refused)
TABLE = [
    # ---- grad edge_attr, the plain launch ----
    ("ge rebuilt", BIT24, F32, ge(E), GE(6, 1, 1, "attn", 255)),
    ("ge rebuilt", BIT24, MMA, ge(E), GE(1, 1, 0, "planes", 255)),
    ("ge rebuilt", ("f16x3",), F32, ge(E), GE(6, 1, 0, "planes", 255)),
    ("ge rebuilt maxima", ("f16x3",), BOTH, ge(E, maxima=True), GE(2, 1, 0, "f16_tmax", 255)),
    ("ge rebuilt", ("f16x3",), MMA, ge(E), GE(1, 1, 0, "planes", 255)),
    ("ge rebuilt", ("bf16x3",), BOTH, ge(E), GE(3, 1, 0, "planes", 255)),
    ("ge rebuilt maxima", BIT24, F32, ge(E, maxima=True), GE(6, 1, 1, "attn", 255)),       # (maxima: f16x3 alone reads them)
    # the bit-plane body's shape: heads of whole column blocks (Hd 128 holds), at most 8 heads
    ("ge H 6 Hd 128", BIT24, F32, ge(E, H=6, Hd=128), GE(6, 1, 1, "attn", 255)),
    ("ge H 8", BIT24, F32, ge(E, H=8), GE(6, 1, 1, "attn", 255, per_group=32)),
    ("ge H 9", BIT24, F32, ge(E, H=9), GE(6, 1, 0, "planes", 255, per_group=36)),
    ("ge Hd 192", BIT24, F32, ge(E, H=4, Hd=192), GE(6, 1, 0, "planes", 255)),
    # stored rows (the node-side products, the dense layer): never one pass, never the bit-plane body
    ("ge stored", BIT24, BOTH, ge(3000, rebuilt=False), GE(6, 0, 0, "planes", 12)),
    ("ge stored", ("f16x3",), BOTH, ge(3000, rebuilt=False), GE(6, 0, 0, "planes", 12)),
    ("ge stored maxima", ("f16x3",), BOTH, ge(3000, rebuilt=False, maxima=True), GE(2, 0, 0, "f16_tmax", 12)),
    ("ge stored", ("bf16x3",), BOTH, ge(3000, rebuilt=False), GE(3, 0, 0, "planes", 12)),
    ("ge stored", ("f32",), F32, ge(3000, rebuilt=False), GE(6, 0, 0, "planes", 12)),      # (no caller launches it in f32: edge_ge_dims)
    ("ge no rows", ALL, F32, ge(0), GE(0, 0, 0, "none", 0, groups=0, per_group=0)),
    # ---- the K-split launch with the groups the layers give it, W2 = 1536: 12 blocks, S in 2 (6 blocks), 3 (4), 6 (2) ----
    ("ksplit 1023", BIT24, F32, ge(1023, launch="ksplit"), GE(6, 1, 1, "attn", 4)),
    ("ksplit 1280", BIT24, F32, ge(1280, launch="ksplit"), GE(6, 1, 1, "attn", 5, 6, 2)),          # 5 tiles: 10, 15, 30 < 192
    ("ksplit 16384", BIT24, F32, ge(16384, launch="ksplit"), GE(6, 1, 1, "attn", 64, 3, 4)),       # 64 tiles: 128, then 192
    ("ksplit 30720", BIT24, F32, ge(30720, launch="ksplit"), GE(6, 1, 1, "attn", 120, 2, 6)),
    ("ksplit 48896", BIT24, F32, ge(48896, launch="ksplit"), GE(6, 1, 1, "attn", 191, 2, 6)),
    ("ksplit 48897", BIT24, F32, ge(48897, launch="ksplit"), GE(6, 1, 1, "attn", 192)),
    ("ksplit stored 1280", BIT24, BOTH, ge(1280, launch="ksplit", rebuilt=False), GE(6, 0, 0, "planes", 5, 6, 2)),
    # rebuilt rows under "bf16-mma": no groups, the one-pass body of the plain launch
    ("ksplit 1280", BIT24, MMA, ge(1280, launch="ksplit"), GE(1, 1, 0, "planes", 5)),
    # a group's blocks against a head: Hd 512 in groups of 2 blocks (24 blocks: S 2, 3, 4, 6, 12 -> 60 < 192) starts inside
    # a head; in groups of 12 (120 tiles: S 2) it does not
    ("ksplit Hd 512 1280", BIT24, F32, ge(1280, Hd=512, launch="ksplit"), GE(6, 1, 0, "planes", 5, 12, 2)),
    ("ksplit Hd 512 30720", BIT24, F32, ge(30720, Hd=512, launch="ksplit"), GE(6, 1, 1, "attn", 120, 2, 12)),
    ("ksplit", ("f16x3", "bf16x3", "f32"), F32, ge(1280, launch="ksplit"), None),
    # ---- a prepared image: fc_out_M as one K = H Hd launch; the mode does not enter ----
    ("prepared", ALL, BOTH, ge(3000, W2=768, rebuilt=False, launch="prepared"), GE(6, 0, 0, "none", 12, per_group=6)),
    # ---- the heads launch: 5 second layers of K = 256 ----
    ("heads", BIT24, F32, ge(3000, H=5, W2=256, rebuilt=False, launch="heads"), GE(6, 0, 0, "planes", 12, per_group=2, heads=5)),
    ("heads", ("f16x3",), F32, ge(3000, H=5, W2=256, rebuilt=False, maxima=True, launch="heads"),
     GE(2, 0, 0, "heads_f16", 12, per_group=2, heads=5)),
    # ---- grad W_e ----
    ("gw H 3", BIT24, F32, gw(E), GW(E, 1536, 6, 1, 1, 1, H=3, SA=36, SM=49)),                       # 255 workgroups; plain: 42 ranges
    ("gw H 5", BIT24, F32, gw(E, H=5), GW(E, 2560, 6, 1, 1, 1, H=5, SA=21, SM=30)),
    ("gw H 1", BIT24, F32, gw(E, H=1), GW(E, 512, 6, 1, 1, 1, H=1, SA=109, SM=147)),                 # 768 / 7; 256 - 109
    ("gw few edges", BIT24, F32, gw(240), GW(240, 1536, 6, 1, 1, 1, H=3, SA=36, SM=49)),
    ("gw Hd 128", BIT24, F32, gw(E, H=6, Hd=128), GW(E, 1536, 6, 1)),
    ("gw bf16-mma", BIT24, MMA, gw(E), GW(E, 1536, 1, 1)),
    ("gw maxima", ("f16x3",), BOTH, gw(E, maxima=True), GW(E, 1536, 2, 1)),
    ("gw", ("f16x3",), F32, gw(E), GW(E, 1536, 6, 1)),
    ("gw", ("f16x3",), MMA, gw(E), GW(E, 1536, 1, 1)),
    ("gw", ("bf16x3",), BOTH, gw(E), GW(E, 1536, 3, 1)),
    ("gw no permutation", BIT24, F32, gw(E, perm=False), GW(E, 1536, 6, 1)),
    ("gw force_six", BIT24, F32, gw(E, force_six=True), GW(E, 1536, 6, 1, 0, 1, H=3, SA=36, SM=49)),
    ("gw force_six te", BIT24, F32, gw(E, force_six=True, te=True), GW(E, 1536, 6, 1, 0, 1, 1, H=3, SA=36, SM=49)),
    ("gw te", BIT24, F32, gw(E, te=True), GW(E, 1536, 6, 1, 1, 1, H=3, SA=36, SM=49)),
    ("gw te Hd 128", BIT24, F32, gw(E, H=6, Hd=128, te=True), None),
    ("gw te", ("f16x3", "bf16x3"), F32, gw(E, te=True), None),
    ("gw te bf16-mma", BIT24, MMA, gw(E, te=True), None),
    # stored rows (the node-side weight gradients): never one pass
    ("gw stored", BIT24, BOTH, gw(3000, rebuilt=False, perm=False), GW(3000, 1536, 6, 0)),
    ("gw stored maxima", ("f16x3",), BOTH, gw(3000, rebuilt=False, perm=False, maxima=True), GW(3000, 1536, 2, 0)),
    ("gw stored", ("bf16x3",), F32, gw(3000, rebuilt=False, perm=False), GW(3000, 1536, 3, 0)),
    ("gw stored", ("f32",), F32, gw(3000, rebuilt=False, perm=False), GW(3000, 1536, 6, 0)),
]
CASES = [(what, mode, st, args, want) for what, modes, storages, args, want in TABLE for mode in modes for st in storages]


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"{c[0]} {c[1]} {c[2]}".replace(" ", "_") for c in CASES])
def test_form_table(case):
    from cgat_amd import debug
    what, mode, storage, args, want = CASES[case]
    with _modes(mode, storage):
        got = debug.edge_bwd_form(**args)
    assert got == want, (what, mode, storage, got, want)


def test_gw_no_rows():
    from cgat_amd import debug
    with _modes("f16x3c", "f32"):
        f = debug.edge_bwd_form(**gw(0))
    assert all(v == 0 for k, v in f.items() if k != "ws_floats"), f


def test_process_wide_switch_moves_the_form_not_the_shape():
    """cgat_debug_edge_gw_force_six (:1057-1058, :1072) keeps the six-pass form; what the layer's saved buffer rests on
    (edge_gw_bitplane_layer, :1075-1078: mode and shape alone) does not move with it."""
    from cgat_amd import debug
    with _modes("f16x3c", "f32"):
        before = debug.nodes_attention_bit_form(2720, 32640, 128, 128, 3, 256)
        was = debug.edge_gw_force_six(True)
        try:
            f = debug.edge_bwd_form(**gw(E))
            te = debug.edge_bwd_form(**gw(E, te=True))
            assert debug.nodes_attention_bit_form(2720, 32640, 128, 128, 3, 256) == before == True  # noqa: E712
        finally:
            debug.edge_gw_force_six(was)
    assert (f["bitplane"], f["bit_shape"], f["te_only"]) == (0, 1, 0) and (te["bitplane"], te["te_only"]) == (0, 1)


@pytest.mark.parametrize("mode", ALL)
def test_ksplit_groups_sweep(mode):
    """Every K group holds an even number of blocks, the groups divide the blocks, and a group count is only taken in a
    24-bit mode between 1 024 rows and 192 row tiles."""
    from cgat_amd import debug
    rows_list = [1, 1023, 1024, 1280, 3000, 5440, 16384, 24575, 24576, 30720, 48896, 48897, 65280, 1000080]
    for storage in BOTH:
        with _modes(mode, storage):
            for W2 in (256, 512, 768, 1536, 2560, 3072, 4096, 4608):
                for rows in rows_list:
                    for rebuilt in (False, True):
                        f = debug.edge_bwd_form(**ge(rows, H=W2 // 512 or 1, Hd=256, W2=W2, rebuilt=rebuilt, launch="ksplit"))
                        if mode not in BIT24:
                            assert f is None, (mode, storage, W2, rows, f)
                            continue
                        ncb, g, per = W2 // 128, f["groups"], f["blocks_per_group"]
                        assert g >= 1 and g * per == ncb and (g == 1 or per % 2 == 0), (mode, storage, W2, rows, f)
                        if g > 1:
                            assert rows >= 1024 and cdiv(rows, 256) < 192 and not (rebuilt and storage == "bf16-mma")
                            assert f["passes"] == 6
                            # (a larger count is taken only while the last one left the chip short of 192 workgroups)
                            smaller = [s for s in range(2, g) if ncb % s == 0 and (ncb // s) % 2 == 0]
                            assert all(cdiv(rows, 256) * s < 192 for s in smaller), (mode, W2, rows, f)
                        assert f["grid_x"] == cdiv(rows, 256)


@pytest.mark.parametrize("mode", ALL)
def test_gw_split_sweep(mode):
    """H * SA + npm * SM <= 256 with both at least 1, the size query covers the carve of whichever form runs, and the
    layer's bit form of the saved buffer is only taken where grad W_e has its bit-plane shape."""
    from cgat_amd import debug
    for storage in BOTH:
        with _modes(mode, storage):
            for Ecount in (1, 240, 14640, 32640, 65280, 1000080):
                for H, Hd in [(h, 256) for h in range(1, 9)] + [(3, 128), (6, 128), (3, 384), (2, 512)]:
                    for kw in ({}, dict(force_six=True), dict(perm=False), dict(maxima=True), dict(rebuilt=False, perm=False)):
                        f = debug.edge_bwd_form(**gw(Ecount, H=H, Hd=Hd, **kw))
                        W2 = 2 * H * Hd
                        assert f["ws_end"] <= f["ws_floats"], (mode, storage, Ecount, H, Hd, kw, f)
                        assert f["ranges"] * (W2 // 256) == f["grid_x"] <= 256
                        if f["bit_shape"]:
                            assert mode in BIT24 and storage == "f32" and Hd == 256 and "perm" not in kw
                            assert f["SA"] >= 1 and f["SM"] >= 1 and f["message_pairs"] == H
                            assert H * f["SA"] + f["message_pairs"] * f["SM"] == f["bit_grid_x"] <= 256
                        else:
                            assert (f["SA"], f["SM"], f["bit_grid_x"], f["bitplane"]) == (0, 0, 0, 0)
                        assert f["bitplane"] == int(bool(f["bit_shape"]) and not kw.get("force_six"))
                    if debug.nodes_attention_bit_form(Ecount // 12, Ecount, 128, 128, H, Hd):
                        assert debug.edge_bwd_form(**gw(Ecount, H=H, Hd=Hd))["bit_shape"] == 1, (mode, storage, Ecount, H, Hd)
