"""Device-side dataset packing, the part that needs no GPU: the numpy restatement of the packing rules
(tests/pack_cases.py) is tied to `PackedDataset.from_dict` as it stands, bit for bit, on every case; the new entry points
are declared, exported and bound; and the new routes refuse what they must before any device call."""
import os
import re

import numpy as np
import pytest
import torch

import pack_cases as PC


@pytest.mark.parametrize("target", PC.TARGETS)
@pytest.mark.parametrize("name", PC.NAMES)
def test_restatement_equals_from_dict(name, target):
    import cgat_amd as P
    c = PC.case(name)
    ref = PC.pack_reference(c, target)
    ds = P.PackedDataset.from_dict(PC.dictionary(name), PC.embedding(), c.K, target, device="cpu")
    for k in PC.ARRAYS:
        got = ds.t[k].numpy()
        assert got.dtype == ref[k].dtype and got.shape == ref[k].shape, k
        assert got.tobytes() == ref[k].tobytes(), k                     # bits, so -0.0 / NaN could not hide
    assert len(ds) == len(ref["kept"])
    assert np.array_equal(ds.host["natoms"], ref["natoms"]) and ds.host["natoms"].dtype == ref["natoms"].dtype
    assert np.array_equal(ds.host["nuniq"], ref["nuniq"]) and ds.host["nuniq"].dtype == ref["nuniq"].dtype


def test_cases_are_what_they_claim():
    tiny = PC.case("tiny")
    assert np.diff(tiny.atom_ptr).tolist() == [1, 2, 5, 7, 3] and tiny.Ks == tiny.K == 4
    ref = PC.pack_reference(tiny, "volume")
    assert np.diff(ref["comp_ptr"]).tolist() == [1, 1, 3, 7, 2]
    assert ref["comp_elem"][2:5].tolist() == [25, 7, 2] and ref["comp_elem"][-2:].tolist() == [7, 25]   # order of appearance
    assert ref["comp_weight"][2:5].tolist() == [np.float32(0.4), np.float32(0.4), np.float32(0.2)]
    assert PC.pack_reference(PC.case("ids_wide"), "volume")["comp_elem"].tolist() == [102, 0, 64, 63, 32, 31]
    drops = PC.case("drops")
    assert np.flatnonzero(drops.status).tolist() == [0, 3, 4, 7] and (drops.Ks, drops.K) == (24, 12)
    for K in (1, 64):
        big = PC.case(f"big_crystal_K{K}")
        assert np.diff(big.atom_ptr).tolist() == [1, 1024, 1] and (big.Ks, big.K) == (64, K)
        assert np.diff(PC.pack_reference(big, "volume")["comp_ptr"]).tolist() == [1, 103, 1]
    odd = PC.case("odd_columns")
    assert (odd.Ks, odd.K) == (7, 5)
    many = PC.case("many")
    assert len(many.status) == PC.MANY_G >= 4 * PC.SCAN_TILE and many.status[5000:5300].all() and many.status[::7].all()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "cgat_amd", "csrc", "pack.hip")).read()
    assert int(re.search(r"#define PACK_SCAN_TILE (\d+)", src).group(1)) == PC.SCAN_TILE
    for name in ("empty", "all_dropped"):
        assert len(PC.pack_reference(PC.case(name), "volume")["kept"]) == 0


def test_entry_points_declared_exported_bound():
    from cgat_amd import _lib
    for n in ("cgat_pack_dataset_workspace_bytes", "cgat_pack_dataset_plan", "cgat_pack_dataset_write"):
        assert n in _lib.PROTOTYPES and hasattr(_lib.lib, n)
    ws = _lib.lib.cgat_pack_dataset_workspace_bytes
    assert ws(0, 0) > 0 and ws(20000, 40000) >= 5 * 4 * 20000 and ws(20000, 0) == ws(20000, 40000)
    # argument checks come before any launch, so they answer without a device
    assert _lib.lib.cgat_pack_dataset_plan(None, None, None, -1, 0, 103, None, None, 0, None) == 1
    assert b"pack_dataset_plan" in _lib.lib.cgat_last_error()


def test_from_tables_refuses_cpu_tensors():
    import cgat_amd as P
    c = PC.case("tiny")
    tabs = tuple(torch.from_numpy(t) for t in (c.shell, c.self_idx, c.nbr_idx, c.status))
    for device in ("cpu", "cuda:0"):
        with pytest.raises(RuntimeError, match="no CPU path"):
            P.PackedDataset.from_tables(tabs, c.atom_ptr, torch.from_numpy(c.atom_elem), PC.embedding(),
                                        {"e_above_hull": c.targets}, max_neighbor_number=c.K, device=device)


def test_from_arrays_unknown_symbol():
    import cgat_amd as P
    lat, frac = np.eye(3)[None] * 4.0, np.zeros((2, 3))
    with pytest.raises(AssertionError, match="^Xx is not an allowed atom type$"):
        P.PackedDataset.from_arrays(lat, frac, np.array([0, 2], np.int32), ["Fe", "Xx"], {"e_above_hull": [0.0]},
                                    PC.embedding(), device="cpu")
    with pytest.raises(AssertionError, match="^Qq is not an allowed atom type$"):      # the first unknown atom, as from_dict
        P.PackedDataset.from_arrays(lat, frac, np.array([0, 2], np.int32), ["Qq", "Aa"], {"e_above_hull": [0.0]},
                                    PC.embedding(), device="cpu")


def test_symbols_map_to_rows_in_one_step():
    from cgat_amd.collate import _symbol_rows
    from cgat_amd.graph import ELEMENT_SYMBOLS
    ids = np.random.RandomState(0).randint(0, 103, size=500)
    rows = _symbol_rows([ELEMENT_SYMBOLS[i] for i in ids], list(ELEMENT_SYMBOLS))
    assert rows.dtype == np.int32 and np.array_equal(rows, ids)
    assert _symbol_rows([], list(ELEMENT_SYMBOLS)).shape == (0,)


def test_from_structures_pack_keyword():
    import cgat_amd as P
    s = [(np.eye(3) * 3.0, np.zeros((1, 3)), ["Fe"])]
    with pytest.raises(ValueError, match="pack must be 'host' or 'device'"):
        P.PackedDataset.from_structures(s, {"e_above_hull": [0.0]}, PC.embedding(), device="cpu", pack="bogus")
