"""Neighbour tables, the part that needs no GPU: the entry is declared, exported and bound; the Python
entries validate their inputs and refuse CPU tensors; the numpy restatement (tests/neighbor_cases.py) reproduces the
hand-known shell structure of simple lattices; and the INPUT CONDITION of the GPU comparisons holds -- no adjacent gap of
the sorted distances that decide a row lies in (1e-10, 1e-6), so shell membership does not depend on last-bit rounding and
the integer tables compare exactly."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import neighbor_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_declared_exported_bound():
    from cgat_amd import _lib
    src = open(os.path.join(ROOT, "include", "cgat_hip.h")).read()
    assert "prepare_data.py:146-169" in src
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("cgat_neighbor_tables", "cgat_debug_neighbor_tables"):
        assert re.search(r"\b%s\s*\(" % n, decl), n
        assert hasattr(lib, n) and n in _lib.PROTOTYPES, n
    assert _lib.ABI_VERSION == 3 and _lib.lib.cgat_abi_version() == 3
    build = open(os.path.join(ROOT, "cgat_amd", "build_lib.sh")).read()
    assert re.search(r"SRCS=\([^)]*\bneighbors\b", build)


def test_names_exported():
    import cgat_amd as P
    for n in ("neighbors", "neighbor_tables", "dataset_dict_from_structures", "synthetic_structures", "NeighborTables"):
        assert hasattr(P, n) and n in P.__all__, n
    assert callable(P.PackedDataset.from_structures)
    assert callable(P.neighbors.synthetic_structures)


def _valid():
    lat, frac, ptr = NC.flat([NC.rocksalt(), NC.hcp()])
    return torch.from_numpy(lat), torch.from_numpy(frac), torch.from_numpy(ptr)


def test_cpu_tensors_refused():
    import cgat_amd as P
    lat, frac, ptr = _valid()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.neighbor_tables(lat, frac, ptr, 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.dataset_dict_from_structures([(NC.rocksalt()[0], NC.rocksalt()[1], ["Na"] * 4 + ["Cl"] * 4)], {"e": [1.0]},
                                       device="cpu")


def test_value_errors():
    import cgat_amd as P
    lat, frac, ptr = _valid()
    for K in (0, 65, -3, 2.5):
        with pytest.raises(ValueError, match="1..64"):
            P.neighbor_tables(lat, frac, ptr, K)
    with pytest.raises(ValueError, match="radius"):
        P.neighbor_tables(lat, frac, ptr, 12, radius=0.0)
    with pytest.raises(ValueError, match="float64"):
        P.neighbor_tables(lat.float(), frac, ptr, 12)
    with pytest.raises(ValueError, match="float64"):
        P.neighbor_tables(lat, frac.float(), ptr, 12)
    with pytest.raises(ValueError, match="int32"):
        P.neighbor_tables(lat, frac, ptr.long(), 12)
    with pytest.raises(ValueError, match=r"\[G, 3, 3\]"):
        P.neighbor_tables(lat.reshape(-1, 9), frac, ptr, 12)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        P.neighbor_tables(lat, frac.reshape(-1), ptr, 12)
    with pytest.raises(ValueError, match="atom_ptr must be"):
        P.neighbor_tables(lat, frac, ptr[:-1], 12)
    for bad in ([1, 8, 10], [0, 8, 9], [0, 12, 10]):
        with pytest.raises(ValueError, match="non-decreasing"):
            P.neighbor_tables(lat, frac, torch.tensor(bad, dtype=torch.int32), 12)
    sing = lat.clone()
    sing[1, 2] = sing[1, 0] + sing[1, 1]              # c in the plane of a and b
    with pytest.raises(ValueError, match="singular"):
        P.neighbor_tables(sing, frac, ptr, 12)
    flat_cell = (np.array([[3., 0, 0], [0, 3., 0], [3., 3., 0]]), np.zeros((1, 3)), ["Fe"])
    with pytest.raises(ValueError, match="singular"):
        P.dataset_dict_from_structures([flat_cell], {"e": [0.0]}, device="cpu")
    with pytest.raises(ValueError, match="species"):
        P.dataset_dict_from_structures([(np.eye(3) * 3, np.zeros((2, 3)), ["Fe"])], {"e": [0.0]}, device="cpu")
    with pytest.raises(ValueError, match="values"):
        P.dataset_dict_from_structures([(np.eye(3) * 3, np.zeros((1, 3)), ["Fe"])], {"e": [0.0, 1.0]}, device="cpu")


def test_restatement_known_shells():
    assert NC.shell_counts(*NC.cubic(3.0), 24) == [6, 12, 6]            # 6 of the 8 at a*sqrt(3)
    assert NC.shell_counts(*NC.cubic(3.0), 6) == [6]
    assert NC.shell_counts(*NC.fcc_primitive(4.0), 24) == [12, 6, 6]    # 6 of the 24 at a*sqrt(3/2)
    assert NC.shell_counts(*NC.fcc_primitive(4.0), 12) == [12]
    assert NC.shell_counts(*NC.rocksalt(), 12) == [6, 6]                # 6 of the 12 at a/sqrt(2)
    assert NC.shell_counts(*NC.hcp(), 24) == [6, 6, 6, 2, 4]
    st, shell, self_idx, nbr, dist = NC.reference_tables(*NC.rocksalt(), 12)
    assert st == 0 and np.allclose(dist[:, :6], 5.64 / 2) and np.allclose(dist[:, 6:], 5.64 / np.sqrt(2))
    assert (self_idx == np.arange(8)[:, None]).all()
    assert (np.diff(shell, axis=1) >= 0).all()
    same = np.diff(shell, axis=1) == 0
    assert (np.diff(nbr, axis=1)[same] >= 0).all()                      # (shell, j) row order
    assert NC.reference_tables(*NC.cubic(8.0), 24)[0] == 0
    assert NC.reference_tables(*NC.cubic(15.0), 24)[0] == 1             # 6 neighbours within 18 A
    assert NC.reference_tables(*NC.cubic(15.0), 6)[0] == 0 and NC.reference_tables(*NC.cubic(15.0), 7)[0] == 1


def test_restatement_skewed_cell_needs_interplanar_range():
    """The triclinic case is one where an image range from |a| is too short: its true nearest neighbours lie further
    than floor(radius / |a|) + 1 images away along some axis at a small radius."""
    lat, frac = NC.triclinic_skewed()
    _, _, h = NC._geometry(lat, frac)
    assert min(h) < 0.4 * min(np.linalg.norm(lat, axis=1))
    a = NC.reference_tables(lat, frac, 24)
    b = NC.reference_tables(lat, frac - np.floor(frac), 24)
    c = NC.reference_tables(lat, frac + np.array([0.37, -1.21, 2.6]), 24)
    for x, y in ((a, b), (a, c)):
        assert x[0] == y[0] == 0 and all(np.array_equal(p, q) for p, q in zip(x[1:4], y[1:4]))
        assert np.abs(x[4] - y[4]).max() < 2e-8


@pytest.mark.parametrize("name,K,radius", NC.GPU_RUNS, ids=[f"{n}-K{k}-r{r:g}" for n, k, r in NC.GPU_RUNS])
def test_input_condition(name, K, radius):
    for (lat, frac), cands in zip(NC.batch(name), NC.candidates(name, radius)):
        assert NC.ambiguous_gaps(lat, frac, K, radius, cands) == 0


def test_synthetic_structures_seeded():
    import cgat_amd as P
    a, b = P.synthetic_structures(5, 3), P.synthetic_structures(5, 3)
    assert len(a) == 5
    for (la, fa, sa), (lb, fb, sb) in zip(a, b):
        assert np.array_equal(la, lb) and np.array_equal(fa, fb) and sa == sb
        assert la.shape == (3, 3) and fa.shape == (len(sa), 3) and 1 <= len(sa) <= 40 and abs(np.linalg.det(la)) > 1
    assert all(len(s[2]) == 20 for s in P.synthetic_structures(3, 0, atoms=20))
