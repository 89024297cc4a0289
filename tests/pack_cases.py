"""Cases for the device-side dataset packing (csrc/pack.hip, PackedDataset.from_tables) and a numpy restatement of its
rules, `pack_reference`.

A case holds flat inputs as `from_tables` takes them -- atom_ptr, element rows per atom, three integer tables [N, Ks], a
status vector, fp64 per-cell targets -- and `dictionary(case)` gives the reference-format dictionary of the crystals whose
status is 0, as `dataset_dict_from_structures` would build it, for `PackedDataset.from_dict`.  The tables need no
geometric meaning (packing only copies them): self_idx / nbr_idx are random in [0, n), shell in [1, Ks].

The rules restated (cgat_amd/collate.py from_dict, include/cgat_hip.h):
  comp_elem    the crystal's distinct element rows in first-appearance order (not sorted)
  comp_weight  float32(float64(count) / float64(n_atoms))
  y_val        q = float32(float64(target) / float64(n_atoms));  q * float32(n_atoms), or q alone for target "volume"
  tables       the first K of the Ks stored columns of every kept row
"""
import functools
from collections import namedtuple

import numpy as np

from cgat_amd.graph import ELEMENT_SYMBOLS, element_table

Case = namedtuple("Case", "name atom_ptr atom_elem shell self_idx nbr_idx status targets Ks K")
ARRAYS = ("table", "atom_ptr", "atom_elem", "shell", "self_idx", "nbr_idx", "comp_ptr", "comp_elem", "comp_weight", "y_val")
TARGETS = ("e_above_hull", "volume")          # target mode 0 (times n_atoms) and 1 (as stored)
# negative, zero, tiny, huge, and values whose quotient by 3 or 7 is inexact
TARGET_VALUES = np.array([-1.5, 0.0, 1e-30, 1e30, 2.75, -3e-7, 10.0, -1e30, 1.0, 0.1], np.float64)
SCAN_TILE = 1024                              # PACK_SCAN_TILE of csrc/pack.hip: crystals per workgroup of the prefix sums
MANY_G = 20000
assert MANY_G >= 4 * SCAN_TILE                # `many` carries offsets across >= 19 tiles and across the tile-sum scan


@functools.lru_cache(maxsize=None)
def embedding():
    table = element_table().numpy()
    return {el: table[k].astype("float64").tolist() for k, el in enumerate(ELEMENT_SYMBOLS)}


def _build(name, species, Ks, K, dropped=(), seed=0, targets=None):
    """species: one sequence of element rows per crystal"""
    rs = np.random.RandomState(seed)
    G = len(species)
    natoms = np.array([len(s) for s in species], np.int64)
    atom_ptr = np.zeros(G + 1, np.int64)
    atom_ptr[1:] = np.cumsum(natoms)
    N = int(atom_ptr[-1])
    elem = np.concatenate([np.asarray(s, np.int32) for s in species]).astype(np.int32) if G else np.zeros(0, np.int32)
    per_atom = np.repeat(natoms, natoms)[:, None] if N else np.ones((0, 1), np.int64)
    self_idx = (rs.randint(0, 2 ** 30, size=(N, Ks)) % per_atom).astype(np.int32)
    nbr_idx = (rs.randint(0, 2 ** 30, size=(N, Ks)) % per_atom).astype(np.int32)
    shell = rs.randint(1, Ks + 1, size=(N, Ks)).astype(np.int32)
    status = np.zeros(G, np.int32)
    status[list(dropped)] = 1
    if targets is None:
        targets = TARGET_VALUES[np.arange(G) % len(TARGET_VALUES)]
    return Case(name, atom_ptr.astype(np.int32), elem, shell, self_idx, nbr_idx, status, np.asarray(targets, np.float64), Ks, K)


def _tiny():
    A, B, C = 25, 7, 2
    return _build("tiny", [[A], [A, A], [A, B, A, C, B], [40, 3, 99, 12, 0, 77, 56], [B, A, B]], 4, 4,
                  targets=[-1.5, 1e-30, 1e30, 2.75, 0.1])     # atom counts 3 (last) and 7: inexact quotients


def _drops():
    rs = np.random.RandomState(1)
    species = [rs.randint(0, 103, size=rs.randint(1, 9)).tolist() for _ in range(8)]
    return _build("drops", species, 24, 12, dropped=(0, 3, 4, 7), seed=1)


def _all_dropped():
    return _build("all_dropped", [[1, 2], [3], [4, 4, 5]], 8, 4, dropped=(0, 1, 2), seed=2)


def _empty():
    return _build("empty", [], 8, 4)


def _ids_wide():
    return _build("ids_wide", [[102, 0, 64, 63, 32, 31, 0, 102]], 4, 4, seed=3, targets=[-0.7])


def _big(K):
    order = np.random.RandomState(4).permutation(103)
    return _build(f"big_crystal_K{K}", [[5], order[np.arange(1024) % 103].tolist(), [9]], 64, K, seed=4,
                  targets=[1.0, -123.456, 1e-30])


def _odd_columns():
    rs = np.random.RandomState(5)
    species = [rs.randint(0, 103, size=n).tolist() for n in (3, 1, 7, 70, 2)]     # one crystal wider than a wave
    return _build("odd_columns", species, 7, 5, dropped=(1,), seed=5)


def _many():
    rs = np.random.RandomState(6)
    n = rs.randint(1, 4, size=MANY_G)
    pool = rs.randint(0, 103, size=int(n.sum()))
    species = np.split(pool, np.cumsum(n)[:-1])
    dropped = sorted(set(range(0, MANY_G, 7)) | set(range(5000, 5300)))
    return _build("many", species, 4, 4, dropped=dropped, seed=6, targets=rs.uniform(-5.0, 5.0, size=MANY_G))


_BUILDERS = {"tiny": _tiny, "drops": _drops, "all_dropped": _all_dropped, "empty": _empty, "ids_wide": _ids_wide,
             "big_crystal_K1": lambda: _big(1), "big_crystal_K64": lambda: _big(64), "odd_columns": _odd_columns,
             "many": _many}
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


def _formula(syms):
    return "".join(f"{el}{syms.count(el)}" for el in dict.fromkeys(syms))


@functools.lru_cache(maxsize=None)
def dictionary(name):
    """The reference-format dictionary (layout 0 of CGAT/data.py:47-50) of the kept crystals of `case(name)`, targets
    stored divided by the atom count (prepare_data.py:139)."""
    c = case(name)
    kept = np.flatnonzero(c.status == 0)
    ptr = c.atom_ptr.astype(np.int64)
    inp = np.empty((3, len(kept)), dtype=object)
    comps = []
    for k, g in enumerate(kept):
        for r, t in enumerate((c.shell, c.self_idx, c.nbr_idx)):
            inp[r][k] = t[ptr[g]:ptr[g + 1]].astype(np.int64)
        comps.append([ELEMENT_SYMBOLS[e] for e in c.atom_elem[ptr[g]:ptr[g + 1]]])
    stored = c.targets[kept] / np.diff(ptr)[kept].astype(np.float64)
    return {"input": inp, "batch_ids": kept.tolist(), "batch_comp": [_formula(s) for s in comps],
            "target": {t: stored.copy() for t in TARGETS}, "comps": comps}


def pack_reference(c, target):
    """The rules of the module docstring in numpy: dict of the ten arrays plus kept, natoms, nuniq."""
    K = c.K
    kept = np.flatnonzero(c.status == 0)
    ptr = c.atom_ptr.astype(np.int64)
    rows, comp_elem, comp_weight = [], [], []
    atom_ptr, comp_ptr = np.zeros(len(kept) + 1, np.int64), np.zeros(len(kept) + 1, np.int64)
    y_val = np.zeros(len(kept), np.float32)
    for k, g in enumerate(kept):
        ids = c.atom_elem[ptr[g]:ptr[g + 1]]
        n = len(ids)
        first = np.sort(np.unique(ids, return_index=True)[1])               # positions that open an element, in order
        counts = np.array([(ids == ids[i]).sum() for i in first], np.float64)
        comp_elem.append(ids[first])
        comp_weight.append((counts / np.float64(n)).astype(np.float32))
        rows.append(np.arange(ptr[g], ptr[g + 1]))
        q = np.float32(np.float64(c.targets[g]) / np.float64(n))
        y_val[k] = q if target == "volume" else q * np.float32(n)
        atom_ptr[k + 1] = atom_ptr[k] + n
        comp_ptr[k + 1] = comp_ptr[k] + len(first)
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)
    table = np.asarray(list(embedding().values()), np.float64).astype(np.float32)
    return {"table": table, "atom_ptr": atom_ptr.astype(np.int32), "atom_elem": c.atom_elem[rows],
            "shell": np.ascontiguousarray(c.shell[rows, :K]), "self_idx": np.ascontiguousarray(c.self_idx[rows, :K]),
            "nbr_idx": np.ascontiguousarray(c.nbr_idx[rows, :K]), "comp_ptr": comp_ptr.astype(np.int32),
            "comp_elem": cat(comp_elem, np.int32), "comp_weight": cat(comp_weight, np.float32), "y_val": y_val,
            "kept": kept, "natoms": np.diff(atom_ptr), "nuniq": np.diff(comp_ptr)}
