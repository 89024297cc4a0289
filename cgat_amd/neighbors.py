"""Neighbour tables on the device: from raw structures -- lattice, fractional coordinates, species -- to the
three integer tables a `PackedDataset` is packed from, without pymatgen.

The reference builds them offline (CGAT/prepare_data.py:146-169: pymatgen's `get_all_neighbors(radius=18)`, a Python sort
and a Python loop per atom).  Here one HIP launch (csrc/neighbors.hip, one workgroup per atom, fp64 geometry) writes, per
atom row, the shell id, the centre index and the neighbour index of its `K` nearest periodic neighbours:

    tabs = neighbor_tables(lattice, frac_coords, atom_ptr, 24)          # device tensors in, device tensors out
    data, kept = dataset_dict_from_structures(structures, targets)      # the reference's dictionary (picklable)
    ds = PackedDataset.from_structures(structures, targets, embedding)  # the dictionary, packed

Definition: wrapped f_j = frac_j - floor(frac_j), r_j = f_j . L (L rows a, b, c); candidates of atom i are all (j, R in
Z^3) with 1e-8 < d = |r_j + R.L - r_i| <= radius; sorted by d; a candidate opens the next shell iff d exceeds the first
distance of the current shell by more than 1e-8; the row keeps the first K, the shell holding the K-th place taken in
ascending j, and is ordered by (shell, j).  A crystal in which some atom has fewer than K candidates is not built
(status 1, dropped with a warning like the reference); status 2 marks a crystal beyond the kernel's limits (more than
1024 atoms, see include/cgat_hip.h) and raises.
"""
import warnings

import numpy as np
import torch

from . import _lib
from .graph import ELEMENT_SYMBOLS

C = _lib.C
MAX_NEIGHBORS = 64


class NeighborTables:
    """shell / self_idx / nbr_idx int32 [N, K], status int32 [G]; dist fp64 [N, K] and passes int32 [N] when asked for."""
    __slots__ = ("shell", "self_idx", "nbr_idx", "status", "dist", "passes")

    def __init__(self, shell, self_idx, nbr_idx, status, dist=None, passes=None):
        self.shell, self.self_idx, self.nbr_idx, self.status, self.dist, self.passes = shell, self_idx, nbr_idx, status, dist, passes


def _validate(lattice, frac_coords, atom_ptr, K, radius):
    for name, t in (("lattice", lattice), ("frac_coords", frac_coords), ("atom_ptr", atom_ptr)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"neighbor_tables: {name} must be a torch tensor")
    if isinstance(K, bool) or int(K) != K or not 1 <= int(K) <= MAX_NEIGHBORS:
        raise ValueError(f"neighbor_tables: max_neighbor_number {K} outside 1..{MAX_NEIGHBORS}")
    if not (float(radius) > 0.0 and np.isfinite(float(radius))):
        raise ValueError("neighbor_tables: radius must be positive and finite")
    if lattice.dtype != torch.float64 or frac_coords.dtype != torch.float64:
        raise ValueError("neighbor_tables: lattice and frac_coords must be float64 (all geometry is fp64)")
    if atom_ptr.dtype != torch.int32:
        raise ValueError("neighbor_tables: atom_ptr must be int32")
    if lattice.dim() != 3 or tuple(lattice.shape[1:]) != (3, 3):
        raise ValueError(f"neighbor_tables: lattice must be [G, 3, 3], got {tuple(lattice.shape)}")
    if frac_coords.dim() != 2 or frac_coords.shape[1] != 3:
        raise ValueError(f"neighbor_tables: frac_coords must be [N, 3], got {tuple(frac_coords.shape)}")
    G, N = lattice.shape[0], frac_coords.shape[0]
    if atom_ptr.dim() != 1 or atom_ptr.shape[0] != G + 1:
        raise ValueError(f"neighbor_tables: atom_ptr must be [G + 1] = [{G + 1}], got {tuple(atom_ptr.shape)}")
    if N * int(K) >= 2 ** 31:
        raise ValueError("neighbor_tables: N * K needs 32-bit row offsets")
    if not (lattice.device == frac_coords.device == atom_ptr.device):
        raise ValueError("neighbor_tables: lattice, frac_coords and atom_ptr must live on one device")
    # value checks where the data lives (host data: before any upload; device data: one small read, this is preprocessing)
    ap = atom_ptr.to(torch.int64)
    if int(ap[0]) != 0 or int(ap[-1]) != N or bool((ap[1:] < ap[:-1]).any()):
        raise ValueError("neighbor_tables: atom_ptr must be non-decreasing from 0 to N")
    if G:
        a, b, c = lattice[:, 0], lattice[:, 1], lattice[:, 2]
        det = (a * torch.cross(b, c, dim=1)).sum(dim=1)
        bad = ~(det.abs() > 0) | ~torch.isfinite(det)
        if bool(bad.any()):
            raise ValueError(f"neighbor_tables: singular lattice (|det| <= 0) at crystal {int(bad.nonzero()[0])}")
    return G, N


def _run(lattice, frac_coords, atom_ptr, K, radius, return_distances, return_passes, cap=None, first_radius=0.0):
    G, N = _validate(lattice, frac_coords, atom_ptr, K, radius)
    if not lattice.is_cuda:
        raise RuntimeError("cgat_amd.neighbor_tables: the tables are built by a HIP kernel on an MI355X device (cuda:N); "
                           "there is no CPU fallback")
    K, dev = int(K), lattice.device
    lattice, frac_coords, atom_ptr = lattice.contiguous(), frac_coords.contiguous(), atom_ptr.contiguous()
    i32 = dict(dtype=torch.int32, device=dev)
    shell, self_idx, nbr_idx = (torch.empty(N, K, **i32) for _ in range(3))
    status = torch.empty(G, **i32)
    dist = torch.empty(N, K, dtype=torch.float64, device=dev) if return_distances else None
    passes = torch.empty(N, **i32) if return_passes else None
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        outs = (ptr(shell), ptr(self_idx), ptr(nbr_idx), ptr(dist), ptr(status), ptr(passes), stream)
        if cap is None:
            rc = _lib.lib.cgat_neighbor_tables(lattice.data_ptr(), frac_coords.data_ptr(), atom_ptr.data_ptr(), G, N, K,
                                               float(radius), *outs)
        else:
            rc = _lib.lib.cgat_debug_neighbor_tables(lattice.data_ptr(), frac_coords.data_ptr(), atom_ptr.data_ptr(), G, N, K,
                                                     float(radius), int(cap), float(first_radius), *outs)
        _lib.check(rc, "cgat_neighbor_tables")
    return NeighborTables(shell, self_idx, nbr_idx, status, dist, passes)


def neighbor_tables(lattice, frac_coords, atom_ptr, max_neighbor_number=24, radius=18.0, return_distances=False,
                    return_passes=False):
    """lattice [G, 3, 3] fp64 (rows a, b, c, in Angstrom), frac_coords [N, 3] fp64, atom_ptr [G + 1] int32, all on the
    device.  Returns a `NeighborTables`.  Crystals with status 1 (too few neighbours within `radius`) have zero rows and
    are the caller's to drop; a crystal beyond the kernel's limits (status 2) raises."""
    res = _run(lattice, frac_coords, atom_ptr, max_neighbor_number, radius, return_distances, return_passes)
    st = res.status.cpu()
    if bool((st == 2).any()):
        which = (st == 2).nonzero().flatten().tolist()
        raise RuntimeError(f"neighbor_tables: crystals {which[:8]}{'...' if len(which) > 8 else ''} are beyond the kernel's "
                           "limits (more than 1024 atoms per crystal, or a cell too thin for the search; include/cgat_hip.h)")
    return res


# ------------------------------------------------------------------------------------------------------------------
# structures -> dataset dictionary / PackedDataset
# ------------------------------------------------------------------------------------------------------------------
def _as_structure(s):
    """(lattice 3x3, frac n x 3, symbols) from a tuple or from an object of pymatgen's shape (duck-typed)."""
    if hasattr(s, "lattice") and hasattr(s, "frac_coords"):
        lat, frac = s.lattice.matrix, s.frac_coords
        syms = [site.specie.symbol for site in s]
    else:
        lat, frac, syms = s
    lat = np.asarray(lat, dtype=np.float64)
    frac = np.asarray(frac, dtype=np.float64).reshape(-1, 3)
    syms = [str(x) for x in syms]
    if lat.shape != (3, 3):
        raise ValueError(f"structure lattice must be 3x3, got {lat.shape}")
    if len(syms) != frac.shape[0]:
        raise ValueError(f"structure with {frac.shape[0]} coordinates but {len(syms)} species")
    if frac.shape[0] == 0:
        raise ValueError("structure without atoms")
    return lat, frac, syms


def _tables_from_structures(structures, K, radius, device):
    parsed = [_as_structure(s) for s in structures]
    G = len(parsed)
    lat = np.stack([p[0] for p in parsed]) if G else np.zeros((0, 3, 3))
    det = np.linalg.det(lat) if G else np.zeros(0)
    if G and not np.all(np.abs(det) > 0):
        raise ValueError(f"singular lattice (|det| <= 0) at structure {int(np.flatnonzero(~(np.abs(det) > 0))[0])}")
    natoms = np.array([p[1].shape[0] for p in parsed], np.int64)
    atom_ptr = np.zeros(G + 1, np.int64)
    atom_ptr[1:] = np.cumsum(natoms)
    if atom_ptr[-1] * max(int(K), 1) >= 2 ** 31:
        raise ValueError("dataset too large for int32 offsets")
    frac = np.concatenate([p[1] for p in parsed]) if G else np.zeros((0, 3))
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    res = neighbor_tables(up(lat), up(frac), up(atom_ptr.astype(np.int32)), K, radius)
    return parsed, atom_ptr, res


def _warn_dropped(ids, status):
    for g in np.flatnonzero(status != 0):
        warnings.warn(f"{ids[g]} does not contain enough neighbors in the cutoff to build the full graph. If it happens "
                      "frequently, consider increase radius. Compound is not added to the feature set")


def _formula(syms):
    return "".join(f"{el}{syms.count(el)}" for el in dict.fromkeys(syms))


def dataset_dict_from_structures(structures, targets, max_neighbor_number=24, radius=18.0, ids=None, device="cuda:0"):
    """The reference's dataset dictionary (prepare_data.py:92-98) for `structures`: a sequence of (lattice 3x3,
    frac_coords n x 3, species symbols) or of objects exposing `.lattice.matrix`, `.frac_coords` and per-site
    `.specie.symbol`.  `targets`: name -> per-cell values, stored divided by the atom count (prepare_data.py:139).
    Returns (data, kept): `data` holds the built crystals only, `kept` their indices into `structures`; a crystal with
    too few neighbours within `radius` is dropped with a warning, as the reference does."""
    structures = list(structures)
    K = int(max_neighbor_number)
    ids = list(range(len(structures))) if ids is None else list(ids)
    if len(ids) != len(structures):
        raise ValueError("ids and structures differ in length")
    for name, v in targets.items():
        if len(v) != len(structures):
            raise ValueError(f"target {name!r} has {len(v)} values for {len(structures)} structures")
    parsed, atom_ptr, res = _tables_from_structures(structures, K, radius, device)
    status = res.status.cpu().numpy()
    _warn_dropped(ids, status)
    kept = np.flatnonzero(status == 0)
    tabs = [t.cpu().numpy().astype(np.int64) for t in (res.shell, res.self_idx, res.nbr_idx)]
    inp = np.empty((3, len(kept)), dtype=object)
    for k, g in enumerate(kept):
        for r in range(3):
            inp[r][k] = tabs[r][atom_ptr[g]:atom_ptr[g + 1]]
    natoms = np.diff(atom_ptr)[kept].astype(np.float64)
    data = {"input": inp,
            "batch_ids": [ids[g] for g in kept],
            "batch_comp": [_formula(parsed[g][2]) for g in kept],
            "target": {name: np.asarray(v, dtype=np.float64)[kept] / natoms for name, v in targets.items()},
            "comps": [list(parsed[g][2]) for g in kept]}
    return data, kept


def synthetic_structures(num, seed, atoms=(1, 40)):
    """`num` seeded random cells as (lattice, frac_coords, symbols): perturbed orthorhombic cells at about 14 A^3 per
    atom, fractional coordinates in (-1, 2) (unwrapped on purpose), 1-4 species from the element table."""
    rs = np.random.RandomState(seed)
    lo, hi = (atoms, atoms) if isinstance(atoms, int) else atoms
    out = []
    for _ in range(int(num)):
        n = int(rs.randint(lo, hi + 1))
        edge = np.maximum(np.cbrt(14.0 * n) * rs.uniform(0.8, 1.25, size=3), 2.5)
        lat = np.diag(edge) + np.cbrt(14.0 * n) * rs.uniform(-0.15, 0.15, size=(3, 3)) * (1 - np.eye(3))
        frac = rs.uniform(-1.0, 2.0, size=(n, 3))
        pool = rs.randint(0, len(ELEMENT_SYMBOLS), size=int(rs.randint(1, 5)))
        syms = [ELEMENT_SYMBOLS[pool[k]] for k in rs.randint(0, len(pool), size=n)]
        out.append((lat, frac, syms))
    return out
