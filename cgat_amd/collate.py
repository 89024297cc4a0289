"""Device-side batch collation: the step right before the hot path.

The reference assembles every batch on the host with per-crystal Python loops
(`CompositionData.__getitem__`, CGAT/data.py:61-144; PyG `Batch.from_data_list`, CGAT/lightning_module.py:200;
`collate_batch`, CGAT/roost_message.py:400-458) and ships it to the GPU each step.  Here the dataset dictionary is
packed ONCE into int32 arrays that live in HBM (`PackedDataset`), and a batch is a list of crystal ids:
`PackedDataset.collate(ids)` launches one HIP kernel (csrc/collate.hip) that writes the tensors of the collated batch
-- same values, shapes and dtypes as the reference's -- directly on the device.  Per batch the host only computes
three prefix sums over the batch's crystals and uploads them with the ids (a few KB).

The element parsing rules of `__getitem__` (string formulas via batch_comp, per-atom tuples, ndarray inputs) are
applied at pack time; they are host logic and mirror data.py:62-80.

Packing itself has two routes to the same arrays: `from_dict` walks the reference's dictionary on the host, crystal by
crystal; `from_tables` / `from_arrays` / `from_structures(pack="device")` pack flat arrays and finished neighbour tables on
the device (csrc/pack.hip: a plan that counts and scans, one 16-byte readback, a write), with no per-crystal host code.
"""
import json
import re

import numpy as np
import torch

from . import _lib
from .graph import GraphBatch

C = _lib.C


def _element_list(data, idx):
    elements = data["comps"][idx]
    if isinstance(elements, str):
        pattern = re.compile(r"([a-z]+)(\d+)", re.IGNORECASE)
        try:
            matches = pattern.findall(data["batch_comp"][idx])
        except TypeError:
            matches = pattern.findall(data["batch_comp"][idx][0])
        elements = []
        for el, count in matches:
            elements += [el] * int(count)
    if hasattr(elements, "tolist"):
        elements = elements.tolist()
    if isinstance(elements[0], (list, tuple)):
        elements = [el[0] for el in elements]
    return list(elements)


def _embedding_table(embedding):
    """(symbols, fp32 table [n_elem, fea]) of an embedding JSON path or dict, rounded as `from_dict` rounds it."""
    if isinstance(embedding, tuple):
        return embedding
    if isinstance(embedding, str):
        with open(embedding) as f:
            embedding = json.load(f)
    symbols = list(embedding.keys())
    return symbols, np.asarray([embedding[el] for el in symbols], dtype=np.float64).astype(np.float32)


def _symbol_rows(species, symbols):
    """Rows of the embedding table for a flat sequence of element symbols: one `np.unique` over the atoms and one lookup
    per distinct symbol.  An unknown symbol raises what `from_dict` raises for the first such atom."""
    species = np.asarray(species, dtype=str).reshape(-1)
    uniq, first, inverse = np.unique(species, return_index=True, return_inverse=True)
    elem_id = {el: k for k, el in enumerate(symbols)}
    unknown = [(i, el) for i, el in zip(first, uniq) if el not in elem_id]
    if unknown:
        raise AssertionError(f"{min(unknown)[1]} is not an allowed atom type")     # Featuriser.get_fea
    rows = np.array([elem_id[el] for el in uniq], np.int32)
    return rows[inverse.reshape(-1)] if species.size else np.zeros(0, np.int32)


def _split_tables(tables):
    if hasattr(tables, "shell"):
        return tables.shell, tables.self_idx, tables.nbr_idx, tables.status
    tables = tuple(tables)
    if len(tables) not in (3, 4):
        raise ValueError("from_tables: tables is a NeighborTables or (shell, self_idx, nbr_idx[, status])")
    return tables + (None,) * (4 - len(tables))


def _to_device(a, dtype, dev, name, check_ptr=None):
    """numpy array, sequence or tensor -> contiguous tensor of `dtype` on `dev`; a host-resident atom_ptr is checked
    against `check_ptr` atoms where it lies (a device-resident one is checked by the kernel)."""
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
    if check_ptr is not None and not a.is_cuda:
        p = a.to(torch.int64)
        if p.dim() != 1 or p.numel() < 1 or int(p[0]) != 0 or int(p[-1]) != check_ptr or bool((p[1:] < p[:-1]).any()):
            raise ValueError(f"{name} must be non-decreasing from 0 to N")
    if a.dim() < 1 or (name == "atom_ptr" and (a.dim() != 1 or a.numel() < 1)):
        raise ValueError(f"{name} must be a 1-d array of G + 1 offsets" if name == "atom_ptr" else f"{name} must be an array")
    return a.to(device=dev, dtype=dtype).contiguous()


def _dropped(G, kept):
    status = np.ones(G, np.int32)
    status[kept] = 0
    return status


class PackedDataset:
    """Packed, device-resident form of the reference's dataset dictionary
    (`{'input', 'comps', 'batch_comp', 'target'}`, either `input` layout of data.py:47-50)."""

    def __init__(self, arrays, host, device):
        self.t, self.host, self.device = arrays, host, device
        s = _lib.PackedDatasetStruct()
        s.n_graphs, s.fea, s.max_nbr, s.n_elem = host["n_graphs"], host["fea"], host["max_nbr"], host["n_elem"]
        for k in ("table", "atom_ptr", "atom_elem", "shell", "self_idx", "nbr_idx", "comp_ptr", "comp_elem",
                  "comp_weight", "y_val"):
            setattr(s, k, arrays[k].data_ptr())
        self.c = s

    @classmethod
    def from_dict(cls, data, embedding, max_neighbor_number=12, target="e_above_hull", device="cuda:0"):
        """`embedding`: path of the element-embedding JSON (reference `fea_path`) or a dict symbol -> vector."""
        if isinstance(embedding, str):
            with open(embedding) as f:
                embedding = json.load(f)
        symbols = list(embedding.keys())
        elem_id = {el: k for k, el in enumerate(symbols)}
        table = np.asarray([embedding[el] for el in symbols], dtype=np.float64).astype(np.float32)
        fmt = 1 if data["input"].shape[0] > 3 else 0
        G = len(data["target"][target])
        K = int(max_neighbor_number)
        atom_ptr, comp_ptr = np.zeros(G + 1, np.int64), np.zeros(G + 1, np.int64)
        atom_elem, shell, self_idx, nbr_idx, comp_elem, comp_weight = [], [], [], [], [], []
        y_val = np.zeros(G, np.float32)
        for g in range(G):
            elements = _element_list(data, g)
            n = len(elements)
            for el in elements:
                if el not in elem_id:
                    raise AssertionError(f"{el} is not an allowed atom type")     # Featuriser.get_fea
            counts = {}
            for el in elements:
                counts[el] = counts.get(el, 0) + 1
            atom_elem.append(np.array([elem_id[el] for el in elements], np.int32))
            comp_elem.append(np.array([elem_id[el] for el in counts], np.int32))
            comp_weight.append(np.array([v / n for v in counts.values()], np.float32))
            tabs = (data["input"][0][g], data["input"][1][g], data["input"][2][g]) if fmt == 0 else \
                   (data["input"][g][0], data["input"][g][1], data["input"][g][2])
            sh, se, nb = (np.asarray(t)[:, 0:K].astype(np.int64) for t in tabs)
            if sh.shape[0] != n:
                raise ValueError(f"crystal {g}: {n} elements but {sh.shape[0]} rows of neighbours")
            if sh.shape[1] != K:
                raise ValueError(f"crystal {g}: {sh.shape[1]} stored neighbours < max_neighbor_number {K}")
            shell.append(sh.astype(np.int32)); self_idx.append(se.astype(np.int32)); nbr_idx.append(nb.astype(np.int32))
            t = np.float32(data["target"][target][g])
            y_val[g] = t * np.float32(n) if target != "volume" else t
            atom_ptr[g + 1] = atom_ptr[g] + n
            comp_ptr[g + 1] = comp_ptr[g] + len(counts)
        if atom_ptr[-1] * max(K, 1) >= 2 ** 31:
            raise ValueError("dataset too large for int32 offsets")
        cat = lambda xs, dt, shape: (np.concatenate(xs).astype(dt) if xs else np.zeros(shape, dt))
        arrays = {"table": table, "atom_ptr": atom_ptr.astype(np.int32), "atom_elem": cat(atom_elem, np.int32, (0,)),
                  "shell": cat(shell, np.int32, (0, K)), "self_idx": cat(self_idx, np.int32, (0, K)),
                  "nbr_idx": cat(nbr_idx, np.int32, (0, K)), "comp_ptr": comp_ptr.astype(np.int32),
                  "comp_elem": cat(comp_elem, np.int32, (0,)), "comp_weight": cat(comp_weight, np.float32, (0,)),
                  "y_val": y_val}
        host = {"n_graphs": G, "fea": table.shape[1], "max_nbr": K, "n_elem": table.shape[0],
                "natoms": np.diff(atom_ptr), "nuniq": np.diff(comp_ptr)}
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in arrays.items()}
        return cls(dev, host, torch.device(device))

    @classmethod
    def from_structures(cls, structures, targets, embedding, max_neighbor_number=12, stored_neighbors=24,
                        target="e_above_hull", radius=18.0, device="cuda:0", pack="host"):
        """From raw structures -- (lattice 3x3, frac_coords n x 3, species symbols) tuples or objects of pymatgen's shape
        -- without the reference's offline stage (prepare_data.py:146-169): the neighbour tables are built on the device
        (csrc/neighbors.hip) with `stored_neighbors` columns, sliced to `max_neighbor_number` and packed.  Equal to
        `from_dict(neighbors.dataset_dict_from_structures(...)[0], ...)`; crystals with too few neighbours within `radius`
        are dropped with a warning, `kept` holds the indices of the others into `structures`.  `pack="host"` goes through
        that dictionary and `from_dict`'s loop; `pack="device"` hands the tables to `from_tables` where they lie (same
        arrays, bit for bit)."""
        if pack not in ("host", "device"):
            raise ValueError(f"from_structures: pack must be 'host' or 'device', got {pack!r}")
        if pack == "device":
            from .neighbors import _tables_from_structures, _warn_dropped
            structures = list(structures)
            if len(targets[target]) != len(structures):
                raise ValueError(f"target {target!r} has {len(targets[target])} values for {len(structures)} structures")
            symbols, table = _embedding_table(embedding)
            parsed, atom_ptr, res = _tables_from_structures(structures, stored_neighbors, radius, device)
            elem = torch.from_numpy(_symbol_rows([el for p in parsed for el in p[2]], symbols)).to(device)
            ds = cls.from_tables(res, atom_ptr, elem, (symbols, table), targets, target, max_neighbor_number, device)
            _warn_dropped(list(range(len(structures))), _dropped(len(structures), ds.kept))
            return ds
        from .neighbors import dataset_dict_from_structures
        data, kept = dataset_dict_from_structures(structures, {target: targets[target]}, stored_neighbors, radius,
                                                  device=device)
        ds = cls.from_dict(data, embedding, max_neighbor_number, target, device)
        ds.kept = kept
        return ds

    @classmethod
    def from_tables(cls, tables, atom_ptr, atom_elem, embedding, targets=None, target="e_above_hull",
                    max_neighbor_number=12, device="cuda:0"):
        """From finished neighbour tables to the packed dataset without leaving the device (csrc/pack.hip): what
        `from_dict` builds from the dictionary of the same crystals, bit for bit, with no per-crystal host code.
        `tables`: a `NeighborTables` or a (shell, self_idx, nbr_idx[, status]) tuple of device int32 tensors [N, Ks];
        crystals whose status is not 0 are left out, `kept` holds the indices of the others.  `atom_ptr` [G + 1]; `atom_elem`
        [N] int32 rows of the embedding table; `targets[target]` [G] per-cell values (None: y = 0).  The host reads the
        four totals once, allocates, and after the write reads back the two pointer arrays and `kept`."""
        shell, self_idx, nbr_idx, status = _split_tables(tables)
        tensors = [t for t in (shell, self_idx, nbr_idx, status, atom_elem) if t is not None]
        dev = torch.device(device)
        if dev.type != "cuda" or not all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors):
            raise RuntimeError("PackedDataset.from_tables packs with a HIP kernel on device-resident tables (cuda:N); "
                               "there is no CPU path")
        symbols, table = _embedding_table(embedding)
        K, n_elem = int(max_neighbor_number), table.shape[0]
        if any(t.dtype != torch.int32 for t in tensors):
            raise ValueError("from_tables: tables, status and atom_elem must be int32")
        if shell.dim() != 2 or self_idx.shape != shell.shape or nbr_idx.shape != shell.shape:
            raise ValueError("from_tables: shell, self_idx and nbr_idx must share one [N, Ks] shape")
        N, Ks = shell.shape
        if not 1 <= K <= Ks:
            raise ValueError(f"from_tables: {Ks} stored neighbours < max_neighbor_number {K} (or it is < 1)")
        if N * Ks >= 2 ** 31:
            raise ValueError("dataset too large for int32 offsets")
        atom_ptr = _to_device(atom_ptr, torch.int32, dev, "atom_ptr", check_ptr=N)
        G = atom_ptr.shape[0] - 1
        if atom_elem.shape != (N,) or (status is not None and status.shape != (G,)):
            raise ValueError(f"from_tables: atom_elem must be [{N}] and status [{G}]")
        tgt = None
        if targets is not None:
            tgt = _to_device(targets[target], torch.float64, dev, f"target {target!r}")
            if tgt.shape != (G,):
                raise ValueError(f"target {target!r} has {tgt.numel()} values for {G} structures")
        shell, self_idx, nbr_idx, atom_elem = (t.contiguous() for t in (shell, self_idx, nbr_idx, atom_elem))
        status = None if status is None else status.contiguous()
        ptr = lambda t: None if t is None else t.data_ptr()
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            ws = torch.empty(_lib.lib.cgat_pack_dataset_workspace_bytes(G, N), dtype=torch.uint8, device=dev)
            totals = torch.empty(4, **i32)
            _lib.check(_lib.lib.cgat_pack_dataset_plan(atom_ptr.data_ptr(), ptr(atom_elem), ptr(status), G, N, n_elem,
                                                       totals.data_ptr(), ws.data_ptr(), ws.numel(), stream),
                       "cgat_pack_dataset_plan")
            Gk, Nk, Uk, bad = totals.cpu().tolist()                  # the one read between the two calls
            if bad:
                raise ValueError(f"from_tables: {bad} element ids outside [0, {n_elem}) (or atom_ptr ranges outside [0, N])")
            if Nk * max(K, 1) >= 2 ** 31:
                raise ValueError("dataset too large for int32 offsets")
            ptrs = torch.empty(3 * Gk + 2, **i32)                    # atom_ptr', comp_ptr', kept: one copy back
            arrays = {"table": torch.from_numpy(table).to(dev), "atom_ptr": ptrs[:Gk + 1],
                      "atom_elem": torch.empty(Nk, **i32), "shell": torch.empty(Nk, K, **i32),
                      "self_idx": torch.empty(Nk, K, **i32), "nbr_idx": torch.empty(Nk, K, **i32),
                      "comp_ptr": ptrs[Gk + 1:2 * Gk + 2], "comp_elem": torch.empty(Uk, **i32),
                      "comp_weight": torch.empty(Uk, **f32), "y_val": torch.empty(Gk, **f32)}
            kept = ptrs[2 * Gk + 2:]
            outs = [arrays[k] for k in ("atom_ptr", "atom_elem", "shell", "self_idx", "nbr_idx", "comp_ptr", "comp_elem",
                                        "comp_weight", "y_val")] + [kept]
            _lib.check(_lib.lib.cgat_pack_dataset_write(atom_ptr.data_ptr(), ptr(atom_elem), ptr(shell), ptr(self_idx),
                                                        ptr(nbr_idx), ptr(status), ptr(tgt), G, N, Ks, K, n_elem,
                                                        1 if target == "volume" else 0, totals.data_ptr(), ws.data_ptr(),
                                                        ws.numel(), Gk, Nk, Uk, *[ptr(t) for t in outs], stream),
                       "cgat_pack_dataset_write")
            back = ptrs.cpu().numpy().astype(np.int64)
        host = {"n_graphs": Gk, "fea": table.shape[1], "max_nbr": K, "n_elem": n_elem,
                "natoms": np.diff(back[:Gk + 1]), "nuniq": np.diff(back[Gk + 1:2 * Gk + 2])}
        ds = cls(arrays, host, dev)
        ds.kept = back[2 * Gk + 2:]
        return ds

    @classmethod
    def from_arrays(cls, lattice, frac_coords, atom_ptr, species, targets, embedding, max_neighbor_number=12,
                    stored_neighbors=24, target="e_above_hull", radius=18.0, ids=None, device="cuda:0"):
        """From flat structure arrays -- lattice [G, 3, 3], frac_coords [N, 3], atom_ptr [G + 1], one species per atom --
        to the packed dataset: `neighbor_tables`, then `from_tables`; no per-crystal host code.  Arrays are numpy arrays
        or tensors (device tensors are used where they lie).  `species`: integer rows of the embedding table, or a flat
        sequence of symbols, mapped to rows on the host in one step.  Crystals with too few neighbours within `radius` are
        dropped with the warning `dataset_dict_from_structures` gives (`ids` names them), `kept` holds the others."""
        from .neighbors import neighbor_tables, _warn_dropped
        symbols, table = _embedding_table(embedding)
        dev = torch.device(device)
        if not isinstance(species, torch.Tensor):
            species = np.asarray(species)
            if species.dtype.kind not in "iu":
                species = _symbol_rows(species, symbols)
        elif species.dtype.is_floating_point:
            raise ValueError("from_arrays: species as a tensor holds integer rows of the embedding table")
        elem = _to_device(species, torch.int32, dev, "species")
        lattice = _to_device(lattice, torch.float64, dev, "lattice")
        frac_coords = _to_device(frac_coords, torch.float64, dev, "frac_coords")
        atom_ptr = _to_device(atom_ptr, torch.int32, dev, "atom_ptr")
        G = atom_ptr.shape[0] - 1
        ids = list(range(G)) if ids is None else list(ids)
        if len(ids) != G:
            raise ValueError("ids and structures differ in length")
        if len(targets[target]) != G:
            raise ValueError(f"target {target!r} has {len(targets[target])} values for {G} structures")
        res = neighbor_tables(lattice, frac_coords, atom_ptr, stored_neighbors, radius)
        ds = cls.from_tables(res, atom_ptr, elem, (symbols, table), targets, target, max_neighbor_number, dev)
        _warn_dropped(ids, _dropped(G, ds.kept))
        return ds

    def __len__(self):
        return self.host["n_graphs"]

    def collate(self, ids):
        """Returns (GraphBatch, roost_tuple) for the crystals `ids` (sequence of ints, in batch order): the
        tensors `Batch.from_data_list(...)` / `collate_batch(...)` produce in the reference, already on the device."""
        if self.device.type != "cuda":
            raise RuntimeError("PackedDataset.collate needs the HIP library and a GPU-resident dataset; there is no CPU path")
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if ids.size and (ids.min() < 0 or ids.max() >= len(self)):
            raise IndexError("crystal id out of range")
        B = ids.size
        na, nu = self.host["natoms"][ids], self.host["nuniq"][ids]
        meta = np.zeros((4, B + 1), np.int32)
        meta[0, :B] = ids
        meta[1, 1:] = np.cumsum(na); meta[2, 1:] = np.cumsum(nu); meta[3, 1:] = np.cumsum(nu * (nu - 1))
        N, Nc, Ec = int(meta[1, B]), int(meta[2, B]), int(meta[3, B])
        K, F, dev = self.host["max_nbr"], self.host["fea"], self.device
        E = N * K
        # pinned staging: a pageable source makes the upload a synchronous copy -- the one host sync per training step that
        # round 4's bench line still showed
        m = torch.from_numpy(meta).pin_memory().to(dev, non_blocking=True)
        f32, i64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int64, device=dev)
        x, ei, ea = torch.empty(N, F, **f32), torch.empty(2, E, **i64), torch.empty(E, **i64)
        y, batch = torch.empty(B, **f32), torch.empty(N, **i64)
        cw, cf = torch.empty(Nc, 1, **f32), torch.empty(Nc, F, **f32)
        cs, cn, cc = torch.empty(Ec, **i64), torch.empty(Ec, **i64), torch.empty(Nc, **i64)
        out = _lib.CollatedStruct(*[t.data_ptr() for t in (x, ei, ea, y, batch, cw, cf, cs, cn, cc)])
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.cgat_collate_batch(C.byref(self.c), m[0].data_ptr(), m[1].data_ptr(), m[2].data_ptr(),
                                                   m[3].data_ptr(), B, E, Ec, C.byref(out),
                                                   torch.cuda.current_stream().cuda_stream), "cgat_collate_batch")
        return GraphBatch(x, ei, ea, batch, y, B), (cw, cf, cs, cn, cc)
