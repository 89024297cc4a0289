"""Device-side dataset packing on the MI355X (csrc/pack.hip): `PackedDataset.from_tables` against `from_dict` on the
dictionary of the same crystals, bit for bit, on every case of tests/pack_cases.py; then structures to batches through all
four builds.  The scan tile of the implementation is 1024 crystals (PACK_SCAN_TILE; test_pack_cpu.py holds the case table
to it): `many` has 20 000 >= 4 x 1024."""
import functools
import warnings

import numpy as np
import pytest
import torch

import pack_cases as PC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _device_case(name):
    c = PC.case(name)
    up = lambda a: torch.from_numpy(a).to(DEV)
    return (up(c.shell), up(c.self_idx), up(c.nbr_idx), up(c.status)), up(c.atom_ptr), up(c.atom_elem)


def _from_tables(name, target):
    import cgat_amd as P
    c = PC.case(name)
    tabs, ptr, elem = _device_case(name)
    return P.PackedDataset.from_tables(tabs, ptr, elem, PC.embedding(), {t: c.targets for t in PC.TARGETS}, target,
                                       max_neighbor_number=c.K, device=DEV)


def _assert_same(a, b):
    for k in PC.ARRAYS:
        assert a.t[k].dtype == b.t[k].dtype and a.t[k].shape == b.t[k].shape, k
        assert torch.equal(a.t[k], b.t[k]), k
    assert len(a) == len(b)
    for k in ("natoms", "nuniq"):
        assert a.host[k].dtype == b.host[k].dtype and np.array_equal(a.host[k], b.host[k]), k


@pytest.mark.parametrize("target", PC.TARGETS)
@pytest.mark.parametrize("name", PC.NAMES)
def test_from_tables_equals_from_dict(name, target):
    import cgat_amd as P
    c = PC.case(name)
    want = P.PackedDataset.from_dict(PC.dictionary(name), PC.embedding(), c.K, target, device=DEV)
    got, again = _from_tables(name, target), _from_tables(name, target)
    _assert_same(got, want)
    _assert_same(again, got)                                             # two calls, identical bits
    assert isinstance(got.kept, np.ndarray) and got.kept.tolist() == np.flatnonzero(c.status == 0).tolist()
    assert _bits(got) == _bits(want)


def _bits(ds):
    return ds.t["y_val"].view(torch.int32).tolist() + ds.t["comp_weight"].view(torch.int32).tolist()


def test_tuple_without_status_and_without_targets():
    import cgat_amd as P
    c = PC.case("tiny")
    tabs, ptr, elem = _device_case("tiny")
    ds = P.PackedDataset.from_tables(tabs[:3], c.atom_ptr, elem, PC.embedding(), max_neighbor_number=2, device=DEV)
    assert len(ds) == 5 and ds.kept.tolist() == [0, 1, 2, 3, 4] and not ds.t["y_val"].any()
    assert torch.equal(ds.t["shell"], tabs[0][:, :2]) and torch.equal(ds.t["atom_elem"], elem)
    g, _ = ds.collate([4, 2])
    assert g.x.shape == (8, 200) and g.edge_index.shape == (2, 16)


@pytest.mark.parametrize("bad", [-1, 103])
def test_out_of_range_element_ids(bad):
    import cgat_amd as P
    c = PC.case("drops")
    tabs, ptr, elem = _device_case("drops")
    elem = elem.clone()
    elem[-1] = bad                                                       # in the last crystal, which is dropped: still refused
    with pytest.raises(ValueError, match="element ids outside"):
        P.PackedDataset.from_tables(tabs, ptr, elem, PC.embedding(), {"e_above_hull": c.targets}, max_neighbor_number=c.K,
                                    device=DEV)


def test_device_atom_ptr_out_of_range_is_refused_not_followed():
    import cgat_amd as P
    c = PC.case("tiny")
    tabs, ptr, elem = _device_case("tiny")
    ptr = ptr.clone()
    ptr[2] = 10 ** 6
    with pytest.raises(ValueError, match="atom_ptr"):
        P.PackedDataset.from_tables(tabs, ptr, elem, PC.embedding(), {"e_above_hull": c.targets}, max_neighbor_number=c.K,
                                    device=DEV)
    with pytest.raises(ValueError, match="non-decreasing"):
        P.PackedDataset.from_tables(tabs, ptr.cpu().numpy(), elem, PC.embedding(), max_neighbor_number=c.K, device=DEV)


def test_no_fall_back_to_the_host_loop(monkeypatch):
    import cgat_amd as P

    def refuse(*a, **k):
        raise AssertionError("from_dict called on the device route")
    want = PC.pack_reference(PC.case("many"), "e_above_hull")
    monkeypatch.setattr(P.PackedDataset, "from_dict", classmethod(refuse))
    ds = _from_tables("many", "e_above_hull")
    assert len(ds) == len(want["kept"]) and np.array_equal(ds.kept, want["kept"])
    assert np.array_equal(ds.t["comp_elem"].cpu().numpy(), want["comp_elem"])


# ---------------------------------------------------------------------------------------------------------------
# end to end on real geometry: four builds of one dataset
# ---------------------------------------------------------------------------------------------------------------
def _structures():
    import cgat_amd as P
    s = P.synthetic_structures(6, 4, (2, 12))
    lone = (np.eye(3) * 15.0, np.zeros((1, 3)), ["Fe"])          # 6 neighbours within 18 A: dropped at 24
    return s[:2] + [lone] + s[2:]


@pytest.mark.parametrize("target", PC.TARGETS)
def test_four_builds_agree(target):
    import cgat_amd as P
    from cgat_amd.graph import ELEMENT_SYMBOLS
    structures, emb = _structures(), PC.embedding()
    G = len(structures)
    targets = {"e_above_hull": np.linspace(-1.0, 2.0, G), "volume": np.linspace(10.0, 90.0, G)}
    lat = np.stack([s[0] for s in structures])
    frac = np.concatenate([s[1] for s in structures])
    ptr = np.zeros(G + 1, np.int32)
    ptr[1:] = np.cumsum([len(s[2]) for s in structures])
    syms = [el for s in structures for el in s[2]]
    rows = np.array([ELEMENT_SYMBOLS.index(el) for el in syms], np.int32)
    up = lambda a: torch.from_numpy(a).to(DEV)
    kw = dict(max_neighbor_number=12, stored_neighbors=24, target=target, device=DEV)
    builds = [lambda: P.PackedDataset.from_structures(structures, targets, emb, **kw),
              lambda: P.PackedDataset.from_structures(structures, targets, emb, pack="device", **kw),
              lambda: P.PackedDataset.from_arrays(lat, frac, ptr, syms, targets, emb, **kw),
              lambda: P.PackedDataset.from_arrays(up(lat), up(frac), up(ptr), up(rows),
                                                  {t: up(v) for t, v in targets.items()}, emb, **kw)]
    sets = []
    for build in builds:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            sets.append(build())
        msgs = [str(x.message) for x in w if "enough neighbors" in str(x.message)]
        assert len(msgs) == 1 and msgs[0].startswith("2 does not contain enough neighbors in the cutoff")
    ids = [5, 0, 3, 3, 1]
    g0, r0 = sets[0].collate(ids)
    for ds in sets:
        assert isinstance(ds.kept, np.ndarray) and ds.kept.tolist() == [0, 1, 3, 4, 5, 6]
        _assert_same(ds, sets[0])
        g, r = ds.collate(ids)
        for x, y in zip((g.x, g.edge_index, g.edge_attr, g.y, g.batch) + tuple(r),
                        (g0.x, g0.edge_index, g0.edge_attr, g0.y, g0.batch) + tuple(r0)):
            assert x.dtype == y.dtype and torch.equal(x, y)
