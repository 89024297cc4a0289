"""Neighbour tables built on the device (csrc/neighbors.hip) against the numpy fp64 restatement of the
definition (tests/neighbor_cases.py): shell, self_idx, nbr_idx and status EQUAL (the CPU tests check the input condition
that makes them comparable exactly), dist within 2e-8 (the width of a shell)."""
import pickle
import types
import warnings

import numpy as np
import pytest
import torch

import neighbor_cases as NC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _inputs(name):
    return tuple(torch.from_numpy(a).to(DEV) for a in NC.flat(NC.batch(name)))


def _build(name, K, radius=18.0, cap=None, first_radius=0.0):
    import cgat_amd as P
    lat, frac, ptr = _inputs(name)
    if cap is None:
        return P.neighbor_tables(lat, frac, ptr, K, radius, return_distances=True, return_passes=True)
    return P.debug.neighbor_tables_with(lat, frac, ptr, K, radius, cap, first_radius)


def _check(res, name, K, radius=18.0):
    ref = NC.reference(name, K, radius)
    ptr = NC.flat(NC.batch(name))[2]
    got = [t.cpu().numpy() for t in (res.shell, res.self_idx, res.nbr_idx, res.dist)]
    assert res.status.cpu().tolist() == [r[0] for r in ref]
    for g, r in enumerate(ref):
        a0, a1 = ptr[g], ptr[g + 1]
        for k, what in enumerate(("shell", "self_idx", "nbr_idx")):
            assert got[k].dtype == np.int32 and np.array_equal(got[k][a0:a1], r[1 + k]), (name, K, g, what)
        assert np.abs(got[3][a0:a1] - r[4]).max() <= 2e-8, (name, K, g)


@pytest.mark.parametrize("K", [6, 12, 24])
@pytest.mark.parametrize("name", ["cubic3", "fcc4"])
def test_one_atom_cells(name, K):
    """Only self-images are neighbours; the K-th place lies on (6, 12 / 12) and inside (24 / 6, 24) a shell boundary."""
    res = _build(name, K)
    _check(res, name, K)
    assert (res.nbr_idx == 0).all() and (res.self_idx == 0).all()


@pytest.mark.parametrize("name,K", [("rocksalt", 12), ("hcp", 24)])
def test_known_lattices(name, K):
    _check(_build(name, K), name, K)


def test_skewed_triclinic_wrapped_and_shifted():
    res = _build("triclinic", 24)
    _check(res, "triclinic", 24)
    for t in (res.shell, res.self_idx, res.nbr_idx):
        assert torch.equal(t[0:2], t[2:4]) and torch.equal(t[0:2], t[4:6])
    assert float((res.dist[0:2] - res.dist[2:4]).abs().max()) <= 2e-8
    assert float((res.dist[0:2] - res.dist[4:6]).abs().max()) <= 2e-8


def test_dropping_and_radius_growth():
    """a = 15 (6 neighbours within 18 A) is not built; a = 8 and the ordinary crystal beside it are.  From a first working
    radius of 3 A every atom has to grow its radius, and the tables do not change."""
    res = _build("drop", 24)
    _check(res, "drop", 24)
    assert res.status.cpu().tolist() == [1, 0, 0]
    assert not res.shell[0].any() and not res.nbr_idx[0].any() and not res.dist[0].any()
    grown = _build("drop", 24, cap=2048, first_radius=3.0)
    _check(grown, "drop", 24)
    assert int(grown.passes.min()) >= 2
    assert all(torch.equal(a, b) for a, b in ((res.shell, grown.shell), (res.nbr_idx, grown.nbr_idx), (res.dist, grown.dist)))
    none = _build("drop", 24, radius=2.0)
    _check(none, "drop", 24, 2.0)
    assert none.status.cpu().tolist() == [1, 1, 1]
    assert not none.shell.any() and not none.self_idx.any() and not none.nbr_idx.any() and not none.dist.any()


@pytest.mark.parametrize("K", [12, 24])
@pytest.mark.parametrize("name", ["random8", "ragged64"])
def test_ragged_random_batches(name, K):
    res = _build(name, K)
    _check(res, name, K)
    assert int(res.passes.min()) >= 1 and int(res.passes.max()) <= 24


@pytest.mark.parametrize("K", [12, 24])
def test_candidate_buffer_shrinks(K):
    """A 256-entry candidate list searched first at the full radius overflows for every atom (the 60-atom 6 A cell holds
    about 6 800 candidates within 18 A): the radius shrinks until the list fits and the tables do not change."""
    res = _build("ragged64", K, cap=256, first_radius=18.0)
    _check(res, "ragged64", K)
    assert int(res.passes.min()) >= 2


def test_cut_shell_that_does_not_fit_is_status_2():
    """Simple cubic at K = 24: the shell holding the 24th place ends at candidate 26.  A 26-entry list builds the row, a
    24-entry list cannot: status 2 and zero rows, never a wrong row; the public entry raises."""
    ok = _build("cubic3", 24, cap=26)
    _check(ok, "cubic3", 24)
    bad = _build("cubic3", 24, cap=24)
    assert bad.status.cpu().tolist() == [2]
    assert not bad.shell.any() and not bad.nbr_idx.any() and not bad.dist.any()
    import cgat_amd as P
    lat = torch.eye(3, dtype=torch.float64, device=DEV)[None] * 30.0
    frac = torch.rand(1025, 3, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="limits"):
        P.neighbor_tables(lat, frac, torch.tensor([0, 1025], dtype=torch.int32, device=DEV), 12, radius=8.0)


def test_atom_limit_1024_builds():
    _check(_build("big1024", 12, radius=8.0), "big1024", 12, 8.0)


@pytest.mark.parametrize("K", [1, 64])
def test_k_extremes(K):
    _check(_build("small", K), "small", K)


def test_bitwise_deterministic():
    a, b = _build("ragged64", 24), _build("ragged64", 24)
    for n in ("shell", "self_idx", "nbr_idx", "status", "dist", "passes"):
        assert torch.equal(getattr(a, n), getattr(b, n)), n


def test_without_optional_outputs_and_empty():
    import cgat_amd as P
    lat, frac, ptr = _inputs("random8")
    full, plain = _build("random8", 12), P.neighbor_tables(lat, frac, ptr, 12)
    assert plain.dist is None and plain.passes is None
    assert torch.equal(plain.shell, full.shell) and torch.equal(plain.nbr_idx, full.nbr_idx)
    empty = P.neighbor_tables(lat[:0], frac[:0], ptr[:1], 12)
    assert empty.shell.shape == (0, 12) and empty.status.shape == (0,)


# ---------------------------------------------------------------------------------------------------------------
# end to end: structures -> dataset dictionary / PackedDataset -> collate -> CGAtNet
# ---------------------------------------------------------------------------------------------------------------
def _structures():
    import cgat_amd as P
    s = P.synthetic_structures(6, 4, (2, 12))
    lone = (np.eye(3) * 15.0, np.zeros((1, 3)), ["Fe"])          # 6 neighbours within 18 A: dropped at 24
    return s[:2] + [lone] + s[2:]


def _embedding():
    from cgat_amd.graph import ELEMENT_SYMBOLS, element_table
    table = element_table().numpy()
    return {el: table[k].astype("float64").tolist() for k, el in enumerate(ELEMENT_SYMBOLS)}


def _duck(s):
    lat, frac, syms = s
    sites = [types.SimpleNamespace(specie=types.SimpleNamespace(symbol=el)) for el in syms]

    class Structure:
        lattice = types.SimpleNamespace(matrix=lat)
        frac_coords = frac

        def __iter__(self):
            return iter(sites)
    return Structure()


def test_structures_to_prediction():
    import cgat_amd as P
    structures, emb = _structures(), _embedding()
    targets = {"e_above_hull": np.linspace(-1.0, 2.0, len(structures)), "volume": np.linspace(10.0, 90.0, len(structures))}
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        data, kept = P.dataset_dict_from_structures(structures, targets, ids=[f"id{k}" for k in range(len(structures))])
    msgs = [str(x.message) for x in w if "enough neighbors" in str(x.message)]
    assert len(msgs) == 1 and msgs[0].startswith("id2 ")
    assert kept.tolist() == [0, 1, 3, 4, 5, 6] and data["batch_ids"] == [f"id{k}" for k in kept]
    assert data["input"].shape == (3, 6) and data["input"].dtype == object
    for k, g in enumerate(kept):
        n = len(structures[g][2])
        for r in range(3):
            assert data["input"][r][k].shape == (n, 24) and data["input"][r][k].dtype == np.int64
        assert data["target"]["e_above_hull"][k] == targets["e_above_hull"][g] / n
        assert data["comps"][k] == structures[g][2]
    back = pickle.loads(pickle.dumps(data))
    assert all(np.array_equal(back["input"][r][k], data["input"][r][k]) for r in range(3) for k in range(6))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        duck, kept2 = P.dataset_dict_from_structures([_duck(s) for s in structures], targets)
    assert kept2.tolist() == kept.tolist() and duck["comps"] == data["comps"] and duck["batch_comp"] == data["batch_comp"]
    assert all(np.array_equal(duck["input"][r][k], data["input"][r][k]) for r in range(3) for k in range(6))
    assert all(np.array_equal(duck["target"][t], data["target"][t]) for t in targets)

    ids = [5, 0, 3, 3, 1]
    for target in ("e_above_hull", "volume"):
        a = P.PackedDataset.from_dict(data, emb, max_neighbor_number=12, target=target, device=DEV)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            b = P.PackedDataset.from_structures(structures, targets, emb, max_neighbor_number=12, stored_neighbors=24,
                                                target=target, device=DEV)
        assert len([x for x in w if "enough neighbors" in str(x.message)]) == 1
        assert len(a) == len(b) == 6 and b.kept.tolist() == kept.tolist()
        (ga, ra), (gb, rb) = a.collate(ids), b.collate(ids)
        for x, y in zip((ga.x, ga.edge_index, ga.edge_attr, ga.y, ga.batch) + tuple(ra),
                        (gb.x, gb.edge_index, gb.edge_attr, gb.y, gb.batch) + tuple(rb)):
            assert x.dtype == y.dtype and torch.equal(x, y)
    torch.manual_seed(0)
    net = P.CGAtNet(200, 64, 2, msg_heads=2, neighbor_number=12, update_edges=True).to(DEV).eval()
    with torch.no_grad():
        out = net(gb, rb)
    assert out.shape == (len(ids), 2) and torch.isfinite(out).all()
