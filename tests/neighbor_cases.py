"""Test infrastructure for the neighbour tables: a numpy fp64 brute-force restatement of the definition and
the named test structures.  The product never imports this file.

The restatement enumerates ALL periodic images from the interplanar-spacing range at the FULL radius -- no working
radius, no candidate buffer -- sorts, applies the chain rule of CGAT/prepare_data.py:163-169 and the (shell, j) tie rule.
"""
import functools

import numpy as np

EPS = 1e-8


def _geometry(lat, frac):
    lat = np.asarray(lat, np.float64)
    frac = np.asarray(frac, np.float64).reshape(-1, 3)
    f = frac - np.floor(frac)
    pos = f[:, 0:1] * lat[0] + f[:, 1:2] * lat[1] + f[:, 2:3] * lat[2]
    a, b, c = lat
    V = abs(float(np.dot(a, np.cross(b, c))))
    h = [V / np.linalg.norm(np.cross(b, c)), V / np.linalg.norm(np.cross(c, a)), V / np.linalg.norm(np.cross(a, b))]
    return lat, pos, h


def sorted_candidates(lat, frac, radius=18.0):
    """Per atom: (d, j) of every candidate with 1e-8 < d <= radius, sorted by (d, j)."""
    lat, pos, h = _geometry(lat, frac)
    m = [int(np.floor(radius / hx * (1.0 + 1e-12))) + 1 for hx in h]
    Ra, Rb, Rc = np.meshgrid(*(np.arange(-mx, mx + 1, dtype=np.float64) for mx in m), indexing="ij")
    Ra, Rb, Rc = Ra.reshape(-1, 1), Rb.reshape(-1, 1), Rc.reshape(-1, 1)
    T = Ra * lat[0] + Rb * lat[1] + Rc * lat[2]                       # [images, 3]
    n = pos.shape[0]
    jj = np.broadcast_to(np.arange(n)[None, :], (T.shape[0], n))
    out = []
    for i in range(n):
        disp = (pos[None, :, :] + T[:, None, :]) - pos[i]
        d = np.sqrt(disp[..., 0] * disp[..., 0] + disp[..., 1] * disp[..., 1] + disp[..., 2] * disp[..., 2])
        keep = (d > EPS) & (d <= radius)
        dd, j = d[keep], jj[keep]
        order = np.lexsort((j, dd))
        out.append((dd[order], j[order]))
    return out


def _row(dd, jj, K):
    """(shell[K], nbr[K], dist[K], p1): chain-rule shells; the shell holding the K-th place in ascending j; ordered by
    (shell, j).  p1: one past the last member of that shell in the sorted list."""
    shell = np.zeros(len(dd), np.int64)
    first, sh, p = dd[0], 1, 0
    while p < len(dd):
        if dd[p] > first + EPS:
            if p >= K:
                break
            first, sh = dd[p], sh + 1
        shell[p] = sh
        p += 1
    p1 = p
    s, j, d = shell[:p1], jj[:p1], dd[:p1]
    order = np.lexsort((d, j, s))[:K]
    return s[order], j[order], d[order], p1


def reference_tables(lat, frac, K, radius=18.0, cands=None):
    """status, shell, self_idx, nbr_idx, dist ([n, K]; zero rows unless status == 0) of one crystal."""
    cands = sorted_candidates(lat, frac, radius) if cands is None else cands
    n = len(cands)
    shell, self_idx, nbr = (np.zeros((n, K), np.int32) for _ in range(3))
    dist = np.zeros((n, K), np.float64)
    if any(len(dd) < K for dd, _ in cands):
        return 1, shell, self_idx, nbr, dist
    for i, (dd, jj) in enumerate(cands):
        shell[i], nbr[i], dist[i], _ = _row(dd, jj, K)
        self_idx[i] = i
    return 0, shell, self_idx, nbr, dist


def shell_counts(lat, frac, K, radius=18.0):
    """Members per shell of atom 0's row."""
    st, shell, _, _, _ = reference_tables(lat, frac, K, radius)
    assert st == 0
    return np.bincount(shell[0])[1:].tolist()


def ambiguous_gaps(lat, frac, K, radius=18.0, cands=None):
    """Adjacent gaps inside (1e-10, 1e-6) among the sorted distances of any atom, through the first K + 1 and through one
    past the shell that holds the K-th place: with none, shell membership does not depend on last-bit rounding."""
    bad = 0
    for dd, jj in (sorted_candidates(lat, frac, radius) if cands is None else cands):
        if len(dd) < K:
            continue
        p1 = _row(dd, jj, K)[3]
        gaps = np.diff(dd[:max(K + 1, p1 + 1)])
        bad += int(((gaps > 1e-10) & (gaps < 1e-6)).sum())
    return bad


# ---------------------------------------------------------------------------------------------------------------
# named structures: (lattice rows a, b, c; fractional coordinates)
# ---------------------------------------------------------------------------------------------------------------
def cubic(a):
    return np.eye(3) * a, np.zeros((1, 3))


def fcc_primitive(a=4.0):
    return np.array([[0, a / 2, a / 2], [a / 2, 0, a / 2], [a / 2, a / 2, 0]], np.float64), np.zeros((1, 3))


def rocksalt(a=5.64):
    fcc = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]], np.float64)
    return np.eye(3) * a, np.concatenate([fcc, fcc + np.array([.5, 0, 0])])


def hcp(a=2.95, c=4.68):      # c/a = 1.586, not the ideal 1.633: the two nearest shells are distinct
    lat = np.array([[a, 0, 0], [-a / 2, a * np.sqrt(3) / 2, 0], [0, 0, c]], np.float64)
    return lat, np.array([[1 / 3, 2 / 3, 1 / 4], [2 / 3, 1 / 3, 3 / 4]], np.float64)


def triclinic_skewed():
    """Interplanar spacings far below the edge lengths: an image range taken from |a| misses neighbours."""
    lat = np.array([[3, 0, 0], [2.9, 0.9, 0], [2.7, 0.8, 1.1]], np.float64)
    return lat, np.array([[0.1, 0.2, 0.3], [-0.4, 1.7, 0.55]], np.float64)


def random_cell(seed, atoms=(1, 12)):
    rs = np.random.RandomState(seed)
    n = int(rs.randint(atoms[0], atoms[1] + 1))
    lat = np.diag(rs.uniform(3.5, 6.5, size=3)) + rs.uniform(-0.8, 0.8, size=(3, 3)) * (1 - np.eye(3))
    return lat, rs.uniform(-1.0, 2.0, size=(n, 3))


def dense_cell(seed=11, n=60, a=6.0):
    rs = np.random.RandomState(seed)
    return np.eye(3) * a + rs.uniform(-0.3, 0.3, size=(3, 3)) * (1 - np.eye(3)), rs.uniform(0.0, 1.0, size=(n, 3))


@functools.lru_cache(maxsize=None)
def batch(name):
    """Named lists of crystals the GPU tests run; the CPU tests check the input condition on every one of them."""
    if name == "cubic3":
        return [cubic(3.0)]
    if name == "fcc4":
        return [fcc_primitive(4.0)]
    if name == "rocksalt":
        return [rocksalt()]
    if name == "hcp":
        return [hcp()]
    if name == "triclinic":
        lat, frac = triclinic_skewed()
        return [(lat, frac), (lat, frac - np.floor(frac)), (lat, frac + np.array([0.37, -1.21, 2.6]))]
    if name == "drop":
        return [cubic(15.0), cubic(8.0), random_cell(3)]
    if name == "random8":
        return [random_cell(s) for s in range(8)]
    if name == "ragged64":
        from cgat_amd.neighbors import synthetic_structures
        cells = [(lat, frac) for lat, frac, _ in synthetic_structures(63, 5, (1, 40))]
        return cells[:31] + [dense_cell()] + cells[31:]
    if name == "small":
        return [random_cell(2, (3, 3))]
    if name == "big1024":      # the documented atom limit, exactly
        rs = np.random.RandomState(21)
        return [(np.eye(3) * 24.0 + rs.uniform(-1, 1, size=(3, 3)) * (1 - np.eye(3)), rs.uniform(0, 1, size=(1024, 3)))]
    raise KeyError(name)


# (batch, K, radius) of every GPU comparison: the CPU input-condition test walks this list
GPU_RUNS = [("cubic3", 6, 18.0), ("cubic3", 12, 18.0), ("cubic3", 24, 18.0), ("fcc4", 6, 18.0), ("fcc4", 12, 18.0),
            ("fcc4", 24, 18.0), ("rocksalt", 12, 18.0), ("hcp", 24, 18.0), ("triclinic", 24, 18.0), ("drop", 24, 18.0),
            ("drop", 24, 2.0), ("random8", 12, 18.0), ("random8", 24, 18.0), ("ragged64", 12, 18.0), ("ragged64", 24, 18.0),
            ("small", 1, 18.0), ("small", 64, 18.0), ("big1024", 12, 8.0)]


@functools.lru_cache(maxsize=None)
def candidates(name, radius=18.0):
    """sorted_candidates of every crystal of a named batch, computed once per radius."""
    return [sorted_candidates(lat, frac, radius) for lat, frac in batch(name)]


@functools.lru_cache(maxsize=None)
def reference(name, K, radius=18.0):
    """The restatement on a named batch, computed once and shared: list of (status, shell, self_idx, nbr_idx, dist)."""
    out = [reference_tables(lat, frac, K, radius, c) for (lat, frac), c in zip(batch(name), candidates(name, radius))]
    for t in out:
        for a in t[1:]:
            a.setflags(write=False)
    return out


def flat(cells):
    """lattice [G,3,3], frac [N,3], atom_ptr [G+1] (numpy) of a list of crystals."""
    lat = np.stack([np.asarray(c[0], np.float64) for c in cells])
    frac = np.concatenate([np.asarray(c[1], np.float64).reshape(-1, 3) for c in cells])
    ptr = np.zeros(len(cells) + 1, np.int32)
    ptr[1:] = np.cumsum([np.asarray(c[1]).reshape(-1, 3).shape[0] for c in cells])
    return lat, frac, ptr
