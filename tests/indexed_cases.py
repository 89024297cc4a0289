"""Cases and the numpy reference of the class plan of the indexed training route (cgat_indexed_class_plan,
csrc/edgeidx.hip), shared by tests/test_indexed_edge_shapes.py (GPU: the three arrays, bit for bit) and
tests/test_indexed_edge_shapes_cpu.py (host arithmetic: the piece bound).  numpy only: no device, no library."""
import numpy as np

PIECE_ROWS = 256            # IDX_PIECE_ROWS: rows of one piece of a class

# (E, R, distribution of the classes over the edges)
PLAN_CASES = (
    (1, 1, "zero"),
    (255, 3, "uniform"),
    (256, 1, "zero"),
    (257, 256, "pairs"),        # every class <= 2 rows: more pieces than ceil(E / 256)
    (65536, 13, "uniform"),     # 256 count blocks: the last size of the scan's one-block-per-thread branch
    (65537, 13, "uniform"),     # 257 count blocks: two per thread
    (200003, 25, "skew"),
    (5000, 13, "clamp"),
)
SKEW_SIZES = (1, 256, 257, 512)


def skew_sizes(E, R):
    """Rows per class of the skewed distribution: classes 0, R // 2 - 1 and R - 1 empty, class R // 2 holds the rest, the
    others exactly 1, 256, 257, 512, 1, ... rows."""
    n = np.zeros(R, dtype=np.int64)
    rest, j = R // 2, 0
    for r in range(1, R - 1):
        if r in (rest - 1, rest):
            continue
        n[r] = SKEW_SIZES[j % 4]
        j += 1
    n[rest] = E - int(n.sum())
    assert n[rest] > 512 and n[0] == 0 and n[R - 1] == 0 and int(n.sum()) == E
    return n


def class_index(E, R, dist, seed=3):
    """index [E] int64 in original edge order."""
    rs = np.random.RandomState(seed)
    if dist == "zero":
        return np.zeros(E, dtype=np.int64)
    if dist == "uniform":
        return rs.randint(0, R, size=E).astype(np.int64)
    if dist == "pairs":
        idx = (np.arange(E) % R).astype(np.int64)
        assert np.bincount(idx, minlength=R).max() <= 2
        return idx[rs.permutation(E)]
    if dist == "skew":
        return np.repeat(np.arange(R, dtype=np.int64), skew_sizes(E, R))[rs.permutation(E)]
    if dist == "clamp":                    # twenty entries below the table and twenty behind it
        idx = rs.randint(0, R, size=E).astype(np.int64)
        bad = rs.permutation(E)[:40]
        idx[bad[:20]], idx[bad[20:]] = -1, R + 5
        return idx
    raise ValueError(dist)


def class_plan_reference(index, dst_perm, R, n_pieces_max):
    """(cls_pos [E], piece_start [R + 1], piece_rowptr [n_pieces_max + 1]) as int32: destination-sorted slot t has class
    k[t] = clip(index[dst_perm[t]], 0, R - 1); cls_pos lists the slots by class, ascending inside a class; piece_start is
    the exclusive prefix of ceil(n_r / 256); piece_rowptr[p] the first row of piece p, E from the total on."""
    E = int(index.shape[0])
    k = np.clip(index[dst_perm], 0, R - 1)
    cls_pos = np.argsort(k, kind="stable").astype(np.int32)
    n = np.bincount(k, minlength=R).astype(np.int64)
    pieces = -(-n // PIECE_ROWS)
    piece_start = np.concatenate([[0], np.cumsum(pieces)]).astype(np.int32)
    row0 = np.concatenate([[0], np.cumsum(n)])
    piece_rowptr = np.full(max(n_pieces_max, int(piece_start[R])) + 1, E, dtype=np.int32)
    for r in range(R):
        for j in range(int(pieces[r])):
            piece_rowptr[piece_start[r] + j] = row0[r] + PIECE_ROWS * j
    return cls_pos, piece_start, piece_rowptr
