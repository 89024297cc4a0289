"""The piece bound of the class plan without a GPU: for every case of tests/indexed_cases.py the numpy reference cuts the
classes into at most cgat_indexed_class_pieces(E, R) pieces -- the rows of the partial sums that the backward's workspace
holds -- and that bound is ceil(E / 256) + R.  Host arithmetic only: no device is touched."""
import numpy as np
import pytest

from indexed_cases import PLAN_CASES, class_index, class_plan_reference


@pytest.mark.parametrize("E,R,dist", PLAN_CASES, ids=lambda v: str(v))
def test_reference_pieces_within_bound(E, R, dist):
    from cgat_amd import _lib
    bound = _lib.lib.cgat_indexed_class_pieces(E, R)
    assert bound == -(-E // 256) + R, (E, R, bound)
    index = class_index(E, R, dist)
    perm = np.random.RandomState(5).permutation(E)
    cls_pos, piece_start, piece_rowptr = class_plan_reference(index, perm, R, bound)
    total = int(piece_start[R])
    print(f"[indexed-shapes] plan ({E}, {R}, {dist}): {total} pieces, bound {bound}, ceil(E / 256) = {-(-E // 256)}")
    assert total <= bound, (total, bound)
    assert piece_rowptr.shape[0] == bound + 1 and bool((piece_rowptr[total:] == E).all())
    assert bool((np.diff(piece_rowptr) >= 0).all()) and int(np.diff(piece_rowptr).max()) <= 256
    assert np.array_equal(np.sort(cls_pos), np.arange(E))
    if dist == "pairs":
        assert total > -(-E // 256)               # the + R of the bound is needed
