"""The numpy reference of the range search (tests/range_search_ref.py) on hand-worked cases, its corpora against the counts the
GPU test's docstring states, and the host helpers of visrag_amd/documents.py (split_ranges, duplicate_groups).  No GPU, no library."""
import numpy as np
import pytest

from tests import range_search_ref as X
from visrag_amd.documents import duplicate_groups, split_ranges

# five rows on two axes; query 0 = e0, query 1 = e1
C = np.array([[1.0, 0.0], [0.5, 0.5], [0.5, 0.25], [0.25, 1.0], [0.5, 0.5]], dtype=np.float32)
Q = np.array([[1.0, 0.0], [0.0, 1.0]], dtype=np.float32)
# scores: q0 = [1, .5, .5, .25, .5]   q1 = [0, .5, .25, 1, .5]


def _lists(res):
    return [x.tolist() for x in res]


def test_a_threshold_equal_to_a_score_keeps_the_row():
    assert _lists(X.range_ref(Q, C, 0.5)) == [[0, 4, 7], [1.0, 0.5, 0.5, 0.5, 0.5, 1.0, 0.5], [0, 1, 2, 4, 1, 3, 4]]
    above = np.nextafter(np.float32(0.5), np.float32(1))                 # the next fp32 threshold drops every 0.5
    assert _lists(X.range_ref(Q, C, above)) == [[0, 1, 2], [1.0, 1.0], [0, 3]]


def test_an_empty_segment_and_a_threshold_per_query():
    lims, sc, ids = X.range_ref(Q, C, [2.0, 0.25])
    assert lims.tolist() == [0, 0, 4] and ids.tolist() == [1, 2, 3, 4] and sc.tolist() == [0.5, 0.25, 1.0, 0.5]
    assert lims.dtype == np.int64 and ids.dtype == np.int64 and sc.dtype == np.float64
    lims, sc, ids = X.range_ref(Q, C, [2.0, 2.0])
    assert lims.tolist() == [0, 0, 0] and len(sc) == 0 and len(ids) == 0


def test_a_threshold_below_every_score_returns_every_row_in_id_order():
    lims, sc, ids = X.range_ref(Q, C, -2.0)
    assert lims.tolist() == [0, 5, 10] and ids.tolist() == [0, 1, 2, 3, 4] * 2
    assert sc.tolist() == [1.0, 0.5, 0.5, 0.25, 0.5, 0.0, 0.5, 0.25, 1.0, 0.5]


def test_a_filter():
    no0 = np.array([0, 1, 1, 1, 1], dtype=bool)
    only3 = np.array([0, 0, 0, 1, 0], dtype=bool)
    lims, sc, ids = X.range_ref(Q, C, 0.5, [no0, only3], [0, -1])
    assert lims.tolist() == [0, 3, 6] and ids.tolist() == [1, 2, 4, 1, 3, 4]
    lims, sc, ids = X.range_ref(Q, C, 0.5, [no0, only3], [1, 1])         # q0: its allowed row scores below t -> empty
    assert lims.tolist() == [0, 0, 1] and ids.tolist() == [3] and sc.tolist() == [1.0]


def test_the_threshold_is_compared_as_the_float32_it_is_handed_over_as():
    c = np.array([[np.float32(0.1)]], dtype=np.float32)                  # float32(0.1) > 0.1
    q = np.ones((1, 1), dtype=np.float32)
    assert X.range_ref(q, c, 0.1)[0].tolist() == [0, 1]
    assert X.range_ref(q, c, np.nextafter(np.float32(0.1), np.float32(1)))[0].tolist() == [0, 0]


def test_sort_ranges_is_score_descending_then_id():
    lims, sc, ids = X.sort_ranges(*X.range_ref(Q, C, 0.25))
    assert lims.tolist() == [0, 5, 9]
    assert ids.tolist() == [0, 1, 2, 4, 3, 3, 1, 4, 2] and sc.tolist() == [1.0, 0.5, 0.5, 0.5, 0.25, 1.0, 0.5, 0.5, 0.25]


@pytest.mark.parametrize("nd,nq,dim,cycle,total,lo,hi", [(5000, 37, 256, (0.10, 0.15, 0.20, 0.30), 3167, 0, 297),
                                                         (3001, 300, 128, (0.15, 0.25, 0.05), 100869, 1, 945)])
def test_random_cases_have_the_stated_counts(nd, nq, dim, cycle, total, lo, hi):
    C_, Q_, t, S = X.random_case(nd, nq, dim, cycle)
    lims, sc, ids = X.range_ref(Q_, C_, t)
    per = np.diff(lims)
    assert lims[-1] == total and per.min() == lo and per.max() == hi
    assert (np.abs(S - t.astype(np.float64)[:, None]) < 3e-7).sum() == 0
    for q in (0, nq - 1):                                                # ascending ids, the scores of those rows
        seg = slice(lims[q], lims[q + 1])
        assert (np.diff(ids[seg]) > 0).all() and np.array_equal(sc[seg], S[q, ids[seg]]) and (sc[seg] >= float(t[q])).all()


def test_families_and_scaled_norms_have_the_stated_counts():
    C_, Q_, S = X.families(64)
    assert C_.shape == (8000, 64) and Q_.shape == (8, 64)
    assert np.diff(X.range_ref(Q_, C_, 0.9)[0]).tolist() == [1500] * 8
    own = np.concatenate([S[q, (q // 2) * 1500:(q // 2 + 1) * 1500] for q in range(8)])
    assert np.float32(np.median(own)) == np.float32(X.FAMILY_MEDIAN[64])
    per = np.diff(X.range_ref(Q_, C_, X.FAMILY_MEDIAN[64])[0])
    assert per.sum() == 6000 and per.min() == 349 and per.max() == 1136
    C_, Q_, S = X.scaled_norms()
    norms = np.linalg.norm(C_, axis=1)
    assert 0.5 <= norms.min() < 0.51 and 2.99 < norms.max() <= 3.0
    for t, total, lo, hi in ((0.2, 3885, 164, 230), (0.4, 181, 4, 17)):
        per = np.diff(X.range_ref(Q_, C_, t)[0])
        assert per.sum() == total and per.min() == lo and per.max() == hi


# ------------------------------------------------------------------------------------------------ host helpers ---
def test_split_ranges():
    lims, sc, ids = X.range_ref(Q, C, [2.0, 0.25])
    parts = split_ranges(lims, sc, ids)
    assert len(parts) == 2 and len(parts[0][0]) == 0 and len(parts[0][1]) == 0
    assert parts[1][0].tolist() == [0.5, 0.25, 1.0, 0.5] and parts[1][1].tolist() == [1, 2, 3, 4]
    assert split_ranges([0], [], []) == []
    for bad in ([1, 4], [0, 3], [0, 3, 2, 4]):
        with pytest.raises(ValueError):
            split_ranges(bad, sc, ids)


def _csr(segments):
    lims = np.concatenate([[0], np.cumsum([len(s) for s in segments])]).astype(np.int64)
    return lims, np.array([i for s in segments for i in s], dtype=np.int64)


def test_duplicate_groups_chains_give_one_group():
    # rows 0..6 as queries: 5-2 and 2-6 chain (5-6 never match directly); 1-3 match; 0 and 4 match only themselves
    lims, ids = _csr([[0], [1, 3], [2, 5, 6], [1, 3], [4], [2, 5], [2, 6]])
    assert duplicate_groups(lims, ids, 7) == [[1, 3], [2, 5, 6]]
    # one direction of a match is enough, the order of the entries does not matter, rows beyond the queries may be matched
    lims, ids = _csr([[], [3], [6, 5], [], [], [], []])
    assert duplicate_groups(lims, ids, 8) == [[1, 3], [2, 5, 6]]
    lims, ids = _csr([[7], [], [6]])
    assert duplicate_groups(lims, ids, 8) == [[0, 7], [2, 6]]


def test_duplicate_groups_the_self_match_alone_gives_no_group():
    lims, ids = _csr([[0], [1], [2]])
    assert duplicate_groups(lims, ids, 3) == []
    assert duplicate_groups([0], [], 5) == []
    lims, ids = _csr([[0, 1, 2], [0, 1, 2], [0, 1, 2]])
    assert duplicate_groups(lims, ids, 3) == [[0, 1, 2]]
    with pytest.raises(ValueError):
        duplicate_groups(*_csr([[3]]), 3)
