"""The numpy reference of the filtered search (tests/filter_search_ref.py) on hand-worked cases, and the host helpers of
visrag_amd/documents.py (pack_filters, group_filter, label_filters).  No GPU, no library."""
import numpy as np
import pytest

from tests import filter_search_ref as F
from visrag_amd.documents import group_filter, label_filters, pack_filters

# five rows on two axes; query 0 = e0, query 1 = e1
C = np.array([[1.0, 0.0], [0.5, 0.5], [0.5, 0.25], [0.25, 1.0], [0.5, 0.5]], dtype=np.float32)
Q = np.array([[1.0, 0.0], [0.0, 1.0]], dtype=np.float32)
# scores: q0 = [1, .5, .5, .25, .5]   q1 = [0, .5, .25, 1, .5]
ALL = np.ones(5, dtype=bool)


def test_a_tie_is_broken_by_id():
    sc, ids = F.filtered_topk_ref(Q, C, [ALL], [0, 0], 4)
    assert ids.tolist() == [[0, 1, 2, 4], [3, 1, 4, 2]]
    assert sc.tolist() == [[1.0, 0.5, 0.5, 0.5], [1.0, 0.5, 0.5, 0.25]]


def test_the_best_row_excluded():
    no0 = np.array([0, 1, 1, 1, 1], dtype=bool)
    no3 = np.array([1, 1, 1, 0, 1], dtype=bool)
    sc, ids = F.filtered_topk_ref(Q, C, [no0, no3], [0, 1], 2)
    assert ids.tolist() == [[1, 2], [1, 4]] and sc.tolist() == [[0.5, 0.5], [0.5, 0.5]]


def test_fewer_than_k_allowed():
    two = np.array([0, 0, 1, 1, 0], dtype=bool)
    sc, ids = F.filtered_topk_ref(Q, C, [two], [0, 0], 4)
    assert ids.tolist() == [[2, 3, -1, -1], [3, 2, -1, -1]]
    assert sc[:, :2].tolist() == [[0.5, 0.25], [1.0, 0.25]] and np.isneginf(sc[:, 2:]).all()


def test_none_allowed():
    sc, ids = F.filtered_topk_ref(Q, C, [np.zeros(5, dtype=bool)], [0, 0], 3)
    assert (ids == -1).all() and np.isneginf(sc).all() and sc.shape == (2, 3) and ids.dtype == np.int64


def test_minus_one_is_no_filter():
    one = np.array([0, 0, 0, 0, 1], dtype=bool)
    sc, ids = F.filtered_topk_ref(Q, C, [one], [-1, 0], 2)
    assert ids.tolist() == [[0, 1], [4, -1]] and sc[0].tolist() == [1.0, 0.5] and sc[1, 0] == 0.5 and np.isneginf(sc[1, 1])
    # k beyond the row count
    sc, ids = F.filtered_topk_ref(Q, C, [one], [-1, -1], 7)
    assert ids[0].tolist() == [0, 1, 2, 4, 3, -1, -1] and np.isneginf(sc[:, 5:]).all()


def test_random_filters_is_reproducible_and_of_the_stated_densities():
    m = F.random_filters(5000, (0.5, 0.05, 0.002))
    assert m.shape == (3, 5000) and m.dtype == np.bool_
    assert m.sum(1).tolist() == [2532, 262, 10]
    assert np.array_equal(m, F.random_filters(5000, (0.5, 0.05, 0.002), seed=11))
    assert F.random_filters(3001, (0.9, 0.3, 0.01, 0.004)).sum(1).tolist() == [2721, 905, 22, 12]
    assert F.random_filters(20000, (0.5, 0.01)).sum(1).tolist() == [10135, 214]
    assert F.random_filters(1000, (0.5, 0.03)).sum(1).tolist() == [520, 32]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1001])
def test_pack_filters(n):
    m = np.random.default_rng(n).random((3, n)) < 0.5
    m[0, -1] = True
    w = pack_filters(m)
    words = (n + 31) // 32
    assert w.dtype == np.uint32 and w.shape == (3, words) and w.flags.c_contiguous
    padded = np.zeros((3, words * 32), dtype=bool)
    padded[:, :n] = m
    assert np.array_equal(w.view(np.uint8), np.packbits(padded, axis=1, bitorder="little"))
    for f in range(3):                                                  # the bit layout, spelled out
        for r in range(n):
            assert bool((int(w[f, r >> 5]) >> (r & 31)) & 1) == bool(m[f, r])
    assert np.array_equal(pack_filters(m[1]), w[1:2])                   # one filter as a vector


def test_group_filter():
    off = [0, 2, 5, 6, 10]
    assert group_filter(off, [1, 3]).tolist() == [False] * 2 + [True] * 3 + [False] + [True] * 4
    assert group_filter(off, []).tolist() == [False] * 10
    assert group_filter(off, [2, 2]).sum() == 1
    with pytest.raises(ValueError):
        group_filter(off, [4])


def test_label_filters():
    labels = ["a", "b", "a", "c", "b"]
    m = label_filters(labels, [{"a"}, ["b", "c"], None, {"zzz"}, set()])
    assert m.dtype == np.bool_ and m.tolist() == [[True, False, True, False, False], [False, True, False, True, True],
                                                  [True] * 5, [False] * 5, [False] * 5]
