"""The numpy reference of the rank search (tests/rank_search_ref.py) on hand-worked cases, the widths of its fp64 intervals on the
corpora of tests/test_gpu_rank_search.py (the table that file's docstring states), the host helpers of visrag_amd/documents.py
(reciprocal_ranks, mrr_from_ranks, recall_at) and the declarations of the three ABI symbols.  No GPU, no library."""
import os

import numpy as np
import pytest

from tests import rank_search_ref as K
from visrag_amd.documents import mrr_from_ranks, recall_at, reciprocal_ranks

# one query, six rows: scores [.5, 1, .5, .25, 1, .5]
S = np.array([0.5, 1.0, 0.5, 0.25, 1.0, 0.5])


def test_rank_is_score_descending_then_lower_id_first():
    assert [K.rank_ref(S, i) for i in range(6)] == [2, 0, 3, 5, 1, 4]
    assert K.ranking(S).tolist() == [1, 4, 0, 2, 5, 3]
    assert K.ranks_of_ranking(K.ranking(S)).tolist() == [2, 0, 3, 5, 1, 4]


def test_rank_under_a_mask_whether_or_not_it_allows_the_target():
    mask = np.array([1, 0, 1, 1, 1, 0], dtype=bool)
    assert [K.rank_ref(S, i, mask) for i in range(6)] == [1, 0, 2, 3, 0, 3]     # rows 1 and 5: the position they WOULD take


def test_counts():
    assert [K.count_ref(S, t) for t in (0.25, 0.5, 0.75, 1.0, 2.0)] == [6, 5, 2, 2, 0]
    assert [K.count_ref(S, t, strict=True) for t in (0.25, 0.5, 0.75, 1.0)] == [5, 2, 2, 0]
    assert K.count_ref(S, 0.5, mask=np.array([1, 0, 1, 1, 1, 0], dtype=bool)) == 3
    assert K.count_ref(np.array([0.0, -1.0]), -0.0) == 1 and K.count_ref(np.array([0.0, -1.0]), -0.0, strict=True) == 0
    s = np.array([np.float64(np.float32(0.1))])                          # the threshold is compared as the float32 it is handed over as
    assert K.count_ref(s, 0.1) == 1 and K.count_ref(s, np.nextafter(np.float32(0.1), np.float32(1))) == 0


def test_interval():
    s = np.array([0.5, 0.5 + 4e-7, 0.5 - 4e-7, 0.5 + 7e-7, 0.2])
    assert K.interval(s, 0.5) == (1, 3)                                  # the row itself and the two within 6e-7 may trade places
    assert K.interval(s, 0.5, tol=3e-7) == (2, 2)
    assert K.interval(s, 0.2) == (4, 4)
    assert K.TOL == 6e-7


def test_targets_are_the_three_best_and_eight_spread_rows():
    Sq = np.stack([np.linspace(1, 0, 1000), np.linspace(0, 1, 1000)])
    assert K.targets(Sq, 0).tolist() == sorted({0, 1, 2} | {(j * 104729 + 1) % 1000 for j in range(8)})
    assert K.targets(Sq, 1).tolist() == sorted({999, 998, 997} | {(7919 + j * 104729 + 1) % 1000 for j in range(8)})
    lims, ids = K.all_targets(Sq)
    assert lims.tolist() == [0, len(K.targets(Sq, 0)), len(K.targets(Sq, 0)) + len(K.targets(Sq, 1))] and len(ids) == lims[-1]


@pytest.mark.parametrize("name", list(K.TABLE))
def test_interval_widths_of_the_corpora(name):
    """the 6e-7 table of the GPU test: (pairs, widened intervals, summed width, max width), and the summed width at 3e-7"""
    wide, narrow = K.TABLE[name]
    S_ = K.case(name)[2]
    assert K.interval_table(S_) == wide
    assert K.interval_table(S_, 3e-7)[2] == narrow
    assert wide[3] <= 3


def test_shards_case_holds_equal_rows_across_shards():
    C, Q, bounds = K.shards_case()
    assert C.shape == (6000, 256) and bounds == (0, 1000, 4001, 6000)
    src, dst = np.arange(50) * 17 + 5, 4001 + np.arange(50) * 31 + 2
    assert src.max() < 1000 and dst.min() >= 4001 and dst.max() < 6000 and np.array_equal(C[src], C[dst])


# ------------------------------------------------------------------------------------------------ host helpers ---
def test_reciprocal_ranks_and_mrr():
    lims = [0, 2, 2, 3, 6]
    ranks = [4, 1, 0, 30, 12, 10]                                        # best: 1 | none | 0 | 10
    assert reciprocal_ranks(ranks, lims).tolist() == [0.5, 0.0, 1.0, 1 / 11]
    assert reciprocal_ranks(ranks, lims, cutoff=10).tolist() == [0.5, 0.0, 1.0, 0.0]      # rank 10 is the 11th row
    assert reciprocal_ranks(ranks, lims, cutoff=11).tolist() == [0.5, 0.0, 1.0, 1 / 11]
    assert mrr_from_ranks(ranks, lims) == pytest.approx((0.5 + 1.0 + 1 / 11) / 4, abs=1e-15)
    assert mrr_from_ranks(ranks, lims, cutoff=1) == 0.25
    assert mrr_from_ranks([], [0]) == 0.0
    for bad in ([1, 6], [0, 7], [0, 4, 2, 6]):
        with pytest.raises(ValueError):
            mrr_from_ranks(ranks, bad)
    with pytest.raises(ValueError):
        mrr_from_ranks([-1], [0, 1])


def test_recall_at():
    lims = [0, 2, 2, 3, 6]
    ranks = [4, 1, 0, 30, 12, 10]
    # k = 1: 0/2, 1/1, 0/3    k = 5: 2/2, 1/1, 0/3    k = 11: 2/2, 1/1, 1/3    k = 100: all; the query without positives is left out
    np.testing.assert_allclose(recall_at(ranks, lims, [1, 5, 11, 100]), [1 / 3, 2 / 3, (2 + 1 / 3) / 3, 1.0], atol=1e-15, rtol=0)
    assert recall_at([], [0, 0], [10]).tolist() == [0.0]
    assert recall_at(ranks, lims, []).shape == (0,)


# ------------------------------------------------------------------------------------------------ declarations ---
def test_the_three_symbols_are_declared_in_every_layer():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from visrag_amd import _lib, build
    header = open(os.path.join(root, "include", "visrag_hip.h")).read()
    for name in ("vr_index_rank_rows", "vr_index_count_range", "vr_index_rank_search_stats"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vr_index_rank_rows"][1]) == 10 and len(_lib.SIGNATURES["vr_index_count_range"][1]) == 10
    assert "search_rank.hip" in build.SOURCES and build.SOURCES.index("search_rank.hip") < build.SOURCES.index("index.hip")
