"""The numpy reference of the document-level search (tests/group_search_ref.py) on hand-worked cases, and the library's
contract for it: the three entry points are declared, bound and exported."""
import ctypes as C
import os
import re

import numpy as np

from tests import group_search_ref as R
from visrag_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _eye_case():
    # rows are multiples of unit axes: the score of row i against query e_j is exactly C[i][j]
    C_ = np.zeros((7, 4), np.float32)
    C_[0, 0] = 0.5; C_[1, 0] = 0.75; C_[2, 0] = 0.75          # group 0: rows 0-2, tie between rows 1 and 2
    C_[3, 0] = 0.25; C_[3, 1] = 0.5                           # group 1: row 3
    C_[4, 0] = 0.75; C_[5, 0] = -1.0                          # group 2: rows 4-5, ties with group 0 on axis 0
    C_[6, 1] = 1.0                                            # group 3: row 6
    return C_, np.array([0, 3, 4, 6, 7])


def test_tie_inside_a_group_takes_the_lower_row():
    C_, off = _eye_case()
    Q = np.array([[1, 0, 0, 0]], np.float32)
    sc, ids, gr = R.group_topk_ref(Q, C_, off, 1)
    assert sc[0, 0] == 0.75 and ids[0, 0] == 1 and gr[0, 0] == 0


def test_tie_between_groups_takes_the_lower_best_row_first():
    C_, off = _eye_case()
    Q = np.array([[1, 0, 0, 0], [0, 1, 0, 0]], np.float32)
    sc, ids, gr = R.group_topk_ref(Q, C_, off, 4)
    assert sc[0].tolist() == [0.75, 0.75, 0.25, 0.0]
    assert ids[0].tolist() == [1, 4, 3, 6] and gr[0].tolist() == [0, 2, 1, 3]
    # axis 1: group 3 (1.0), group 1 (0.5), then groups 0 and 2 tie at 0 with best rows 0 and 4
    assert sc[1].tolist() == [1.0, 0.5, 0.0, 0.0]
    assert ids[1].tolist() == [6, 3, 0, 4] and gr[1].tolist() == [3, 1, 0, 2]


def test_fewer_groups_than_k_fills_the_tail():
    C_, off = _eye_case()
    Q = np.array([[1, 0, 0, 0]], np.float32)
    sc, ids, gr = R.group_topk_ref(Q, C_, off, 6)
    assert ids[0].tolist() == [1, 4, 3, 6, -1, -1] and gr[0].tolist() == [0, 2, 1, 3, -1, -1]
    assert np.isneginf(sc[0, 4:]).all() and np.isfinite(sc[0, :4]).all()


def test_groups_of_one_row_are_the_row_ranking_and_one_group_is_the_best_row():
    C_, Q = R.unit(50, 16, 1), R.unit(3, 16, 2)
    S = R.scores64(Q, C_)
    sc, ids, gr = R.group_topk_ref(Q, C_, np.arange(51), 5)
    assert np.array_equal(ids, np.argsort(-S, axis=1, kind="stable")[:, :5]) and np.array_equal(ids, gr)
    sc, ids, gr = R.group_topk_ref(Q, C_, np.array([0, 50]), 2)
    assert np.array_equal(ids[:, 0], S.argmax(1)) and (gr[:, 0] == 0).all() and (ids[:, 1] == -1).all()
    np.testing.assert_array_equal(sc[:, 0], S.max(1))


def test_scores_are_fp64_on_the_fp32_data():
    C_, Q = R.unit(20, 2304, 3), R.unit(2, 2304, 4)
    sc, ids, _ = R.group_topk_ref(Q, C_, R.random_offsets(20, 3), 3)
    for q in range(2):
        for s, i in zip(sc[q], ids[q]):
            # (fp64 throughout: two summation orders of 2304 products of unit vectors agree to ~1e-16; an fp32 product is 1e-8 off)
            assert abs(s - float(np.dot(Q[q].astype(np.float64), C_[i].astype(np.float64)))) < 1e-14


def test_random_offsets_partition_the_rows():
    for n, mean in [(5000, 7), (3001, 10), (1000, 3), (1, 5)]:
        off = R.random_offsets(n, mean)
        assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 1).all() and (np.diff(off) < 2 * mean).all()


def test_tie_tier_corpus_is_what_the_gpu_tests_take_it_for():
    C, Q, ids = R.tie_tier()                                 # (its own asserts: one exact tier, gaps > 1e-2 above it, > 1e-4 among the rest)
    assert C.shape == (3000, 64) and Q.shape == (3, 64) and ids.shape == (3, 150) and C.dtype == Q.dtype == np.float32
    high = 7 * np.arange(100) + 3
    assert (np.sort(ids[:, :100], axis=1) == high).all() and (ids[0, :100] != high).any()     # (score order is not id order)
    assert (ids[:, 100:] == np.setdiff1d(np.arange(3000), high)[:50]).all()
    _, ri, rg = R.group_topk_ref(Q, C, np.arange(3001), 150)
    assert np.array_equal(ri, ids) and np.array_equal(rg, ids)


def test_grouped_search_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "visrag_hip.h")).read()
    lib = _lib.load()
    for name in ("vr_index_set_groups", "vr_index_search_groups", "vr_index_group_search_stats"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["vr_index_search_groups"][1].count(C.c_void_p) == 6      # ix, queries, three outputs, stream
