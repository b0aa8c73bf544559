"""Plain numpy statement of the document window search (include/visrag_hip.h: vr_index_search_groups_window), the reference of
tests/test_gpu_group_window_search.py.  A document (group of adjacent rows) is present for a query if the query's mask allows one
of its pages; it scores as its best ALLOWED page does, its best row is the lowest allowed row that attains that score; present
documents rank score descending, then lower best row first; entry j of the window at offset o is the document of rank o + j,
slots at or past the number of present documents are (-inf, -1, -1).  Built on group_search_ref.group_best, with the score
matrix masked to -inf first.

Against fp64 the library's result is held to the rank and window searches' interval, with no excuse mechanism: the document of
fp64 score s at position j of the window at offset o has o + j in [#(E > s + TOL), #(E >= s - TOL) - 1] over the present
documents (TOL = 6e-7), its score lies within 1e-5 of s and its best row's fp64 score within TOL of s.
tests/test_cpu_group_window_search_ref.py pins how many of these intervals are wider than one position for the reference's own
windows on the corpora the GPU test uses.  Nothing here needs a GPU or the built library."""
import functools

import numpy as np

from tests import filter_search_ref as F
from tests import group_search_ref as R
from tests.rank_search_ref import TOL
from tests.window_search_ref import intervals

ATOL = 1e-5


def masked(S, mask):
    """S [nq][n] with the entries `mask` (bool [nq][n], [n] or None) forbids set to -inf"""
    S = np.asarray(S)
    if mask is None:
        return S
    return np.where(np.broadcast_to(np.asarray(mask, dtype=bool), S.shape), S, -np.inf)


def ordered(S):
    """fp32 scores -> int64 that order like the library's keys (-0.0 < +0.0); other dtypes are returned as they are"""
    S = np.asarray(S)
    if S.dtype != np.float32:
        return S
    u = np.ascontiguousarray(S).view(np.uint32).astype(np.int64)
    return np.where(u >> 31 != 0, 0xFFFFFFFF - u, u + 0x80000000)


def present_best(S, offsets, mask=None):
    """-> (E [nq][n_groups] the documents' best allowed score, -inf where absent; best [nq][n_groups] the lowest allowed row that
    attains it, -1 where absent; present bool [nq][n_groups])"""
    Sm = masked(S, mask)
    allowed = np.ones(Sm.shape, dtype=bool) if mask is None else np.broadcast_to(np.asarray(mask, dtype=bool), Sm.shape)
    E, best = R.group_best(Sm, offsets)
    present = np.maximum.reduceat(allowed, np.asarray(offsets, dtype=np.int64)[:-1], axis=1)
    return E, np.where(present, best, -1), present


def group_window_ref(S, offsets, mask, o, k):
    """S [nq][n] (fp64, or the library's own fp32 scores: ranked on their orderable bits), mask bool [nq][n] / [n] / None, o an int
    or one per query -> (scores [nq][k] of S's dtype, best row ids i64 [nq][k], groups i64 [nq][k])"""
    S = np.asarray(S)
    E, best, present = present_best(S, offsets, mask)
    nq, ng = E.shape
    o = np.broadcast_to(np.asarray(o, dtype=np.int64), (nq,))
    sc = np.full((nq, k), -np.inf, dtype=S.dtype)
    ids = np.full((nq, k), -1, dtype=np.int64)
    gr = np.full((nq, k), -1, dtype=np.int64)
    key = ordered(E)
    for q in range(nq):
        g = np.flatnonzero(present[q])
        order = g[np.lexsort((best[q][g], -key[q][g]))]       # score descending, then best row ascending
        part = order[o[q]:o[q] + k]
        sc[q, :len(part)], ids[q, :len(part)], gr[q, :len(part)] = E[q][part], best[q][part], part
    return sc, ids, gr


def check_docs(S_row, offsets, mask_row, scores, ids, groups, o, tol=TOL, atol=ATOL):
    """the fp64 bar for one query: what the library returned at offset o against its fp64 score row S_row [n] -> (entries,
    positions whose document differs from the reference's window, largest |score - fp64 document score|, first violation or None)"""
    E, _, present = present_best(S_row[None, :], offsets, None if mask_row is None else np.asarray(mask_row)[None, :])
    E, present = E[0], present[0]
    groups, ids = np.asarray(groups, dtype=np.int64), np.asarray(ids, dtype=np.int64)
    live = groups >= 0
    nd = int(present.sum())
    assert live.sum() == max(0, min(len(groups), nd - o)) and live[:live.sum()].all(), "the window's length is exact"
    assert ((ids >= 0) == live).all() and np.isneginf(np.asarray(scores)[~live]).all()
    got, rows = groups[live], ids[live]
    assert present[got].all() and len(set(got.tolist())) == len(got)
    off = np.asarray(offsets, dtype=np.int64)
    assert ((off[got] <= rows) & (rows < off[got + 1])).all(), "a best row lies inside its document"
    if mask_row is not None:
        assert np.asarray(mask_row, dtype=bool)[rows].all(), "a best row is an allowed row"
    s = E[got]
    lo, hi = intervals(E[present], s, tol)
    pos = o + np.arange(len(got))
    err = float(np.abs(np.asarray(scores, dtype=np.float64)[live] - s).max()) if len(got) else 0.0
    bad = np.flatnonzero((pos < lo) | (pos > hi) | (np.abs(S_row[rows] - s) > tol) | (np.abs(np.asarray(scores, dtype=np.float64)[live] - s) > atol))
    want = group_window_ref(S_row[None, :], offsets, None if mask_row is None else np.asarray(mask_row)[None, :], o, len(groups))[2][0][live]
    first = None if len(bad) == 0 else (int(bad[0]), int(got[bad[0]]), int(lo[bad[0]]), int(hi[bad[0]]))
    return len(got), int((got != want).sum()), err, first


def widened(S, offsets, mask, o, k, tol=TOL):
    """-> (entries, intervals wider than one position) over the documents of the reference's own windows [o, o + k) of every
    query of S; the reference's own position always lies inside its interval"""
    E, _, present = present_best(S, offsets, mask)
    gr = group_window_ref(S, offsets, mask, o, k)[2]
    entries = wide = 0
    for q in range(len(S)):
        g = gr[q][gr[q] >= 0]
        lo, hi = intervals(E[q][present[q]], E[q][g], tol)
        pos = o + np.arange(len(g))
        assert ((lo <= pos) & (pos <= hi)).all()
        entries += len(g); wide += int((hi > lo).sum())
    return entries, wide


K_FP64 = 100
# the windows of the fp64 test (k = 100 each): name -> (offset, filter density or None, (entries, widened intervals)) — what the
# reference alone says about its own windows at TOL = 6e-7
TABLE = {
    "unit-5000x37x256-mean7": [(0, None, (3700, 10)), (300, None, (3700, 27)), (200, 0.5, (3700, 21))],
    "unit-3001x300x128-mean3": [(500, None, (30000, 209))],
    "unit-2000x8x2304-mean5": [(100, 0.5, (800, 10))],
    "decks-256": [(100, None, (1600, 6))],
    "decks-2304": [(100, None, (1600, 8))],
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (C, Q, offsets, S fp64) of a TABLE entry; read-only, shared between tests"""
    if name.startswith("decks-"):
        dim = int(name.split("-")[1])
        C, off = R.decks(300, 10, dim, 3e-4)
        Q = R.unit(16, dim, 2)
    else:
        shape, mean = name.split("-")[1:]
        nd, nq, dim = (int(x) for x in shape.split("x"))
        C, Q = R.unit(nd, dim, 1), R.unit(nq, dim, 2)
        off = R.random_offsets(nd, int(mean[4:]))
    return R.frozen(C, Q, off, R.scores64(Q, C))


def case_mask(name, density):
    """the one filter of a TABLE row: bool [rows] or None"""
    return None if density is None else F.random_filters(len(case(name)[0]), (density,), seed=11)[0]
