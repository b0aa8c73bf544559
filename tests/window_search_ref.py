"""Plain numpy statement of the windowed search (include/visrag_hip.h: vr_index_search_window), the reference of
tests/test_gpu_window_search.py.  Scores are fp64 dot products of the fp32 data (group_search_ref.scores64).  The window of query
q at offset o is rows o .. o + k - 1 of its ranking — score descending, then lower id first — over the rows its filter allows;
slots at or past the number of allowed rows are (-inf, -1).

The library ranks by its fp32 scores, the reference by fp64: a row of fp64 score s that the library returns at position j of the
window at offset o must have o + j in `rank_search_ref.interval(S[q], s)` = [#(S > s + TOL), #(S >= s - TOL) - 1] with
TOL = 6e-7 — the rank search's interval bar, on the same grounds (two fp32 scores are compared, each inside the project's
NEAR_TIE = 3e-7).  tests/test_cpu_window_search_ref.py pins how wide these intervals are for the rows of the reference's own
windows on the corpora the GPU test uses.  Nothing here needs a GPU or the built library."""
import numpy as np

from tests.rank_search_ref import TOL, case, ranking  # noqa: F401  (the corpora and the ranking order are the rank search's)


def window_ref(S_row, o, k, mask=None):
    """-> (scores f64 [k], ids i64 [k]): ranks [o, o + k) of one query's scores among the rows of `mask`; tails (-inf, -1)"""
    S_row = np.asarray(S_row, dtype=np.float64)
    order = ranking(S_row)
    if mask is not None:
        order = order[np.asarray(mask, dtype=bool)[order]]
    ids = np.full(k, -1, dtype=np.int64)
    sc = np.full(k, -np.inf, dtype=np.float64)
    part = order[o:o + k]
    ids[:len(part)], sc[:len(part)] = part, S_row[part]
    return sc, ids


def intervals(S_row, s, tol=TOL):
    """vectorised rank_search_ref.interval: s [m] fp64 scores -> (lo [m], hi [m]) with lo = #(S > s + tol), hi = #(S >= s - tol) - 1"""
    asc = np.sort(np.asarray(S_row, dtype=np.float64))
    s = np.asarray(s, dtype=np.float64)
    lo = len(asc) - np.searchsorted(asc, s + tol, side="right")
    hi = len(asc) - np.searchsorted(asc, s - tol, side="left") - 1
    return lo, hi


def check_window(S_row, ids, o, tol=TOL):
    """the bar of the fp64 test for one query: ids [k] as the library returned them at offset o -> (entries, positions that differ
    from the reference's window, first violation or None)"""
    ids = np.asarray(ids, dtype=np.int64)
    live = ids >= 0
    n = len(S_row)
    assert live.sum() == max(0, min(len(ids), n - o)) and live[:live.sum()].all(), "the window's length is exact"
    got = ids[live]
    lo, hi = intervals(S_row, np.asarray(S_row)[got], tol)
    pos = o + np.arange(len(got))
    bad = np.flatnonzero((pos < lo) | (pos > hi))
    want = window_ref(S_row, o, len(ids))[1][live]
    return len(got), int((got != want).sum()), (None if len(bad) == 0 else (int(bad[0]), int(got[bad[0]]), int(lo[bad[0]]), int(hi[bad[0]])))


def interval_table(S, o, k, tol=TOL):
    """-> (entries, widened intervals, max width) over the rows of the reference's own windows [o, o + k) of every query of S;
    width = hi - lo, and the reference's own position always lies inside"""
    entries = widened = widest = 0
    for q in range(len(S)):
        ids = window_ref(S[q], o, k)[1]
        ids = ids[ids >= 0]
        lo, hi = intervals(S[q], S[q][ids], tol)
        pos = o + np.arange(len(ids))
        assert ((lo <= pos) & (pos <= hi)).all()
        w = hi - lo
        entries += len(ids); widened += int((w > 0).sum()); widest = max(widest, int(w.max()) if len(w) else 0)
    return entries, widened, widest


K_FP64 = 100
# the windows of the fp64 test (k = 100 each) and what the reference alone says about them at TOL = 6e-7:
#   name -> {offset: (entries, widened intervals, max width)}
# The family corpora hold 4 x 1500 near-identical rows: offset 1450 straddles the end of a query's own family, where 1 500 scores
# crowd into a few 1e-3 — the densest part of any ranking in the suite.
TABLE = {
    "unit-5000x37x256": {0: (3700, 9, 1), 2500: (3700, 112, 1)},
    "unit-3001x300x128": {0: (30000, 50, 1), 2500: (30000, 290, 1)},
    "unit-20000x64x2304": {10000: (6400, 2389, 4)},         # the middle of 20 000 scores of spread 0.02: the widest is 4, not <= 3
    "families-64": {0: (800, 39, 2), 1450: (800, 4, 1)},
    "families-2304": {0: (800, 97, 2), 1450: (800, 52, 2)},
}
