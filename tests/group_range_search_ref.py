"""Plain numpy statement of the document range search (include/visrag_hip.h: vr_index_search_groups_range), the reference of
tests/test_gpu_group_range_search.py.  The semantics are the document window search's and the document count's
(group_window_search_ref.present_best / ordered, range_search_ref.thresholds_of): a document (group of adjacent rows) is present
for a query if the query's mask allows one of its pages; it scores as its best ALLOWED page does, its best row is the lowest
allowed row that attains that score; query q's result is every present document with score >= float32(threshold[q]) — a float
compare, -0.0 == +0.0 — in CSR form (lims, scores, best rows, groups): ascending group inside a query (the ABI's order), or score
descending on the keys' orderable bits, then lower group first (the order HipIndex.search_groups_range(sort=True) returns:
search_groups_window's).

Against fp64 the bar is the row-level range test's: scores within ATOL = 1e-5 of the fp64 document score; the best row's fp64
score within TOL = 6e-7 of that document score; membership identical to the reference's except for a (query, document) pair
whose fp64 score lies within NEAR = 3e-7 of the threshold; excused pairs at most 0.5 % of the entries the reference returns for
the case.  tests/test_cpu_group_range_search_ref.py pins the reference's entries and that it has NO pair within NEAR of its
threshold on the cases of TABLE.  Nothing here needs a GPU or the built library."""
import numpy as np

from tests import group_window_search_ref as G
from tests.range_search_ref import thresholds_of
from tests.rank_search_ref import TOL

ATOL = G.ATOL
NEAR = 3e-7
EXCUSED_SHARE = 0.005


def sort_group_ranges(lims, scores, rows, groups):
    """every segment by score descending on orderable bits, then group ascending"""
    lims, scores, rows, groups = np.asarray(lims), np.asarray(scores), np.asarray(rows), np.asarray(groups)
    seg = np.repeat(np.arange(len(lims) - 1), np.diff(lims))
    key = G.ordered(scores)
    order = np.lexsort((groups, -key, seg))
    return lims, scores[order], rows[order], groups[order]


def group_range_ref(S, offsets, mask, threshold, sort=False):
    """S [nq][n] (fp64, or the library's own fp32 scores), mask bool [nq][n] / [n] / None, threshold a scalar or one per query
    (taken as fp32 values) -> (lims i64 [nq + 1], scores [total] of S's dtype, best rows i64 [total], groups i64 [total])"""
    S = np.asarray(S)
    E, best, present = G.present_best(S, offsets, mask)
    t = thresholds_of(threshold, len(S)).astype(E.dtype)
    keep = present & (E >= t[:, None])
    lims = np.concatenate([np.zeros(1, np.int64), np.cumsum(keep.sum(1))]).astype(np.int64)
    qs, gs = np.nonzero(keep)                               # row-major: query after query, groups ascending
    out = lims, E[qs, gs], best[qs, gs].astype(np.int64), gs.astype(np.int64)
    return sort_group_ranges(*out) if sort else out


def near_threshold(S, offsets, mask, threshold, near=NEAR):
    """(query, present document) pairs whose score lies within `near` of the query's threshold"""
    E, _, present = G.present_best(np.asarray(S, dtype=np.float64), offsets, mask)
    t = thresholds_of(threshold, len(E)).astype(np.float64)
    return int((present & (np.abs(E - t[:, None]) <= near)).sum())


def check_range(S, offsets, mask, threshold, lims, scores, rows, groups, tol=TOL, atol=ATOL, near=NEAR):
    """the fp64 bar over a whole call: what the library returned against the fp64 scores S -> (entries the reference returns,
    excused pairs, largest |score - fp64 document score|, first violation or None)"""
    S = np.asarray(S, dtype=np.float64)
    E, _, present = G.present_best(S, offsets, mask)
    t = thresholds_of(threshold, len(S)).astype(np.float64)
    off = np.asarray(offsets, dtype=np.int64)
    allowed = None if mask is None else np.broadcast_to(np.asarray(mask, dtype=bool), S.shape)
    lims, scores, rows, groups = (np.asarray(x) for x in (lims, scores, rows, groups))
    want = present & (E >= t[:, None])
    excused, err, first = 0, 0.0, None
    assert lims[0] == 0 and lims[-1] == len(groups) == len(rows) == len(scores) and (np.diff(lims) >= 0).all()
    for q in range(len(S)):
        g, r, sc = groups[lims[q]:lims[q + 1]], rows[lims[q]:lims[q + 1]], scores[lims[q]:lims[q + 1]].astype(np.float64)
        got = np.zeros(E.shape[1], dtype=bool)
        got[g] = True
        bad = None
        if got.sum() != len(g) or not present[q][g].all():
            bad = (q, "a document twice, or an absent one")
        differ = np.flatnonzero(got != want[q])
        far = differ[np.abs(E[q][differ] - t[q]) > near]
        excused += len(differ) - len(far)
        if bad is None and len(far):
            bad = (q, int(far[0]), float(E[q][far[0]]), float(t[q]))
        if bad is None and len(g):
            inside = (off[g] <= r) & (r < off[g + 1]) & (True if allowed is None else allowed[q][np.clip(r, 0, S.shape[1] - 1)])
            ok = inside & (np.abs(S[q][np.clip(r, 0, S.shape[1] - 1)] - E[q][g]) <= tol) & (np.abs(sc - E[q][g]) <= atol)
            err = max(err, float(np.abs(sc - E[q][g]).max()))
            if not ok.all():
                j = int(np.flatnonzero(~ok)[0])
                bad = (q, int(g[j]), float(sc[j]), int(r[j]))
        if bad is not None and first is None:
            first = bad
    return int(want.sum()), excused, err, first


# the cases of the fp64 test, on the corpora of group_window_search_ref.case: name -> (thresholds cycling per query, entries
# without a filter, entries under the density-0.5 filter of group_window_search_ref.case_mask, (min, median, max) entries per
# query without a filter); the reference has NO pair within NEAR of its threshold in any of them
TABLE = {
    "unit-5000x37x256-mean7": ((0.10, 0.15, 0.20, 0.30), 2644, 1430, (0, 25, 238)),
    "unit-3001x300x128-mean3": ((0.15, 0.25, 0.05), 73596, 43193, (1, 127, 639)),
    "unit-2000x8x2304-mean5": ((0.05, 0.07), 68, 31, (0, 6, 21)),
    "decks-256": ((0.10, 0.15, 0.20), 106, 105, (0, 2, 18)),
    "decks-2304": ((0.03, 0.05, 0.07), 157, 154, (0, 2, 33)),
}


def case_thresholds(name, nq):
    """float32 [nq]: the case's thresholds, cycling per query"""
    cycle = np.asarray(TABLE[name][0], dtype=np.float32)
    return cycle[np.arange(nq) % len(cycle)]
