"""Plain numpy statement of the document rank search (include/visrag_hip.h: vr_index_rank_groups / vr_index_count_groups_range),
the reference of tests/test_gpu_group_rank_search.py.  The ranking is the document window search's
(group_window_search_ref.present_best / ordered): a document (group of adjacent rows) is present for a query if the query's mask
allows one of its pages; it scores as its best ALLOWED page does, its best row is the lowest allowed row that attains that score;
present documents rank score descending, then lower group first.  The rank of a present document is the number of present
documents ahead of it; a document the mask leaves no page of is not in the ranking: (-inf, -1, -1).  A count is the number of
present documents with score >= t, or > t when strict (-0.0 == +0.0: a float compare).

Against fp64 the library's result is held to the rank search's interval (rank_search_ref.interval) with no excuse mechanism: the
rank returned for a document of fp64 score s lies in [#(E > s + TOL), #(E >= s - TOL) - 1] over the present documents (TOL =
6e-7), its score within 1e-5 of s and its best row's fp64 score within TOL of s.  tests/test_cpu_group_rank_search_ref.py pins
how many of these intervals are wider than one position on the corpora the GPU test uses.  Nothing here needs a GPU or the
built library."""
import numpy as np

from tests import group_window_search_ref as G
from tests.rank_search_ref import TOL, interval

ATOL = G.ATOL


def group_rank_ref(S, offsets, mask, groups):
    """S [nq][n] (fp64, or the library's own fp32 scores: ranked on their orderable bits), mask bool [nq][n] / [n] / None, groups
    int [nq][T] -> (scores [nq][T] of S's dtype, best rows i64 [nq][T], ranks i64 [nq][T]); (-inf, -1, -1) for an absent target"""
    S = np.asarray(S)
    E, best, present = G.present_best(S, offsets, mask)
    groups = np.asarray(groups, dtype=np.int64)
    nq, T = groups.shape
    key = G.ordered(E)
    sc = np.full((nq, T), -np.inf, dtype=S.dtype)
    rows = np.full((nq, T), -1, dtype=np.int64)
    rk = np.full((nq, T), -1, dtype=np.int64)
    for q in range(nq):
        g = np.flatnonzero(present[q])
        order = g[np.lexsort((g, -key[q][g]))]                # score descending, then group ascending
        pos = np.full(E.shape[1], -1, dtype=np.int64)
        pos[order] = np.arange(len(order))
        t = groups[q]
        sc[q], rows[q], rk[q] = np.where(present[q][t], E[q][t], -np.inf), best[q][t], pos[t]
    return sc, rows, rk


def group_count_ref(S, offsets, mask, t, strict=False):
    """t [nq][T] (taken as fp32 values) -> int64 [nq][T]: present documents with score >= t (> t when strict)"""
    E, _, present = G.present_best(np.asarray(S), offsets, mask)
    t = np.asarray(t, dtype=np.float32).astype(E.dtype)
    hit = (E[:, None, :] > t[:, :, None]) if strict else (E[:, None, :] >= t[:, :, None])
    return (hit & present[:, None, :]).sum(-1).astype(np.int64)


def targets(S, offsets, mask):
    """the targets of the fp64 test: every 7th document plus the reference's top 20 of every query -> int64 [nq][T] (the same T
    for every query: the top 20 are appended, duplicates allowed)"""
    ng = len(offsets) - 1
    top = G.group_window_ref(S, offsets, mask, 0, 20)[2]
    top = np.where(top >= 0, top, 0)
    spread = np.broadcast_to(np.arange(0, ng, 7, dtype=np.int64), (len(S), len(range(0, ng, 7))))
    return np.ascontiguousarray(np.concatenate([spread, top], axis=1))


def check_ranks(S, offsets, mask, groups, scores, rows, ranks, tol=TOL, atol=ATOL):
    """the fp64 bar over a whole call: what the library returned for `groups` [nq][T] against the fp64 scores S -> (pairs, ranks
    that differ from the fp64 rank, largest |score - fp64 document score|, first violation or None)"""
    E, _, present = G.present_best(S, offsets, mask)
    want = group_rank_ref(S, offsets, mask, groups)[2]
    off = np.asarray(offsets, dtype=np.int64)
    allowed = None if mask is None else np.broadcast_to(np.asarray(mask, dtype=bool), np.asarray(S).shape)
    differ, err, first = 0, 0.0, None
    for q in range(len(S)):
        Ep = E[q][present[q]]
        for j, g in enumerate(np.asarray(groups[q], dtype=np.int64)):
            sc, r, rk = float(scores[q][j]), int(rows[q][j]), int(ranks[q][j])
            if not present[q][g]:
                ok = np.isneginf(sc) and r == -1 and rk == -1
            else:
                s = E[q][g]
                lo, hi = interval(Ep, s, tol)
                ok = off[g] <= r < off[g + 1] and (allowed is None or allowed[q][r]) and lo <= rk <= hi and \
                    abs(S[q][r] - s) <= tol and abs(sc - s) <= atol
                err = max(err, abs(sc - s))
                differ += int(rk != want[q][j])
            if not ok and first is None:
                first = (q, int(g), sc, r, rk)
    return int(np.asarray(groups).size), differ, err, first


def interval_table(S, offsets, mask, tol=TOL):
    """-> (pairs, absent targets, widened intervals, max width) over `targets`; width = hi - lo; the reference's own rank always
    lies inside its interval"""
    E, _, present = G.present_best(S, offsets, mask)
    T = targets(S, offsets, mask)
    rk = group_rank_ref(S, offsets, mask, T)[2]
    absent, widths = 0, []
    for q in range(len(S)):
        Ep = E[q][present[q]]
        for j, g in enumerate(T[q]):
            if not present[q][g]:
                absent += 1
                continue
            lo, hi = interval(Ep, E[q][g], tol)
            assert lo <= rk[q][j] <= hi
            widths.append(hi - lo)
    w = np.asarray(widths)
    return int(T.size), absent, int((w > 0).sum()), int(w.max())


# the fp64 test runs on the corpora of group_window_search_ref.TABLE, once per distinct filter density of a corpus' rows there:
#   name -> [(density or None, (pairs, absent targets, widened intervals, max width))] at TOL = 6e-7
TABLE = {
    "unit-5000x37x256-mean7": [(None, (4588, 0, 30, 1)), (0.5, (4588, 296, 22, 1))],
    "unit-3001x300x128-mean3": [(None, (49800, 0, 213, 2))],
    "unit-2000x8x2304-mean5": [(0.5, (624, 104, 5, 1))],
    "decks-256": [(None, (1008, 0, 2, 1))],
    "decks-2304": [(None, (1008, 0, 3, 1))],
}


def table_rows(name):
    """the distinct filter densities of a corpus in group_window_search_ref.TABLE, None first"""
    return sorted({d for _, d, _ in G.TABLE[name]}, key=lambda d: (d is not None, d))
