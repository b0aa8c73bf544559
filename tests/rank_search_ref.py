"""Plain numpy statement of the rank search (include/visrag_hip.h: vr_index_rank_rows / vr_index_count_range), the reference of
tests/test_gpu_rank_search.py.  Scores are fp64 dot products of the fp32 data (group_search_ref.scores64).  The rank of row i for
query q is the number of rows j — allowed by the query's filter when one is given — that come before it in the ranking order:
score descending, then lower id first.  A count is the number of (allowed) rows with score >= t, or > t when strict.

The library ranks by its fp32 scores, the reference by fp64: the rank the library returns for a target of fp64 score s must lie in
`interval(S[q], s)` = [#(S > s + TOL), #(S >= s - TOL) - 1] with TOL = 6e-7 — twice the project's NEAR_TIE = 3e-7, because two
fp32 scores are compared and each lies inside that standing bar.  tests/test_cpu_rank_search_ref.py pins how wide these
intervals are on the corpora the GPU test uses.  Nothing here needs a GPU or the built library."""
import functools

import numpy as np

from tests import range_search_ref as X
from tests.group_search_ref import frozen, scores64, unit

TOL = 6e-7          # 2 x NEAR_TIE


def rank_ref(S_row, i, mask=None):
    """the position of row i in the ranking of one query's scores (among the rows of `mask`, whether or not it allows i)"""
    S_row = np.asarray(S_row)
    ahead = (S_row > S_row[i]) | ((S_row == S_row[i]) & (np.arange(len(S_row)) < i))
    if mask is not None:
        ahead &= np.asarray(mask, dtype=bool)
    return int(ahead.sum())


def ranking(S_row):
    """row ids in ranking order: score descending, then id ascending"""
    return np.lexsort((np.arange(len(S_row)), -np.asarray(S_row, dtype=np.float64)))


def ranks_of_ranking(order):
    """order [n] (row ids, best first) -> rank of every row"""
    r = np.empty(len(order), dtype=np.int64)
    r[np.asarray(order)] = np.arange(len(order))
    return r


def count_ref(S_row, t, strict=False, mask=None):
    t = np.float64(np.float32(t))
    keep = (S_row > t) if strict else (S_row >= t)
    if mask is not None:
        keep = keep & np.asarray(mask, dtype=bool)
    return int(keep.sum())


def targets(S, q):
    """the targets of query q in the fp64 test: the three best rows of the reference and eight rows spread over the index"""
    nd = S.shape[1]
    best = ranking(S[q])[:3]
    spread = [(q * 7919 + j * 104729 + 1) % nd for j in range(8)]
    return np.unique(np.concatenate([best, np.asarray(spread, dtype=np.int64)])).astype(np.int64)


def interval(S_row, s, tol=TOL):
    """[lo, hi]: the ranks a row of fp64 score s may take when every compared pair of fp32 scores is off by less than tol"""
    return int((S_row > s + tol).sum()), int((S_row >= s - tol).sum()) - 1


def all_targets(S):
    """-> (lims i64 [nq + 1], ids i64 [pairs]) of `targets` for every query"""
    per = [targets(S, q) for q in range(len(S))]
    lims = np.concatenate([np.zeros(1, np.int64), np.cumsum([len(p) for p in per])]).astype(np.int64)
    return lims, np.concatenate(per)


def interval_table(S, tol=TOL):
    """-> (pairs, widened intervals, summed width, max width) over all_targets(S); width = hi - lo"""
    lims, ids = all_targets(S)
    widths = []
    for q in range(len(S)):
        for i in ids[lims[q]:lims[q + 1]]:
            lo, hi = interval(S[q], S[q, i], tol)
            assert lo <= rank_ref(S[q], i) <= hi
            widths.append(hi - lo)
    w = np.asarray(widths)
    return len(w), int((w > 0).sum()), int(w.sum()), int(w.max())


# the corpora of the fp64 test and what the reference alone says about them (tests/test_cpu_rank_search_ref.py pins it):
#   name -> (pairs, widened intervals, summed width, max width) at TOL = 6e-7, and the summed width at 3e-7
TABLE = {
    "unit-5000x37x256": ((406, 5, 5, 1), 3),
    "unit-3001x300x128": ((3299, 32, 32, 1), 17),
    "unit-20000x64x2304": ((704, 147, 174, 3), 90),
    "families-64": ((88, 3, 3, 1), 1),
    "families-2304": ((88, 14, 14, 1), 10),
    "norms-4000x20x256": ((220, 3, 3, 1), 0),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (C, Q, S fp64) of a TABLE entry; read-only, shared between tests (the range search's corpora)"""
    if name.startswith("unit-"):
        nd, nq, dim = (int(x) for x in name[5:].split("x"))
        C, Q, _, S = X.random_case(nd, nq, dim, {256: (0.10, 0.15, 0.20, 0.30), 128: (0.15, 0.25, 0.05), 2304: (0.05, 0.07)}[dim])
        return C, Q, S
    if name.startswith("families-"):
        return X.families(int(name[9:]))
    assert name == "norms-4000x20x256"
    return X.scaled_norms()


@functools.lru_cache(maxsize=None)
def shards_case():
    """6 000 x 256 unit rows as three shards of 1 000, 3 001 and 1 999 rows, 50 rows of shard 0 copied bit for bit into shard 2:
    equal scores across shards, where the global tie rule (earlier position first) decides -> (C, Q, bounds)"""
    C = unit(6000, 256, 21).copy()
    src = np.arange(50) * 17 + 5                       # rows of shard 0
    dst = 4001 + np.arange(50) * 31 + 2                # rows of shard 2
    C[dst] = C[src]
    return frozen(C, unit(9, 256, 22)) + ((0, 1000, 4001, 6000),)
