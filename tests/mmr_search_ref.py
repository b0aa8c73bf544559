"""Plain numpy statement of the diversified search (include/visrag_hip.h: vr_index_search_diverse), the reference of
tests/test_gpu_mmr_search.py.  Everything is fp64 arithmetic on the fp32 data.  Per query: the pool is the first `pool` rows of
the ranking (score descending, then row id ascending; with a filter, of the rows it allows), rows that do not exist are no
members; pick 0 is pool position 0; pick t >= 1 is the unselected member of largest
    v = lam * r - (1 - lam) * max over the picked rows of <d, d_picked>,
the lower pool position among equal v; the result holds the picks in pick order with their relevance r, tail (-inf, -1).
`walk` is the test of a result that need not be the reference's: every pick epsilon-optimal given its own prefix.
tests/test_cpu_mmr_search_ref.py pins both on hand-worked cases.  Nothing here needs a GPU or the built library."""
import functools

import numpy as np

from tests.filter_search_ref import masked_scores
from tests.group_search_ref import decks, frozen, scores64, unit


def pools(Q, C, pool, masks=None, foq=None):
    """-> (S f64 [nq][n] masked scores, order i64 [nq][min(pool + 1, n)]): the ranking's first pool rows AND the row behind
    them (pool_boundary_gaps); entries whose score is -inf are no members"""
    S = scores64(Q, C)
    if masks is not None and foq is not None:
        S = masked_scores(S, masks, foq)
    n = S.shape[1]
    order = np.lexsort((np.broadcast_to(np.arange(n), S.shape), -S), axis=1)[:, : pool + 1]
    return S, order


def pool_boundary_gaps(Q, C, pool, masks=None, foq=None):
    """per query: score of the pool's last member - score of the best row left out (inf: nothing is left out)"""
    S, order = pools(Q, C, pool, masks, foq)
    gaps = np.full(len(S), np.inf)
    for q in range(len(S)):
        s = S[q][order[q]]
        if len(s) > pool and np.isfinite(s[pool]):
            gaps[q] = s[pool - 1] - s[pool]
    return gaps


def mmr_ref(Q, C, k, pool, lam, masks=None, foq=None):
    """-> (scores f64 [nq][k], ids i64 [nq][k], margins f64 [nq]); margins[q] = the smallest gap between the best and the
    second-best v over the picks t >= 1 of query q (inf where no pick had a rival)"""
    assert 1 <= k <= pool
    S, order = pools(Q, C, pool, masks, foq)
    C64 = np.asarray(C, np.float32).astype(np.float64)
    nq = len(S)
    sc = np.full((nq, k), -np.inf)
    ids = np.full((nq, k), -1, dtype=np.int64)
    margins = np.full(nq, np.inf)
    for q in range(nq):
        members = order[q][:pool]
        members = members[np.isfinite(S[q][members])]
        if len(members) == 0:
            continue
        r = S[q][members]
        D = C64[members]
        m = np.full(len(members), -np.inf)
        free = np.ones(len(members), dtype=bool)
        b = 0
        for t in range(min(k, len(members))):
            if t > 0:
                m = np.maximum(m, D @ D[b])
                v = np.where(free, lam * r - (1.0 - lam) * m, -np.inf)
                b = int(np.argmax(v))                                   # (the first maximum: the lower pool position)
                if free.sum() > 1:
                    margins[q] = min(margins[q], v[b] - np.partition(v, -2)[-2])
            free[b] = False
            sc[q, t], ids[q, t] = r[b], members[b]
    return sc, ids, margins


def walk(Q, C, ids, pool, lam, masks=None, foq=None):
    """A result `ids` [nq][k] (pick order, -1 tail) against the semantics, pick by pick, each GIVEN THE ROWS RETURNED BEFORE IT:
    -> (deficit f64 [nq][k], outside f64 [nq][k]).  deficit[q][t] = (the largest fp64 v among the reference pool's members not
    returned before t) - (the fp64 v of the row returned at t); for t = 0 the objective is the relevance alone.  outside[q][t] =
    0 for a member of the reference pool, else (score of the pool's last member) - (score of the returned row).  Both are nan
    at the -1 tail.  A result that returns a row twice, a row that does not exist or a row its filter does not allow raises."""
    S, order = pools(Q, C, pool, masks, foq)
    C64 = np.asarray(C, np.float32).astype(np.float64)
    ids = np.asarray(ids)
    deficit = np.full(ids.shape, np.nan)
    outside = np.full(ids.shape, np.nan)
    for q in range(len(S)):
        members = order[q][:pool]
        members = members[np.isfinite(S[q][members])]
        got = ids[q][ids[q] >= 0]
        assert (ids[q][len(got):] == -1).all(), (q, "a pick behind the tail")
        assert len(got) == min(ids.shape[1], len(members)), (q, len(got), len(members))
        assert len(set(got.tolist())) == len(got) and (got < len(C64)).all(), (q, "a row twice / no such row")
        assert np.isfinite(S[q][got]).all(), (q, "a row the filter does not allow")
        r = S[q][members]
        D = C64[members]
        m = np.full(len(members), -np.inf)
        m_got = np.full(len(got), -np.inf)
        free = np.ones(len(members), dtype=bool)
        for t, row in enumerate(got):
            if t > 0:
                prev = C64[got[t - 1]]
                m = np.maximum(m, D @ prev)
                m_got = np.maximum(m_got, C64[got] @ prev)
                best = np.where(free, lam * r - (1.0 - lam) * m, -np.inf).max()
                mine = lam * S[q][row] - (1.0 - lam) * m_got[t]
            else:
                best, mine = r[0], S[q][row]
            deficit[q, t] = best - mine
            at = np.flatnonzero(members == row)
            outside[q, t] = 0.0 if len(at) else r[-1] - S[q][row]
            free[at] = False
    return deficit, outside


@functools.lru_cache(maxsize=None)
def random_case(nd, nq, dim, k, pool, lam):
    """unit(nd, dim, 1) rows, unit(nq, dim, 2) queries -> (C, Q, (scores, ids, margins)); read-only, shared between tests"""
    C, Q = unit(nd, dim, 1), unit(nq, dim, 2)
    return frozen(C, Q) + (frozen(*mmr_ref(Q, C, k, pool, lam)),)


@functools.lru_cache(maxsize=None)
def deck_case(dim, noise, nq=48, k=10, pool=100, lam=0.5):
    """decks(300, 10, dim, noise), unit(nq, dim, 2) queries -> (C, Q, (scores, ids, margins)); read-only"""
    C, _ = decks(300, 10, dim, noise)
    Q = unit(nq, dim, 2)
    return frozen(C, Q) + (frozen(*mmr_ref(Q, C, k, pool, lam)),)
