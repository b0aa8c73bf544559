"""Plain numpy statement of the range search (include/visrag_hip.h: vr_index_search_range), the reference of
tests/test_gpu_range_search.py, and the corpora that file runs it on.  Scores are fp64 dot products of the fp32 data
(group_search_ref.scores64); query q's result is every row with score >= float64(float32(threshold[q])), among the rows its filter
allows when a filter is given (a bool row mask; filter_of_query[q] = -1: no filter); the result is CSR (lims, scores, ids) with a
query's entries in ascending row id.  tests/test_cpu_range_search_ref.py pins it on hand-worked cases.  Nothing here needs a GPU
or the built library."""
import functools

import numpy as np

from tests.group_search_ref import decks, frozen, scores64, unit


def thresholds_of(threshold, nq):
    """a scalar or [nq] -> float32 [nq]: the values the library compares with"""
    t = np.asarray(threshold, dtype=np.float32).reshape(-1)
    t = np.full(nq, t[0], dtype=np.float32) if t.size == 1 else t
    assert len(t) == nq
    return t


def membership(S, threshold, masks=None, filter_of_query=None):
    """S [nq][n] fp64 -> bool [nq][n]: row i belongs to query q's result"""
    S = np.asarray(S, dtype=np.float64)
    keep = S >= thresholds_of(threshold, len(S)).astype(np.float64)[:, None]
    if filter_of_query is not None:
        masks = np.asarray(masks, dtype=bool)
        for q, f in enumerate(np.asarray(filter_of_query).reshape(-1)):
            if f >= 0:
                keep[q] &= masks[f]
    return keep


def range_ref(Q, C, threshold, masks=None, filter_of_query=None):
    """-> (lims i64 [nq + 1], scores f64 [total], ids i64 [total]), ascending id inside a query"""
    S = scores64(Q, C)
    keep = membership(S, threshold, masks, filter_of_query)
    lims = np.concatenate([np.zeros(1, np.int64), np.cumsum(keep.sum(1))]).astype(np.int64)
    qs, ids = np.nonzero(keep)                             # row-major: query after query, ids ascending
    return lims, S[qs, ids], ids.astype(np.int64)


def sort_ranges(lims, scores, ids):
    """every segment by score descending, then id ascending: the order HipIndex.search_range(sort=True) returns"""
    seg = np.repeat(np.arange(len(lims) - 1), np.diff(lims))
    order = np.lexsort((ids, -np.asarray(scores, dtype=np.float64), seg))
    return lims, np.asarray(scores)[order], np.asarray(ids)[order]


# ---------------------------------------------------------------------------------------------------- corpora ---
@functools.lru_cache(maxsize=None)
def random_case(nd, nq, dim, cycle):
    """unit rows and queries, thresholds cycling per query -> (C, Q, t f32 [nq], S fp64); read-only, shared between tests"""
    C, Q = unit(nd, dim, 1), unit(nq, dim, 2)
    t = np.asarray(cycle, dtype=np.float32)[np.arange(nq) % len(cycle)]
    return frozen(C, Q, t, scores64(Q, C))


FAMILY_NOISE = {64: 0.02, 2304: 0.004}
FAMILY_MEDIAN = {64: 0.97579408, 2304: 0.96454531}         # the median score of a query against its own family


@functools.lru_cache(maxsize=None)
def families(dim):
    """4 families x 1500 near-identical rows (group_search_ref.decks) followed by 2000 unrelated unit rows; two queries per
    family: its base vector plus noise, renormalised -> (C, Q, S fp64).  A family is beyond what a top-k search can return."""
    noise = FAMILY_NOISE[dim]
    C = np.concatenate([decks(4, 1500, dim, noise)[0], unit(2000, dim, 9)])
    base = np.repeat(unit(4, dim, 5), 2, axis=0)
    Q = base + np.float32(noise) * np.random.default_rng(8).standard_normal((8, dim)).astype(np.float32)
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    return frozen(C, Q, scores64(Q, C))


@functools.lru_cache(maxsize=None)
def scaled_norms(nd=4000, nq=20, dim=256):
    """unit rows scaled to norms U[0.5, 3]: the error model's max |d| is not 1 -> (C, Q, S fp64)"""
    C = (unit(nd, dim, 1) * np.random.default_rng(14).uniform(0.5, 3.0, size=(nd, 1))).astype(np.float32)
    Q = unit(nq, dim, 2)
    return frozen(C, Q, scores64(Q, C))
