"""Plain numpy statement of the filtered search (include/visrag_hip.h: vr_index_search_filtered), the reference of
tests/test_gpu_filter_search.py.  Scores are fp64 dot products of the fp32 data (group_search_ref.scores64); a filter is a bool
row mask; the rows a query's filter does not allow score -inf; the result is ordered by score descending, then row id ascending,
and the tail beyond the allowed rows is (-inf, -1).  filter_of_query[q] = -1: no filter.  tests/test_cpu_filter_search_ref.py pins
it on hand-worked cases.  Nothing here needs a GPU or the built library."""
import numpy as np

from tests.group_search_ref import scores64


def random_filters(n, densities, seed=11):
    """bool [len(densities)][n]: filter j allows a row with probability densities[j], drawn filter after filter from one stream"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.random(n) < d for d in densities])


def masked_scores(S, masks, filter_of_query):
    """S [nq][n] with the rows query q may not see set to -inf"""
    masks = np.asarray(masks, dtype=bool)
    S = np.array(S, dtype=np.float64)
    for q, f in enumerate(np.asarray(filter_of_query).reshape(-1)):
        if f >= 0:
            S[q, ~masks[f]] = -np.inf
    return S


def filtered_topk_ref(Q, C, masks, filter_of_query, k):
    """-> (scores f64 [nq][k], ids i64 [nq][k]); fewer than k allowed rows: tail (-inf, -1)"""
    S = masked_scores(scores64(Q, C), masks, filter_of_query)
    nq, n = S.shape
    order = np.lexsort((np.broadcast_to(np.arange(n), S.shape), -S), axis=1)[:, :k]      # score descending, then id ascending
    kk = order.shape[1]
    sc = np.full((nq, k), -np.inf)
    ids = np.full((nq, k), -1, dtype=np.int64)
    sc[:, :kk] = np.take_along_axis(S, order, 1)
    ids[:, :kk] = np.where(np.isneginf(sc[:, :kk]), -1, order)
    return sc, ids
