"""Plain numpy statement of the document-level search (include/visrag_hip.h: vr_index_search_groups), the reference of
tests/test_gpu_group_search.py, and the corpora that file runs it on.  Scores are fp64 dot products of the fp32 data; rows of
the index are partitioned into groups of adjacent rows by `offsets`; a group's score is its best row's, the lowest row id among
equal scores; groups rank by score, the lower best row id first among equal scores.  tests/test_cpu_group_search_ref.py pins it
on hand-worked cases.  Nothing here needs a GPU or the built library."""
import numpy as np


def unit(n, d, seed):
    """tests/test_gpu_search.py::_unit"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def random_offsets(n, mean, seed=3):
    """group lengths drawn one by one from [1, 2 * mean) until the n rows are used up, the last one clipped"""
    rng = np.random.default_rng(seed)
    off = [0]
    while off[-1] < n:
        off.append(min(n, off[-1] + int(rng.integers(1, 2 * mean))))
    return np.asarray(off, dtype=np.int64)


def decks(n_docs, pages, dim, noise, base_seed=5, noise_seed=6):
    """near-duplicate decks: page = its document's unit vector + noise * N(0, 1), renormalised -> (C f32, offsets)"""
    base = unit(n_docs, dim, base_seed)
    z = np.random.default_rng(noise_seed).standard_normal((n_docs * pages, dim)).astype(np.float32)
    c = np.repeat(base, pages, axis=0) + np.float32(noise) * z
    c = (c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32)
    return c, np.arange(n_docs + 1, dtype=np.int64) * pages


def scores64(Q, C):
    return np.asarray(Q, np.float32).astype(np.float64) @ np.asarray(C, np.float32).astype(np.float64).T


def group_best(S, offsets):
    """S [nq][n] -> (E [nq][n_groups] the groups' maxima, best [nq][n_groups] the LOWEST row that attains each)"""
    off = np.asarray(offsets, dtype=np.int64)
    n = S.shape[1]
    assert off[0] == 0 and off[-1] == n and (np.diff(off) > 0).all()
    E = np.maximum.reduceat(S, off[:-1], axis=1)
    gid = np.repeat(np.arange(len(off) - 1), np.diff(off))
    rows = np.where(S == E[:, gid], np.arange(n)[None, :], n)
    return E, np.minimum.reduceat(rows, off[:-1], axis=1)


def group_topk_ref(Q, C, offsets, k):
    """-> (scores f64 [nq][k], best row ids i64 [nq][k], groups i64 [nq][k]); fewer than k groups: tail (-inf, -1, -1)"""
    E, best = group_best(scores64(Q, C), offsets)
    nq, ng = E.shape
    order = np.lexsort((best, -E), axis=1)[:, :k]          # score descending, then best row ascending
    kk = order.shape[1]
    sc = np.full((nq, k), -np.inf)
    ids = np.full((nq, k), -1, dtype=np.int64)
    gr = np.full((nq, k), -1, dtype=np.int64)
    sc[:, :kk] = np.take_along_axis(E, order, 1)
    ids[:, :kk] = np.take_along_axis(best, order, 1)
    gr[:, :kk] = order
    return sc, ids, gr


def frozen(*arrays):
    """shared between tests: read-only"""
    for a in arrays:
        a.setflags(write=False)
    return arrays
