"""Plain numpy statement of the document-level search (include/visrag_hip.h: vr_index_search_groups), the reference of
tests/test_gpu_group_search.py, and the corpora that file runs it on.  Scores are fp64 dot products of the fp32 data; rows of
the index are partitioned into groups of adjacent rows by `offsets`; a group's score is its best row's, the lowest row id among
equal scores; groups rank by score, the lower best row id first among equal scores.  tests/test_cpu_group_search_ref.py pins it
on hand-worked cases.  Nothing here needs a GPU or the built library."""
import functools

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


@functools.lru_cache(maxsize=None)
def tie_tier(n=3000, dim=64, n_high=100, nq=3, k=150):
    """A tie tier at the selection threshold with rows above it: n - n_high rows are bit-identical copies of one unit vector t,
    the n_high rows at ids 7 i + 3 are distinct and score above t for every query.  -> (C, Q, ids [nq][k]): the row search's
    answer, the high rows in fp64 order and then the lowest tied ids ascending.  Read-only, shared between tests.
    t = (+-1/8, ...) and the queries are fp32: a score of t is a sum of 64 terms that fp64 adds exactly in any order, so the
    tied rows tie in the fp64 reference too.  With t, u and the queries' own noise mutually orthogonal and every v_i orthogonal
    to them, high row i = cos(th_i) u + sin(th_i) v_i scores cos(th_i) (q . u) and t scores 0.3 (q . u): the construction is
    checked below all the same."""
    rng = np.random.default_rng(21)
    t = np.where(rng.standard_normal(dim) < 0, -0.125, 0.125)
    basis = [t]

    def fresh(keep):                                    # a unit vector orthogonal to the basis (and one more of it)
        v = rng.standard_normal(dim)
        for b in basis:
            v -= np.dot(v, b) * b
        v /= np.linalg.norm(v)
        if keep:
            basis.append(v)
        return v

    u = fresh(True)
    Q = np.stack([u + 0.3 * t + 0.05 * (j + 1) * fresh(True) for j in range(nq)])
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    high = 7 * np.arange(n_high) + 3
    th = 0.2 + 0.008 * rng.permutation(n_high)          # (score order is not id order)
    C = np.tile(t.astype(np.float32), (n, 1))
    C[high] = np.stack([np.cos(a) * u + np.sin(a) * fresh(False) for a in th]).astype(np.float32)
    assert high[-1] < n and k > n_high
    S = scores64(Q, C)
    tied = np.setdiff1d(np.arange(n), high)
    assert (S[:, tied] == S[:, tied[:1]]).all()                              # one tier, exactly
    assert (S[:, high].min(1) - S[:, tied[0]] > 1e-2).all()                  # every high row beats it clearly
    assert (np.diff(np.sort(S[:, high], axis=1), axis=1) > 1e-4).all()       # no near-tie among the high rows
    order = np.take_along_axis(np.broadcast_to(high, (nq, n_high)), np.argsort(-S[:, high], axis=1), 1)
    ids = np.concatenate([order, np.broadcast_to(tied[: k - n_high], (nq, k - n_high))], axis=1).astype(np.int64)
    return frozen(C, Q, ids)
