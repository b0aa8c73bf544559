"""Plain numpy statement of the fused document search (include/visrag_hip.h: vr_index_search_multi_groups), the reference of
tests/test_gpu_multi_group_search.py.  Question g holds sub-queries lims[g] .. lims[g + 1] - 1; a document (group of adjacent
rows) is present for it if its mask allows one of the document's pages; per sub-query j the document scores E_j(D) = its best
ALLOWED page's score, row_j(D) the lowest allowed row attaining it; F(D) = max_j E_j(D) ("any-of") or min_j E_j(D) ("all-of");
which(D) = the lowest j with E_j(D) == F(D), best_row(D) = row_which(D).  Present documents rank by F descending, then lower
document first; slots past them hold (-inf, -1, -1, -1), their evidence entries (-inf, -1).  Built on
group_search_ref.group_best, group_window_search_ref.ordered and multi_search_ref.layout: a score matrix of float32 (the library's own) is
compared on its orderable bits (-0.0 < +0.0), any other dtype as it is.

Against fp64 the library's result is held to the rank search's interval, with no excuse mechanism (TOL = 6e-7, two fp32 scores
are compared; scores within ATOL = 1e-5): see check_question.  Nothing here needs a GPU or the built library."""
import functools

import numpy as np

from tests import filter_search_ref as FS
from tests import group_search_ref as R
from tests.group_window_search_ref import ATOL, ordered
from tests.multi_search_ref import layout  # noqa: F401  (the layouts are the fused search's)
from tests.rank_search_ref import TOL
from tests.window_search_ref import intervals


def per_sub(S, lims, offsets, mask=None):
    """S [n_sub][rows]; mask: None, one bool [rows] for every question, or per question a bool [rows] or None
    -> (K [n_sub][n_docs] the documents' best allowed score as an orderable key (S itself unless float32), row [n_sub][n_docs]
    the lowest allowed row attaining it (-1: absent), present bool [n_questions][n_docs])"""
    S = np.asarray(S)
    lims = np.asarray(lims, dtype=np.int64)
    nq = len(lims) - 1
    if mask is not None and not isinstance(mask, (list, tuple)) and np.asarray(mask).ndim == 1:
        mask = [mask] * nq
    K = ordered(S)
    lowest = np.int64(-1) if S.dtype == np.float32 else -np.inf
    off = np.asarray(offsets, dtype=np.int64)
    Ks, rows, present = [], [], []
    for g in range(nq):
        m = np.ones(S.shape[1], dtype=bool) if mask is None or mask[g] is None else np.asarray(mask[g], dtype=bool)
        E, best = R.group_best(np.where(m[None, :], K[lims[g]:lims[g + 1]], lowest), off)
        pres = np.maximum.reduceat(m, off[:-1])
        Ks.append(E); rows.append(np.where(pres[None, :], best, -1)); present.append(pres)
    return np.concatenate(Ks), np.concatenate(rows), np.stack(present)


def multi_group_ref(S, lims, offsets, k, fuse, mask=None):
    """-> (scores [nq][k] of S's dtype, best rows i64, docs i64, which i32, ev_scores flat [n_sub * k], ev_rows i64 flat): the
    evidence of question g starts at k * lims[g] and reads [k][m_g]"""
    S = np.asarray(S)
    lims = np.asarray(lims, dtype=np.int64)
    K, row, present = per_sub(S, lims, offsets, mask)
    nq, n_sub = len(lims) - 1, len(S)
    sc = np.full((nq, k), -np.inf, dtype=S.dtype)
    rows = np.full((nq, k), -1, dtype=np.int64)
    docs = np.full((nq, k), -1, dtype=np.int64)
    which = np.full((nq, k), -1, dtype=np.int32)
    evs = np.full(n_sub * k, -np.inf, dtype=S.dtype)
    evr = np.full(n_sub * k, -1, dtype=np.int64)
    for g in range(nq):
        a, b = int(lims[g]), int(lims[g + 1])
        m = b - a
        Kg, Rg = K[a:b], row[a:b]
        Fk = Kg.max(axis=0) if fuse == "max" else Kg.min(axis=0)
        d = np.flatnonzero(present[g])
        part = d[np.lexsort((d, -Fk[d]))][:k]                              # F descending, then lower document first
        n = len(part)
        w = np.argmax(Kg[:, part] == Fk[part][None, :], axis=0)          # the first of the equal sub-queries
        best = Rg[w, part]
        docs[g, :n], which[g, :n], rows[g, :n] = part, w, best
        sc[g, :n] = S[a + w, best]
        e_rows = Rg[:, part].T                                            # [n][m]
        e_sc = S[np.arange(a, b)[None, :], e_rows]
        evs[k * a:k * a + n * m] = e_sc.reshape(-1)
        evr[k * a:k * a + n * m] = e_rows.reshape(-1)
    return sc, rows, docs, which, evs, evr


def evidence_of(ev, lims, g, k):
    """question g's [k][m_g] block of a flat evidence array"""
    a, b = int(lims[g]), int(lims[g + 1])
    return np.asarray(ev)[k * a:k * b].reshape(k, b - a)


def fused64(S64, lims, offsets, fuse, mask=None):
    """fp64 -> (E [n_sub][n_docs] (-inf: absent), F [n_questions][n_docs], present)"""
    E, _, present = per_sub(np.asarray(S64, dtype=np.float64), lims, offsets, mask)
    op = np.max if fuse == "max" else np.min
    F = np.stack([op(E[lims[g]:lims[g + 1]], axis=0) for g in range(len(lims) - 1)])
    return E, F, present


def check_question(S64, lims, offsets, g, fuse, mask_row, scores, rows, docs, which, ev_scores, ev_rows, tol=TOL, atol=ATOL):
    """the fp64 bar for one question: what the library returned ([k] each, the evidence [k][m]) against the fp64 score rows
    -> (entries, positions whose document differs from the reference's ranking, largest |score - fp64 F|, first violation or None)"""
    a, b = int(lims[g]), int(lims[g + 1])
    sub = np.asarray(S64, dtype=np.float64)[a:b]
    E, F, present = fused64(sub, np.array([0, b - a]), offsets, fuse, mask_row)
    F, present = F[0], present[0]
    docs, rows, which = np.asarray(docs, dtype=np.int64), np.asarray(rows, dtype=np.int64), np.asarray(which, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float64)
    live = docs >= 0
    n = int(live.sum())
    assert n == min(len(docs), int(present.sum())) and live[:n].all(), "the result's length is exact"
    assert (rows[~live] == -1).all() and (which[~live] == -1).all() and np.isneginf(scores[~live]).all()
    assert np.isneginf(np.asarray(ev_scores)[~live]).all() and (np.asarray(ev_rows)[~live] == -1).all()
    got = docs[:n]
    assert present[got].all() and len(set(got.tolist())) == n, "a present document is returned once"
    off = np.asarray(offsets, dtype=np.int64)
    er = np.asarray(ev_rows, dtype=np.int64)[:n]
    assert ((off[got][:, None] <= er) & (er < off[got + 1][:, None])).all(), "an evidence row lies inside its document"
    if mask_row is not None:
        assert np.asarray(mask_row, dtype=bool)[er].all(), "an evidence row is an allowed row"
    w = which[:n]
    assert ((0 <= w) & (w < b - a)).all() and (rows[:n] == er[np.arange(n), w]).all(), "the best row is the named sub-query's evidence row"
    s = F[got]
    lo, hi = intervals(F[present], s, tol)
    pos = np.arange(n)
    err = float(np.abs(scores[:n] - s).max()) if n else 0.0
    named = E[w, got]
    ev64 = sub[np.arange(b - a)[None, :], er]                             # fp64 score of every evidence row
    bad = np.flatnonzero((pos < lo) | (pos > hi) | (np.abs(scores[:n] - s) > atol) | (np.abs(named - s) > tol) |
                         (np.abs(ev64 - E[:, got].T) > tol).any(axis=1))
    d = np.flatnonzero(present)
    want = d[np.lexsort((d, -F[d]))][:n]
    first = None if len(bad) == 0 else (int(bad[0]), int(got[bad[0]]), int(lo[bad[0]]), int(hi[bad[0]]), float(named[bad[0]] - s[bad[0]]))
    return n, int((got != want).sum()), err, first


def widened(S64, lims, offsets, k, fuse, mask=None, tol=TOL):
    """-> (entries, intervals wider than one position) over the documents of the reference's own top k of every question"""
    _, F, present = fused64(S64, lims, offsets, fuse, mask)
    docs = multi_group_ref(np.asarray(S64, dtype=np.float64), lims, offsets, k, fuse, mask)[2]
    entries = wide = 0
    for g in range(len(F)):
        d = docs[g][docs[g] >= 0]
        lo, hi = intervals(F[g][present[g]], F[g][d], tol)
        pos = np.arange(len(d))
        assert ((lo <= pos) & (pos <= hi)).all()
        entries += len(d); wide += int((hi > lo).sum())
    return entries, wide


K_FP64 = 100
# the cases of the fp64 test (k = 100): name -> (size cycle of the questions, filter density or None,
# {fuse: (entries, widened intervals)}) — what the reference alone says about its own rankings at TOL = 6e-7
TABLE = {
    "unit-5000x37x256-mean7": [((1, 2, 3, 4, 5, 6, 7, 9), None, {"max": (800, 2), "min": (800, 6)}),
                               ((1, 2, 3, 4, 5, 6, 7, 9), 0.5, {"max": (800, 4), "min": (800, 2)})],
    "unit-3001x300x128-mean3": [((1, 3, 8, 2, 64, 5), None, {"max": (2300, 2), "min": (2300, 6)})],
    "unit-2000x24x2304-mean5": [((1, 2, 3, 6), 0.5, {"max": (800, 6), "min": (800, 4)})],
    "decks-256": [((4,), None, {"max": (1600, 2), "min": (1600, 6)})],
    "decks-2304": [((4,), None, {"max": (1600, 10), "min": (1600, 6)})],
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (C, Q, offsets, S fp64) of a TABLE entry; read-only, shared between tests"""
    if name.startswith("decks-"):
        dim = int(name.split("-")[1])
        C, off = R.decks(300, 10, dim, 3e-4)
        Q = R.unit(64, dim, 2)                                            # 16 questions of 4 sub-queries
    else:
        shape, mean = name.split("-")[1:]
        nd, nq, dim = (int(x) for x in shape.split("x"))
        C, Q = R.unit(nd, dim, 1), R.unit(nq, dim, 2)
        off = R.random_offsets(nd, int(mean[4:]))
    return R.frozen(C, Q, off, R.scores64(Q, C))


def case_mask(name, density):
    """the one filter of a TABLE row: bool [rows] or None"""
    return None if density is None else FS.random_filters(len(case(name)[0]), (density,), seed=11)[0]
