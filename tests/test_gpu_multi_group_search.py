"""-m gpu: the fused document search (vr_index_search_multi_groups / vr_index_multi_group_search_stats,
csrc/search_multi_group.hip) against the library's own fp32 scores — strict, bit for bit — and against the numpy reference
tests/multi_group_search_ref.py.

Strict tests (no tolerance, host arrays and CUDA tensors): the oracle is the library's own fp32 score matrix, every row of
`search_range(threshold = -4, sort=False)`, masked, reduced per document, fused and ranked in numpy on orderable bits
(multi_group_search_ref.multi_group_ref); scores, best rows, documents, which and both evidence arrays must equal it.  A question
of one sub-query IS `search_groups_window(offset 0)` (and `search_groups`), documents of one row ARE `search_multi`, in every
setting of `set_search_eps`.

The multi-hop case is what the search is for: 300 documents of 10 random unit pages, 48 questions of two sub-queries that are
noisy copies of two DIFFERENT pages of one document; all-of over documents must name that document and those two pages, while
all-of over pages (`search_multi`) has no page that serves both.

Against fp64 (no excuse mechanism, the interval is the whole test; k = 100, max and min): scores within 1e-5 of the fp64 F; the
document of fp64 score s at position j has j in [#(F > s + 6e-7), #(F >= s - 6e-7) - 1] over the present documents; the sub-query
named by `which` has fp64 E_j(D) within 6e-7 of s; every evidence row's fp64 score lies within 6e-7 of its sub-query's fp64
E_j(D).  The reference alone widens these intervals (tests/test_cpu_multi_group_search_ref.py pins them; max / min):

    case                                  filter density   entries   widened intervals
    (5000, 37, 256), mean 7                    none            800        2 / 6
    (5000, 37, 256), mean 7                    0.5             800        4 / 2
    (3001, 300, 128), mean 3                   none          2 300        2 / 6
    (2000, 24, 2304), mean 5                   0.5             800        6 / 4
    decks 300 x 10, noise 3e-4, dim 256        none          1 600        2 / 6
    decks 300 x 10, noise 3e-4, dim 2304       none          1 600       10 / 6

Measured on an MI355X (the same for host arrays and CUDA tensors; max / min): every position inside its interval; 0 of the 15 800
positions differ from the reference's own fp64 ranking; largest |score - fp64| 2.5e-8 / 2.2e-8, 2.7e-8 / 1.8e-8, 5.3e-8 / 3.3e-8,
7.2e-9 / 7.1e-9, 2.3e-8 / 1.5e-8, 1.0e-8 / 6.9e-9 in the table's order.  Band documents re-scored per document returned: 1.36 /
1.48, 1.30 / 1.35, 1.28 / 1.36, 1.66 / 1.66, 1.19 / 1.19, 1.59 / 1.61; fp32 page dots per document returned: 7.2 / 8.0, 6.7 / 7.1,
19.4 / 21.3, 6.6 / 6.8, 47.7 / 47.4, 63.8 / 64.3 — in the decks every page of a band document lies within 2 eps of its document's
maximum and is re-scored for each of the four sub-queries.  Multi-hop: all 48 questions return d and (p, p'); 0 of the 48 pages of
`search_multi(min, k = 1)` lie in d.
"""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import filter_search_ref as F  # noqa: E402
from tests import group_search_ref as R  # noqa: E402
from tests import multi_group_search_ref as M  # noqa: E402
from tests import range_search_ref as X  # noqa: E402
from tests import rank_search_ref as K  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.engine import HipIndex, _stream_ptr  # noqa: E402

VR_OK, VR_ERR_INVALID, VR_ERR_STATE = 0, 1, 3
CYCLE_C = (0.05, 0.07)
ZERO = {"questions": 0, "documents": 0, "page_dots": 0}
FUSES = ("max", "min")


def _index(C, off, masks=None):
    ix = HipIndex(C.shape[1], len(C))
    ix.add(C[: len(C) // 2]); ix.add(C[len(C) // 2:])
    ix.set_groups(off)
    if masks is not None:
        ix.set_filters(masks)
    return ix


def _np(*xs):
    return [x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in xs]


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _scores(ix, Q):
    """the library's own fp32 score of every (query, row): f32 [nq][rows]"""
    lims, sc, ids = ix.search_range(Q, -4.0, None, sort=False)
    n = len(ix)
    assert np.array_equal(lims, np.arange(len(Q) + 1) * n) and np.array_equal(ids, np.tile(np.arange(n), len(Q)))
    return sc.reshape(len(Q), n)


def _masks_of(Mk, fog, n):
    """per question the rows its filter allows (-1: None)"""
    return [None if f < 0 else Mk[f] for f in fog]


def _same(got, want):
    """all six outputs, bit for bit (the evidence flat or reshaped)"""
    got = _np(*got)
    assert len(got) == 6
    sc, rows, docs, which, evs, evr = got
    assert sc.dtype == np.float32 and rows.dtype == np.int64 and docs.dtype == np.int64 and which.dtype == np.int32
    assert evs.dtype == np.float32 and evr.dtype == np.int64
    assert sc.shape == rows.shape == docs.shape == which.shape == want[2].shape
    assert np.array_equal(docs, want[2])
    assert np.array_equal(which, want[3])
    assert np.array_equal(rows, want[1])
    assert np.array_equal(_u32(sc), _u32(want[0]))
    assert np.array_equal(evr.reshape(-1), np.asarray(want[5]).reshape(-1))
    assert np.array_equal(_u32(evs.reshape(-1)), _u32(np.asarray(want[4]).reshape(-1)))


def _both(Q, lims, fog=None):
    """the call's inputs as host arrays and as CUDA tensors"""
    yield Q, lims, fog
    yield torch.tensor(Q).cuda(), lims, fog if fog is None or np.isscalar(fog) else torch.tensor(np.asarray(fog)).cuda()


# ----------------------------------------------------------------------------------------------- 1. the oracle ---
@pytest.mark.parametrize("nd,nq,dim,cycle,mean", [(5000, 37, 256, (1, 2, 3, 4, 5, 6, 7, 9), 7), (5000, 37, 256, (1, 2, 3, 4, 5, 6, 7, 9), 1),
                                                   (2000, 24, 2304, (1, 2, 3, 6), 5)])
def test_all_six_outputs_equal_the_oracle(nd, nq, dim, cycle, mean):
    C, Q = R.unit(nd, dim, 1), R.unit(nq, dim, 2)
    off = np.arange(nd + 1) if mean == 1 else R.random_offsets(nd, mean)   # mean 1: 5 000 documents, two re-score chunks
    lims = M.layout(nq, cycle)
    ix = _index(C, off)
    S32 = _scores(ix, Q)
    for k in (1, 10, 100, 1000):
        for fuse in FUSES:
            want = M.multi_group_ref(S32, lims, off, k, fuse)
            for q_in, l_in, _ in _both(Q, lims):
                ix.multi_group_search_stats(reset=True)
                got = ix.search_multi_groups(q_in, l_in, k, fuse, evidence=True)
                cuda = isinstance(q_in, torch.Tensor)
                assert all((isinstance(x, torch.Tensor) and x.is_cuda) if cuda else isinstance(x, np.ndarray) for x in got)
                _same(got, want)
                st = ix.multi_group_search_stats()
                assert st["questions"] == len(lims) - 1 and st["page_dots"] >= st["documents"] >= int((want[2] >= 0).sum())
            four = ix.search_multi_groups(Q, lims, k, fuse)              # without the evidence: the same four
            assert len(four) == 4
            _same(tuple(four) + (want[4], want[5]), want)
    ix.close()


def test_layouts_that_fill_and_split_blocks_equal_one_call_per_question():
    C, Q = R.unit(3001, 128, 1), R.unit(300, 128, 2)
    off = R.random_offsets(3001, 3)
    ix = _index(C, off)
    S32 = _scores(ix, Q)
    cube = Q.reshape(60, 5, 128)
    for fuse in FUSES:
        for lims in (np.array([0, 200, 300]), np.array([0, 256, 300]), M.layout(300, (1, 3, 8, 2, 64, 5))):
            want = M.multi_group_ref(S32, lims, off, 10, fuse)
            for q_in, l_in, _ in _both(Q, lims):
                _same(ix.search_multi_groups(q_in, l_in, 10, fuse, evidence=True), want)
            for g in range(0, len(lims) - 1, 5):
                a, b = lims[g], lims[g + 1]
                one = _np(*ix.search_multi_groups(Q[a:b], [0, b - a], 10, fuse, evidence=True))
                for i in range(4):
                    assert np.array_equal(_u32(one[i][0]) if i == 0 else one[i][0], _u32(want[i][g]) if i == 0 else want[i][g])
                assert np.array_equal(one[5], M.evidence_of(want[5], lims, g, 10).reshape(-1))
                assert np.array_equal(_u32(one[4]), _u32(M.evidence_of(want[4], lims, g, 10).reshape(-1)))
        # [n_questions][m][dim] with lims=None: the evidence comes as [n_questions][k][m]
        want = M.multi_group_ref(S32, np.arange(61) * 5, off, 7, fuse)
        for c_in in (cube, torch.tensor(cube).cuda()):
            got = ix.search_multi_groups(c_in, None, 7, fuse, evidence=True)
            assert tuple(got[4].shape) == tuple(got[5].shape) == (60, 7, 5)
            _same(got, want)
    ix.close()


# ---------------------------------------------------------------------------------------------- 2. identities ---
def _eps_settings(ix):
    for eps in (float("nan"), -1.0, 0.01):                               # the default, certification off, a caller's model
        ix.set_search_eps(eps)
        yield eps
    ix.set_search_eps(float("nan"))


def test_questions_of_one_are_the_document_window_search():
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    off = R.random_offsets(5000, 7)
    Mk = np.concatenate([F.random_filters(len(C), (0.5, 0.01), seed=11), np.zeros((1, len(C)), dtype=bool)])
    fog = (np.arange(len(Q)) % 4 - 1).astype(np.int64)
    ix = _index(C, off, Mk)
    lims = np.arange(len(Q) + 1)
    for _ in _eps_settings(ix):
        for k in (10, 100, 1000):
            for f in (None, fog):
                sc, rows, gr = _np(*ix.search_groups_window(Q, 0, k, f))
                want = (sc, rows, gr, np.where(gr >= 0, 0, -1).astype(np.int32), sc.reshape(-1), rows.reshape(-1))
                for fuse in FUSES:
                    for q_in, l_in, f_in in _both(Q, lims, f):
                        _same(ix.search_multi_groups(q_in, l_in, k, fuse, f_in, evidence=True), want)
    ix.close()


def test_documents_of_one_row_are_the_fused_search():
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    Mk = F.random_filters(len(C), (0.5, 0.01), seed=11)
    lims = M.layout(37, (1, 2, 3, 4, 5, 6, 7, 9))
    fog = (np.arange(len(lims) - 1) % 3 - 1).astype(np.int64)
    ix = _index(C, np.arange(len(C) + 1), Mk)
    for _ in _eps_settings(ix):
        for k in (10, 1000):
            for fuse in FUSES:
                for f in (None, fog):
                    sc, ids, which = _np(*ix.search_multi(Q, lims, k, fuse, f))
                    for q_in, l_in, f_in in _both(Q, lims, f):
                        got = _np(*ix.search_multi_groups(q_in, l_in, k, fuse, f_in))
                        assert np.array_equal(_u32(got[0]), _u32(sc)) and np.array_equal(got[1], ids) and np.array_equal(got[2], ids)
                        assert np.array_equal(got[3], which)
    ix.close()


def test_questions_of_one_are_search_groups_on_the_large_corpus():
    C, Q, _, _ = X.random_case(20000, 64, 2304, CYCLE_C)
    off = R.random_offsets(20000, 10)
    ix = _index(C, off)
    lims = np.arange(len(Q) + 1)
    for k in (10, 100):
        ix.set_search_eps(float("nan"))
        sc, rows, gr = _np(*ix.search_groups(Q, k))
        want = (sc, rows, gr, np.zeros_like(gr, dtype=np.int32), sc.reshape(-1), rows.reshape(-1))
        for _ in _eps_settings(ix):
            for q_in, l_in, _f in _both(Q, lims):
                _same(ix.search_multi_groups(q_in, l_in, k, "min", evidence=True), want)
    ix.close()


def test_repeated_and_permuted_sub_queries():
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    off = R.random_offsets(5000, 7)
    ix = _index(C, off)
    k = 50
    for fuse in FUSES:
        one = _np(*ix.search_multi_groups(Q[:1], [0, 1], k, fuse, evidence=True))
        for q_in, l_in, _ in _both(np.repeat(Q[:1], 5, axis=0), [0, 5]):
            got = _np(*ix.search_multi_groups(q_in, l_in, k, fuse, evidence=True))
            for i in range(4):
                assert np.array_equal(got[i].view(np.uint32) if i == 0 else got[i], one[i].view(np.uint32) if i == 0 else one[i])
            assert (got[3] == 0).all()                                   # which: the lowest of the equal sub-queries
            assert np.array_equal(got[5].reshape(k, 5), np.repeat(one[5].reshape(k, 1), 5, axis=1))
        base = _np(*ix.search_multi_groups(Q[:6], [0, 6], k, fuse, evidence=True))
        perm = np.array([3, 0, 5, 1, 4, 2])
        got = _np(*ix.search_multi_groups(Q[:6][perm], [0, 6], k, fuse, evidence=True))
        assert np.array_equal(_u32(got[0]), _u32(base[0])) and np.array_equal(got[1], base[1]) and np.array_equal(got[2], base[2])
        assert np.array_equal(perm[got[3]], base[3])                     # which follows the permutation ...
        assert np.array_equal(got[5].reshape(k, 6), base[5].reshape(k, 6)[:, perm])       # ... and so does the evidence order
        assert np.array_equal(_u32(got[4]).reshape(k, 6), _u32(base[4]).reshape(k, 6)[:, perm])
    qq = np.repeat(Q[:1], 2, axis=0)
    _same(ix.search_multi_groups(qq, [0, 2], k, "min", evidence=True), _np(*ix.search_multi_groups(qq, [0, 2], k, "max", evidence=True)))
    ix.close()


# ----------------------------------------------------------------------------------------- 3. document shapes ---
def test_document_shapes():
    n, dim = 6000, 64
    C, Q = R.unit(n, dim, 1), R.unit(9, dim, 2)
    lengths = [4500, 63, 64, 65, 1, 128, 129, 2, 62]                      # one document longer than a chunk of 4 096 rows; lengths around 64
    offs = {
        "one document": np.array([0, n]),
        "long and short": np.concatenate([[0], np.cumsum(lengths), np.arange(sum(lengths) + 4, n, 4), [n]]),
        "not a multiple of four": np.concatenate([np.arange(0, 5995, 5), [n]]),
    }
    assert (len(offs["not a multiple of four"]) - 1) % 4 == 3
    mask = F.random_filters(n, (0.5,), seed=5)
    lims = np.array([0, 1, 3, 6, 9])
    ix = HipIndex(dim, n)
    ix.add(C)
    ix.set_filters(mask)
    S32 = _scores(ix, Q)
    for name, off in offs.items():
        off = off.astype(np.int64)
        ix.set_groups(off)
        for f in (None, 0):
            for fuse in FUSES:
                for k in (1, 10, 100):
                    want = M.multi_group_ref(S32, lims, off, k, fuse, None if f is None else mask[0])
                    for q_in, l_in, f_in in _both(Q, lims, f):
                        _same(ix.search_multi_groups(q_in, l_in, k, fuse, f_in, evidence=True), want)
        if name == "one document":
            sc, rows, docs, which, evs, evr = ix.search_multi_groups(Q, lims, 3, "max", evidence=True)
            assert (docs[:, 0] == 0).all() and (docs[:, 1:] == -1).all() and (rows[:, 1:] == -1).all()
            assert np.array_equal(M.evidence_of(evr, lims, 3, 3)[0], S32[6:9].argmax(1))
    ix.close()


# ------------------------------------------------------------------------------------------------ 4. filters ---
@pytest.fixture(scope="module")
def filtered():
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    off = R.random_offsets(5000, 7)
    Mk = np.concatenate([F.random_filters(len(C), (0.5, 0.01), seed=11), np.zeros((1, len(C)), dtype=bool)])
    ix = _index(C, off, Mk)
    yield ix, C, Q, off, Mk, _scores(ix, Q), M.layout(37, (1, 2, 3, 4, 5, 6, 7, 9))
    ix.close()


def test_questions_under_filters(filtered):
    ix, C, Q, off, Mk, S32, lims = filtered
    nq = len(lims) - 1
    fog = (np.arange(nq) % 4 - 1).astype(np.int64)                        # -1 (no filter), 0, 1, 2 (allows nothing), ...
    for fuse in FUSES:
        for k in (10, 100, 1000):
            want = M.multi_group_ref(S32, lims, off, k, fuse, _masks_of(Mk, fog, len(C)))
            assert (want[2][fog == 2] == -1).all() and (want[2][fog == -1][:, :min(k, len(off) - 1)] >= 0).all()
            for q_in, l_in, f_in in _both(Q, lims, fog):
                _same(ix.search_multi_groups(q_in, l_in, k, fuse, f_in, evidence=True), want)
        for f in (0, 1, 2):                                              # one filter for every question: density 0.5, 0.01, 0
            _same(ix.search_multi_groups(Q, lims, 100, fuse, f, evidence=True), M.multi_group_ref(S32, lims, off, 100, fuse, Mk[f]))
        _same(ix.search_multi_groups(Q, lims, 20, fuse, -1, evidence=True), _np(*ix.search_multi_groups(Q, lims, 20, fuse, evidence=True)))


def test_filters_on_the_questions_of_a_second_block():
    """600 rows, 300 sub-queries in questions of 1, 3, 8, 2, 5: two blocks of sub-queries, the second one's filters expanded from the
    questions that start past sub-query 256.  A half-density and an empty filter mixed per question, with and without evidence."""
    C, Q = R.unit(600, 64, 1), R.unit(300, 64, 2)
    off = R.random_offsets(600, 3)
    lims = M.layout(300, (1, 3, 8, 2, 5))
    Mk = np.concatenate([F.random_filters(600, (0.5,), seed=11), np.zeros((1, 600), dtype=bool)])
    fog = (np.arange(len(lims) - 1) % 3 - 1).astype(np.int64)             # -1 (no filter), 0, 1 (allows nothing), ...
    late = lims[:-1] >= 256
    assert (fog[late] == 0).any() and (fog[late] == 1).any()
    ix = _index(C, off, Mk)
    S32 = _scores(ix, Q)
    for fuse in FUSES:
        want = M.multi_group_ref(S32, lims, off, 10, fuse, _masks_of(Mk, fog, 600))
        assert (want[2][fog == 1] == -1).all() and (want[2][fog != 1] >= 0).all()
        for q_in, l_in, f_in in _both(Q, lims, fog):
            _same(ix.search_multi_groups(q_in, l_in, 10, fuse, f_in, evidence=True), want)
            four = ix.search_multi_groups(q_in, l_in, 10, fuse, f_in)
            assert len(four) == 4
            _same(tuple(four) + (want[4], want[5]), want)
    ix.close()


def test_a_filter_with_pages_in_three_documents_and_one_that_forbids_the_best_pages(filtered):
    ix, C, Q, off, Mk, S32, lims = filtered
    n = len(C)
    three = np.zeros(n, dtype=bool)
    three[[off[6] - 1, off[400], off[401] - 1, off[722]]] = True          # the last page of document 5, the ends of 400, the first of 722
    g = 3                                                                # a question of four sub-queries
    a, b = lims[g], lims[g + 1]
    assert b - a == 4
    base = _np(*ix.search_multi_groups(Q[a:b], [0, 4], 20, "max", evidence=True))
    forbid = np.ones(n, dtype=bool)
    forbid[base[5].reshape(20, 4)[:, 1]] = False                         # sub-query 1's best page in each of the top 20 documents
    ix.set_filters(np.stack([three, forbid]))
    try:
        for fuse in FUSES:
            want = M.multi_group_ref(S32, lims, off, 10, fuse, three)
            for q_in, l_in, f_in in _both(Q, lims, 0):
                got = _np(*ix.search_multi_groups(q_in, l_in, 10, fuse, f_in, evidence=True))
                _same(got, want)
                assert (np.sort(got[2][:, :3], axis=1) == [5, 400, 722]).all() and (got[2][:, 3:] == -1).all() and three[got[1][:, :3]].all()
        want = M.multi_group_ref(S32[a:b], [0, 4], off, 20, "max", forbid)
        for q_in, l_in, f_in in _both(Q[a:b], [0, 4], 1):
            got = _np(*ix.search_multi_groups(q_in, l_in, 20, "max", f_in, evidence=True))
            _same(got, want)
            assert forbid[got[5]].all()
            changed = 0
            for j, d in enumerate(base[2][0]):                           # every document that lost sub-query 1's best page
                at = np.flatnonzero(got[2][0] == d)
                if len(at) == 0:
                    continue                                             # (a one-page document is absent, or it fell out of the top 20)
                e0, e1 = base[5].reshape(20, 4)[j], got[5].reshape(20, 4)[at[0]]
                assert e1[1] != e0[1] and got[4].reshape(20, 4)[at[0], 1] <= base[4].reshape(20, 4)[j, 1]
                changed += 1
            assert changed >= 5
            assert not np.array_equal(_u32(got[0]), _u32(base[0])) and not np.array_equal(got[1], base[1])
            assert not np.array_equal(got[3], base[3]) and not np.array_equal(got[5], base[5])
    finally:
        ix.set_filters(Mk)


# --------------------------------------------------------------------------------------------------- 5. ties ---
def test_tied_documents_come_in_index_order():
    C, Q, _ = R.tie_tier()
    n = len(C)
    off = np.arange(0, n + 1, 5)                                          # 600 documents of five rows
    high = np.unique((7 * np.arange(100) + 3) // 5)
    tied = np.setdiff1d(np.arange(600), high)                             # 500 documents of five bit-identical rows: one tier
    ix = _index(C, off)
    S32 = _scores(ix, Q)
    lims = np.array([0, 1, 3])
    mask = np.ones(n, dtype=bool)
    mask[tied[:250] * 5] = False                                         # the first row of half the tied documents forbidden
    ix.set_filters(mask[None, :])
    for fuse in FUSES:
        for k in (150, 300, 1000):
            for f, mk in ((None, None), (0, mask)):
                want = M.multi_group_ref(S32, lims, off, k, fuse, mk)
                for q_in, l_in, f_in in _both(Q, lims, f):
                    got = _np(*ix.search_multi_groups(q_in, l_in, k, fuse, f_in, evidence=True))
                    _same(got, want)
                    kk = min(k, 600)
                    assert np.array_equal(got[2][:, 100:kk], np.tile(tied[:kk - 100], (2, 1)))          # the tier: in index order
                    first = tied[:kk - 100] * 5 + (0 if f is None else (np.arange(kk - 100) < 250))
                    assert np.array_equal(got[1][:, 100:kk], np.tile(first, (2, 1)))                    # the lowest ALLOWED tied row
    ix.close()


def test_decks_where_every_page_of_a_band_document_is_rescored():
    C, Q, off, S = M.case("decks-2304")
    ix = _index(C, off)
    S32 = _scores(ix, Q)
    lims = np.arange(17) * 4
    for fuse in FUSES:
        for k in (10, 100):
            want = M.multi_group_ref(S32, lims, off, k, fuse)
            for q_in, l_in, _ in _both(Q, lims):
                ix.multi_group_search_stats(reset=True)
                _same(ix.search_multi_groups(q_in, l_in, k, fuse, evidence=True), want)
                st = ix.multi_group_search_stats()
                assert st["page_dots"] == 10 * 4 * st["documents"] and st["documents"] >= 16 * k      # pages x sub-queries x band documents
    ix.close()


# -------------------------------------------------------------------------------------------------- 6. edits ---
def _vp(x):
    if x is None:
        return ctypes.c_void_p(None)
    return ctypes.c_void_p(x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data)


def _raw(ix, Q, lims, k, fuse=0, fog=None, n_sub=None, ng=None, ev=(True, True)):
    """vr_index_search_multi_groups itself, host arrays -> (status, scores, rows, docs, which, ev_scores, ev_rows); the outputs start as -7"""
    lims = np.asarray(lims, dtype=np.int64)
    n = max((len(lims) - 1) * max(k, 1), 1)
    ne = max(len(Q) * max(k, 1), 1)
    sc, rows, docs = np.full(n, -7, dtype=np.float32), np.full(n, -7, dtype=np.int64), np.full(n, -7, dtype=np.int64)
    which, evs, evr = np.full(n, -7, dtype=np.int32), np.full(ne, -7, dtype=np.float32), np.full(ne, -7, dtype=np.int64)
    st = ix.lib.vr_index_search_multi_groups(ix._h, _vp(Q), len(Q) if n_sub is None else n_sub, _vp(lims), len(lims) - 1 if ng is None else ng,
                                             k, fuse, _vp(fog), _vp(sc), _vp(rows), _vp(docs), _vp(which), _vp(evs if ev[0] else None),
                                             _vp(evr if ev[1] else None), 0, ctypes.c_void_p(_stream_ptr(ix.device)))
    return st, sc, rows, docs, which, evs, evr


def test_an_edited_index_answers_as_a_fresh_one():
    C, Q = R.unit(3001, 128, 1).copy(), R.unit(40, 128, 2)
    off = R.random_offsets(3001, 3)
    lims = M.layout(40, (1, 3, 8, 2))
    rng = np.random.default_rng(17)
    gone_docs = rng.choice(len(off) - 1, 300, replace=False)
    gone = np.concatenate([np.arange(off[g], off[g + 1]) for g in gone_docs] + [off[[5, 9, 700]]])
    ix = _index(C, off)
    ix.search_multi_groups(Q, lims, 10)                                  # (nothing is stored: nothing to invalidate)
    new_id = ix.remove(gone)
    assert _raw(ix, Q, lims, 10)[0] == VR_ERR_STATE                      # the grouping went with the removal
    assert "vr_index_set_groups" in _lib.load().vr_last_error().decode()
    with pytest.raises(_lib.VisragHipError):
        ix.search_multi_groups(Q, lims, 10)
    left = C[new_id >= 0]
    gid = (np.searchsorted(off, np.arange(len(C)), side="right") - 1)[new_id >= 0]
    left_off = np.concatenate([[0], np.flatnonzero(np.diff(gid)) + 1, [len(left)]]).astype(np.int64)
    ix.set_groups(left_off)
    fresh = _index(left, left_off)
    for fuse in FUSES:
        _same(ix.search_multi_groups(Q, lims, 100, fuse, evidence=True), _np(*fresh.search_multi_groups(Q, lims, 100, fuse, evidence=True)))
    upd = rng.choice(len(left), 5, replace=False)
    fresh_rows = R.unit(5, 128, 33)
    ix.update(upd, fresh_rows)                                           # no row moves: the grouping stays
    left[upd] = fresh_rows
    fresh.close()
    fresh = _index(left, left_off)
    for fuse in FUSES:
        got = _np(*ix.search_multi_groups(Q, lims, 100, fuse, evidence=True))
        _same(got, _np(*fresh.search_multi_groups(Q, lims, 100, fuse, evidence=True)))
        _same(got, M.multi_group_ref(_scores(fresh, Q), lims, left_off, 100, fuse))
    ix.close(); fresh.close()


# ------------------------------------------------------------------------------------ 7. arguments, the raw ABI ---
def test_argument_checks_come_before_any_launch():
    n = 600
    C, Q = R.unit(n, 64, 1), R.unit(300, 64, 2)
    off = R.random_offsets(n, 4)
    Mk = F.random_filters(n, (0.5, 0.1), seed=11)
    lims = np.array([0, 2, 3, 7])
    Q7 = Q[:7]
    fog = np.array([0, -1, 1], dtype=np.int32)
    ix = HipIndex(64, n + 10)
    st, sc, rows, docs, which, evs, evr = _raw(ix, Q7, lims, 5)          # an empty index: tails
    assert st == VR_OK and np.isneginf(sc).all() and (rows == -1).all() and (docs == -1).all() and (which == -1).all()
    assert np.isneginf(evs).all() and (evr == -1).all()
    ix.add(C)
    out = _raw(ix, Q7, lims, 5)
    assert out[0] == VR_ERR_STATE and all((o == -7).all() for o in out[1:])      # no grouping set
    assert ix.multi_group_search_stats() == ZERO
    ix.set_groups(off)
    out = _raw(ix, Q7, lims, 5, 0, fog)
    assert out[0] == VR_ERR_STATE and all((o == -7).all() for o in out[1:])      # filters named but none set
    ix.set_filters(Mk)
    S32 = _scores(ix, Q7)
    out = _raw(ix, Q7, lims, 20, 1, fog)
    assert out[0] == VR_OK
    want = M.multi_group_ref(S32, lims, off, 20, "min", _masks_of(Mk, fog, n))
    _same((out[1].reshape(3, 20), out[2].reshape(3, 20), out[3].reshape(3, 20), out[4].reshape(3, 20), out[5], out[6]), want)
    out = _raw(ix, Q7, lims, 20, 1, fog, ev=(False, False))              # no evidence asked for: the same four, nothing else written
    assert out[0] == VR_OK and np.array_equal(out[3].reshape(3, 20), want[2]) and (out[5] == -7).all() and (out[6] == -7).all()
    stats = ix.multi_group_search_stats()
    assert stats["questions"] == 6
    foq = np.array([0, 1, -1, 1, 0, 0, -1], dtype=np.int64)
    before = (ix.search(Q7, 10), ix.search_multi(Q7, lims, 10, "min", fog), ix.search_groups_window(Q7, 3, 10, foq))
    others = (ix.search_stats(), ix.group_search_stats(), ix.filter_search_stats(), ix.range_search_stats(), ix.rank_search_stats(),
              ix.window_search_stats(), ix.multi_search_stats(), ix.group_window_search_stats())

    def nothing_ran(st, *outs):
        return st == VR_ERR_INVALID and all((o == -7).all() for o in outs) and ix.multi_group_search_stats() == stats

    for k in (0, -1, 1001):
        assert nothing_ran(*_raw(ix, Q7, lims, k, 0, fog)), k
    assert "k=1001 unsupported (1..1000)" in _lib.load().vr_last_error().decode()
    for fuse in (2, -1):
        assert nothing_ran(*_raw(ix, Q7, lims, 5, fuse, fog)), fuse
    for bad in ([1, 2, 3, 7], [0, 3, 2, 7], [0, 2, 2, 7], [0, 2, 3, 6], [0, 2, 3, 8]):      # lims[0], decreasing, empty, the end
        assert nothing_ran(*_raw(ix, Q7, bad, 5, 0, fog)), bad
    assert nothing_ran(*_raw(ix, Q, [0, 257, 300], 5))                   # a question of 257 sub-queries
    assert "257 sub-queries" in _lib.load().vr_last_error().decode()
    assert _raw(ix, Q, [0, 256, 300], 5)[0] == VR_OK
    stats = ix.multi_group_search_stats()
    assert nothing_ran(*_raw(ix, Q7, lims, 5, 0, fog, ev=(True, False)))          # one evidence pointer of the two
    assert nothing_ran(*_raw(ix, Q7, lims, 5, 0, fog, ev=(False, True)))
    for bad in (2, -2):                                                  # a filter index out of range
        fb = np.array([0, bad, -1], dtype=np.int32)
        assert nothing_ran(*_raw(ix, Q7, lims, 5, 0, fb))
        with pytest.raises(ValueError):
            ix.search_multi_groups(Q7, lims, 5, "max", filter_of_group=fb)
    assert "outside [-1, 2)" in _lib.load().vr_last_error().decode()
    assert ix.lib.vr_index_search_multi_groups(ix._h, _vp(Q7), 7, _vp(None), 3, 5, 0, _vp(None), _vp(None), _vp(None), _vp(None), _vp(None),
                                               _vp(None), _vp(None), 0, None) == VR_ERR_INVALID
    assert nothing_ran(*_raw(ix, Q7, lims, 5, 0, fog, n_sub=-1))
    assert nothing_ran(*_raw(ix, Q7, lims, 5, 0, fog, ng=-1))
    assert nothing_ran(*_raw(ix, Q7, lims, 5, 0, None, ng=0))            # sub-queries in no question
    out = _raw(ix, Q7, lims, 5, 0, None, n_sub=0, ng=0)                  # no question: VR_OK, nothing launched, nothing written
    assert out[0] == VR_OK and all((o == -7).all() for o in out[1:]) and ix.multi_group_search_stats() == stats
    for bad in ("sum", "MAX"):
        with pytest.raises(ValueError):
            ix.search_multi_groups(Q7, lims, 5, bad)
    with pytest.raises(ValueError):
        ix.search_multi_groups(Q7, None, 5)                              # lims=None wants [n_questions][m][dim]
    with pytest.raises(_lib.VisragHipError):
        ix.search_multi_groups(Q7, lims, 1001)
    # on the device an out-of-range filter index cannot be seen before the launch: that question gets a row of tails
    qd = torch.tensor(Q7).cuda()
    fb = torch.tensor(np.array([0, 7, 1], dtype=np.int32)).cuda()
    o4 = [torch.full((3, 5), -7, dtype=d).cuda() for d in (torch.float32, torch.int64, torch.int64, torch.int32)]
    oe = [torch.full((35,), -7, dtype=d).cuda() for d in (torch.float32, torch.int64)]
    st = ix.lib.vr_index_search_multi_groups(ix._h, _vp(qd), 7, _vp(np.asarray(lims, dtype=np.int64)), 3, 5, 0, _vp(fb), *[_vp(x) for x in o4 + oe],
                                             1, ctypes.c_void_p(_stream_ptr(ix.device)))
    torch.cuda.synchronize()
    assert st == VR_OK
    want = [np.array(x) for x in M.multi_group_ref(S32, lims, off, 5, "max", [Mk[0], np.zeros(n, dtype=bool), Mk[1]])]
    assert (want[2][1] == -1).all()
    _same(tuple(o4 + oe), want)
    # no other search's state or counters were touched, and they answer with the same bits
    assert (ix.search_stats(), ix.group_search_stats(), ix.filter_search_stats(), ix.range_search_stats(), ix.rank_search_stats(),
            ix.window_search_stats(), ix.multi_search_stats(), ix.group_window_search_stats()) == others
    after = (ix.search(Q7, 10), ix.search_multi(Q7, lims, 10, "min", fog), ix.search_groups_window(Q7, 3, 10, foq))
    for a, b in zip(before, after):
        assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                   for x, y in zip(a, b))
    st2 = ix.multi_group_search_stats()
    assert ix.multi_group_search_stats(reset=True) == st2 and ix.multi_group_search_stats() == ZERO
    ix.add(C[:10])                                                       # rows appended: grouping and filters are gone with them
    assert ix.n_groups == 0 and _raw(ix, Q7, lims, 5)[0] == VR_ERR_STATE
    ix.close()


# ------------------------------------------------------------------------------------------- 8. the multi-hop case ---
def test_multi_hop_questions_find_their_document_and_both_pages():
    """Measured on an MI355X: all 48 questions name d and (p, p') at k = 1 under fuse="min"; of search_multi(min, k = 1)'s 48 pages
    0 lie in d (recorded, not asserted: the README's fused document search section quotes it)."""
    nd, pages, dim, nq = 300, 10, 256, 48
    C = R.unit(nd * pages, dim, 41)
    off = np.arange(nd + 1) * pages
    rng = np.random.default_rng(42)
    d = rng.integers(0, nd, nq)
    p = rng.integers(0, pages, nq)
    p2 = (p + rng.integers(1, pages, nq)) % pages
    assert (p != p2).all()
    rows = np.stack([d * pages + p, d * pages + p2], axis=1)              # [nq][2]
    Q = C[rows.reshape(-1)].astype(np.float64) + 0.05 * rng.standard_normal((2 * nq, dim))
    Q = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    lims = np.arange(nq + 1) * 2
    _, F64, _ = M.fused64(R.scores64(Q, C), lims, off, "min")
    others = F64.copy()
    others[np.arange(nq), d] = -np.inf
    assert (F64[np.arange(nq), d] - others.max(axis=1) > 0.1).all()      # in fp64 d wins by more than 0.1
    ix = _index(C, off)
    for q_in, l_in, _ in _both(Q, lims):
        sc, best, docs, which, evs, evr = _np(*ix.search_multi_groups(q_in, l_in, 1, "min", evidence=True))
        assert np.array_equal(docs[:, 0], d)
        assert np.array_equal(evr.reshape(nq, 2), rows)
    _, ids, _ = _np(*ix.search_multi(Q, lims, 1, "min"))
    print(f"multi-hop: {int((ids[:, 0] // pages == d).sum())} of search_multi(min, k = 1)'s {nq} pages lie in the question's document")
    ix.close()


# ------------------------------------------------------------------------------------------------ against fp64 ---
@pytest.mark.parametrize("name", list(M.TABLE))
def test_documents_scores_and_evidence_against_fp64(name):
    C, Q, off, S = M.case(name)
    k = M.K_FP64
    ix = _index(C, off)
    for cycle, density, table in M.TABLE[name]:
        lims = M.layout(len(Q), cycle)
        mask = M.case_mask(name, density)
        if mask is not None:
            ix.set_filters(mask[None, :])
        for fuse in FUSES:
            first = None
            for q_in, l_in, f_in in _both(Q, lims, None if mask is None else 0):
                ix.multi_group_search_stats(reset=True)
                sc, rows, docs, which, evs, evr = _np(*ix.search_multi_groups(q_in, l_in, k, fuse, f_in, evidence=True))
                st = ix.multi_group_search_stats()
                entries = moved = 0
                worst, err = None, 0.0
                for g in range(len(lims) - 1):
                    n_g, moved_g, err_g, bad = M.check_question(S, lims, off, g, fuse, mask, sc[g], rows[g], docs[g], which[g],
                                                                M.evidence_of(evs, lims, g, k), M.evidence_of(evr, lims, g, k))
                    entries += n_g; moved += moved_g; err = max(err, err_g)
                    worst = worst or (bad and (g,) + bad)
                print(f"{name} {fuse} density {density}: {entries} entries, {moved} positions differ from the fp64 ranking, max |score - fp64| "
                      f"{err:.2e}, {st['documents'] / max(entries, 1):.2f} band documents and {st['page_dots'] / max(entries, 1):.2f} page dots "
                      f"per document returned")
                assert entries == table[fuse][0]
                assert err <= M.ATOL
                assert worst is None, worst                              # (question, position, document, lo, hi, named - F)
                now = (_u32(sc).tolist(), rows.tolist(), docs.tolist(), which.tolist(), _u32(evs).tolist(), evr.tolist())
                first = first or now
                assert now == first                                      # host and device callers: the same bits
    ix.close()


# ------------------------------------------------------------------------------------------------ host consumers ---
def test_retrieve_documents_fused_over_pickle_shards(tmp_path):
    from visrag_amd import retriever
    from visrag_amd.utils import write_shard
    C, Q, bounds = K.shards_case()                                       # shards of 1 000, 3 001 and 1 999 rows, 9 queries
    doc_of = lambda page: f"doc_{int(page.split('_')[1]) // 7}"          # noqa: E731  (documents of seven pages straddle the shards)
    label_of_doc = lambda dd: int(dd.split("_")[1]) % 3                  # noqa: E731
    names = [f"page_{i}" for i in range(len(C))]
    for s in range(3):
        write_shard(str(tmp_path / f"embeddings.corpus.rank.{s}"), C[bounds[s]:bounds[s + 1]], names[bounds[s]:bounds[s + 1]])
    qids = [f"q{q}" for q in range(len(Q))]
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, qids)
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    group_of = lambda q: int(q[1:]) // 3                                 # noqa: E731  (three questions of three)
    lims = np.arange(4) * 3
    wanted = {g: (None, {0}, {1, 2})[g % 3] for g in range(3)}
    off = np.concatenate([np.arange(0, len(C), 7), [len(C)]])
    whole = _index(C, off)
    S32 = _scores(whole, Q)
    whole.close()
    docs = [f"doc_{g}" for g in range(len(off) - 1)]
    masks = [None if wanted[g] is None else np.repeat(np.isin(np.arange(len(docs)) % 3, list(wanted[g])), np.diff(off)) for g in range(3)]
    for fuse in FUSES:
        for topk, filt in ((10, False), (25, True)):
            want = M.multi_group_ref(S32, lims, off, topk, fuse, masks if filt else None)
            sc, pg = retriever.retrieve_documents_fused(args, group_of, topk, doc_of, fuse, *((label_of_doc, lambda g: wanted[g]) if filt else ()))
            for g in range(3):
                assert list(sc[g]) == [docs[x] for x in want[2][g]] == list(pg[g])
                assert np.array_equal(_u32(list(sc[g].values())), _u32(want[0][g]))
                ev = M.evidence_of(want[5], lims, g, topk)
                assert list(pg[g].values()) == [[names[r] for r in slot] for slot in ev]


def test_demo_retrieve_documents_any(tmp_path):
    from visrag_amd import demo
    D, _ = R.decks(6, 5, 64, 0.05)
    C = np.concatenate([D, R.unit(40, 64, 9)])
    names = [f"deck_{d}.pdf_{i}.png" for d in range(6) for i in range(5)] + [f"other_{j}.pdf_0.png" for j in range(40)]
    perm = np.random.default_rng(2).permutation(len(C))                  # on disk the pages of a document are not adjacent
    qv = np.stack([C[2 * 5 + 1], C[2 * 5 + 4], C[3 * 5]]) + 0.02 * R.unit(3, 64, 5)
    kb = str(tmp_path / "kb")
    os.makedirs(kb)
    np.save(os.path.join(kb, "reps.npy"), C[perm])
    with open(os.path.join(kb, "index2img_filename.txt"), "w") as f:
        f.write("\n".join(names[i] for i in perm))
    ix, nm = demo.load_document_base(kb, 0)
    doc = lambda pth: demo.doc_of_page(os.path.basename(pth))            # noqa: E731
    base = lambda pth: os.path.basename(pth)                             # noqa: E731
    paths, scores, ev = demo.retrieve_documents_any(kb, qv[:2], 5, None, None, index=ix, names=nm, fuse="min", return_evidence=True)
    assert len(paths) == 5 and len({doc(x) for x in paths}) == 5 and doc(paths[0]) == "deck_2.pdf"
    assert [base(x) for x, _ in ev[0]] == ["deck_2.pdf_1.png", "deck_2.pdf_4.png"] and all(doc(x) == doc(paths[i]) for i in range(5) for x, _ in ev[i])
    assert scores[0] == min(s for _, s in ev[0]) and scores == sorted(scores, reverse=True)
    anyof = demo.retrieve_documents_any(kb, qv, 2, None, None, index=ix, names=nm)
    assert {doc(x) for x in anyof} == {"deck_2.pdf", "deck_3.pdf"}
    only = demo.retrieve_documents_any(kb, qv, 10, None, None, index=ix, names=nm, documents=["deck_3.pdf", "other_7.pdf"])
    assert [doc(x) for x in only] == ["deck_3.pdf", "other_7.pdf"]
    with pytest.raises(ValueError):
        demo.retrieve_documents_any(kb, qv, 5, None, None, index=ix, names=nm, documents=["nowhere.pdf"])
    ix.close()
    assert demo.retrieve_documents_any(kb, qv[:2], 5, None, None, fuse="min") == paths      # an index of its own
