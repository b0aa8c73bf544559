"""-m gpu: the document window search (vr_index_search_groups_window / vr_index_group_window_search_stats,
csrc/search_group_window.hip) against the library's own fp32 scores — strict, bit for bit — and against the numpy reference
tests/group_window_search_ref.py.

Strict tests (no tolerance, host arrays and CUDA tensors): the oracle is the library's own fp32 score matrix, every row of
`search_range(threshold = -4, sort=False)`, masked, group-reduced and ranked in numpy on orderable bits
(group_window_search_ref.group_window_ref); scores, best rows and groups must equal it.  With offset 0 and no filter the result IS
`search_groups`, in every setting of `set_search_eps`; with groups of one row it IS `search_window` with groups == ids; pages
concatenated are every present document once; windows inside a tier of tied documents come in group order; an edited index
answers as a freshly built one.

Against fp64 (no excuse mechanism, the interval is the whole test): scores within ATOL = 1e-5 of the fp64 document score; the
document of fp64 score s at position j of the window at offset o has o + j in [#(E > s + 6e-7), #(E >= s - 6e-7) - 1] over the
present documents; the best row's fp64 score within 6e-7 of s.  Windows of k = 100; the reference alone gives these intervals for
the documents of its own windows (tests/test_cpu_group_window_search_ref.py pins them):

    case                              offset   filter density   entries   widened intervals
    (5000, 37, 256), mean 7                0        none          3 700          10
    (5000, 37, 256), mean 7              300        none          3 700          27
    (5000, 37, 256), mean 7              200        0.5           3 700          21
    (3001, 300, 128), mean 3             500        none         30 000         209
    (2000, 8, 2304), mean 5              100        0.5             800          10
    decks 300 x 10, noise 3e-4, dim 256  100        none          1 600           6
    decks 300 x 10, noise 3e-4, dim 2304 100        none          1 600           8

Measured on an MI355X (the same for host arrays and CUDA tensors): every position inside its interval; 2 of the 45 100 positions
differ from the reference's own fp64 ranking (0 / 0 / 0 / 2 / 0 / 0 / 0 in the table's order, inside near-ties); largest
|score - fp64| 2.8e-8 / 1.7e-8 / 1.8e-8 / 2.8e-8 / 6.1e-9 / 1.6e-8 / 5.9e-9.  Band documents re-scored per document returned:
1.31 / 1.92 / 1.72 / 1.82 / 1.96 / 1.25 / 1.71; fp32 page dots per document returned: 1.36 / 2.25 / 1.91 / 1.96 / 2.58 / 12.51 /
17.09 — in the decks every page of a band document lies within 2 eps of its document's maximum and is re-scored.
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
from tests import group_window_search_ref as G  # noqa: E402
from tests import range_search_ref as X  # noqa: E402
from tests import rank_search_ref as K  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.engine import HipIndex, _stream_ptr  # noqa: E402

VR_OK, VR_ERR_INVALID, VR_ERR_STATE = 0, 1, 3
CYCLE_C = (0.05, 0.07)
ZERO = {"queries": 0, "documents": 0, "page_dots": 0}


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


def _masks_of(M, foq, n):
    """bool [nq][rows]: the rows every query's filter allows (-1: all)"""
    return np.stack([np.ones(n, dtype=bool) if f < 0 else M[f] for f in foq])


def _ranking(S32, off, mask, pad):
    """the oracle's whole document ranking of every query, `pad` tails behind it -> (scores, best rows, groups) [nq][n_groups + pad]"""
    return G.group_window_ref(S32, off, mask, 0, len(off) - 1 + pad)


def _slices(full, o, k):
    """entries [o[q], o[q] + k) of every row of the padded ranking (o: an int or one per query)"""
    o = np.broadcast_to(np.asarray(o, dtype=np.int64), (len(full[0]),))
    cols = np.minimum(o[:, None] + np.arange(k)[None, :], full[0].shape[1] - 1)      # (past the padding: a tail like any other)
    return tuple(np.take_along_axis(a, cols, 1) for a in full)


def _same(got, want):
    sc, ids, gr = _np(*got)
    assert sc.dtype == np.float32 and ids.dtype == np.int64 and gr.dtype == np.int64 and sc.shape == ids.shape == gr.shape == want[2].shape
    assert np.array_equal(gr, want[2])
    assert np.array_equal(ids, want[1])
    assert np.array_equal(_u32(sc), _u32(want[0]))


# ------------------------------------------------------------------------------------------ 1. the whole ranking ---
@pytest.mark.parametrize("nd,nq,dim,mean", [(5000, 37, 256, 7), (5000, 37, 256, 1), (2000, 8, 2304, 5), (3001, 300, 128, 3)])
def test_windows_are_slices_of_the_oracles_ranking(nd, nq, dim, mean):
    C, Q = R.unit(nd, dim, 1), R.unit(nq, dim, 2)
    off = np.arange(nd + 1) if mean == 1 else R.random_offsets(nd, mean)
    ng = len(off) - 1
    assert ng == {7: 723, 1: 5000}.get(mean, ng)
    ix = _index(C, off)
    full = _ranking(_scores(ix, Q), off, None, 1010)
    assert (full[2][:, :ng] >= 0).all() and (full[2][:, ng:] == -1).all()
    qd = torch.tensor(Q).cuda()
    for k in (1, 10, 100, 1000):
        offsets = [0, 1, 7, ng // 2, max(ng - k, 0), ng - 3, ng, ng + 5]
        mixed = np.asarray(offsets, dtype=np.int64)[(np.arange(nq) * 3 + 1) % len(offsets)]
        for o in offsets + [mixed]:
            want = _slices(full, o, k)
            for cuda in (False, True):
                ix.group_window_search_stats(reset=True)
                got = ix.search_groups_window(qd if cuda else Q, torch.tensor(o) if cuda and not np.isscalar(o) else o, k)
                assert all((isinstance(x, torch.Tensor) and x.is_cuda) if cuda else isinstance(x, np.ndarray) for x in got)
                _same(got, want)
                st = ix.group_window_search_stats()
                assert st["queries"] == nq and st["page_dots"] >= st["documents"] >= int((want[2] >= 0).sum())
    for o in (0, ng // 2):
        ix.group_window_search_stats(reset=True)
        ix.search_groups_window(Q, o, 100)
        st = ix.group_window_search_stats()
        print(f"whole ranking {nd}x{nq}x{dim} mean {mean} offset {o} k 100: {st}, {st['documents'] / (nq * 100):.1f} band documents and "
              f"{st['page_dots'] / (nq * 100):.1f} page dots per document returned")
    ix.close()


# ------------------------------------------------------------------------------- 2. identity with search_groups ---
def test_offset_zero_without_a_filter_is_search_groups():
    C, Q, _, _ = X.random_case(20000, 64, 2304, CYCLE_C)
    off = R.random_offsets(20000, 10)
    ix = _index(C, off)
    qd = torch.tensor(Q).cuda()
    for k in (10, 100):
        ix.set_search_eps(float("nan"))                                  # the default setting
        want = ix.search_groups(Q, k)
        for q_in in (Q, qd):
            _same(ix.search_groups_window(q_in, 0, k), want)
        deep = ix.search_groups_window(Q, 40, k)
        for eps in (-1.0, 0.01):                                         # certification off / a caller's model: still the same result
            ix.set_search_eps(eps)
            _same(ix.search_groups_window(Q, 0, k), want)
            _same(ix.search_groups_window(qd, 40, k), deep)
    ix.set_search_eps(float("nan"))
    _same(ix.search_groups_window(Q, 40, 100), tuple(x[:, 40:] for x in ix.search_groups(Q, 140)))
    ix.close()


# ------------------------------------------------------------------------------------------------ 3. filters ---
@pytest.fixture(scope="module")
def filtered():
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    off = R.random_offsets(5000, 7)
    M = np.concatenate([F.random_filters(len(C), (0.5, 0.01), seed=11), np.zeros((1, len(C)), dtype=bool)])
    ix = _index(C, off, M)
    yield ix, C, Q, off, M, _scores(ix, Q)
    ix.close()


def test_windows_under_filters(filtered):
    ix, C, Q, off, M, S32 = filtered
    ng = len(off) - 1
    foq = (np.arange(len(Q)) % 4 - 1).astype(np.int64)                   # -1 (no filter), 0, 1, 2 (allows nothing), ...
    mask = _masks_of(M, foq, len(C))
    full = _ranking(S32, off, mask, 1100)
    present = (full[2] >= 0).sum(1)
    assert (present[foq == -1] == ng).all() and (present[foq == 2] == 0).all() and 25 < present[2] < 100 < present[1] < ng
    qd, fd = torch.tensor(Q).cuda(), torch.tensor(foq).cuda()
    for k in (10, 100, 1000):
        for o in (0, 20, int(present[2]) - 7, int(present[2]), int(present[1]) - 3, int(present[1]), ng - 3, ng):
            want = _slices(full, o, k)
            _same(ix.search_groups_window(Q, o, k, foq), want)
            _same(ix.search_groups_window(qd, o, k, fd), want)
    part = _np(*ix.search_groups_window(Q, int(present[2]) - 7, 10, foq))[2]
    assert (part[2] >= 0).sum() == 7 and (part[3] == -1).all()           # a partial tail; nothing at all under the empty filter
    o = np.maximum(present - 3, 0)                                       # per-query offsets: every query's own last three documents
    want = _slices(full, o, 10)
    _same(ix.search_groups_window(Q, o, 10, foq), want)
    assert np.array_equal((want[2] >= 0).sum(1), np.minimum(present, 3))
    # one filter for every query, and -1 / None = no filter
    for f in (0, 1, 2):
        _same(ix.search_groups_window(Q, 5, 20, f), _slices(_ranking(S32, off, M[f], 30), 5, 20))
    plain = ix.search_groups_window(Q, 10, 20)
    _same(ix.search_groups_window(Q, 10, 20, -1), plain)
    _same(plain, tuple(x[:, 10:] for x in ix.search_groups(Q, 30)))


def test_a_filter_on_the_queries_of_a_second_block():
    """600 rows, 257 queries (a second block of one query), a half-density and an empty filter mixed per query, per-query offsets:
    the block's filter ids and offsets start at its first query.  Query 256 is on filter 0."""
    C, Q = R.unit(600, 64, 1), R.unit(257, 64, 2)
    off = R.random_offsets(600, 3)
    M = np.concatenate([F.random_filters(600, (0.5,), seed=11), np.zeros((1, 600), dtype=bool)])
    foq = (np.arange(257) % 3 - 1).astype(np.int64)                      # -1 (no filter), 0, 1 (allows nothing), ...
    ix = _index(C, off, M)
    full = _ranking(_scores(ix, Q), off, _masks_of(M, foq, 600), 30)
    present = (full[2] >= 0).sum(1)
    assert foq[256] == 0 and 10 < present[256] < len(off) - 1 and (present[foq == 1] == 0).all()
    o = (np.arange(257) % 5).astype(np.int64)
    want = _slices(full, o, 20)
    _same(ix.search_groups_window(Q, o, 20, foq), want)
    _same(ix.search_groups_window(torch.tensor(Q).cuda(), torch.tensor(o), 20, torch.tensor(foq).cuda()), want)
    ix.close()


def test_a_filter_with_pages_in_three_documents_and_one_that_forbids_the_best_pages(filtered):
    ix, C, Q, off, M, S32 = filtered
    n = len(C)
    three = np.zeros(n, dtype=bool)
    three[[off[6] - 1, off[400], off[401] - 1, off[722]]] = True          # the last page of document 5, the ends of 400, the first of 722
    sc0, rows0, gr0 = ix.search_groups(Q[:1], 20)
    forbid = np.ones(n, dtype=bool)
    forbid[rows0[0]] = False                                             # the best page of each of query 0's top 20 documents
    ix.set_filters(np.stack([three, forbid]))
    try:
        for q_in in (Q, torch.tensor(Q).cuda()):
            sc, rows, gr = _np(*ix.search_groups_window(q_in, 0, 10, 0))
            _same((sc, rows, gr), _slices(_ranking(S32, off, three, 10), 0, 10))
            assert (np.sort(gr[:, :3], axis=1) == [5, 400, 722]).all() and (gr[:, 3:] == -1).all() and three[rows[:, :3]].all()
            sc, rows, gr = _np(*ix.search_groups_window(q_in, 0, 1000, 1))
            _same((sc, rows, gr), _slices(_ranking(S32, off, forbid, 300), 0, 1000))
            longer = 0
            for j, g in enumerate(gr0[0]):                               # every document that lost its best page
                pages = np.arange(off[g], off[g + 1])
                allowed = pages[forbid[pages]]
                at = np.flatnonzero(gr[0] == g)
                if len(allowed) == 0:
                    assert len(at) == 0                                  # ... a one-page document is absent
                    continue
                longer += 1                                              # ... a longer one scores as its best ALLOWED page does
                assert len(at) == 1 and rows[0, at[0]] == allowed[np.argmax(S32[0, allowed])] != rows0[0, j]
                assert _u32(sc[0, at[0]]) == _u32(S32[0, allowed].max()) and sc[0, at[0]] <= sc0[0, j]
            assert longer >= 10 and not np.isin(rows[0], rows0[0]).any()
            assert not np.array_equal(gr[0, :longer], [g for g in gr0[0] if off[g + 1] - off[g] > 1])         # the order changed with it
    finally:
        ix.set_filters(M)


def test_groups_of_one_row_are_the_windowed_search():
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    M = np.concatenate([F.random_filters(len(C), (0.5, 0.01), seed=11), np.zeros((1, len(C)), dtype=bool)])
    foq = (np.arange(len(Q)) % 4 - 1).astype(np.int64)
    ix = _index(C, np.arange(len(C) + 1), M)                             # 5 000 documents: the re-score grid has two chunks
    qd, fd = torch.tensor(Q).cuda(), torch.tensor(foq).cuda()
    for o, k in ((0, 10), (7, 100), (2400, 1000), (4090, 20), (4995, 10), (5000, 3)):
        for q_in, f_in in ((Q, foq), (qd, fd), (Q, None)):
            sc, ids = _np(*ix.search_window(q_in, o, k, f_in))
            _same(ix.search_groups_window(q_in, o, k, f_in), (sc, ids, ids))
    ix.close()


# ------------------------------------------------------------------------------------------- 4. group shapes ---
def test_group_shapes():
    n, dim = 6000, 64
    C, Q = R.unit(n, dim, 1), R.unit(9, dim, 2)
    lengths = [4500, 63, 64, 65, 1, 128, 129, 2, 62]                      # one document longer than a chunk of 4 096 rows; lengths around 64
    offs = {
        "one group": np.array([0, n]),
        "long and short": np.concatenate([[0], np.cumsum(lengths), np.arange(sum(lengths) + 4, n, 4), [n]]),
        "not a multiple of four": np.concatenate([np.arange(0, 5995, 5), [n]]),
    }
    assert (len(offs["not a multiple of four"]) - 1) % 4 == 3
    mask = F.random_filters(n, (0.5,), seed=5)
    ix = HipIndex(dim, n)
    ix.add(C)
    ix.set_filters(mask)
    S32 = _scores(ix, Q)
    qd = torch.tensor(Q).cuda()
    for name, off in offs.items():
        off = off.astype(np.int64)
        ix.set_groups(off)
        ng = len(off) - 1
        for f in (None, 0):
            full = _ranking(S32, off, None if f is None else mask[0], 120)
            for o, k in ((0, 1), (0, 10), (1, 100), (ng // 2, 100), (max(ng - 5, 0), 10)):
                want = _slices(full, o, k)
                _same(ix.search_groups_window(Q, o, k, f), want)
                _same(ix.search_groups_window(qd, o, k, f), want)
        if name == "one group":
            sc, rows, gr = ix.search_groups_window(Q, 0, 3)
            assert np.array_equal(rows[:, 0], S32.argmax(1)) and (gr[:, 0] == 0).all() and (gr[:, 1:] == -1).all()
            assert (ix.search_groups_window(Q, 1, 3)[2] == -1).all()
    ix.close()


# -------------------------------------------------------------------------------------------------- 5. paging ---
def test_pages_concatenated_are_every_present_document_once(filtered):
    ix, C, Q, off, M, S32 = filtered
    ng = len(off) - 1
    assert ng == 723
    for f, mask in ((None, None), (0, M[0])):
        full = _ranking(S32, off, mask, 900 - ng)
        present = int((full[2][0] >= 0).sum())
        for q_in in (Q, torch.tensor(Q).cuda()):
            pages = [_np(*ix.search_groups_window(q_in, o, 100, f)) for o in range(0, 900, 100)]
            got = tuple(np.concatenate([p[i] for p in pages], 1) for i in range(3))
            _same(got, full)
            assert np.array_equal(np.sort(got[2][:, :present], axis=1), np.sort(full[2][:, :present], axis=1))
            assert all(len(set(row[:present].tolist())) == present for row in got[2])                   # every document exactly once
            assert (got[2][:, present:] == -1).all() and np.isneginf(got[0][:, present:]).all()
            assert (np.diff(got[0][:, :present].astype(np.float64), axis=1) <= 0).all()                 # in order


# ---------------------------------------------------------------------------------------------------- 6. ties ---
def test_tied_documents_come_in_group_order():
    C, Q, _ = R.tie_tier()
    n = len(C)
    off = np.arange(0, n + 1, 5)                                          # 600 documents of five rows
    high = np.unique((7 * np.arange(100) + 3) // 5)                       # the 100 documents that hold a distinct high row
    tied = np.setdiff1d(np.arange(600), high)                             # 500 documents of five bit-identical rows: one tier
    assert len(high) == 100
    ix = _index(C, off)
    full = _ranking(_scores(ix, Q), off, None, 1000)
    assert np.isin(full[2][:, :100], high).all() and np.array_equal(full[2][:, 100:600], np.tile(tied, (3, 1)))
    assert np.array_equal(full[1][:, 100:600], np.tile(tied * 5, (3, 1)))                # the best row of a tied document: its first
    for o, k in ((50, 100), (150, 100), (200, 300), (550, 100), (100, 1), (99, 2), (599, 1), (0, 1000)):
        want = _slices(full, o, k)                                       # ends inside the tier / starts inside it / both / runs out of it
        for q_in in (Q, torch.tensor(Q).cuda()):
            _same(ix.search_groups_window(q_in, o, k), want)
    gr = ix.search_groups_window(Q, 200, 300)[2]
    assert np.array_equal(gr, np.tile(tied[100:400], (3, 1)))            # both edges inside the tier: consecutive documents, in order
    mask = np.ones(n, dtype=bool)
    mask[tied[:250] * 5] = False                                         # the first row of half the tied documents forbidden
    ix.set_filters(mask[None, :])
    sc, rows, gr = ix.search_groups_window(Q, 200, 300, 0)
    assert np.array_equal(gr, np.tile(tied[100:400], (3, 1)))            # ... they still tie, through their second row
    assert np.array_equal(rows, np.tile(np.where(np.arange(100, 400) < 250, tied[100:400] * 5 + 1, tied[100:400] * 5), (3, 1)))
    ix.close()


def test_decks_where_every_page_of_a_band_document_is_rescored():
    """300 decks of 10 pages, noise 3e-4, dim 2304: the pages of a deck score within ~1e-3 of each other, the error model's 2 eps
    is ~7e-3 (bf16 residual norms of ~1.7e-3 on either side), so every page of a band document passes the limit"""
    C, Q, off, S = G.case("decks-2304")
    ix = _index(C, off)
    full = _ranking(_scores(ix, Q), off, None, 100)
    mask = F.random_filters(len(C), (0.5,), seed=11)
    ix.set_filters(mask)
    fullf = _ranking(_scores(ix, Q), off, mask[0], 100)
    for o, k in ((0, 10), (100, 100), (250, 100)):
        for q_in in (Q, torch.tensor(Q).cuda()):
            ix.group_window_search_stats(reset=True)
            _same(ix.search_groups_window(q_in, o, k), _slices(full, o, k))
            st = ix.group_window_search_stats()
            assert st["page_dots"] == 10 * st["documents"] and st["documents"] >= len(Q) * min(k, 300 - o)
            ix.group_window_search_stats(reset=True)
            _same(ix.search_groups_window(q_in, o, k, 0), _slices(fullf, o, k))
            st = ix.group_window_search_stats()
            assert st["documents"] < st["page_dots"] < 10 * st["documents"]                  # only allowed pages are re-scored
    ix.close()


# --------------------------------------------------------------------------------------------------- 7. edits ---
def _vp(x):
    if x is None:
        return ctypes.c_void_p(None)
    return ctypes.c_void_p(x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data)


def _raw(ix, Q, offsets, k, foq=None, nq=None):
    """vr_index_search_groups_window itself, host arrays -> (status, scores, ids, groups); the outputs start as -7"""
    offsets = np.asarray(offsets, dtype=np.int64)
    n = max(len(Q) * max(k, 1), 1)
    sc, ids, gr = np.full(n, -7, dtype=np.float32), np.full(n, -7, dtype=np.int64), np.full(n, -7, dtype=np.int64)
    st = ix.lib.vr_index_search_groups_window(ix._h, _vp(Q), len(Q) if nq is None else nq, _vp(offsets), k, _vp(foq), _vp(sc), _vp(ids),
                                              _vp(gr), 0, ctypes.c_void_p(_stream_ptr(ix.device)))
    return st, sc, ids, gr


def test_an_edited_index_answers_as_a_fresh_one():
    C, Q = R.unit(3001, 128, 1).copy(), R.unit(40, 128, 2)
    off = R.random_offsets(3001, 3)
    rng = np.random.default_rng(17)
    gone_docs = rng.choice(len(off) - 1, 300, replace=False)
    gone = np.concatenate([np.arange(off[g], off[g + 1]) for g in gone_docs] + [off[[5, 9, 700]]])     # whole documents and single pages
    ix = _index(C, off)
    ix.search_groups_window(Q, 100, 10)                                  # (nothing is stored: nothing to invalidate)
    new_id = ix.remove(gone)
    assert _raw(ix, Q, np.zeros(40), 10)[0] == VR_ERR_STATE              # the grouping went with the removal
    assert "vr_index_set_groups" in _lib.load().vr_last_error().decode()
    with pytest.raises(_lib.VisragHipError):
        ix.search_groups_window(Q, 0, 10)
    left = C[new_id >= 0]
    gid = (np.searchsorted(off, np.arange(len(C)), side="right") - 1)[new_id >= 0]
    left_off = np.concatenate([[0], np.flatnonzero(np.diff(gid)) + 1, [len(left)]]).astype(np.int64)
    ix.set_groups(left_off)
    fresh = _index(left, left_off)
    ng = len(left_off) - 1
    for o in (0, 50, ng // 2, ng - 50):
        _same(ix.search_groups_window(Q, o, 100), fresh.search_groups_window(Q, o, 100))
    upd = rng.choice(len(left), 5, replace=False)
    fresh_rows = R.unit(5, 128, 33)
    ix.update(upd, fresh_rows)                                           # no row moves: the grouping stays
    left[upd] = fresh_rows
    fresh.close()
    fresh = _index(left, left_off)
    for o in (0, ng // 2):
        _same(ix.search_groups_window(Q, o, 100), fresh.search_groups_window(Q, o, 100))
    _same(ix.search_groups_window(Q, ng // 2, 100), _slices(_ranking(_scores(fresh, Q), left_off, None, 100), ng // 2, 100))
    ix.close(); fresh.close()


# ------------------------------------------------------------------------------------ 8. arguments, the raw ABI ---
def test_argument_checks_come_before_any_launch():
    n = 600
    C, Q = R.unit(n, 64, 1), R.unit(4, 64, 2)
    off = R.random_offsets(n, 4)
    M = F.random_filters(n, (0.5, 0.1), seed=11)
    foq = np.array([0, 1, -1, 1], dtype=np.int32)
    ix = HipIndex(64, n + 10)
    assert _raw(ix, Q, [0, 1, 2, 3], 5)[0] == VR_ERR_STATE               # the empty index has no grouping
    ix.add(C)
    assert _raw(ix, Q, [0, 1, 2, 3], 5)[0] == VR_ERR_STATE               # no grouping set
    assert ix.group_window_search_stats() == ZERO
    ix.set_groups(off)
    st, sc, ids, gr = _raw(ix, Q, [0, 1, 2, 3], 5, foq)
    assert st == VR_ERR_STATE and (sc == -7).all() and (ids == -7).all() and (gr == -7).all()      # filters named but none set
    ix.set_filters(M)
    S32 = _scores(ix, Q)
    offs = [0, 3, len(off) - 3, 700]
    st, sc, ids, gr = _raw(ix, Q, offs, 20, foq)
    assert st == VR_OK
    _same((sc.reshape(4, 20), ids.reshape(4, 20), gr.reshape(4, 20)), _slices(_ranking(S32, off, _masks_of(M, foq, n), 800), offs, 20))
    stats = ix.group_window_search_stats()
    assert stats["queries"] == 4
    before = (ix.search(Q, 10), ix.search_groups(Q, 10), ix.search_window(Q, 3, 10, foq.astype(np.int64)))
    others = (ix.search_stats(), ix.group_search_stats(), ix.filter_search_stats(), ix.range_search_stats(), ix.rank_search_stats(),
              ix.window_search_stats())

    def nothing_ran(st, *outs):
        return st == VR_ERR_INVALID and all((o == -7).all() for o in outs) and ix.group_window_search_stats() == stats

    for k in (0, -1, 1001):
        assert nothing_ran(*_raw(ix, Q, offs, k, foq)), k
    assert "k=1001 unsupported (1..1000)" in _lib.load().vr_last_error().decode()
    for bad in (-1, -(1 << 40)):                                         # a negative offset
        assert nothing_ran(*_raw(ix, Q, [0, 3, bad, 7], 20, foq)), bad
    assert "offsets[2]" in _lib.load().vr_last_error().decode()
    for bad in (2, -2):                                                  # a filter index out of range
        fb = np.array([0, bad, -1, 1], dtype=np.int32)
        assert nothing_ran(*_raw(ix, Q, offs, 20, fb))
        with pytest.raises(ValueError):
            ix.search_groups_window(Q, 0, 20, filter_of_query=fb)
    assert "outside [-1, 2)" in _lib.load().vr_last_error().decode()
    assert ix.lib.vr_index_search_groups_window(ix._h, _vp(Q), 4, _vp(None), 5, _vp(None), _vp(None), _vp(None), _vp(None), 0,
                                                None) == VR_ERR_INVALID
    assert nothing_ran(*_raw(ix, Q, offs, 20, foq, nq=-1))
    st, sc, ids, gr = _raw(ix, Q, offs, 20, foq, nq=0)                   # no query: VR_OK, nothing launched, nothing written
    assert st == VR_OK and (ids == -7).all() and (sc == -7).all() and (gr == -7).all() and ix.group_window_search_stats() == stats
    for bad_off in ([1, 2, 3], -1, [0, -5, 0, 0]):                       # the binding's own checks
        with pytest.raises(ValueError):
            ix.search_groups_window(Q, bad_off, 5)
    with pytest.raises(_lib.VisragHipError):
        ix.search_groups_window(Q, 0, 1001)
    # k = 1 000 is served (the grouped search's candidate margin is not this call's)
    assert _raw(ix, Q, offs, 1000, foq)[0] == VR_OK
    # on the device an out-of-range filter index cannot be seen before the launch: that query gets a row of tails
    qd = torch.tensor(Q).cuda()
    fb = torch.tensor(np.array([0, 7, -1, 1], dtype=np.int32)).cuda()
    out_s, out_i, out_g = torch.full((4, 5), -7.0).cuda(), torch.full((4, 5), -7, dtype=torch.int64).cuda(), torch.full((4, 5), -7, dtype=torch.int64).cuda()
    st = ix.lib.vr_index_search_groups_window(ix._h, _vp(qd), 4, _vp(np.zeros(4, dtype=np.int64)), 5, _vp(fb), _vp(out_s), _vp(out_i),
                                              _vp(out_g), 1, ctypes.c_void_p(_stream_ptr(ix.device)))
    torch.cuda.synchronize()
    want = _np(*ix.search_groups_window(Q, 0, 5, np.array([0, 0, -1, 1])))
    want[0][1], want[1][1], want[2][1] = -np.inf, -1, -1
    assert st == VR_OK
    _same((out_s, out_i, out_g), want)
    # no other search's state or counters were touched, and they answer with the same bits
    assert (ix.search_stats(), ix.group_search_stats(), ix.filter_search_stats(), ix.range_search_stats(), ix.rank_search_stats(),
            ix.window_search_stats()) == others
    after = (ix.search(Q, 10), ix.search_groups(Q, 10), ix.search_window(Q, 3, 10, foq.astype(np.int64)))
    for a, b in zip(before, after):
        assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                   for x, y in zip(a, b))
    st2 = ix.group_window_search_stats()
    assert ix.group_window_search_stats(reset=True) == st2 and ix.group_window_search_stats() == ZERO
    # rows appended: grouping and filters are gone with them
    ix.add(C[:10])
    assert ix.n_groups == 0 and _raw(ix, Q, offs, 20)[0] == VR_ERR_STATE
    ix.close()


# ------------------------------------------------------------------------------------------------ against fp64 ---
@pytest.mark.parametrize("name", list(G.TABLE))
def test_documents_and_scores_against_fp64(name):
    C, Q, off, S = G.case(name)
    k = G.K_FP64
    ix = _index(C, off)
    for o, density, (want_entries, _) in G.TABLE[name]:
        mask = G.case_mask(name, density)
        if mask is not None:
            ix.set_filters(mask[None, :])
        first = None
        for q_in in (Q, torch.tensor(Q).cuda()):
            ix.group_window_search_stats(reset=True)
            sc, ids, gr = _np(*ix.search_groups_window(q_in, o, k, None if mask is None else 0))
            st = ix.group_window_search_stats()
            entries = moved = 0
            worst, err = None, 0.0
            for q in range(len(Q)):
                n_q, moved_q, err_q, bad = G.check_docs(S[q], off, mask, sc[q], ids[q], gr[q], o)
                entries += n_q; moved += moved_q; err = max(err, err_q)
                worst = worst or (bad and (q,) + bad)
            print(f"{name} offset {o} density {density}: {entries} entries, {moved} positions differ from the fp64 ranking, max |score - fp64| "
                  f"{err:.2e}, {st['documents'] / max(entries, 1):.2f} band documents and {st['page_dots'] / max(entries, 1):.2f} page dots per "
                  f"document returned")
            assert entries == want_entries
            assert err <= G.ATOL
            assert worst is None, worst                                  # (query, position, document, lo, hi)
            if first is None:
                first = (_u32(sc).tolist(), ids.tolist(), gr.tolist())
            assert (_u32(sc).tolist(), ids.tolist(), gr.tolist()) == first           # host and device callers: the same bits
    ix.close()


# ------------------------------------------------------------------------------------------------ host consumers ---
def test_retrieve_documents_filtered_over_pickle_shards(tmp_path):
    from visrag_amd import retriever
    from visrag_amd.utils import write_shard
    C, Q, bounds = K.shards_case()                                       # shards of 1 000, 3 001 and 1 999 rows
    doc_of = lambda page: f"doc_{int(page.split('_')[1]) // 7}"          # noqa: E731  (documents of seven pages straddle the shards)
    label_of_doc = lambda d: int(d.split("_")[1]) % 3                    # noqa: E731
    names = [f"page_{i}" for i in range(len(C))]
    for s in range(3):
        write_shard(str(tmp_path / f"embeddings.corpus.rank.{s}"), C[bounds[s]:bounds[s + 1]], names[bounds[s]:bounds[s + 1]])
    qids = [f"q{q}" for q in range(len(Q))]
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, qids)
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    wanted = {q: (None, {0}, {1, 2})[i % 3] for i, q in enumerate(qids)}
    off = np.concatenate([np.arange(0, len(C), 7), [len(C)]])
    whole = _index(C, off)
    S32 = _scores(whole, Q)
    whole.close()
    docs = [f"doc_{g}" for g in range(len(off) - 1)]
    mask = np.stack([np.ones(len(C), dtype=bool) if wanted[q] is None else np.repeat(np.isin(np.arange(len(docs)) % 3, list(wanted[q])), np.diff(off))
                     for q in qids])
    for offset, topk in ((0, 10), (300, 25), (850, 20)):
        want = _slices(_ranking(S32, off, mask, 20), offset, topk)
        sc, pg = retriever.retrieve_documents_filtered(args, topk, doc_of, label_of_doc, lambda q: wanted[q], offset=offset)
        for qi, q in enumerate(qids):
            live = want[2][qi] >= 0
            assert list(sc[q]) == [docs[g] for g in want[2][qi][live]] == list(pg[q])
            assert np.array_equal(_u32(list(sc[q].values())), _u32(want[0][qi][live]))
            assert list(pg[q].values()) == [names[r] for r in want[1][qi][live]]
    assert len(sc["q0"]) == 8 and len(sc["q1"]) == 0                      # 858 documents; 286 of them in collection 0
    first = retriever.retrieve_documents_filtered(args, 10, doc_of, label_of_doc, lambda q: None)
    assert first == retriever.retrieve_documents(args, 10, doc_of)


def test_demo_retrieve_documents_with_documents_and_offset(tmp_path):
    from visrag_amd import demo
    D, _ = R.decks(6, 5, 64, 0.05)
    C = np.concatenate([D, R.unit(40, 64, 9)])
    names = [f"deck_{d}.pdf_{i}.png" for d in range(6) for i in range(5)] + [f"other_{j}.pdf_0.png" for j in range(40)]
    perm = np.random.default_rng(2).permutation(len(C))                  # on disk the pages of a document are not adjacent
    qvec = R.unit(6, 64, 5)[2:3]
    kb = str(tmp_path / "kb")
    os.makedirs(kb)
    np.save(os.path.join(kb, "reps.npy"), C[perm])
    with open(os.path.join(kb, "index2img_filename.txt"), "w") as f:
        f.write("\n".join(names[i] for i in perm))
    ix, nm = demo.load_document_base(kb, 0)
    doc = lambda p: demo.doc_of_page(os.path.basename(p))                # noqa: E731
    before = ix.group_window_search_stats()
    p46, s46 = demo.retrieve_documents(kb, qvec, 46, None, None, index=ix, names=nm, return_scores=True)
    assert ix.group_window_search_stats() == before                      # both at their defaults: search_groups, as before
    assert len(p46) == 46 and len({doc(p) for p in p46}) == 46
    for o in (0, 10, 40):
        p, s = demo.retrieve_documents(kb, qvec, 10, None, None, index=ix, names=nm, return_scores=True, offset=o)
        assert p == p46[o:o + 10] and np.array_equal(_u32(s), _u32(s46[o:o + 10]))
    assert ix.group_window_search_stats()["queries"] == before["queries"] + 2
    assert demo.retrieve_documents(kb, qvec, 10, None, None, index=ix, names=nm, offset=46) == []
    docs = ["deck_2.pdf", "other_7.pdf", "deck_4.pdf"]
    only, so = demo.retrieve_documents(kb, qvec, 10, None, None, index=ix, names=nm, documents=docs, return_scores=True)
    assert only == [p for p in p46 if doc(p) in docs] and np.array_equal(_u32(so), _u32([v for p, v in zip(p46, s46) if doc(p) in docs]))
    assert demo.retrieve_documents(kb, qvec, 5, None, None, index=ix, names=nm, documents=docs, offset=1) == only[1:]
    assert demo.retrieve_documents(kb, qvec, 5, None, None, index=ix, names=nm, documents=docs, offset=3) == []
    with pytest.raises(ValueError):
        demo.retrieve_documents(kb, qvec, 5, None, None, index=ix, names=nm, documents=["nowhere.pdf"])
    with pytest.raises(ValueError):
        demo.retrieve_documents(kb, qvec, 5, None, None, index=ix, names=nm, offset=-1)
    ix.close()
    assert demo.retrieve_documents(kb, qvec, 3, None, None, documents=docs, offset=1) == only[1:]      # an index of its own
