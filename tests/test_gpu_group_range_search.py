"""-m gpu: the document range search (vr_index_search_groups_range / vr_index_group_range_results /
vr_index_group_range_search_stats, csrc/search_group_range.hip) against the library's own fp32 scores — strict, bit for bit —
against the searches that stand and against the numpy reference tests/group_range_search_ref.py.

Strict tests (no tolerance, host arrays and CUDA tensors): the oracle is the library's own fp32 score matrix, every row of
`search_range(threshold = -4, sort=False)`, masked, group-reduced and thresholded in numpy
(group_range_search_ref.group_range_ref); lims, scores, best rows and groups must equal it, in the ABI's group order and in the
sorted order.  `np.diff(lims)` is `count_groups_range`; a sorted segment of m <= 1 000 entries is `search_groups_window(Q, 0, m)`;
with groups of one row the call IS `search_range`; a tie tier at the threshold comes whole or not at all; an edited index answers
as a freshly built one; no other search's state or counters are touched.

Against fp64 (the row-level range test's bar): scores within 1e-5 of the fp64 document score; the best row's fp64 score within
6e-7 of it; membership identical to the reference's except for a pair whose fp64 score lies within 3e-7 of the threshold, such
pairs at most 0.5 % of the reference's entries.  The reference alone has NO such pair on these cases
(tests/test_cpu_group_range_search_ref.py pins that and the entries):

    case                                  thresholds (cycling)        entries: no filter / density 0.5
    (5000, 37, 256), mean 7               0.10, 0.15, 0.20, 0.30            2 644 /  1 430
    (3001, 300, 128), mean 3              0.15, 0.25, 0.05                 73 596 / 43 193
    (2000, 8, 2304), mean 5               0.05, 0.07                           68 /     31
    decks 300 x 10, noise 3e-4, dim 256   0.10, 0.15, 0.20                    106 /    105
    decks 300 x 10, noise 3e-4, dim 2304  0.03, 0.05, 0.07                    157 /    154

Measured on an MI355X (the same bits from host arrays and CUDA tensors): 0 excused pairs in every case, without and under the
filter — membership is the fp64 reference's; largest |score - fp64| 2.5e-8 / 5.3e-8 / 7.0e-9 / 2.3e-8 / 7.3e-9 in the table's
order.  Band documents re-scored / fp32 page dots per document returned, without the filter: 1.10 / 1.16, 1.04 / 1.09,
1.63 / 1.68, 1.11 / 11.1, 1.40 / 14.0 — in the decks every page of a band document lies within 2 eps of its document's maximum
and is re-scored.
"""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import filter_search_ref as F  # noqa: E402
from tests import group_range_search_ref as N  # noqa: E402
from tests import group_search_ref as R  # noqa: E402
from tests import group_window_search_ref as G  # noqa: E402
from tests.rank_search_ref import shards_case  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.engine import HipIndex, _stream_ptr  # noqa: E402

VR_OK, VR_ERR_INVALID, VR_ERR_STATE, VR_ERR_CAPACITY = 0, 1, 3, 4
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


def _cycle(values, nq):
    return np.asarray(values, dtype=np.float32)[np.arange(nq) % len(values)]


def _same(got, want, cuda=None):
    if cuda is not None:
        assert all((isinstance(x, torch.Tensor) and x.is_cuda) if cuda else isinstance(x, np.ndarray) for x in got)
    lims, sc, rows, gr = _np(*got)
    assert lims.dtype == np.int64 and sc.dtype == np.float32 and rows.dtype == np.int64 and gr.dtype == np.int64
    assert np.array_equal(lims, want[0])
    assert np.array_equal(gr, want[3])
    assert np.array_equal(rows, want[2])
    assert np.array_equal(_u32(sc), _u32(want[1]))


def _check(ix, Q, t, S32, off, mask, foq=None):
    """the call from host arrays and from cuda tensors, in both orders, against the oracle, the count and the window -> lims"""
    want = N.group_range_ref(S32, off, mask, t)
    want_sorted = N.sort_group_ranges(*want)
    m = np.diff(want[0])
    for cuda in (False, True):
        q_in = torch.tensor(Q).cuda() if cuda else Q
        f_in = foq if foq is None or np.isscalar(foq) else (torch.tensor(np.asarray(foq)).cuda() if cuda else foq)
        t_in = torch.tensor(t).cuda() if cuda and not np.isscalar(t) else t
        _same(ix.search_groups_range(q_in, t_in, f_in, sort=False), want, cuda)
        got = ix.search_groups_range(q_in, t_in, f_in)
        _same(got, want_sorted, cuda)
        assert np.array_equal(_np(ix.count_groups_range(q_in, t, filter_of_query=f_in))[0], m)
        k = int(min(1000, m.max()))
        if k > 0:                                                        # a sorted segment of m <= 1 000 entries IS the window at offset 0
            wsc, wrows, wgr = _np(*ix.search_groups_window(q_in, 0, k, f_in))
            lims, sc, rows, gr = _np(*got)
            for q in np.flatnonzero(m <= 1000):
                a, b = lims[q], lims[q + 1]
                assert np.array_equal(gr[a:b], wgr[q, :m[q]]) and np.array_equal(rows[a:b], wrows[q, :m[q]])
                assert np.array_equal(_u32(sc[a:b]), _u32(wsc[q, :m[q]]))
    return want[0]


# ------------------------------------------------------------------------------- 1. corpora and thresholds ---
@pytest.mark.parametrize("nd,nq,dim,mean,cycle", [(5000, 37, 256, 7, (0.10, 0.15, 0.20, 0.30)), (5000, 37, 256, 1, (0.10, 0.15, 0.20, 0.30)),
                                                  (2000, 8, 2304, 5, (0.05, 0.07)), (3001, 300, 128, 3, (0.15, 0.25, 0.05))])
def test_the_call_is_the_oracle(nd, nq, dim, mean, cycle):
    C, Q = R.unit(nd, dim, 1), R.unit(nq, dim, 2)
    off = np.arange(nd + 1) if mean == 1 else R.random_offsets(nd, mean)      # mean 1: 5 000 groups: two re-score chunks, five scan slots
    ng = len(off) - 1
    assert ng == {7: 723, 1: 5000}.get(mean, ng)
    ix = _index(C, off)
    S32 = _scores(ix, Q)
    t = _cycle(cycle, nq)
    ix.group_range_search_stats(reset=True)
    lims = _check(ix, Q, t, S32, off, None)
    st = ix.group_range_search_stats()
    assert st["queries"] == 4 * nq and st["page_dots"] >= st["documents"] >= 4 * lims[-1]
    print(f"{nd}x{nq}x{dim} mean {mean}: {lims[-1]} entries, {st['documents'] / max(4 * lims[-1], 1):.2f} band documents and "
          f"{st['page_dots'] / max(4 * lims[-1], 1):.2f} page dots per document returned")
    if nq == 300:                                                        # two query blocks, and more than the first reservation of 65 536
        assert lims[256] > 0 and lims[-1] > lims[256] and lims[-1] > 65536
    _same(ix.search_groups_range(Q, 0.2, sort=False), N.group_range_ref(S32, off, None, 0.2))          # a scalar threshold
    _same(ix.search_groups_range(Q, -4.0, sort=False), N.group_range_ref(S32, off, None, -4.0))        # every document
    assert ix.search_groups_range(Q, 4.0)[0][-1] == 0                    # none
    if mean == 1:                                                        # groups of one: the call IS search_range, groups == rows
        rl, rs, ri = ix.search_range(Q, t, sort=False)
        gl, gs, grow, gg = ix.search_groups_range(Q, t, sort=False)
        assert np.array_equal(gl, rl) and np.array_equal(_u32(gs), _u32(rs)) and np.array_equal(grow, ri) and np.array_equal(gg, ri)
    ix.close()


# ------------------------------------------------------------------------------------------------ 2. filters ---
@pytest.fixture(scope="module")
def filtered():
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    off = R.random_offsets(5000, 7)
    M = np.concatenate([F.random_filters(len(C), (0.5, 0.01), seed=11), np.zeros((1, len(C)), dtype=bool)])
    ix = _index(C, off, M)
    yield ix, C, Q, off, M, _scores(ix, Q)
    ix.close()


def test_filters_of_every_density_and_a_per_query_mix(filtered):
    ix, C, Q, off, M, S32 = filtered
    t = _cycle((0.10, 0.15, 0.20, 0.30), len(Q))
    for f in (0, 1, 2):                                                  # densities 0.5, 0.01 and 0
        lims = _check(ix, Q, t, S32, off, M[f], f)
        assert (lims[-1] == 0) == (f == 2)
    foq = (np.arange(len(Q)) % 4 - 1).astype(np.int32)                   # -1 (no filter), 0 (0.5), 1 (0.01), 2 (allows nothing), ...
    lims = _check(ix, Q, t, S32, off, _masks_of(M, foq, len(C)), foq)
    assert (np.diff(lims)[foq == 2] == 0).all() and lims[-1] > 0
    _same(ix.search_groups_range(Q, t, -1), ix.search_groups_range(Q, t))
    t_low = np.full(len(Q), -4.0, dtype=np.float32)                      # every PRESENT document, and no absent one
    lims = _check(ix, Q, t_low, S32, off, M[1], 1)
    present = int(G.present_best(S32[:1], off, M[1])[2].sum())
    assert 0 < present < len(off) - 1 and np.array_equal(np.diff(lims), np.full(len(Q), present))


def test_groups_of_one_row_are_search_range_under_the_same_filter():
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    M = np.concatenate([F.random_filters(len(C), (0.5, 0.01), seed=11), np.zeros((1, len(C)), dtype=bool)])
    foq = (np.arange(len(Q)) % 4 - 1).astype(np.int32)
    ix = _index(C, np.arange(len(C) + 1), M)
    t = _cycle((0.10, 0.15, 0.20, 0.30), len(Q))
    for q_in, f_in in ((Q, foq), (torch.tensor(Q).cuda(), torch.tensor(foq).cuda())):
        for sort in (False, True):
            rl, rs, ri = _np(*ix.search_range(q_in, t, f_in, sort=sort))
            gl, gs, grow, gg = _np(*ix.search_groups_range(q_in, t, f_in, sort=sort))
            assert rl[-1] > 100
            assert np.array_equal(gl, rl) and np.array_equal(_u32(gs), _u32(rs)) and np.array_equal(grow, ri) and np.array_equal(gg, ri)
    ix.close()


def test_a_filter_that_forbids_the_best_page_of_the_top_documents(filtered):
    ix, C, Q, off, M, S32 = filtered
    sc0, rows0, gr0 = ix.search_groups(Q[:1], 20)
    forbid = np.ones(len(C), dtype=bool)
    forbid[rows0[0]] = False                                             # the best page of each of query 0's top 20 documents
    ix.set_filters(forbid[None, :])
    try:
        t = np.float32(sc0[0, 19])                                       # without the filter: exactly those 20 (and later ties)
        free = _check(ix, Q[:1], np.asarray([t]), S32[:1], off, None)
        assert free[-1] >= 20
        lims = _check(ix, Q[:1], np.asarray([t]), S32[:1], off, forbid, 0)
        assert lims[-1] < free[-1]                                       # a document whose best ALLOWED page is below t is out
        _, sc, rows, gr = ix.search_groups_range(Q[:1], -4.0, 0, sort=False)
        longer = 0
        for j, g in enumerate(gr0[0]):
            pages = np.arange(off[g], off[g + 1])
            allowed = pages[forbid[pages]]
            if len(allowed) == 0:                                        # a one-page document is absent
                assert g not in gr
                continue
            longer += 1                                                  # a longer one scores as its best ALLOWED page does
            at = int(np.flatnonzero(gr == g)[0])
            assert rows[at] == allowed[np.argmax(S32[0, allowed])] != rows0[0, j] and sc[at] <= sc0[0, j]
        assert longer >= 10
    finally:
        ix.set_filters(M)


# ------------------------------------------------------------------ 3. a threshold taken from the window's own scores ---
def test_a_threshold_at_the_30th_score_of_the_window_returns_its_first_30(filtered):
    ix, C, Q, off, M, S32 = filtered
    for f in (None, 0):
        wsc, wrows, wgr = ix.search_groups_window(Q, 0, 60, f)
        t = np.ascontiguousarray(wsc[:, 29])
        for q_in in (Q, torch.tensor(Q).cuda()):
            lims, sc, rows, gr = _np(*ix.search_groups_range(q_in, t, f))
            m = np.diff(lims)
            assert (m >= 30).all() and (m < 60).all()
            for q in range(len(Q)):
                a = lims[q]
                assert np.array_equal(gr[a:a + m[q]], wgr[q, :m[q]]) and np.array_equal(rows[a:a + m[q]], wrows[q, :m[q]])
                assert np.array_equal(_u32(sc[a:a + m[q]]), _u32(wsc[q, :m[q]]))
                assert (sc[a + 29:a + m[q]] == t[q]).all()               # beyond the 30th: later members of its tie only


# ------------------------------------------------------------------------------------------- 4. group shapes ---
def test_group_shapes():
    n, dim = 6000, 64
    C, Q = R.unit(n, dim, 1), R.unit(9, dim, 2)
    lengths = [4500, 63, 64, 65, 1, 128, 129, 2, 62]                      # one document longer than a chunk of 4 096 rows; lengths around 64
    offs = {
        "one group": np.array([0, n]),
        "long and short": np.concatenate([[0], np.cumsum(lengths), np.arange(sum(lengths) + 4, n, 4), [n]]),
        "1 199 groups": np.concatenate([np.arange(0, 5995, 5), [n]]),
    }
    assert len(offs["1 199 groups"]) - 1 == 1199
    mask = F.random_filters(n, (0.5,), seed=5)
    ix = HipIndex(dim, n)
    ix.add(C)
    ix.set_filters(mask)
    S32 = _scores(ix, Q)
    for name, off in offs.items():
        off = off.astype(np.int64)
        ix.set_groups(off)
        for f in (None, 0):
            m = None if f is None else mask[0]
            E = G.present_best(S32, off, m)[0]
            # thresholds at a document's own score (the comparison is >=), between scores and below everything
            for t in (E[:, 0].astype(np.float32), np.sort(E, axis=1)[:, E.shape[1] // 2].astype(np.float32), _cycle((0.3, 0.0, -0.0, -4.0), len(Q))):
                _check(ix, Q, np.ascontiguousarray(t), S32, off, m, f)
        if name == "one group":
            lims, sc, rows, gr = ix.search_groups_range(Q, S32.max(1))
            assert np.array_equal(lims, np.arange(10)) and np.array_equal(rows, S32.argmax(1)) and (gr == 0).all()
            assert np.array_equal(_u32(sc), _u32(S32.max(1)))
            assert ix.search_groups_range(Q, np.nextafter(S32.max(1), np.float32(4)))[0][-1] == 0
    ix.close()


# --------------------------------------------------------------------------------------------------- 5. ties ---
def test_a_tie_tier_at_the_threshold_comes_whole_or_not_at_all():
    C, Q, _ = R.tie_tier()
    n = len(C)
    off = np.arange(0, n + 1, 5)                                          # 600 documents of five rows
    high = np.unique((7 * np.arange(100) + 3) // 5)                       # the 100 documents that hold a distinct high row
    tied = np.setdiff1d(np.arange(600), high)                             # 500 documents of five bit-identical rows: one tier
    ix = _index(C, off)
    S32 = _scores(ix, Q)
    tier = S32[:, tied[0] * 5].copy()                                    # the tier's score of every query
    assert (_u32(S32[:, tied * 5]) == _u32(tier)[:, None]).all()
    above = np.nextafter(tier, np.float32(np.inf))
    lims = _check(ix, Q, tier, S32, off, None)
    assert np.array_equal(np.diff(lims), np.full(3, 600))
    lims = _check(ix, Q, above, S32, off, None)
    assert np.array_equal(np.diff(lims), np.full(3, 100))
    _, sc, rows, gr = ix.search_groups_range(Q, tier)
    assert np.array_equal(gr.reshape(3, 600)[:, 100:], np.tile(tied, (3, 1))) and np.array_equal(rows.reshape(3, 600)[:, 100:], np.tile(tied * 5, (3, 1)))
    mask = np.ones(n, dtype=bool)
    mask[tied * 5] = False                                               # the first row of every tied document forbidden
    ix.set_filters(mask[None, :])
    lims = _check(ix, Q, tier, S32, off, mask, 0)
    assert np.array_equal(np.diff(lims), np.full(3, 600))                # ... they still tie, through their second row
    _, sc, rows, gr = ix.search_groups_range(Q, tier, 0)
    assert np.array_equal(rows.reshape(3, 600)[:, 100:], np.tile(tied * 5 + 1, (3, 1)))
    assert np.array_equal(np.diff(_check(ix, Q, above, S32, off, mask, 0)), np.full(3, 100))
    ix.close()


def test_decks_where_every_page_of_a_band_document_is_rescored():
    """300 decks of 10 pages, noise 3e-4, dim 2304: the pages of a deck score within ~1e-3 of each other, the error model's 2 eps
    is ~7e-3, so every page of a band document passes the limit"""
    C, Q, off, S = G.case("decks-2304")
    ix = _index(C, off)
    S32 = _scores(ix, Q)
    t = N.case_thresholds("decks-2304", len(Q))
    want = N.group_range_ref(S32, off, None, t)
    for q_in in (Q, torch.tensor(Q).cuda()):
        ix.group_range_search_stats(reset=True)
        _same(ix.search_groups_range(q_in, t, sort=False), want)
        st = ix.group_range_search_stats()
        assert st["queries"] == len(Q) and st["documents"] >= want[0][-1] > 0 and st["page_dots"] == 10 * st["documents"]
    ix.close()


# ----------------------------------------------------------------------------------------------- 6. settings ---
def test_the_same_bits_in_every_setting_of_set_search_eps(filtered):
    ix, C, Q, off, M, S32 = filtered
    t = _cycle((0.10, 0.15, 0.20, 0.30), len(Q))
    want = N.group_range_ref(S32, off, M[0], t)
    try:
        for eps in (float("nan"), -1.0, 0.01):                           # the default / certification off / a caller's model
            ix.set_search_eps(eps)
            _same(ix.search_groups_range(Q, t, 0, sort=False), want)
            _same(ix.search_groups_range(torch.tensor(Q).cuda(), t, 0, sort=False), want)
    finally:
        ix.set_search_eps(float("nan"))


# ------------------------------------------------------------------------------------- 7. lifecycle and errors ---
def _vp(x):
    if x is None:
        return ctypes.c_void_p(None)
    return ctypes.c_void_p(x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data)


def _raw(ix, Q, thr, foq=None, max_total=1 << 20, nq=None):
    """vr_index_search_groups_range itself, host arrays -> (status, lims, total); the outputs start as -7"""
    thr = np.ascontiguousarray(thr, dtype=np.float32)
    lims = np.full(len(Q) + 1, -7, dtype=np.int64)
    total = ctypes.c_int64(-7)
    st = ix.lib.vr_index_search_groups_range(ix._h, _vp(Q), len(Q) if nq is None else nq, _vp(thr), _vp(foq), max_total, _vp(lims),
                                             ctypes.byref(total), 0, ctypes.c_void_p(_stream_ptr(ix.device)))
    return st, lims, total.value


def _raw_results(ix, n):
    sc, rows, gr = np.full(max(n, 1), -7, dtype=np.float32), np.full(max(n, 1), -7, dtype=np.int64), np.full(max(n, 1), -7, dtype=np.int64)
    st = ix.lib.vr_index_group_range_results(ix._h, _vp(sc), _vp(rows), _vp(gr), n, 0, ctypes.c_void_p(_stream_ptr(ix.device)))
    return st, sc, rows, gr


def test_the_stored_result_and_what_drops_it():
    C, Q = R.unit(3001, 128, 1), R.unit(40, 128, 2)
    off = R.random_offsets(3001, 3)
    ix = HipIndex(128, len(C) + 10)
    assert _raw_results(ix, 1)[0] == VR_ERR_STATE                        # before any search
    st, lims, total = _raw(ix, Q, np.zeros(40))                          # an empty index: zeros, nothing launched
    assert st == VR_OK and (lims == 0).all() and total == 0 and ix.group_range_search_stats() == ZERO
    assert _raw_results(ix, 0)[0] == VR_OK and _raw_results(ix, 1)[0] == VR_ERR_STATE
    ix.add(C)
    assert _raw_results(ix, 0)[0] == VR_ERR_STATE                        # rows appended: the (empty) result is gone
    ix.set_groups(off)
    S32 = _scores(ix, Q)
    t = np.full(40, 0.15, dtype=np.float32)
    want = N.group_range_ref(S32, off, None, t)

    def search():
        st, lims, total = _raw(ix, Q, t)
        assert st == VR_OK and total == want[0][-1] > 10 and np.array_equal(lims, want[0])
        return total

    total = search()
    st, sc, rows, gr = _raw_results(ix, total)
    assert st == VR_OK
    _same((want[0], sc, rows, gr), want)
    st, sc, rows, gr = _raw_results(ix, 7)                               # a prefix
    assert st == VR_OK and np.array_equal(gr, want[3][:7])
    st, sc, rows, gr = _raw_results(ix, total + 1)                       # more than the total
    assert st == VR_ERR_STATE and (sc == -7).all() and (rows == -7).all() and (gr == -7).all()
    assert "found" in _lib.load().vr_last_error().decode()
    ix.set_groups(off)                                                   # a grouping set anew: the groups it named are gone
    assert _raw_results(ix, 1)[0] == VR_ERR_STATE
    search()
    ix.update([5], R.unit(1, 128, 33))                                   # a row overwritten
    assert _raw_results(ix, 1)[0] == VR_ERR_STATE
    ix.update([5], C[5:6])
    search()
    ix.reset()
    assert _raw_results(ix, 1)[0] == VR_ERR_STATE and "vr_index_search_groups_range" in _lib.load().vr_last_error().decode()
    ix.close()


def test_an_edited_index_answers_as_a_fresh_one():
    C, Q = R.unit(3001, 128, 1).copy(), R.unit(40, 128, 2)
    off = R.random_offsets(3001, 3)
    rng = np.random.default_rng(17)
    gone_docs = rng.choice(len(off) - 1, 300, replace=False)
    gone = np.concatenate([np.arange(off[g], off[g + 1]) for g in gone_docs] + [off[[5, 9, 700]]])     # whole documents and single pages
    ix = _index(C, off)
    t = _cycle((0.15, 0.25, 0.05), 40)
    total = ix.search_groups_range(Q, t)[0][-1]
    assert total > 0
    new_id = ix.remove(gone)
    assert _raw_results(ix, 1)[0] == VR_ERR_STATE                        # its rows and groups name the index as it was
    st, lims, tot = _raw(ix, Q, t)
    assert st == VR_ERR_STATE and (lims == -7).all() and tot == -7       # the grouping went with the removal
    assert "vr_index_set_groups" in _lib.load().vr_last_error().decode()
    with pytest.raises(_lib.VisragHipError):
        ix.search_groups_range(Q, t)
    left = C[new_id >= 0]
    gid = (np.searchsorted(off, np.arange(len(C)), side="right") - 1)[new_id >= 0]
    left_off = np.concatenate([[0], np.flatnonzero(np.diff(gid)) + 1, [len(left)]]).astype(np.int64)
    ix.set_groups(left_off)
    fresh = _index(left, left_off)
    _same(ix.search_groups_range(Q, t), fresh.search_groups_range(Q, t))
    upd = rng.choice(len(left), 5, replace=False)
    fresh_rows = R.unit(5, 128, 33)
    ix.update(upd, fresh_rows)                                           # no row moves: the grouping stays
    left[upd] = fresh_rows
    fresh.close()
    fresh = _index(left, left_off)
    _same(ix.search_groups_range(Q, t), fresh.search_groups_range(Q, t))
    _same(ix.search_groups_range(Q, t, sort=False), N.group_range_ref(_scores(fresh, Q), left_off, None, t))
    ix.close(); fresh.close()


def test_the_store_grows_in_the_second_block_and_a_capacity_failure_there():
    """800 rows in 400 documents of two, 300 queries (two blocks); thresholds -4 (every document) for queries 0..155 and 256..299, 4
    (none) between them.  Block 0 packs 62 400 entries into the first reservation of 65 536; block 1's 17 600 make the store grow
    with those kept.  A fresh index per caller, so that the device caller and the host caller each grow it.  With max_total one
    short the failure is raised in block 1: no result is left."""
    C, Q = R.unit(800, 64, 1), R.unit(300, 64, 2)
    off = np.arange(0, 801, 2)
    t = np.where((np.arange(300) < 156) | (np.arange(300) >= 256), -4.0, 4.0).astype(np.float32)
    for cuda in (True, False):
        ix = _index(C, off)
        want = N.group_range_ref(_scores(ix, Q), off, None, t)
        assert want[0][256] == 62400 and want[0][300] == 80000
        q_in, t_in = (torch.tensor(Q).cuda(), torch.tensor(t).cuda()) if cuda else (Q, t)
        _same(ix.search_groups_range(q_in, t_in, sort=False), want, cuda)
        st, _, total = _raw(ix, Q, t, max_total=79999)
        assert st == VR_ERR_CAPACITY and total == -7 and "query block 1" in _lib.load().vr_last_error().decode()
        assert _raw_results(ix, 0)[0] == VR_ERR_STATE and _raw_results(ix, 1)[0] == VR_ERR_STATE
        st, lims, total = _raw(ix, Q, t, max_total=80000)                # exactly enough
        assert st == VR_OK and total == 80000
        _same((lims,) + tuple(_raw_results(ix, total)[1:]), want)
        ix.close()


def test_capacity_argument_checks_and_the_other_searches_state():
    n = 600
    C, Q = R.unit(n, 64, 1), R.unit(4, 64, 2)
    off = R.random_offsets(n, 4)
    ng = len(off) - 1
    M = F.random_filters(n, (0.5, 0.1), seed=11)
    foq = np.array([0, 1, -1, 1], dtype=np.int32)
    thr = np.array([0.0, -0.1, 0.1, -4.0], dtype=np.float32)
    ix = HipIndex(64, n + 10)
    ix.add(C)
    assert _raw(ix, Q, thr)[0] == VR_ERR_STATE and ix.group_range_search_stats() == ZERO               # no grouping set
    ix.set_groups(off)
    st, lims, total = _raw(ix, Q, thr, foq)
    assert st == VR_ERR_STATE and (lims == -7).all() and total == -7     # filters named but none set
    ix.set_filters(M)
    S32 = _scores(ix, Q)
    mask = _masks_of(M, foq, n)
    want = N.group_range_ref(S32, off, mask, thr)
    st, lims, total = _raw(ix, Q, thr, foq)
    assert st == VR_OK and np.array_equal(lims, want[0]) and total == want[0][-1] > 20
    _same((lims,) + tuple(_raw_results(ix, total)[1:]), want)
    # ---- the other searches: same bits, unchanged counters, a stored range result survives
    fl = foq.astype(np.int64)
    run_others = lambda: (ix.search(Q, 10), ix.search_range(Q, 0.1), ix.search_groups(Q, 10), ix.search_groups_window(Q, 3, 10, fl),   # noqa: E731
                          (ix.count_groups_range(Q, thr, filter_of_query=fl),))
    before = run_others()
    rl, rs, ri = ix.search_range(Q, 0.05, sort=False)                    # ... stored before the call
    others = lambda: (ix.search_stats(), ix.group_search_stats(), ix.filter_search_stats(), ix.range_search_stats(), ix.rank_search_stats(),   # noqa: E731
                      ix.window_search_stats(), ix.group_window_search_stats(), ix.group_rank_search_stats())
    counters = others()
    for q_in, f_in in ((Q, foq), (torch.tensor(Q).cuda(), torch.tensor(foq).cuda())):
        _same(ix.search_groups_range(q_in, thr, f_in, sort=False), want)
    assert others() == counters
    sc2, id2 = np.empty(rl[-1], dtype=np.float32), np.empty(rl[-1], dtype=np.int64)
    assert ix.lib.vr_index_range_results(ix._h, _vp(sc2), _vp(id2), int(rl[-1]), 0, ctypes.c_void_p(_stream_ptr(ix.device))) == VR_OK
    assert np.array_equal(_u32(sc2), _u32(rs)) and np.array_equal(id2, ri)
    # ---- capacity
    stats = ix.group_range_search_stats()
    assert stats["queries"] == 12
    st, lims, total = _raw(ix, Q, thr, foq, max_total=int(want[0][-1]) - 1)
    assert st == VR_ERR_CAPACITY and total == -7
    msg = _lib.load().vr_last_error().decode()
    assert "max_total" in msg and "query block 0" in msg
    assert _raw_results(ix, 1)[0] == VR_ERR_STATE                        # the previous result is gone
    with pytest.raises(_lib.VisragHipError):
        ix.search_groups_range(Q, thr, foq, max_total=3)
    st, lims, total = _raw(ix, Q, thr, foq, max_total=int(want[0][-1]))  # exactly enough; a later call succeeds
    assert st == VR_OK and total == want[0][-1]
    stats = ix.group_range_search_stats()

    # ---- argument checks: before any launch, outputs and the stored result untouched
    def nothing_ran(st, lims, total, code=VR_ERR_INVALID):
        return st == code and (lims == -7).all() and total == -7 and ix.group_range_search_stats() == stats and \
            _raw_results(ix, int(want[0][-1]))[0] == VR_OK

    assert nothing_ran(*_raw(ix, Q, thr, foq, max_total=0))
    assert "max_total" in _lib.load().vr_last_error().decode()
    assert nothing_ran(*_raw(ix, Q, thr, foq, nq=0)) and nothing_ran(*_raw(ix, Q, thr, foq, nq=-1))
    for bad in (np.nan, np.inf, -np.inf):                                # a host threshold that is not finite
        assert nothing_ran(*_raw(ix, Q, [0.1, 0.2, bad, 0.1], foq))
    assert "thresholds[2]" in _lib.load().vr_last_error().decode()
    for bad in (2, -2):                                                  # a host filter index out of range
        fb = np.array([0, bad, -1, 1], dtype=np.int32)
        assert nothing_ran(*_raw(ix, Q, thr, fb))
        with pytest.raises(ValueError):
            ix.search_groups_range(Q, thr, fb)
    total = ctypes.c_int64(-7)
    assert ix.lib.vr_index_search_groups_range(ix._h, _vp(Q), 4, _vp(None), _vp(None), 10, _vp(None), ctypes.byref(total), 0, None) == VR_ERR_INVALID
    assert ix.lib.vr_index_group_range_results(ix._h, _vp(None), _vp(None), _vp(None), 3, 0, None) == VR_ERR_INVALID
    with pytest.raises(ValueError):
        ix.search_groups_range(Q, [0.1, 0.2])                            # the binding's own check: one threshold per query
    # ---- on the device neither a threshold nor a filter index can be seen before the launch: an empty segment
    qd = torch.tensor(Q).cuda()
    fb = torch.tensor(np.array([0, 7, -1, 1], dtype=np.int32)).cuda()
    tb = torch.tensor(np.array([0.0, -0.1, np.nan, np.inf], dtype=np.float32)).cuda()
    ld = torch.full((5,), -7, dtype=torch.int64).cuda()
    total = ctypes.c_int64(-7)
    st = ix.lib.vr_index_search_groups_range(ix._h, _vp(qd), 4, _vp(tb), _vp(fb), 1 << 20, _vp(ld), ctypes.byref(total), 1,
                                             ctypes.c_void_p(_stream_ptr(ix.device)))
    torch.cuda.synchronize()
    assert st == VR_OK and np.array_equal(ld.cpu().numpy(), [0, want[0][1], want[0][1], want[0][1], want[0][1]]) and total.value == want[0][1] > 0
    st, sc, rows, gr = _raw_results(ix, total.value)
    assert st == VR_OK and np.array_equal(gr, want[3][:want[0][1]]) and np.array_equal(rows, want[2][:want[0][1]])
    # ---- and all of this left the other searches alone
    for a, b in zip(before, run_others()):
        assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                   for x, y in zip(a, b))
    st2 = ix.group_range_search_stats()
    assert ix.group_range_search_stats(reset=True) == st2 and ix.group_range_search_stats() == ZERO
    ix.add(C[:10])                                                       # rows appended: grouping, filters and the stored result are gone
    assert ix.n_groups == 0 and _raw(ix, Q, thr)[0] == VR_ERR_STATE and _raw_results(ix, 1)[0] == VR_ERR_STATE
    ix.close()


# ------------------------------------------------------------------------------------------------ against fp64 ---
@pytest.mark.parametrize("name", list(N.TABLE))
def test_membership_and_scores_against_fp64(name):
    """Measured on an MI355X: see the README section "Document range search" for the figures of this test (excused pairs, largest
    score error, band documents and page dots per document returned)."""
    C, Q, off, S = G.case(name)
    ix = _index(C, off)
    t = N.case_thresholds(name, len(Q))
    _, plain, filtered_entries, _ = N.TABLE[name]
    for density, entries in ((None, plain), (0.5, filtered_entries)):
        mask = G.case_mask(name, density)
        if mask is not None:
            ix.set_filters(mask[None, :])
        first = None
        for q_in in (Q, torch.tensor(Q).cuda()):
            ix.group_range_search_stats(reset=True)
            lims, sc, rows, gr = _np(*ix.search_groups_range(q_in, t, None if mask is None else 0, sort=False))
            st = ix.group_range_search_stats()
            ref_entries, excused, err, bad = N.check_range(S, off, mask, t, lims, sc, rows, gr)
            print(f"{name} density {density}: {lims[-1]} entries (reference {ref_entries}), {excused} excused, max |score - fp64| {err:.2e}, "
                  f"{st['documents'] / max(lims[-1], 1):.2f} band documents and {st['page_dots'] / max(lims[-1], 1):.2f} page dots per document returned")
            assert ref_entries == entries
            assert bad is None, bad
            assert err <= N.ATOL
            assert excused <= N.EXCUSED_SHARE * ref_entries
            if first is None:
                first = (lims.tolist(), _u32(sc).tolist(), rows.tolist(), gr.tolist())
            assert (lims.tolist(), _u32(sc).tolist(), rows.tolist(), gr.tolist()) == first       # host and device callers: the same bits
    ix.close()


# ------------------------------------------------------------------------------------------------ host consumers ---
def test_retrieve_documents_range_over_pickle_shards(tmp_path):
    from visrag_amd import retriever
    from visrag_amd.utils import write_shard
    C, Q, bounds = shards_case()                                         # shards of 1 000, 3 001 and 1 999 rows
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
    t = 0.12
    for labelled, m in ((False, None), (True, mask)):
        scores, pages = retriever.retrieve_documents_range(args, t, doc_of, *((label_of_doc, lambda q: wanted[q]) if labelled else ()))
        lims, sc, rows, gr = N.group_range_ref(S32, off, m, t, sort=True)
        assert lims[-1] > 20
        for qi, q in enumerate(qids):
            a, b = lims[qi], lims[qi + 1]
            assert list(scores[q]) == [docs[g] for g in gr[a:b]] == list(pages[q])
            assert np.array_equal(_u32(list(scores[q].values())), _u32(sc[a:b])) and list(pages[q].values()) == [names[r] for r in rows[a:b]]
    top, _ = retriever.retrieve_documents_range(args, t, doc_of, max_per_query=2)
    assert all(list(top[q]) == list(scores_q)[:2] for q, scores_q in retriever.retrieve_documents_range(args, t, doc_of)[0].items())


def test_demo_retrieve_documents_above(tmp_path):
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
    p46, s46 = demo.retrieve_documents(kb, qvec, 46, None, None, index=ix, names=nm, return_scores=True)
    cut = float(np.float32(s46[11]))
    p, s = demo.retrieve_documents_above(kb, qvec, cut, None, None, index=ix, names=nm, return_scores=True)
    assert p == p46[:12] and np.array_equal(_u32(s), _u32(s46[:12]))
    assert demo.retrieve_documents_above(kb, torch.tensor(qvec).cuda(), -4.0, None, None, index=ix, names=nm) == p46
    assert demo.retrieve_documents_above(kb, qvec, 2.0, None, None, index=ix, names=nm) == []
    assert demo.retrieve_documents_above(kb, qvec, -4.0, None, None, index=ix, names=nm, max_documents=5) == p46[:5]
    docs = ["deck_2.pdf", "other_7.pdf", "deck_4.pdf"]
    only, so = demo.retrieve_documents(kb, qvec, 10, None, None, index=ix, names=nm, documents=docs, return_scores=True)
    got, gs = demo.retrieve_documents_above(kb, qvec, -4.0, None, None, index=ix, names=nm, documents=docs, return_scores=True)
    assert got == only and np.array_equal(_u32(gs), _u32(so))
    with pytest.raises(ValueError):
        demo.retrieve_documents_above(kb, qvec, 0.0, None, None, index=ix, names=nm, documents=["nowhere.pdf"])
    ix.close()
    assert demo.retrieve_documents_above(kb, qvec, cut, None, None) == p46[:12]           # an index of its own
