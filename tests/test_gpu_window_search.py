"""-m gpu: the windowed search (vr_index_search_window / vr_index_window_search_stats, csrc/search_window.hip) against the
library's own searches — strict, bit for bit — and against the numpy reference tests/window_search_ref.py.

Strict tests (no tolerance): a window IS entries [o, o + k) of every segment of `search_range(threshold = -4, sort=True)`, of
`search(o + k)` and of `search_filtered(o + k)`, ids and score bits, with tails (-inf, -1) past the allowed rows; `rank_rows` of
the ids returned is o + arange(k); windows inside a tier of bit-identical rows come in id order; pages of 1 000 concatenated are
the whole ranking, every row once; an edited index answers as a freshly built one; host arrays and CUDA tensors give the same.

Against fp64 (no excuse mechanism, the interval is the whole test): scores within the project's ATOL = 1e-5; a row of fp64 score
s returned at position j of the window at offset o has o + j in [#(S > s + 6e-7), #(S >= s - 6e-7) - 1] — the rank search's
interval bar, on the same grounds.  Windows of k = 100; the reference alone gives these intervals for the rows of its own windows
(tests/test_cpu_window_search_ref.py pins them, so this test cannot grow loose unnoticed):

    case                  offset   entries   widened intervals   max width
    (5000, 37, 256)            0     3 700            9              1
    (5000, 37, 256)         2500     3 700          112              1
    (3001, 300, 128)           0    30 000           50              1
    (3001, 300, 128)        2500    30 000          290              1
    (20000, 64, 2304)      10000     6 400        2 389              4
    families, dim 64           0       800           39              2
    families, dim 64        1450       800            4              1
    families, dim 2304         0       800           97              2
    families, dim 2304      1450       800           52              2

The widest interval at (20000, 64, 2304), offset 10 000 is 4: wider than the rank test's 3.  The middle of 20 000 scores of spread
0.02 holds five rows inside 1.2e-6 of each other; the bar is the issue's and stays as it is.

Measured on an MI355X (the same for host arrays and CUDA tensors): every position inside its interval; 24 of the 77 000 positions
differ from the reference's own fp64 ranking (0 / 0 / 2 / 4 / 8 / 2 / 0 / 6 / 2 in the table's order, all inside near-ties);
largest |score - fp64| 2.8e-8 / 1.9e-8 / 5.3e-8 / 3.0e-8 / 8.3e-9 / 1.3e-7 / 1.0e-7 / 8.9e-8 / 8.7e-8.  Band candidates re-scored
per row returned: 1.4 / 5.6 / 1.2 / 2.2 / 56.9 / 11.4 / 9.2 / 15.0 / 16.1 — at (20000, 64, 2304) the band of 4 eps plus the
window's own span holds 5 690 of the 20 000 rows per query; at (2000, 8, 2304) 2.0 at offset 0 and 6.5 at offset 1 000.
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
from tests import range_search_ref as X  # noqa: E402
from tests import rank_search_ref as K  # noqa: E402
from tests import window_search_ref as W  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.engine import HipIndex, _stream_ptr  # noqa: E402

ATOL = 1e-5
VR_OK, VR_ERR_INVALID, VR_ERR_STATE = 0, 1, 3
CYCLE_C = (0.05, 0.07)


def _index(C, masks=None):
    ix = HipIndex(C.shape[1], len(C))
    ix.add(C[: len(C) // 2]); ix.add(C[len(C) // 2:])
    if masks is not None:
        ix.set_filters(masks)
    return ix


def _np(*xs):
    return [x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in xs]


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _padded_ranking(ix, Q, pad, foq=None):
    """-> (scores f32 [nq][n + pad], ids i64 [nq][n + pad]): every query's segment of the range search — every allowed row, score
    descending then id ascending — followed by tails (-inf, -1)"""
    n = len(ix)
    lims, sc, ids = ix.search_range(Q, -4.0, foq, sort=True)
    S = np.full((len(Q), n + pad), -np.inf, dtype=np.float32)
    I = np.full((len(Q), n + pad), -1, dtype=np.int64)
    for q in range(len(Q)):
        m = lims[q + 1] - lims[q]
        S[q, :m], I[q, :m] = sc[lims[q]:lims[q + 1]], ids[lims[q]:lims[q + 1]]
    return S, I


def _slices(S, I, off, k):
    """entries [off[q], off[q] + k) of every row of the padded ranking (off: an int or one per query)"""
    off = np.broadcast_to(np.asarray(off, dtype=np.int64), (len(S),))
    cols = np.minimum(off[:, None] + np.arange(k)[None, :], S.shape[1] - 1)      # (past the padding: a tail like any other)
    return np.take_along_axis(S, cols, 1), np.take_along_axis(I, cols, 1)


def _same(got, want_s, want_i):
    sc, ids = _np(*got)
    assert sc.dtype == np.float32 and ids.dtype == np.int64 and sc.shape == ids.shape == want_i.shape
    assert np.array_equal(ids, want_i)
    assert np.array_equal(_u32(sc), _u32(want_s))


# ------------------------------------------------------------------------------------------ 1. the whole ranking ---
@pytest.mark.parametrize("nd,nq,dim", [(5000, 37, 256), (2000, 8, 2304)])
def test_windows_are_slices_of_the_range_searchs_ranking(nd, nq, dim):
    C, Q = R.unit(nd, dim, 1), R.unit(nq, dim, 2)
    ix = _index(C)
    S, I = _padded_ranking(ix, Q, 1010)
    assert (I[:, :nd] >= 0).all()
    qd = torch.tensor(Q).cuda()
    for k in (1, 10, 100, 1000):
        offsets = [0, 1, 7, 990, 1000, nd // 2, nd - k, nd - 3, nd, nd + 5]
        mixed = np.asarray(offsets, dtype=np.int64)[(np.arange(nq) * 3 + 1) % len(offsets)]
        for o in offsets + [mixed]:
            want_s, want_i = _slices(S, I, o, k)
            for cuda in (False, True):
                ix.window_search_stats(reset=True)
                got = ix.search_window(qd if cuda else Q, torch.tensor(o) if cuda and not np.isscalar(o) else o, k)
                assert all((isinstance(x, torch.Tensor) and x.is_cuda) if cuda else isinstance(x, np.ndarray) for x in got)
                _same(got, want_s, want_i)
                st = ix.window_search_stats()
                assert st["queries"] == nq and st["candidates"] >= int((want_i >= 0).sum())
                assert st["ahead"] <= int(np.broadcast_to(o, (nq,)).sum())
    for o in (0, nd // 2):
        ix.window_search_stats(reset=True)
        ix.search_window(Q, o, 100)
        st = ix.window_search_stats()
        print(f"whole ranking {nd}x{nq}x{dim} offset {o} k 100: {st}, {st['candidates'] / (nq * 100):.1f} band candidates per row returned")
    ix.close()


# --------------------------------------------------------------------------------------- 2. agreement with top-k ---
@pytest.fixture(scope="module")
def big():
    C, Q, _, _ = X.random_case(20000, 64, 2304, CYCLE_C)
    ix = _index(C)
    yield ix, Q
    ix.close()


def test_a_window_is_the_tail_of_search(big):
    ix, Q = big
    for o, k in ((0, 10), (5, 21), (90, 10), (0, 1000), (900, 100)):
        s, i = ix.search(Q, o + k)
        for q_in in (Q, torch.tensor(Q).cuda()):
            _same(ix.search_window(q_in, o, k), s[:, o:], i[:, o:])
    for eps in (-1.0, 0.01, float("nan")):                               # certification off / a caller's model / the default again
        ix.set_search_eps(eps)
        s, i = ix.search(Q, 26)
        _same(ix.search_window(Q, 5, 21), s[:, 5:], i[:, 5:])


def test_rank_rows_is_the_inverse(big):
    ix, Q = big
    k = 10
    for o in (0, 3000, 19990):
        for q_in in (Q, torch.tensor(Q).cuda()):
            sc, ids = ix.search_window(q_in, o, k)
            rs, rk = _np(*ix.rank_rows(q_in, ids))
            assert np.array_equal(rk, np.tile(o + np.arange(k), (len(Q), 1))), o
            assert np.array_equal(_u32(rs), _u32(_np(sc)[0])), o
    sc, ids = ix.search_window(Q, 19995, k)                              # the ranking ends inside the window
    assert (ids[:, :5] >= 0).all() and (ids[:, 5:] == -1).all() and np.isneginf(sc[:, 5:]).all()


# ---------------------------------------------------------------------------------- 3. agreement under a filter ---
def test_windows_under_filters():
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    M = np.concatenate([F.random_filters(len(C), (0.5, 0.01), seed=11), np.zeros((1, len(C)), dtype=bool)])
    foq = (np.arange(len(Q)) % 4 - 1).astype(np.int64)                   # -1 (no filter), 0, 1, 2 (allows nothing), ...
    allowed = np.asarray([len(C) if f < 0 else int(M[f].sum()) for f in foq])
    ix = HipIndex(256, len(C))
    ix.add(C)
    with pytest.raises(_lib.VisragHipError):                             # no filters set: VR_ERR_STATE
        ix.search_window(Q, 0, 10, filter_of_query=np.zeros(len(Q), dtype=np.int64))
    ix.set_filters(M)
    S, I = _padded_ranking(ix, Q, 1100, foq)
    assert np.array_equal((I >= 0).sum(1), allowed) and 30 < allowed[2] < 100
    qd, fd = torch.tensor(Q).cuda(), torch.tensor(foq).cuda()
    for k in (10, 100):
        s, i = ix.search_filtered(Q, k, foq)
        for o in (0, 20, int(allowed[2]) - 7, int(allowed[2]), int(allowed[1]) - 3, int(allowed[1]), 4990, 5000):
            want_s, want_i = _slices(S, I, o, k)
            _same(ix.search_window(Q, o, k, foq), want_s, want_i)
            _same(ix.search_window(qd, o, k, fd), want_s, want_i)
            if o == 0:
                _same(ix.search_window(Q, o, k, foq), s, i)
        # a partial tail inside the last k allowed rows, all tails at or past the allowed rows, nothing at all for filter 2
        part = _np(*ix.search_window(Q, int(allowed[2]) - 7, k, foq))[1]
        assert ((part[2] >= 0).sum() == 7) and (part[3] == -1).all()
        assert (_np(*ix.search_window(Q, int(allowed[2]), k, foq))[1][2] == -1).all()
    # per-query offsets: every query's own last three allowed rows
    o = np.maximum(allowed - 3, 0)
    want_s, want_i = _slices(S, I, o, 10)
    _same(ix.search_window(Q, o, 10, foq), want_s, want_i)
    assert np.array_equal((want_i >= 0).sum(1), np.minimum(allowed, 3))
    # one filter for every query, and -1 / None = no filter
    s, i = ix.search_filtered(Q, 30, 0)
    _same(ix.search_window(Q, 10, 20, 0), s[:, 10:], i[:, 10:])
    plain = ix.search_window(Q, 10, 20)
    _same(ix.search_window(Q, 10, 20, -1), *plain)
    _same(plain, *(x[:, 10:] for x in ix.search(Q, 30)))
    ix.close()


def test_two_query_blocks_under_filters():
    """600 rows (three 256-row tiles, the last partial), 257 queries (a second block of one query), a half-density and an empty
    filter, per-query offsets: the block's offsets, filters and outputs start at its first query.  Against the fp64 reference
    (the interval bar of the module docstring) and, bit for bit, the range search's ranking; query 256 is on filter 0."""
    C, Q = R.unit(600, 64, 1), R.unit(257, 64, 2)
    M = np.concatenate([F.random_filters(600, (0.5,), seed=11), np.zeros((1, 600), dtype=bool)])
    foq = (np.arange(257) % 3 - 1).astype(np.int64)                      # -1 (no filter), 0, 1 (allows nothing), ...
    off = (np.arange(257) * 7 % 40).astype(np.int64)
    assert foq[256] == 0 and off[256] > 0
    k, S64 = 5, R.scores64(Q, C)
    ix = _index(C, M)
    want_s, want_i = _slices(*_padded_ranking(ix, Q, 50, foq), off, k)
    assert (want_i[foq == 1] == -1).all() and (want_i[foq != 1] >= 0).all()
    for q_in, f_in in ((Q, foq), (torch.tensor(Q).cuda(), torch.tensor(foq).cuda())):
        got = ix.search_window(q_in, off, k, f_in)
        _same(got, want_s, want_i)
        sc, ids = _np(*got)
        for q in np.flatnonzero(foq != 1):
            rows = np.arange(600) if foq[q] < 0 else np.flatnonzero(M[foq[q]])
            pos = {int(r): j for j, r in enumerate(rows)}
            n_q, _, bad = W.check_window(S64[q][rows], np.asarray([pos[int(i)] for i in ids[q]]), int(off[q]))
            assert n_q == k and bad is None, (q, bad)
            np.testing.assert_allclose(sc[q], S64[q][ids[q]], atol=ATOL, rtol=0)
    ix.close()


# ------------------------------------------------------------------------------------------------ 4. tie tier ---
def test_tie_tier():
    C, Q, _ = R.tie_tier()
    n, high = len(C), 7 * np.arange(100) + 3
    tied = np.setdiff1d(np.arange(n), high)
    ix = _index(C)
    S, I = _padded_ranking(ix, Q, 1000)
    assert np.isin(I[:, :100], high).all() and np.array_equal(I[:, 100:n], np.tile(tied, (3, 1)))     # ranks 100 .. 2999: one tier
    for o, k in ((50, 100), (1500, 1000), (2950, 100), (100, 1), (99, 2), (2999, 1)):
        want_s, want_i = _slices(S, I, o, k)
        for q_in in (Q, torch.tensor(Q).cuda()):
            _same(ix.search_window(q_in, o, k), want_s, want_i)
    ids = ix.search_window(Q, 1500, 1000)[1]
    assert np.array_equal(ids, np.tile(tied[1400:2400], (3, 1)))         # both edges inside the tier: consecutive ids, in id order
    assert (ix.search_window(Q, 2950, 100)[1][:, 50:] == -1).all()
    ix.close()


# -------------------------------------------------------------------------------------------------- 5. paging ---
def test_pages_concatenated_are_the_whole_ranking():
    C, Q = R.unit(3001, 128, 1), R.unit(16, 128, 2)
    ix = _index(C)
    S, I = _padded_ranking(ix, Q, 1999)
    for q_in in (Q, torch.tensor(Q).cuda()):
        pages = [_np(*ix.search_window(q_in, o, 1000)) for o in range(0, 5000, 1000)]
        sc, ids = np.concatenate([p[0] for p in pages], 1), np.concatenate([p[1] for p in pages], 1)
        assert np.array_equal(ids, I) and np.array_equal(_u32(sc), _u32(S))
        assert np.array_equal(np.sort(ids[:, :3001], axis=1), np.tile(np.arange(3001), (16, 1)))      # every row exactly once
        assert (ids[:, 3001:] == -1).all() and np.isneginf(sc[:, 3001:]).all()
    ix.close()


# --------------------------------------------------------------------------------------------------- 6. edits ---
def test_an_edited_index_answers_as_a_fresh_one():
    C, Q = R.unit(3001, 128, 1).copy(), R.unit(40, 128, 2)
    rng = np.random.default_rng(17)
    gone = rng.choice(len(C), int(0.3 * len(C)), replace=False)
    ix = _index(C)
    ix.search_window(Q, 100, 10)                                         # (nothing is stored: nothing to invalidate)
    new_id = ix.remove(gone)
    left = C[new_id >= 0]
    upd = rng.choice(len(left), 5, replace=False)
    fresh_rows = R.unit(5, 128, 33)
    ix.update(upd, fresh_rows)
    left[upd] = fresh_rows
    fresh = _index(left)
    n = len(left)
    for o in (0, 500, n // 2, n - 50):
        a, b = ix.search_window(Q, o, 100), fresh.search_window(Q, o, 100)
        _same(a, *b)
    S, I = _padded_ranking(fresh, Q, 100)
    _same(ix.search_window(Q, n // 2, 100), *_slices(S, I, n // 2, 100))
    ix.close(); fresh.close()


# ------------------------------------------------------------------------------------ 7. arguments, the raw ABI ---
def _vp(x):
    if x is None:
        return ctypes.c_void_p(None)
    return ctypes.c_void_p(x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data)


def _raw(ix, Q, offsets, k, foq=None, nq=None):
    """vr_index_search_window itself, host arrays -> (status, scores, ids); the outputs start as -7"""
    offsets = np.asarray(offsets, dtype=np.int64)
    n = max(len(Q) * max(k, 1), 1)
    sc, ids = np.full(n, -7, dtype=np.float32), np.full(n, -7, dtype=np.int64)
    st = ix.lib.vr_index_search_window(ix._h, _vp(Q), len(Q) if nq is None else nq, _vp(offsets), k, _vp(foq), _vp(sc), _vp(ids), 0,
                                       ctypes.c_void_p(_stream_ptr(ix.device)))
    return st, sc, ids


def test_argument_checks_come_before_any_launch():
    n = 600
    C, Q = R.unit(n, 64, 1), R.unit(4, 64, 2)
    M = F.random_filters(n, (0.5, 0.1), seed=11)
    foq = np.array([0, 1, -1, 1], dtype=np.int32)
    ix = HipIndex(64, n + 10)
    # the empty index: tails, nothing is launched, nothing counted
    st, sc, ids = _raw(ix, Q, [0, 1, 2, 3], 5)
    assert st == VR_OK and (ids == -1).all() and np.isneginf(sc).all()
    qd, out_s, out_i = torch.tensor(Q).cuda(), torch.full((20,), -7.0).cuda(), torch.full((20,), -7, dtype=torch.int64).cuda()
    st = ix.lib.vr_index_search_window(ix._h, _vp(qd), 4, _vp(np.zeros(4, dtype=np.int64)), 5, _vp(None), _vp(out_s), _vp(out_i), 1,
                                       ctypes.c_void_p(_stream_ptr(ix.device)))
    torch.cuda.synchronize()
    assert st == VR_OK and (out_i.cpu().numpy() == -1).all() and np.isneginf(out_s.cpu().numpy()).all()
    assert ix.window_search_stats() == {"queries": 0, "candidates": 0, "ahead": 0}
    ix.add(C)
    ix.set_filters(M)
    off = [0, 3, 590, 700]
    st, sc, ids = _raw(ix, Q, off, 20, foq)
    assert st == VR_OK
    S = R.scores64(Q, C)
    for q in range(4):
        want = W.window_ref(S[q], off[q], 20, None if foq[q] < 0 else M[foq[q]])[1]
        assert np.array_equal(ids.reshape(4, 20)[q], want), q
    live = ids >= 0
    np.testing.assert_allclose(sc[live], S[np.repeat(np.arange(4), 20)[live], ids[live]], atol=ATOL, rtol=0)
    stats = ix.window_search_stats()
    assert stats["queries"] == 4
    others = (ix.search_stats(), ix.filter_search_stats(), ix.range_search_stats(), ix.rank_search_stats())

    def nothing_ran(st, *outs):
        return st == VR_ERR_INVALID and all((o == -7).all() for o in outs) and ix.window_search_stats() == stats

    for k in (0, -1, 1001):
        assert nothing_ran(*_raw(ix, Q, off, k, foq)), k
    assert "k=1001 unsupported (1..1000)" in _lib.load().vr_last_error().decode()
    for bad in (-1, -(1 << 40)):                                         # a negative offset
        assert nothing_ran(*_raw(ix, Q, [0, 3, bad, 7], 20, foq)), bad
    assert "offsets[2]" in _lib.load().vr_last_error().decode()
    for bad in (2, -2):                                                  # a filter index out of range
        fb = np.array([0, bad, -1, 1], dtype=np.int32)
        assert nothing_ran(*_raw(ix, Q, off, 20, fb))
        with pytest.raises(ValueError):
            ix.search_window(Q, 0, 20, filter_of_query=fb)
    assert "outside [-1, 2)" in _lib.load().vr_last_error().decode()
    assert ix.lib.vr_index_search_window(ix._h, _vp(Q), 4, _vp(None), 5, _vp(None), _vp(None), _vp(None), 0, None) == VR_ERR_INVALID
    assert nothing_ran(*_raw(ix, Q, off, 20, foq, nq=-1))
    st, sc, ids = _raw(ix, Q, off, 20, foq, nq=0)                        # no query: VR_OK, nothing launched, nothing written
    assert st == VR_OK and (ids == -7).all() and (sc == -7).all() and ix.window_search_stats() == stats
    # a dim the fp32 re-scoring does not take cannot reach the call: no index of such a dim can be created
    h = ctypes.c_void_p()
    assert ix.lib.vr_index_create(ix.device, 2624, 16, ctypes.byref(h)) == VR_ERR_INVALID
    for bad_off in ([1, 2, 3], -1, [0, -5, 0, 0]):                       # the binding's own checks
        with pytest.raises(ValueError):
            ix.search_window(Q, bad_off, 5)
    with pytest.raises(_lib.VisragHipError):
        ix.search_window(Q, 0, 1001)
    # on the device an out-of-range filter index cannot be seen before the launch: that query gets a row of tails
    fb = torch.tensor(np.array([0, 7, -1, 1], dtype=np.int32)).cuda()
    out_s, out_i = torch.full((4, 5), -7.0).cuda(), torch.full((4, 5), -7, dtype=torch.int64).cuda()
    st = ix.lib.vr_index_search_window(ix._h, _vp(qd), 4, _vp(np.zeros(4, dtype=np.int64)), 5, _vp(fb), _vp(out_s), _vp(out_i), 1,
                                       ctypes.c_void_p(_stream_ptr(ix.device)))
    torch.cuda.synchronize()
    want = _np(*ix.search_window(Q, 0, 5, np.array([0, 0, -1, 1])))
    want[0][1], want[1][1] = -np.inf, -1
    assert st == VR_OK and np.array_equal(out_i.cpu().numpy(), want[1]) and np.array_equal(_u32(out_s.cpu().numpy()), _u32(want[0]))
    assert (ix.search_stats(), ix.filter_search_stats(), ix.range_search_stats(), ix.rank_search_stats()) == others
    st2 = ix.window_search_stats()
    assert ix.window_search_stats(reset=True) == st2 and ix.window_search_stats() == {"queries": 0, "candidates": 0, "ahead": 0}
    # a filter index while no filters are set for the rows present
    ix.add(C[:10])
    assert ix.n_filters == 0
    assert _raw(ix, Q, off, 20, foq)[0] == VR_ERR_STATE and _raw(ix, Q, off, 20)[0] == VR_OK
    ix.close()


# ------------------------------------------------------------------------------------------------ against fp64 ---
@pytest.mark.parametrize("name", list(W.TABLE))
def test_windows_and_scores_against_fp64(name):
    C, Q, S = W.case(name)
    ix = _index(C)
    k = W.K_FP64
    for o in W.TABLE[name]:
        first = None
        for q_in in (Q, torch.tensor(Q).cuda()):
            ix.window_search_stats(reset=True)
            sc, ids = _np(*ix.search_window(q_in, o, k))
            st = ix.window_search_stats()
            entries = moved = 0
            worst, err = None, 0.0
            for q in range(len(Q)):
                n_q, moved_q, bad = W.check_window(S[q], ids[q], o)
                entries += n_q; moved += moved_q
                worst = worst or (bad and (q,) + bad)
                err = max(err, float(np.abs(sc[q][ids[q] >= 0] - S[q][ids[q][ids[q] >= 0]]).max()))
            print(f"{name} offset {o}: {entries} entries, {moved} positions differ from the fp64 ranking, max |score - fp64| {err:.2e}, "
                  f"{st['candidates'] / max(entries, 1):.1f} band candidates per row returned, {st['ahead']} rows certainly ahead")
            assert entries == W.TABLE[name][o][0]
            assert err <= ATOL
            assert worst is None, worst                                  # (query, position, row, lo, hi)
            if first is None:
                first = (_u32(sc).tolist(), ids.tolist())
            assert (_u32(sc).tolist(), ids.tolist()) == first            # host and device callers: the same bits
    ix.close()


# ------------------------------------------------------------------------------------------------ host consumers ---
def test_retrieve_deep_and_mine_negatives_over_pickle_shards(tmp_path):
    from visrag_amd import retriever
    from visrag_amd.utils import write_shard
    C, Q, bounds = K.shards_case()
    names = [f"page_{i}" for i in range(len(C))]
    for s in range(3):
        write_shard(str(tmp_path / f"embeddings.corpus.rank.{s}"), C[bounds[s]:bounds[s + 1]], names[bounds[s]:bounds[s + 1]])
    qids = [f"q{q}" for q in range(len(Q))]
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, qids)
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    whole = _index(C)
    S, I = _padded_ranking(whole, Q, 0)
    whole.close()
    run = retriever.retrieve_deep(args, 2500)
    for qi, q in enumerate(qids):
        assert list(run[q]) == [names[i] for i in I[qi, :2500]]
        assert np.array_equal(_u32(list(run[q].values())), _u32(S[qi, :2500]))
    assert retriever.retrieve_deep(args, 10) == retriever.distributed_parallel_retrieve(args, 10, global_topk=True)
    positives = {q: [names[i] for i in I[qi, [0, 31, 35]]] for qi, q in enumerate(qids)}
    neg = retriever.mine_negatives(args, positives, 30, 50)
    for qi, q in enumerate(qids):
        assert neg[q] == [names[i] for i in I[qi, 30:83] if names[i] not in positives[q]][:50] and len(neg[q]) == 50


def test_demo_retrieve_offset(tmp_path):
    from visrag_amd import demo
    D, _ = R.decks(6, 5, 64, 0.05)
    C = np.concatenate([D, R.unit(40, 64, 9)])
    names = [f"deck_{d}.pdf_{i}.png" for d in range(6) for i in range(5)] + [f"other_{j}.pdf_0.png" for j in range(40)]
    qvec = R.unit(6, 64, 5)[2:3]
    kb = str(tmp_path / "kb")
    os.makedirs(kb)
    np.save(os.path.join(kb, "reps.npy"), C)
    with open(os.path.join(kb, "index2img_filename.txt"), "w") as f:
        f.write("\n".join(names))
    ix, nm = demo.load_knowledge_base(kb, 0)
    every = [n.rsplit("_", 1)[0] for n in names]                         # (an embedding as the query: the filtered path takes it)
    p20, s20 = demo.retrieve(kb, qvec, 20, None, None, index=ix, names=nm, return_scores=True, documents=every)
    for docs in (None, every):
        p, s = demo.retrieve(kb, qvec, 10, None, None, index=ix, names=nm, return_scores=True, documents=docs, offset=10)
        assert p == p20[10:] and np.array_equal(_u32(s), _u32(s20[10:]))
    p70 = demo.retrieve(kb, qvec, 70, None, None, index=ix, names=nm, documents=every)
    assert demo.retrieve(kb, qvec, 10, None, None, index=ix, names=nm, offset=65) == p70[65:] and len(p70) == 70     # the ranking ends
    assert demo.retrieve(kb, qvec, 10, None, None, index=ix, names=nm, offset=70) == []
    docs = ["deck_2.pdf", "other_7.pdf"]
    only = demo.retrieve(kb, qvec, 6, None, None, index=ix, names=nm, documents=docs)
    assert demo.retrieve(kb, qvec, 3, None, None, index=ix, names=nm, documents=docs, offset=2) == only[2:5]
    assert demo.retrieve(kb, qvec, 10, None, None, index=ix, names=nm, documents=docs, offset=4) == only[4:]
    with pytest.raises(ValueError):
        demo.retrieve(kb, qvec, 10, None, None, index=ix, names=nm, diverse=0.5, offset=10)
    with pytest.raises(ValueError):
        demo.retrieve(kb, qvec, 10, None, None, index=ix, names=nm, offset=-1)
    ix.close()
