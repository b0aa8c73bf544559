"""-m gpu: the range search (vr_index_search_range / vr_index_range_results, csrc/search_range.hip) against the numpy reference
tests/range_search_ref.py.

Bars (those of tests/test_gpu_filter_search.py and tests/test_gpu_group_search.py, no new tolerance): scores within 1e-5 of the
fp64 reference; membership identical to the reference's, except for a (query, row) pair whose fp64 score lies within 3e-7 of the
threshold, which is fp32 summation order.  At most 0.5 % of a case's returned rows may use that excuse.  The reference alone, rows
R.unit(nd, dim, 1), queries R.unit(nq, dim, 2), thresholds cycling per query (tests/test_cpu_range_search_ref.py pins the counts):

    case (nd, nq, dim), thresholds                      rows returned (per query min / median / max)   within 3e-7 of t
    (5000, 37, 256), 0.10 / 0.15 / 0.20 / 0.30          3 167 (0 / 25 / 297)                           0
    (3001, 300, 128), 0.15 / 0.25 / 0.05                100 869 (1 / 135 / 945)                        0
    (20000, 64, 2304), 0.05 / 0.07                      5 400 (3 / 80 / 184)                           0
    families, dim 64, t = 0.9                           12 000 (1 500 each)                            0
    families, dim 64, t = 0.97579408 (median own)       6 000 (349 / 864 / 1 136)                      0
    families, dim 2304, t = 0.9                         12 000 (1 500 each)                            0
    families, dim 2304, t = 0.96454531 (median own)     6 000 (332 / 733 / 1 355)                      3 (0.05 %)
    norms U[0.5, 3], (4000, 20, 256), t = 0.2 / 0.4     3 885 (164-230) / 181 (4-17)                   0

so the reference alone stays a factor ten inside the cap everywhere.  A family of 1 500 rows is beyond what `search` can return;
at the median threshold nearly the whole family lies inside the error band, so the fp32 re-scoring alone decides.

Measured on an MI355X (excused pairs / rows returned; the same for host arrays and CUDA tensors, sorted or not): families, dim
2304, median threshold 1 / 6 001 (0.017 %: one of the reference's three pairs within 3e-7 of t); every other case, the filtered
one included, 0.  Candidates re-scored per row returned: 1.00 (families, t = 0.9) to 2.0 (families, dim 2304, median), 1.06-1.63
on the random cases.  The t = 0.9 family cases, the agreement with `search`, the tie tier and everything / nothing are strict."""
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
from visrag_amd import _lib  # noqa: E402
from visrag_amd.documents import doc_of_page, split_ranges  # noqa: E402
from visrag_amd.engine import HipIndex, _stream_ptr  # noqa: E402

ATOL, NEAR_TIE, EXCUSED = 1e-5, 3e-7, 0.005
VR_OK, VR_ERR_INVALID, VR_ERR_STATE, VR_ERR_CAPACITY = 0, 1, 3, 4
CYCLE_A, CYCLE_B, CYCLE_C = (0.10, 0.15, 0.20, 0.30), (0.15, 0.25, 0.05), (0.05, 0.07)


def _index(C, masks=None):
    ix = HipIndex(C.shape[1], len(C))
    ix.add(C[: len(C) // 2]); ix.add(C[len(C) // 2:])
    if masks is not None:
        ix.set_filters(masks)
    return ix


def _np(*xs):
    return [x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in xs]


def _bits(got):
    lims, sc, ids = _np(*got)
    return lims.tolist(), sc.view(np.uint32).tolist(), ids.tolist()


def _check(got, S, t, masks=None, foq=None, strict=False, ranked=False):
    """`got` = (lims, scores, ids) against the fp64 scores S under the bars of the module docstring -> excused pairs.
    ranked: every segment in ranking order (score descending, then id ascending), else in ascending id."""
    lims, sc, ids = _np(*got)
    nq, n = S.shape
    assert lims.dtype == np.int64 and sc.dtype == np.float32 and ids.dtype == np.int64
    assert lims.shape == (nq + 1,) and lims[0] == 0 and (np.diff(lims) >= 0).all() and lims[-1] == len(sc) == len(ids)
    assert ((ids >= 0) & (ids < n)).all()
    want = X.membership(S, t, masks, foq)
    have = np.zeros_like(want)
    t32 = X.thresholds_of(t, nq)
    for q, (s, i) in enumerate(split_ranges(lims, sc, ids)):
        if ranked:
            ds, di = np.diff(s.astype(np.float64)), np.diff(i)
            assert ((ds < 0) | ((ds == 0) & (di > 0))).all(), q
            assert len(set(i.tolist())) == len(i), q
        else:
            assert (np.diff(i) > 0).all(), q
        assert (s >= t32[q]).all(), q                                     # the library's own fp32 compare
        np.testing.assert_allclose(s, S[q, i], atol=ATOL, rtol=0)
        have[q, i] = True
        if foq is not None and foq[q] >= 0:
            assert np.asarray(masks)[foq[q]][i].all(), q
    bad = np.argwhere(have != want)
    if strict:
        assert len(bad) == 0, bad[:5]
    for q, i in bad:
        assert abs(S[q, i] - float(t32[q])) < NEAR_TIE, (q, i, S[q, i], t32[q])
    assert len(bad) <= EXCUSED * max(int(lims[-1]), 1), (len(bad), int(lims[-1]))
    return len(bad)


def _four_ways(ix, Q, S, t, name, strict=False, masks=None, foq=None):
    """host arrays and CUDA tensors, sort=False and sort=True; statistics of every call"""
    nq = len(Q)
    first = None
    for cuda in (False, True):
        q_in = torch.tensor(Q).cuda() if cuda else Q
        for sort in (False, True):
            ix.range_search_stats(reset=True)
            got = ix.search_range(q_in, t, foq, sort=sort)
            assert all((isinstance(x, torch.Tensor) and x.is_cuda) if cuda else isinstance(x, np.ndarray) for x in got)
            excused = _check(got, S, t, masks, foq, strict=strict, ranked=sort)
            print(f"{name} cuda={cuda} sort={sort}: {int(_np(got[0])[0][-1])} rows, {excused} excused")
            st = ix.range_search_stats()
            assert st["queries"] == nq and st["returned"] == int(_np(got[0])[0][-1]) and st["candidates"] >= st["returned"], st
            if sort:
                assert _bits(got) == _bits(X.sort_ranges(*_np(*unsorted)))     # the same entries, reordered
            else:
                unsorted = got
            if first is None:
                first = _bits(got)
        assert _bits(unsorted) == first                                  # host and device callers: the same bits
    print(f"{name}: band {ix.range_search_stats()}")


# ------------------------------------------------------------------------------------------ 1. the table's cases ---
@pytest.mark.parametrize("nd,nq,dim,cycle", [(5000, 37, 256, CYCLE_A), (3001, 300, 128, CYCLE_B), (20000, 64, 2304, CYCLE_C)])
def test_random_unit_rows(nd, nq, dim, cycle):
    C, Q, t, S = X.random_case(nd, nq, dim, cycle)
    ix = _index(C)
    _four_ways(ix, Q, S, t, f"unit-{nd}x{nq}x{dim}")
    ix.close()


@pytest.mark.parametrize("dim", [64, 2304])
def test_families_larger_than_any_k(dim):
    C, Q, S = X.families(dim)
    ix = _index(C)
    _four_ways(ix, Q, S, 0.9, f"families-{dim}-0.9", strict=True)
    lims = ix.search_range(Q, 0.9)[0]
    assert np.diff(lims).tolist() == [1500] * 8                         # the whole family, beyond search's k <= 1000
    _four_ways(ix, Q, S, X.FAMILY_MEDIAN[dim], f"families-{dim}-median")
    ix.close()


def test_rows_of_norms_other_than_one():
    C, Q, S = X.scaled_norms()
    ix = _index(C)
    assert ix.error_model()["max_row_norm"] > 2.9
    for t in (0.2, 0.4):
        _four_ways(ix, Q, S, t, f"norms-{t}")
    ix.close()


# ----------------------------------------------------------------------------------- 2. agreement with search ---
def test_agrees_with_search_bit_for_bit():
    """thresholds = search's own 30th score: the range result is search's first 30 rows as a set, with the same score bits.  In
    fp64 the rank 30 / 31 gap is >= 7.8e-6 and rank 50 lies >= 5.5e-3 below rank 30: nothing to excuse."""
    C, Q, _, S = X.random_case(5000, 37, 256, CYCLE_A)
    o = -np.sort(-S, axis=1)
    assert (o[:, 29] - o[:, 30]).min() >= 7.8e-6 and (o[:, 29] - o[:, 49]).min() >= 5.5e-3
    ix = _index(C)
    s, i = ix.search(Q, 50)
    for q_in in (Q, torch.tensor(Q).cuda()):
        lims, sc, ids = _np(*ix.search_range(q_in, s[:, 29]))
        assert np.diff(lims).tolist() == [30] * len(Q)
        assert np.array_equal(ids.reshape(-1, 30), i[:, :30])            # sort=True: search's own order
        assert np.array_equal(sc.reshape(-1, 30).view(np.uint32), s[:, :30].view(np.uint32))
        lims, sc, ids = _np(*ix.search_range(q_in, s[:, 29], sort=False))
        for q, (sq, iq) in enumerate(split_ranges(lims, sc, ids)):
            order = np.argsort(i[q, :30])
            assert np.array_equal(iq, i[q, :30][order]) and np.array_equal(sq.view(np.uint32), s[q, :30][order].view(np.uint32))
    ix.close()


# ------------------------------------------------------------------------------------------------ 3. tie tier ---
def test_tie_tier():
    """R.tie_tier: 2 900 bit-identical rows and 100 rows clearly above them.  A threshold equal to the library's own score of a
    tied row returns all 3 000 rows; the next float above it exactly the 100 high rows.  Strict."""
    C, Q, _ = R.tie_tier()
    n, high = len(C), 7 * np.arange(100) + 3
    ix = _index(C)
    s, i = ix.search(Q, 150)
    assert not np.isin(i[:, 100], high).any()
    t = s[:, 100].copy()
    for q_in in (Q, torch.tensor(Q).cuda()):
        lims, sc, ids = _np(*ix.search_range(q_in, t, sort=False))
        assert lims.tolist() == [0, n, 2 * n, 3 * n] and np.array_equal(ids, np.tile(np.arange(n), 3))
        lims, sc, ids = _np(*ix.search_range(q_in, np.nextafter(t, np.float32(2)), sort=False))
        assert lims.tolist() == [0, 100, 200, 300] and np.array_equal(ids, np.tile(high, 3))
        lims, sc, ids = _np(*ix.search_range(q_in, np.nextafter(t, np.float32(2))))
        assert np.array_equal(ids.reshape(3, 100), i[:, :100])
    ix.close()


# ----------------------------------------------------------------------------------- 4. everything and nothing ---
def test_everything_and_nothing():
    n, dim = 1001, 64
    C, Q = R.unit(n, dim, 1), R.unit(3, dim, 2)
    ix = _index(C)
    s, i = ix.search(Q, 1000)
    for q_in in (Q, torch.tensor(Q).cuda()):
        lims, sc, ids = _np(*ix.search_range(q_in, -2.0, sort=False))
        assert lims.tolist() == [0, n, 2 * n, 3 * n] and np.array_equal(ids, np.tile(np.arange(n), 3))
        for q in range(3):                                               # search's 1000 rows carry the same bits here
            assert np.array_equal(sc[q * n:(q + 1) * n][i[q]].view(np.uint32), s[q].view(np.uint32))
        everything = sc.reshape(3, n)
        lims, sc, ids = _np(*ix.search_range(q_in, 2.0))
        assert lims.tolist() == [0, 0, 0, 0] and len(sc) == 0 and len(ids) == 0
        assert sc.dtype == np.float32 and ids.dtype == np.int64
        lims, sc, ids = _np(*ix.search_range(q_in, [-2.0, 2.0, -2.0], sort=False))
        assert lims.tolist() == [0, n, n, 2 * n] and np.array_equal(ids, np.tile(np.arange(n), 2))
        assert np.array_equal(sc.view(np.uint32), everything[[0, 2]].reshape(-1).view(np.uint32))
    assert ix.range_search_stats()["queries"] == 2 * 9
    ix.close()


def test_all_scores_negative_padded_columns_are_never_returned():
    """1001 rows in the positive orthant, negated queries: every score is negative, the zero of a padded column of the score
    row is not — a threshold below zero must not return it"""
    n, dim = 1001, 64
    C = np.abs(R.unit(n, dim, 1))
    Q = -np.abs(R.unit(5, dim, 2))
    S = R.scores64(Q, C)
    assert (S < 0).all()
    t = np.median(S, axis=1).astype(np.float32)
    ix = _index(C)
    for q_in in (Q, torch.tensor(Q).cuda()):
        got = ix.search_range(q_in, t, sort=False)
        _check(got, S, t)
        assert (_np(got[2])[0] < n).all() and (_np(got[1])[0] < 0).all()
    lims, _, ids = ix.search_range(Q, -10.0, sort=False)
    assert lims.tolist() == [0, n, 2 * n, 3 * n, 4 * n, 5 * n] and ids.max() == n - 1
    ix.close()


# -------------------------------------------------------------------------------------------------- 5. filters ---
def test_filters():
    C, Q, t, S = X.random_case(5000, 37, 256, CYCLE_A)
    M = F.random_filters(len(C), (0.5, 0.05, 0.002), seed=11)
    foq = (np.arange(len(Q)) % 4 - 1).astype(np.int64)
    ref_lims = X.range_ref(Q, C, t, M, foq)[0]
    assert (np.diff(ref_lims)[foq == 2] == 0).all() and M[2].sum() == 10  # a filter whose 10 allowed rows all score below t = 0.30
    assert (np.diff(ref_lims)[foq == 0] > 0).any()
    ix = _index(C, M)
    _four_ways(ix, Q, S, t, "filters", masks=M, foq=foq)
    plain = split_ranges(*_np(*ix.search_range(Q, t, sort=False)))
    for q_in, f_in in ((Q, foq), (torch.tensor(Q).cuda(), torch.tensor(foq).cuda())):
        got = split_ranges(*_np(*ix.search_range(q_in, t, f_in, sort=False)))
        for q in range(len(Q)):                                          # the unfiltered result cut by the mask, bit for bit
            keep = M[foq[q]][plain[q][1]] if foq[q] >= 0 else np.ones(len(plain[q][1]), dtype=bool)
            assert np.array_equal(got[q][1], plain[q][1][keep])
            assert np.array_equal(got[q][0].view(np.uint32), plain[q][0][keep].view(np.uint32))
    assert len(got[3][1]) == 0 and foq[3] == 2
    ix.close()


def test_two_query_blocks_under_filters():
    """600 rows (three 256-row tiles, the last partial), 257 queries (a second block of one query), a half-density and an empty
    filter: the block's thresholds, filters and lims start at its first query.  Query 256 is on filter 0."""
    C, Q, t, S = X.random_case(600, 257, 64, CYCLE_B)
    M = np.concatenate([F.random_filters(600, (0.5,), seed=11), np.zeros((1, 600), dtype=bool)])
    foq = (np.arange(257) % 3 - 1).astype(np.int64)                      # -1 (no filter), 0, 1 (allows nothing), ...
    ref_lims = X.range_ref(Q, C, t, M, foq)[0]
    assert foq[256] == 0 and ref_lims[257] > ref_lims[256] and (np.diff(ref_lims)[foq == 1] == 0).all()
    ix = _index(C, M)
    _four_ways(ix, Q, S, t, "two blocks, filters", masks=M, foq=foq)
    ix.close()


# --------------------------------------------------------------------------- 6. a segment does not depend on its batch ---
def test_a_query_alone_equals_its_segment_in_the_batch():
    C, Q, t, S = X.random_case(3001, 300, 128, CYCLE_B)
    ix = _index(C)
    lims, sc, ids = ix.search_range(Q, t, sort=False)
    seg = slice(lims[299], lims[300])                                    # query 299: beyond the 256-query block boundary
    assert lims[300] - lims[299] > 0
    l1, s1, i1 = ix.search_range(Q[299:300], t[299:300], sort=False)
    assert l1.tolist() == [0, lims[300] - lims[299]]
    assert np.array_equal(i1, ids[seg]) and np.array_equal(s1.view(np.uint32), sc[seg].view(np.uint32))
    ix.close()


# ---------------------------------------------------------------------------------------- 7. certification off ---
def test_certification_off_is_still_exact():
    C, Q, t, S = X.random_case(5000, 37, 256, CYCLE_A)
    ix = _index(C)
    want = _bits(ix.search_range(Q, t, sort=False))
    ix.set_search_eps(-1.0)
    got = ix.search_range(Q, t, sort=False)
    _check(got, S, t)
    assert _bits(got) == want
    ix.close()


# ------------------------------------------------------------------------------------- 8. errors, the raw ABI ---
def _vp(x):
    if x is None:
        return ctypes.c_void_p(None)
    return ctypes.c_void_p(x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data)


def _raw_range(ix, Q, thr, foq=None, max_total=1 << 20, lims=None):
    """vr_index_search_range itself: host arrays, or cuda tensors -> (status, lims, total)"""
    cuda = isinstance(Q, torch.Tensor)
    nq = Q.shape[0]
    if lims is None:
        lims = torch.full((nq + 1,), -7, dtype=torch.int64, device=Q.device) if cuda else np.full(nq + 1, -7, dtype=np.int64)
    total = ctypes.c_int64(-7)
    st = ix.lib.vr_index_search_range(ix._h, _vp(Q), nq, _vp(thr), _vp(foq), max_total, _vp(lims), ctypes.byref(total), 1 if cuda else 0,
                                      ctypes.c_void_p(_stream_ptr(ix.device)))
    return st, _np(lims)[0], int(total.value)


def _raw_results(ix, n):
    sc, ids = np.full(max(n, 1), -7, dtype=np.float32), np.full(max(n, 1), -7, dtype=np.int64)
    st = ix.lib.vr_index_range_results(ix._h, _vp(sc), _vp(ids), n, 0, ctypes.c_void_p(_stream_ptr(ix.device)))
    return st, sc[:n], ids[:n]


def _same_bits(a, b):
    (s0, i0), (s1, i1) = _np(*a), _np(*b)
    return np.array_equal(s0.view(np.uint32), s1.view(np.uint32)) and np.array_equal(i0, i1)


def test_errors_leave_everything_else_alone():
    n = 600
    C, Q = R.unit(n, 64, 1), R.unit(4, 64, 2)
    M = F.random_filters(n, (0.5, 0.1), seed=11)
    S = R.scores64(Q, C)
    t = np.full(4, 0.1, dtype=np.float32)
    foq = np.array([0, 1, -1, 1], dtype=np.int32)
    ix = HipIndex(64, n + 10)
    # an empty index: zero lims and total 0, and an (empty) result to fetch
    st, lims, total = _raw_range(ix, Q, t)
    assert st == VR_OK and lims.tolist() == [0] * 5 and total == 0 and _raw_results(ix, 0)[0] == VR_OK
    assert _raw_results(ix, 1)[0] == VR_ERR_STATE
    ix.add(C)
    assert _raw_results(ix, 0)[0] == VR_OK                               # add keeps the result, reset drops it
    ix.reset(); ix.add(C)
    assert _raw_results(ix, 0)[0] == VR_ERR_STATE                        # no range search since the reset
    ix.set_filters(M)
    before = (ix.search(Q, 10), ix.search_filtered(Q, 10, foq))
    stats = (ix.search_stats(), ix.filter_search_stats(), ix.group_search_stats(), ix.search_plan(4))

    def untouched():
        return (ix.search_stats(), ix.filter_search_stats(), ix.group_search_stats(), ix.search_plan(4)) == stats

    st, lims, total = _raw_range(ix, Q, t, foq)
    ref = X.range_ref(Q, C, t, M, foq)
    assert st == VR_OK and np.array_equal(lims, ref[0]) and total == ref[0][-1] > 2
    good = _raw_results(ix, total)
    assert good[0] == VR_OK and np.array_equal(good[2], ref[2])
    assert _raw_results(ix, total + 1)[0] == VR_ERR_STATE                # n above the last total
    assert "range search found" in _lib.load().vr_last_error().decode()
    st, part_sc, part_ids = _raw_results(ix, 2)                          # a prefix is fine
    assert st == VR_OK and np.array_equal(part_ids, ref[2][:2])

    def previous_result_intact():
        again = _raw_results(ix, total)
        return again[0] == VR_OK and np.array_equal(again[2], good[2]) and np.array_equal(again[1].view(np.uint32), good[1].view(np.uint32))

    # argument checks: before any launch, outputs and the previous result untouched
    for bad in (np.nan, np.inf, -np.inf):
        tb = t.copy(); tb[2] = bad
        st, lims, tot = _raw_range(ix, Q, tb)
        assert st == VR_ERR_INVALID and (lims == -7).all() and tot == -7 and previous_result_intact()
    assert _raw_range(ix, Q, t, max_total=0)[0] == VR_ERR_INVALID
    assert _raw_range(ix, Q[:0], t[:0])[0] == VR_ERR_INVALID             # nq < 1
    assert ix.lib.vr_index_search_range(ix._h, _vp(Q), 4, _vp(None), _vp(None), 100, _vp(np.zeros(5, np.int64)),
                                        ctypes.byref(ctypes.c_int64()), 0, None) == VR_ERR_INVALID
    for bad in (2, -2):
        st, lims, tot = _raw_range(ix, Q, t, np.array([0, bad, -1, 1], dtype=np.int32))
        assert st == VR_ERR_INVALID and (lims == -7).all() and previous_result_intact()
        with pytest.raises(ValueError):
            ix.search_range(Q, t, [0, bad, -1, 1])
    with pytest.raises(ValueError):
        ix.search_range(Q, [0.1, 0.2])                                   # 2 thresholds for 4 queries
    assert untouched()
    # capacity: one below the needed total
    st, lims, tot = _raw_range(ix, Q, t, foq, max_total=total - 1)
    assert st == VR_ERR_CAPACITY and tot == -7 and (lims == -7).all()
    assert "query block 0" in _lib.load().vr_last_error().decode()
    assert _raw_results(ix, 1)[0] == VR_ERR_STATE and _raw_results(ix, 0)[0] == VR_ERR_STATE    # the previous result is gone
    with pytest.raises(_lib.VisragHipError):
        ix.search_range(Q, t, foq, max_total=total - 1)
    st, lims, tot = _raw_range(ix, Q, t, foq, max_total=total)           # exactly enough
    assert st == VR_OK and tot == total and previous_result_intact()
    # on the device a NaN threshold or an out-of-range filter cannot be seen before the launch: an empty segment, neighbours unaffected
    tb = t.copy(); tb[1] = np.nan
    st, lims, tot = _raw_range(ix, torch.tensor(Q).cuda(), torch.tensor(tb).cuda(), torch.tensor(foq).cuda())
    per, per_ref = np.diff(lims), np.diff(ref[0])
    assert st == VR_OK and per[1] == 0 and per[[0, 2, 3]].tolist() == per_ref[[0, 2, 3]].tolist() and tot == per.sum()
    st, _, ids = _raw_results(ix, tot)
    keep = np.ones(len(ref[2]), dtype=bool); keep[ref[0][1]:ref[0][2]] = False
    assert st == VR_OK and np.array_equal(ids, ref[2][keep])
    for bad_t, bad_f in ((np.inf, 0), (0.1, 2), (0.1, -7)):
        tb, fb = t.copy(), foq.copy()
        tb[3], fb[3] = bad_t, bad_f
        st, lims, tot = _raw_range(ix, torch.tensor(Q).cuda(), torch.tensor(tb).cuda(), torch.tensor(fb).cuda())
        per = np.diff(lims)
        assert st == VR_OK and per[3] == 0 and per[:3].tolist() == per_ref[:3].tolist()
    _check(ix.search_range(Q, t, foq, sort=False), S, t, M, foq)
    assert untouched()
    assert _same_bits(ix.search(Q, 10), before[0]) and _same_bits(ix.search_filtered(Q, 10, foq), before[1])
    # filter_of_query while no filters are set for the rows present
    ix.add(C[:10])
    assert ix.n_filters == 0 and _raw_range(ix, Q, t, foq)[0] == VR_ERR_STATE
    assert _raw_range(ix, Q, t)[0] == VR_OK                              # ... but none are needed without it
    ix.close()


def test_the_store_grows_in_the_second_block_and_a_capacity_failure_there():
    """400 rows, 300 queries (two blocks); thresholds -4 (every row) for queries 0..155 and 256..299, 4 (no row) between them.
    Block 0 packs 62 400 entries into the first reservation of 65 536; block 1's 17 600 make the store grow with those kept.  A
    fresh index per caller, so that the device caller and the host caller each grow it.  With max_total one short the failure is
    raised in block 1: no result is left."""
    C, Q = R.unit(400, 64, 1), R.unit(300, 64, 2)
    t = np.where((np.arange(300) < 156) | (np.arange(300) >= 256), -4.0, 4.0).astype(np.float32)
    ref = X.range_ref(Q, C, t)
    assert ref[0][256] == 62400 and ref[0][300] == 80000
    first = None
    for cuda in (True, False):
        ix = _index(C)
        q_in, t_in = (torch.tensor(Q).cuda(), torch.tensor(t).cuda()) if cuda else (Q, t)
        got = ix.search_range(q_in, t_in, sort=False)
        lims, sc, ids = _np(*got)
        assert np.array_equal(lims, ref[0]) and np.array_equal(ids, ref[2])
        np.testing.assert_allclose(sc, ref[1], atol=ATOL, rtol=0)
        first = first or _bits(got)
        assert _bits(got) == first                                       # host and device callers: the same bits
        st, _, tot = _raw_range(ix, q_in, t_in, max_total=79999)
        assert st == VR_ERR_CAPACITY and tot == -7 and "query block 1" in _lib.load().vr_last_error().decode()
        assert _raw_results(ix, 0)[0] == VR_ERR_STATE and _raw_results(ix, 1)[0] == VR_ERR_STATE
        st, lims, tot = _raw_range(ix, q_in, t_in, max_total=80000)       # exactly enough
        assert st == VR_OK and tot == 80000 and np.array_equal(lims, ref[0]) and np.array_equal(_raw_results(ix, tot)[2], ref[2])
        ix.close()


def test_existing_searches_are_untouched():
    C, Q, t, S = X.random_case(5000, 37, 256, CYCLE_A)
    M = F.random_filters(len(C), (0.5, 0.05, 0.002), seed=11)
    foq = (np.arange(len(Q)) % 4 - 1).astype(np.int64)
    ix = _index(C, M)
    ix.set_groups(R.random_offsets(len(C), 7))
    before = [ix.search(Q, 10), ix.search(Q, 40), ix.search_filtered(Q, 10, foq), ix.search_groups(Q, 10)[:2], ix.search_diverse(Q, 5)]
    stats = (ix.search_stats(), ix.filter_search_stats(), ix.group_search_stats(), ix.search_plan(len(Q)))
    ix.search_range(Q, t); ix.search_range(torch.tensor(Q).cuda(), t, foq)
    assert (ix.search_stats(), ix.filter_search_stats(), ix.group_search_stats(), ix.search_plan(len(Q))) == stats
    assert ix.n_filters == 3 and ix.n_groups > 0
    rstats = ix.range_search_stats()
    assert rstats["queries"] == 2 * len(Q)
    now = [ix.search(Q, 10), ix.search(Q, 40), ix.search_filtered(Q, 10, foq), ix.search_groups(Q, 10)[:2], ix.search_diverse(Q, 5)]
    assert all(_same_bits(a, b) for a, b in zip(now, before))
    assert ix.range_search_stats() == rstats                             # ... and the other searches count nothing here
    ix.close()


# ------------------------------------------------------------------------------------------ 9. host consumers ---
def _write_kb(path, C, names):
    os.makedirs(path)
    np.save(os.path.join(path, "reps.npy"), C)
    with open(os.path.join(path, "index2img_filename.txt"), "w") as f:
        f.write("\n".join(names))


def test_demo_duplicate_pages(tmp_path):
    from visrag_amd import demo
    D, _ = R.decks(30, 10, 256, 3e-4)
    C = np.concatenate([D, R.unit(200, 256, 9)])
    names = [f"deck_{d}.pdf_{i}.png" for d in range(30) for i in range(10)] + [f"filler_{j}.pdf_0.png" for j in range(200)]
    perm = np.random.default_rng(3).permutation(len(C))                  # decks scattered over the base
    C, names = C[perm], [names[i] for i in perm]
    S = R.scores64(C, C)
    same = np.array([doc_of_page(a) for a in names])[:, None] == np.array([doc_of_page(b) for b in names])[None, :]
    assert S[same].min() > 0.99 + 1e-3 and S[~same].max() < 0.99 - 1e-3  # the threshold separates decks from everything else
    kb = str(tmp_path / "kb")
    _write_kb(kb, C, names)
    groups = demo.duplicate_pages(kb, 0.99, batch=128)                   # 500 rows: four batches
    assert len(groups) == 30 and all(len(g) == 10 for g in groups)
    assert all(len({doc_of_page(n) for n in g}) == 1 and doc_of_page(g[0]).startswith("deck_") for g in groups)
    first = [names.index(g[0]) for g in groups]
    assert first == sorted(first) and all([names.index(n) for n in g] == sorted(names.index(n) for n in g) for g in groups)
    ix, nm = demo.load_knowledge_base(kb, 0)
    assert demo.duplicate_pages(kb, 0.99, index=ix, names=nm) == groups
    assert demo.duplicate_pages(kb, 1.5, index=ix, names=nm) == []
    assert demo.duplicate_pages(str(tmp_path / "missing"), 0.99) is None
    ix.close()


def test_demo_retrieve_above(tmp_path, monkeypatch):
    from visrag_amd import demo
    D, _ = R.decks(6, 5, 64, 0.05)
    C = np.concatenate([D, R.unit(40, 64, 9)])
    names = [f"deck_{d}.pdf_{i}.png" for d in range(6) for i in range(5)] + [f"other_{j}.pdf_0.png" for j in range(40)]
    qvec = R.unit(6, 64, 5)[2:3]                                         # the base vector of deck 2
    kb = str(tmp_path / "kb")
    _write_kb(kb, C, names)
    asked = []
    monkeypatch.setattr(demo, "encode", lambda model, tok, texts: (asked.append(texts), qvec)[1])   # the model: a fixed query vector
    S = R.scores64(qvec, C)[0]
    order = np.lexsort((np.arange(len(C)), -S))
    want = [int(i) for i in order if S[i] >= 0.2]
    assert len(want) >= 5 and min(abs(S - 0.2)) > 1e-4
    ix, nm = demo.load_knowledge_base(kb, 0)
    paths, scores = demo.retrieve_above(kb, "which deck?", 0.2, None, None, index=ix, names=nm, return_scores=True)
    assert asked == [[demo.QUERY_INSTRUCTION + "which deck?"]]
    assert paths == [os.path.join(kb, names[i]) for i in want]
    np.testing.assert_allclose(scores, S[want], atol=ATOL, rtol=0)
    assert scores == sorted(scores, reverse=True)
    assert demo.retrieve_above(kb, qvec[0], 0.2, None, None, index=ix, names=nm) == paths          # an embedding as the query
    assert demo.retrieve_above(kb, torch.tensor(qvec), 0.2, None, None, index=ix, names=nm, max_pages=3) == paths[:3]
    docs = ["deck_2.pdf", "other_7.pdf", "no_such.pdf"]
    only = demo.retrieve_above(kb, qvec, 0.2, None, None, index=ix, names=nm, documents=docs)
    assert only == [p for p in paths if doc_of_page(os.path.basename(p)) in docs] and len(only) >= 5
    assert demo.retrieve_above(kb, qvec, 0.2, None, None, index=ix, names=nm, documents=["no_such.pdf"], return_scores=True) == ([], [])
    assert demo.retrieve_above(kb, qvec, 5.0, None, None, index=ix, names=nm) == []
    assert demo.retrieve_above(str(tmp_path / "missing"), qvec, 0.2, None, None) is None
    assert demo.retrieve(kb, qvec, 3, None, None, index=ix, names=nm, documents=docs) == only[:3]   # retrieve: as before
    ix.close()


def test_retriever_retrieve_range(tmp_path):
    from visrag_amd import retriever
    from visrag_amd.utils import save_as_trec, write_shard
    C, Q = R.unit(301, 64, 9), R.unit(3, 64, 10)
    names = [f"page_{i}" for i in range(len(C))]
    half = 150
    write_shard(str(tmp_path / "embeddings.corpus.rank.0"), C[:half], names[:half])
    write_shard(str(tmp_path / "embeddings.corpus.rank.1"), C[half:], names[half:])
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, ["q0", "q1", "q2"])
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    result = retriever.retrieve_range(args, 0.15)
    ix = _index(C)
    lims, sc, ids = ix.search_range(Q, 0.15)
    ix.close()
    single = {f"q{q}": {names[int(i)]: float(s) for s, i in zip(*seg)} for q, seg in enumerate(split_ranges(lims, sc, ids))}
    assert result == single and all(list(result[q].items()) == list(single[q].items()) for q in single)
    assert min(len(v) for v in single.values()) >= 5 and len({len(v) for v in single.values()}) > 1   # a run of variable depth
    _check((lims, sc, ids), R.scores64(Q, C), 0.15, ranked=True)
    capped = retriever.retrieve_range(args, 0.15, max_per_query=4)
    assert all(list(capped[q].items()) == list(single[q].items())[:4] for q in single)
    save_as_trec(result, str(tmp_path / "run.trec"))
    assert sum(1 for _ in open(tmp_path / "run.trec")) == int(lims[-1])
