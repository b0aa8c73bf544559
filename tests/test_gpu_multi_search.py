"""-m gpu: the fused search (vr_index_search_multi / vr_index_multi_search_stats, csrc/search_multi.hip) against the library's own
searches — strict, bit for bit — and against the numpy reference tests/multi_search_ref.py.

Strict tests (no tolerance, from host arrays and from CUDA tensors): the library's own score matrix (`search_range(threshold =
-4, sort=False)`: every row, the library's score bits) fused and ranked in numpy on orderable bits IS the result — scores, ids
and `which`; groups of one are `search` / `search_filtered` with which == 0, in every setting of set_search_eps; a repeated
sub-query changes nothing, a permutation changes `which` alone; one call over many groups equals one call per group however the
groups pack into blocks of 256 sub-queries; tails (-inf, -1, -1) past the allowed rows; the lowest ids inside a tier of
bit-identical rows; an edited index answers as a freshly built one; every argument error leaves the outputs untouched.

Against fp64 (no excuse mechanism, the bar is the whole test): scores within the project's ATOL = 1e-5 of the fp64 fused score; a
row of fp64 fused score s returned at position j has j in [#(F > s + 6e-7), #(F >= s - 6e-7) - 1]; the sub-query named by
`which` has an fp64 score within 6e-7 of the fp64 fused score.  6e-7 is the rank search's TOL: a fused fp32 score is one fp32 dot
product, inside the standing 3e-7 of its fp64 value, and two such scores are compared.  k = 100; the reference alone gives these
intervals for its own top 100 (tests/test_cpu_multi_search_ref.py pins them), as (positions, widened intervals, widest):

    corpus                size cycle          groups     max             min
    (5000, 37, 256)       1,2,3,4,5,6,7,9        8       (800, 2, 1)     (800, 1, 1)
    (3001, 300, 128)      1,3,8,2,64,5          23       (2300, 2, 1)    (2300, 4, 1)
    (20000, 64, 2304)     4,1,7,2,16,3          12       (1200, 18, 1)   (1200, 14, 1)
    families, dim 2304    2,3                    4       (400, 60, 2)    (400, 33, 2)
    norms (4000, 20, 256) 1,4,2,5                8       (800, 0, 0)     (800, 0, 0)

Measured on an MI355X (the same for host arrays and CUDA tensors), max / min in the table's order: every position inside its
interval; positions that differ from the reference's own fp64 ranking 0 / 0, 0 / 0, 0 / 0, 9 / 4, 0 / 0 (all inside near-ties);
largest |score - fp64| 2.5e-8 / 2.2e-8, 5.3e-8 / 3.3e-8, 9.4e-9 / 9.3e-9, 8.6e-8 / 7.6e-8, 7.0e-8 / 5.9e-8.  Band columns re-scored
per row returned: 1.4 / 1.6, 1.3 / 1.4, 3.1 / 5.1, 22.5 / 11.0, 1.4 / 1.7; fp32 row dots per row returned: 6.6 / 7.6, 18.8 / 23.6,
18.4 / 39.4, 48.8 / 18.9, 3.5 / 5.0.
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
from tests import multi_search_ref as M  # noqa: E402
from tests import range_search_ref as X  # noqa: E402
from tests import rank_search_ref as K  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.engine import HipIndex, _stream_ptr  # noqa: E402

ATOL = 1e-5
VR_OK, VR_ERR_INVALID, VR_ERR_STATE = 0, 1, 3
FUSES = ("max", "min")


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


def _orderable(x):
    """the library's order-preserving key of a float32 (search_common.h: f32_orderable): -0.0 < +0.0"""
    u = _u32(x)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _matrix(ix, Q):
    """E f32 [n_sub][rows]: the library's own score of every (sub-query, row) — the range search below every score, ids ascending"""
    n = len(ix)
    lims, sc, ids = ix.search_range(Q, -4.0, sort=False)
    assert np.array_equal(lims, np.arange(len(Q) + 1) * n) and np.array_equal(ids.reshape(len(Q), n), np.tile(np.arange(n), (len(Q), 1)))
    return sc.reshape(len(Q), n)


def _expect(E, lims, k, fuse, masks=None):
    """the contract in numpy on orderable bits -> (scores f32, ids i64, which i32) [n_groups][k]; masks: per group a bool row mask
    or None"""
    ng, n = len(lims) - 1, E.shape[1]
    sc, ids = np.full((ng, k), -np.inf, dtype=np.float32), np.full((ng, k), -1, dtype=np.int64)
    which = np.full((ng, k), -1, dtype=np.int32)
    O = _orderable(E)
    for g in range(ng):
        sub = O[lims[g]:lims[g + 1]]
        fused = sub.max(0) if fuse == "max" else sub.min(0)
        rows = np.arange(n) if masks is None or masks[g] is None else np.flatnonzero(masks[g])
        order = rows[np.lexsort((rows, -fused[rows].astype(np.int64)))][:k]
        w = np.argmax(sub[:, order] == fused[order][None, :], axis=0)
        ids[g, :len(order)], which[g, :len(order)] = order, w
        sc[g, :len(order)] = E[lims[g] + w, order]
    return sc, ids, which


def _same(got, want):
    sc, ids, which = _np(*got)
    assert sc.dtype == np.float32 and ids.dtype == np.int64 and which.dtype == np.int32
    assert sc.shape == ids.shape == which.shape == want[1].shape
    assert np.array_equal(ids, want[1])
    assert np.array_equal(_u32(sc), _u32(want[0]))
    assert np.array_equal(which, want[2])


def _both(Q, lims=None, fog=None):
    """the same call from host arrays and from CUDA tensors"""
    yield Q, lims, fog
    yield torch.tensor(Q).cuda(), (None if lims is None else torch.tensor(lims)), (None if fog is None else torch.tensor(fog).cuda())


# ------------------------------------------------------------------------- 1. the library's own score matrix ---
@pytest.mark.parametrize("nd,nq,dim,cycle", [(5000, 37, 256, (1, 2, 3, 4, 5, 6, 7, 9)), (2000, 24, 2304, (1, 2, 3, 6))])
def test_fused_ranking_of_the_librarys_own_scores(nd, nq, dim, cycle):
    C, Q = R.unit(nd, dim, 1), R.unit(nq, dim, 2)
    lims = M.layout(nq, cycle)
    ix = _index(C)
    E = _matrix(ix, Q)
    for fuse in FUSES:
        for k in (1, 10, 100, 1000):
            want = _expect(E, lims, k, fuse)
            assert (want[1] >= 0).all()
            for q_in, l_in, _ in _both(Q, lims):
                ix.multi_search_stats(reset=True)
                got = ix.search_multi(q_in, l_in, k, fuse)
                assert all((isinstance(x, torch.Tensor) and x.is_cuda) if q_in is not Q else isinstance(x, np.ndarray) for x in got)
                _same(got, want)
                st = ix.multi_search_stats()
                assert st["groups"] == len(lims) - 1 and st["candidates"] >= (len(lims) - 1) * k and st["dots"] >= st["candidates"]
        ix.multi_search_stats(reset=True)
        ix.search_multi(Q, lims, 100, fuse)
        st = ix.multi_search_stats()
        print(f"{nd}x{nq}x{dim} {fuse} k 100: {st}, {st['candidates'] / ((len(lims) - 1) * 100):.1f} band candidates per row returned")
    # [n_groups][m][dim] with lims=None is the flat layout with equal groups
    m = 3
    cube = Q[: (nq // m) * m].reshape(nq // m, m, dim)
    _same(ix.search_multi(cube, None, 10, "min"), _expect(E, np.arange(nq // m + 1) * m, 10, "min"))
    _same(ix.search_multi(torch.tensor(cube).cuda(), None, 10, "max"), _expect(E, np.arange(nq // m + 1) * m, 10, "max"))
    ix.close()


# ------------------------------------------------------------------------------------------ 2. groups of one ---
@pytest.fixture(scope="module")
def big():
    C, Q, _, _ = X.random_case(20000, 64, 2304, (0.05, 0.07))
    M_ = F.random_filters(len(C), (0.5, 0.01), seed=11)
    ix = _index(C, M_)
    yield ix, Q
    ix.close()


def test_groups_of_one_are_the_plain_search(big):
    ix, Q = big
    lims = np.arange(len(Q) + 1)
    zero = lambda k: np.zeros((len(Q), k), dtype=np.int32)
    for k in (10, 100):
        s, i = ix.search(Q, k)
        for fuse in FUSES:
            for q_in, l_in, _ in _both(Q, lims):
                _same(ix.search_multi(q_in, l_in, k, fuse), (s, i, zero(k)))
    for eps in (-1.0, 0.01, float("nan")):                               # certification off / a caller's model / the default again
        ix.set_search_eps(eps)
        s, i = ix.search(Q, 10)
        for fuse in FUSES:
            _same(ix.search_multi(Q, lims, 10, fuse), (s, i, zero(10)))
    foq = (np.arange(len(Q)) % 2).astype(np.int64)                       # densities 0.5 and 0.01
    for k in (10, 100):
        s, i = ix.search_filtered(Q, k, foq)
        for fuse in FUSES:
            for q_in, l_in, f_in in _both(Q, lims, foq):
                _same(ix.search_multi(q_in, l_in, k, fuse, f_in), (s, i, zero(k)))


def test_repeated_and_permuted_sub_queries(big):
    ix, Q = big
    k = 20
    for fuse in FUSES:
        one = _np(*ix.search_multi(Q[:6], np.arange(7), k, fuse))
        rep = np.repeat(Q[:6], 5, axis=0)                                 # every group: one vector five times
        for q_in, l_in, _ in _both(rep, np.arange(7) * 5):
            _same(ix.search_multi(q_in, l_in, k, fuse), one)              # (which == 0: the lowest of the equal sub-queries)
        lims = np.array([0, 5, 12, 13])
        base = _np(*ix.search_multi(Q[:13], lims, k, fuse))
        assert (base[2][:2] > 0).any()                                    # (more than one sub-query decides rows)
        perm = np.concatenate([[3, 0, 4, 1, 2], 5 + np.array([6, 5, 4, 3, 2, 1, 0]), [12]])
        got = _np(*ix.search_multi(Q[:13][perm], lims, k, fuse))
        assert np.array_equal(got[1], base[1]) and np.array_equal(_u32(got[0]), _u32(base[0]))
        for g in range(3):                                                # position `which` of the permuted group is the same sub-query
            assert np.array_equal(perm[lims[g] + got[2][g]], lims[g] + base[2][g]), g


# ------------------------------------------------------------------------------------------------ 3. packing ---
def test_packing_into_blocks_of_256_sub_queries():
    C, Q = R.unit(3001, 128, 1), R.unit(300, 128, 2)
    ix = _index(C)
    E = _matrix(ix, Q)
    layouts = [np.array([0, 200, 300]),                                   # the second group does not fit: the block closes early
               np.array([0, 256, 300]),                                   # a group that fills a block
               M.layout(300, (1, 3, 8, 2, 64, 5))]
    for lims in layouts:
        for fuse in FUSES:
            want = _expect(E, lims, 10, fuse)
            for q_in, l_in, _ in _both(Q, lims):
                _same(ix.search_multi(q_in, l_in, 10, fuse), want)
            for g in range(len(lims) - 1):                                # one call equals one call per group
                got = ix.search_multi(Q[lims[g]:lims[g + 1]], [0, lims[g + 1] - lims[g]], 10, fuse)
                _same(got, tuple(x[g:g + 1] for x in want))
    ix.close()


# -------------------------------------------------------------------------------------- 4. tails and filters ---
def test_tails_and_filters():
    n = 700
    C, Q = R.unit(n, 64, 1), R.unit(12, 64, 2)
    three = np.zeros(n, dtype=bool); three[[5, 300, 699]] = True
    masks = np.concatenate([F.random_filters(n, (0.5,), seed=11), three[None], np.zeros((1, n), dtype=bool)])
    lims = np.array([0, 1, 4, 6, 12])
    ix = HipIndex(64, n)
    ix.add(C)
    E = _matrix(ix, Q)
    with pytest.raises(_lib.VisragHipError):                             # no filters set: VR_ERR_STATE
        ix.search_multi(Q, lims, 10, "max", filter_of_group=np.zeros(4, dtype=np.int64))
    ix.set_filters(masks)
    for fuse in FUSES:
        for q_in, l_in, _ in _both(Q, lims):                             # k greater than the number of rows
            got = ix.search_multi(q_in, l_in, 1000, fuse)
            _same(got, _expect(E, lims, 1000, fuse))
            assert (_np(*got)[1][:, n:] == -1).all() and (_np(*got)[2][:, n:] == -1).all() and (_np(*got)[1][:, :n] >= 0).all()
        for fog in ([1, 1, 1, 1], [2, 2, 2, 2], [0, -1, 2, 1], [-1, -1, -1, -1]):   # 3 rows allowed; none; a mix with -1; no filter
            fog = np.asarray(fog, dtype=np.int64)
            want = _expect(E, lims, 10, fuse, [None if f < 0 else masks[f] for f in fog])
            for q_in, l_in, f_in in _both(Q, lims, fog):
                _same(ix.search_multi(q_in, l_in, 10, fuse, f_in), want)
        got = _np(*ix.search_multi(Q, lims, 10, fuse, 1))
        assert np.array_equal(np.sort(got[1][:, :3], axis=1), np.tile([5, 300, 699], (4, 1))) and (got[1][:, 3:] == -1).all()
        got = _np(*ix.search_multi(Q, lims, 10, fuse, 2))                # density 0: a full row of tails
        assert (got[1] == -1).all() and np.isneginf(got[0]).all() and (got[2] == -1).all()
        _same(ix.search_multi(Q, lims, 10, fuse, -1), _np(*ix.search_multi(Q, lims, 10, fuse)))
    ix.close()


def test_two_blocks_of_sub_queries_under_filters():
    """600 rows (three 256-row tiles, the last partial), 257 sub-queries in groups of 1, 2 and 3 (the last group alone in a second
    block), a half-density and an empty filter: the block's lims, filters of sub-queries and outputs start at its first group"""
    C, Q = R.unit(600, 64, 1), R.unit(257, 64, 2)
    masks = np.concatenate([F.random_filters(600, (0.5,), seed=11), np.zeros((1, 600), dtype=bool)])
    lims = M.layout(257, (1, 2, 3))
    ng = len(lims) - 1
    fog = ((ng - np.arange(ng)) % 3 - 1).astype(np.int64)                # -1 (no filter), 0, 1 (allows nothing); the last group on filter 0
    assert lims[-2] <= 256 < lims[-1] and fog[-1] == 0 and set(fog.tolist()) == {-1, 0, 1}
    ix = _index(C, masks)
    E = _matrix(ix, Q)
    for fuse in FUSES:
        want = _expect(E, lims, 5, fuse, [None if f < 0 else masks[f] for f in fog])
        assert (want[1][fog == 1] == -1).all() and (want[1][fog != 1] >= 0).all()
        for q_in, l_in, f_in in _both(Q, lims, fog):
            _same(ix.search_multi(q_in, l_in, 5, fuse, f_in), want)
    ix.close()


# ------------------------------------------------------------------------------------------------ 5. tie tier ---
def test_tie_tier():
    C, Q, _ = R.tie_tier()
    n, high = len(C), 7 * np.arange(100) + 3
    tied = np.setdiff1d(np.arange(n), high)
    ix = _index(C)
    E = _matrix(ix, Q)
    lims = np.array([0, 2, 3])
    for fuse in FUSES:
        for k in (50, 150, 1000):                                        # 150 and 1 000 cut inside the tier: the lowest ids
            want = _expect(E, lims, k, fuse)
            for q_in, l_in, _ in _both(Q, lims):
                _same(ix.search_multi(q_in, l_in, k, fuse), want)
            if k > 100:
                assert np.isin(want[1][:, :100], high).all() and np.array_equal(want[1][:, 100:], np.tile(tied[:k - 100], (2, 1)))
    qq = np.stack([Q[0], Q[0]])                                          # min-fusion of [q, q] equals max-fusion of it
    for k in (50, 1000):
        _same(ix.search_multi(qq, [0, 2], k, "min"), _np(*ix.search_multi(qq, [0, 2], k, "max")))
        _same(ix.search_multi(qq, [0, 2], k, "min"), _np(*ix.search_multi(Q[:1], [0, 1], k, "max")))
    ix.close()


# --------------------------------------------------------------------------------------------------- 6. edits ---
def test_an_edited_index_answers_as_a_fresh_one():
    C, Q = R.unit(3001, 128, 1).copy(), R.unit(40, 128, 2)
    lims = M.layout(40, (3, 1, 6))
    rng = np.random.default_rng(17)
    gone = rng.choice(len(C), int(0.3 * len(C)), replace=False)
    ix = _index(C)
    ix.search_multi(Q, lims, 10, "max")                                  # (nothing is stored: nothing to invalidate)
    new_id = ix.remove(gone)
    left = C[new_id >= 0]
    upd = rng.choice(len(left), 5, replace=False)
    fresh_rows = R.unit(5, 128, 33)
    ix.update(upd, fresh_rows)
    left[upd] = fresh_rows
    fresh = _index(left)
    E = _matrix(fresh, Q)
    for fuse in FUSES:
        for k in (10, 1000):
            got = ix.search_multi(Q, lims, k, fuse)
            _same(got, _np(*fresh.search_multi(Q, lims, k, fuse)))
            _same(got, _expect(E, lims, k, fuse))
    ix.close(); fresh.close()


# ------------------------------------------------------------------------------------ 7. arguments, the raw ABI ---
def _vp(x):
    if x is None:
        return ctypes.c_void_p(None)
    return ctypes.c_void_p(x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data)


def _raw(ix, Q, lims, k, fuse=0, fog=None, n_sub=None, n_groups=None):
    """vr_index_search_multi itself, host arrays -> (status, scores, ids, which); the outputs start as -7"""
    lims = np.asarray(lims, dtype=np.int64)
    ng = len(lims) - 1 if n_groups is None else n_groups
    n = max((len(lims) - 1) * max(k, 1), 1)
    sc, ids, wh = np.full(n, -7, dtype=np.float32), np.full(n, -7, dtype=np.int64), np.full(n, -7, dtype=np.int32)
    st = ix.lib.vr_index_search_multi(ix._h, _vp(Q), len(Q) if n_sub is None else n_sub, _vp(lims), ng, k, fuse, _vp(fog), _vp(sc),
                                      _vp(ids), _vp(wh), 0, ctypes.c_void_p(_stream_ptr(ix.device)))
    return st, sc, ids, wh


def test_argument_checks_come_before_any_launch():
    n = 600
    C, Q = R.unit(n, 64, 1), R.unit(7, 64, 2)
    masks = F.random_filters(n, (0.5, 0.1), seed=11)
    lims = [0, 3, 4, 7]
    fog = np.array([0, -1, 1], dtype=np.int32)
    zeros = {"groups": 0, "candidates": 0, "dots": 0}
    ix = HipIndex(64, n + 10)
    # the empty index: tails, nothing is launched, nothing counted
    st, sc, ids, wh = _raw(ix, Q, lims, 5)
    assert st == VR_OK and (ids == -1).all() and np.isneginf(sc).all() and (wh == -1).all()
    qd = torch.tensor(Q).cuda()
    out_s, out_i, out_w = torch.full((15,), -7.0).cuda(), torch.full((15,), -7, dtype=torch.int64).cuda(), torch.full((15,), -7, dtype=torch.int32).cuda()
    st = ix.lib.vr_index_search_multi(ix._h, _vp(qd), 7, _vp(np.asarray(lims, dtype=np.int64)), 3, 5, 1, _vp(None), _vp(out_s), _vp(out_i),
                                      _vp(out_w), 1, ctypes.c_void_p(_stream_ptr(ix.device)))
    torch.cuda.synchronize()
    assert st == VR_OK and (out_i.cpu().numpy() == -1).all() and np.isneginf(out_s.cpu().numpy()).all() and (out_w.cpu().numpy() == -1).all()
    assert ix.multi_search_stats() == zeros
    ix.add(C)
    ix.set_filters(masks)
    st, sc, ids, wh = _raw(ix, Q, lims, 20, 1, fog)
    assert st == VR_OK
    E = _matrix(ix, Q)
    want = _expect(E, np.asarray(lims), 20, "min", [masks[0], None, masks[1]])
    _same((sc.reshape(3, 20), ids.reshape(3, 20), wh.reshape(3, 20)), want)
    stats = ix.multi_search_stats()
    assert stats["groups"] == 3
    others = (ix.search_stats(), ix.filter_search_stats(), ix.range_search_stats(), ix.rank_search_stats(), ix.window_search_stats())

    def nothing_ran(st, *outs, code=VR_ERR_INVALID):
        return st == code and all((o == -7).all() for o in outs) and ix.multi_search_stats() == stats

    for k in (0, -1, 1001):
        assert nothing_ran(*_raw(ix, Q, lims, k, 0, fog)), k
    assert "k=1001 unsupported (1..1000)" in _lib.load().vr_last_error().decode()
    for fuse in (2, -1):
        assert nothing_ran(*_raw(ix, Q, lims, 20, fuse, fog)), fuse
    assert "fuse=" in _lib.load().vr_last_error().decode()
    for bad in ([1, 3, 4, 7], [0, 4, 3, 7], [0, 3, 3, 7], [0, 3, 4, 6], [0, 3, 4, 8]):   # lims[0] != 0, decreasing, an empty group, the end
        assert nothing_ran(*_raw(ix, Q, bad, 20, 0, fog)), bad
    wide = R.unit(300, 64, 3)
    assert nothing_ran(*_raw(ix, wide, [0, 257, 300], 20)), "a group of 257"
    assert "257 sub-queries" in _lib.load().vr_last_error().decode()
    assert _raw(ix, wide, [0, 256, 300], 20)[0] == VR_OK
    stats = ix.multi_search_stats()
    for bad in (2, -2):                                                  # a filter index out of range
        fb = np.array([0, bad, -1], dtype=np.int32)
        assert nothing_ran(*_raw(ix, Q, lims, 20, 0, fb))
        with pytest.raises(ValueError):
            ix.search_multi(Q, lims, 20, "max", filter_of_group=fb)
    assert "outside [-1, 2)" in _lib.load().vr_last_error().decode()
    assert ix.lib.vr_index_search_multi(ix._h, _vp(Q), 7, _vp(None), 3, 5, 0, _vp(None), _vp(None), _vp(None), _vp(None), 0, None) == VR_ERR_INVALID
    assert nothing_ran(*_raw(ix, Q, lims, 20, 0, fog, n_groups=-1))
    assert nothing_ran(*_raw(ix, Q, lims, 20, 0, fog, n_sub=-1))
    assert nothing_ran(*_raw(ix, Q, [0], 20, 0, None, n_sub=0), code=VR_OK)      # no group: VR_OK, nothing launched, nothing written
    for bad in ("sum", 0):                                               # the binding's own checks
        with pytest.raises(ValueError):
            ix.search_multi(Q, lims, 5, bad)
    with pytest.raises(ValueError):
        ix.search_multi(Q, None, 5)                                      # lims=None wants [n_groups][m][dim]
    with pytest.raises(ValueError):
        ix.search_multi(Q, lims, 5, "max", filter_of_group=[0, 1])       # one entry per group
    with pytest.raises(_lib.VisragHipError):
        ix.search_multi(Q, lims, 1001)
    # on the device an out-of-range filter index cannot be seen before the launch: that group gets a row of tails
    fb = torch.tensor(np.array([0, 7, 1], dtype=np.int32)).cuda()
    out_s, out_i, out_w = torch.full((3, 5), -7.0).cuda(), torch.full((3, 5), -7, dtype=torch.int64).cuda(), torch.full((3, 5), -7, dtype=torch.int32).cuda()
    st = ix.lib.vr_index_search_multi(ix._h, _vp(qd), 7, _vp(np.asarray(lims, dtype=np.int64)), 3, 5, 0, _vp(fb), _vp(out_s), _vp(out_i),
                                      _vp(out_w), 1, ctypes.c_void_p(_stream_ptr(ix.device)))
    torch.cuda.synchronize()
    want = [np.array(x) for x in _np(*ix.search_multi(Q, lims, 5, "max", np.array([0, 0, 1])))]
    want[0][1], want[1][1], want[2][1] = -np.inf, -1, -1
    assert st == VR_OK
    _same((out_s, out_i, out_w), want)
    assert (ix.search_stats(), ix.filter_search_stats(), ix.range_search_stats(), ix.rank_search_stats(), ix.window_search_stats()) == others
    st2 = ix.multi_search_stats()
    assert ix.multi_search_stats(reset=True) == st2 and ix.multi_search_stats() == zeros
    # a filter index while no filters are set for the rows present
    ix.add(C[:10])
    assert ix.n_filters == 0
    assert _raw(ix, Q, lims, 20, 0, fog)[0] == VR_ERR_STATE and _raw(ix, Q, lims, 20)[0] == VR_OK
    ix.close()


# ------------------------------------------------------------------------------------------------ against fp64 ---
@pytest.mark.parametrize("name", list(M.TABLE))
def test_fused_rankings_and_scores_against_fp64(name):
    C, Q, S = M.case(name)
    cycle, groups, table = M.TABLE[name]
    lims = M.layout(len(Q), cycle)
    ix = _index(C)
    k = M.K_FP64
    for fuse in FUSES:
        Ff = M.fuse_ref(S, lims, fuse)
        first = None
        for q_in, l_in, _ in _both(Q, lims):
            ix.multi_search_stats(reset=True)
            sc, ids, which = _np(*ix.search_multi(q_in, l_in, k, fuse))
            st = ix.multi_search_stats()
            entries = moved = 0
            worst, err = None, 0.0
            for g in range(groups):
                n_g, moved_g, bad = M.check_group(S, lims, g, fuse, ids[g], which[g])
                entries += n_g; moved += moved_g
                worst = worst or (bad and (g,) + bad)
                err = max(err, float(np.abs(sc[g][ids[g] >= 0] - Ff[g][ids[g][ids[g] >= 0]]).max()))
            print(f"{name} {fuse}: {entries} entries, {moved} positions differ from the fp64 ranking, max |score - fp64| {err:.2e}, "
                  f"{st['candidates'] / max(entries, 1):.1f} band candidates and {st['dots'] / max(entries, 1):.1f} row dots per row returned")
            assert entries == table[fuse][0]
            assert err <= ATOL
            assert worst is None, worst                                  # (group, position, row, lo, hi, which, named - fused)
            if first is None:
                first = (_u32(sc).tolist(), ids.tolist(), which.tolist())
            assert (_u32(sc).tolist(), ids.tolist(), which.tolist()) == first    # host and device callers: the same bits
    ix.close()


# ------------------------------------------------------------------------------------------------ host consumers ---
def test_retrieve_fused_over_pickle_shards(tmp_path):
    from visrag_amd import retriever
    from visrag_amd.documents import group_rows
    from visrag_amd.utils import write_shard
    C, Q, bounds = K.shards_case()
    names = [f"page_{i}" for i in range(len(C))]
    for s in range(3):
        write_shard(str(tmp_path / f"embeddings.corpus.rank.{s}"), C[bounds[s]:bounds[s + 1]], names[bounds[s]:bounds[s + 1]])
    qids = [f"t{q % 4}-part{q}" for q in range(len(Q))]
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, qids)
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    topic = lambda qid: qid.split("-")[0]
    order, lims, topics = group_rows([topic(q) for q in qids])
    whole = _index(C)
    for fuse in FUSES:
        sc, ids, _ = whole.search_multi(Q[order], lims, 300, fuse)
        run = retriever.retrieve_fused(args, topic, 300, fuse)
        assert list(run) == topics
        for g, t in enumerate(topics):
            assert list(run[t]) == [names[i] for i in ids[g]]
            assert np.array_equal(_u32(list(run[t].values())), _u32(sc[g]))
    whole.close()


def test_demo_retrieve_any(tmp_path):
    from visrag_amd import demo
    D, _ = R.decks(6, 5, 64, 0.05)
    C = np.concatenate([D, R.unit(40, 64, 9)])
    names = [f"deck_{d}.pdf_{i}.png" for d in range(6) for i in range(5)] + [f"other_{j}.pdf_0.png" for j in range(40)]
    qs = R.unit(6, 64, 5)[[2, 4]]                                        # (embeddings as the questions: decks 2 and 4)
    kb = str(tmp_path / "kb")
    os.makedirs(kb)
    np.save(os.path.join(kb, "reps.npy"), C)
    with open(os.path.join(kb, "index2img_filename.txt"), "w") as f:
        f.write("\n".join(names))
    ix, nm = demo.load_knowledge_base(kb, 0)
    # one question: demo.retrieve's pages
    for fuse in FUSES:
        p, s, w = demo.retrieve_any(kb, qs[:1], 10, None, None, index=ix, names=nm, fuse=fuse, return_scores=True)
        every = [n.rsplit("_", 1)[0] for n in names]
        p1, s1 = demo.retrieve(kb, qs[:1], 10, None, None, index=ix, names=nm, return_scores=True, documents=every)
        assert p == p1 and np.array_equal(_u32(s), _u32(s1)) and w == [0] * 10
    # two questions, any-of: the fused order with the deciding question per page
    E = _matrix(ix, qs)
    want = _expect(E, np.array([0, 2]), 12, "max")
    p, s, w = demo.retrieve_any(kb, qs, 12, None, None, index=ix, names=nm, return_scores=True)
    assert p == [os.path.join(kb, names[i]) for i in want[1][0]] and np.array_equal(_u32(s), _u32(want[0][0])) and w == want[2][0].tolist()
    assert {n.split(".")[0] for n in map(os.path.basename, p[:10])} == {"deck_2", "deck_4"} and set(w[:10]) == {0, 1}
    assert demo.retrieve_any(kb, qs, 12, None, None, index=ix, names=nm) == p
    assert demo.retrieve_any(kb, torch.tensor(qs), 12, None, None, index=ix, names=nm, fuse="min") == \
        [os.path.join(kb, names[i]) for i in _expect(E, np.array([0, 2]), 12, "min")[1][0]]
    # documents=[...] restricts the result
    docs = ["deck_2.pdf", "other_7.pdf"]
    allowed = np.array([n.rsplit("_", 1)[0] in docs for n in names])
    want = _expect(E, np.array([0, 2]), 6, "max", [allowed])
    p, s, w = demo.retrieve_any(kb, qs, 10, None, None, index=ix, names=nm, documents=docs, return_scores=True)
    assert len(p) == 6 and p == [os.path.join(kb, names[i]) for i in want[1][0]] and w == want[2][0].tolist()
    assert demo.retrieve_any(kb, qs, 10, None, None, index=ix, names=nm, documents=["nothing.pdf"]) == []
    assert demo.retrieve_any(kb, qs, 100, None, None, index=ix, names=nm, fuse="min")[69:] == \
        [os.path.join(kb, names[int(_expect(E, np.array([0, 2]), 70, "min")[1][0][69])])]               # the ranking ends at 70 pages
    assert demo.retrieve_any(str(tmp_path / "none"), qs, 5, None, None) is None
    ix.close()
