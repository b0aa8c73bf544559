"""-m gpu: rank fusion (vr_rrf_fuse / vr_index_search_rrf / vr_index_rrf_search_stats, csrc/search_rrf.hip) against the plain-loop
oracle tests/rrf_search_ref.py.  RRF scores depend on positions only, so everything here is strict — score bits, ids and hits —
with no tolerance anywhere, from host arrays and from CUDA tensors.

`rrf_fuse` alone runs on random lists (many exact ties, the whole id range, holes, c = 0 / 60 / 1e6, weights with a zero and a
negative one, a group of 256 lists, a group at exactly rrf_max_entries(), entry counts that are no power of two).  `search_rrf`
is held to the oracle applied to the library's OWN lists — `search(k = depth)`, `search_filtered`, the groups of
`search_groups(k = depth)` — on the corpora and block layouts of the fused-search test.  A layout whose largest group times the
depth exceeds rrf_max_entries() is not a legal call: for those (depth, layout) pairs the test requires the refusal instead.
Against fp64 end to end the inputs are first REQUIRED to have every adjacent fp64 gap among each sub-query's top 21 above
2e-6 (measured: the smallest is 1.6e-5), then ids, hits and score bits must equal the oracle over the fp64 rankings."""
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
from tests import rank_search_ref as K  # noqa: E402
from tests import rrf_search_ref as RR  # noqa: E402
from visrag_amd import _lib, engine  # noqa: E402
from visrag_amd.engine import HipIndex, _stream_ptr  # noqa: E402

VR_OK, VR_ERR_INVALID, VR_ERR_STATE = 0, 1, 3
f32 = np.float32


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


def _same(got, want, k=None):
    """strict: dtypes, shapes, ids, hits, score bits; k: the first k slots of a deeper oracle result"""
    sc, ids, hits = _np(*got)
    if k is not None:
        want = tuple(x[:, :k] for x in want)
    assert sc.dtype == np.float32 and ids.dtype == np.int64 and hits.dtype == np.int32
    assert sc.shape == ids.shape == hits.shape == want[1].shape
    assert np.array_equal(ids, want[1])
    assert np.array_equal(hits, want[2])
    assert np.array_equal(_u32(sc), _u32(want[0]))


def _sizes_lims(n_groups, cycle):
    return np.concatenate([[0], np.cumsum([cycle[g % len(cycle)] for g in range(n_groups)])]).astype(np.int64)


def _fuse_both(ids, lims, k, c=60.0, w=None):
    """engine.rrf_fuse from host arrays and from CUDA tensors"""
    yield engine.rrf_fuse(ids, lims, k, c, w)
    got = engine.rrf_fuse(torch.tensor(ids).cuda(), torch.tensor(lims), k, c, None if w is None else torch.tensor(w))
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in got)
    yield got


def _search_both(ix, Q, lims, k, depth, c=60.0, w=None, fog=None, documents=False):
    """HipIndex.search_rrf from host arrays and from CUDA tensors"""
    got = ix.search_rrf(Q, lims, k, depth, c, w, fog, documents)
    assert all(isinstance(x, np.ndarray) for x in got)
    yield got
    got = ix.search_rrf(torch.tensor(Q).cuda(), torch.tensor(lims), k, depth, c, w, None if fog is None else torch.tensor(fog).cuda(), documents)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in got)
    yield got


def _weights(n, seed):
    w = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    w[n // 3], w[n // 2] = 0.0, -abs(w[n // 2]) - 0.5
    return w


# --------------------------------------------------------------------------------- 1. rrf_fuse alone, random lists ---
@pytest.mark.parametrize("universe,holes", [(50, 0.0), (2 ** 31 - 1, 0.0), (50, 0.3)])
def test_rrf_fuse_on_random_lists(universe, holes):
    lims = _sizes_lims(37, (1, 2, 3, 4, 5, 6, 7, 9))
    n = int(lims[-1])
    ids = RR.random_lists(n, 10, universe, holes, seed=universe % 97)
    if universe > 50:
        ids[0, 0], ids[n - 1, 9], ids[7, 3] = 0, 2 ** 31 - 2, 2 ** 31 - 2
        assert (ids == 0).any() and (ids == 2 ** 31 - 2).sum() >= 2
    w = _weights(n, 5)
    for c in (0.0, 60.0, 1e6):
        for weights in (None, w):
            want = RR.rrf_ref(ids, lims, 100, c, weights)
            for k in (1, 10, 100):
                for got in _fuse_both(ids, lims, k, c, weights):
                    _same(got, want, k)
    if universe == 50 and holes == 0:                                    # (many exact ties: the id decides)
        sc, _, _ = RR.rrf_ref(ids, lims, 100, 60.0)
        assert any(len(np.unique(_u32(row[np.isfinite(row)]))) < np.isfinite(row).sum() for row in sc)


def test_rrf_fuse_when_fp32_scores_collide():
    """positions (1, 4) beat positions (2, 3) in fp64; at c = 1e6 the two sums are one float32 and the lower id leads"""
    lists = np.array([[9, 2, -1, -1], [-1, -1, 2, 9]], dtype=np.int64)
    for got in _fuse_both(lists, np.array([0, 2]), 3, 60.0):
        assert _np(*got)[1].tolist() == [[9, 2, -1]]
        _same(got, RR.rrf_ref(lists, [0, 2], 3, 60.0))
    for got in _fuse_both(lists, np.array([0, 2]), 3, 1e6):
        sc, ids, hits = _np(*got)
        assert ids.tolist() == [[2, 9, -1]] and hits.tolist() == [[2, 2, 0]] and _u32(sc)[0, 0] == _u32(sc)[0, 1] and np.isneginf(sc[0, 2])
        _same(got, RR.rrf_ref(lists, [0, 2], 3, 1e6))
    # the hand-worked exact tie, a duplicate inside a list, a group of empty lists
    lists = np.array([[3, 7, 9], [7, 3, 5], [5, 6, 5], [-1, -1, -1]], dtype=np.int64)
    for got in _fuse_both(lists, np.array([0, 2, 3, 4]), 4):
        assert _np(*got)[1].tolist() == [[3, 7, 5, 9], [5, 6, -1, -1], [-1, -1, -1, -1]] and _np(*got)[2].tolist() == [[2, 2, 1, 1], [2, 1, 0, 0], [0] * 4]
        _same(got, RR.rrf_ref(lists, [0, 2, 3, 4], 4))
    cube = lists[:2].reshape(1, 2, 3)                                    # lims=None: [n_groups][m][depth]
    _same(engine.rrf_fuse(cube, None, 4), RR.rrf_ref(lists[:2], [0, 2], 4))
    _same(engine.rrf_fuse(torch.tensor(cube).cuda(), None, 4), RR.rrf_ref(lists[:2], [0, 2], 4))


@pytest.mark.parametrize("m,depth,universe", [(256, 32, 3000), ("cap", 64, 40000), (7, 33, 120), (3, 21, 40), (13, 79, 5000)])
def test_rrf_fuse_on_large_and_odd_groups(m, depth, universe):
    """256 lists x 32; exactly rrf_max_entries() entries in 64 lists; entry counts that are no power of two (231, 63, 1027)"""
    cap = int(_lib.load().vr_rrf_max_entries())
    assert cap >= 8192
    if m == "cap":
        m, depth = 64, cap // 64
        assert m * depth == cap
    ids = RR.random_lists(m, depth, universe, 0.1, seed=m + depth)
    w = _weights(m, 9)
    for weights, k in ((None, 1000), (w, 100)):
        want = RR.rrf_ref(ids, [0, m], k, 60.0, weights)
        for got in _fuse_both(ids, np.array([0, m]), k, 60.0, weights):
            _same(got, want)
    # the same group between two small ones: every workgroup finds its own lists
    small = RR.random_lists(3, depth, 20, 0.0, seed=1)
    ids3 = np.concatenate([small, ids, small[::-1]])
    lims = np.array([0, 3, 3 + m, 6 + m])
    _same(engine.rrf_fuse(ids3, lims, 50), RR.rrf_ref(ids3, lims, 50))


# ------------------------------------------------------- 2. search_rrf against the oracle over the library's own lists ---
LAYOUTS = [(5000, 37, 256, [M.layout(37, (1, 2, 3, 4, 5, 6, 7, 9))]),
           (2000, 24, 2304, [M.layout(24, (1, 2, 3, 6))]),
           (3001, 300, 128, [np.array([0, 200, 300]), np.array([0, 256, 300]), M.layout(300, (1, 3, 8, 2, 64, 5))])]


@pytest.mark.parametrize("nd,nq,dim,layouts", LAYOUTS)
def test_search_rrf_is_the_oracle_over_the_librarys_own_lists(nd, nq, dim, layouts):
    C, Q = R.unit(nd, dim, 1), R.unit(nq, dim, 2)
    ix = _index(C)
    cap = ix.rrf_max_entries()
    w = _weights(nq, 3)
    for depth in (10, 100, 1000):
        lists = ix.search(Q, depth)[1]
        assert (lists >= 0).all()
        for lims in layouts:
            lims = np.asarray(lims, dtype=np.int64)
            if int(np.diff(lims).max()) * depth > cap:                   # not a legal call: refused, nothing else
                with pytest.raises(_lib.VisragHipError, match="entries"):
                    ix.search_rrf(Q, lims, 10, depth)
                continue
            for weights in (None, w):
                want = RR.rrf_ref(lists, lims, 1000, 60.0, weights)
                for k in (1, 10, 100, 1000):
                    ix.rrf_search_stats(reset=True)
                    for got in _search_both(ix, Q, lims, k, depth, 60.0, weights):
                        _same(got, want, k)
                    st = ix.rrf_search_stats()
                    assert st["groups"] == 2 * (len(lims) - 1) and st["entries"] == 2 * nq * depth
                    assert st["distinct"] == 2 * sum(len(np.unique(lists[lims[g]:lims[g + 1]])) for g in range(len(lims) - 1))
    # [n_groups][m][dim] with lims=None is the flat layout with equal groups
    m = 3
    cube = Q[: (nq // m) * m].reshape(nq // m, m, dim)
    want = RR.rrf_ref(ix.search(Q, 20)[1], np.arange(nq // m + 1) * m, 10)
    _same(ix.search_rrf(cube, None, 10, 20), want)
    _same(ix.search_rrf(torch.tensor(cube).cuda(), None, 10, 20), want)
    ix.close()


# ------------------------------------------------------------------------------------------------ 3. special groups ---
def test_special_groups():
    C, Q = R.unit(5000, 256, 1), R.unit(12, 256, 2)
    ix = _index(C)
    for c in (0.0, 60.0):
        for k, depth in ((10, 10), (10, 100), (100, 100), (26, 26), (27, 27)):
            s, i = ix.search(Q, depth)
            want_s = np.tile(np.array([f32(np.float64(1) / (np.float64(f32(c)) + np.float64(r + 1))) for r in range(k)], dtype=f32), (12, 1))
            for got in _search_both(ix, Q, np.arange(13), k, depth, c):   # a group of one: the list itself
                _same(got, (want_s, i[:, :k], np.ones((12, k), dtype=np.int32)))
    for eps in (-1.0, 0.01, float("nan")):                               # certification off / a caller's model / the default again
        ix.set_search_eps(eps)
        _same(ix.search_rrf(Q, np.arange(13), 10, 50), (np.tile(np.array([f32(1 / (60.0 + r + 1)) for r in range(10)], dtype=f32), (12, 1)),
                                                        ix.search(Q, 10)[1], np.ones((12, 10), dtype=np.int32)))
    m = 5
    rep = np.repeat(Q[:6], m, axis=0)                                    # every group: one vector m times
    one = _np(*ix.search_rrf(Q[:6], np.arange(7), 20, 40))
    for got in _search_both(ix, rep, np.arange(7) * m, 20, 40):
        sc, ids, hits = _np(*got)
        assert np.array_equal(ids, one[1]) and (hits == m).all()
        _same(got, RR.rrf_ref(np.repeat(ix.search(Q[:6], 40)[1], m, axis=0), np.arange(7) * m, 20))
    ix.close()


# ------------------------------------------------------------------------------------------------------ 4. filters ---
def test_filters():
    n = 3001
    C, Q = R.unit(n, 128, 1), R.unit(24, 128, 2)
    three = np.zeros(n, dtype=bool); three[[5, 300, 2999]] = True
    masks = np.concatenate([F.random_filters(n, (0.5, 0.01), seed=11), np.zeros((1, n), dtype=bool), three[None]])
    lims = M.layout(24, (1, 2, 3, 6))
    ng = len(lims) - 1
    ix = HipIndex(128, n)
    ix.add(C)
    with pytest.raises(_lib.VisragHipError):                             # no filters set: VR_ERR_STATE
        ix.search_rrf(Q, lims, 10, 20, filter_of_group=np.zeros(ng, dtype=np.int64))
    ix.set_filters(masks)
    w = _weights(24, 4)
    mixes = [np.full(ng, 0), np.full(ng, 1), np.full(ng, 2), np.full(ng, 3), (np.arange(ng) % 5) - 1, np.full(ng, -1)]
    for fog in mixes:                                                    # density 0.5, 0.01, 0, three rows, a per-group mix with -1, none
        fog = np.asarray(fog, dtype=np.int64)
        foq = np.repeat(fog, np.diff(lims))
        for depth in (10, 100):
            lists = ix.search_filtered(Q, depth, foq)[1]
            for weights in (None, w):
                want = RR.rrf_ref(lists, lims, 100, 60.0, weights)
                for k in (10, 100):
                    for got in _search_both(ix, Q, lims, k, depth, 60.0, weights, fog):
                        _same(got, want, k)
    got = _np(*ix.search_rrf(Q, lims, 10, 20, filter_of_group=3))
    assert np.array_equal(np.sort(got[1][:, :3], axis=1), np.tile([5, 300, 2999], (ng, 1))) and (got[1][:, 3:] == -1).all()
    assert np.array_equal(got[2][:, :3], np.tile(np.diff(lims)[:, None], (1, 3)))     # every list holds all three rows
    got = _np(*ix.search_rrf(Q, lims, 10, 20, filter_of_group=2))       # density 0: rows of tails
    assert (got[1] == -1).all() and np.isneginf(got[0]).all() and (got[2] == 0).all()
    _same(ix.search_rrf(Q, lims, 10, 20, filter_of_group=-1), _np(*ix.search_rrf(Q, lims, 10, 20)))
    with pytest.raises(ValueError):
        ix.search_rrf(Q, lims, 10, 20, filter_of_group=np.full(ng, 4))
    ix.close()


# ---------------------------------------------------------------------------------------------------- 5. documents ---
def test_documents():
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    off = R.random_offsets(5000, 6)
    lims = M.layout(37, (1, 2, 3, 4, 5, 6, 7, 9))
    masks = F.random_filters(5000, (0.5,), seed=11)
    ix = _index(C, masks)
    with pytest.raises(_lib.VisragHipError, match="grouping"):           # VR_ERR_STATE
        ix.search_rrf(Q, lims, 10, 20, documents=True)
    ix.set_groups(off)
    w = _weights(37, 6)
    for depth in (10, 100):
        docs = ix.search_groups(Q, depth)[2]
        assert (docs >= 0).all()
        for weights in (None, w):
            want = RR.rrf_ref(docs, lims, 100, 60.0, weights)
            for k in (1, 10, 100):
                for got in _search_both(ix, Q, lims, k, depth, 60.0, weights, None, True):
                    _same(got, want, k)
    fog = ((np.arange(len(lims) - 1) % 2) - 1).astype(np.int64)          # documents under filters: the document window search's groups
    docs = ix.search_groups_window(Q, 0, 50, np.repeat(fog, np.diff(lims)))[2]
    for got in _search_both(ix, Q, lims, 30, 50, 60.0, None, fog, True):
        _same(got, RR.rrf_ref(docs, lims, 30))
    ix.close()


def test_filtered_pools_of_two_blocks_leave_the_document_window_search_as_it_was():
    """600 rows in documents of about three, 300 sub-queries — the search that makes the pool runs two blocks — and a per-group mix
    of no filter, a half-density and an empty one.  The lists are search_filtered's and, with documents, search_groups_window's;
    and the nested call leaves nothing behind: the document window search from host arrays, filter ids included, returns the same
    bits after every rank fusion as before."""
    C, Q = R.unit(600, 64, 1), R.unit(300, 64, 2)
    off = R.random_offsets(600, 3)
    lims = M.layout(300, (1, 3, 8, 2, 5))
    masks = np.concatenate([F.random_filters(600, (0.5,), seed=11), np.zeros((1, 600), dtype=bool)])
    ix = _index(C, masks)
    ix.set_groups(off)
    fog = ((np.arange(len(lims) - 1) % 3) - 1).astype(np.int64)          # -1 (no filter), 0, 1 (allows nothing), ...
    foq = np.repeat(fog, np.diff(lims))
    assert (foq[256:] == 0).any() and (foq[256:] == 1).any()
    before = ix.search_groups_window(Q, 0, 20, foq)
    rows = ix.search_filtered(Q, 20, foq)[1]
    assert (before[2][foq == 1] == -1).all() and (before[2][foq != 1] >= 0).all()
    for documents, lists in ((True, before[2]), (False, rows)):
        want = RR.rrf_ref(lists, lims, 10)
        for got in _search_both(ix, Q, lims, 10, 20, 60.0, None, fog, documents):
            _same(got, want)
            after = ix.search_groups_window(Q, 0, 20, foq)
            assert all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(after, before))
    ix.close()


# ------------------------------------------------------------------------------------------- 6. other index states ---
def test_tie_tier():
    C, Q, _ = R.tie_tier()
    ix = _index(C)
    lims = np.array([0, 2, 3])
    for depth in (50, 150, 1000):                                        # 150 and 1 000 cut inside the tier of bit-identical rows
        lists = ix.search(Q, depth)[1]
        want = RR.rrf_ref(lists, lims, 1000)
        for k in (50, 1000):
            for got in _search_both(ix, Q, lims, k, depth):
                _same(got, want, k)
    ix.close()


def test_an_edited_index_answers_as_a_fresh_one():
    C, Q = R.unit(3001, 128, 1).copy(), R.unit(40, 128, 2)
    lims = M.layout(40, (3, 1, 6))
    rng = np.random.default_rng(17)
    gone = rng.choice(len(C), int(0.3 * len(C)), replace=False)
    ix = _index(C)
    ix.search_rrf(Q, lims, 10, 30)                                       # (nothing is stored: nothing to invalidate)
    new_id = ix.remove(gone)
    left = C[new_id >= 0]
    upd = rng.choice(len(left), 5, replace=False)
    fresh_rows = R.unit(5, 128, 33)
    ix.update(upd, fresh_rows)
    left[upd] = fresh_rows
    fresh = _index(left)
    for depth, k in ((30, 10), (1000, 1000)):
        got = ix.search_rrf(Q, lims, k, depth)
        _same(got, _np(*fresh.search_rrf(Q, lims, k, depth)))
        _same(got, RR.rrf_ref(fresh.search(Q, depth)[1], lims, k))
    ix.close(); fresh.close()


# ------------------------------------------------------------------------------------ 7. arguments, the raw ABI ---
def _vp(x):
    if x is None:
        return ctypes.c_void_p(None)
    return ctypes.c_void_p(x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data)


def _outs(n):
    return np.full(n, -7, dtype=np.float32), np.full(n, -7, dtype=np.int64), np.full(n, -7, dtype=np.int32)


def _raw_fuse(ids, lims, k, c=60.0, w=None, n_lists=None, n_groups=None, depth=None):
    """vr_rrf_fuse itself, host arrays -> (status, scores, ids, hits); the outputs start as -7"""
    ids, lims = np.ascontiguousarray(ids, dtype=np.int64), np.asarray(lims, dtype=np.int64)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float32)
    outs = _outs(max((len(lims) - 1) * max(k, 1), 1))
    st = _lib.load().vr_rrf_fuse(0, _vp(ids), len(ids) if n_lists is None else n_lists, ids.shape[1] if depth is None else depth, _vp(lims),
                                 len(lims) - 1 if n_groups is None else n_groups, k, c, _vp(w), _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), 0,
                                 ctypes.c_void_p(_stream_ptr(0)))
    return (st,) + outs


def _raw_search(ix, Q, lims, k, depth, c=60.0, w=None, fog=None, by_groups=0, n_sub=None, n_groups=None):
    """vr_index_search_rrf itself, host arrays -> (status, scores, ids, hits); the outputs start as -7"""
    lims = np.asarray(lims, dtype=np.int64)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float32)
    outs = _outs(max((len(lims) - 1) * max(k, 1), 1))
    st = ix.lib.vr_index_search_rrf(ix._h, _vp(Q), len(Q) if n_sub is None else n_sub, _vp(lims), len(lims) - 1 if n_groups is None else n_groups,
                                    k, depth, c, _vp(w), _vp(fog), by_groups, _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), 0,
                                    ctypes.c_void_p(_stream_ptr(ix.device)))
    return (st,) + outs


def _untouched(st, *outs, code=VR_ERR_INVALID):
    return st == code and all((o == -7).all() for o in outs)


def test_rrf_fuse_argument_checks():
    cap = int(_lib.load().vr_rrf_max_entries())
    ids = RR.random_lists(7, 10, 50, 0.1, seed=1)
    lims = [0, 3, 4, 7]
    st, sc, i, h = _raw_fuse(ids, lims, 5, 60.0, np.ones(7))
    assert st == VR_OK
    _same((sc.reshape(3, 5), i.reshape(3, 5), h.reshape(3, 5)), RR.rrf_ref(ids, lims, 5))
    for k in (0, -1, 1001):
        assert _untouched(*_raw_fuse(ids, lims, k)), k
    assert "k=1001 unsupported (1..1000)" in _lib.load().vr_last_error().decode()
    for depth in (0, -1, 1001):
        assert _untouched(*_raw_fuse(ids, lims, 5, depth=depth)), depth
    for bad in ([1, 3, 4, 7], [0, 4, 3, 7], [0, 3, 3, 7], [0, 3, 4, 6], [0, 3, 4, 8]):   # lims[0] != 0, decreasing, an empty group, the end
        assert _untouched(*_raw_fuse(ids, bad, 5)), bad
    for c in (-1.0, float("nan"), float("inf")):
        assert _untouched(*_raw_fuse(ids, lims, 5, c)), c
    for bad in (float("nan"), float("inf"), -float("inf")):
        w = np.ones(7, dtype=np.float32); w[4] = bad
        assert _untouched(*_raw_fuse(ids, lims, 5, 60.0, w)), bad
    for bad in (-2, 2 ** 31 - 1, 2 ** 40):                               # host ids lie in [-1, 2^31 - 2]
        x = ids.copy(); x[5, 2] = bad
        assert _untouched(*_raw_fuse(x, lims, 5)), bad
    assert "outside [-1, 2^31 - 2]" in _lib.load().vr_last_error().decode()
    wide = RR.random_lists(300, 2, 50, 0.0, seed=2)
    assert _untouched(*_raw_fuse(wide, [0, 257, 300], 5)), "a group of 257"
    assert "257 lists" in _lib.load().vr_last_error().decode()
    assert _raw_fuse(wide, [0, 256, 300], 5)[0] == VR_OK
    deep = RR.random_lists(17, 1000, 5000, 0.0, seed=3)                  # 17 x 1000 entries
    assert 17 * 1000 > cap and _untouched(*_raw_fuse(deep, [0, 17], 5)) and "entries" in _lib.load().vr_last_error().decode()
    assert _raw_fuse(deep[: cap // 1000], [0, cap // 1000], 5)[0] == VR_OK
    assert _untouched(*_raw_fuse(ids, lims, 5, n_groups=-1)) and _untouched(*_raw_fuse(ids, lims, 5, n_lists=-1))
    assert _untouched(*_raw_fuse(ids, [0], 5, n_lists=0), code=VR_OK)    # no group: VR_OK, nothing launched, nothing written
    assert _untouched(*_raw_fuse(ids, [0], 5), code=VR_ERR_INVALID)      # lists in no group
    lib = _lib.load()
    assert lib.vr_rrf_fuse(0, _vp(None), 7, 10, _vp(np.asarray(lims, dtype=np.int64)), 3, 5, 60.0, _vp(None), _vp(None), _vp(None), _vp(None), 0,
                           None) == VR_ERR_INVALID
    # a device id outside [0, 2^31 - 2] cannot be seen before the launch: it is an empty slot, as -1 is
    x = ids.copy(); x[5, 2], x[0, 0], x[6, 9] = 2 ** 31 - 1, -9, 2 ** 40
    y = x.copy(); y[5, 2] = y[0, 0] = y[6, 9] = -1
    _same(engine.rrf_fuse(torch.tensor(x).cuda(), lims, 20), RR.rrf_ref(y, lims, 20))
    for bad in (dict(weights=[1.0, 2.0]), dict(c=-1.0)):                 # the binding's own check; the library's through the binding
        with pytest.raises((ValueError, _lib.VisragHipError)):
            engine.rrf_fuse(ids, lims, 5, **bad)
    with pytest.raises(ValueError):
        engine.rrf_fuse(ids, None, 5)                                    # lims=None wants [n_groups][m][depth]


def test_search_rrf_argument_checks_come_before_any_launch():
    n = 600
    C, Q = R.unit(n, 64, 1), R.unit(7, 64, 2)
    masks = F.random_filters(n, (0.5, 0.1), seed=11)
    lims = [0, 3, 4, 7]
    fog = np.array([0, -1, 1], dtype=np.int32)
    zeros = {"groups": 0, "entries": 0, "distinct": 0}
    ix = HipIndex(64, n + 10)
    cap = ix.rrf_max_entries()
    # the empty index: tails, nothing is launched, nothing counted
    st, sc, ids, hits = _raw_search(ix, Q, lims, 5, 20)
    assert st == VR_OK and (ids == -1).all() and np.isneginf(sc).all() and (hits == 0).all()
    got = _np(*ix.search_rrf(torch.tensor(Q).cuda(), lims, 5, 20))
    assert (got[1] == -1).all() and np.isneginf(got[0]).all() and (got[2] == 0).all()
    assert ix.rrf_search_stats() == zeros
    assert _raw_search(ix, Q, lims, 5, 20, by_groups=1)[0] == VR_ERR_STATE
    ix.add(C)
    ix.set_filters(masks)
    st, sc, ids, hits = _raw_search(ix, Q, lims, 20, 30, 10.0, np.arange(7) - 2.0, fog)
    assert st == VR_OK
    lists = ix.search_filtered(Q, 30, np.repeat(fog, np.diff(lims)))[1]
    _same((sc.reshape(3, 20), ids.reshape(3, 20), hits.reshape(3, 20)), RR.rrf_ref(lists, lims, 20, 10.0, np.arange(7) - 2.0))
    stats = ix.rrf_search_stats()
    assert stats["groups"] == 3 and stats["entries"] == int((lists >= 0).sum())
    base_s, base_i = ix.search(Q, 10)
    base_m = _np(*ix.search_multi(Q, lims, 10, "max", fog))
    others = lambda: (ix.search_stats(), ix.filter_search_stats(), ix.range_search_stats(), ix.rank_search_stats(), ix.window_search_stats(),
                      ix.multi_search_stats(), ix.group_search_stats(), ix.group_window_search_stats())
    before = others()

    def nothing_ran(st, *outs, code=VR_ERR_INVALID):
        return _untouched(st, *outs, code=code) and ix.rrf_search_stats() == stats and others() == before

    for k in (0, -1, 1001):
        assert nothing_ran(*_raw_search(ix, Q, lims, k, 20, fog=fog)), k
    assert "k=1001 unsupported (1..1000)" in _lib.load().vr_last_error().decode()
    for depth in (0, -1, 1001):
        assert nothing_ran(*_raw_search(ix, Q, lims, 5, depth, fog=fog)), depth
    assert "depth=1001 unsupported (1..1000)" in _lib.load().vr_last_error().decode()
    for bad in ([1, 3, 4, 7], [0, 4, 3, 7], [0, 3, 3, 7], [0, 3, 4, 6], [0, 3, 4, 8]):
        assert nothing_ran(*_raw_search(ix, Q, bad, 5, 20, fog=fog)), bad
    for c in (-1.0, float("nan"), float("inf")):
        assert nothing_ran(*_raw_search(ix, Q, lims, 5, 20, c)), c
    for bad in (float("nan"), float("inf")):
        w = np.ones(7, dtype=np.float32); w[6] = bad
        assert nothing_ran(*_raw_search(ix, Q, lims, 5, 20, 60.0, w)), bad
    wide = R.unit(300, 64, 3)
    assert nothing_ran(*_raw_search(ix, wide, [0, 257, 300], 5, 2)), "a group of 257"
    assert "257 lists" in _lib.load().vr_last_error().decode()
    m_over = cap // 100 + 1                                              # m * depth one list over the cap
    assert nothing_ran(*_raw_search(ix, wide[:m_over], [0, m_over], 5, 100)) and "entries" in _lib.load().vr_last_error().decode()
    for bad in (2, -2):                                                  # a filter index out of range
        fb = np.array([0, bad, -1], dtype=np.int32)
        assert nothing_ran(*_raw_search(ix, Q, lims, 5, 20, fog=fb))
        with pytest.raises(ValueError):
            ix.search_rrf(Q, lims, 5, 20, filter_of_group=fb)
    assert "outside [-1, 2)" in _lib.load().vr_last_error().decode()
    assert nothing_ran(*_raw_search(ix, Q, lims, 5, 20, by_groups=1), code=VR_ERR_STATE)      # no grouping
    assert ix.lib.vr_index_search_rrf(ix._h, _vp(Q), 7, _vp(None), 3, 5, 20, 60.0, _vp(None), _vp(None), 0, _vp(None), _vp(None), _vp(None), 0,
                                      None) == VR_ERR_INVALID
    assert nothing_ran(*_raw_search(ix, Q, lims, 5, 20, n_groups=-1)) and nothing_ran(*_raw_search(ix, Q, lims, 5, 20, n_sub=-1))
    assert nothing_ran(*_raw_search(ix, Q, [0], 5, 20, n_sub=0), code=VR_OK)                  # no group: VR_OK, nothing launched
    with pytest.raises(ValueError):
        ix.search_rrf(Q, None, 5)                                        # lims=None wants [n_groups][m][dim]
    with pytest.raises(ValueError):
        ix.search_rrf(Q, lims, 5, weights=[1.0, 2.0])                    # one weight per sub-query
    with pytest.raises(ValueError):
        ix.search_rrf(Q, lims, 5, filter_of_group=[0, 1])                # one entry per group
    with pytest.raises(_lib.VisragHipError):
        ix.search_rrf(Q, lims, 1001)
    # afterwards the other searches return the same bits, their counters unchanged by the failed calls
    assert others() == before
    s, i = ix.search(Q, 10)
    assert np.array_equal(i, base_i) and np.array_equal(_u32(s), _u32(base_s))
    again = _np(*ix.search_multi(Q, lims, 10, "max", fog))
    assert all(np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
               for a, b in zip(again, base_m))
    # the pool counts in its own search's statistics, the fusion in its own, nothing else moves
    before = others()
    ix.search_rrf(Q, lims, 5, 20)
    after = others()
    done = lambda st: st["certified"] + st["certified_extended"] + st["flagged"] + st["uncertified"]
    assert after[1:] == before[1:] and done(after[0]) == done(before[0]) + 7
    st2 = ix.rrf_search_stats()
    assert st2["groups"] == stats["groups"] + 3 and ix.rrf_search_stats(reset=True) == st2 and ix.rrf_search_stats() == zeros
    # a filter index while no filters are set for the rows present
    ix.add(C[:10])
    assert ix.n_filters == 0
    assert _raw_search(ix, Q, lims, 5, 20, fog=fog)[0] == VR_ERR_STATE and _raw_search(ix, Q, lims, 5, 20)[0] == VR_OK
    ix.close()


# ------------------------------------------------------------------------------------------------ against fp64 ---
def test_against_fp64_end_to_end():
    rng = np.random.default_rng(0)
    C = rng.standard_normal((600, 64)).astype(np.float32)
    Q = rng.standard_normal((12, 64)).astype(np.float32)
    C /= np.linalg.norm(C, axis=1, keepdims=True)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    S = R.scores64(Q, C)
    order = np.stack([K.ranking(S[q]) for q in range(12)])
    top = np.take_along_axis(S, order[:, :21], 1)
    gap = float((top[:, :-1] - top[:, 1:]).min())
    print(f"smallest adjacent fp64 gap among the top 21: {gap:.2e}")
    assert gap > 2e-6                                                    # a condition on the inputs
    lims = np.arange(4) * 4
    want = RR.rrf_ref(order[:, :20], lims, 10)
    ix = _index(C)
    for got in _search_both(ix, Q, lims, 10, 20):
        _same(got, want)
    ix.close()


# ------------------------------------------------------------------------------------------------ host consumers ---
def test_retrieve_rrf_over_pickle_shards(tmp_path):
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
    weight = lambda qid: 0.5 + int(qid.split("part")[1]) / 4
    order, lims, topics = group_rows([topic(q) for q in qids])
    whole = _index(C)
    for depth, k, wfn in ((100, 300, None), (300, 50, weight)):
        w = None if wfn is None else [wfn(qids[i]) for i in order]
        sc, ids, _ = whole.search_rrf(Q[order], lims, k, depth, 60.0, w)
        run = retriever.retrieve_rrf(args, topic, k, depth, 60.0, wfn)
        assert list(run) == topics
        for g, t in enumerate(topics):
            live = ids[g] >= 0
            assert list(run[t]) == [names[i] for i in ids[g][live]]
            assert np.array_equal(_u32(list(run[t].values())), _u32(sc[g][live]))
    whole.close()


def test_demo_retrieve_rrf(tmp_path):
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
    want = RR.rrf_ref(ix.search(qs, 20)[1], [0, 2], 12)
    p, s, h = demo.retrieve_rrf(kb, qs, 12, None, None, index=ix, names=nm, depth=20, return_scores=True)
    assert p == [os.path.join(kb, names[i]) for i in want[1][0]] and np.array_equal(_u32(s), _u32(want[0][0])) and h == want[2][0].tolist()
    assert len(p) == 12 and len(set(p)) == 12 and h[0] >= 1
    assert demo.retrieve_rrf(kb, torch.tensor(qs), 12, None, None, index=ix, names=nm, depth=20) == p
    docs = ["deck_2.pdf", "other_7.pdf"]
    allowed = np.array([n.rsplit("_", 1)[0] in docs for n in names])
    p = demo.retrieve_rrf(kb, qs, 10, None, None, index=ix, names=nm, documents=docs, weights=[2.0, 1.0])
    lists = ix.search_filtered(qs, 6, 0)[1]                              # (the filter demo.retrieve_rrf set)
    assert set(lists.ravel().tolist()) == set(np.flatnonzero(allowed).tolist())
    assert len(p) == 6 and p == [os.path.join(kb, names[i]) for i in RR.rrf_ref(lists, [0, 2], 6, 60.0, [2.0, 1.0])[1][0]]
    assert demo.retrieve_rrf(kb, qs, 10, None, None, index=ix, names=nm, documents=["nothing.pdf"]) == []
    assert demo.retrieve_rrf(str(tmp_path / "none"), qs, 5, None, None) is None
    ix.close()
