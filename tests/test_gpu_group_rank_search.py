"""-m gpu: the document rank search (vr_index_rank_groups / vr_index_count_groups_range / vr_index_group_rank_search_stats,
csrc/search_group_rank.hip) against the library's own fp32 scores — strict, bit for bit — against the searches that stand and
against the numpy reference tests/group_rank_search_ref.py.

Strict tests (no tolerance, host arrays and CUDA tensors): the oracle is the library's own fp32 score matrix, every row of
`search_range(threshold = -4, sort=False)`, masked, group-reduced and ranked in numpy on orderable bits
(group_rank_search_ref.group_rank_ref / group_count_ref); scores, best rows, ranks and counts must equal it.  The groups
`search_groups_window` returns at offset o get ranks o + arange(k) with the same score bits and best rows, in every setting of
`set_search_eps`; with groups of one row the result IS `rank_rows` / `count_range`; tied documents rank consecutively in group
order; an edited index answers as a freshly built one.

Against fp64 (no excuse mechanism, the interval is the whole test, nothing is excluded): scores within ATOL = 1e-5 of the fp64
document score; the rank of a document of fp64 score s in [#(E > s + 6e-7), #(E >= s - 6e-7) - 1] over the present documents; the
best row's fp64 score within 6e-7 of s; an absent target gets (-inf, -1, -1).  Targets: every 7th document and the reference's top
20 per query.  The reference alone gives these intervals (tests/test_cpu_group_rank_search_ref.py pins them):

    case                                  filter density    pairs   absent   widened intervals   widest
    (5000, 37, 256), mean 7                    none          4 588       0          30              1
    (5000, 37, 256), mean 7                    0.5           4 588     296          22              1
    (3001, 300, 128), mean 3                   none         49 800       0         213              2
    (2000, 8, 2304), mean 5                    0.5             624     104           5              1
    decks 300 x 10, noise 3e-4, dim 256        none          1 008       0           2              1
    decks 300 x 10, noise 3e-4, dim 2304       none          1 008       0           3              1

Measured on an MI355X (the same for host arrays and CUDA tensors): every rank inside its interval; 2 of the 61 616 ranks differ
from the reference's own fp64 rank (0 / 0 / 2 / 0 / 0 / 0 in the table's order, inside near-ties); largest |score - fp64| 2.5e-8 /
2.7e-8 / 5.3e-8 / 6.5e-9 / 2.3e-8 / 1.0e-8.  Band documents re-scored per pair (the target among them): 29.1 / 22.2 / 27.7 / 26.7 /
9.8 / 24.8; fp32 page dots per pair: 33.4 / 24.6 / 29.5 / 33.9 / 97.8 / 248.3 — in the decks every page of a band document lies
within 2 eps of its document's maximum and is re-scored.
"""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import filter_search_ref as F  # noqa: E402
from tests import group_rank_search_ref as K  # noqa: E402
from tests import group_search_ref as R  # noqa: E402
from tests import group_window_search_ref as G  # noqa: E402
from tests import range_search_ref as X  # noqa: E402
from tests.rank_search_ref import shards_case  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.engine import HipIndex, _stream_ptr  # noqa: E402

VR_OK, VR_ERR_INVALID, VR_ERR_STATE = 0, 1, 3
CYCLE_C = (0.05, 0.07)
ZERO = {"pairs": 0, "documents": 0, "page_dots": 0}


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


def _same(got, want):
    sc, rows, rk = _np(*got)
    assert sc.dtype == np.float32 and rows.dtype == np.int64 and rk.dtype == np.int64 and sc.shape == rows.shape == rk.shape == want[2].shape
    assert np.array_equal(rk, want[2])
    assert np.array_equal(rows, want[1])
    assert np.array_equal(_u32(sc), _u32(want[0]))


def _every(nq, ng):
    return np.ascontiguousarray(np.broadcast_to(np.arange(ng, dtype=np.int64), (nq, ng)))


def _thresholds(want_scores, cols):
    """finite thresholds [nq][len(cols) + 2]: the scores of some targets (absent ones: 0) and two fixed values"""
    t = want_scores[:, cols].astype(np.float32)
    t = np.where(np.isfinite(t), t, np.float32(0))
    return np.ascontiguousarray(np.concatenate([t, np.full((len(t), 1), 0.0, np.float32), np.full((len(t), 1), -0.05, np.float32)], axis=1))


def _check_counts(ix, q_in, S32, off, mask, t, foq):
    for strict in (False, True):
        got = _np(ix.count_groups_range(q_in, t, filter_of_query=foq, strict=strict))[0]
        assert got.dtype == np.int64 and np.array_equal(got, K.group_count_ref(S32, off, mask, t, strict))


# --------------------------------------------------------------------------------- 1. every group as a target ---
@pytest.mark.parametrize("nd,nq,dim,mean", [(5000, 37, 256, 7), (5000, 37, 256, 1), (2000, 8, 2304, 5), (3001, 300, 128, 3)])
def test_every_group_ranks_as_in_the_oracle(nd, nq, dim, mean):
    C, Q = R.unit(nd, dim, 1), R.unit(nq, dim, 2)
    off = np.arange(nd + 1) if mean == 1 else R.random_offsets(nd, mean)      # mean 1: 5 000 groups, two chunks of 4 096
    ng = len(off) - 1
    assert ng == {7: 723, 1: 5000}.get(mean, ng)
    ix = _index(C, off)
    S32 = _scores(ix, Q)
    T = _every(nq, ng)
    want = K.group_rank_ref(S32, off, None, T)
    assert all(np.array_equal(np.sort(r), np.arange(ng)) for r in want[2])
    qd = torch.tensor(Q).cuda()
    t = _thresholds(want[0], [0, ng // 2, ng - 1, 4095 % ng, 4096 % ng])
    for q_in in (Q, qd):
        ix.group_rank_search_stats(reset=True)
        got = ix.rank_groups(q_in, T)
        assert all((isinstance(x, torch.Tensor) and x.is_cuda) if q_in is qd else isinstance(x, np.ndarray) for x in got)
        _same(got, want)
        st = ix.group_rank_search_stats()
        assert st["pairs"] == nq * ng and st["page_dots"] >= st["documents"] >= nq * ng
        _check_counts(ix, q_in, S32, off, None, t, None)
    print(f"every group {nd}x{nq}x{dim} mean {mean}: {st}, {st['documents'] / (nq * ng):.2f} documents and {st['page_dots'] / (nq * ng):.2f} page "
          f"dots per pair")
    one = ix.rank_groups(Q, T[:, 5])                                     # [nq]: one target per query
    _same(one, tuple(w[:, 5] for w in want))
    assert np.array_equal(ix.count_groups_range(Q, -4.0), np.full(nq, ng))                # a scalar threshold
    ix.close()


def test_flat_lims_queries_without_targets_and_a_block_without_pairs():
    C, Q = R.unit(3001, 128, 1), R.unit(300, 128, 2)                     # two blocks: queries 0..255 and 256..299
    off = R.random_offsets(3001, 3)
    ng = len(off) - 1
    ix = _index(C, off)
    S32 = _scores(ix, Q)
    rng = np.random.default_rng(4)
    for name, counts in (("mixed", rng.integers(0, 4, 300) * (np.arange(300) % 3 != 1)),
                         ("first block empty", np.where(np.arange(300) < 256, 0, 3)),
                         ("second block empty", np.where(np.arange(300) < 256, np.arange(300) % 2, 0))):
        lims = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        groups = rng.integers(0, ng, lims[-1]).astype(np.int64)
        want = [np.empty(lims[-1], dtype=d) for d in (np.float32, np.int64, np.int64)]
        for q in range(300):
            part = K.group_rank_ref(S32[q:q + 1], off, None, groups[None, lims[q]:lims[q + 1]])
            for w, p in zip(want, part):
                w[lims[q]:lims[q + 1]] = p[0]
        for q_in in (Q, torch.tensor(Q).cuda()):
            ix.group_rank_search_stats(reset=True)
            _same(ix.rank_groups(q_in, groups, lims), want)
            assert ix.group_rank_search_stats()["pairs"] == lims[-1], name
            thr = np.where(np.isfinite(want[0]), want[0], 0).astype(np.float32)
            got = _np(ix.count_groups_range(q_in, thr, lims))[0]
            ref = np.concatenate([K.group_count_ref(S32[q:q + 1], off, None, thr[None, lims[q]:lims[q + 1]])[0] for q in range(300)])
            assert np.array_equal(got, ref), name
    ix.group_rank_search_stats(reset=True)
    empty = ix.rank_groups(Q, np.zeros(0, dtype=np.int64), np.zeros(301, dtype=np.int64))             # zero pairs: nothing launched
    assert all(len(x) == 0 for x in empty) and ix.group_rank_search_stats() == ZERO
    ix.close()


def test_a_filter_on_the_queries_of_a_second_block():
    """600 rows, 257 queries (a second block of one query), a half-density and an empty filter mixed per query: the block's filter
    ids start at its first query.  Query 256 is on filter 0.  Counts and ranks, from host arrays and cuda tensors."""
    C, Q = R.unit(600, 64, 1), R.unit(257, 64, 2)
    off = R.random_offsets(600, 3)
    ng = len(off) - 1
    M = np.concatenate([F.random_filters(600, (0.5,), seed=11), np.zeros((1, 600), dtype=bool)])
    foq = (np.arange(257) % 3 - 1).astype(np.int32)                      # -1 (no filter), 0, 1 (allows nothing), ...
    assert foq[256] == 0
    ix = _index(C, off, M)
    S32 = _scores(ix, Q)
    mask = _masks_of(M, foq, 600)
    T = _every(257, ng)
    want = K.group_rank_ref(S32, off, mask, T)
    t = _thresholds(want[0], [0, ng // 2, ng - 1])
    ref = K.group_count_ref(S32, off, mask, t)
    assert 0 < ref[256, -1] < K.group_count_ref(S32, off, None, t)[256, -1] and (ref[foq == 1] == 0).all()
    for cuda in (False, True):
        q_in, f_in = (torch.tensor(Q).cuda(), torch.tensor(foq).cuda()) if cuda else (Q, foq)
        _check_counts(ix, q_in, S32, off, mask, t, f_in)
        _same(ix.rank_groups(q_in, T, filter_of_query=f_in), want)
    ix.close()


# ------------------------------------------------------------------- 2. cross-checks against the searches that stand ---
@pytest.fixture(scope="module")
def filtered():
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    off = R.random_offsets(5000, 7)
    M = np.concatenate([F.random_filters(len(C), (0.5, 0.01), seed=11), np.zeros((1, len(C)), dtype=bool)])
    ix = _index(C, off, M)
    yield ix, C, Q, off, M, _scores(ix, Q)
    ix.close()


def test_the_groups_of_a_window_get_its_ranks_scores_and_best_rows(filtered):
    ix, C, Q, off, M, S32 = filtered
    ng, k = len(off) - 1, 100
    qd = torch.tensor(Q).cuda()
    for f, nd in ((None, ng), (0, int(G.present_best(S32[:1], off, M[0])[2].sum()))):
        for o in (0, 300, nd - k):
            sc, rows, gr = ix.search_groups_window(Q, o, k, f)
            assert (gr >= 0).all()
            want = (sc, rows, np.broadcast_to(o + np.arange(k), gr.shape))
            _same(ix.rank_groups(Q, gr, filter_of_query=f), want)
            _same(ix.rank_groups(qd, gr, filter_of_query=f), want)
            # the count at the score of entry j: o + j + 1 and the later members of its tie tier; strict: the entries strictly above
            mask = None if f is None else M[f]
            ge = _np(ix.count_groups_range(qd, sc, filter_of_query=f))[0]
            gt = ix.count_groups_range(Q, sc, filter_of_query=f, strict=True)
            assert np.array_equal(ge, K.group_count_ref(S32, off, mask, sc)) and np.array_equal(gt, K.group_count_ref(S32, off, mask, sc, True))
            pos = o + np.arange(k)[None, :]
            assert (ge >= pos + 1).all() and (gt <= pos).all()
            distinct = np.concatenate([np.diff(_u32(sc).astype(np.int64), axis=1) != 0, np.ones((len(Q), 1), dtype=bool)], axis=1)
            if o + k < nd:
                distinct[:, -1] = False                                  # (the next entry is not in the window: unknown)
            assert (ge[distinct] == np.broadcast_to(pos + 1, ge.shape)[distinct]).all()


def test_ranks_of_search_groups_in_every_setting_of_set_search_eps():
    C, Q, _, _ = X.random_case(20000, 64, 2304, CYCLE_C)
    off = R.random_offsets(20000, 10)
    ix = _index(C, off)
    qd = torch.tensor(Q).cuda()
    for k in (10, 100):
        ix.set_search_eps(float("nan"))                                  # the default setting
        sc, rows, gr = ix.search_groups(Q, k)
        want = (sc, rows, np.broadcast_to(np.arange(k), gr.shape))
        for eps in (float("nan"), -1.0, 0.01):                           # the default / certification off / a caller's model
            ix.set_search_eps(eps)
            _same(ix.rank_groups(Q, gr), want)
            _same(ix.rank_groups(qd, gr), want)
            assert np.array_equal(ix.count_groups_range(Q, sc[:, -1], strict=True), (_u32(sc) != _u32(sc[:, -1:])).sum(1))
    ix.set_search_eps(float("nan"))
    ix.close()


def test_groups_of_one_row_are_rank_rows_and_count_range():
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    M = np.concatenate([F.random_filters(len(C), (0.5, 0.01), seed=11), np.zeros((1, len(C)), dtype=bool)])
    foq = (np.arange(len(Q)) % 4 - 1).astype(np.int64)
    ix = _index(C, np.arange(len(C) + 1), M)                             # 5 000 documents: the count grid has two chunks
    rng = np.random.default_rng(8)
    ids = np.concatenate([rng.integers(0, 5000, (len(Q), 60)), np.tile([0, 4095, 4096, 4999], (len(Q), 1))], axis=1).astype(np.int64)
    qd, fd = torch.tensor(Q).cuda(), torch.tensor(foq).cuda()
    for q_in, f_in in ((Q, foq), (qd, fd), (Q, None)):
        sc, rk = _np(*ix.rank_rows(q_in, ids, filter_of_query=f_in))
        gsc, grow, grk = _np(*ix.rank_groups(q_in, ids, filter_of_query=f_in))
        allowed = np.ones(ids.shape, dtype=bool) if f_in is None else np.take_along_axis(_masks_of(M, foq, len(C)), ids, 1)
        assert allowed.sum() > 0.3 * ids.size
        assert np.array_equal(_u32(gsc[allowed]), _u32(sc[allowed])) and np.array_equal(grk[allowed], rk[allowed])
        assert np.array_equal(grow[allowed], ids[allowed])
        assert np.isneginf(gsc[~allowed]).all() and (grow[~allowed] == -1).all() and (grk[~allowed] == -1).all()   # rank_rows: the would-be position
        for strict in (False, True):
            a = _np(ix.count_range(q_in, sc, filter_of_query=f_in, strict=strict))[0]
            b = _np(ix.count_groups_range(q_in, sc, filter_of_query=f_in, strict=strict))[0]
            assert np.array_equal(a, b)
    ix.close()


# ------------------------------------------------------------------------------------------- 3. group shapes ---
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
    qd = torch.tensor(Q).cuda()
    for name, off in offs.items():
        off = off.astype(np.int64)
        ix.set_groups(off)
        ng = len(off) - 1
        T = _every(len(Q), ng)
        for f in (None, 0):
            m = None if f is None else mask[0]
            want = K.group_rank_ref(S32, off, m, T)
            _same(ix.rank_groups(Q, T, filter_of_query=f), want)
            _same(ix.rank_groups(qd, T, filter_of_query=f), want)
            _check_counts(ix, Q, S32, off, m, _thresholds(want[0], [0, ng - 1, min(3, ng - 1)]), f)
        if name == "one group":
            sc, rows, rk = ix.rank_groups(Q, np.zeros(len(Q), dtype=np.int64))
            assert np.array_equal(rows, S32.argmax(1)) and (rk == 0).all() and np.array_equal(_u32(sc), _u32(S32.max(1)))
            assert np.array_equal(ix.count_groups_range(Q, sc), np.ones(len(Q))) and (ix.count_groups_range(Q, sc, strict=True) == 0).all()
    ix.close()


# ------------------------------------------------------------------------------------------------ 4. filters ---
def test_ranks_under_filters_with_absent_targets(filtered):
    ix, C, Q, off, M, S32 = filtered
    ng = len(off) - 1
    foq = (np.arange(len(Q)) % 4 - 1).astype(np.int64)                   # -1 (no filter), 0 (0.5), 1 (0.01), 2 (allows nothing), ...
    mask = _masks_of(M, foq, len(C))
    T = _every(len(Q), ng)
    want = K.group_rank_ref(S32, off, mask, T)
    absent = want[2] < 0
    assert not absent[foq == -1].any() and absent[foq == 2].all() and 0 < absent[1].sum() < 100 and 600 < absent[2].sum() < ng
    qd, fd = torch.tensor(Q).cuda(), torch.tensor(foq).cuda()
    _same(ix.rank_groups(Q, T, filter_of_query=foq), want)
    _same(ix.rank_groups(qd, T, filter_of_query=fd), want)
    sc = _np(ix.rank_groups(Q, T, filter_of_query=foq)[0])[0]
    assert np.isneginf(sc[absent]).all() and np.isfinite(sc[~absent]).all()
    t = _thresholds(want[0], [0, 100, 400, ng - 1])
    _check_counts(ix, Q, S32, off, mask, t, foq)
    _check_counts(ix, qd, S32, off, mask, t, fd)
    assert (ix.count_groups_range(Q, -4.0, filter_of_query=2) == 0).all()
    for f in (0, 1, 2):                                                  # one filter for every query; -1 / None = no filter
        _same(ix.rank_groups(Q, T, filter_of_query=f), K.group_rank_ref(S32, off, M[f], T))
    _same(ix.rank_groups(Q, T, filter_of_query=-1), ix.rank_groups(Q, T))


def test_a_filter_that_forbids_the_best_page_of_the_top_documents(filtered):
    ix, C, Q, off, M, S32 = filtered
    sc0, rows0, gr0 = ix.search_groups(Q[:1], 20)
    forbid = np.ones(len(C), dtype=bool)
    forbid[rows0[0]] = False                                             # the best page of each of query 0's top 20 documents
    ix.set_filters(forbid[None, :])
    try:
        want = K.group_rank_ref(S32[:1], off, forbid, gr0)
        for q_in in (Q[:1], torch.tensor(Q[:1]).cuda()):
            sc, rows, rk = _np(*ix.rank_groups(q_in, gr0, filter_of_query=0))
            _same((sc, rows, rk), want)
            longer = 0
            for j, g in enumerate(gr0[0]):
                pages = np.arange(off[g], off[g + 1])
                allowed = pages[forbid[pages]]
                if len(allowed) == 0:                                    # a one-page document is absent
                    assert (sc[0, j], rows[0, j], rk[0, j]) == (-np.inf, -1, -1)
                    continue
                longer += 1                                              # a longer one scores as its best ALLOWED page does: all three change
                assert rows[0, j] == allowed[np.argmax(S32[0, allowed])] != rows0[0, j] and sc[0, j] <= sc0[0, j] and rk[0, j] >= 0
            assert longer >= 10 and not np.array_equal(rk[0][rk[0] >= 0], np.arange((rk[0] >= 0).sum()))
    finally:
        ix.set_filters(M)


# --------------------------------------------------------------------------------------------------- 5. ties ---
def test_tied_documents_rank_consecutively_in_group_order():
    C, Q, _ = R.tie_tier()
    n = len(C)
    off = np.arange(0, n + 1, 5)                                          # 600 documents of five rows
    high = np.unique((7 * np.arange(100) + 3) // 5)                       # the 100 documents that hold a distinct high row
    tied = np.setdiff1d(np.arange(600), high)                             # 500 documents of five bit-identical rows: one tier
    ix = _index(C, off)
    S32 = _scores(ix, Q)
    T = _every(len(Q), 600)
    want = K.group_rank_ref(S32, off, None, T)
    assert np.array_equal(want[2][:, tied], np.tile(100 + np.arange(500), (3, 1))) and np.array_equal(want[1][:, tied], np.tile(tied * 5, (3, 1)))
    qd = torch.tensor(Q).cuda()
    for q_in in (Q, qd):
        _same(ix.rank_groups(q_in, T), want)
    tier = want[0][:, tied[0]].astype(np.float32)                        # the tier's score of every query
    assert (_u32(want[0][:, tied]) == _u32(tier)[:, None]).all()
    above = np.nextafter(tier, np.float32(np.inf))
    for q_in in (Q, qd):
        assert np.array_equal(_np(ix.count_groups_range(q_in, tier))[0], np.full(3, 600))
        assert np.array_equal(_np(ix.count_groups_range(q_in, tier, strict=True))[0], np.full(3, 100))
        assert np.array_equal(_np(ix.count_groups_range(q_in, above))[0], np.full(3, 100))
    mask = np.ones(n, dtype=bool)
    mask[tied[:250] * 5] = False                                         # the first row of half the tied documents forbidden
    ix.set_filters(mask[None, :])
    sc, rows, rk = ix.rank_groups(Q, T, filter_of_query=0)
    _same((sc, rows, rk), K.group_rank_ref(S32, off, mask, T))
    assert np.array_equal(rk[:, tied], np.tile(100 + np.arange(500), (3, 1)))            # ... they still tie, through their second row
    assert np.array_equal(rows[:, tied], np.tile(np.where(np.arange(500) < 250, tied * 5 + 1, tied * 5), (3, 1)))
    assert np.array_equal(ix.count_groups_range(Q, tier, filter_of_query=0), np.full(3, 600))
    ix.close()


def test_decks_where_every_page_of_a_band_document_is_rescored():
    """300 decks of 10 pages, noise 3e-4, dim 2304: the pages of a deck score within ~1e-3 of each other, the error model's 2 eps
    is ~7e-3, so every page of a band document — the target among them — passes the limit"""
    C, Q, off, S = G.case("decks-2304")
    ix = _index(C, off)
    S32 = _scores(ix, Q)
    T = _every(len(Q), 300)
    want = K.group_rank_ref(S32, off, None, T)
    for q_in in (Q, torch.tensor(Q).cuda()):
        ix.group_rank_search_stats(reset=True)
        _same(ix.rank_groups(q_in, T), want)
        st = ix.group_rank_search_stats()
        assert st["pairs"] == T.size and st["documents"] >= T.size and st["page_dots"] == 10 * st["documents"]
        ix.group_rank_search_stats(reset=True)
        _check_counts(ix, q_in, S32, off, None, _thresholds(want[0], [0, 150, 299]), None)
        st = ix.group_rank_search_stats()
        assert st["pairs"] == 2 * 5 * len(Q) and st["page_dots"] == 10 * st["documents"]
    ix.close()


# ------------------------------------------------------------------------------------- 6. lifecycle and errors ---
def _vp(x):
    if x is None:
        return ctypes.c_void_p(None)
    return ctypes.c_void_p(x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data)


def _raw_rank(ix, Q, lims, groups, foq=None, nq=None):
    """vr_index_rank_groups itself, host arrays -> (status, scores, rows, ranks); the outputs start as -7"""
    lims, groups = np.asarray(lims, dtype=np.int64), np.asarray(groups, dtype=np.int64)
    n = max(len(groups), 1)
    sc, rows, rk = np.full(n, -7, dtype=np.float32), np.full(n, -7, dtype=np.int64), np.full(n, -7, dtype=np.int64)
    st = ix.lib.vr_index_rank_groups(ix._h, _vp(Q), len(Q) if nq is None else nq, _vp(lims), _vp(groups), _vp(foq), _vp(sc), _vp(rows),
                                     _vp(rk), 0, ctypes.c_void_p(_stream_ptr(ix.device)))
    return st, sc, rows, rk


def _raw_count(ix, Q, lims, thr, foq=None, strict=0):
    lims, thr = np.asarray(lims, dtype=np.int64), np.asarray(thr, dtype=np.float32)
    out = np.full(max(len(thr), 1), -7, dtype=np.int64)
    st = ix.lib.vr_index_count_groups_range(ix._h, _vp(Q), len(Q), _vp(lims), _vp(thr), strict, _vp(foq), _vp(out), 0,
                                            ctypes.c_void_p(_stream_ptr(ix.device)))
    return st, out


def test_an_edited_index_answers_as_a_fresh_one():
    C, Q = R.unit(3001, 128, 1).copy(), R.unit(40, 128, 2)
    off = R.random_offsets(3001, 3)
    rng = np.random.default_rng(17)
    gone_docs = rng.choice(len(off) - 1, 300, replace=False)
    gone = np.concatenate([np.arange(off[g], off[g + 1]) for g in gone_docs] + [off[[5, 9, 700]]])     # whole documents and single pages
    ix = _index(C, off)
    ix.rank_groups(Q, np.zeros(40, dtype=np.int64))                      # (nothing is stored: nothing to invalidate)
    new_id = ix.remove(gone)
    st, sc, rows, rk = _raw_rank(ix, Q, np.arange(41), np.zeros(40))
    assert st == VR_ERR_STATE and (sc == -7).all() and (rows == -7).all() and (rk == -7).all()          # the grouping went with the removal
    assert "vr_index_set_groups" in _lib.load().vr_last_error().decode()
    assert _raw_count(ix, Q, np.arange(41), np.zeros(40))[0] == VR_ERR_STATE
    with pytest.raises(_lib.VisragHipError):
        ix.rank_groups(Q, np.zeros(40, dtype=np.int64))
    left = C[new_id >= 0]
    gid = (np.searchsorted(off, np.arange(len(C)), side="right") - 1)[new_id >= 0]
    left_off = np.concatenate([[0], np.flatnonzero(np.diff(gid)) + 1, [len(left)]]).astype(np.int64)
    ix.set_groups(left_off)
    fresh = _index(left, left_off)
    ng = len(left_off) - 1
    T = _every(40, ng)[:, ::3]
    _same(ix.rank_groups(Q, T), fresh.rank_groups(Q, T))
    upd = rng.choice(len(left), 5, replace=False)
    fresh_rows = R.unit(5, 128, 33)
    ix.update(upd, fresh_rows)                                           # no row moves: the grouping stays
    left[upd] = fresh_rows
    fresh.close()
    fresh = _index(left, left_off)
    _same(ix.rank_groups(Q, T), fresh.rank_groups(Q, T))
    _same(ix.rank_groups(Q, T), K.group_rank_ref(_scores(fresh, Q), left_off, None, T))
    t = np.full(40, 0.1, dtype=np.float32)
    assert np.array_equal(ix.count_groups_range(Q, t), fresh.count_groups_range(Q, t))
    ix.close(); fresh.close()


def test_argument_checks_come_before_any_launch():
    n = 600
    C, Q = R.unit(n, 64, 1), R.unit(4, 64, 2)
    off = R.random_offsets(n, 4)
    ng = len(off) - 1
    M = F.random_filters(n, (0.5, 0.1), seed=11)
    foq = np.array([0, 1, -1, 1], dtype=np.int32)
    lims, groups = [0, 2, 2, 3, 5], [3, ng - 1, 0, 7, 7]
    ix = HipIndex(64, n + 10)
    assert _raw_rank(ix, Q, lims, groups)[0] == VR_ERR_STATE             # the empty index has no grouping
    ix.add(C)
    assert _raw_rank(ix, Q, lims, groups)[0] == VR_ERR_STATE and _raw_count(ix, Q, lims, np.zeros(5))[0] == VR_ERR_STATE      # no grouping set
    assert ix.group_rank_search_stats() == ZERO
    ix.set_groups(off)
    st, sc, rows, rk = _raw_rank(ix, Q, lims, groups, foq)
    assert st == VR_ERR_STATE and (sc == -7).all() and (rows == -7).all() and (rk == -7).all()         # filters named but none set
    ix.set_filters(M)
    S32 = _scores(ix, Q)
    mask = _masks_of(M, foq, n)
    st, sc, rows, rk = _raw_rank(ix, Q, lims, groups, foq)
    assert st == VR_OK
    want = [np.concatenate([K.group_rank_ref(S32[q:q + 1], off, mask[q:q + 1], [groups[lims[q]:lims[q + 1]]])[i][0] for q in range(4)])
            for i in range(3)]
    _same((sc, rows, rk), want)
    thr = np.where(np.isfinite(want[0]), want[0], 0.25).astype(np.float32)
    st, cnt = _raw_count(ix, Q, lims, thr, foq, strict=1)
    assert st == VR_OK
    assert np.array_equal(cnt, np.concatenate([K.group_count_ref(S32[q:q + 1], off, mask[q:q + 1], thr[None, lims[q]:lims[q + 1]], True)[0]
                                               for q in range(4)]))
    stats = ix.group_rank_search_stats()
    assert stats["pairs"] == 10
    fl = foq.astype(np.int64)
    run_others = lambda: (ix.search(Q, 10), ix.search_groups(Q, 10), ix.search_groups_window(Q, 3, 10, fl), ix.rank_rows(Q, [5, 6, 7, 8], filter_of_query=fl))   # noqa: E731
    before = run_others()
    others = (ix.search_stats(), ix.group_search_stats(), ix.filter_search_stats(), ix.range_search_stats(), ix.rank_search_stats(),
              ix.window_search_stats(), ix.group_window_search_stats())

    def nothing_ran(st, *outs):
        return st == VR_ERR_INVALID and all((o == -7).all() for o in outs) and ix.group_rank_search_stats() == stats

    assert nothing_ran(*_raw_rank(ix, Q, [1, 2, 2, 3, 5], groups, foq))
    assert "lims[0]" in _lib.load().vr_last_error().decode()
    assert nothing_ran(*_raw_rank(ix, Q, [0, 2, 1, 3, 5], groups, foq)) and nothing_ran(*_raw_count(ix, Q, [0, 2, 1, 3, 5], thr, foq))
    for bad in (-1, ng, 1 << 40):                                        # a group id out of range
        assert nothing_ran(*_raw_rank(ix, Q, lims, [3, ng - 1, bad, 7, 7], foq)), bad
    assert "groups[2]" in _lib.load().vr_last_error().decode()
    for bad in (np.nan, np.inf, -np.inf):                                # a threshold that is not finite
        assert nothing_ran(*_raw_count(ix, Q, lims, [0.1, 0.2, bad, 0.1, 0.1], foq))
    assert "thresholds[2]" in _lib.load().vr_last_error().decode()
    for bad in (2, -2):                                                  # a host filter index out of range
        fb = np.array([0, bad, -1, 1], dtype=np.int32)
        assert nothing_ran(*_raw_rank(ix, Q, lims, groups, fb)) and nothing_ran(*_raw_count(ix, Q, lims, thr, fb))
        with pytest.raises(ValueError):
            ix.rank_groups(Q, groups, np.asarray(lims), filter_of_query=fb)
    assert nothing_ran(*_raw_rank(ix, Q, lims, groups, foq, nq=-1))
    assert ix.lib.vr_index_rank_groups(ix._h, _vp(Q), 4, _vp(np.asarray(lims, dtype=np.int64)), _vp(None), _vp(None), _vp(None), _vp(None),
                                       _vp(None), 0, None) == VR_ERR_INVALID
    st, sc, rows, rk = _raw_rank(ix, Q, [0, 0, 0, 0, 0], [])             # zero pairs: VR_OK, nothing launched, nothing written
    assert st == VR_OK and (sc == -7).all() and (rows == -7).all() and (rk == -7).all() and ix.group_rank_search_stats() == stats
    for bad_groups in ([1, 2, 3], np.zeros((3, 2))):                     # the binding's own checks
        with pytest.raises(ValueError):
            ix.rank_groups(Q, bad_groups)
    # on the device an out-of-range filter index cannot be seen before the launch: it allows nothing
    qd = torch.tensor(Q).cuda()
    fb = torch.tensor(np.array([0, 7, -1, 1], dtype=np.int32)).cuda()
    T = np.tile([3, ng - 1, 0], (4, 1)).astype(np.int64)
    o_s, o_r, o_k = torch.full((12,), -7.0).cuda(), torch.full((12,), -7, dtype=torch.int64).cuda(), torch.full((12,), -7, dtype=torch.int64).cuda()
    l3 = np.arange(5, dtype=np.int64) * 3
    st = ix.lib.vr_index_rank_groups(ix._h, _vp(qd), 4, _vp(l3), _vp(T), _vp(fb), _vp(o_s), _vp(o_r), _vp(o_k), 1,
                                     ctypes.c_void_p(_stream_ptr(ix.device)))
    torch.cuda.synchronize()
    want = [w.copy() for w in _np(*ix.rank_groups(Q, T, filter_of_query=np.array([0, 0, -1, 1])))]
    want[0][1], want[1][1], want[2][1] = -np.inf, -1, -1
    assert st == VR_OK
    _same((o_s.reshape(4, 3), o_r.reshape(4, 3), o_k.reshape(4, 3)), want)
    o_c = torch.full((12,), -7, dtype=torch.int64).cuda()
    st = ix.lib.vr_index_count_groups_range(ix._h, _vp(qd), 4, _vp(l3), _vp(np.full(12, -4.0, dtype=np.float32)), 0, _vp(fb), _vp(o_c), 1,
                                            ctypes.c_void_p(_stream_ptr(ix.device)))
    torch.cuda.synchronize()
    cnt = o_c.cpu().numpy().reshape(4, 3)
    assert st == VR_OK and (cnt[1] == 0).all() and (cnt[2] == ng).all() and (0 < cnt[0]).all() and (cnt[0] <= ng).all()
    # no other search's state or counters were touched, and they answer with the same bits
    assert (ix.search_stats(), ix.group_search_stats(), ix.filter_search_stats(), ix.range_search_stats(), ix.rank_search_stats(),
            ix.window_search_stats(), ix.group_window_search_stats()) == others
    for a, b in zip(before, run_others()):
        assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
                   for x, y in zip(a, b))
    st2 = ix.group_rank_search_stats()
    assert ix.group_rank_search_stats(reset=True) == st2 and ix.group_rank_search_stats() == ZERO
    # rows appended: grouping and filters are gone with them
    ix.add(C[:10])
    assert ix.n_groups == 0 and _raw_rank(ix, Q, lims, groups)[0] == VR_ERR_STATE
    ix.close()


# ------------------------------------------------------------------------------------------------ against fp64 ---
@pytest.mark.parametrize("name", list(K.TABLE))
def test_ranks_and_scores_against_fp64(name):
    C, Q, off, S = G.case(name)
    ix = _index(C, off)
    for density, (want_pairs, want_absent, _, _) in K.TABLE[name]:
        mask = G.case_mask(name, density)
        if mask is not None:
            ix.set_filters(mask[None, :])
        T = K.targets(S, off, mask)
        first = None
        for q_in in (Q, torch.tensor(Q).cuda()):
            ix.group_rank_search_stats(reset=True)
            sc, rows, rk = _np(*ix.rank_groups(q_in, T, filter_of_query=None if mask is None else 0))
            st = ix.group_rank_search_stats()
            pairs, differ, err, bad = K.check_ranks(S, off, mask, T, sc, rows, rk)
            print(f"{name} density {density}: {pairs} pairs, {int((rk < 0).sum())} absent, {differ} ranks differ from the fp64 rank, max |score - "
                  f"fp64| {err:.2e}, {st['documents'] / pairs:.2f} band documents and {st['page_dots'] / pairs:.2f} page dots per pair")
            assert pairs == want_pairs and int((rk < 0).sum()) == want_absent
            assert err <= K.ATOL
            assert bad is None, bad                                      # (query, document, score, best row, rank)
            if first is None:
                first = (_u32(sc).tolist(), rows.tolist(), rk.tolist())
            assert (_u32(sc).tolist(), rows.tolist(), rk.tolist()) == first              # host and device callers: the same bits
    ix.close()


# ------------------------------------------------------------------------------------------------ host consumers ---
def test_rank_documents_over_pickle_shards(tmp_path):
    from visrag_amd import retriever
    from visrag_amd.documents import never_retrieved, recall_at
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
    T = np.stack([(np.arange(12) * 71 + 13 * qi) % len(docs) for qi in range(len(qids))]).astype(np.int64)
    qrels = {q: [docs[g] for g in T[qi]] for qi, q in enumerate(qids) if qi != 4}
    for labelled, m in ((False, None), (True, mask)):
        got = retriever.rank_documents(args, qrels, doc_of, *((label_of_doc, lambda q: wanted[q]) if labelled else ()))
        want = K.group_rank_ref(S32, off, m, T)
        assert got["q4"] == {}
        for qi, q in enumerate(qids):
            if qi == 4:
                continue
            assert list(got[q]) == qrels[q]
            sc, pg, rk = zip(*got[q].values())
            assert np.array_equal(_u32(sc), _u32(want[0][qi])) and list(rk) == want[2][qi].tolist()
            assert list(pg) == [names[r] if r >= 0 else None for r in want[1][qi]]
    assert any(r[2] == -1 for r in got["q1"].values())
    flat = never_retrieved([r[2] for q in qids for r in got[q].values()])
    lims = np.concatenate([[0], np.cumsum([len(got[q]) for q in qids])])
    assert 0.0 < recall_at(flat, lims, [len(docs)])[0] < 1.0             # the absent positives count as misses at every k


def test_demo_explain_documents(tmp_path):
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
    p46, s46 = demo.retrieve_documents(kb, qvec, 46, None, None, index=ix, names=nm, return_scores=True)
    out = demo.explain_documents(kb, qvec, [doc(p) for p in p46], index=ix, names=nm)
    assert [r for _, _, r in out] == list(range(46)) and [os.path.join(kb, p) for _, p, _ in out] == p46
    assert np.array_equal(_u32([s for s, _, _ in out]), _u32(s46))
    docs = ["deck_2.pdf", "other_7.pdf", "deck_4.pdf"]
    only, so = demo.retrieve_documents(kb, qvec, 10, None, None, index=ix, names=nm, documents=docs, return_scores=True)
    got = demo.explain_documents(kb, qvec, docs + ["deck_0.pdf"], documents=docs, index=ix, names=nm)
    assert got[3] == (-np.inf, None, -1)
    by_rank = sorted(got[:3], key=lambda t: t[2])
    assert [t[2] for t in by_rank] == [0, 1, 2] and [os.path.join(kb, t[1]) for t in by_rank] == only
    assert np.array_equal(_u32([t[0] for t in by_rank]), _u32(so))
    with pytest.raises(ValueError):
        demo.explain_documents(kb, qvec, ["nowhere.pdf"], index=ix, names=nm)
    ix.close()
    assert demo.explain_documents(kb, qvec, "deck_4.pdf", documents=docs) == got[2]      # an index of its own, one name: one triple
