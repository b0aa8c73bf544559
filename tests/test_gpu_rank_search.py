"""-m gpu: the rank search (vr_index_rank_rows / vr_index_count_range / vr_index_rank_search_stats, csrc/search_rank.hip) against
the library's own searches — strict, bit for bit — and against the numpy reference tests/rank_search_ref.py.

Strict tests (no tolerance): a row's rank IS its position in `search_range(threshold = -4, sort=True)`, in `search(k)` and in
`search_filtered(k)`, with the score bits those return; a count IS the size of `search_range`'s segment; bit-identical rows
rank consecutively in id order; 66 560 pairs in one query block equal the same pairs asked in four calls; per-shard counts add up
to the rank over the whole corpus; an edited index answers as a freshly built one.

Against fp64 (no excuse mechanism, the interval is the whole test): scores within the project's ATOL = 1e-5; the rank of a target
of fp64 score s lies in [#(S > s + 6e-7), #(S >= s - 6e-7) - 1] — 6e-7 is twice the project's NEAR_TIE = 3e-7, because two fp32
scores are compared and each lies inside that standing bar.  Targets of query q: the three best rows of the reference and rows
(q 7919 + j 104729 + 1) mod nd, j = 0..7.  The reference alone gives these intervals (tests/test_cpu_rank_search_ref.py pins
them, so this test cannot grow loose unnoticed; no interval is wider than 3):

    case                  pairs   widened intervals   share    summed width   max width   summed width at 3e-7
    (5000, 37, 256)         406           5           1.2 %          5            1               3
    (3001, 300, 128)      3 299          32           1.0 %         32            1              17
    (20000, 64, 2304)       704         147          20.9 %        174            3              90
    families, dim 64         88           3                          3            1               1
    families, dim 2304       88          14                         14            1              10
    norms (4000, 20, 256)   220           3                          3            1               0

Measured on an MI355X (the same for host arrays and CUDA tensors): every rank inside its interval, and 0 of the 4 805 ranks differ
from the reference's own fp64 rank; largest |score - fp64| 2.3e-8 / 4.2e-8 / 9.0e-9 / 7.9e-8 / 6.4e-8 / 7.0e-8 in the table's
order.  Band candidates re-scored per pair when every row is a target: 165.6 at (5000, 37, 256), 201.6 at (2000, 8, 2304).
"""
import ctypes
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import filter_search_ref as F  # noqa: E402
from tests import group_search_ref as R  # noqa: E402
from tests import range_search_ref as X  # noqa: E402
from tests import rank_search_ref as K  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.documents import mrr_from_ranks, recall_at  # noqa: E402
from visrag_amd.engine import HipIndex, _stream_ptr  # noqa: E402

ATOL = 1e-5
VR_OK, VR_ERR_INVALID, VR_ERR_STATE = 0, 1, 3
CYCLE_A, CYCLE_B, CYCLE_C = (0.10, 0.15, 0.20, 0.30), (0.15, 0.25, 0.05), (0.05, 0.07)


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


def _whole_ranking(ix, Q):
    """-> (ids [nq][n] in ranking order, scores [nq][n]) from the range search: every row, score descending then id ascending"""
    n = len(ix)
    lims, sc, ids = ix.search_range(Q, -4.0, sort=True)
    assert np.array_equal(lims, np.arange(len(Q) + 1) * n)
    return ids.reshape(len(Q), n), sc.reshape(len(Q), n)


# ------------------------------------------------------------------------------------------ 1. the whole ranking ---
@pytest.mark.parametrize("nd,nq,dim", [(5000, 37, 256), (2000, 8, 2304)])
def test_every_row_ranks_where_the_range_search_puts_it(nd, nq, dim):
    C, Q = R.unit(nd, dim, 1), R.unit(nq, dim, 2)
    ix = _index(C)
    order, osc = _whole_ranking(ix, Q)
    want_rank = np.stack([K.ranks_of_ranking(o) for o in order])
    want_bits = np.empty((nq, nd), dtype=np.uint32)
    np.put_along_axis(want_bits, order, _u32(osc), 1)
    every = np.tile(np.arange(nd, dtype=np.int64), (nq, 1))
    for cuda in (False, True):
        ix.rank_search_stats(reset=True)
        q_in = torch.tensor(Q).cuda() if cuda else Q
        got = ix.rank_rows(q_in, every)
        assert all((isinstance(x, torch.Tensor) and x.is_cuda) if cuda else isinstance(x, np.ndarray) for x in got)
        sc, rk = _np(*got)
        assert sc.dtype == np.float32 and rk.dtype == np.int64 and sc.shape == rk.shape == (nq, nd)
        assert np.array_equal(rk, want_rank)
        assert np.array_equal(_u32(sc), want_bits)
        st = ix.rank_search_stats()
        assert st["pairs"] == nq * nd and st["candidates"] >= st["pairs"] and st["counted"] == int(want_rank.sum())
        print(f"whole ranking {nd}x{nq}x{dim} cuda={cuda}: {st}, {st['candidates'] / st['pairs']:.1f} candidates per pair")
    # flat with lims, and one target per query: the same numbers
    lims = np.arange(nq + 1, dtype=np.int64) * 3
    sc3, rk3 = ix.rank_rows(Q, every[:, 5:8].reshape(-1), lims)
    assert sc3.shape == rk3.shape == (3 * nq,) and np.array_equal(rk3.reshape(nq, 3), want_rank[:, 5:8])
    sc1, rk1 = ix.rank_rows(Q, order[:, 7])
    assert rk1.shape == (nq,) and (rk1 == 7).all() and np.array_equal(_u32(sc1), _u32(osc[:, 7]))
    ix.close()


# --------------------------------------------------------------------------------------- 2. agreement with top-k ---
def test_the_rows_of_search_have_ranks_0_to_k():
    C, Q, _, _ = X.random_case(20000, 64, 2304, CYCLE_C)
    ix = _index(C)
    for k in (10, 100, 1000):
        s, i = ix.search(Q, k)
        for q_in in (Q, torch.tensor(Q).cuda()):
            sc, rk = _np(*ix.rank_rows(q_in, i))
            assert np.array_equal(rk, np.tile(np.arange(k), (len(Q), 1))), k
            assert np.array_equal(_u32(sc), _u32(s)), k
    sc, rk = ix.rank_rows(Q, np.concatenate([i[:, :3], i[:, :3]], axis=1))     # duplicate targets
    assert np.array_equal(rk, np.tile([0, 1, 2, 0, 1, 2], (len(Q), 1)))
    ix.close()


# ---------------------------------------------------------------------------------- 3. agreement under a filter ---
def test_ranks_under_a_filter():
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    M = F.random_filters(len(C), (0.5, 0.01), seed=11)
    foq = (np.arange(len(Q)) % 3 - 1).astype(np.int64)                   # -1 (no filter), 0, 1, ...
    ix = _index(C, M)
    k = 20
    assert M[1].sum() >= k
    s, i = ix.search_filtered(Q, k, foq)
    assert (i >= 0).all()
    for q_in, f_in in ((Q, foq), (torch.tensor(Q).cuda(), torch.tensor(foq).cuda())):
        sc, rk = _np(*ix.rank_rows(q_in, i, filter_of_query=f_in))
        assert np.array_equal(rk, np.tile(np.arange(k), (len(Q), 1))) and np.array_equal(_u32(sc), _u32(s))
    # every row, allowed or not: the allowed rows ahead of it in the unfiltered ranking; the score does not depend on the filter
    order, osc = _whole_ranking(ix, Q)
    nd = len(C)
    want = np.empty((len(Q), nd), dtype=np.int64)
    for q in range(len(Q)):
        allowed = np.ones(nd, dtype=bool) if foq[q] < 0 else M[foq[q]]
        a = allowed[order[q]].astype(np.int64)
        want[q, order[q]] = np.cumsum(a) - a
    every = np.tile(np.arange(nd, dtype=np.int64), (len(Q), 1))
    sc, rk = ix.rank_rows(Q, every, filter_of_query=foq)
    assert np.array_equal(rk, want)
    plain = ix.rank_rows(Q, every)
    assert np.array_equal(_u32(sc), _u32(plain[0])) and np.array_equal(plain[1][foq < 0], rk[foq < 0])
    forbidden = ~M[1][every[2]]                                          # query 2 is on filter 1 (1 % of the rows)
    assert foq[2] == 1 and forbidden.sum() > 4000 and rk[2].max() <= M[1].sum()
    ix.close()


def test_two_query_blocks_under_filters():
    """600 rows (three 256-row tiles, the last partial), 257 queries (a second block of one query), a half-density and an empty
    filter: the block's pairs and filters start at its first query.  Ranks against the fp64 reference inside the interval bar
    of the module docstring, counts equal to the range search's segments; query 256 is on filter 0."""
    C, Q, t, S = X.random_case(600, 257, 64, CYCLE_B)
    M = np.concatenate([F.random_filters(600, (0.5,), seed=11), np.zeros((1, 600), dtype=bool)])
    foq = (np.arange(257) % 3 - 1).astype(np.int64)                      # -1 (no filter), 0, 1 (allows nothing), ...
    assert foq[256] == 0
    T = np.tile(np.arange(0, 600, 120, dtype=np.int64), (257, 1))        # five targets per query
    ix = _index(C, M)
    first = None
    for q_in, f_in in ((Q, foq), (torch.tensor(Q).cuda(), torch.tensor(foq).cuda())):
        sc, rk = _np(*ix.rank_rows(q_in, T, filter_of_query=f_in))
        np.testing.assert_allclose(sc, np.take_along_axis(S, T, 1), atol=ATOL, rtol=0)
        for q in range(257):
            Sq = S[q] if foq[q] < 0 else S[q][M[foq[q]]]
            for i, r in zip(T[q], rk[q]):
                lo, hi = K.interval(Sq, S[q, i])
                hi += 0 if foq[q] < 0 or M[foq[q]][i] else 1             # (a forbidden target is not among the rows counted)
                assert lo <= r <= hi, (q, i, r, lo, hi)
        assert (rk[foq == 1] == 0).all()
        first = first or (_u32(sc).tolist(), rk.tolist())
        assert (_u32(sc).tolist(), rk.tolist()) == first                 # host and device callers: the same bits
    want = _counts_equal_range(ix, Q, t, foq)
    assert want[256] > 0 and (want[foq == 1] == 0).all()
    ix.close()


# ------------------------------------------------------------------------------------------------ 4. tie tier ---
def test_tie_tier():
    C, Q, _ = R.tie_tier()
    n, high = len(C), 7 * np.arange(100) + 3
    tied = np.setdiff1d(np.arange(n), high)
    ix = _index(C)
    s, i = ix.search(Q, 150)
    assert np.isin(i[:, :100], high).all() and not np.isin(i[:, 100], high).any()
    t = s[:, 100].copy()
    every = np.tile(np.arange(n, dtype=np.int64), (3, 1))
    for q_in in (Q, torch.tensor(Q).cuda()):
        sc, rk = _np(*ix.rank_rows(q_in, every))
        assert np.array_equal(rk[:, tied], np.tile(100 + np.arange(n - 100), (3, 1)))      # consecutive, in id order
        assert (_u32(sc[:, tied]) == _u32(t)[:, None]).all()
        assert np.array_equal(np.take_along_axis(rk, i[:, :100], 1), np.tile(np.arange(100), (3, 1)))
        assert _np(ix.count_range(q_in, t))[0].tolist() == [n] * 3
        assert _np(ix.count_range(q_in, np.nextafter(t, np.float32(2))))[0].tolist() == [100] * 3
        assert _np(ix.count_range(q_in, t, strict=True))[0].tolist() == [100] * 3
    ix.close()


# -------------------------------------------------------------------------- 5. counts against the range search ---
def _counts_equal_range(ix, Q, t, foq=None):
    want = np.diff(ix.search_range(Q, t, foq, sort=False)[0])
    for q_in in (Q, torch.tensor(Q).cuda()):
        got = ix.count_range(q_in, t, filter_of_query=foq)
        assert (isinstance(got, torch.Tensor) and got.is_cuda) if isinstance(q_in, torch.Tensor) else isinstance(got, np.ndarray)
        got = _np(got)[0]
        assert got.dtype == np.int64 and got.shape == (len(Q),) and np.array_equal(got, want)
    return want


@pytest.mark.parametrize("nd,nq,dim,cycle", [(5000, 37, 256, CYCLE_A), (3001, 300, 128, CYCLE_B), (20000, 64, 2304, CYCLE_C)])
def test_counts_equal_the_range_search_random_unit_rows(nd, nq, dim, cycle):
    C, Q, t, S = X.random_case(nd, nq, dim, cycle)
    ix = _index(C)
    want = _counts_equal_range(ix, Q, t)
    assert want.sum() > 0
    # [nq][4] thresholds = four scalar calls; strict counts never exceed the others
    T = np.stack([np.full(nq, c, dtype=np.float32) for c in (cycle + cycle)[:4]], axis=1)
    got = ix.count_range(Q, T)
    assert got.shape == (nq, 4)
    for j in range(4):
        assert np.array_equal(got[:, j], ix.count_range(Q, float(T[0, j])))
        assert np.array_equal(got[:, j], np.diff(ix.search_range(Q, float(T[0, j]), sort=False)[0]))
    assert (ix.count_range(Q, T, strict=True) <= got).all()
    flat = ix.count_range(Q, T.reshape(-1), np.arange(nq + 1, dtype=np.int64) * 4)
    assert np.array_equal(flat, got.reshape(-1))
    ix.close()


@pytest.mark.parametrize("dim", [64, 2304])
def test_counts_equal_the_range_search_families(dim):
    C, Q, S = X.families(dim)
    ix = _index(C)
    assert _counts_equal_range(ix, Q, 0.9).tolist() == [1500] * 8
    _counts_equal_range(ix, Q, X.FAMILY_MEDIAN[dim])
    ix.close()


def test_counts_equal_the_range_search_norms_and_filters():
    C, Q, S = X.scaled_norms()
    ix = _index(C)
    for t in (0.2, 0.4):
        _counts_equal_range(ix, Q, t)
    ix.close()
    C, Q, t, S = X.random_case(5000, 37, 256, CYCLE_A)
    M = F.random_filters(len(C), (0.5, 0.05, 0.002), seed=11)
    foq = (np.arange(len(Q)) % 4 - 1).astype(np.int64)
    ix = _index(C, M)
    want = _counts_equal_range(ix, Q, t, foq)
    assert (want[foq == 2] == 0).all() and (want[foq == 0] > 0).any()
    # everything, nothing, and -0.0 as +0.0
    assert ix.count_range(Q, -4.0).tolist() == [len(C)] * len(Q) and ix.count_range(Q, 4.0).tolist() == [0] * len(Q)
    assert ix.count_range(Q, -4.0, filter_of_query=foq).tolist() == [len(C) if f < 0 else int(M[f].sum()) for f in foq]
    assert np.array_equal(ix.count_range(Q, -0.0), ix.count_range(Q, 0.0))
    assert np.array_equal(ix.count_range(Q, -0.0, strict=True), ix.count_range(Q, 0.0, strict=True))
    # certification off: the default error model defines the band, the answer stays the fp32 answer
    targets = np.tile(np.arange(0, 5000, 97, dtype=np.int64), (len(Q), 1))
    before = ix.rank_rows(Q, targets, filter_of_query=foq)
    ix.set_search_eps(-1.0)
    after = ix.rank_rows(Q, targets, filter_of_query=foq)
    assert np.array_equal(before[1], after[1]) and np.array_equal(_u32(before[0]), _u32(after[0]))
    assert np.array_equal(ix.count_range(Q, t, filter_of_query=foq), want)
    ix.close()


# -------------------------------------------------------------------------------------------- 6. launch split ---
def test_more_pairs_in_a_query_block_than_a_grid_dimension_holds():
    """66 560 pairs in the first block of 256 queries: the smallest count past 65 535"""
    C, Q, _, _ = X.random_case(3001, 300, 128, CYCLE_B)
    ix = _index(C)
    rng = np.random.default_rng(5)
    T = rng.integers(0, len(C), size=(256, 260)).astype(np.int64)
    lims = np.concatenate([np.arange(257, dtype=np.int64) * 260, np.full(44, 256 * 260, dtype=np.int64)])
    assert len(lims) == 301 and lims[-1] == 66560
    ix.rank_search_stats(reset=True)
    sc, rk = ix.rank_rows(Q, T.reshape(-1), lims)
    assert ix.rank_search_stats()["pairs"] == 66560
    for j in range(4):
        s4, r4 = ix.rank_rows(Q[:256], T[:, 65 * j:65 * (j + 1)])
        assert np.array_equal(rk.reshape(256, 260)[:, 65 * j:65 * (j + 1)], r4)
        assert np.array_equal(_u32(sc.reshape(256, 260)[:, 65 * j:65 * (j + 1)]), _u32(s4))
    order, _ = _whole_ranking(ix, Q[:256])
    want = np.stack([K.ranks_of_ranking(o) for o in order])
    assert np.array_equal(rk.reshape(256, 260), np.take_along_axis(want, T, 1))
    ix.close()


# -------------------------------------------------------------------------------------------------- 7. shards ---
def _shard_targets(nq, bounds):
    """per query: the 50 rows of shard 0 and their bit-for-bit copies in shard 2, and 30 more rows over all shards"""
    src, dst = np.arange(50) * 17 + 5, 4001 + np.arange(50) * 31 + 2
    rng = np.random.default_rng(9)
    rest = np.setdiff1d(np.arange(bounds[-1]), np.concatenate([src, dst]))
    return np.stack([np.concatenate([src, dst, rng.choice(rest, 30, replace=False)]) for _ in range(nq)]).astype(np.int64)


def test_per_shard_counts_add_up_to_the_global_rank():
    C, Q, bounds = K.shards_case()
    T = _shard_targets(len(Q), bounds)
    whole = _index(C)
    want_sc, want_rk = whole.rank_rows(Q, T)
    whole.close()
    assert (np.diff(np.sort(want_rk, axis=1), axis=1) > 0).all()         # equal rows across shards still rank apart
    shards = [_index(C[bounds[s]:bounds[s + 1]]) for s in range(3)]
    home = np.searchsorted(bounds, T, side="right") - 1
    sc, rk = np.zeros(T.shape, dtype=np.float32), np.zeros(T.shape, dtype=np.int64)
    nq = len(Q)
    for s, ix in enumerate(shards):                                      # the target's shard: its score, its rank in the shard
        here = home == s
        lims = np.concatenate([[0], np.cumsum(here.sum(1))]).astype(np.int64)
        sc[here], rk[here] = ix.rank_rows(Q, (T - bounds[s])[here], lims)
    for s, ix in enumerate(shards):                                      # earlier shards: >= the score; later shards: > it
        for strict, there in ((False, home > s), (True, home < s)):
            lims = np.concatenate([[0], np.cumsum(there.sum(1))]).astype(np.int64)
            rk[there] += ix.count_range(Q, sc[there], lims, strict=strict)
        ix.close()
    assert np.array_equal(rk, want_rk) and np.array_equal(_u32(sc), _u32(want_sc))
    src = slice(0, 50)
    assert (rk[:, 50:100] > rk[:, src]).all() and np.array_equal(_u32(sc[:, 50:100]), _u32(sc[:, src]))


def test_retriever_rank_rows_over_pickle_shards(tmp_path):
    from visrag_amd import retriever
    from visrag_amd.utils import write_shard
    C, Q, bounds = K.shards_case()
    T = _shard_targets(len(Q), bounds)
    names = [f"page_{i}" for i in range(len(C))]
    for s in range(3):
        write_shard(str(tmp_path / f"embeddings.corpus.rank.{s}"), C[bounds[s]:bounds[s + 1]], names[bounds[s]:bounds[s + 1]])
    qids = [f"q{q}" for q in range(len(Q))]
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, qids)
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    wanted = {q: [names[i] for i in T[qi]] for qi, q in enumerate(qids)}
    wanted["q3"] = []
    got = retriever.rank_rows(args, wanted)
    whole = _index(C)
    sc, rk = whole.rank_rows(Q, T)
    whole.close()
    for qi, q in enumerate(qids):
        if q == "q3":
            assert got[q] == {}
            continue
        assert list(got[q]) == wanted[q]
        assert [got[q][d][1] for d in wanted[q]] == rk[qi].tolist()
        assert np.array_equal(_u32([got[q][d][0] for d in wanted[q]]), _u32(sc[qi]))
    assert retriever.rank_rows(args, lambda q: wanted[q][:2]) == {q: dict(list(got[q].items())[:2]) for q in qids}
    with pytest.raises(ValueError):
        retriever.rank_rows(args, {"q0": ["no_such_page"]})


# --------------------------------------------------------------------------------------------------- 8. edits ---
def test_an_edited_index_answers_as_a_fresh_one():
    C, Q = R.unit(3001, 128, 1).copy(), R.unit(40, 128, 2)
    rng = np.random.default_rng(17)
    gone = rng.choice(len(C), int(0.3 * len(C)), replace=False)
    ix = _index(C)
    ix.rank_rows(Q, np.zeros(len(Q), dtype=np.int64))                    # (nothing is stored: nothing to invalidate)
    new_id = ix.remove(gone)
    left = C[new_id >= 0]
    upd = rng.choice(len(left), 5, replace=False)
    fresh_rows = R.unit(5, 128, 33)
    ix.update(upd, fresh_rows)
    left[upd] = fresh_rows
    fresh = _index(left)
    T = np.concatenate([np.tile(upd, (len(Q), 1)), rng.integers(0, len(left), size=(len(Q), 40))], axis=1).astype(np.int64)
    thr = np.asarray(CYCLE_B, dtype=np.float32)[np.arange(len(Q)) % 3]
    a, b = ix.rank_rows(Q, T), fresh.rank_rows(Q, T)
    assert np.array_equal(a[1], b[1]) and np.array_equal(_u32(a[0]), _u32(b[0]))
    for strict in (False, True):
        assert np.array_equal(ix.count_range(Q, thr, strict=strict), fresh.count_range(Q, thr, strict=strict))
    assert np.array_equal(ix.count_range(Q, thr), np.diff(ix.search_range(Q, thr)[0]))
    ix.close(); fresh.close()


# ------------------------------------------------------------------------------------------------- 9. metrics ---
def test_metrics_from_ranks():
    from visrag_amd.utils import eval_mrr
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    ix = _index(C)
    s31, i31 = ix.search(Q, 31)
    s10, i10 = ix.search(Q, 10)
    rng = np.random.default_rng(4)
    drawn = [np.sort(rng.choice(31, rng.integers(1, 4), replace=False)) for _ in range(len(Q))]    # one to three positives, ranks 0..30
    lims = np.concatenate([[0], np.cumsum([len(d) for d in drawn])]).astype(np.int64)
    positives = np.concatenate([i31[q][d] for q, d in enumerate(drawn)])
    _, ranks = ix.rank_rows(Q, positives, lims)
    ix.close()
    assert np.array_equal(ranks, np.concatenate(drawn))
    qrel = {f"q{q}": {f"d{int(i)}": 1 for i in i31[q][d]} for q, d in enumerate(drawn)}
    run = {f"q{q}": {f"d{int(i)}": float(s) for s, i in zip(s10[q], i10[q])} for q in range(len(Q))}
    assert any(d.min() >= 10 for d in drawn) and any(d.min() < 10 for d in drawn)
    assert abs(mrr_from_ranks(ranks, lims, cutoff=10) - eval_mrr(qrel, run, 10)["all"]) < 1e-12
    assert mrr_from_ranks(ranks, lims) > mrr_from_ranks(ranks, lims, cutoff=10)
    ks = [1, 10, 31]
    by_hand = [np.mean([sum(1 for r in d if r < k) / len(d) for d in drawn]) for k in ks]
    np.testing.assert_allclose(recall_at(ranks, lims, ks), by_hand, atol=1e-15, rtol=0)
    assert recall_at(ranks, lims, [31])[0] == 1.0


# ----------------------------------------------------------------------------------- 10. arguments, the raw ABI ---
def _vp(x):
    if x is None:
        return ctypes.c_void_p(None)
    return ctypes.c_void_p(x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data)


def _raw_rank(ix, Q, lims, ids, foq=None):
    """vr_index_rank_rows itself, host arrays -> (status, scores, ranks); the outputs start as -7"""
    lims, ids = np.asarray(lims, dtype=np.int64), np.asarray(ids, dtype=np.int64)
    n = max(len(ids), 1)
    sc, rk = np.full(n, -7, dtype=np.float32), np.full(n, -7, dtype=np.int64)
    st = ix.lib.vr_index_rank_rows(ix._h, _vp(Q), len(Q), _vp(lims), _vp(ids), _vp(foq), _vp(sc), _vp(rk), 0,
                                   ctypes.c_void_p(_stream_ptr(ix.device)))
    return st, sc, rk


def _raw_count(ix, Q, lims, thr, foq=None, strict=0):
    lims, thr = np.asarray(lims, dtype=np.int64), np.asarray(thr, dtype=np.float32)
    out = np.full(max(len(thr), 1), -7, dtype=np.int64)
    st = ix.lib.vr_index_count_range(ix._h, _vp(Q), len(Q), _vp(lims), _vp(thr), strict, _vp(foq), _vp(out), 0,
                                     ctypes.c_void_p(_stream_ptr(ix.device)))
    return st, out


def test_argument_checks_come_before_any_launch():
    n = 600
    C, Q = R.unit(n, 64, 1), R.unit(4, 64, 2)
    M = F.random_filters(n, (0.5, 0.1), seed=11)
    foq = np.array([0, 1, -1, 1], dtype=np.int32)
    ix = HipIndex(64, n + 10)
    # the empty index: counts are zeros, a target row cannot be in range, zero pairs are fine
    st, out = _raw_count(ix, Q, [0, 1, 2, 3, 4], [0.1] * 4)
    assert st == VR_OK and out.tolist() == [0] * 4
    assert _raw_rank(ix, Q, [0, 1, 1, 1, 1], [0])[0] == VR_ERR_INVALID
    assert _raw_rank(ix, Q, [0, 0, 0, 0, 0], [])[0] == VR_OK and _raw_count(ix, Q, [0, 0, 0, 0, 0], [])[0] == VR_OK
    assert ix.rank_search_stats() == {"pairs": 0, "candidates": 0, "counted": 0}
    ix.add(C)
    ix.set_filters(M)
    lims, ids, thr = [0, 2, 2, 3, 5], [5, 599, 0, 7, 7], [0.1, 0.2, 0.0, -0.3, 0.3]
    st, sc, rk = _raw_rank(ix, Q, lims, ids, foq)
    assert st == VR_OK
    S = R.scores64(Q, C)
    pair_q = np.repeat(np.arange(4), np.diff(lims))
    np.testing.assert_allclose(sc, S[pair_q, ids], atol=ATOL, rtol=0)
    st, cnt = _raw_count(ix, Q, lims, thr, foq)
    assert st == VR_OK and cnt.tolist() == [K.count_ref(S[q], t, mask=None if foq[q] < 0 else M[foq[q]]) for q, t in zip(pair_q, thr)]
    stats = ix.rank_search_stats()
    assert stats["pairs"] == 10
    others = (ix.search_stats(), ix.filter_search_stats(), ix.range_search_stats())

    def nothing_ran(st, *outs):
        return st == VR_ERR_INVALID and all((o == -7).all() for o in outs) and ix.rank_search_stats() == stats

    for bad in ([1, 2, 2, 3, 5], [0, 2, 1, 3, 5], [0, 2, 2, 3, -1]):     # lims[0] != 0, decreasing
        assert nothing_ran(*_raw_rank(ix, Q, bad, ids, foq)), bad
        assert nothing_ran(*_raw_count(ix, Q, bad, thr, foq)), bad
    assert "lims" in _lib.load().vr_last_error().decode()
    for bad in (-1, n, 1 << 40):                                         # ids outside [0, n)
        assert nothing_ran(*_raw_rank(ix, Q, lims, [5, 599, bad, 7, 7], foq)), bad
    assert "outside [0, 600)" in _lib.load().vr_last_error().decode()
    for bad in (np.nan, np.inf, -np.inf):
        assert nothing_ran(*_raw_count(ix, Q, lims, [0.1, 0.2, bad, -0.3, 0.3], foq)), bad
    for bad in (2, -2):                                                  # a filter index out of range
        fb = np.array([0, bad, -1, 1], dtype=np.int32)
        assert nothing_ran(*_raw_rank(ix, Q, lims, ids, fb)) and nothing_ran(*_raw_count(ix, Q, lims, thr, fb))
        with pytest.raises(ValueError):
            ix.rank_rows(Q, np.zeros(4, dtype=np.int64), filter_of_query=fb)
    assert ix.lib.vr_index_rank_rows(ix._h, _vp(Q), 4, _vp(None), _vp(None), _vp(None), _vp(None), _vp(None), 0, None) == VR_ERR_INVALID
    assert _raw_rank(ix, Q, [0, 0, 0, 0, 0], [])[0] == VR_OK and ix.rank_search_stats() == stats      # zero pairs: nothing launched
    with pytest.raises(ValueError):
        ix.rank_rows(Q, np.zeros(3, dtype=np.int64))                     # 3 targets for 4 queries, no lims
    with pytest.raises(ValueError):
        ix.count_range(Q, [0.1, 0.2], [0, 1, 1, 1, 1])                   # lims do not end at the thresholds
    with pytest.raises(_lib.VisragHipError):
        ix.rank_rows(Q, np.full(4, n, dtype=np.int64))
    # on the device an out-of-range filter index cannot be seen before the launch: that query counts nothing
    fb, qd = torch.tensor(np.array([0, 7, -1, 1], dtype=np.int32)).cuda(), torch.tensor(Q).cuda()
    out = torch.full((4,), -7, dtype=torch.int64).cuda()
    st = ix.lib.vr_index_count_range(ix._h, _vp(qd), 4, _vp(np.arange(5, dtype=np.int64)), _vp(np.full(4, -4, dtype=np.float32)), 0,
                                     _vp(fb), _vp(out), 1, ctypes.c_void_p(_stream_ptr(ix.device)))
    torch.cuda.synchronize()
    assert st == VR_OK and out.cpu().tolist() == [int(M[0].sum()), 0, n, int(M[1].sum())]
    assert (ix.search_stats(), ix.filter_search_stats(), ix.range_search_stats()) == others
    # a filter index while no filters are set for the rows present
    ix.add(C[:10])
    assert ix.n_filters == 0
    assert _raw_rank(ix, Q, lims, ids, foq)[0] == VR_ERR_STATE and _raw_count(ix, Q, lims, thr, foq)[0] == VR_ERR_STATE
    assert _raw_rank(ix, Q, lims, ids)[0] == VR_OK and _raw_count(ix, Q, lims, thr)[0] == VR_OK
    ix.close()


# -------------------------------------------------------------------------------------------------- 11. stats ---
def test_stats_count_pairs_band_candidates_and_rows():
    C, Q, t, S = X.random_case(5000, 37, 256, CYCLE_A)
    ix = _index(C)
    assert ix.rank_search_stats() == {"pairs": 0, "candidates": 0, "counted": 0}
    T = np.tile(np.arange(0, 5000, 250, dtype=np.int64), (len(Q), 1))
    _, rk = ix.rank_rows(Q, T)
    st = ix.rank_search_stats()
    assert st["pairs"] == T.size and st["candidates"] >= T.size and st["counted"] == int(rk.sum())   # a target lies in its own band
    cnt = ix.count_range(Q, t)
    st2 = ix.rank_search_stats()
    assert st2["pairs"] == T.size + len(Q) and st2["counted"] == st["counted"] + int(cnt.sum()) and st2["candidates"] >= st["candidates"]
    assert ix.rank_search_stats(reset=True) == st2 and ix.rank_search_stats() == {"pairs": 0, "candidates": 0, "counted": 0}
    ix.close()


# ------------------------------------------------------------------------------------------------ against fp64 ---
@pytest.mark.parametrize("name", list(K.TABLE))
def test_ranks_and_scores_against_fp64(name):
    C, Q, S = K.case(name)
    lims, ids = K.all_targets(S)
    pair_q = np.repeat(np.arange(len(Q)), np.diff(lims))
    ix = _index(C)
    first = None
    for q_in in (Q, torch.tensor(Q).cuda()):
        sc, rk = _np(*ix.rank_rows(q_in, ids, lims))
        moved = widest = 0
        for p, (q, i) in enumerate(zip(pair_q, ids)):
            lo, hi = K.interval(S[q], S[q, i])
            widest = max(widest, hi - lo)
            moved += int(rk[p] != K.rank_ref(S[q], i))
        print(f"{name}: {len(ids)} pairs, {moved} ranks differ from the fp64 rank, widest interval {widest}, "
              f"max |score - fp64| {np.abs(sc - S[pair_q, ids]).max():.2e}")
        np.testing.assert_allclose(sc, S[pair_q, ids], atol=ATOL, rtol=0)
        assert widest <= 3
        for p, (q, i) in enumerate(zip(pair_q, ids)):
            lo, hi = K.interval(S[q], S[q, i])
            assert lo <= rk[p] <= hi, (q, i, int(rk[p]), lo, hi)
        if first is None:
            first = (_u32(sc).tolist(), rk.tolist())
        assert (_u32(sc).tolist(), rk.tolist()) == first                 # host and device callers: the same bits
    ix.close()


# ------------------------------------------------------------------------------------------------ host consumer ---
def test_demo_explain(tmp_path):
    import os
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
    paths, scores = demo.retrieve(kb, qvec, 70, None, None, index=ix, names=nm, documents=[n.rsplit("_", 1)[0] for n in names],
                                  return_scores=True)
    ranked = [os.path.basename(p) for p in paths]
    assert len(ranked) == 70
    pages = [ranked[0], ranked[33], ranked[69]]
    got = demo.explain(kb, qvec, pages, index=ix, names=nm)
    assert [r for _, r in got] == [0, 33, 69]
    assert np.array_equal(_u32([s for s, _ in got]), _u32([scores[0], scores[33], scores[69]]))
    assert demo.explain(kb, torch.tensor(qvec[0]), ranked[5], index=ix, names=nm) == (scores[5], 5)
    docs = ["deck_2.pdf", "other_7.pdf"]
    only = [os.path.basename(p) for p in demo.retrieve(kb, qvec, 70, None, None, index=ix, names=nm, documents=docs)]
    assert len(only) == 6
    assert [r for _, r in demo.explain(kb, qvec, only, documents=docs, index=ix, names=nm)] == list(range(6))
    outside = next(n for n in ranked if n not in only)                   # the best page overall is not of these documents ...
    assert demo.explain(kb, qvec, outside, documents=docs, index=ix, names=nm)[1] == sum(1 for n in ranked[:ranked.index(outside)] if n in only)
    with pytest.raises(ValueError):
        demo.explain(kb, qvec, ["no_such_page.png"], index=ix, names=nm)
    assert demo.explain(kb, qvec, [], index=ix, names=nm) == []
    assert demo.explain(kb, qvec, ranked[0]) == (scores[0], 0)          # an index of its own, closed again
    assert demo.explain(str(tmp_path / "missing"), qvec, ranked[0]) is None
    ix.close()
