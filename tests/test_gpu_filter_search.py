"""-m gpu: the filtered search (vr_index_set_filters / vr_index_search_filtered, csrc/search_filter.hip) against the numpy
reference tests/filter_search_ref.py.

Bars (tests/test_gpu_group_search.py's): scores within 1e-5 of the fp64 reference; ids identical, except where the two scores
involved — the fp64 score of the row that was returned and the reference's score at that position — differ by less than 3e-7,
which is fp32 summation order.  At most 0.5 % of a case's (query, rank) positions may use that excuse.  Near-ties under 3e-7
between adjacent ranks of the reference alone, random_filters(nd, densities, seed=11), filter_of_query[q] = q % (n_filters + 1) - 1:

    case (nd, nq, dim, k)        near-ties / positions     allowed rows per filter
    (5000, 37, 256, 10)          0 / 370                   2532, 262, 10
    (3001, 300, 128, 26)         4 / 7 800 (0.05 %)        2721, 905, 22, 12
    (20000, 64, 2304, 10)        0 / 640                   10135, 214
    (1000, 5, 64, 40)            0 / 200                   520, 32

so the reference alone stays a factor ten inside the cap.  The cases hold a filter with exactly k rows (10 of k = 10), filters
with fewer than k rows (22 and 12 of k = 26, 32 of k = 40), the 256-query block boundary (300 queries), -1 queries next to
filtered ones and row counts that are no multiple of 32.  The deck and tie cases are strict: their references have no near-tie."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import filter_search_ref as F  # noqa: E402
from tests import group_search_ref as R  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.documents import doc_of_page, pack_filters  # noqa: E402
from visrag_amd.engine import HipIndex, _stream_ptr  # noqa: E402

ATOL, NEAR_TIE, EXCUSED = 1e-5, 3e-7, 0.005
VR_ERR_INVALID, VR_ERR_STATE = 1, 3


def _index(C, masks=None):
    ix = HipIndex(C.shape[1], len(C))
    ix.add(C[: len(C) // 2]); ix.add(C[len(C) // 2:])
    if masks is not None:
        ix.set_filters(masks)
    return ix


def _np(*xs):
    return [x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in xs]


def _check(got, ref, Q, C, masks, foq, strict=False):
    """`got` against `ref` under the bars of the module docstring; strict: no excuse at all."""
    (sc, ids), (rs, ri) = _np(*got), ref
    assert sc.shape == rs.shape and ids.shape == ri.shape
    assert sc.dtype == np.float32 and ids.dtype == np.int64
    none = ri < 0
    assert np.array_equal(ids < 0, none)
    assert (ids[none] == -1).all() and np.isneginf(sc[none]).all()
    np.testing.assert_allclose(sc[~none], rs[~none], atol=ATOL, rtol=0)
    for q, f in enumerate(np.asarray(foq).reshape(-1)):                  # whatever is returned is allowed, and no row comes twice
        i = ids[q][ids[q] >= 0]
        assert len(set(i.tolist())) == len(i) and (i < len(C)).all()
        assert f < 0 or np.asarray(masks)[f][i].all(), (q, f)
    bad = np.argwhere(ids != ri)
    if strict:
        assert len(bad) == 0, bad[:5]
    for q, c in bad:
        s = float(np.dot(Q[q].astype(np.float64), C[ids[q, c]].astype(np.float64)))
        assert abs(s - rs[q, c]) < NEAR_TIE, (q, c, ids[q, c], ri[q, c], s, rs[q, c])
    assert len(bad) <= EXCUSED * ids.size, (len(bad), ids.size)


def _same_bits(a, b):
    (s0, i0), (s1, i1) = _np(*a), _np(*b)
    return np.array_equal(s0.view(np.uint32), s1.view(np.uint32)) and np.array_equal(i0, i1)


@functools.lru_cache(maxsize=None)
def _random_case(nd, nq, dim, k, densities):
    C, Q, M = R.unit(nd, dim, 1), R.unit(nq, dim, 2), F.random_filters(nd, densities, seed=11)
    foq = (np.arange(nq) % (len(densities) + 1) - 1).astype(np.int64)
    return R.frozen(C, Q, M, foq) + (F.filtered_topk_ref(Q, C, M, foq, k),)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nd,nq,dim,k,densities", [(5000, 37, 256, 10, (0.5, 0.05, 0.002)), (3001, 300, 128, 26, (0.9, 0.3, 0.01, 0.004)),
                                                   (20000, 64, 2304, 10, (0.5, 0.01)), (1000, 5, 64, 40, (0.5, 0.03))])
def test_random_unit_rows(nd, nq, dim, k, densities, on_device):
    C, Q, M, foq, ref = _random_case(nd, nq, dim, k, densities)
    if on_device:
        ix = _index(C, torch.tensor(M).cuda())
        got = ix.search_filtered(torch.tensor(Q).cuda(), k, torch.tensor(foq).cuda())
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in got)
    else:
        ix = _index(C, M)
        got = ix.search_filtered(Q, k, foq)
        assert all(isinstance(x, np.ndarray) for x in got)
    assert ix.n_filters == len(densities)
    _check(got, ref, Q, C, M, foq)
    assert sum(ix.filter_search_stats().values()) == nq
    ix.close()


def test_allowed_count_edges():
    """n = 1001 rows (31.3 words), k = 10, one filter per allowed count around 0, k and k + 24 (the candidate margin): filter j
    allows the first counts[j] entries of a fixed permutation of the rows.  The filters arrive packed, the 23 spare bits of the
    last word SET: garbage that must be ignored.  Every query against every filter, strictly."""
    n, dim, k = 1001, 64, 10
    counts = [0, 1, 9, 10, 11, 33, 34, 35]
    C, Q = R.unit(n, dim, 1), R.unit(6, dim, 2)
    perm = np.random.default_rng(12).permutation(n)
    M = np.zeros((len(counts), n), dtype=bool)
    for j, c in enumerate(counts):
        M[j, perm[:c]] = True
    W = pack_filters(M)
    W[:, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(n & 31)
    assert W.shape == (len(counts), 32) and (W[:, -1] >> np.uint32(31)).all()
    Qt = np.tile(Q, (len(counts), 1))
    foq = np.repeat(np.arange(len(counts)), len(Q))
    ref = F.filtered_topk_ref(Qt, C, M, foq, k)
    for j, c in enumerate(counts):                                       # the tails of the reference itself
        assert (ref[1][foq == j][:, min(c, k):] == -1).all() and (ref[1][foq == j][:, :min(c, k)] >= 0).all()
    ix = _index(C, W)
    got = ix.search_filtered(Qt, k, foq)
    _check(got, ref, Qt, C, M, foq, strict=True)
    assert sum(ix.filter_search_stats(reset=True).values()) == len(Qt)
    ix.set_filters(torch.tensor(W.view(np.int32)).cuda())                # the same words handed over on the device
    got = ix.search_filtered(torch.tensor(Qt).cuda(), k, foq)
    _check(got, ref, Qt, C, M, foq, strict=True)
    assert sum(ix.filter_search_stats().values()) == len(Qt)
    ix.close()


@pytest.mark.parametrize("k", [10, 40])
def test_all_ones_filter_and_minus_one_are_the_plain_search(k):
    """bit-for-bit scores and equal ids (k = 10: against the fused sweep, k = 40: against the deep path)"""
    n = 5000
    C, Q = R.unit(n, 256, 1), R.unit(37, 256, 2)
    ix = _index(C, np.ones((1, n), dtype=bool))
    plain = ix.search(Q, k)
    assert _same_bits(ix.search_filtered(Q, k, 0), plain)
    assert _same_bits(ix.search_filtered(Q, k, -1), plain)
    assert _same_bits(ix.search_filtered(Q, k), plain)
    assert _same_bits(ix.search_filtered(torch.tensor(Q).cuda(), k, [0, -1] * 18 + [0]), plain)
    ix.close()


def test_the_best_rows_are_excluded():
    n, k = 5000, 10
    C, Q = R.unit(n, 256, 1), R.unit(37, 256, 2)
    ix = _index(C)
    top40 = ix.search(Q, 40)[1][0]
    M = np.ones((1, n), dtype=bool)
    M[0, top40] = False
    ix.set_filters(M)
    foq = np.zeros(len(Q), dtype=np.int64)
    got = ix.search_filtered(Q, k, 0)
    _check(got, F.filtered_topk_ref(Q, C, M, foq, k), Q, C, M, foq)
    order = np.argsort(-R.scores64(Q[:1], C)[0], kind="stable")
    assert set(order[:40].tolist()) == set(top40.tolist())
    assert np.array_equal(got[1][0], order[40:40 + k])                   # ranks 41.. of the unfiltered reference
    assert not np.isin(got[1], top40).any()
    ix.close()


def test_all_scores_negative_padded_columns_never_win():
    """The construction of tests/test_gpu_group_search.py's test of the same name (1001 rows in the positive orthant, negated
    queries: the zero of a padded column beats every real score) under a density-0.5 filter."""
    n, dim, k = 1001, 64, 10
    C = np.abs(R.unit(n, dim, 1))
    rng = np.random.default_rng(4)
    Q = np.empty((20, dim), np.float32)
    for q in range(len(Q)):
        for _ in range(100):
            v = -C[rng.integers(0, n, size=3)].sum(0)
            Q[q] = v / np.linalg.norm(v)
            if (R.scores64(Q[q:q + 1], C) < 0).all():
                break
        else:
            raise AssertionError("no query with negative scores only")
    M = F.random_filters(n, (0.5,), seed=11)
    foq = np.zeros(len(Q), dtype=np.int64)
    ref = F.filtered_topk_ref(Q, C, M, foq, k)
    assert (ref[0] < 0).all()
    ix = _index(C, M)
    for q_in in (Q, torch.tensor(Q).cuda()):
        got = ix.search_filtered(q_in, k, 0)
        sc, ids = _np(*got)
        assert (sc < 0).all() and (ids >= 0).all() and (ids < n).all() and M[0][ids].all()
        _check(got, ref, Q, C, M, foq)
    ix.close()


def test_near_duplicate_decks_under_a_filter_that_cuts_inside_decks():
    """300 documents x 10 near-identical pages (noise 1e-3), dim 256 and dim 2304, filters of density 0.5 and 0.2 that cut
    inside the decks, filter_of_query[q] = q % 2, k = 10.  Strict: the reference has 0 near-ties in 500 positions for both dims
    (noise 3e-4 at dim 2304 has 4 and is therefore not used).  The allowed pages of a deck lie inside the error band of each
    other, so this is where the k + 24 candidates can fall short.  Emulated on the CPU from the error model (bf16-rounded
    operands, fp64 products, eps of query_eps): at dim 256 every query certifies from its first candidate set (the smallest
    margin tau - T is 4.7e-3), at dim 2304 one query has T above tau by 6e-4 and must widen; fp32 accumulation moves either
    figure by ~1e-6.  Over the two dims: certified_widened + exact > 0, and the counters sum to the queries searched."""
    total = {"certified": 0, "certified_widened": 0, "exact": 0}
    for dim in (256, 2304):
        C, _ = R.decks(300, 10, dim, 1e-3)
        Q = R.unit(50, dim, 7)
        M = F.random_filters(3000, (0.5, 0.2), seed=11)
        foq = np.arange(len(Q)) % 2
        ref = F.filtered_topk_ref(Q, C, M, foq, 10)
        ix = _index(C, M)
        _check(ix.search_filtered(Q, 10, foq), ref, Q, C, M, foq, strict=True)
        st = ix.filter_search_stats()
        print(dim, st)
        assert sum(st.values()) == len(Q), st
        _check(ix.search_filtered(torch.tensor(Q).cuda(), 10, foq), ref, Q, C, M, foq, strict=True)
        st = ix.filter_search_stats(reset=True)
        assert sum(st.values()) == 2 * len(Q) and sum(ix.filter_search_stats().values()) == 0
        for key in total:
            total[key] += st[key]
        ix.close()
    assert total["certified_widened"] + total["exact"] > 0, total
    assert sum(total.values()) == 2 * 2 * 50


def test_ties():
    """R.tie_tier (3000 rows, 2900 of them identical, 100 distinct rows above), k = 150.  Filter 0 allows every second row: 50
    high rows, then the lowest allowed tied ids ascending — the 1450 allowed ties exceed any candidate set, every query is redone
    exactly.  Filter 1 allows all high rows and 500 tied ones: the widened set (600 <= 1024) holds them, never the exact pass."""
    C, Q, _ = R.tie_tier()
    n, k = len(C), 150
    high = 7 * np.arange(100) + 3
    tied = np.setdiff1d(np.arange(n), high)
    M = np.zeros((2, n), dtype=bool)
    M[0, ::2] = True
    M[1, high] = True
    M[1, tied[3::5][:500]] = True
    assert M[0][tied].sum() == 1450 and M[1].sum() == 600
    S = R.scores64(Q, C)
    hi0 = high[M[0][high]]
    want = np.stack([np.concatenate([hi0[np.argsort(-S[q][hi0])], tied[M[0][tied]][: k - len(hi0)]]) for q in range(len(Q))])
    ix = _index(C, M)
    foq0, foq1 = np.zeros(len(Q), dtype=np.int64), np.ones(len(Q), dtype=np.int64)
    ref0 = F.filtered_topk_ref(Q, C, M, foq0, k)
    assert np.array_equal(ref0[1], want)
    for q_in in (Q, torch.tensor(Q).cuda()):
        got = ix.search_filtered(q_in, k, 0)
        assert np.array_equal(_np(*got)[1], want)
        _check(got, ref0, Q, C, M, foq0, strict=True)
    assert ix.filter_search_stats(reset=True) == {"certified": 0, "certified_widened": 0, "exact": 2 * len(Q)}
    ref1 = F.filtered_topk_ref(Q, C, M, foq1, k)
    for q_in in (Q, torch.tensor(Q).cuda()):
        _check(ix.search_filtered(q_in, k, 1), ref1, Q, C, M, foq1, strict=True)
    st = ix.filter_search_stats()
    assert st["exact"] == 0 and st["certified"] + st["certified_widened"] == 2 * len(Q), st
    ix.close()


def test_uncertified_mode_returns_rescored_allowed_candidates():
    C, Q, M, foq, _ = _random_case(5000, 37, 256, 10, (0.5, 0.05, 0.002))
    ix = _index(C, M)
    ix.set_search_eps(-1.0)
    sc, ids = ix.search_filtered(Q, 10, foq)
    assert sum(ix.filter_search_stats().values()) == 0                   # nothing certified, nothing counted
    for q in range(len(Q)):                                              # whatever comes back is allowed and carries its exact fp32 score
        for s, i in zip(sc[q], ids[q]):
            if i < 0:
                assert np.isneginf(s)
                continue
            assert foq[q] < 0 or M[foq[q]][i]
            assert abs(s - float(np.dot(Q[q].astype(np.float64), C[i].astype(np.float64)))) < ATOL
    ix.close()


# ------------------------------------------------------------------------------------- errors and isolation ---
def _status(fn, *a):
    with pytest.raises(_lib.VisragHipError) as e:
        fn(*a)
    return int(str(e.value).split("(status ")[1].split(")")[0])


def _raw_search(ix, Q, k, foq):
    """vr_index_search_filtered itself, past the wrapper's range check: host arrays, or cuda tensors -> (status, scores, ids)"""
    cuda = isinstance(Q, torch.Tensor)
    nq = Q.shape[0]
    if cuda:
        sc = torch.empty((nq, max(k, 1)), dtype=torch.float32, device=Q.device)
        ids = torch.empty((nq, max(k, 1)), dtype=torch.int64, device=Q.device)
        ptr = [Q.data_ptr(), foq.data_ptr(), sc.data_ptr(), ids.data_ptr()]
    else:
        sc, ids = np.empty((nq, max(k, 1)), np.float32), np.empty((nq, max(k, 1)), np.int64)
        ptr = [Q.ctypes.data, foq.ctypes.data, sc.ctypes.data, ids.ctypes.data]
    st = ix.lib.vr_index_search_filtered(ix._h, ctypes.c_void_p(ptr[0]), nq, k, ctypes.c_void_p(ptr[1]), ctypes.c_void_p(ptr[2]),
                                         ctypes.c_void_p(ptr[3]), 1 if cuda else 0, ctypes.c_void_p(_stream_ptr(ix.device)))
    if cuda:
        torch.cuda.synchronize()
    return st, sc, ids


def test_errors_leave_the_plain_search_alone():
    n = 600
    C, Q = R.unit(n, 64, 1), R.unit(4, 64, 2)
    M = F.random_filters(n, (0.5, 0.1), seed=11)
    W = pack_filters(M)
    ix = HipIndex(64, n + 10)
    before = None

    def same():
        return _same_bits(ix.search(Q, 10), before[0]) and _same_bits(ix.search(Q, 40), before[1])

    def set_raw(bits, nf):
        return ix.lib.vr_index_set_filters(ix._h, ctypes.c_void_p(bits), nf, 0, ctypes.c_void_p(_stream_ptr(ix.device)))

    assert set_raw(W.ctypes.data, 2) == VR_ERR_INVALID                                 # an empty index
    ix.add(C)
    before = (ix.search(Q, 10), ix.search(Q, 40))
    assert _status(ix.search_filtered, Q, 5, 0) == VR_ERR_STATE and same()             # before set_filters
    assert set_raw(None, 2) == VR_ERR_INVALID and same()                               # NULL bits
    assert set_raw(W.ctypes.data, 0) == VR_ERR_INVALID and same()                      # no filter
    assert _status(ix.search_filtered, Q, 5, 0) == VR_ERR_STATE and same()             # none of them set anything
    ix.set_filters(M)
    foq = np.array([0, 1, -1, 1], dtype=np.int32)
    ref = F.filtered_topk_ref(Q, C, M, foq, 5)
    _check(ix.search_filtered(Q, 5, foq), ref, Q, C, M, foq)
    assert set_raw(None, 2) == VR_ERR_INVALID and set_raw(W.ctypes.data, 0) == VR_ERR_INVALID
    _check(ix.search_filtered(Q, 5, foq), ref, Q, C, M, foq)                            # the index keeps the filters it had
    assert same()
    assert _status(ix.search_filtered, Q, 0, 0) == VR_ERR_INVALID and same()
    assert _status(ix.search_filtered, Q, 1001, 0) == VR_ERR_INVALID and same()
    for bad in (2, -2):                                                                # a host entry == n_filters, == -2
        with pytest.raises(ValueError):
            ix.search_filtered(Q, 5, [0, bad, -1, 1])
        assert _raw_search(ix, Q, 5, np.array([0, bad, -1, 1], dtype=np.int32))[0] == VR_ERR_INVALID and same()
    # on the device the entries cannot be seen before the launch: such a query gets an empty row, the others their results
    dev_foq = np.array([0, 2, -1, -7], dtype=np.int32)
    st, sc, ids = _raw_search(ix, torch.tensor(Q).cuda(), 5, torch.tensor(dev_foq).cuda())
    sc, ids = _np(sc, ids)
    assert st == 0 and (ids[[1, 3]] == -1).all() and np.isneginf(sc[[1, 3]]).all()
    good = np.array([0, 2])
    _check((sc[good], ids[good]), tuple(x[good] for x in F.filtered_topk_ref(Q, C, M, np.array([0, 0, -1, 0]), 5)), Q[good], C, M,
           dev_foq[good])
    assert same()
    ix.add(C[:10])                                                                     # a further add drops the filters
    assert ix.n_filters == 0 and _status(ix.search_filtered, Q, 5, 0) == VR_ERR_STATE
    ix.reset(); ix.add(C)
    assert same()
    ix.set_filters(W)
    ix.reset()                                                                         # so does reset
    assert ix.n_filters == 0 and _status(ix.search_filtered, Q, 5, 0) == VR_ERR_STATE
    ix.add(C)
    assert _status(ix.search_filtered, Q, 5, 0) == VR_ERR_STATE and same()
    ix.close()


def test_existing_searches_are_untouched():
    C, Q, M, foq, _ = _random_case(5000, 37, 256, 10, (0.5, 0.05, 0.002))
    off = R.random_offsets(len(C), 7)
    ix = _index(C)
    ix.set_groups(off)
    before = [ix.search(Q, k) for k in (10, 40)]
    groups_before = ix.search_groups(Q, 10)
    ix.set_filters(M)
    assert ix.n_groups == len(off) - 1 and ix.n_filters == len(M)                      # independent state
    stats, plan, gstats = ix.search_stats(), ix.search_plan(len(Q)), ix.group_search_stats()
    ix.search_filtered(Q, 10, foq); ix.search_filtered(torch.tensor(Q).cuda(), 40, foq)
    assert ix.search_stats() == stats and ix.search_plan(len(Q)) == plan and ix.group_search_stats() == gstats
    assert sum(ix.filter_search_stats().values()) == 2 * len(Q)
    for k, b in zip((10, 40), before):
        assert _same_bits(ix.search(Q, k), b)
    groups_now = ix.search_groups(Q, 10)                                               # still works with filters set
    assert _same_bits(groups_now[:2], groups_before[:2]) and np.array_equal(groups_now[2], groups_before[2])
    fstats = ix.filter_search_stats()
    ix.search(Q, 40); ix.search_groups(Q, 10)
    assert ix.filter_search_stats() == fstats                                          # ... and the other searches count nothing here
    ix.close()


# ---------------------------------------------------------------------------------------------- host paths ---
def _paged_corpus():
    """12 documents of 1-6 pages, page names `<pdf>_<idx>.png`, pages of the documents interleaved
    (the shape of tests/test_gpu_group_search.py's corpus)"""
    rng = np.random.default_rng(8)
    docs = [f"deck_{d}.pdf" for d in range(12)]
    names = [f"{doc}_{i}.png" for d, doc in enumerate(docs) for i in range(1 + d % 6)]
    names = [names[i] for i in rng.permutation(len(names))]
    return names, R.unit(len(names), 64, 9), R.unit(3, 64, 10)


def _label_ref(labels, wanted, C, q, k):
    """-> [(row of C, score)] of the k best rows whose label is wanted, best first"""
    mask = np.array([lab in wanted for lab in labels], dtype=bool)[None, :]
    sc, ids = F.filtered_topk_ref(q.reshape(1, -1), C, mask, [0], k)
    return [(int(i), float(s)) for s, i in zip(sc[0], ids[0]) if i >= 0]


def test_demo_retrieve_documents_argument(tmp_path):
    from visrag_amd import demo
    names, C, Q = _paged_corpus()
    kb = str(tmp_path / "kb")
    os.makedirs(kb)
    np.save(os.path.join(kb, "reps.npy"), C)
    with open(os.path.join(kb, "index2img_filename.txt"), "w") as f:
        f.write("\n".join(names))
    labels = [doc_of_page(n) for n in names]
    wanted = ["deck_3.pdf", "deck_10.pdf", "no_such.pdf"]                  # 4 + 5 pages; an unknown name contributes nothing
    plain, plain_names = demo.load_knowledge_base(kb, 0)
    grouped, grouped_names = demo.load_document_base(kb, 0)
    for q in range(len(Q)):
        ref = _label_ref(labels, wanted, C, Q[q], 5)
        for ix, nm in ((plain, plain_names), (grouped, grouped_names)):
            paths, scores = demo.retrieve(kb, Q[q], 5, None, None, index=ix, names=nm, return_scores=True, documents=wanted)
            assert paths == [os.path.join(kb, names[row]) for row, _ in ref]
            assert {doc_of_page(os.path.basename(p)) for p in paths} <= set(wanted)
            np.testing.assert_allclose(scores, [s for _, s in ref], atol=ATOL, rtol=0)
    assert grouped.n_groups == 12                                         # the grouping is still there
    assert len(demo.retrieve(kb, Q[0], 50, None, None, index=plain, names=plain_names, documents=iter(wanted))) == 9
    assert demo.retrieve(kb, torch.tensor(Q[0]), 5, None, None, index=plain, names=plain_names, documents=["deck_0.pdf"]) == \
        [os.path.join(kb, "deck_0.pdf_0.png")]
    assert demo.retrieve(kb, Q[0], 5, None, None, index=plain, names=plain_names, documents=["no_such.pdf"]) == []
    assert demo.retrieve(kb, Q[0], 5, None, None, index=plain, names=plain_names, documents=[], return_scores=True) == ([], [])
    assert demo.retrieve(str(tmp_path / "missing"), Q[0], 5, None, None, documents=wanted) is None
    plain.close(); grouped.close()


def test_retriever_retrieve_filtered(tmp_path):
    from visrag_amd import retriever
    from visrag_amd.utils import save_as_trec, write_shard
    names, C, Q = _paged_corpus()
    half = len(names) // 2
    write_shard(str(tmp_path / "embeddings.corpus.rank.0"), C[:half], names[:half])
    write_shard(str(tmp_path / "embeddings.corpus.rank.1"), C[half:], names[half:])
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, ["q0", "q1", "q2"])
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    wanted = {"q0": {"deck_3.pdf", "deck_5.pdf"}, "q1": None, "q2": {"deck_0.pdf"}}     # 4 + 6 pages | all | 1 page
    result = retriever.retrieve_filtered(args, 4, doc_of_page, wanted.get)
    labels = [doc_of_page(n) for n in names]
    for q, qid in enumerate(["q0", "q1", "q2"]):
        ref = _label_ref(labels, set(labels) if wanted[qid] is None else wanted[qid], C, Q[q], 4)
        assert list(result[qid]) == [names[row] for row, _ in ref]
        np.testing.assert_allclose(list(result[qid].values()), [s for _, s in ref], atol=ATOL, rtol=0)
    assert len(result["q2"]) == 1
    save_as_trec(result, str(tmp_path / "run.trec"))
    assert sum(1 for _ in open(tmp_path / "run.trec")) == 4 + 4 + 1
