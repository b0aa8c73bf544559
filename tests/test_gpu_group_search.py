"""-m gpu: the document-level search (vr_index_set_groups / vr_index_search_groups, csrc/search_group.hip) against the numpy
reference tests/group_search_ref.py.

Bars (tests/test_gpu_search.py's): scores within 1e-5 of the fp64 reference; best rows and groups identical, except where the
two scores involved — the fp64 score of the row that was returned and the reference's score at that position — differ by less
than 3e-7, which is fp32 summation order.  At most 0.5 % of a case's (query, rank) positions may use that excuse (the reference
alone has at most 4 near-ties of that size among the 7 800 positions of the listed random cases, none in the deck cases)."""
import functools
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import group_search_ref as R  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.engine import HipIndex  # noqa: E402

ATOL, NEAR_TIE, EXCUSED = 1e-5, 3e-7, 0.005


def _index(C, offsets=None):
    ix = HipIndex(C.shape[1], len(C))
    ix.add(C[: len(C) // 2]); ix.add(C[len(C) // 2:])
    if offsets is not None:
        ix.set_groups(offsets)
    return ix


def _np(*xs):
    return [x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in xs]


def _check(got, ref, Q, C, offsets, strict=False):
    """`got` against `ref` under the bars of the module docstring; strict: no excuse at all."""
    (sc, ids, gr), (rs, ri, rg) = _np(*got), ref
    off = np.asarray(offsets)
    assert sc.shape == rs.shape and ids.shape == ri.shape and gr.shape == rg.shape
    assert sc.dtype == np.float32 and ids.dtype == np.int64 and gr.dtype == np.int64
    none = ri < 0
    assert np.array_equal(ids < 0, none) and np.array_equal(gr < 0, none)
    assert (ids[none] == -1).all() and (gr[none] == -1).all() and np.isneginf(sc[none]).all()
    np.testing.assert_allclose(sc[~none], rs[~none], atol=ATOL, rtol=0)
    # whatever is returned is a row of the group it is returned for, and no group comes twice
    assert (off[gr[~none]] <= ids[~none]).all() and (ids[~none] < off[gr[~none] + 1]).all()
    for q in range(len(gr)):
        g = gr[q][gr[q] >= 0]
        assert len(set(g.tolist())) == len(g)
    bad = np.argwhere((ids != ri) | (gr != rg))
    if strict:
        assert len(bad) == 0, bad[:5]
    for q, c in bad:
        s = float(np.dot(Q[q].astype(np.float64), C[ids[q, c]].astype(np.float64)))
        assert abs(s - rs[q, c]) < NEAR_TIE, (q, c, ids[q, c], ri[q, c], gr[q, c], rg[q, c], s, rs[q, c])
    assert len(bad) <= EXCUSED * ids.size, (len(bad), ids.size)


@functools.lru_cache(maxsize=None)
def _random_case(nd, nq, dim, k, mean):
    C, Q, off = R.unit(nd, dim, 1), R.unit(nq, dim, 2), R.random_offsets(nd, mean)
    return R.frozen(C, Q, off) + (R.group_topk_ref(Q, C, off, k),)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nd,nq,dim,k,mean", [(5000, 37, 256, 10, 7), (3001, 300, 128, 26, 10), (20000, 64, 2304, 10, 10),
                                              (1000, 5, 64, 40, 3)])
def test_random_unit_rows(nd, nq, dim, k, mean, on_device):
    C, Q, off, ref = _random_case(nd, nq, dim, k, mean)
    ix = _index(C, off)
    got = ix.search_groups(torch.tensor(Q).cuda() if on_device else Q, k)
    assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in got) if on_device else all(isinstance(x, np.ndarray) for x in got)
    _check(got, ref, Q, C, off)
    ix.close()


@pytest.mark.parametrize("k", [10, 40])
def test_groups_of_one_row_are_the_row_search(k):
    """offsets = arange(n + 1): the grouped search is the row search, bit for bit (k = 10: the fused sweep, k = 40: the deep path)"""
    n = 5000
    C, Q = R.unit(n, 256, 1), R.unit(37, 256, 2)
    ix = _index(C, np.arange(n + 1))
    ps, pi = ix.search(Q, k)
    sc, ids, gr = ix.search_groups(Q, k)
    assert np.array_equal(ids, pi) and np.array_equal(sc.view(np.uint32), ps.view(np.uint32))
    assert np.array_equal(gr, ids)
    ix.close()


def test_one_group_over_the_whole_index():
    n, k = 3001, 10
    C, Q = R.unit(n, 128, 1), R.unit(9, 128, 2)
    ix = _index(C, [0, n])
    sc, ids, gr = ix.search_groups(Q, k)
    ps, pi = ix.search(Q, 1)
    assert np.array_equal(ids[:, 0], pi[:, 0]) and np.array_equal(sc[:, 0], ps[:, 0]) and (gr[:, 0] == 0).all()
    assert np.array_equal(ids[:, 0], R.scores64(Q, C).argmax(1))
    assert (ids[:, 1:] == -1).all() and (gr[:, 1:] == -1).all() and np.isneginf(sc[:, 1:]).all()
    ix.close()


def test_all_scores_negative_padded_columns_never_win():
    """1001 rows: the score rows are padded to 1024 columns, and the padding's zero beats every real score here.
    Rows are the absolute values of _unit(1001, 64, .) and a query is minus the normalised sum of a few of them: with rows of
    mixed signs no query has all 1001 scores negative (about half of them are positive for any direction), so the rows are
    folded into the positive orthant first; a query with a positive score in the fp64 reference is still remade."""
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
    off = R.random_offsets(n, 5)
    ref = R.group_topk_ref(Q, C, off, k)
    assert (ref[0] < 0).all()
    for q_in in (Q, torch.tensor(Q).cuda()):
        ix = _index(C, off)
        got = ix.search_groups(q_in, k)
        sc, ids, gr = _np(*got)
        assert (sc < 0).all() and (ids >= 0).all() and (ids < n).all()        # nothing from a padded column
        _check(got, ref, Q, C, off)
        ix.close()


@pytest.mark.parametrize("dim,noise", [(256, 1e-3), (2304, 3e-4)])
def test_near_duplicate_decks(dim, noise):
    """300 documents x 10 near-identical pages: the bf16 scores pick another page than the fp32 scores do in ~9 % of the (query,
    document) pairs, so the best rows are right only if every row within 2 eps of its group's bf16 maximum is re-scored.  The
    best-to-second gaps inside the returned documents are >= 5e-7 in the fp64 reference: no excuse."""
    C, off = R.decks(300, 10, dim, noise)
    Q = R.unit(50, dim, 7)
    ref = R.group_topk_ref(Q, C, off, 10)
    ix = _index(C, off)
    _check(ix.search_groups(Q, 10), ref, Q, C, off, strict=True)
    st = ix.group_search_stats()
    assert sum(st.values()) == len(Q), st
    _check(ix.search_groups(torch.tensor(Q).cuda(), 10), ref, Q, C, off, strict=True)
    assert sum(ix.group_search_stats(reset=True).values()) == 2 * len(Q)
    assert sum(ix.group_search_stats().values()) == 0
    ix.close()


def test_exact_ties():
    dim, n = 128, 2000
    C = R.unit(n, dim, 3)
    off = R.random_offsets(n, 6)
    lens = np.diff(off)
    ga, gb, gc = [int(g) for g in np.flatnonzero(lens >= 3)[[2, 40, 90]]]
    r1, r2 = int(off[ga]) + 0, int(off[ga]) + 2
    C[r2] = C[r1]                                     # a duplicated row inside group ga
    ra, rb = int(off[gb]) + 1, int(off[gc]) + 0
    C[rb] = C[ra]                                     # one row in group gb and a copy of it in group gc > gb
    Q = np.concatenate([C[r1:r1 + 1], C[ra:ra + 1], R.unit(5, dim, 4)])
    ix = _index(C, off)
    ref = R.group_topk_ref(Q, C, off, 10)
    for q_in in (Q, torch.tensor(Q).cuda()):
        sc, ids, gr = _np(*ix.search_groups(q_in, 10))
        assert ids[0, 0] == r1 and gr[0, 0] == ga
        assert list(ids[1, :2]) == [ra, rb] and list(gr[1, :2]) == [gb, gc] and sc[1, 0] == sc[1, 1]
        _check((sc, ids, gr), ref, Q, C, off)
    ix.close()


def test_more_tied_groups_than_any_candidate_set():
    """3 000 groups of two identical rows: every group ties, neither candidate set can hold them, the queries are redone exactly"""
    dim, ng, k = 64, 3000, 10
    C = np.tile(R.unit(1, dim, 6), (2 * ng, 1))
    Q = R.unit(3, dim, 2)
    ix = _index(C, np.arange(ng + 1) * 2)
    sc, ids, gr = ix.search_groups(Q, k)
    assert np.array_equal(ids, np.tile(np.arange(k) * 2, (3, 1))) and np.array_equal(gr, np.tile(np.arange(k), (3, 1)))
    np.testing.assert_allclose(sc, np.repeat(R.scores64(Q, C[:1]), k, 1), atol=ATOL, rtol=0)
    assert ix.group_search_stats() == {"certified": 0, "certified_widened": 0, "exact": 3}
    ix.close()


def test_tie_tier_below_distinct_groups():
    """R.tie_tier: 100 distinct rows above 2 900 identical ones, k = 150 — the candidates are every key above the threshold and
    then the LOWEST of its ties.  Groups of one row: the row search, and that the expected rows; groups of three adjacent rows:
    the reference, strictly (the input has no near-tie: R.tie_tier checks it).  The tier lies inside the error band: 2 900 tied
    groups are beyond any candidate set (exact scores, the select with kp = k: 100 above, 50 of the ties), 900 tied groups of
    three and the 100 above them fit the widened one (<= 1 024)."""
    C, Q, want = R.tie_tier()
    n, k = len(C), want.shape[1]
    ix = _index(C, np.arange(n + 1))
    pi = ix.search(Q, k)[1]
    sc, ids, gr = ix.search_groups(Q, k)
    assert np.array_equal(ids, pi) and np.array_equal(ids, want) and np.array_equal(gr, ids)
    assert ix.group_search_stats(reset=True) == {"certified": 0, "certified_widened": 0, "exact": len(Q)}
    off = np.arange(0, n + 1, 3)
    ix.set_groups(off)
    ref = R.group_topk_ref(Q, C, off, k)
    _check(ix.search_groups(Q, k), ref, Q, C, off, strict=True)
    _check(ix.search_groups(torch.tensor(Q).cuda(), k), ref, Q, C, off, strict=True)
    assert ix.group_search_stats() == {"certified": 0, "certified_widened": 2 * len(Q), "exact": 0}
    ix.close()


def test_fewer_groups_than_k():
    C, Q = R.unit(100, 64, 1), R.unit(6, 64, 2)
    off = [0, 1, 40, 99, 100]
    ix = _index(C, off)
    for k in (10, 40):
        got = ix.search_groups(Q, k)
        assert (got[1][:, 4:] == -1).all() and (got[2][:, 4:] == -1).all() and np.isneginf(got[0][:, 4:]).all()
        _check(got, R.group_topk_ref(Q, C, off, k), Q, C, off)
    ix.close()


def test_uncertified_mode_returns_rescored_candidates():
    C, Q, off, ref = _random_case(5000, 37, 256, 10, 7)
    ix = _index(C, off)
    ix.set_search_eps(-1.0)
    sc, ids, gr = ix.search_groups(Q, 10)
    assert sum(ix.group_search_stats().values()) == 0            # nothing certified, nothing counted
    for q in range(len(Q)):                                       # whatever comes back carries its exact fp32 score
        for s, i in zip(sc[q], ids[q]):
            assert abs(s - float(np.dot(Q[q].astype(np.float64), C[i].astype(np.float64)))) < ATOL
    ix.close()


def _status(fn, *a):
    with pytest.raises(_lib.VisragHipError) as e:
        fn(*a)
    return int(str(e.value).split("(status ")[1].split(")")[0])


def test_errors_leave_the_plain_search_alone():
    VR_ERR_INVALID, VR_ERR_STATE = 1, 3
    n = 600
    C, Q = R.unit(n, 64, 1), R.unit(4, 64, 2)
    ix = HipIndex(64, n + 10)
    ix.add(C)
    before = ix.search(Q, 10)

    def same():
        now = ix.search(Q, 10)
        return np.array_equal(now[0].view(np.uint32), before[0].view(np.uint32)) and np.array_equal(now[1], before[1])

    assert _status(ix.search_groups, Q, 5) == VR_ERR_STATE and same()                  # before set_groups
    assert _status(ix.set_groups, [0, 300, 200, n]) == VR_ERR_INVALID and same()       # not monotonic
    assert _status(ix.set_groups, [0, 300, 300, n]) == VR_ERR_INVALID and same()       # not STRICTLY increasing
    assert _status(ix.set_groups, [0, 300, n - 1]) == VR_ERR_INVALID and same()        # wrong last offset
    assert _status(ix.set_groups, [0, 300, n + 1]) == VR_ERR_INVALID and same()
    assert _status(ix.set_groups, [1, 300, n]) == VR_ERR_INVALID and same()            # does not start at 0
    assert _status(ix.set_groups, [0]) == VR_ERR_INVALID and same()                    # no group
    assert ix.lib.vr_index_set_groups(ix._h, None, 1) == VR_ERR_INVALID and same()     # NULL
    assert _status(ix.search_groups, Q, 5) == VR_ERR_STATE and same()                  # none of them set anything
    ix.set_groups([0, 300, n])
    assert ix.search_groups(Q, 2)[2].shape == (4, 2)
    assert _status(ix.search_groups, Q, 0) == VR_ERR_INVALID and same()
    assert _status(ix.search_groups, Q, 1001) == VR_ERR_INVALID and same()
    ix.add(C[:10])                                                                     # a further add drops the grouping
    assert _status(ix.search_groups, Q, 5) == VR_ERR_STATE
    ix.reset(); ix.add(C)
    assert same()
    ix.set_groups([0, 300, n])
    ix.reset()                                                                         # so does reset
    assert _status(ix.search_groups, Q, 5) == VR_ERR_STATE
    ix.add(C)
    assert _status(ix.search_groups, Q, 5) == VR_ERR_STATE and same()
    ix.close()


def test_existing_searches_are_untouched():
    C, Q, off, _ = _random_case(5000, 37, 256, 10, 7)
    ix = _index(C, off)
    before = [ix.search(Q, k) for k in (10, 40)]
    stats = ix.search_stats()
    plan = ix.search_plan(len(Q))
    ix.search_groups(Q, 10); ix.search_groups(torch.tensor(Q).cuda(), 40)
    assert ix.search_stats() == stats and ix.search_plan(len(Q)) == plan
    for k, (s0, i0) in zip((10, 40), before):
        s1, i1 = ix.search(Q, k)
        assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)) and np.array_equal(i0, i1)
    ix.close()


# ---------------------------------------------------------------------------------------------- host paths ---
def _paged_corpus():
    """12 documents of 1-6 pages, page names `<pdf>_<idx>.png`, pages of the documents interleaved"""
    rng = np.random.default_rng(8)
    docs = [f"deck_{d}.pdf" for d in range(12)]
    names = [f"{doc}_{i}.png" for d, doc in enumerate(docs) for i in range(1 + d % 6)]
    names = [names[i] for i in rng.permutation(len(names))]
    return names, R.unit(len(names), 64, 9), R.unit(3, 64, 10)


def _host_ref(labels, C, Q, k):
    """documents by label on the host: -> per query [(label, score, row of C)], best first"""
    from visrag_amd.documents import group_rows
    order, off, docs = group_rows(labels)
    sc, ids, gr = R.group_topk_ref(Q, C[order], off, k)
    return [[(docs[g], s, int(order[i])) for s, i, g in zip(sc[q], ids[q], gr[q]) if i >= 0] for q in range(len(Q))]


def test_demo_retrieve_documents(tmp_path):
    from visrag_amd import demo
    from visrag_amd.documents import doc_of_page
    names, C, Q = _paged_corpus()
    kb = str(tmp_path / "kb")
    os.makedirs(kb)
    np.save(os.path.join(kb, "reps.npy"), C)
    with open(os.path.join(kb, "index2img_filename.txt"), "w") as f:
        f.write("\n".join(names))
    ref = _host_ref([doc_of_page(n) for n in names], C, Q, 5)
    ix, ix_names = demo.load_document_base(kb, 0)
    assert sorted(ix_names) == sorted(names) and ix.n_groups == 12
    for q in range(len(Q)):
        paths, scores = demo.retrieve_documents(kb, Q[q], 5, None, None, index=ix, names=ix_names, return_scores=True)
        assert paths == [os.path.join(kb, names[row]) for _, _, row in ref[q]]
        assert len({doc_of_page(os.path.basename(p)) for p in paths}) == 5          # five documents, not five pages of one
        np.testing.assert_allclose(scores, [s for _, s, _ in ref[q]], atol=ATOL, rtol=0)
    assert demo.retrieve_documents(kb, torch.tensor(Q[0]), 5, None, None, index=ix, names=ix_names) == \
        [os.path.join(kb, names[row]) for _, _, row in ref[0]]
    assert len(demo.retrieve_documents(kb, Q[0], 50, None, None, index=ix, names=ix_names)) == 12
    ix.close()
    # an index in the order on disk (pages interleaved) cannot be grouped in place
    plain, plain_names = demo.load_knowledge_base(kb, 0)
    with pytest.raises(ValueError):
        demo.retrieve_documents(kb, Q[0], 5, None, None, index=plain, names=plain_names)
    plain.close()
    assert demo.retrieve_documents(str(tmp_path / "missing"), Q[0], 5, None, None) is None


def test_retriever_retrieve_documents(tmp_path):
    from visrag_amd import retriever
    from visrag_amd.documents import doc_of_page
    from visrag_amd.utils import write_shard
    names, C, Q = _paged_corpus()
    half = len(names) // 2
    write_shard(str(tmp_path / "embeddings.corpus.rank.0"), C[:half], names[:half])
    write_shard(str(tmp_path / "embeddings.corpus.rank.1"), C[half:], names[half:])
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, ["q0", "q1", "q2"])
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    scores, pages = retriever.retrieve_documents(args, 4, doc_of_page)
    ref = _host_ref([doc_of_page(n) for n in names], C, Q, 4)
    for q, qid in enumerate(["q0", "q1", "q2"]):
        assert list(scores[qid]) == [d for d, _, _ in ref[q]] and list(pages[qid]) == list(scores[qid])
        assert [pages[qid][d] for d, _, _ in ref[q]] == [names[row] for _, _, row in ref[q]]
        np.testing.assert_allclose(list(scores[qid].values()), [s for _, s, _ in ref[q]], atol=ATOL, rtol=0)
    from visrag_amd.utils import save_as_trec
    save_as_trec(scores, str(tmp_path / "run.trec"))
    assert sum(1 for _ in open(tmp_path / "run.trec")) == 3 * 4
