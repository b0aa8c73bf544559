"""The numpy reference of the document rank search (tests/group_rank_search_ref.py) on hand-worked cases, what it alone says about
the fp64 intervals on the corpora of tests/test_gpu_group_rank_search.py, the host helpers (documents.never_retrieved,
demo.explain_documents, retriever.rank_documents over a host stand-in for the index) and the declarations of the three ABI
symbols.  No GPU, no library."""
import os
import types

import numpy as np
import pytest

from tests import group_rank_search_ref as K
from tests import group_search_ref as R
from tests import group_window_search_ref as G
from tests.test_cpu_group_window_search_ref import HostIndex, _base
from visrag_amd import demo, retriever
from visrag_amd.documents import NEVER_RETRIEVED, mrr_from_ranks, never_retrieved, recall_at, reciprocal_ranks
from visrag_amd.utils import write_shard

# one query, nine pages in four documents
#   document 0 = rows 0-2 (.5, .75, .75)   document 1 = row 3 (.25)   document 2 = rows 4-6 (.75, .9, .1)   document 3 = rows 7-8 (.75, .2)
S = np.array([[0.5, 0.75, 0.75, 0.25, 0.75, 0.9, 0.1, 0.75, 0.2]])
OFF = np.array([0, 3, 4, 7, 9])
ALL = [[0, 1, 2, 3]]


def _ref(mask, groups=ALL):
    sc, rows, rk = K.group_rank_ref(S, OFF, None if mask is None else np.asarray(mask, dtype=bool), groups)
    return sc[0].tolist(), rows[0].tolist(), rk[0].tolist()


def test_ranks_are_the_inverse_of_the_window_and_a_tie_goes_to_the_lower_group():
    # documents 0 and 3 tie at .75: the lower group is ahead
    assert _ref(None) == ([0.75, 0.25, 0.9, 0.75], [1, 3, 5, 7], [1, 3, 0, 2])
    assert _ref(None, [[3, 3, 0]]) == ([0.75, 0.75, 0.75], [7, 7, 1], [2, 2, 1])          # duplicates allowed
    sc, rows, gr = G.group_window_ref(S, OFF, None, 0, 4)
    a = K.group_rank_ref(S, OFF, None, gr)
    assert a[2][0].tolist() == [0, 1, 2, 3] and np.array_equal(a[0], sc) and np.array_equal(a[1], rows)


def test_an_absent_target_gets_the_tail_triple_and_the_others_close_ranks():
    mask = [1, 1, 1, 0, 1, 1, 1, 1, 1]                                    # document 1 has no allowed page
    assert _ref(mask) == ([0.75, -np.inf, 0.9, 0.75], [1, -1, 5, 7], [1, -1, 0, 2])
    mask = [0, 0, 0, 1, 1, 1, 1, 1, 1]                                    # document 0 absent: 3 moves up
    assert _ref(mask) == ([-np.inf, 0.25, 0.9, 0.75], [-1, 3, 5, 7], [-1, 2, 0, 1])
    assert _ref(np.zeros(9)) == ([-np.inf] * 4, [-1] * 4, [-1] * 4)


def test_a_forbidden_best_page_changes_score_best_row_and_rank():
    mask = [1, 1, 1, 1, 1, 0, 1, 1, 1]                                    # row 5 (best of document 2) forbidden: .9 -> .75 (row 4)
    assert _ref(mask) == ([0.75, 0.25, 0.75, 0.75], [1, 3, 4, 7], [0, 3, 1, 2])
    mask = [1, 0, 1, 1, 0, 0, 1, 1, 1]                                    # document 0 answers with row 2; document 2 drops to .1: last
    assert _ref(mask) == ([0.75, 0.25, 0.1, 0.75], [2, 3, 6, 7], [0, 2, 3, 1])


def test_counts_at_a_tied_score_strict_and_negative_zero():
    S32 = S.astype(np.float32)                                            # thresholds are fp32 values: so are the scores here
    t = [[0.75, 0.9, 0.25, 1.0, 0.0]]
    assert K.group_count_ref(S32, OFF, None, t)[0].tolist() == [3, 1, 4, 0, 4]
    assert K.group_count_ref(S32, OFF, None, t, strict=True)[0].tolist() == [1, 0, 3, 0, 4]
    mask = np.asarray([1, 1, 1, 0, 1, 0, 1, 1, 1], dtype=bool)           # document 1 absent, document 2 drops to .75
    assert K.group_count_ref(S32, OFF, mask, t)[0].tolist() == [3, 0, 3, 0, 3]
    assert K.group_count_ref(S32, OFF, mask, t, strict=True)[0].tolist() == [0, 0, 3, 0, 3]
    z = np.array([[0.0, -0.0, -1.0, 1.0]], dtype=np.float32)              # four documents of one row; -0.0 counts as +0.0
    for t0 in (0.0, -0.0):
        assert K.group_count_ref(z, np.arange(5), None, [[t0]])[0].tolist() == [3]
        assert K.group_count_ref(z, np.arange(5), None, [[t0]], strict=True)[0].tolist() == [1]
    # ... while the RANKING tells the two zeros apart, as the library's keys do
    assert K.group_rank_ref(z, np.arange(5), None, [[0, 1, 2, 3]])[2][0].tolist() == [1, 2, 3, 0]
    # the count at a document's own score is its rank + 1 + the later members of its tie tier
    rk = K.group_rank_ref(S32, OFF, None, ALL)
    assert K.group_count_ref(S32, OFF, None, rk[0])[0].tolist() == [3, 4, 1, 3]
    assert K.group_count_ref(S32, OFF, None, rk[0], strict=True)[0].tolist() == [1, 3, 0, 1]


def test_fp32_scores_rank_on_their_orderable_bits():
    a, b = K.group_rank_ref(S.astype(np.float32), OFF, None, ALL), K.group_rank_ref(S, OFF, None, ALL)
    assert a[0].dtype == np.float32 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_check_ranks_accepts_a_near_tie_swap_and_nothing_else():
    s = np.array([[0.9, 0.1, 0.5, 0.2, 0.5 + 4e-7, 0.0, 0.3, 0.1]])     # four documents of two rows: .9, .5, .5 + 4e-7, .3
    off = np.arange(0, 9, 2)
    f32 = lambda *x: np.asarray([x], dtype=np.float32)                   # noqa: E731
    g = [[0, 1, 2, 3]]
    assert K.check_ranks(s, off, None, g, f32(.9, .5, .5, .3), [[0, 2, 4, 6]], [[0, 2, 1, 3]])[1::2] == (0, None)
    assert K.check_ranks(s, off, None, g, f32(.9, .5, .5, .3), [[0, 2, 4, 6]], [[0, 1, 2, 3]])[1::2] == (2, None)     # 4e-7 apart: may trade places
    assert K.check_ranks(s, off, None, g, f32(.9, .5, .5, .3), [[0, 2, 4, 6]], [[0, 3, 1, 2]])[3] is not None         # ... 0.2 apart: may not
    assert K.check_ranks(s, off, None, g, f32(.9, .5, .5, .3), [[0, 3, 4, 6]], [[0, 2, 1, 3]])[3] is not None         # a best row that is not the best
    assert K.check_ranks(s, off, None, g, f32(.9, .5001, .5, .3), [[0, 2, 4, 6]], [[0, 2, 1, 3]])[3] is not None      # a score 1e-4 off
    mask = np.ones(8, dtype=bool); mask[6:] = False                      # document 3 absent: only the tail triple will do
    assert K.check_ranks(s, off, mask, g, f32(.9, .5, .5, -np.inf), [[0, 2, 4, -1]], [[0, 2, 1, -1]])[3] is None
    assert K.check_ranks(s, off, mask, g, f32(.9, .5, .5, .3), [[0, 2, 4, 6]], [[0, 2, 1, 3]])[3] == (0, 3, pytest.approx(.3), 6, 3)


@pytest.mark.parametrize("name", list(K.TABLE))
def test_intervals_of_the_reference_ranks(name):
    """the 6e-7 table of the GPU test: (pairs, absent targets, widened intervals, widest) per filter of the corpus' rows in
    group_window_search_ref.TABLE; targets: every 7th document and the reference's top 20 per query"""
    C, Q, off, S_ = G.case(name)
    assert [d for d, _ in K.TABLE[name]] == K.table_rows(name)
    for density, want in K.TABLE[name]:
        assert K.interval_table(S_, off, G.case_mask(name, density)) == want, density
    assert set(K.TABLE) == set(G.TABLE)


# ------------------------------------------------------------------------------------------------ host helpers ---
def test_never_retrieved_with_the_three_metrics():
    ranks, lims = np.array([3, -1, -1, 0, -1]), np.array([0, 2, 3, 3, 5])       # query 1: its only positive absent; query 2: none
    with pytest.raises(ValueError):
        reciprocal_ranks(ranks, lims)
    r = never_retrieved(ranks)
    assert r.dtype == np.int64 and r.tolist() == [3, NEVER_RETRIEVED, NEVER_RETRIEVED, 0, NEVER_RETRIEVED] and NEVER_RETRIEVED == 1 << 62
    assert ranks.tolist() == [3, -1, -1, 0, -1]                           # a copy
    assert reciprocal_ranks(r, lims, cutoff=10 ** 12).tolist() == [0.25, 0.0, 0.0, 1.0]
    rr = reciprocal_ranks(r, lims)
    assert rr[[0, 2, 3]].tolist() == [0.25, 0.0, 1.0] and 0.0 < rr[1] < 1e-18
    assert mrr_from_ranks(r, lims) == pytest.approx(1.25 / 4, abs=1e-15)
    assert recall_at(r, lims, [1, 4, 1 << 61]).tolist() == pytest.approx([0.5 / 3, 1.0 / 3, 1.0 / 3])
    assert never_retrieved(np.array([[2, -1]])).shape == (1, 2) and never_retrieved([]).shape == (0,)
    with pytest.raises(ValueError):
        never_retrieved([0, -2])


class RankHostIndex(HostIndex):
    """HostIndex with the reference's rank_groups"""

    def rank_groups(self, Q, groups, lims=None, filter_of_query=None):
        assert self.n_groups
        HostIndex.calls.append(("rank_groups", filter_of_query is not None))
        S_ = R.scores64(Q, self.C).astype(np.float32)
        groups = np.asarray(groups, dtype=np.int64)
        assert ((groups >= 0) & (groups < self.n_groups)).all()
        mask = None
        if filter_of_query is not None:
            f = np.broadcast_to(np.asarray(filter_of_query, dtype=np.int64), (len(S_),))
            assert self.n_filters and ((f >= -1) & (f < self.n_filters)).all()
            mask = np.stack([np.ones(len(self.C), dtype=bool) if i < 0 else self.masks[i] for i in f])
        if lims is None:
            out = K.group_rank_ref(S_, self.off, mask, groups.reshape(len(S_), -1))
            return tuple(x.reshape(groups.shape) for x in out)
        outs = [np.empty(len(groups), dtype=d) for d in (np.float32, np.int64, np.int64)]
        for q in range(len(S_)):
            part = K.group_rank_ref(S_[q:q + 1], self.off, None if mask is None else mask[q:q + 1], groups[None, lims[q]:lims[q + 1]])
            for o, p in zip(outs, part):
                o[lims[q]:lims[q + 1]] = p[0]
        return tuple(outs)


def test_demo_explain_documents(tmp_path):
    kb, C, names = _base(tmp_path)
    ix = RankHostIndex(64, len(C)); ix.add(C)
    qvec = R.unit(6, 64, 5)[2:3]
    doc = lambda p: demo.doc_of_page(os.path.basename(p))                # noqa: E731
    p46, s46 = demo.retrieve_documents(kb, qvec, 46, None, None, index=ix, names=names, return_scores=True)
    every = [doc(p) for p in p46]
    HostIndex.calls = []
    out = demo.explain_documents(kb, qvec, every, index=ix, names=names)
    assert HostIndex.calls == [("rank_groups", False)]
    assert [r for _, _, r in out] == list(range(46))
    assert [s for s, _, _ in out] == s46 and [os.path.join(kb, p) for _, p, _ in out] == p46
    assert demo.explain_documents(kb, qvec, every[7], index=ix, names=names) == out[7]                 # one name: one triple
    assert demo.explain_documents(kb, qvec, [], index=ix, names=names) == []
    docs = ["deck_2.pdf", "other_7.pdf", "deck_4.pdf"]
    only, so = demo.retrieve_documents(kb, qvec, 10, None, None, index=ix, names=names, documents=docs, return_scores=True)
    HostIndex.calls = []
    got = demo.explain_documents(kb, qvec, docs + ["deck_0.pdf"], documents=docs, index=ix, names=names)
    assert HostIndex.calls == [("rank_groups", True)] and ix.n_filters == 1
    assert got[3][1] is None and got[3][2] == -1 and got[3][0] == -np.inf                              # outside the restriction
    by_rank = sorted(got[:3], key=lambda t: t[2])
    assert [t[2] for t in by_rank] == [0, 1, 2]
    assert [os.path.join(kb, t[1]) for t in by_rank] == only and [t[0] for t in by_rank] == so
    with pytest.raises(ValueError, match="nowhere.pdf"):
        demo.explain_documents(kb, qvec, ["deck_2.pdf", "nowhere.pdf"], index=ix, names=names)
    with pytest.raises(ValueError, match="nowhere.pdf"):
        demo.explain_documents(kb, qvec, ["deck_2.pdf"], documents=["nowhere.pdf"], index=ix, names=names)
    scattered = RankHostIndex(64, len(C)); scattered.add(C[::-1])
    with pytest.raises(ValueError, match="not adjacent"):
        demo.explain_documents(kb, qvec, ["deck_2.pdf"], index=scattered, names=names[::2] + names[1::2])
    assert demo.explain_documents(str(tmp_path / "missing"), qvec, docs) is None


def test_rank_documents_over_pickle_shards(tmp_path):
    """three shards, the pages of a deck spread over them; qrels that name documents; with and without collections"""
    _, C, names = _base(tmp_path)
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(C))                                        # pages of a document are neither adjacent nor in one shard
    Cp, pids = C[perm], [names[i] for i in perm]
    bounds = (0, 20, 55, 70)
    for s in range(3):
        write_shard(str(tmp_path / f"embeddings.corpus.rank.{s}"), Cp[bounds[s]:bounds[s + 1]], pids[bounds[s]:bounds[s + 1]])
    Q = R.unit(5, 64, 42)
    qids = [f"q{q}" for q in range(5)]
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, qids)
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    everything, best_page = retriever.retrieve_documents(args, 46, demo.doc_of_page, index_factory=RankHostIndex)
    qrels = {"q0": ["deck_1.pdf", "other_3.pdf"], "q1": ["deck_0.pdf", "deck_0.pdf", "other_8.pdf"], "q3": list(everything["q3"]), "q4": ["other_39.pdf"]}
    HostIndex.calls = []
    got = retriever.rank_documents(args, qrels, demo.doc_of_page, index_factory=RankHostIndex)
    assert HostIndex.calls == [("rank_groups", False)]                    # ONE index over all shards, one call, no filter
    assert got["q2"] == {} and list(got["q1"]) == ["deck_0.pdf", "other_8.pdf"]
    for q, docs in qrels.items():
        order = list(everything[q])
        for d in dict.fromkeys(docs):
            assert got[q][d] == (everything[q][d], best_page[q][d], order.index(d)), (q, d)
    assert [got["q3"][d][2] for d in everything["q3"]] == list(range(46))
    # collections: a label per document, a label set per query; a named document outside the set is not in the ranking
    label_of_doc = lambda d: "decks" if d.startswith("deck") else ("odd" if int(d.split("_")[1].split(".")[0]) % 2 else "even")      # noqa: E731
    wanted = {"q0": None, "q1": {"decks"}, "q2": {"odd"}, "q3": {"odd", "decks"}, "q4": {"none-such"}}
    HostIndex.calls = []
    got = retriever.rank_documents(args, lambda q: qrels.get(q, ()), demo.doc_of_page, label_of_doc, lambda q: wanted[q], index_factory=RankHostIndex)
    assert HostIndex.calls == [("rank_groups", True)]
    for q, docs in qrels.items():
        allowed = [d for d in everything[q] if wanted[q] is None or label_of_doc(d) in wanted[q]]
        for d in dict.fromkeys(docs):
            if d in allowed:
                assert got[q][d] == (everything[q][d], best_page[q][d], allowed.index(d)), (q, d)
            else:
                assert got[q][d] == (-np.inf, None, -1), (q, d)
    assert got["q1"]["other_8.pdf"][2] == -1 and got["q4"] == {"other_39.pdf": (-np.inf, None, -1)}
    with pytest.raises(ValueError, match="nowhere.pdf"):
        retriever.rank_documents(args, {"q0": ["nowhere.pdf"]}, demo.doc_of_page, index_factory=RankHostIndex)
    with pytest.raises(ValueError):
        retriever.rank_documents(args, qrels, demo.doc_of_page, label_of_doc, None, index_factory=RankHostIndex)
    assert retriever.rank_documents(args, {}, demo.doc_of_page, index_factory=RankHostIndex) == {q: {} for q in qids}


# ------------------------------------------------------------------------------------------------ declarations ---
def test_the_three_symbols_are_declared_in_every_layer():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from visrag_amd import _lib, build
    from visrag_amd.engine import HipIndex
    header = open(os.path.join(root, "include", "visrag_hip.h")).read()
    for name in ("vr_index_rank_groups", "vr_index_count_groups_range", "vr_index_group_rank_search_stats"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vr_index_rank_groups"][1]) == 11 and len(_lib.SIGNATURES["vr_index_count_groups_range"][1]) == 10
    assert len(_lib.SIGNATURES["vr_index_group_rank_search_stats"][1]) == 3
    assert "search_group_rank.hip" in build.SOURCES
    assert build.SOURCES.index("search_group_rank.hip") < build.SOURCES.index("index.hip")
    assert callable(HipIndex.rank_groups) and callable(HipIndex.count_groups_range) and callable(HipIndex.group_rank_search_stats)
    assert callable(demo.explain_documents) and callable(retriever.rank_documents)
