"""The numpy reference of the document range search (tests/group_range_search_ref.py) on hand-worked cases, what it alone says on
the corpora of tests/test_gpu_group_range_search.py (entries, and no pair near its threshold), the host helpers
(documents.split_document_ranges, demo.retrieve_documents_above, retriever.retrieve_documents_range over a host stand-in for the
index) and the declarations of the three ABI symbols.  No GPU, no library."""
import os
import types

import numpy as np
import pytest

from tests import group_range_search_ref as N
from tests import group_search_ref as R
from tests import group_window_search_ref as G
from tests.test_cpu_group_window_search_ref import HostIndex, _base
from visrag_amd import demo, retriever
from visrag_amd.documents import split_document_ranges
from visrag_amd.utils import write_shard

# one query, nine pages in four documents
#   document 0 = rows 0-2 (.5, .75, .75)   document 1 = row 3 (.25)   document 2 = rows 4-6 (.75, .9, .1)   document 3 = rows 7-8 (.75, .2)
S = np.array([[0.5, 0.75, 0.75, 0.25, 0.75, 0.9, 0.1, 0.75, 0.2]])
OFF = np.array([0, 3, 4, 7, 9])


def _ref(mask, t, sort=False, S_=S, off=OFF):
    lims, sc, rows, gr = N.group_range_ref(S_, off, None if mask is None else np.asarray(mask, dtype=bool), t, sort)
    return lims.tolist(), sc.tolist(), rows.tolist(), gr.tolist()


def test_group_order_sorted_order_and_a_threshold_on_a_tied_tier():
    # documents 0 and 3 tie at .75: a threshold AT the tier takes both, in group order from the ABI, the lower group first when sorted
    assert _ref(None, 0.75) == ([0, 3], [0.75, 0.9, 0.75], [1, 5, 7], [0, 2, 3])
    assert _ref(None, 0.75, sort=True) == ([0, 3], [0.9, 0.75, 0.75], [5, 1, 7], [2, 0, 3])
    above = np.nextafter(np.float32(0.75), np.float32(1))                 # the next float above the tier: the tier is out
    assert _ref(None, above) == ([0, 1], [0.9], [5], [2])
    assert _ref(None, 0.0)[3] == [0, 1, 2, 3] and _ref(None, 0.0, sort=True)[3] == [2, 0, 3, 1]
    # the sorted order is search_groups_window's
    sc, rows, gr = G.group_window_ref(S, OFF, None, 0, 4)
    assert _ref(None, 0.0, sort=True)[1:] == (sc[0].tolist(), rows[0].tolist(), gr[0].tolist())


def test_an_absent_document_and_an_empty_result():
    mask = [1, 1, 1, 0, 1, 1, 1, 1, 1]                                    # document 1 has no allowed page: below every threshold
    assert _ref(mask, -4.0) == ([0, 3], [0.75, 0.9, 0.75], [1, 5, 7], [0, 2, 3])
    assert _ref(np.zeros(9), -4.0) == ([0, 0], [], [], [])
    assert _ref(None, 1.0) == ([0, 0], [], [], [])                        # nothing reaches 1.0
    out = N.group_range_ref(S.astype(np.float32), OFF, None, 1.0)
    assert out[0].dtype == np.int64 and out[1].dtype == np.float32 and out[2].dtype == np.int64 and out[3].dtype == np.int64


def test_a_forbidden_best_page_takes_a_document_below_the_threshold():
    assert _ref(None, 0.8) == ([0, 1], [0.9], [5], [2])
    mask = [1, 1, 1, 1, 1, 0, 1, 1, 1]                                    # row 5 (best of document 2) forbidden: .9 -> .75 (row 4)
    assert _ref(mask, 0.8) == ([0, 0], [], [], [])
    assert _ref(mask, 0.75) == ([0, 3], [0.75, 0.75, 0.75], [1, 4, 7], [0, 2, 3])


def test_the_best_row_is_the_lowest_allowed_tied_row():
    mask = [1, 0, 1, 1, 0, 0, 1, 1, 1]                                    # document 0 answers with row 2; document 2 drops to .1
    assert _ref(mask, 0.5) == ([0, 2], [0.75, 0.75], [2, 7], [0, 3])
    assert _ref(mask, 0.0625) == ([0, 4], [0.75, 0.25, 0.1, 0.75], [2, 3, 6, 7], [0, 1, 2, 3])


def test_negative_zero_thresholds_of_several_queries_and_per_query_masks():
    z = np.array([[0.0, -0.0, -1.0, 1.0]], dtype=np.float32)              # four documents of one row; -0.0 counts as +0.0
    for t0 in (0.0, -0.0):
        assert _ref(None, t0, S_=z, off=np.arange(5))[3] == [0, 1, 3]
        assert _ref(None, t0, True, S_=z, off=np.arange(5))[3] == [3, 0, 1]      # ... while the ORDER tells the two zeros apart
    S2 = np.concatenate([S, S[:, ::-1]])
    mask = np.ones((2, 9), dtype=bool)
    mask[1, :5] = False                                                   # query 1 (the scores reversed): documents 0 and 1 absent,
    lims, sc, rows, gr = N.group_range_ref(S2, OFF, mask, [0.75, 0.2])    # document 2 by rows 5-6 (.25, .75), document 3 = (.75, .5)
    assert lims.tolist() == [0, 3, 5] and gr.tolist() == [0, 2, 3, 2, 3] and rows.tolist() == [1, 5, 7, 6, 7]
    assert sc.tolist() == [0.75, 0.9, 0.75, 0.75, 0.75]
    with pytest.raises(AssertionError):
        N.group_range_ref(S2, OFF, None, [0.1, 0.2, 0.3])


def test_check_range_excuses_a_pair_at_the_threshold_and_nothing_else():
    s = np.array([[0.9, 0.1, 0.5, 0.2, 0.5 + 2e-7, 0.0, 0.3, 0.1]])     # four documents of two rows: .9, .5, .5 + 2e-7, .3
    off = np.arange(0, 9, 2)
    t = np.float32(0.5)
    f32 = lambda *x: np.asarray(x, dtype=np.float32)                      # noqa: E731
    assert N.check_range(s, off, None, t, [0, 3], f32(.9, .5, .5), [0, 2, 4], [0, 1, 2])[::3] == (3, None)
    assert N.check_range(s, off, None, t, [0, 2], f32(.9, .5), [0, 4], [0, 2])[:2] == (3, 1)            # 0 from the threshold: excused
    assert N.check_range(s, off, None, t, [0, 1], f32(.9), [0], [0])[1::2] == (2, None)
    assert N.check_range(s, off, None, t, [0, 4], f32(.9, .5, .5, .3), [0, 2, 4, 6], [0, 1, 2, 3])[3] is not None      # .2 below: not
    assert N.check_range(s, off, None, t, [0, 2], f32(.5, .5), [2, 4], [1, 2])[3] is not None           # the best document missing
    assert N.check_range(s, off, None, t, [0, 3], f32(.9, .5, .5), [0, 3, 4], [0, 1, 2])[3] is not None       # a best row that is not the best
    assert N.check_range(s, off, None, t, [0, 3], f32(.9, .5001, .5), [0, 2, 4], [0, 1, 2])[3] is not None    # a score 1e-4 off
    mask = np.ones(8, dtype=bool); mask[0] = False                        # document 0 by its second row: .1
    assert N.check_range(s, off, mask, t, [0, 2], f32(.5, .5), [2, 4], [1, 2])[3] is None
    assert N.check_range(s, off, mask, np.float32(0.1), [0, 4], f32(.1, .5, .5, .3), [0, 2, 4, 6], [0, 1, 2, 3])[3] is not None      # a forbidden row
    assert N.near_threshold(s, off, None, t) == 2 and N.near_threshold(s, off, None, 0.4) == 0


@pytest.mark.parametrize("name", list(N.TABLE))
def test_entries_of_the_reference_and_no_pair_near_its_threshold(name):
    """the table of the GPU test: entries without a filter / under the density-0.5 filter, per-query (min, median, max), and that
    no (query, document) pair of the reference lies within 3e-7 of its threshold: the excuse of the fp64 bar is not needed"""
    C, Q, off, S_ = G.case(name)
    cycle, plain, filtered, spread = N.TABLE[name]
    t = N.case_thresholds(name, len(Q))
    assert t.dtype == np.float32 and t[:len(cycle)].tolist() == [np.float32(c) for c in cycle]
    lims = N.group_range_ref(S_, off, None, t)[0]
    d = np.diff(lims)
    assert lims[-1] == plain and (int(d.min()), int(np.median(d)), int(d.max())) == spread
    mask = G.case_mask(name, 0.5)
    assert N.group_range_ref(S_, off, mask, t)[0][-1] == filtered
    assert N.near_threshold(S_, off, None, t) == 0 and N.near_threshold(S_, off, mask, t) == 0
    assert set(N.TABLE) == set(G.TABLE)


# ------------------------------------------------------------------------------------------------ host helpers ---
def test_split_document_ranges():
    lims, sc, rows, gr = N.group_range_ref(np.concatenate([S, S, S]), OFF, None, [0.75, 1.0, 0.8])
    parts = split_document_ranges(lims, sc, rows, gr)
    assert [tuple(x.tolist() for x in p) for p in parts] == [([0.75, 0.9, 0.75], [1, 5, 7], [0, 2, 3]), ([], [], []), ([0.9], [5], [2])]
    assert parts[0][0].base is not None                                   # views
    assert split_document_ranges([0], [], [], []) == []
    for bad in (([1, 4], sc, rows, gr), ([0, 3, 2, 4], sc, rows, gr), ([0, 3], sc, rows, gr), (lims, sc[:3], rows, gr), (lims, sc, rows[:3], gr)):
        with pytest.raises(ValueError):
            split_document_ranges(*bad)


class RangeHostIndex(HostIndex):
    """HostIndex with the reference's search_groups_range"""

    def search_groups_range(self, Q, threshold, filter_of_query=None, max_total=None, sort=True):
        assert self.n_groups
        HostIndex.calls.append(("groups_range", filter_of_query is not None))
        S_ = R.scores64(Q, self.C).astype(np.float32)
        mask = None
        if filter_of_query is not None:
            f = np.broadcast_to(np.asarray(filter_of_query, dtype=np.int64), (len(S_),))
            assert self.n_filters and ((f >= -1) & (f < self.n_filters)).all()
            mask = np.stack([np.ones(len(self.C), dtype=bool) if i < 0 else self.masks[i] for i in f])
        return N.group_range_ref(S_, self.off, mask, threshold, sort)


def test_demo_retrieve_documents_above(tmp_path):
    kb, C, names = _base(tmp_path)
    ix = RangeHostIndex(64, len(C)); ix.add(C)
    qvec = R.unit(6, 64, 5)[2:3]
    p46, s46 = demo.retrieve_documents(kb, qvec, 46, None, None, index=ix, names=names, return_scores=True)
    cut = float(np.float32(s46[11]))
    HostIndex.calls = []
    p, s = demo.retrieve_documents_above(kb, qvec, cut, None, None, index=ix, names=names, return_scores=True)
    assert HostIndex.calls == [("groups_range", False)]
    assert p == p46[:12] and s == s46[:12]                                # best document first, the best page of each
    assert demo.retrieve_documents_above(kb, qvec, cut, None, None, index=ix, names=names) == p46[:12]
    assert demo.retrieve_documents_above(kb, qvec, -4.0, None, None, index=ix, names=names) == p46
    assert demo.retrieve_documents_above(kb, qvec, 2.0, None, None, index=ix, names=names) == []
    assert demo.retrieve_documents_above(kb, qvec, cut, None, None, index=ix, names=names, max_documents=5) == p46[:5]
    assert demo.retrieve_documents_above(kb, qvec, cut, None, None, index=ix, names=names, max_documents=0) == []
    docs = ["deck_2.pdf", "other_7.pdf", "deck_4.pdf"]
    only, so = demo.retrieve_documents(kb, qvec, 10, None, None, index=ix, names=names, documents=docs, return_scores=True)
    HostIndex.calls = []
    got = demo.retrieve_documents_above(kb, qvec, -4.0, None, None, index=ix, names=names, documents=docs, return_scores=True)
    assert HostIndex.calls == [("groups_range", True)] and ix.n_filters == 1          # one filter set for the question
    assert got == (only, so)
    got = demo.retrieve_documents_above(kb, qvec, float(np.float32(so[1])), None, None, index=ix, names=names, documents=docs)
    assert got == only[:2]
    with pytest.raises(ValueError, match="nowhere.pdf"):
        demo.retrieve_documents_above(kb, qvec, 0.0, None, None, index=ix, names=names, documents=["deck_2.pdf", "nowhere.pdf"])
    fresh = RangeHostIndex(64, len(C)); fresh.add(C)                      # an index without groups: they are set from the names
    assert demo.retrieve_documents_above(kb, qvec, cut, None, None, index=fresh, names=names) == p46[:12] and fresh.n_groups == 46
    scattered = RangeHostIndex(64, len(C)); scattered.add(C[::-1])
    with pytest.raises(ValueError, match="not adjacent"):
        demo.retrieve_documents_above(kb, qvec, 0.0, None, None, index=scattered, names=names[::2] + names[1::2])
    assert demo.retrieve_documents_above(str(tmp_path / "missing"), qvec, 0.0, None, None) is None


def test_retrieve_documents_range_over_pickle_shards(tmp_path):
    """three shards, the pages of a deck spread over them; with and without collections"""
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
    everything, best_page = retriever.retrieve_documents(args, 46, demo.doc_of_page, index_factory=RangeHostIndex)
    t = 0.05
    HostIndex.calls = []
    scores, pages = retriever.retrieve_documents_range(args, t, demo.doc_of_page, index_factory=RangeHostIndex)
    assert HostIndex.calls == [("groups_range", False)]                   # ONE index over all shards, one call, no filter
    total = 0
    for q in qids:
        want = [d for d, s_ in everything[q].items() if np.float32(s_) >= np.float32(t)]
        assert list(scores[q]) == want and list(pages[q]) == want         # best first: the order of the document ranking
        assert all(scores[q][d] == everything[q][d] and pages[q][d] == best_page[q][d] for d in want)
        total += len(want)
    assert 5 < total < 46 * 5
    assert retriever.retrieve_documents_range(args, 2.0, demo.doc_of_page, index_factory=RangeHostIndex) == ({q: {} for q in qids}, {q: {} for q in qids})
    top3, pg3 = retriever.retrieve_documents_range(args, -4.0, demo.doc_of_page, max_per_query=3, index_factory=RangeHostIndex)
    assert all(list(top3[q]) == list(everything[q])[:3] == list(pg3[q]) for q in qids)
    assert retriever.retrieve_documents_range(args, -4.0, demo.doc_of_page, max_per_query=0, index_factory=RangeHostIndex)[0] == {q: {} for q in qids}
    # collections: a label per document, a label set per query
    label_of_doc = lambda d: "decks" if d.startswith("deck") else ("odd" if int(d.split("_")[1].split(".")[0]) % 2 else "even")      # noqa: E731
    wanted = {"q0": None, "q1": {"decks"}, "q2": {"odd"}, "q3": {"odd", "decks"}, "q4": {"none-such"}}
    HostIndex.calls = []
    scores, pages = retriever.retrieve_documents_range(args, -4.0, demo.doc_of_page, label_of_doc, lambda q: wanted[q], index_factory=RangeHostIndex)
    assert HostIndex.calls == [("groups_range", True)]
    for q in qids:
        allowed = [d for d in everything[q] if wanted[q] is None or label_of_doc(d) in wanted[q]]
        assert list(scores[q]) == allowed and all(pages[q][d] == best_page[q][d] for d in allowed)
    assert scores["q4"] == {} and len(scores["q1"]) == 6
    with pytest.raises(ValueError):
        retriever.retrieve_documents_range(args, 0.0, demo.doc_of_page, label_of_doc, None, index_factory=RangeHostIndex)


# ------------------------------------------------------------------------------------------------ declarations ---
def test_the_three_symbols_are_declared_in_every_layer():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from visrag_amd import _lib, build
    from visrag_amd.engine import HipIndex
    header = open(os.path.join(root, "include", "visrag_hip.h")).read()
    for name in ("vr_index_search_groups_range", "vr_index_group_range_results", "vr_index_group_range_search_stats"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vr_index_search_groups_range"][1]) == 10 and len(_lib.SIGNATURES["vr_index_group_range_results"][1]) == 7
    assert len(_lib.SIGNATURES["vr_index_group_range_search_stats"][1]) == 3
    assert "search_group_range.hip" in build.SOURCES
    assert build.SOURCES.index("search_group_range.hip") < build.SOURCES.index("index.hip")
    assert callable(HipIndex.search_groups_range) and callable(HipIndex.group_range_search_stats)
    assert callable(demo.retrieve_documents_above) and callable(retriever.retrieve_documents_range) and callable(split_document_ranges)
    # the row loop of the document rank search is shared, not copied
    csrc = os.path.join(root, "visrag_amd", "csrc")
    defs = [f for f in sorted(os.listdir(csrc)) if "uint64_t group_best_row(" in open(os.path.join(csrc, f)).read()]
    assert defs == ["search_rescore.h"]
    walks = [f for f in sorted(os.listdir(csrc)) if f.startswith("search_") and "__ffsll" in open(os.path.join(csrc, f)).read()]
    assert walks == ["search_rescore.h", "search_select.h"]              # (search_select.h: select_kth's bin scan)
