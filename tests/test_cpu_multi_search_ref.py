"""The numpy reference of the fused search (tests/multi_search_ref.py) on hand-worked cases, the widths of its fp64 intervals on
the layouts of tests/test_gpu_multi_search.py (the table that file's docstring states), the host helpers (documents.fuse_runs,
retriever.retrieve_fused over a host stand-in for the index) and the declarations of the two ABI symbols.  No GPU, no library."""
import os
import types

import numpy as np
import pytest

from tests import multi_search_ref as M
from tests import rank_search_ref as K
from tests.group_search_ref import scores64
from visrag_amd import retriever
from visrag_amd.documents import fuse_runs, group_rows
from visrag_amd.utils import write_shard

# three sub-queries, five rows; groups {0, 1} and {2}
S = np.array([[0.9, 0.2, 0.5, 0.5, 0.1],
              [0.1, 0.8, 0.5, 0.6, 0.1],
              [0.3, 0.3, 0.7, 0.3, 0.2]])
LIMS = np.array([0, 2, 3])


def test_layout_cycles_the_sizes():
    assert M.layout(37, (1, 2, 3, 4, 5, 6, 7, 9)).tolist() == [0, 1, 3, 6, 10, 15, 21, 28, 37]
    assert M.layout(8, (2, 3)).tolist() == [0, 2, 5, 7, 8]                # the last group takes what is left
    assert M.layout(3, (5,)).tolist() == [0, 3] and M.layout(0, (2,)).tolist() == [0]
    for name, (cycle, groups, _) in M.TABLE.items():
        assert len(M.layout(len(M.case(name)[1]), cycle)) - 1 == groups, name


def test_fused_scores_and_rankings():
    assert M.fuse_ref(S, LIMS, "max").tolist() == [[0.9, 0.8, 0.5, 0.6, 0.1], S[2].tolist()]
    assert M.fuse_ref(S, LIMS, "min").tolist() == [[0.1, 0.2, 0.5, 0.5, 0.1], S[2].tolist()]
    sc, ids, which = M.multi_ref(S, LIMS, 3, "max")
    assert ids.tolist() == [[0, 1, 3], [2, 0, 1]] and which.tolist() == [[0, 1, 1], [0, 0, 0]]
    assert sc.tolist() == [[0.9, 0.8, 0.6], [0.7, 0.3, 0.3]]
    sc, ids, which = M.multi_ref(S, LIMS, 4, "min")
    assert ids[0].tolist() == [2, 3, 1, 0] and which[0].tolist() == [0, 0, 0, 1]      # row 2: both score 0.5, the lower index named
    assert sc[0].tolist() == [0.5, 0.5, 0.2, 0.1]
    # a page at the top for one part and at the bottom for the other: ahead under any-of, behind under all-of
    assert M.multi_ref(S, LIMS, 1, "max")[1][0, 0] == 0 and M.multi_ref(S, LIMS, 5, "min")[1][0, 3] == 0


def test_tails_and_masks():
    sc, ids, which = M.multi_ref(S, LIMS, 7, "max")
    assert ids[0].tolist() == [0, 1, 3, 2, 4, -1, -1] and which[0, 5:].tolist() == [-1, -1] and np.isneginf(sc[0, 5:]).all()
    mask = [np.array([0, 1, 1, 0, 1], dtype=bool), None]
    sc, ids, which = M.multi_ref(S, LIMS, 4, "max", mask)
    assert ids.tolist() == [[1, 2, 4, -1], [2, 0, 1, 3]] and which[0].tolist() == [1, 0, 0, -1]
    none = [np.zeros(5, dtype=bool), np.zeros(5, dtype=bool)]
    assert (M.multi_ref(S, LIMS, 2, "min", none)[1] == -1).all()


def test_check_group_accepts_a_near_tie_swap_and_nothing_else():
    s = np.array([[0.9, 0.5, 0.5 + 4e-7, 0.2, 0.1], [0.1, 0.1, 0.1, 0.2 - 3e-7, 0.05]])
    lims = np.array([0, 2])                                               # max: 0.9, 0.5, 0.5 + 4e-7, 0.2, 0.1 -> ranking 0, 2, 1, 3, 4
    assert M.check_group(s, lims, 0, "max", [0, 2, 1], [0, 0, 0]) == (3, 0, None)
    assert M.check_group(s, lims, 0, "max", [0, 1, 2], [0, 0, 0]) == (3, 2, None)      # the two rows 4e-7 apart may trade places
    assert M.check_group(s, lims, 0, "max", [0, 3, 1], [0, 0, 0])[2] is not None       # ... a row 0.3 away may not
    assert M.check_group(s, lims, 0, "max", [0, 2, 1, 3], [0, 0, 0, 1])[2] is None     # row 3: both sub-queries inside 6e-7
    assert M.check_group(s, lims, 0, "max", [0, 2, 1], [0, 0, 1])[2] is not None       # a sub-query 0.4 below the fused score
    assert M.check_group(s, lims, 0, "max", [0, 2, 1, 3, 4, -1], [0, 0, 0, 0, 0, -1]) == (5, 0, None)
    with pytest.raises(AssertionError):
        M.check_group(s, lims, 0, "max", [0, 2, -1], [0, 0, -1])          # a result that ends early
    with pytest.raises(AssertionError):
        M.check_group(s, lims, 0, "max", [0, 2, 2], [0, 0, 0])            # the duplicates of the merged-lists workaround


@pytest.mark.parametrize("name", list(M.TABLE))
def test_interval_widths_of_the_fused_rankings(name):
    """the 6e-7 table of the GPU test: (positions, widened intervals, max width) at k = 100, for max and for min; and no position
    has a second sub-query within TOL of the fused score: `which` is unambiguous on all of them"""
    S_ = M.case(name)[2]
    cycle, groups, want = M.TABLE[name]
    lims = M.layout(len(S_), cycle)
    assert len(lims) - 1 == groups
    for fuse in ("max", "min"):
        positions, widened, widest, gap = M.interval_table(S_, lims, M.K_FP64, fuse)
        assert (positions, widened, widest) == want[fuse], fuse
        assert gap > M.TOL, (fuse, gap)


# ------------------------------------------------------------------------------------------------ host helpers ---
def test_fuse_runs_any_of_is_determined_by_the_lists():
    # group {0, 1}: depth-3 lists of the hand-worked scores
    sc = np.array([[0.9, 0.5, 0.5], [0.8, 0.6, 0.5]], dtype=np.float32)
    ids = np.array([[0, 2, 3], [1, 3, 2]])
    s, i, ok = fuse_runs(sc, ids, [0, 2], 3, "max")
    assert i.tolist() == [[0, 1, 3]] and s.tolist() == [[np.float32(0.9), np.float32(0.8), np.float32(0.6)]] and ok.tolist() == [True]
    assert i[0].tolist() == M.multi_ref(S, LIMS, 3, "max")[1][0].tolist()
    # the merged lists hold duplicates (rows 2 and 3): four distinct rows from six entries; deeper than the lists: undetermined
    s, i, ok = fuse_runs(sc, ids, [0, 2], 5, "max")
    assert i.tolist() == [[0, 1, 3, 2, -1]] and np.isneginf(s[0, 4]) and ok.tolist() == [False]
    # lists that ended (a tail): every row is listed, determined at any k
    sc2 = np.array([[0.9, 0.5, -np.inf], [0.8, -np.inf, -np.inf]], dtype=np.float32)
    ids2 = np.array([[0, 2, -1], [1, -1, -1]])
    s, i, ok = fuse_runs(sc2, ids2, [0, 1, 2], 3, "max")
    assert i.tolist() == [[0, 2, -1], [1, -1, -1]] and ok.tolist() == [True, True]


def test_fuse_runs_all_of_needs_the_row_in_every_list():
    sc = np.array([[0.9, 0.5, 0.5], [0.8, 0.6, 0.5]], dtype=np.float32)
    ids = np.array([[0, 2, 3], [1, 3, 2]])
    # rows 2 and 3 stand in both lists: min 0.5 and 0.5; rows 0 and 1 in one list only: unknown, at most 0.5 (the other list's end)
    s, i, ok = fuse_runs(sc, ids, [0, 2], 2, "min")
    assert i.tolist() == [[2, 3]] and s.tolist() == [[0.5, 0.5]]
    assert ok.tolist() == [False]                  # 0.5 is not strictly above the bound 0.5: row 0 or 1 could tie and, with a lower id, lead
    assert M.multi_ref(S, LIMS, 2, "min")[1][0].tolist() == [2, 3]        # (here the truth agrees; the lists cannot know)
    # the issue's case: a row at the top of one list and deep in the other is in no intersection
    sc = np.array([[0.9, 0.8, 0.7], [0.95, 0.6, 0.5]], dtype=np.float32)
    ids = np.array([[5, 6, 7], [8, 5, 9]])
    s, i, ok = fuse_runs(sc, ids, [0, 2], 1, "min")
    assert i.tolist() == [[5]] and s.tolist() == [[np.float32(0.6)]] and ok.tolist() == [False]   # row 6 may score min(0.8, <= 0.5) ... and
    # row 8 min(0.95, <= 0.7) = up to 0.7 > 0.6: undetermined.  With both lists' ends below the candidate it is determined:
    sc = np.array([[0.9, 0.8, 0.3], [0.95, 0.6, 0.2]], dtype=np.float32)
    s, i, ok = fuse_runs(sc, ids, [0, 2], 1, "min")
    assert i.tolist() == [[5]] and ok.tolist() == [True]
    s, i, ok = fuse_runs(sc, ids, [0, 2], 2, "min")                        # ... but a second row is not there to return
    assert i.tolist() == [[5, -1]] and ok.tolist() == [False]
    # groups of one: the list itself, for either fusion
    for fuse in ("max", "min"):
        s, i, ok = fuse_runs(sc, ids, [0, 1, 2], 3, fuse)
        assert np.array_equal(i, ids) and np.array_equal(s, sc) and ok.all()
    with pytest.raises(ValueError):
        fuse_runs(sc, ids, [0, 0, 2], 1, "max")                           # an empty group
    with pytest.raises(ValueError):
        fuse_runs(sc, ids, [0, 2], 1, "sum")
    with pytest.raises(ValueError):
        fuse_runs(sc, ids, [0, 1], 1, "max")


def test_group_rows_makes_the_lims_of_sub_queries():
    order, lims, names = group_rows(["a", "b", "a", "c", "b", "a"])
    assert order.tolist() == [0, 2, 5, 1, 4, 3] and lims.tolist() == [0, 3, 5, 6] and names == ["a", "b", "c"]


class HostIndex:
    """stands in for HipIndex: the fused ranking over fp32-rounded fp64 scores, on the host"""
    calls = []

    def __init__(self, dim, capacity, device=0):
        self.C = np.zeros((0, dim), dtype=np.float32)

    def add(self, reps):
        self.C = np.concatenate([self.C, np.asarray(reps, dtype=np.float32)])

    def __len__(self):
        return len(self.C)

    def search_multi(self, Q, lims, k, fuse="max", filter_of_group=None):
        assert 1 <= k <= 1000 and filter_of_group is None and np.diff(lims).max() <= 256
        HostIndex.calls.append((len(self.C), len(Q), len(lims) - 1, int(k), fuse))
        sc, ids, which = M.multi_ref(scores64(Q, self.C).astype(np.float32), lims, k, fuse)
        return sc.astype(np.float32), ids, which

    def close(self):
        pass


def test_retrieve_fused_merges_the_shards_on_the_host(tmp_path):
    C, Q, bounds = K.shards_case()                                        # shards of 1 000, 3 001 and 1 999 rows, 9 queries
    names = [f"page_{i}" for i in range(len(C))]
    for s in range(3):
        write_shard(str(tmp_path / f"embeddings.corpus.rank.{s}"), C[bounds[s]:bounds[s + 1]], names[bounds[s]:bounds[s + 1]])
    qids = [f"t{q % 4}-part{q}" for q in range(len(Q))]                   # topics t0 (3 queries), t1, t2, t3 (2 each), interleaved
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, qids)
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    topic = lambda qid: qid.split("-")[0]
    order, lims, topics = group_rows([topic(q) for q in qids])
    assert topics == ["t0", "t1", "t2", "t3"] and np.diff(lims).tolist() == [3, 2, 2, 2]
    S_ = scores64(Q[order], C).astype(np.float32)
    for fuse in ("max", "min"):
        HostIndex.calls = []
        run = retriever.retrieve_fused(args, topic, 120, fuse, index_factory=HostIndex)
        assert HostIndex.calls == [(1000, 9, 4, 120, fuse), (3001, 9, 4, 120, fuse), (1999, 9, 4, 120, fuse)]
        sc, ids, _ = M.multi_ref(S_, lims, 120, fuse)
        assert list(run) == topics
        for g, t in enumerate(topics):
            assert list(run[t]) == [names[i] for i in ids[g]]             # equal scores across shards: the earlier position first
            assert list(run[t].values()) == [float(np.float32(s)) for s in sc[g]]
    deep = retriever.retrieve_fused(args, topic, 1000, "max", index_factory=HostIndex)
    F = M.fuse_ref(S_, lims, "max")
    assert any(F[0][K.ranking(F[0])[j]] == F[0][K.ranking(F[0])[j + 1]] for j in range(999))       # the copied rows tie inside it
    assert list(deep["t0"]) == [names[i] for i in K.ranking(F[0])[:1000]]
    assert retriever.retrieve_fused(args, topic, 0, "max", index_factory=HostIndex) == {t: {} for t in topics}
    one = retriever.retrieve_fused(args, lambda qid: qid, 5, "min", index_factory=HostIndex)       # groups of one: a plain run
    assert list(one) == qids and list(one[qids[3]]) == [names[i] for i in K.ranking(scores64(Q[3:4], C).astype(np.float32)[0])[:5]]


# ------------------------------------------------------------------------------------------------ declarations ---
def test_the_two_symbols_are_declared_in_every_layer():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from visrag_amd import _lib, build, demo
    from visrag_amd.engine import HipIndex
    header = open(os.path.join(root, "include", "visrag_hip.h")).read()
    for name in ("vr_index_search_multi", "vr_index_multi_search_stats"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vr_index_search_multi"][1]) == 13 and len(_lib.SIGNATURES["vr_index_multi_search_stats"][1]) == 3
    assert "search_multi.hip" in build.SOURCES and build.SOURCES.index("search_multi.hip") < build.SOURCES.index("index.hip")
    assert callable(HipIndex.search_multi) and callable(HipIndex.multi_search_stats)
    assert callable(retriever.retrieve_fused) and callable(demo.retrieve_any)
