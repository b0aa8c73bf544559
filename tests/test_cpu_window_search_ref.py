"""The numpy reference of the windowed search (tests/window_search_ref.py) on hand-worked cases, the widths of its fp64 intervals on
the corpora of tests/test_gpu_window_search.py (the table that file's docstring states), the host helpers (documents.
window_negatives, retriever.merge_pages_host / retrieve_deep / mine_negatives over a host stand-in for the index) and the
declarations of the two ABI symbols.  No GPU, no library."""
import os
import types

import numpy as np
import pytest

from tests import rank_search_ref as K
from tests import window_search_ref as W
from tests.group_search_ref import scores64, unit
from visrag_amd import retriever
from visrag_amd.documents import window_negatives
from visrag_amd.utils import write_shard

# one query, six rows: scores [.5, 1, .5, .25, 1, .5] -> ranking 1, 4, 0, 2, 5, 3
S = np.array([0.5, 1.0, 0.5, 0.25, 1.0, 0.5])


def test_window_is_a_slice_of_the_ranking_with_tails():
    assert W.window_ref(S, 0, 3)[1].tolist() == [1, 4, 0]
    assert W.window_ref(S, 2, 3)[1].tolist() == [0, 2, 5]                 # inside the tie tier: id order
    sc, ids = W.window_ref(S, 4, 4)
    assert ids.tolist() == [5, 3, -1, -1] and sc.tolist() == [0.5, 0.25, -np.inf, -np.inf]
    assert W.window_ref(S, 6, 2)[1].tolist() == [-1, -1] and W.window_ref(S, 11, 1)[1].tolist() == [-1]
    whole = np.concatenate([W.window_ref(S, o, 2)[1] for o in (0, 2, 4)])
    assert whole.tolist() == K.ranking(S).tolist()


def test_window_under_a_mask():
    mask = np.array([1, 0, 1, 1, 1, 0], dtype=bool)                       # allowed ranking: 4, 0, 2, 3
    assert W.window_ref(S, 0, 2, mask)[1].tolist() == [4, 0]
    assert W.window_ref(S, 3, 3, mask)[1].tolist() == [3, -1, -1]
    assert W.window_ref(S, 4, 1, mask)[1].tolist() == [-1]
    assert W.window_ref(S, 0, 2, np.zeros(6, dtype=bool))[1].tolist() == [-1, -1]


def test_intervals_are_the_rank_searchs():
    s = np.array([0.5, 0.5 + 4e-7, 0.5 - 4e-7, 0.5 + 7e-7, 0.2])
    lo, hi = W.intervals(s, s)
    assert [(int(a), int(b)) for a, b in zip(lo, hi)] == [K.interval(s, x) for x in s]
    assert K.interval(s, 0.5) == (1, 3) and W.TOL == 6e-7


def test_check_window_accepts_a_near_tie_swap_and_nothing_else():
    s = np.array([0.9, 0.5, 0.5 + 4e-7, 0.2, 0.1])                        # ranking 0, 2, 1, 3, 4
    assert W.check_window(s, [2, 1, 3], 1) == (3, 0, None)
    assert W.check_window(s, [1, 2, 3], 1) == (3, 2, None)                # the two rows 4e-7 apart may trade places
    assert W.check_window(s, [2, 3, 1], 1)[2] is not None                 # ... a row 0.3 away may not
    assert W.check_window(s, [3, 4, -1], 3) == (2, 0, None)
    with pytest.raises(AssertionError):
        W.check_window(s, [3, -1, -1], 3)                                 # a window that ends early


@pytest.mark.parametrize("name", list(W.TABLE))
def test_interval_widths_of_the_windows(name):
    """the 6e-7 table of the GPU test: (entries, widened intervals, max width) per offset at k = 100"""
    S_ = W.case(name)[2]
    for o, want in W.TABLE[name].items():
        assert W.interval_table(S_, o, W.K_FP64) == want, o
    widest = max(w[2] for w in W.TABLE[name].values())
    assert widest <= (4 if name == "unit-20000x64x2304" else 3)           # the rank test's 3 is exceeded once: the docstring says so


# ------------------------------------------------------------------------------------------------ host helpers ---
def test_window_negatives():
    ids = np.array([[7, 3, 9, 4, 1], [2, 5, -1, -1, -1], [8, 6, 0, -1, -1]])
    pos = [[3, 1], [], [8, 6, 0]]
    assert window_negatives(ids, pos, 2).tolist() == [[7, 9], [2, 5], [-1, -1]]
    assert window_negatives(ids, pos, 4).tolist() == [[7, 9, 4, -1], [2, 5, -1, -1], [-1, -1, -1, -1]]
    assert window_negatives(ids, lambda q: pos[q], 1).tolist() == [[7], [2], [-1]]
    out = window_negatives(ids, pos, 0)
    assert out.shape == (3, 0) and out.dtype == np.int64
    with pytest.raises(ValueError):
        window_negatives(ids, pos[:2], 2)
    with pytest.raises(ValueError):
        window_negatives(ids[0], pos, 2)
    with pytest.raises(ValueError):
        window_negatives(ids, pos, -1)


def test_merge_pages_host_orders_by_score_then_global_position():
    a_s, a_p = np.array([[0.9, 0.5, 0.5]], dtype=np.float32), np.array([[2, 0, 1]])
    b_s, b_p = np.array([[0.9, 0.5, -np.inf]], dtype=np.float32), np.array([[7, 5, -1]])
    sc, pos = retriever.merge_pages_host([a_s, b_s], [a_p, b_p], 4)
    assert pos.tolist() == [[2, 7, 0, 1]] and sc.tolist() == [[np.float32(0.9), np.float32(0.9), 0.5, 0.5]]
    sc, pos = retriever.merge_pages_host([a_s, b_s], [a_p, b_p], 7)
    assert pos.tolist() == [[2, 7, 0, 1, 5, -1, -1]] and sc[0, 5:].tolist() == [-np.inf, -np.inf]


class HostIndex:
    """stands in for HipIndex: the same ranking rule over fp32-rounded fp64 scores, on the host"""
    calls = []

    def __init__(self, dim, capacity, device=0):
        self.C = np.zeros((0, dim), dtype=np.float32)

    def add(self, reps):
        self.C = np.concatenate([self.C, np.asarray(reps, dtype=np.float32)])

    def __len__(self):
        return len(self.C)

    def _ranked(self, Q):
        S_ = scores64(Q, self.C).astype(np.float32)
        return S_, [K.ranking(row) for row in S_]

    def search_window(self, Q, offset, k, filter_of_query=None):
        assert 1 <= k <= 1000 and filter_of_query is None
        HostIndex.calls.append((len(self.C), int(offset), int(k)))
        S_, orders = self._ranked(Q)
        sc, ids = np.full((len(Q), k), -np.inf, dtype=np.float32), np.full((len(Q), k), -1, dtype=np.int64)
        for q, order in enumerate(orders):
            part = order[offset:offset + k]
            ids[q, :len(part)], sc[q, :len(part)] = part, S_[q][part]
        return sc, ids

    def search(self, Q, k):
        return self.search_window(Q, 0, k)

    def close(self):
        pass


def _shards(tmp_path, tag):
    """three corpus shards of 700, 1500 and 300 rows (30 rows of the first copied bit for bit into the last) and 5 queries"""
    C = unit(2500, 64, 41).copy()
    C[2200 + np.arange(30) * 7] = C[np.arange(30) * 11 + 3]
    Q = unit(5, 64, 42)
    bounds = (0, 700, 2200, 2500)
    names = [f"page_{i}" for i in range(len(C))]
    for s in range(3):
        write_shard(str(tmp_path / f"embeddings.corpus.rank.{s}"), C[bounds[s]:bounds[s + 1]], names[bounds[s]:bounds[s + 1]])
    qids = [f"q{q}" for q in range(len(Q))]
    write_shard(str(tmp_path / "embeddings.query.rank.0"), Q, qids)
    args = types.SimpleNamespace(output_dir=str(tmp_path), process_index=0, device="cuda:0")
    return C, Q, names, qids, args


def test_retrieve_deep_merges_paged_shards_on_the_host(tmp_path):
    C, Q, names, qids, args = _shards(tmp_path, "deep")
    whole = HostIndex(64, len(C)); whole.add(C)
    S_, orders = whole._ranked(Q)
    HostIndex.calls = []
    run = retriever.retrieve_deep(args, 1800, index_factory=HostIndex)
    # every shard paged in windows of <= 1000 down to min(depth, its rows)
    assert HostIndex.calls == [(700, 0, 700), (1500, 0, 1000), (1500, 1000, 500), (300, 0, 300)]
    for qi, q in enumerate(qids):
        assert list(run[q]) == [names[i] for i in orders[qi][:1800]]     # equal scores across shards: the earlier position first
        assert list(run[q].values()) == [float(s) for s in S_[qi][orders[qi][:1800]]]
    assert any(S_[qi][orders[qi][j]] == S_[qi][orders[qi][j + 1]] for qi in range(len(Q)) for j in range(1799))
    for depth in (10, 1000):
        assert retriever.retrieve_deep(args, depth, index_factory=HostIndex) == \
            retriever.distributed_parallel_retrieve(args, depth, global_topk=True, index_factory=HostIndex)
    deep = retriever.retrieve_deep(args, 4000, index_factory=HostIndex)
    assert all(len(deep[q]) == 2500 for q in qids)
    assert retriever.retrieve_deep(args, 0, index_factory=HostIndex) == {q: {} for q in qids}


def test_mine_negatives_takes_a_window_minus_the_positives(tmp_path):
    C, Q, names, qids, args = _shards(tmp_path, "neg")
    whole = HostIndex(64, len(C)); whole.add(C)
    _, orders = whole._ranked(Q)
    positives = {q: [names[i] for i in orders[qi][[0, 31, 35]]] for qi, q in enumerate(qids)}
    positives["q2"] = []
    got = retriever.mine_negatives(args, positives, 30, 20, index_factory=HostIndex)
    for qi, q in enumerate(qids):
        window = [names[i] for i in orders[qi][30:53]]
        assert got[q] == [d for d in window if d not in positives[q]][:20] and len(got[q]) == 20
    assert retriever.mine_negatives(args, lambda q: positives[q], 30, 20, index_factory=HostIndex) == got
    tail = retriever.mine_negatives(args, positives, 2490, 20, index_factory=HostIndex)
    assert all(tail[q] == [names[i] for i in orders[qi][2490:]] for qi, q in enumerate(qids))
    with pytest.raises(ValueError):
        retriever.mine_negatives(args, positives, -1, 5, index_factory=HostIndex)
    # one shard: the window itself is asked for, not everything above it
    one = tmp_path / "one"
    one.mkdir()
    write_shard(str(one / "embeddings.corpus.rank.0"), C, names)
    write_shard(str(one / "embeddings.query.rank.0"), Q, qids)
    args1 = types.SimpleNamespace(output_dir=str(one), process_index=0, device="cuda:0")
    HostIndex.calls = []
    assert retriever.mine_negatives(args1, positives, 30, 20, index_factory=HostIndex) == got
    assert HostIndex.calls == [(2500, 30, 23)]


# ------------------------------------------------------------------------------------------------ declarations ---
def test_the_two_symbols_are_declared_in_every_layer():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from visrag_amd import _lib, build
    from visrag_amd.engine import HipIndex
    header = open(os.path.join(root, "include", "visrag_hip.h")).read()
    for name in ("vr_index_search_window", "vr_index_window_search_stats"):
        assert f"int {name}(" in header and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["vr_index_search_window"][1]) == 10
    assert "search_window.hip" in build.SOURCES and build.SOURCES.index("search_window.hip") < build.SOURCES.index("index.hip")
    assert callable(HipIndex.search_window) and callable(HipIndex.window_search_stats)
