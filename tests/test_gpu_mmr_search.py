"""-m gpu: the diversified search (vr_index_search_diverse, csrc/search_diverse.hip) against the numpy reference
tests/mmr_search_ref.py.

Bars
  scores       every returned score within 1e-5 of the fp64 dot product of its query and row (the project's bar).
  eps-optimal  every pick t >= 1, GIVEN THE ROWS RETURNED BEFORE IT, has an fp64 objective v within 1e-6 of the best unselected
               member of the reference pool (M.walk).  r and m are each within 3e-7 of fp64, the weights sum to 1 and v takes
               three fp32 roundings at magnitude <= 1: under 5e-7 per objective, two objectives compared.  Pick 0 is a
               comparison of relevances alone: within NEAR_TIE = 3e-7 of the best (fp32 summation order, the bar of the other
               search tests).  A returned row belongs to the reference pool or scores within 3e-7 of its last member.
               No pick is exempt.
  strict       a query whose reference margin (the smallest gap between the best and the second-best v over its picks)
               exceeds 2e-6 returns the reference's ids exactly, in order; at least 90 % of a random case's queries are strict.

Reference near-ties (pinned by tests/test_cpu_mmr_search_ref.py), unit(nd, dim, 1) rows, unit(nq, dim, 2) queries:

    case (nd, nq, dim, k, pool, lam)       margins under 2e-6     pool-boundary gaps under 3e-7
    (5000, 37, 256, 10, 50, 0.5)           0 of 37                0
    (3001, 300, 128, 26, 100, 0.7)         7 of 300 (2.3 %)       0
    (20000, 64, 2304, 10, 100, 0.5)        2 of 64 (3.1 %)        1
    (1200, 2, 64, 100, 1000, 0.5)          0 of 2 (5e-6)          0
    (5000, 37, 256, 5, 20, 0.5)            0 of 37 (5.6e-6)       0
    (1200, 2, 64, 1000, 1000, 0.5)         2 of 2 (7e-8, 2.6e-7): eps-optimality and the id set only

The cases cover the 256-query block boundary (300 queries), the real dim (2304), pools on the fused sweep's depth (20) and on
the deep path (50 .. 1000), and an index added in two halves."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import filter_search_ref as F  # noqa: E402
from tests import group_search_ref as R  # noqa: E402
from tests import mmr_search_ref as M  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.documents import doc_of_page  # noqa: E402
from visrag_amd.engine import HipIndex, _stream_ptr  # noqa: E402

ATOL, NEAR_TIE, EPS_V, STRICT_MARGIN = 1e-5, 3e-7, 1e-6, 2e-6
VR_ERR_INVALID, VR_ERR_STATE = 1, 3


def _index(C, masks=None):
    ix = HipIndex(C.shape[1], len(C))
    ix.add(C[: len(C) // 2]); ix.add(C[len(C) // 2:])
    if masks is not None:
        ix.set_filters(masks)
    return ix


def _np(*xs):
    return [x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in xs]


def _same_bits(a, b):
    (s0, i0), (s1, i1) = _np(*a), _np(*b)
    return np.array_equal(s0.view(np.uint32), s1.view(np.uint32)) and np.array_equal(i0, i1)


def _check(got, Q, C, k, pool, lam, ref=None, masks=None, foq=None):
    """`got` under the bars of the module docstring -> the share of queries held to the reference's ids (ref given)"""
    sc, ids = _np(*got)
    assert sc.shape == (len(Q), k) and ids.shape == (len(Q), k) and sc.dtype == np.float32 and ids.dtype == np.int64
    none = ids < 0
    assert (ids[none] == -1).all() and np.isneginf(sc[none]).all()
    deficit, outside = M.walk(Q, C, ids, pool, lam, masks, foq)          # (also: no row twice, every row exists and is allowed)
    exact = np.einsum("qkd,qd->qk", C[np.where(none, 0, ids)].astype(np.float64), Q.astype(np.float64))
    err = np.abs(sc.astype(np.float64) - exact)[~none]
    print(f"k={k} pool={pool} lam={lam}: score error {err.max() if err.size else 0:.2e}, deficit pick 0 {np.nanmax(deficit[:, 0]):.2e}, "
          f"later picks {np.nanmax(deficit[:, 1:]) if k > 1 and not none[:, 1:].all() else 0:.2e}, outside {np.nanmax(outside):.2e}")
    assert (err <= ATOL).all()
    assert not (deficit[:, 0] > NEAR_TIE).any(), np.argwhere(deficit[:, 0] > NEAR_TIE)[:5]
    assert not (deficit[:, 1:] > EPS_V).any(), np.argwhere(deficit[:, 1:] > EPS_V)[:5]
    assert not (outside > NEAR_TIE).any(), np.argwhere(outside > NEAR_TIE)[:5]
    if ref is None:
        return None
    rs, ri, margins = ref
    strict = margins > STRICT_MARGIN
    bad = [q for q in np.flatnonzero(strict) if not np.array_equal(ids[q], ri[q])]
    print(f"   strict queries {int(strict.sum())} of {len(Q)}, of the others {int((ids[~strict] == ri[~strict]).all(1).sum())} identical too")
    assert not bad, (bad[:5], ids[bad[0]], ri[bad[0]])
    return float(strict.mean())


RANDOM_CASES = [(5000, 37, 256, 10, 50, 0.5), (3001, 300, 128, 26, 100, 0.7), (20000, 64, 2304, 10, 100, 0.5),
                (1200, 2, 64, 100, 1000, 0.5), (5000, 37, 256, 5, 20, 0.5)]


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("nd,nq,dim,k,pool,lam", RANDOM_CASES)
def test_random_unit_rows(nd, nq, dim, k, pool, lam, on_device):
    C, Q, ref = M.random_case(nd, nq, dim, k, pool, lam)
    ix = _index(C)
    if on_device:
        got = ix.search_diverse(torch.tensor(Q).cuda(), k, pool, lam)
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in got)
    else:
        got = ix.search_diverse(Q, k, pool, lam)
        assert all(isinstance(x, np.ndarray) for x in got)
    assert _check(got, Q, C, k, pool, lam, ref) >= 0.9
    ix.close()


def test_k_equal_pool_equal_1000():
    """1200 rows, dim 64, 2 queries: the reference's margins are 7e-8 and 2.6e-7 — near-ties are unavoidable at that depth, so
    no identity claim: every pick eps-optimal, and the id set is search(k = 1000)'s."""
    C, Q, _ = M.random_case(1200, 2, 64, 1000, 1000, 0.5)
    ix = _index(C)
    for q_in in (Q, torch.tensor(Q).cuda()):
        got = ix.search_diverse(q_in, 1000, 1000, 0.5)
        _check(got, Q, C, 1000, 1000, 0.5)
        plain = _np(*ix.search(q_in, 1000))
        assert np.array_equal(np.sort(_np(*got)[1], axis=1), np.sort(plain[1], axis=1))
        assert np.array_equal(_np(*got)[1][:, 0], plain[1][:, 0])
    ix.close()


@pytest.mark.parametrize("dim,noise", [(256, 1e-3), (2304, 3e-4)])
def test_near_duplicate_decks(dim, noise):
    """300 documents x 10 near-identical pages, 48 queries, k = 10, pool = 100, lam = 0.5: search(k = 10) returns pages of at
    most 2 documents, the diverse search of exactly 10, for every query.  The reference has 3 (dim 256) and 6 (dim 2304)
    queries with a margin under 2e-6, contests between the pages of one document: eps-optimality, no identity claim."""
    C, Q, ref = M.deck_case(dim, noise)
    ix = _index(C)
    plain = ix.search(Q, 10)[1] // 10
    assert max(len(set(d)) for d in plain.tolist()) <= 2
    for q_in in (Q, torch.tensor(Q).cuda()):
        got = ix.search_diverse(q_in, 10, 100, 0.5)
        _check(got, Q, C, 10, 100, 0.5)
        assert all(len(set(d)) == 10 for d in (_np(*got)[1] // 10).tolist())
    ix.close()


def test_exact_ties_go_to_the_lower_pool_position():
    """Rows i and i + 500 are bit-identical: equal relevance (the lower id ranks first in the pool) and, pick after pick, equal
    v — the twin with the lower id must be picked first, whichever wave scored which."""
    U = R.unit(500, 64, 1)
    C, Q = np.vstack([U, U]), R.unit(5, 64, 2)
    ix = _index(C)
    for q_in in (Q, torch.tensor(Q).cuda()):
        got = ix.search_diverse(q_in, 40, 200, 0.5)
        _check(got, Q, C, 40, 200, 0.5)
        for row in _np(*got)[1].tolist():
            assert all(i - 500 in row[:t] for t, i in enumerate(row) if i >= 500), row
    ix.close()


def test_lambda_edges():
    C, Q, _ = M.random_case(5000, 37, 256, 10, 50, 0.5)
    masks = F.random_filters(5000, (0.5, 0.05, 0.002), seed=11)
    foq = np.arange(len(Q)) % 4 - 1
    ix = _index(C, masks)
    for pool in (20, 50):                                                # the fused sweep's depth, the deep path
        for q_in in (Q, torch.tensor(Q).cuda()):
            ps, pi = _np(*ix.search(q_in, pool))
            assert _same_bits(ix.search_diverse(q_in, 10, pool, 1.0), (ps[:, :10], pi[:, :10]))
            fs, fi = _np(*ix.search_filtered(q_in, pool, foq))
            assert _same_bits(ix.search_diverse(q_in, 10, pool, 1.0, foq), (fs[:, :10], fi[:, :10]))
            got = ix.search_diverse(q_in, 10, pool, 0.0)
            assert np.array_equal(_np(*got)[1][:, 0], pi[:, 0])
            _check(got, Q, C, 10, pool, 0.0)
    ix.close()


def test_few_rows_and_filters():
    C7, Q7 = R.unit(7, 64, 1), R.unit(3, 64, 2)
    ix = HipIndex(64, 16)
    ix.add(C7)
    ref7 = M.mmr_ref(Q7, C7, 10, 20, 0.5)
    for q_in in (Q7, torch.tensor(Q7).cuda()):
        got = ix.search_diverse(q_in, 10, 20, 0.5)
        sc, ids = _np(*got)
        assert (ids[:, :7] >= 0).all() and (ids[:, 7:] == -1).all() and np.isneginf(sc[:, 7:]).all()
        _check(got, Q7, C7, 10, 20, 0.5, ref7)
    ix.close()
    # the 262-row and the 10-row filter (margins all above 4e-6: strict), a 3-row filter (fewer than k), -1 queries between them
    C, Q, _ = M.random_case(5000, 37, 256, 10, 50, 0.5)
    masks = np.vstack([F.random_filters(5000, (0.5, 0.05, 0.002), seed=11), np.zeros((1, 5000), dtype=bool)])
    masks[3, [17, 2500, 4999]] = True
    foq = np.array([1, 2, 3, -1] * 10)[: len(Q)]
    ref = M.mmr_ref(Q, C, 10, 50, 0.5, masks, foq)
    assert (ref[2][foq != 3] > 4e-6).all() and (ref[1][foq == 3][:, 3:] == -1).all() and (ref[1][foq == 3][:, :3] >= 0).all()
    for q_in, m_in in ((Q, masks), (torch.tensor(Q).cuda(), torch.tensor(masks).cuda())):
        ix = _index(C, m_in)
        got = ix.search_diverse(q_in, 10, 50, 0.5, foq)
        ids = _np(*got)[1]
        for q, f in enumerate(foq):
            assert f < 0 or masks[f][ids[q][ids[q] >= 0]].all()
        assert _check(got, Q, C, 10, 50, 0.5, ref, masks, foq) >= 0.9
        one = ix.search_diverse(q_in, 10, 50, 0.5, 3)                    # one filter for every query
        assert (_np(*one)[1][:, 3:] == -1).all() and (np.sort(_np(*one)[1][:, :3], axis=1) == [17, 2500, 4999]).all()
        ix.close()


def test_two_query_blocks_under_filters_and_the_empty_index():
    """600 rows (three 256-row tiles, the last partial), 257 queries (a second block of one query), a half-density and an empty
    filter, pool 20 (the plain pool is the fused sweep's, the filtered one the deep path's): query 256 is on filter 0.  After
    reset() the pool is empty: k tails for a host and a device caller, and a filter is a state error."""
    C, Q = R.unit(600, 64, 1), R.unit(257, 64, 2)
    masks = np.concatenate([F.random_filters(600, (0.5,), seed=11), np.zeros((1, 600), dtype=bool)])
    foq = np.arange(257) % 3 - 1                                         # -1 (no filter), 0, 1 (allows nothing), ...
    assert foq[256] == 0
    ref = M.mmr_ref(Q, C, 5, 20, 0.5, masks, foq)
    assert (ref[1][foq == 1] == -1).all() and (ref[1][foq != 1] >= 0).all()
    plain_ref = M.mmr_ref(Q, C, 5, 20, 0.5)
    ix = _index(C, masks)
    for q_in in (Q, torch.tensor(Q).cuda()):
        _check(ix.search_diverse(q_in, 5, 20, 0.5, foq), Q, C, 5, 20, 0.5, ref, masks, foq)
        _check(ix.search_diverse(q_in, 5, 20, 0.5), Q, C, 5, 20, 0.5, plain_ref)
    ix.reset()
    for q_in in (Q, torch.tensor(Q).cuda()):
        sc, ids = _np(*ix.search_diverse(q_in, 5, 20, 0.5))
        assert sc.shape == ids.shape == (257, 5) and (ids == -1).all() and np.isneginf(sc).all()
    assert _raw(ix, Q, 5, 20, 0.5, foq.astype(np.int32)) == (VR_ERR_STATE, True)
    ix.close()


def _raw(ix, Q, k, pool, lam, foq=None):
    """vr_index_search_diverse itself on host arrays whose outputs hold a sentinel -> (status, outputs untouched?)"""
    sc, ids = np.full((len(Q), max(k, 1)), 7.5, np.float32), np.full((len(Q), max(k, 1)), 77, np.int64)
    st = ix.lib.vr_index_search_diverse(ix._h, ctypes.c_void_p(Q.ctypes.data), len(Q), k, pool, lam,
                                        ctypes.c_void_p(None if foq is None else foq.ctypes.data), ctypes.c_void_p(sc.ctypes.data),
                                        ctypes.c_void_p(ids.ctypes.data), 0, ctypes.c_void_p(_stream_ptr(ix.device)))
    return st, bool((sc == 7.5).all() and (ids == 77).all())


def test_arguments_and_isolation():
    C, Q, _ = M.random_case(5000, 37, 256, 10, 50, 0.5)
    masks = F.random_filters(5000, (0.5, 0.05, 0.002), seed=11)
    foq = (np.arange(len(Q)) % 4 - 1).astype(np.int32)
    ix = _index(C)
    ix.set_groups(R.random_offsets(len(C), 7))
    for k, pool, lam in ((0, 50, 0.5), (51, 50, 0.5), (10, 1001, 0.5), (10, 50, -0.1), (10, 50, 1.5), (10, 50, float("nan"))):
        assert _raw(ix, Q, k, pool, lam) == (VR_ERR_INVALID, True), (k, pool, lam)
    assert _raw(ix, Q, 10, 50, 0.5, foq) == (VR_ERR_STATE, True)           # a filter, no filters set
    with pytest.raises(_lib.VisragHipError):
        ix.search_diverse(Q, 10, 50, 0.5, 0)
    ix.set_filters(masks)
    assert _raw(ix, Q, 10, 50, 0.5, np.full(len(Q), 3, np.int32)) == (VR_ERR_INVALID, True)    # a host entry == n_filters
    with pytest.raises(ValueError):
        ix.search_diverse(Q, 10, 50, 0.5, 3)
    assert _raw(ix, Q, 10, 50, 0.5, foq) == (0, False) and _raw(ix, Q, 10, 50, 0.5) == (0, False)
    assert ix.search_diverse(Q, 3)[1].shape == (len(Q), 3)                 # pool=None: min(1000, max(4 k, 32))
    assert _same_bits(ix.search_diverse(Q, 3), ix.search_diverse(Q, 3, 32, 0.5))
    # the other searches before and after diverse calls, host and device, plain and filtered, both pool routes
    def others():
        return [ix.search(Q, 10), ix.search(Q, 40), ix.search_filtered(Q, 10, foq), ix.search_filtered(Q, 40, foq)], ix.search_groups(Q, 10)
    before, groups_before = others()
    gstats = ix.group_search_stats()
    for q_in in (Q, torch.tensor(Q).cuda()):
        for pool in (20, 50):
            ix.search_diverse(q_in, 10, pool, 0.5); ix.search_diverse(q_in, 10, pool, 0.5, foq)
    after, groups_after = others()
    assert all(_same_bits(a, b) for a, b in zip(after, before))
    assert _same_bits(groups_after[:2], groups_before[:2]) and np.array_equal(groups_after[2], groups_before[2])
    assert sum(ix.group_search_stats().values()) == sum(gstats.values()) + len(Q)   # (the one grouped search of others())
    ix.close()


def test_demo_retrieve_diverse(tmp_path):
    """A deck knowledge base of embeddings (12 decks x 5 near-identical pages, interleaved on disk), no model run: diverse=0.5
    returns pages of distinct documents in pick order — the reference's, its margins are above 4e-5, not 2e-6 — also among the pages
    of `documents`; diverse=None is the path it was."""
    from visrag_amd import demo
    C, _ = R.decks(12, 5, 64, 1e-3)
    perm = np.random.default_rng(8).permutation(len(C))
    C = np.ascontiguousarray(C[perm])
    names = [f"deck_{r // 5}.pdf_{r % 5}.png" for r in perm]
    Q = R.unit(3, 64, 10)
    kb = str(tmp_path / "kb")
    os.makedirs(kb)
    np.save(os.path.join(kb, "reps.npy"), C)
    with open(os.path.join(kb, "index2img_filename.txt"), "w") as f:
        f.write("\n".join(names))
    labels = np.array([doc_of_page(n) for n in names])
    wanted = ["deck_2.pdf", "deck_5.pdf", "deck_7.pdf", "deck_11.pdf", "no_such.pdf"]
    mask = np.isin(labels, wanted)[None, :]
    index, nm = demo.load_knowledge_base(kb, 0)
    for q in range(len(Q)):
        rs, ri, mg = M.mmr_ref(Q[q:q + 1], C, 5, 32, 0.5)
        assert mg[0] > 1e-5 and len(set(labels[ri[0]])) == 5
        paths, scores = demo.retrieve(kb, Q[q], 5, None, None, index=index, names=nm, return_scores=True, diverse=0.5)
        assert paths == [os.path.join(kb, names[i]) for i in ri[0]]
        np.testing.assert_allclose(scores, rs[0], atol=ATOL, rtol=0)
        assert demo.retrieve(kb, torch.tensor(Q[q]), 5, None, None, index=index, names=nm, diverse=0.5, pool=32) == paths
        plain = demo.retrieve(kb, Q[q], 5, None, None, index=index, names=nm, diverse=1.0)       # lam = 1: the plain top-5
        assert len({doc_of_page(os.path.basename(p)) for p in plain}) <= 2
        rs, ri, mg = M.mmr_ref(Q[q:q + 1], C, 3, 32, 0.5, mask, [0])
        assert mg[0] > 1e-5
        paths = demo.retrieve(kb, Q[q], 3, None, None, index=index, names=nm, documents=wanted, diverse=0.5)
        assert paths == [os.path.join(kb, names[i]) for i in ri[0]]
        docs = [doc_of_page(os.path.basename(p)) for p in paths]
        assert len(set(docs)) == 3 and set(docs) <= set(wanted)
        fs, fi = F.filtered_topk_ref(Q[q:q + 1], C, mask, [0], 3)
        old = demo.retrieve(kb, Q[q], 3, None, None, index=index, names=nm, documents=wanted, return_scores=True)
        assert old == demo.retrieve(kb, Q[q], 3, None, None, index=index, names=nm, documents=wanted, return_scores=True, diverse=None)
        assert old[0] == [os.path.join(kb, names[i]) for i in fi[0]]
    assert len(demo.retrieve(kb, Q[0], 50, None, None, index=index, names=nm, documents=wanted, diverse=0.5)) == 20
    assert demo.retrieve(kb, Q[0], 5, None, None, index=index, names=nm, documents=["no_such.pdf"], diverse=0.5) == []
    assert demo.retrieve(str(tmp_path / "missing"), Q[0], 5, None, None, diverse=0.5) is None
    index.close()
