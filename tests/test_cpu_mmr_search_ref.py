"""The numpy reference of the diversified search (tests/mmr_search_ref.py) on hand-worked cases, and the facts about the GPU
test's cases that tests/test_gpu_mmr_search.py quotes in its docstrings.  No GPU, no built library."""
import numpy as np
import pytest

from tests import filter_search_ref as F
from tests import group_search_ref as R
from tests import mmr_search_ref as M

# q = (0.8, 0.6); relevance r = q . d:   d0 0.8   d1 0.936   d2 0.28   d3 0.96   d4 0.6   -> ranking d3 d1 d0 d4 d2
ROWS = np.array([[1.0, 0.0], [0.96, 0.28], [0.8, -0.6], [0.6, 0.8], [0.0, 1.0]], dtype=np.float32)
QUERY = np.array([[0.8, 0.6]], dtype=np.float32)


def test_hand_worked_pool_of_four():
    """pool = {d3, d1, d0, d4}, lam = 0.5.  Pick 0 = d3.  Dots with d3: d1 0.8, d0 0.6, d4 0.8 ->
    v: d1 0.468 - 0.4 = 0.068, d0 0.4 - 0.3 = 0.1, d4 0.3 - 0.4 = -0.1 -> d0 (margin 0.032).  Dots with d0: d1 0.96, d4 0 ->
    m: d1 0.96, d4 0.8 -> v: d1 0.468 - 0.48 = -0.012, d4 -0.1 -> d1 (margin 0.088).  Then d4, alone."""
    sc, ids, mg = M.mmr_ref(QUERY, ROWS, 4, 4, 0.5)
    assert ids.tolist() == [[3, 0, 1, 4]]
    np.testing.assert_allclose(sc, [[0.96, 0.8, 0.936, 0.6]], atol=1e-6)
    np.testing.assert_allclose(mg, [0.032], atol=1e-6)
    sc3, ids3, _ = M.mmr_ref(QUERY, ROWS, 3, 4, 0.5)                      # k cuts the picks, not the pool
    assert ids3.tolist() == [[3, 0, 1]] and np.array_equal(sc3, sc[:, :3])
    assert not np.all(np.diff(sc[0]) <= 0)                                # the scores are the relevance: not monotone


def test_hand_worked_pool_of_five():
    """d2 joins the pool: <d2, d3> = 0, v = 0.14 - 0 -> picked second.  Then m = 0.8 for d1 (d3), d0 (d2), d4 (d3):
    v: d1 0.068, d0 0, d4 -0.1 -> d1; then d0: 0.4 - 0.48 = -0.08 against d4: -0.1 -> d0; then d4."""
    sc, ids, mg = M.mmr_ref(QUERY, ROWS, 5, 5, 0.5)
    assert ids.tolist() == [[3, 2, 1, 0, 4]]
    np.testing.assert_allclose(sc, [[0.96, 0.28, 0.936, 0.8, 0.6]], atol=1e-6)
    np.testing.assert_allclose(mg, [0.02], atol=1e-6)                     # the last contest: d0 -0.08 against d4 -0.1
    sc, ids, _ = M.mmr_ref(QUERY, ROWS, 5, 5, 0.0)                        # lam = 0: only unlikeness counts
    assert ids[0, 0] == 3 and ids[0, 1] == 2                              # ... but pick 0 is still the best row


def test_pool_larger_than_the_rows_and_k_larger_than_the_pool_members():
    sc, ids, mg = M.mmr_ref(QUERY, ROWS, 7, 20, 0.5)
    assert ids.tolist() == [[3, 2, 1, 0, 4, -1, -1]]
    assert np.isneginf(sc[0, 5:]).all() and np.isfinite(sc[0, :5]).all()
    masks = np.array([[True, True, False, False, True], [False] * 5])
    sc, ids, mg = M.mmr_ref(np.repeat(QUERY, 3, 0), ROWS, 4, 5, 0.5, masks, [0, 1, -1])
    # filter 0 allows d0 d1 d4: ranking d1 d0 d4; <d1, d0> = 0.96, <d1, d4> = 0.28 -> v: d0 -0.08, d4 0.16 -> d4
    assert ids.tolist() == [[1, 4, 0, -1], [-1] * 4, [3, 2, 1, 0]]
    assert np.isneginf(sc[1]).all() and mg[1] == np.inf


def test_equal_v_goes_to_the_lower_pool_position_and_equal_scores_to_the_lower_id():
    C = np.vstack([ROWS, ROWS])                                           # rows i and i + 5 are bit-identical
    sc, ids, mg = M.mmr_ref(QUERY, C, 10, 10, 0.5)
    assert mg[0] == 0.0                                                   # exact ties, decided by position
    pos = {int(i): t for t, i in enumerate(ids[0])}
    assert sorted(pos) == list(range(10)) and all(pos[i] < pos[i + 5] for i in range(5))
    assert ids[0, 0] == 3


@pytest.mark.parametrize("nd,nq,dim,k,pool", [(500, 9, 32, 7, 30), (300, 4, 16, 30, 30)])
def test_lambda_one_is_the_plain_topk_and_pool_equal_k_permutes_it(nd, nq, dim, k, pool):
    C, Q = R.unit(nd, dim, 1), R.unit(nq, dim, 2)
    S = R.scores64(Q, C)
    order = np.lexsort((np.broadcast_to(np.arange(nd), S.shape), -S), axis=1)
    sc, ids, _ = M.mmr_ref(Q, C, k, pool, 1.0)
    assert np.array_equal(ids, order[:, :k]) and np.array_equal(sc, np.take_along_axis(S, order[:, :k], 1))
    for lam in (0.0, 0.3, 0.7):
        sc, ids, _ = M.mmr_ref(Q, C, k, k, lam)
        assert np.array_equal(np.sort(ids, axis=1), np.sort(order[:, :k], axis=1))
        assert np.array_equal(ids[:, 0], order[:, 0])
        np.testing.assert_array_equal(sc, np.take_along_axis(S, ids, 1))


def test_walk_accepts_the_reference_and_measures_a_worse_pick():
    C, Q = R.unit(500, 32, 1), R.unit(9, 32, 2)
    masks = F.random_filters(500, (0.5, 0.02), seed=11)
    foq = np.arange(9) % 3 - 1
    for mk, fq in ((None, None), (masks, foq)):
        _, ids, mg = M.mmr_ref(Q, C, 12, 40, 0.5, mk, fq)
        deficit, outside = M.walk(Q, C, ids, 40, 0.5, mk, fq)
        assert np.array_equal(np.isnan(deficit), ids < 0) and np.array_equal(np.isnan(outside), ids < 0)
        assert np.nanmax(np.abs(deficit)) == 0.0 and np.nanmax(outside) == 0.0
    _, ids, mg = M.mmr_ref(Q, C, 12, 40, 0.5)
    swapped = ids.copy()
    swapped[:, [3, 4]] = swapped[:, [4, 3]]                               # pick 4 taken at step 3: short by at least the margin
    deficit, _ = M.walk(Q, C, swapped, 40, 0.5)
    assert (deficit[:, 3] >= mg - 1e-15).all() and (deficit[:, :3] == 0).all()
    stranger = ids.copy()
    S = R.scores64(Q, C)
    stranger[0, 5] = int(np.argsort(-S[0])[45])                           # rank 46: not in the pool of 40
    _, outside = M.walk(Q, C, stranger, 40, 0.5)
    assert outside[0, 5] > 0 and (np.delete(outside[0], 5) == 0).all()
    with pytest.raises(AssertionError):
        M.walk(Q, C, np.where(np.arange(12) == 5, ids[:, :1], ids), 40, 0.5)       # a row twice


@pytest.mark.parametrize("dim,noise,near_ties", [(256, 1e-3, 3), (2304, 3e-4, 6)])
def test_decks_plain_topk_is_one_template_mmr_spans_ten_documents(dim, noise, near_ties):
    """300 documents x 10 near-identical pages, 48 queries unit(48, dim, 2), k = 10, pool = 100, lam = 0.5: the plain top-10
    spans 1-2 documents, the MMR top-10 exactly 10, for every query.  Queries with a margin under 2e-6 (contests between the
    pages of one document): 3 of 48 at dim 256, 6 of 48 at dim 2304 — no strict-identity claim on the GPU for this corpus."""
    C, Q, (sc, ids, mg) = M.deck_case(dim, noise)
    S = R.scores64(Q, C)
    plain = np.argsort(-S, axis=1, kind="stable")[:, :10] // 10
    assert max(len(set(d)) for d in plain.tolist()) <= 2
    assert all(len(set(d)) == 10 for d in (ids // 10).tolist())
    assert int((mg < 2e-6).sum()) == near_ties


@pytest.mark.parametrize("case,tight,boundary,smallest", [
    ((5000, 37, 256, 10, 50, 0.5), 0, 0, 1.9e-5),
    ((3001, 300, 128, 26, 100, 0.7), 7, 0, 2.8e-7),
    ((20000, 64, 2304, 10, 100, 0.5), 2, 1, 1.5e-6),
    ((1200, 2, 64, 100, 1000, 0.5), 0, 0, 5.0e-6),
    ((5000, 37, 256, 5, 20, 0.5), 0, 0, 5.6e-6),
    ((1200, 2, 64, 1000, 1000, 0.5), 2, 0, 7.0e-8),
])
def test_near_ties_of_the_gpu_cases(case, tight, boundary, smallest):
    """What tests/test_gpu_mmr_search.py's docstring quotes: queries whose smallest margin lies under 2e-6 (not held to the
    reference's ids there), pool-boundary gaps under 3e-7, the smallest margin of the case."""
    nd, nq, dim, k, pool, lam = case
    C, Q, (_, ids, mg) = M.random_case(*case)
    assert int((mg < 2e-6).sum()) == tight
    assert int((M.pool_boundary_gaps(Q, C, pool) < 3e-7).sum()) == boundary
    assert smallest * 0.95 < mg.min() < smallest * 1.05
    if tight * 10 <= nq:
        assert (mg > 2e-6).mean() >= 0.9 * 1.03                           # the reference alone: well inside the 90 % condition


def test_near_ties_of_the_filtered_and_tie_cases():
    """The 262-row and 10-row filters of random_filters(5000, (0.5, 0.05, 0.002), seed=11), k = 10, pool = 50: every margin
    above 4e-6 (strict on the GPU).  vstack([U, U]), U = unit(500, 64, 1), k = 40, pool = 200: twins tie exactly."""
    C, Q = R.unit(5000, 256, 1), R.unit(37, 256, 2)
    masks = F.random_filters(5000, (0.5, 0.05, 0.002), seed=11)
    assert masks.sum(1).tolist() == [2532, 262, 10]
    for f in (1, 2):
        _, ids, mg = M.mmr_ref(Q, C, 10, 50, 0.5, masks, np.full(37, f))
        assert mg.min() > 4e-6 and (ids >= 0).all() and masks[f][ids].all()
    U = R.unit(500, 64, 1)
    _, ids, mg = M.mmr_ref(R.unit(5, 64, 2), np.vstack([U, U]), 40, 200, 0.5)
    for row in ids.tolist():
        assert all(i - 500 in row[: t] for t, i in enumerate(row) if i >= 500)
