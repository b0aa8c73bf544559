"""The numpy reference of tests/test_gpu_search_domain.py (tests/search_domain_ref.py): hand-worked cases of its ranking rule,
and — for every shape and seed the GPU file uses — the properties the GPU tests rely on: every score of all_negative is below 0,
the tie tier of zero_tier is exact in any precision, and NO two distinct fp64 scores inside a query's top k + 1 lie closer than
2 * tol(q, d), so that the GPU tests can demand identical ids.  No GPU, no library."""
import numpy as np
import pytest

from tests import search_domain_ref as D
from tests.group_search_ref import scores64

SHAPES = D.all_shapes()


def test_ranking_rule_on_a_hand_worked_case():
    C = np.array([[1.0, 0.0], [0.5, 0.5], [0.5, 0.25], [0.25, 1.0], [0.5, 0.5]], dtype=np.float32)
    Q = np.array([[1.0, 0.0], [0.0, 1.0]], dtype=np.float32)
    ids, sc = D.topk_ref(Q, C, 4)
    assert ids.tolist() == [[0, 1, 2, 4], [3, 1, 4, 2]]
    assert sc.tolist() == [[1.0, 0.5, 0.5, 0.5], [1.0, 0.5, 0.5, 0.25]]
    ids, sc = D.topk_ref(Q, C, 7)
    assert ids[:, 5:].tolist() == [[-1, -1], [-1, -1]] and np.isneginf(sc[:, 5:]).all() and (ids[:, :5] >= 0).all()


def test_a_nan_score_never_ranks():
    C = np.array([[1.0, 0.0], [0.5, 0.5], [0.5, 0.25], [0.25, 1.0], [0.5, 0.5]], dtype=np.float32)
    Q = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0]], dtype=np.float32)
    Cn, Qn, ids, sc = D.nan_rows((C, Q), [0, 3], 4, comp=1)
    assert ids.tolist() == [[1, 2, 4, -1], [1, 4, 2, -1], [1, 4, 2, -1]] and np.isneginf(sc[:, 3]).all()
    assert np.isnan(Cn[[0, 3], 1]).all() and not np.isnan(C).any()                     # the base is not written to
    Cq, Qq, ids, sc = D.nan_queries((C, Q), [1], 2)
    assert ids.tolist() == [[0, 1], [-1, -1], [3, 0]] and np.isneginf(sc[1]).all()


def test_signed_zeros_tie_and_the_lower_id_wins():
    C = np.array([[0.0, 1.0], [0.0, -1.0], [0.0, 0.0], [-1.0, 0.0], [0.5, 0.0]], dtype=np.float32)
    Q = np.array([[1.0, 0.0]], dtype=np.float32)
    ids, sc = D.topk_ref(Q, C, 5)
    assert ids.tolist() == [[4, 0, 1, 2, 3]] and not np.signbit(sc[0, 1:4]).any() and (sc[0, 1:4] == 0).all()


def test_tol_counts_the_roundings_of_the_one_fp32_dot():
    assert D.tol_factor(256) == 11 and D.tol_factor(2304) == 19 and D.tol_factor(64) == 10.25
    t = D.tol(np.ones((1, 2304), np.float32) / 48.0, np.ones((1, 2304), np.float32) / 48.0)       # unit data at dim 2304
    assert abs(t[0, 0] - 19 * 2.0 ** -24) < 1e-12 and 1.1e-6 < t[0, 0] < 1.2e-6


def test_bf16_round_is_round_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.3], dtype=np.float32)
    r = D.bf16_round(x)
    assert r[:4].tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7]
    assert (r.view(np.uint32) & 0xFFFF == 0).all() and abs(r[4] + 0.3) <= 0.3 * 2.0 ** -8


@pytest.mark.parametrize("nd,nq,dim,k", SHAPES)
def test_all_negative_scores_are_below_zero_without_near_ties(nd, nq, dim, k):
    C, Q, ids, sc = D.build("all_negative", nd, nq, dim, k)
    assert (scores64(Q, C) < 0).all() and (C >= 0).all() and (Q <= 0).all()
    kk = min(k, nd)
    assert (sc[:, :kk] < 0).all() and (np.diff(sc[:, :kk], axis=1) < 0).all()
    assert D.near_ties(Q, C, k) == 0


@pytest.mark.parametrize("nd,nq,dim,k", SHAPES)
def test_scaled_norms_span_four_decades_without_near_ties(nd, nq, dim, k):
    C, Q, ids, sc = D.build("scaled_norms", nd, nq, dim, k)
    dn, qn = np.linalg.norm(C.astype(np.float64), axis=1), np.linalg.norm(Q.astype(np.float64), axis=1)
    assert 0.99e-2 < dn.min() and dn.max() < 1.01e2 and 0.99e-2 < qn.min() and qn.max() < 1.01e2
    if nd >= 1000:
        assert dn.min() < 0.1 and dn.max() > 10
        # the planted pairs: for every third query the order by cosine and the order by inner product differ inside the top k
        S = scores64(Q, C)
        for q in range(0, nq, 3):
            cos = S[q, ids[q]] / (qn[q] * dn[ids[q]])
            assert ids[q, 0] == np.argmax(S[q]) and abs(cos[0] - 0.8) < 1e-3 and abs(dn[ids[q, 0]] - 100) < 1e-3
            j = int(np.argmax(cos))
            assert 0 < j < k and cos[j] > 0.9999 and dn[ids[q, j]] < 0.7 * dn[ids[q, 0]], (q, j, cos)
    assert D.near_ties(Q, C, k) == 0


@pytest.mark.parametrize("nd,nq,dim,k", SHAPES)
def test_zero_tier_is_exact_in_fp32_and_fp64(nd, nq, dim, k):
    C, Q, ids, sc = D.build("zero_tier", nd, nq, dim, k)
    p, m = D.zero_tier_layout(nd, k)
    h = dim // 2
    S = scores64(Q, C)
    tier = np.flatnonzero((C[:, :h] == 0).all(1))
    assert len(tier) == nd - p - m and p < k and (Q[:, h:] == 0).all()
    # every product of a tier row has a zero factor: +0.0 or -0.0 whatever the precision and the summation order
    assert (S[:, tier] == 0).all() and (C[tier][:, h:] != 0).any(1).sum() == len(tier) - 1
    t = tier[:64]
    prod = Q[:, None, :] * C[None, t, :]                                                 # fp32 products
    assert prod.dtype == np.float32 and (prod == 0).all() and np.signbit(prod).any() and not np.signbit(prod).all()
    assert (prod.sum(-1, dtype=np.float32) == 0).all()
    # wanted: the p positive rows in order, more than 1e-2 apart, then the zero rows by ascending id
    kk = min(k, nd)
    assert (sc[:, :p] > 0).all() and (np.diff(sc[:, :p + 1], axis=1) < -1e-2).all()
    nz = min(kk - p, len(tier))
    assert (ids[:, p:p + nz] == tier[:nz][None, :]).all() and (sc[:, p:p + nz] == 0).all() and not np.signbit(sc[:, p:p + nz]).any()
    assert ((S < 0).sum(1) == m).all()
    if kk == k:
        assert (sc >= 0).all()                                                           # a negative row never appears
    else:
        assert (sc[:, p + nz:kk] < 0).all() and (ids[:, kk:] == -1).all()
    assert D.near_ties(Q, C, k) == 0


@pytest.mark.parametrize("domain", ["all_negative", "unit"])
@pytest.mark.parametrize("nd,nq,dim,k", D.NAN_SHAPES)
def test_nan_cases_rank_the_finite_rows_without_near_ties(domain, nd, nq, dim, k):
    base = D.build(domain, nd, nq, dim, k)
    C, Q, ids, sc, rows, q_nan = D.nan_case(domain, nd, nq, dim, k)
    assert D.near_ties(base[1], base[0], k) == 0 and D.near_ties(Q, C, k) == 0
    assert len(rows) == 3 and rows[-1] == nd - 1 and base[2][0, 0] in rows and base[2][1, 1] in rows
    assert np.isnan(C[list(rows), D.NAN_COMP]).all() and np.isnan(C).sum() == 3 and np.isnan(Q).sum() == 1
    assert np.signbit(C[list(rows), D.NAN_COMP]).tolist() == [False, True, False] and np.signbit(Q[q_nan, D.NAN_COMP]) == (domain == "unit")
    assert (base[1][:, D.NAN_COMP] != 0).all()                                           # the queries' support touches the component
    assert (ids[q_nan] == -1).all() and np.isneginf(sc[q_nan]).all()
    fin = [q for q in range(nq) if q != q_nan]
    assert not np.isin(ids[fin], rows).any() and (ids[fin] >= 0).all()
    # == the reference over the finite rows alone
    keep = np.setdiff1d(np.arange(nd), rows)
    ids2, sc2 = D.topk_ref(base[1][fin], base[0][keep], k)
    assert np.array_equal(keep[ids2], ids[fin]) and np.array_equal(sc2, sc[fin])
