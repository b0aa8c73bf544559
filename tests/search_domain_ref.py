"""Plain numpy fp64 reference of the plain top-k search (include/visrag_hip.h: vr_index_search) over the parts of the score
domain that random unit vectors never reach, the reference of tests/test_gpu_search_domain.py: all scores negative, row and
query norms between 1e-2 and 1e2, a tie tier at exactly 0 made of signed-zero products, and NaN rows / queries.

Every builder is seeded, parametrised by (nd, nq, dim, k), cached, and returns read-only (C, Q, want_ids, want_scores64).  The
ranking is by fp64 score descending, then row id ascending; a NaN score never ranks; slots beyond the rows that rank are
(-inf, -1).  tests/test_cpu_search_domain_ref.py pins the properties the GPU tests rely on.  Nothing here needs a GPU or the
built library."""
import functools

import numpy as np

from tests.group_search_ref import scores64, unit


def tol_factor(dim):
    """Roundings a product passes through in the library's one fp32 dot (search_common.h: dot_chunk / dot_lane, common.h:
    wave_sum): the multiply and the three fmas of its 4-float chunk (4), the lane's `a + t` per chunk (dim / 256 chunks per
    lane, the first onto a = 0: exact), the 6 levels of wave_sum (offsets 32, 16, 8, 4, 2, 1)."""
    return dim / 256 + 10


def tol(Q, C):
    """[nq][nd] bound of |fp32 score - fp64 score|: tol_factor(dim) * 2^-24 * |q| * |d| (sum |q_i d_i| <= |q| |d|)"""
    Q, C = np.asarray(Q, np.float64), np.asarray(C, np.float64)
    qn = np.sqrt(np.nansum(Q * Q, axis=1))
    dn = np.sqrt(np.nansum(C * C, axis=1))
    return tol_factor(Q.shape[1]) * 2.0 ** -24 * qn[:, None] * dn[None, :]


def rank_scores(Q, C):
    """fp64 scores with what never ranks (a NaN score) at -inf, and +0.0 for either zero"""
    S = scores64(Q, C) + 0.0
    return np.where(np.isnan(S), -np.inf, S)


def topk_ref(Q, C, k):
    """-> (ids i64 [nq][k], scores f64 [nq][k]): score descending, then id ascending; tail (-1, -inf)"""
    S = rank_scores(Q, C)
    nq, n = S.shape
    kk = min(k, n)
    sc = np.full((nq, k), -np.inf)
    ids = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        s = S[q]
        cand = np.flatnonzero(s >= np.partition(s, n - kk)[n - kk])      # the kk best and every tie of the kk-th
        order = cand[np.lexsort((cand, -s[cand]))][:kk]
        sc[q, :kk] = s[order]
        ids[q, :kk] = np.where(np.isneginf(s[order]), -1, order)
    return ids, sc


def near_ties(Q, C, k):
    """Pairs inside a query's top k + 1 whose fp64 scores are DISTINCT and closer than 2 * tol (the larger tol of the two
    rows): where the fp32 ranking could differ from the fp64 one.  Exactly equal scores are ties, decided by id."""
    ids, sc = topk_ref(Q, C, k + 1)
    T = tol(Q, C)
    t = np.where(ids >= 0, np.take_along_axis(T, np.maximum(ids, 0), 1), 0.0)
    ok = ids >= 0
    with np.errstate(invalid="ignore"):
        gap = np.abs(sc[:, :, None] - sc[:, None, :])
        close = (gap < 2.0 * np.maximum(t[:, :, None], t[:, None, :])) & (gap > 0)
    close &= ok[:, :, None] & ok[:, None, :]
    return int(np.triu(close, 1).sum())


def _done(C, Q, k):
    ids, sc = topk_ref(Q, C, k)
    for a in (C, Q, ids, sc):
        a.setflags(write=False)
    return C, Q, ids, sc


@functools.lru_cache(maxsize=None)
def all_negative(nd, nq, dim, k, seed=0):
    """Rows in the positive orthant, queries in the negative one (the negated, normalised sum of three random rows, redrawn
    until every fp64 score is below 0): the 0 of a padded row or score column beats every real score."""
    C = np.abs(unit(nd, dim, 1000 + seed))
    rng = np.random.default_rng(2000 + seed)
    Q = np.empty((nq, dim), np.float32)
    for q in range(nq):
        for _ in range(100):
            v = -C[rng.integers(0, nd, size=3)].sum(0)
            Q[q] = v / np.linalg.norm(v)
            if (scores64(Q[q:q + 1], C) < 0).all():
                break
        else:
            raise AssertionError("no query with negative scores only")
    return _done(C, Q, k)


@functools.lru_cache(maxsize=None)
def scaled_norms(nd, nq, dim, k, seed=0):
    """Unit rows and unit queries, each multiplied by 10 ** U(-2, 2).  For every third query (and enough rows) two rows are
    planted: a row of norm 100 at cosine 0.8 — the query's best row — and, below it in the ranking, a row of cosine ~1 whose
    norm puts its score half way between the query's third and fourth best: the order by cosine and by inner product differ."""
    rng = np.random.default_rng(3000 + seed)
    C = unit(nd, dim, 4000 + seed).astype(np.float64) * 10.0 ** rng.uniform(-2, 2, size=(nd, 1))
    Q = unit(nq, dim, 5000 + seed).astype(np.float64) * 10.0 ** rng.uniform(-2, 2, size=(nq, 1))
    C, Q = C.astype(np.float32), Q.astype(np.float32)
    planted = list(range(0, nq, 3))
    if nd >= 2 * len(planted) + 8:
        rows = rng.choice(nd, size=2 * len(planted), replace=False)
        for j, q in enumerate(planted):
            qh = Q[q].astype(np.float64) / np.linalg.norm(Q[q].astype(np.float64))
            o = rng.standard_normal(dim)
            o -= (o @ qh) * qh
            o /= np.linalg.norm(o)
            top = np.sort(scores64(Q[q:q + 1], C)[0])[::-1][:4]
            C[rows[2 * j]] = (100.0 * (0.8 * qh + 0.6 * o)).astype(np.float32)
            n1 = 0.5 * (top[2] + top[3]) / np.linalg.norm(Q[q].astype(np.float64))
            C[rows[2 * j + 1]] = (n1 * (qh + 1e-3 * o)).astype(np.float32)
    return _done(C, Q, k)


def zero_tier_layout(nd, k):
    """(p, m): rows with positive scores (p < k), rows with negative scores; the other nd - p - m rows score exactly 0"""
    p = max(1, min(k - 3, nd // 3))
    m = max(1, min(64, nd // 3))
    return p, m


@functools.lru_cache(maxsize=None)
def zero_tier(nd, nq, dim, k, seed=0):
    """Queries with support on components [0, dim / 2); nd - p - m rows with support on [dim / 2, dim) only, of mixed signs —
    every product is +0.0 or -0.0 — one of them all zeros; p rows c_j * v with distinct positive scores more than 1e-2 apart;
    m rows with negative scores.  Wanted: the p rows in order, then the zero rows by ascending id; a negative row appears only
    where the index has fewer than k rows, behind every zero."""
    h = dim // 2
    p, m = zero_tier_layout(nd, k)
    rng = np.random.default_rng(6000 + seed)
    v = np.zeros(dim)
    v[:h] = unit(1, h, 7000 + seed)[0]
    Q = np.zeros((nq, dim), np.float32)
    Q[:, :h] = v[None, :h] + 0.1 * unit(nq, h, 8000 + seed)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    C = np.zeros((nd, dim), np.float32)
    C[:, h:] = unit(nd, h, 9000 + seed)
    perm = rng.permutation(nd)
    pos, neg, zero = perm[:p], perm[p:p + m], perm[p + m]
    cpos = 1.0 - 0.8 * np.arange(p) / p                                  # Q . v > 0.9: scores >= 0.02 * 0.9 apart for p <= 37
    cneg = -rng.permutation(np.linspace(0.2, 1.0, m))
    C[pos] = (cpos[:, None] * v[None, :]).astype(np.float32)
    C[neg] = (cneg[:, None] * v[None, :]).astype(np.float32)
    C[zero] = 0.0
    return _done(C, Q, k)


@functools.lru_cache(maxsize=None)
def unit_corpus(nd, nq, dim, k, seed=0):
    """random unit rows and queries (the corpus of tests/test_gpu_search.py): the finite base of the NaN cases"""
    return _done(unit(nd, dim, 10000 + seed), unit(nq, dim, 11000 + seed), k)


BUILDERS = {"all_negative": all_negative, "scaled_norms": scaled_norms, "zero_tier": zero_tier, "unit": unit_corpus}


def nan_rows(base, rows, k, comp=0, negative=()):
    """`base` = (C, Q, ...) of a builder with a NaN in component `comp` of the named rows (sign bit set for those also named in
    `negative`) -> (C, Q, want_ids, want_scores64)"""
    C = np.array(base[0])
    C[np.asarray(rows), comp] = np.nan
    if len(negative):
        C[np.asarray(negative), comp] = np.copysign(np.float32(np.nan), np.float32(-1.0))
    return _done(C, np.array(base[1]), k)


def nan_queries(base, qs, k, comp=0, negative=()):
    """... and of the named queries: such a query gets (-inf, -1) in every slot"""
    Q = np.array(base[1])
    Q[np.asarray(qs), comp] = np.nan
    if len(negative):
        Q[np.asarray(negative), comp] = np.copysign(np.float32(np.nan), np.float32(-1.0))
    return _done(np.array(base[0]), Q, k)


NAN_COMP = 3        # a component every query of all_negative and unit_corpus touches (none of theirs is 0)


@functools.lru_cache(maxsize=None)
def nan_case(domain, nd, nq, dim, k):
    """The NaN case of a finite base: three NaN rows — query 0's best row, query 1's second best, row nd - 1 (the ragged last
    tile) — and one NaN query in the middle of the batch -> (C, Q, want_ids, want_scores64, rows, q_nan).  Both NaN signs
    occur: the middle one of the three rows has the sign bit set, and so has the query of the "unit" base (a sweep that
    filters by the sign of score - threshold must not depend on it)."""
    base = build(domain, nd, nq, dim, k)
    rows = sorted({int(base[2][0, 0]), int(base[2][1, 1]), nd - 1})
    q_nan = nq // 2
    withrows = nan_rows(base, rows, k, NAN_COMP, negative=rows[1:2])
    return nan_queries(withrows, [q_nan], k, NAN_COMP, negative=[q_nan] if domain == "unit" else ()) + (tuple(rows), q_nan)


def bf16_round(x):
    """round to nearest even bf16, as fp32 (finite input)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32)


# ---- the shapes of tests/test_gpu_search_domain.py: (route, nd, nq, dim, k) -------------------------------------------------
ROUTE_SHAPES = [
    ("stream_empty_workgroups", 1001, 5, 256, 10),
    ("stream_several_strips", 12501, 16, 512, 26),
    ("sweep128", 1001, 7, 64, 10),
    ("sweep128", 1001, 7, 192, 10),
    ("sweep256w_compacted", 3001, 40, 128, 10),
    ("sweep256", 3001, 40, 192, 16),
    ("prepass_plain", 9001, 40, 128, 10),
    ("prepass_plain", 9001, 40, 192, 10),
    ("prepass_own_ragged", 36700, 300, 128, 10),
    ("deep", 1001, 5, 64, 40),
    ("deep", 1001, 40, 64, 40),
    ("deep", 5001, 5, 64, 40),
    ("deep", 5001, 40, 64, 40),
    ("fewer_rows_than_k", 7, 2, 64, 10),
    ("fewer_rows_than_k", 7, 2, 256, 10),
]
FALLBACK_SHAPES = [                      # forced with set_search_eps(100.0)
    ("band_pass", 3001, 40, 128, 10),
    ("exact_pass", 9001, 40, 128, 10),
    ("in_place_walk", 9001, 5, 256, 10),
    ("deep_exact", 9001, 5, 64, 40),
]
NAN_SHAPES = [(1001, 5, 256, 10), (1001, 7, 64, 10), (3001, 40, 128, 10), (9001, 40, 128, 10), (1001, 5, 64, 40)]
# seeds for which near_ties(...) == 0 (tests/test_cpu_search_domain_ref.py asserts it); a shape not named here uses seed 0
SEEDS = {("all_negative", 12501, 16, 512, 26): 1, ("all_negative", 1001, 7, 64, 10): 1, ("scaled_norms", 3001, 40, 128, 10): 2,
         ("all_negative", 36700, 300, 128, 10): 45, ("all_negative", 1001, 5, 64, 40): 1, ("all_negative", 1001, 40, 64, 40): 8,
         ("unit", 1001, 7, 64, 10): 1, ("unit", 1001, 5, 64, 40): 1}


def seed_of(domain, nd, nq, dim, k):
    return SEEDS.get((domain, nd, nq, dim, k), 0)


def all_shapes():
    seen, out = set(), []
    for _, nd, nq, dim, k in ROUTE_SHAPES + FALLBACK_SHAPES:
        if (nd, nq, dim, k) not in seen:
            seen.add((nd, nq, dim, k))
            out.append((nd, nq, dim, k))
    return out


def build(domain, nd, nq, dim, k):
    return BUILDERS[domain](nd, nq, dim, k, seed_of(domain, nd, nq, dim, k))
