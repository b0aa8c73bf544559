"""-m gpu: the plain top-k search (HipIndex.search / search_keys: vr_index_search, vr_index_search_keys) over the parts of the
score domain that the random unit vectors of tests/test_gpu_search.py never reach — every score negative (a padded row or score
column scores 0 and would win), the negative half of the orderable key, row and query norms between 1e-2 and 1e2, a tie tier at
exactly 0 made of signed-zero products, NaN rows and NaN queries — on every route of that search and on its fallbacks.

Reference: tests/search_domain_ref.py (fp64, score descending then id ascending).  tests/test_cpu_search_domain_ref.py has shown
that no two distinct fp64 scores inside a top k + 1 lie closer than 2 * tol for any shape and seed used here, so the ids must be
IDENTICAL to the reference's: no near-tie excuse.  tol(q, d) = (dim / 256 + 10) * 2^-24 * |q| * |d| bounds the library's one
fp32 dot (search_common.h: 4 roundings in a 4-float chunk, dim / 256 chunk adds per lane, common.h: 6 levels of wave_sum)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import search_domain_ref as D  # noqa: E402
from visrag_amd.engine import HipIndex, topk_merge, topk_merge_keys  # noqa: E402
from visrag_amd.retriever import merge_topk_host, unpack_keys_host  # noqa: E402

DOMAINS = ("all_negative", "scaled_norms", "zero_tier")
OUTCOMES = ("certified", "certified_extended", "flagged", "uncertified")


def _index(C):
    nd, dim = C.shape
    ix = HipIndex(dim, nd)
    ix.add(C[: nd // 2]); ix.add(C[nd // 2:])
    assert len(ix) == nd
    return ix


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _assert_result(sc, ids, C, Q, want_ids, want_sc, what):
    """ids identical to the reference's, empty slots (-inf, -1), every score within tol of the fp64 dot of ITS row"""
    ok = want_ids >= 0
    assert ids.dtype == np.int64 and sc.dtype == np.float32
    bad = np.argwhere(ids != want_ids)
    assert len(bad) == 0, (what, "wrong ids", len(bad), [(int(q), int(c), int(ids[q, c]), int(want_ids[q, c])) for q, c in bad[:8]])
    assert np.isneginf(sc[~ok]).all(), (what, "tail scores")
    T = np.take_along_axis(D.tol(Q, C), np.maximum(ids, 0), 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(sc.astype(np.float64) - want_sc)                                   # (empty slots: -inf - -inf, not looked at)
        ratio = np.where(ok & (T > 0), err / T, 0.0).max(initial=0.0)
    print(f"{what}: max |score - fp64| / tol = {ratio:.3f}")
    assert (err[ok] <= T[ok]).all(), (what, "score out of tol", float(ratio))


def _assert_counters(st, nq, what):
    assert st["uncertified"] == 0 and sum(st[w] for w in OUTCOMES) == nq, (what, st)
    assert st["band_pass"] + st["exact_pass"] == st["flagged"], (what, st)


def _assert_domain(domain, sc, ids, C, want_ids, want_sc, ix):
    nd = len(C)
    ok = want_ids >= 0
    if domain == "all_negative":
        assert (sc[ok] < 0).all() and (ids[ok] >= 0).all() and (ids[ok] < nd).all()
    if domain == "zero_tier":
        tier = ok & (want_sc == 0)
        assert tier.any() and (sc[tier] == 0).all() and not np.signbit(sc[tier]).any(), "the tier: +0.0, never the -0.0 bit pattern"
        for q in range(len(ids)):
            assert (np.diff(ids[q][tier[q]]) > 0).all(), (q, ids[q])
    if domain == "scaled_norms":
        em = ix.error_model()
        C64 = C.astype(np.float64)
        dmax = np.sqrt((C64 * C64).sum(1)).max()
        R = C64 - D.bf16_round(C).astype(np.float64)
        rmax = np.sqrt((R * R).sum(1)).max()
        print(f"max_row_norm / fp64 = {em['max_row_norm'] / dmax:.8f}, max_row_bf16_residual / fp64 = {em['max_row_bf16_residual'] / rmax:.8f}")
        assert 1.0 <= em["max_row_norm"] / dmax <= 1.0 + 1e-4, (em, dmax)
        assert em["max_row_bf16_residual"] >= rmax, (em, rmax)                            # upper bounds by design


def _search_checked(ix, domain, C, Q, want_ids, want_sc, k, what):
    nq = len(Q)
    ix.search_stats(reset=True)
    sc, ids = ix.search(Q, k)
    st = ix.search_stats()
    _assert_result(sc, ids, C, Q, want_ids, want_sc, what)
    _assert_counters(st, nq, what)
    _assert_domain(domain, sc, ids, C, want_ids, want_sc, ix)
    sc2, ids2 = ix.search(Q, k)                                # (after a band beyond 8192 rows: through the exact pass, not the walk)
    assert np.array_equal(ids2, ids) and np.array_equal(_bits(sc2), _bits(sc)), (what, "a second search differs")
    return sc, ids, st


def _ceil(a, b):
    return (a + b - 1) // b


def _assert_route(ix, route, nd, nq, dim, k):
    """the route a shape is named for, from the plan the library reports (kernels.h: search_uses_stream, search_uses_256,
    search_prepass_owned; search.hip: launch_kp) and the documented conditions"""
    plan = ix.search_plan(nq)
    t128, t256 = _ceil(nd, 128), _ceil(nd, 256)
    if route.startswith("stream"):
        assert nq <= 16 and dim % 256 == 0 and k <= 26
        assert plan["list_chunks"] == 256 and plan["tiles_per_chunk"] == 0 and plan["prepass_chunks"] == 0, plan
        rows_per_wg = _ceil(_ceil(nd, 256), 16) * 16
        if route == "stream_empty_workgroups":
            assert _ceil(nd, rows_per_wg) < 256 and nd % 16 != 0
        else:
            assert rows_per_wg >= 32 and nd % rows_per_wg != 0                        # several strips per workgroup, a ragged last one
    elif route == "sweep128":
        assert nq <= 16 and dim % 256 != 0 and k <= 26
        assert plan["prepass_chunks"] == 0 and plan["sweep_chunks"] == plan["list_chunks"] and plan["list_chunks"] != 256, plan
        assert plan["tiles_per_chunk"] == _ceil(t128, plan["sweep_chunks"]) >= 1 and nd % 128 != 0, plan
    elif route in ("sweep256w_compacted", "sweep256", "prepass_plain"):
        assert nq >= 17 and k <= 26 and plan["prepass_chunks"] == 0 and plan["sweep_chunks"] == plan["list_chunks"], plan
        assert plan["tiles_per_chunk"] == _ceil(t256, plan["sweep_chunks"]) >= 1 and nd % 256 != 0, plan
        if route != "prepass_plain":
            assert (dim % 128 == 0) == (route == "sweep256w_compacted")            # the one-wave sweep needs dim % 128 == 0
        assert (t128 >= 64) == (route == "prepass_plain") and t256 < 128           # the pre-pass: >= 64 tiles of 128 rows
    elif route == "prepass_own_ragged":
        assert plan["prepass_chunks"] == 8 and plan["list_chunks"] == plan["sweep_chunks"] + 8 and dim % 128 == 0, plan
        S = t256 // 16
        assert 15 * S + S - 1 == t256 - 1 and nd - (t256 - 1) * 256 == 92           # the last sampled tile is the ragged last tile
        assert plan["tiles_per_chunk"] == _ceil(t256 - 16, plan["sweep_chunks"]), plan
    elif route == "deep":
        assert k > 26 and nd > k + 24
    elif route == "fewer_rows_than_k":
        assert nd < k
    else:
        raise AssertionError(route)


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("route,nd,nq,dim,k", D.ROUTE_SHAPES, ids=[f"{r}-{a}x{b}x{c}-k{d}" for r, a, b, c, d in D.ROUTE_SHAPES])
def test_every_route_over_the_domain(route, nd, nq, dim, k, domain):
    """all_negative / scaled_norms / zero_tier over every route of the plain search, at the smallest ragged shapes that take the
    route (confirmed from search_plan): ids identical to fp64, scores within tol, every query certified or redone, and the same
    bits on a second search."""
    C, Q, want_ids, want_sc = D.build(domain, nd, nq, dim, k)
    ix = _index(C)
    _assert_route(ix, route, nd, nq, dim, k)
    sc, ids, st = _search_checked(ix, domain, C, Q, want_ids, want_sc, k, f"{route} {domain}")
    if nd < k:
        assert (ids[:, nd:] == -1).all() and np.isneginf(sc[:, nd:]).all() and (ids[:, :nd] >= 0).all()
    ix.close()


@pytest.mark.parametrize("domain", DOMAINS)
@pytest.mark.parametrize("route,nd,nq,dim,k", D.FALLBACK_SHAPES, ids=[r for r, *_ in D.FALLBACK_SHAPES])
def test_every_fallback_alone_over_the_domain(route, nd, nq, dim, k, domain):
    """An error model nothing satisfies (set_search_eps(100.0)): every query is flagged and its band is the whole index — the
    band pass (<= 8192 rows), the exact fp32 pass, the merge workgroup's own walk in segments of 8192 rows (the first streaming
    search of an index), the deep path's exact select."""
    C, Q, want_ids, want_sc = D.build(domain, nd, nq, dim, k)
    ix = _index(C)
    ix.set_search_eps(100.0)
    assert ix.search_plan(nq)["exact_pass_launched"] == 0
    if route == "in_place_walk":
        assert ix.search_plan(nq)["list_chunks"] == 256 and nq <= 16 and dim % 256 == 0 and nd > 8192
    sc, ids, st = _search_checked(ix, domain, C, Q, want_ids, want_sc, k, f"{route} {domain}")
    assert st["flagged"] == nq, st
    if route == "band_pass":
        assert st["band_pass"] == nq and nd <= 8192, st
    else:
        assert st["exact_pass"] == nq and nd > 8192, st
        if route != "deep_exact":
            # the first such bands were walked by one workgroup each and set the index's word; the second search of
            # _search_checked went through exact_scores_kernel + the exact select, to the same bits
            assert ix.search_plan(nq)["exact_pass_launched"] == 1
    ix.close()


@pytest.mark.parametrize("domain", ["all_negative", "zero_tier"])
@pytest.mark.parametrize("nd,nq,dim,k", [(3001, 40, 128, 10), (1001, 5, 64, 40)])
def test_packed_keys_and_merges_over_the_domain(nd, nq, dim, k, domain):
    """The negative half of the orderable key and the zero tier through the exchange format: search_keys + unpack_keys_host ==
    search with shifted ids; two half-shards merged by topk_merge_keys == the single index, bit for bit; topk_merge on
    (score, id) pairs == merge_topk_host."""
    C, Q, want_ids, want_sc = D.build(domain, nd, nq, dim, k)
    q = torch.from_numpy(np.array(Q)).cuda()
    full = _index(C)
    fs, fi = full.search(q, k)
    sc, ids = fs.cpu().numpy(), fi.cpu().numpy()
    _assert_result(sc, ids, C, Q, want_ids, want_sc, f"packed {domain}")
    us, ui = unpack_keys_host(full.search_keys(q, k, id_offset=7).cpu().numpy())
    assert np.array_equal(_bits(us), _bits(sc)) and np.array_equal(ui, np.where(ids >= 0, ids + 7, -1))
    half = nd // 2
    keys, psc, pid = [], [], []
    for lo, hi in ((0, half), (half, nd)):
        sh = HipIndex(dim, hi - lo); sh.add(C[lo:hi])
        keys.append(sh.search_keys(q, k, id_offset=lo))
        s_, i_ = sh.search(q, k)
        psc.append(s_); pid.append(torch.where(i_ >= 0, i_ + lo, i_))
        sh.close()
    ms, mi = topk_merge_keys(torch.stack(keys))
    assert torch.equal(mi, fi) and np.array_equal(_bits(ms.cpu().numpy()), _bits(sc))
    ps, pi = topk_merge(torch.stack(psc), torch.stack(pid))
    hs, hi_ = merge_topk_host(torch.stack(psc).cpu().numpy(), torch.stack(pid).cpu().numpy(), k)
    assert np.array_equal(pi.cpu().numpy(), hi_) and np.array_equal(ps.cpu().numpy(), hs)
    assert np.array_equal(pi.cpu().numpy(), ids) and np.array_equal(_bits(ps.cpu().numpy()), _bits(sc))
    full.close()


@pytest.mark.parametrize("eps", [None, 100.0], ids=["default", "eps100"])
@pytest.mark.parametrize("domain", ["all_negative", "unit"])
@pytest.mark.parametrize("nd,nq,dim,k", D.NAN_SHAPES)
def test_nan_rows_never_rank_and_a_nan_query_gets_nothing(nd, nq, dim, k, domain, eps):
    """The NaN contract of vr_index_search on every route: three NaN rows (query 0's best row, query 1's second best, the last
    row) and one NaN query in the middle of the batch.  Finite queries: the reference over the finite rows, ids identical; the
    NaN query: (-inf, -1) in every slot, key 0 from search_keys; the counters still sum to nq.  Under the default bound (the
    sweeps, the merges, the deep path) and under set_search_eps(100.0) (the band pass, the walks, the exact pass: the second
    search of an index of more than 8192 rows is the one that runs exact_scores_kernel).  NaNs of both signs occur
    (search_domain_ref.nan_case): three sweeps compare `score >= threshold`, the one-wave sweep (search256w.hip) goes by the sign
    bit of `score - threshold`; selection from score rows (deep path, exact pass) goes by the orderable key, where a positive NaN
    is the largest there is unless search_select.h's select_key<true> and search_common.h's make_key_ranked keep it out."""
    C, Q, want_ids, want_sc, rows, q_nan = D.nan_case(domain, nd, nq, dim, k)
    ix = _index(C)
    if eps is not None:
        ix.set_search_eps(eps)
    fin = np.array([q for q in range(nq) if q != q_nan])
    for rep in range(2):
        ix.search_stats(reset=True)
        sc, ids = ix.search(Q, k)
        st = ix.search_stats()
        what = f"nan {domain} {'default' if eps is None else 'eps100'} search {rep}"
        assert (ids[q_nan] == -1).all() and np.isneginf(sc[q_nan]).all(), (what, ids[q_nan], sc[q_nan])
        assert not np.isin(ids, rows).any(), (what, "a NaN row ranks", np.argwhere(np.isin(ids, rows))[:8].tolist())
        _assert_result(sc[fin], ids[fin], C, Q[fin], want_ids[fin], want_sc[fin], what)
        assert not np.isnan(sc).any()
        assert st["uncertified"] == 0 and sum(st[w] for w in OUTCOMES) == nq, (what, st)
    keys = ix.search_keys(torch.from_numpy(np.array(Q)).cuda(), k, id_offset=7).cpu().numpy()
    us, ui = unpack_keys_host(keys)
    assert (keys[q_nan] == 0).all()
    assert np.array_equal(ui, np.where(ids >= 0, ids + 7, -1)) and np.array_equal(_bits(us), _bits(sc))
    ix.close()
