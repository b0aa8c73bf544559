"""The references and planted inputs of tests/chat_ref.py, checked on the host alone: every GPU test of
tests/test_gpu_decode_ops.py that compares against them must be able to FAIL.  No GPU, no built library."""
import numpy as np
import pytest

from tests import chat_ref as R
from tests.decode_bars import ATTN_FP32_TERM, ACCUM_FP32_TERM, SWIGLU_FP32_TERM


def test_bf16_rounding_is_nearest_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0e38, 1e-30, 0.1], np.float32)     # 1 + 2^-8 and 1 + 3 * 2^-8: ties, to even
    r = R.bf16_round(x)
    assert r[0] == 1.0 and r[1] == 1.0 and r[2] == np.float32(1.015625)
    assert np.all(np.abs(r - x) <= 2.0 ** -8 * np.abs(x))
    assert np.all((R.bf16_bits(r).astype(np.uint32) << 16).view(np.float32) == r)


# ---------------------------------------------------------------------------------- decode attention
def test_attention_cases_reach_every_branch():
    """the planted cases cover what their names promise (host bookkeeping of the kernel's branches)"""
    c = R.attention_case("mixed16")
    assert c["n"] == 16 and [len(g[2]) for g in R.ATTN_CASES["mixed16"]["groups"]] == [1, 3, 5, 4, 3]
    assert [len(R.split_ranges(g[1])) for g in R.ATTN_CASES["mixed16"]["groups"]] == [1, 2, 8, 1, 3]
    tails = sorted(t for _, _, t in c["step"])
    assert tails[0] == 0 and len(set(tails)) > 4                                   # unequal tails, from one key up
    assert {s for _, s, _ in R.attention_case("P257_nb1")["step"]} == {2} and {s for _, s, _ in R.attention_case("P257_nb5")["step"]} == {0}
    assert [t + 1 for _, _, t in R.attention_case("tails_1_256_257_300")["step"]] == [1, 256, 257, 300]
    per = [hi - lo for lo, hi in R.split_ranges(2600)]
    assert len(per) == 8 and max(per) > R.CHAT_KEYS                                # several chunks per split
    assert sum(1 for lo, hi in R.split_ranges(1, 8) if lo == hi) == 7              # forced: seven ranges without a key
    for P in (1, 255, 256, 257, 513, 2049, 2600):                                  # the policy itself never makes an empty range
        assert all(lo < hi for lo, hi in R.split_ranges(P))


def test_attention_fp32_term_is_measured():
    """ATTN_FP32_TERM = 8 x the largest |fp32 restatement - fp64 reference| over the planted inputs, re-derived here"""
    a = R.fp32_term(R.all_attention_cases, R.decode_attention_ref)
    print("attention fp32 term, re-derived:", a)
    assert a <= ATTN_FP32_TERM <= 2 * a


@pytest.mark.parametrize("name", list(R.ATTN_CASES))
def test_attention_dropped_key_is_seen(name):
    """Removing ONE key — the last prompt key, the keys at a chunk edge, the first key of a split, the first / last tail key
    of a row — moves every affected (row, head) by at least 10 x the tolerance of the GPU test."""
    c = R.attention_case(name)
    ref = R.decode_attention_ref(c)
    kinds = {(k, o, j) for k, o, j, _ in c["drops"]}
    for slot, P, members in R.ATTN_CASES[name]["groups"]:
        assert ("prompt", slot, P - 1) in kinds
        for lo, hi in R.split_ranges(P, c["force"]):
            assert lo == hi or ("prompt", slot, lo) in kinds
        for j in (255, 256):
            assert j >= P or ("prompt", slot, j) in kinds
        for row, tl in members:
            assert ("tail", row, 0) in kinds and ("tail", row, tl - 1) in kinds
            for j in (255, 256):
                assert j >= tl or ("tail", row, j) in kinds
    worst = np.inf
    for drop in c["drops"]:
        got = R.decode_attention_ref(c, drop=drop, only_rows=drop[3])
        for i in drop[3]:
            for h in range(c["H"]):
                s = slice(h * R.HD, (h + 1) * R.HD)
                ratio = float((np.abs(got[i, s] - ref[i, s]) / R.bf16_tol(ref[i, s], ATTN_FP32_TERM)).max())
                worst = min(worst, ratio)
                assert ratio >= 10.0, (name, drop[:3], i, h, ratio)
    print(name, "weakest dropped key: %.0f x the tolerance" % worst)


# ---------------------------------------------------------------------- residual + RMSNorm, SwiGLU
def test_accum_and_swiglu_fp32_terms_are_measured():
    worst = 0.0
    for rows, dim, nsplit, seed in R.ACCUM_CASES:
        x, parts, w, alpha = R.accum_case(rows, dim, nsplit, seed)
        worst = max(worst, float(np.abs(R.accum_ref(x, parts, w, alpha, dtype=np.float32)[0].astype(np.float64)
                                        - R.accum_ref(x, parts, w, alpha)[0]).max()))
    print("rmsnorm_accum fp32 term, re-derived:", 8 * worst)
    assert 8 * worst <= ACCUM_FP32_TERM <= 16 * worst
    worst = 0.0
    for M, I, K, seed in R.SWIGLU_CASES:
        worst = max(worst, float(np.abs(R.swiglu_case(M, I, K, seed, np.float32)[3].astype(np.float64) - R.swiglu_case(M, I, K, seed)[3]).max()))
    print("swiglu fp32 term, re-derived:", 8 * worst)
    assert 8 * worst <= SWIGLU_FP32_TERM <= 16 * worst


def test_gemm_split_planes_sum_to_the_product():
    A, W, b = R.gemm_inputs(5, 260, 320, 1)
    for ks in (1, 2, 3, 7, 9):
        planes = R.gemm_split_ref(A, W, ks, b)
        np.testing.assert_allclose(planes.sum(0), R.gemm_ref(A, W, b), rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(planes[1:] + 0.0, R.gemm_split_ref(A, W, ks)[1:])       # the bias is on split 0 only
    assert np.all(R.gemm_split_ref(A, W, 9)[5:] == 0)                                     # 5 K-steps: splits past the end are zero


def test_interleave16_layout():
    g, u = np.arange(32.0), 100 + np.arange(32.0)
    il = R.interleave16(g, u)
    assert il[:16].tolist() == g[:16].tolist() and il[16:32].tolist() == u[:16].tolist() and il[32:48].tolist() == g[16:].tolist()
    i = 21
    assert il[(i // 16) * 32 + i % 16] == g[i] and il[(i // 16) * 32 + i % 16 + 16] == u[i]   # swiglu_sum's addressing


# ------------------------------------------------------------------------------------- selection
@pytest.mark.parametrize("name", list(R.selection_cases()))
def test_topk_reference_is_a_stable_sort(name):
    """ties to the lower flat index = a stable argsort of the negated scores; gaps between distinct scores among the first
    K + 1 are >= 1e-3 (fp32 lse rounding on the device cannot reorder them), ties are exact"""
    c = R.selection_cases()[name]
    for sc, tok, par, s in R.selection_ref(c):
        flat = s.reshape(-1)
        order = np.argsort(-flat, kind="stable")
        order = [int(f) for f in order[:c["K"]] if flat[f] > -np.inf]
        k = len(order)
        assert (par[:k] * c["V"] + tok[:k]).tolist() == order
        assert np.all(tok[k:] == -1) and np.all(par[k:] == -1) and np.all(sc[k:] == -np.inf)
        assert len(set(order)) == k
        head = np.sort(flat[np.isfinite(flat)])[::-1][:c["K"] + 1]
        d = -np.diff(head)
        assert np.all((d == 0) | (d >= 1e-3)), (name, d[(d != 0) & (d < 1e-3)])


def test_selection_cases_hold_what_they_promise():
    S = R.selection_cases()
    c = S["one_slice"]
    lo, hi = R.slice_bounds(3, c["V"])[5]
    _, tok, par, _ = R.selection_ref(c)[0]
    assert np.all(par == 0) and np.all((tok >= lo) & (tok < hi)) and len(tok) == 16
    c = S["one_per_slice"]
    _, tok, par, _ = R.selection_ref(c)[0]
    b = R.slice_bounds(1, c["V"])
    assert sorted(next(w for w, (lo, hi) in enumerate(b) if lo <= t < hi) for t in tok) == list(range(64))
    assert max(hi - lo for lo, hi in R.slice_bounds(1, 1000)) < S["short_slices"]["K"]
    assert any((R.selection_ref(S["ties_beam"])[0][0][:-1] == R.selection_ref(S["ties_beam"])[0][0][1:]))
    for name in ("neg_inf_beam", "neg_inf_greedy"):
        sc, tok, par, _ = R.selection_ref(S[name])[-1]
        assert sorted(tok[:3].tolist()) == [17, 500, 999] and np.all(tok[3:] == -1)
    # the penalty at the word boundaries changes the result, penalty 1.0 does not
    for tag in ("greedy", "beam"):
        a, b = R.selection_ref(S[f"seen_edges_{tag}_pen1.2"])[0], R.selection_ref(S[f"seen_edges_{tag}_pen1.0"])[0]
        assert a[1].tolist() != b[1].tolist()
        V = S[f"seen_edges_{tag}_pen1.2"]["V"]
        assert {0, 31, 32, V - 1, 1, 30, 33, V - 2} <= set(a[1].tolist())
    w = R.seen_words(S["seen_edges_beam_pen1.2"]["seen"])
    assert w.shape == (2, 129) and w[0, 0] == (1 | 1 << 31) and w[0, 1] == 1 and w[0, 128] == 1 << (4098 & 31)


# -------------------------------------------------------------------------------------- sampling
def test_chi_square_separates_the_temperatures():
    """A host Gumbel-max sampler passes the chi-square test against its own distribution and fails it against the other
    temperature's: the GPU test has power."""
    crit = R.chi2_critical(7, 1e-6)
    assert 40.0 < crit < 46.0, crit                       # (the chi-square table: 40.5 at 1e-6... Wilson-Hilferty within a few %)
    x, ids = R.sampling_logits()
    for T in R.SAMPLE_TEMPS:
        tok, p = R.sampler_probs(x.astype(np.float64), R.SAMPLE_TOPK, T)
        assert tok.tolist() == ids.tolist()
        assert (R.SAMPLE_DRAWS * p).min() >= 40.0
    for seed in R.SAMPLE_SEEDS:
        for T, other in (R.SAMPLE_TEMPS, R.SAMPLE_TEMPS[::-1]):
            _, p = R.sampler_probs(x.astype(np.float64), R.SAMPLE_TOPK, T)
            _, po = R.sampler_probs(x.astype(np.float64), R.SAMPLE_TOPK, other)
            counts = R.gumbel_max_draws(R.SAMPLE_TOP, T, R.SAMPLE_DRAWS, seed)
            own, cross = R.chi2_stat(counts, p), R.chi2_stat(counts, po)
            print("T", T, "seed", seed, "chi2 own %.1f other %.1f critical %.1f" % (own, cross, crit))
            assert own < crit < cross
    # ... and an argmax "sampler" fails
    assert R.chi2_stat(np.array([R.SAMPLE_DRAWS] + [0] * 7), p) > crit
