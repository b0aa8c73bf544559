"""-m gpu: the nucleus sampler (csrc/chat_sample.hip) at op level through vr_op_chat_sample, against the present sampler
(vr_op_chat_select in SAMPLE mode: strict identity where both can answer) and against the fp64 reference of
tests/chat_sample_ref.py, and at model level on the recorded tiny model (HipChat.sample, generate_items(nucleus=...), chat).
tests/test_cpu_chat_sample_ref.py pins the reference itself on hand-worked rows and against transformers' warpers."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import chat_ref as R  # noqa: E402
from tests import chat_sample_ref as S  # noqa: E402
from tests.chat_sample_util import DEV, load_tiny_chat, op_chat_sample, op_chat_sample_raw, upload  # noqa: E402
from tests.gpu_util import P, op_chat_select  # noqa: E402
from visrag_amd.generation import NucleusSampling, generate_items  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------- identity with the present sampler ---
def _edge_rows(V, seed, step):
    """two grid rows whose best four values sit on the seen ids 0 / 31 / 32 / V - 1 (the penalty reorders the top)"""
    x = R.grid_logits(2, V, seed, step)
    edge = [0, 31, 32, V - 1]
    for r in range(2):
        x[r] = R._put_top(x[r], edge)
    seen = np.zeros((2, V), bool)
    seen[:, edge] = True
    return x, seen


@pytest.mark.parametrize("V,step", [(1000, 0.01), (16385, 0.001)])
@pytest.mark.parametrize("top_k", [1, 8, 50, 64])
def test_identity_with_present_sampler(V, step, top_k):
    """top_p = 1 and top_k <= 64 is what the present sampler does: token and score BITS are equal over 256 steps, two seeds,
    penalties 1.0 / 1.3 on seen ids 0 / 31 / 32 / V - 1 and temperatures 0.7 / 1.5; n_kept = min(top_k, candidates)."""
    x, seen = _edge_rows(V, 400 + top_k, step)
    lg, sw = upload(x, seen)
    for pen in (1.0, 1.3):
        for T in (0.7, 1.5):
            refs = [S.Row(x[r], seen[r], pen, T) for r in range(2)]
            for seed in (20240611, 77):
                for st in range(256):
                    sc0, tk0, _ = op_chat_select(R.SAMPLE, lg, sw, V, [0, 1, 2], top_k, 1, penalty=pen, temperature=T, seed=seed, step=st)
                    sc, tk, kept, cut = op_chat_sample(lg, sw, V, pen, T, top_k, 1.0, seed, st)
                    assert tk.tolist() == tk0[:, 0].tolist(), (pen, T, seed, st)
                    assert _bits(sc).tolist() == _bits(sc0[:, 0]).tolist(), (pen, T, seed, st)
                    assert kept.tolist() == [min(top_k, r.candidates) for r in refs]
                    assert cut.tolist() == [r.cut_token(top_k) for r in refs]


def test_top_k_1_and_tiny_top_p_are_greedy():
    x, seen = _edge_rows(1000, 431, 0.01)
    lg, sw = upload(x, seen)
    for pen in (1.0, 1.3):
        _, g, _ = op_chat_select(R.GREEDY, lg, sw, 1000, [0, 1, 2], 1, 1, penalty=pen)
        for st in range(32):
            for top_k, top_p in ((1, 1.0), (1, 0.8), (0, 1e-6), (100, 1e-6)):
                sc, tk, kept, cut = op_chat_sample(lg, sw, 1000, pen, 0.7, top_k, top_p, 5, st)
                assert tk.tolist() == g[:, 0].tolist() and kept.tolist() == [1, 1] and cut.tolist() == tk.tolist()


# ------------------------------------------------------------------------- kept set against fp64 ---
GRID = {1000: (0.01, tuple(range(11, 27))), 16385: (0.001, tuple(range(31, 35))), 122753: (0.0002, (41, 42))}
TOP_KS, TOP_PS = (0, 1, 2, 64, 65, 100, 1000), (0.1, 0.5, 0.8, 0.95)


@functools.lru_cache(maxsize=None)
def _grid_rows(V):
    step, seeds = GRID[V]
    x = np.concatenate([R.grid_logits(1, V, s, step) for s in seeds])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _grid_refs(V, T):
    return tuple(S.Row(row, temperature=T) for row in _grid_rows(V))


@pytest.mark.parametrize("T", [0.7, 1.5])
@pytest.mark.parametrize("V", list(GRID))
def test_kept_set_against_fp64(V, T):
    """n_kept lies in [#(j < K : A_j / Z < top_p - DELTA), #(... < top_p + DELTA)] of the fp64 reference (DELTA = 2e-5, derived in
    tests/chat_sample_ref.py), and where that interval is one value cut_token is the reference's.  The order itself is exact
    (z is the same fp32 value on both sides), so cut_token is ALWAYS the n_kept-th token of the reference's order and the draw
    lies in front of it.  Prints how many intervals the reference alone widens and the largest |A_j / Z - top_p| at a position
    where the device and the fp64 kept counts differ (0: they never differ).
    First MI355X run: 22 of the 1 232 intervals are wider than one value (V = 1000: 0 / 0 at T = 0.7 / 1.5; 16385: 4 / 8;
    122753: 6 / 4) and the device's count equalled the fp64 count in every one of the 1 232."""
    x = _grid_rows(V)
    refs = _grid_refs(V, T)
    lg, sw = upload(x)
    wide, differ, worst = 0, 0, 0.0
    for top_k in TOP_KS:
        for top_p in TOP_PS:
            sc, tk, kept, cut = op_chat_sample(lg, sw, V, 1.0, T, top_k, top_p, seed=9, step=top_k)
            for i, r in enumerate(refs):
                lo, hi, _ = r.interval(top_k, top_p)
                n = int(kept[i])
                assert lo <= n <= hi, (V, T, top_k, top_p, i, n, lo, hi)
                assert int(cut[i]) == r.cut_token(n), (V, T, top_k, top_p, i)
                if lo == hi:
                    assert int(cut[i]) == r.cut_token(r.n_kept(top_k, top_p))
                else:
                    wide += 1
                want = r.n_kept(top_k, top_p)
                if n != want:
                    differ += 1
                    K, A, Z = S._first_k(r.w, top_k)
                    worst = max(worst, float(np.abs(A[min(n, want):max(n, want)] / Z - top_p).max()))
                assert int(tk[i]) in r.order[:n] and sc[i] == r.s[tk[i]]
    total = len(TOP_KS) * len(TOP_PS) * len(refs)
    print(f"nucleus V={V} T={T}: {wide} of {total} intervals wider than one value; device != fp64 count in {differ}, "
          f"largest |A_j/Z - top_p| there {worst:.2e}")


# ------------------------------------------------------------------------------------------ ties ---
def test_ties_are_exact():
    """all logits equal: the sums are integers, so the cut is exact — top_p 0.5 / 0.25 keep 500 / 250 of 1000 (the lowest
    ids), 50 / 25 of the top_k = 100; every draw lies below n_kept"""
    lg, sw = upload(np.full((1, 1000), 0.375, np.float32))
    for top_k, top_p, want in ((0, 0.5, 500), (0, 0.25, 250), (100, 0.5, 50), (100, 0.25, 25), (100, 1.0, 100), (0, 1.0, 1000)):
        drawn = set()
        for st in range(512):
            sc, tk, kept, cut = op_chat_sample(lg, sw, 1000, 1.0, 0.7, top_k, top_p, seed=3, step=st)
            assert kept[0] == want and cut[0] == want - 1, (top_k, top_p, st)
            assert 0 <= tk[0] < want and sc[0] == np.float32(0.375)
            drawn.add(int(tk[0]))
        assert len(drawn) > min(want, 512) // 4                 # (not one token over and over)


def test_split_tier_below_a_distinct_top():
    """three distinct leaders, then a tier of 40 equal values at scattered ids: top_k = 10 keeps the 7 lowest ids of the tier"""
    x = np.full((1, 1000), -30.0, np.float32)
    tier = np.arange(13, 1000, 25)[:40]
    x[0, tier] = 1.0
    x[0, [900, 5, 450]] = [3.0, 2.5, 2.0]
    lg, sw = upload(x)
    r = S.Row(x[0], temperature=1.5)
    for top_k, top_p in ((10, 1.0), (10, 0.9), (0, 0.6), (25, 0.95)):
        n = r.n_kept(top_k, top_p)
        assert r.interval(top_k, top_p)[2] > 1e-3
        for st in range(64):
            sc, tk, kept, cut = op_chat_sample(lg, sw, 1000, 1.0, 1.5, top_k, top_p, seed=8, step=st)
            assert kept[0] == n and cut[0] == r.cut_token(n) and int(tk[0]) in r.order[:n], (top_k, top_p, st)
    assert r.n_kept(10, 1.0) == 10 and r.cut_token(10) == int(tier[6])


# ------------------------------------------------------------------------------------ membership ---
def test_membership():
    x = R.grid_logits(1, 1000, 501, 0.01)
    seen = np.zeros((1, 1000), bool)
    seen[0, np.argsort(-x[0])[:5]] = True
    lg, sw = upload(x, seen)
    r = S.Row(x[0], seen[0], 1.3, 0.7)
    assert r.interval(100, 0.8)[2] > 1e-4
    keep = set(r.kept(100, 0.8).tolist())
    for seed in (3, 4):
        drawn = set()
        for st in range(512):
            sc, tk, kept, cut = op_chat_sample(lg, sw, 1000, 1.3, 0.7, 100, 0.8, seed, st)
            assert int(tk[0]) in keep and kept[0] == len(keep) and sc[0] == r.s[tk[0]]
            drawn.add(int(tk[0]))
        assert len(drawn) > 10


# ---------------------------------------------------------------------------------- distribution ---
# Chi-square with 4 degrees of freedom, critical value at p = 1e-6; against the unfiltered eight with 7.
@pytest.mark.parametrize("T", R.SAMPLE_TEMPS)
def test_distribution(T):
    """chat_ref.sampling_logits (SAMPLE_TOP planted), top_k = 0, top_p between A_4 / Z and A_5 / Z: exactly 5 of the 8 planted
    tokens are kept.  4096 draws per seed pass a chi-square test against the renormalised five and fail it against the
    unfiltered eight; nothing outside the five is ever drawn."""
    x, ids = R.sampling_logits()
    r = S.Row(x, temperature=T)
    K, A, Z = S._first_k(r.w, 0)
    top_p = float(0.5 * (A[4] + A[5]) / Z)
    assert r.order[:8].tolist() == ids.tolist() and r.n_kept(0, top_p) == 5
    assert r.interval(0, top_p)[2] > 1e-3                       # the edge is far from top_p
    tok, p = r.probs(0, top_p)
    p8 = r.w[:8] / r.w[:8].sum()
    assert (R.SAMPLE_DRAWS * p).min() >= 40.0
    crit4, crit7 = R.chi2_critical(4, 1e-6), R.chi2_critical(7, 1e-6)
    index = {int(t): i for i, t in enumerate(ids)}
    lg, sw = upload(x[None])
    for seed in R.SAMPLE_SEEDS:
        counts = np.zeros(8, np.int64)
        for st in range(R.SAMPLE_DRAWS):
            sc, tk, kept, cut = op_chat_sample(lg, sw, x.size, 1.0, T, 0, top_p, seed, st)
            t = int(tk[0])
            assert t in index and index[t] < 5, (seed, st, t)
            assert kept[0] == 5 and cut[0] == ids[4] and sc[0] == x[t]
            counts[index[t]] += 1
        own, cross = R.chi2_stat(counts[:5], p), R.chi2_stat(counts, p8)
        print(f"nucleus T={T} seed={seed}: chi2 against the kept five {own:.1f} (critical {crit4:.1f}), against the unfiltered eight "
              f"{cross:.1f} (critical {crit7:.1f})")
        assert own < crit4, (T, seed, counts.tolist())
        assert cross > crit7, (T, seed, counts.tolist())


# --------------------------------------------------------------------------- rows are independent ---
def test_rows_are_independent():
    """16 rows in one call equal 16 calls of one row: 13 grid rows with different seen sets, a row of three finite tokens
    (fewer candidates than top_k), a row of equal values (the cut splits a tier) and a row with -inf holes"""
    rng = np.random.default_rng(77)
    x = R.grid_logits(16, 1000, 601, 0.01)
    seen = np.zeros((16, 1000), bool)
    for r in range(13):
        seen[r, rng.choice(np.argsort(-x[r])[:40], 6, replace=False)] = True
    x[13] = -np.inf
    x[13, [17, 500, 999]] = [0.5, 2.0, -1.0]
    x[14] = 0.25
    x[15, rng.permutation(1000)[:400]] = -np.inf
    lg, sw = upload(x, seen)
    for top_k, top_p in ((100, 0.8), (0, 0.5), (6, 1.0), (2, 0.95)):
        for st in (0, 1, 2):
            whole = op_chat_sample(lg, sw, 1000, 1.2, 0.7, top_k, top_p, seed=21, step=st)
            for r in range(16):
                one = op_chat_sample(lg[r:r + 1], sw[r:r + 1], 1000, 1.2, 0.7, top_k, top_p, seed=21, step=st)
                assert [_bits(whole[0])[r], whole[1][r], whole[2][r], whole[3][r]] == [_bits(one[0])[0], one[1][0], one[2][0], one[3][0]]
            ref = [S.Row(x[r], seen[r], 1.2, 0.7) for r in (13, 14)]
            assert whole[2][13] == ref[0].n_kept(top_k, top_p) and whole[2][14] == ref[1].n_kept(top_k, top_p)


def test_unaligned_rows_equal_aligned_rows():
    """The kernel reads a 16-byte aligned row four tokens at a time and any other row token by token: rows at byte offsets
    0 / 12 / 8 modulo 16 (row stride V + 2 = 16387 floats) give the outputs of the same rows at stride 16512."""
    V = 16385
    x = R.grid_logits(3, V, 651, 0.001)
    seen = np.zeros((3, V), bool)
    seen[:, [0, 31, 32, V - 1]] = True
    lg, sw = upload(x, seen)
    odd = torch.full((3, V + 2), 1e30, dtype=torch.float32, device=DEV)
    odd[:, :V] = torch.from_numpy(x).to(DEV)
    assert [(odd.data_ptr() + 4 * r * odd.stride(0)) % 16 for r in range(3)] == [0, 12, 8]
    for top_k, top_p in ((100, 0.8), (0, 0.5), (64, 1.0), (0, 1.0)):
        for st in range(4):
            a = op_chat_sample(lg, sw, V, 1.3, 0.7, top_k, top_p, seed=6, step=st)
            b = op_chat_sample(odd, sw, V, 1.3, 0.7, top_k, top_p, seed=6, step=st)
            assert _bits(a[0]).tolist() == _bits(b[0]).tolist() and all(p.tolist() == q.tolist() for p, q in zip(a[1:], b[1:]))
            n1 = op_chat_sample(odd[1:2], sw[1:2], V, 1.3, 0.7, top_k, top_p, seed=6, step=st)
            assert [int(v[0]) for v in n1[1:]] == [int(v[1]) for v in a[1:]]


@pytest.mark.parametrize("V", [1, 63])
def test_small_vocabularies(V):
    x = R.grid_logits(2, V, 701, 0.3) if V > 1 else np.array([[0.5], [-np.inf]], np.float32)
    lg, sw = upload(x)
    refs = [S.Row(row, temperature=0.7) for row in x]
    for top_k, top_p in ((0, 1.0), (0, 0.8), (5, 0.8), (100, 0.5), (1, 1.0)):
        for st in range(16):
            sc, tk, kept, cut = op_chat_sample(lg, sw, V, 1.0, 0.7, top_k, top_p, seed=2, step=st)
            for i, r in enumerate(refs):
                n = r.n_kept(top_k, top_p)
                assert r.candidates == 0 or r.interval(top_k, top_p)[2] > 1e-4
                assert kept[i] == n and cut[i] == r.cut_token(n)
                if n:
                    assert int(tk[i]) in r.order[:n] and sc[i] == r.s[tk[i]]
                else:
                    assert tk[i] == -1 and sc[i] == -np.inf


# ----------------------------------------------------------------------------------- masked rows ---
def test_masked_rows():
    """an all -inf row returns (-inf, -1, 0, -1), not what an earlier call left in the buffers; three finite tokens at
    top_k = 6 are drawn among those three; a NaN logit is never drawn (nor counted)"""
    x = R.grid_logits(3, 1000, 311)
    keep = [17, 500, 999]
    x[0] = -np.inf
    x[1] = -np.inf
    x[1, keep] = [0.5, 2.0, -1.0]
    best = int(np.argmax(x[2]))
    x[2, best] = np.nan
    full, _ = upload(R.grid_logits(3, 1000, 312))
    lg, sw = upload(x)
    drawn = set()
    for st in range(64):
        if st % 16 == 0:
            _, tk, kept, _ = op_chat_sample(full, sw, 1000, 1.0, 1.0, 6, 1.0, 11, st)       # the buffers hold three valid draws
            assert np.all(tk >= 0) and kept.tolist() == [6, 6, 6]
        sc, tk, kept, cut = op_chat_sample(lg, sw, 1000, 1.0, 1.0, 6, 1.0, 11, st)
        assert (sc[0], tk[0], kept[0], cut[0]) == (-np.inf, -1, 0, -1), st
        assert int(tk[1]) in keep and kept[1] == 3 and cut[1] == 999 and sc[1] == x[1, tk[1]], st
        top6 = np.argsort(-np.where(np.isnan(x[2]), -np.inf, x[2]), kind="stable")[:6]
        assert int(tk[2]) in top6 and tk[2] != best and kept[2] == 6 and cut[2] == top6[5]
        drawn.add(int(tk[1]))
    assert len(drawn) >= 2
    sc, tk, kept, cut = op_chat_sample(lg, sw, 1000, 1.0, 1.0, 0, 1.0, 11, 0)
    assert kept.tolist() == [0, 3, 999]


# -------------------------------------------------------------------------------- bad arguments ---
def test_bad_arguments_leave_outputs_and_the_present_sampler():
    x = R.grid_logits(2, 100, 801, 0.05)
    lg, sw = upload(x)
    before = op_chat_select(R.SAMPLE, lg, sw, 100, [0, 1, 2], 8, 1, temperature=0.7, seed=4, step=2)
    good = dict(device=0, logits_ptr=P(lg), ld=lg.stride(0), V=100, seen_ptr=P(sw), words=sw.stride(0), n=2, penalty=1.0,
                temperature=0.7, top_k=100, top_p=0.8, seed=1, step=0)

    def outs():
        return [np.full(2, 7.5, np.float32), np.full(2, 77, np.int32), np.full(2, 77, np.int32), np.full(2, 77, np.int32)]

    bad = [(dict(temperature=0.0), 1), (dict(temperature=-1.0), 1), (dict(temperature=float("nan")), 1), (dict(penalty=0.0), 1),
           (dict(penalty=-2.0), 1), (dict(top_p=0.0), 1), (dict(top_p=-0.5), 1), (dict(top_p=1.0000001), 1), (dict(top_p=float("nan")), 1),
           (dict(top_k=-1), 1), (dict(n=0), 1), (dict(n=-3), 1), (dict(n=17), 4), (dict(logits_ptr=None), 1), (dict(seen_ptr=None), 1),
           (dict(V=0), 1), (dict(V=200), 1), (dict(words=3), 1)]
    for kw, status in bad:
        o = outs()
        assert op_chat_sample_raw(**dict(good, **kw), outs=o) == status, kw
        assert o[0].tolist() == [7.5, 7.5] and all(a.tolist() == [77, 77] for a in o[1:]), kw
    for k in range(4):
        o = outs()
        o[k] = None
        assert op_chat_sample_raw(**good, outs=o) == 1, k
        assert all(a is None or a.tolist() in ([7.5, 7.5], [77, 77]) for a in o)
    o = outs()
    assert op_chat_sample_raw(**good, outs=o) == 0 and np.all(o[1] >= 0)
    after = op_chat_select(R.SAMPLE, lg, sw, 100, [0, 1, 2], 8, 1, temperature=0.7, seed=4, step=2)
    for a, b in zip(before, after):
        assert a.view(np.uint32).tolist() == b.view(np.uint32).tolist()


# ----------------------------------------------------------------------------------- model level ---
@pytest.fixture(scope="module")
def tiny():
    return load_tiny_chat()


def test_nucleus_top_p_1_equals_top_k_generation(tiny):
    cfg, enc, head, chat, F, items, tok = tiny
    kw = dict(max_new_tokens=12, do_sample=True, temperature=0.7, repetition_penalty=1.02, seed=5)
    a = generate_items(chat, items, nucleus=NucleusSampling(1.0, 50), **kw)
    b = generate_items(chat, items, top_k=50, **kw)
    assert a == b and all(len(t) >= 1 for t in a)


def test_nucleus_generation_is_seeded(tiny):
    cfg, enc, head, chat, F, items, tok = tiny
    kw = dict(max_new_tokens=32, do_sample=True, temperature=0.7, repetition_penalty=1.05, nucleus=NucleusSampling(0.8, 100), eos=-1)
    a = generate_items(chat, items[:1], seed=5, **kw)
    assert a == generate_items(chat, items[:1], seed=5, **kw) and len(a[0]) == 32
    assert a != generate_items(chat, items[:1], seed=6, **kw)


def test_teacher_forced_draws_lie_in_the_reference_kept_set(tiny):
    """every step: the row's logits come back to the host, the reference's kept set is computed from them and the seen ids so
    far, and the device's draw, n_kept and cut_token are checked against it (n_kept inside the DELTA interval)"""
    cfg, enc, head, chat, F, items, tok = tiny
    V = cfg.vocab_size
    chat.prefill(0, 0, items[0])
    seen = np.zeros(V, bool)
    for st in range(12):
        r = S.Row(chat.logits(0), seen, 1.05, 0.7)
        sc, tk, kept, cut = chat.sample([0], repetition_penalty=1.05, temperature=0.7, top_k=100, top_p=0.8, seed=13, step=st)
        lo, hi, _ = r.interval(100, 0.8)
        n = int(kept[0])
        assert lo <= n <= hi and int(cut[0]) == r.cut_token(n), st
        assert int(tk[0]) in r.order[:n] and sc[0] == r.s[tk[0]], st
        seen[int(tk[0])] = True
        chat.step([0], [0], [int(tk[0])])


def test_handle_entry_refuses_bad_arguments(tiny):
    """vr_chat_sample checks as vr_op_chat_sample does, plus the rows: one without logits is VR_ERR_STATE (3), more rows than
    the handle holds VR_ERR_CAPACITY (4); a refused call changes nothing — the next good draw is the draw it was before"""
    from visrag_amd._lib import VisragHipError
    cfg, enc, head, chat, F, items, tok = tiny
    chat.prefill(0, 0, items[2])
    good = dict(repetition_penalty=1.05, temperature=0.7, top_k=100, top_p=0.8, seed=3, step=0)
    before = chat.sample([0], **good)
    for rows, kw, status in (([0], dict(temperature=0.0), 1), ([0], dict(repetition_penalty=0.0), 1), ([0], dict(top_p=0.0), 1),
                             ([0], dict(top_p=1.5), 1), ([0], dict(top_k=-1), 1), ([], {}, 1), ([0] * 10, {}, 4), ([-1], {}, 3),
                             ([9], {}, 3)):
        with pytest.raises(VisragHipError, match=f"status {status}"):
            chat.sample(rows, **dict(good, **kw))
    chat2 = type(chat)(enc, max_len=64, max_rows=2, dim_model_base=256.0, max_slots=1, max_new=8)
    try:
        chat2.load_head(head.cuda())
        with pytest.raises(VisragHipError, match="status 3"):
            chat2.sample([1], **good)                           # in range, but no logits yet
    finally:
        chat2.close()
    after = chat.sample([0], **good)
    assert all(a.view(np.uint32).tolist() == b.view(np.uint32).tolist() for a, b in zip(before, after))


def test_public_chat_with_answer_defaults(tiny):
    import os
    from PIL import Image
    from tests.chat_sample_util import HERE, QUESTIONS
    from visrag_amd.answer import answer_page_concatenation
    from visrag_amd.generation import GenerationConfig
    from visrag_amd.modeling import DRModelForInference
    cfg, enc, head, chat, F, items, tok = tiny
    model = DRModelForInference(cfg, enc).lm_q.attach_generator(head.cuda(), GenerationConfig(dim_model_base=256.0),
                                                                max_inp_length=700, max_new_tokens=20, num_beams=3)
    img = Image.open(os.path.join(HERE, "golden", "inputs", "cat.jpeg")).convert("RGB")
    msgs = [[{"role": "user", "content": QUESTIONS[0]}]]
    a = model.chat([img], msgs, tok, sampling=True, assistant_turn=True, answer_defaults=True, max_new_tokens=8, seed=11)
    assert a == model.chat([img], msgs, tok, sampling=True, assistant_turn=True, answer_defaults=True, max_new_tokens=8, seed=11)
    assert isinstance(a[0], str) and a[0]
    # the defaults are overridable by their own keys only, and the old path next to it is untouched
    b = model.chat([img], msgs, tok, sampling=True, assistant_turn=True, answer_defaults=True, max_new_tokens=8, seed=11, top_k=1)
    g = model.chat([img], msgs, tok, sampling=True, assistant_turn=True, answer_defaults=True, max_new_tokens=8, seed=12, top_k=1)
    assert b == g                                                # top_k = 1: greedy whatever the seed
    assert answer_page_concatenation(model, tok, msgs[0], [img], max_new_tokens=6, sampling=True, seed=11) == \
        answer_page_concatenation(model, tok, msgs[0], [img], max_new_tokens=6, sampling=True, seed=11)
    with pytest.raises(NotImplementedError):
        model.generate(data_list=["<用户>hi"], tokenizer=tok, top_p=0.5)
