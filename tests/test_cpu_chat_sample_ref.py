"""The nucleus sampler's reference (tests/chat_sample_ref.py) on hand-worked rows and against transformers' warpers, and the
host side of the feature: NucleusSampling's checks, the answer package's generation defaults, generate_items' argument rules.
No GPU."""
import numpy as np
import pytest

from tests import chat_ref
from tests import chat_sample_ref as S
from visrag_amd.generation import NucleusSampling, answer_chat_generation_config, chat_generation_config, generate_items

P4 = [50.0, 30.0, 15.0, 5.0]            # masses of probabilities 0.5 / 0.3 / 0.15 / 0.05 (exact in fp64, like their sums)


@pytest.mark.parametrize("top_p,kept", [(0.5, 1), (0.51, 2), (0.8, 2), (0.81, 3), (0.95, 3), (0.96, 4), (1.0, 4)])
def test_four_tokens_by_hand(top_p, kept):
    """A_j = 0, 0.5, 0.8, 0.95 of Z: kept iff A_j < top_p — an edge that is met exactly is NOT below it (HF removes a token
    whose ascending cumulative probability is <= 1 - top_p)."""
    assert S.kept_count(P4, 0, top_p) == kept
    assert S.kept_count(P4, 4, top_p) == kept and S.kept_count(P4, 9, top_p) == kept


@pytest.mark.parametrize("top_p,kept", [(0.5, 1), (0.51, 1), (0.62, 1), (0.63, 2), (0.8, 2), (0.81, 2), (1.0, 2)])
def test_four_tokens_under_top_k_2(top_p, kept):
    """top_k = 2 first: Z = 80, A = 0, 50 -> A_1 / Z = 0.625; top_k = 1 keeps one whatever top_p"""
    assert S.kept_count(P4, 2, top_p) == kept
    assert S.kept_count(P4, 1, top_p) == 1


def test_row_from_logits_order_and_penalty():
    """The logits path: log-probabilities at scattered ids, the best one seen and penalised below the second"""
    x = np.full(40, -np.inf, np.float32)
    ids = [33, 7, 21, 2]
    x[ids] = np.log(np.array(P4) / 100.0).astype(np.float32)
    r = S.Row(x, temperature=1.0)
    assert r.order.tolist() == ids and r.candidates == 4
    np.testing.assert_allclose(r.w, np.array(P4) / 50.0, rtol=1e-6)
    assert [r.n_kept(0, p) for p in (0.45, 0.55, 0.75, 0.85, 0.97)] == [1, 2, 2, 3, 4]
    assert r.kept(0, 0.85).tolist() == ids[:3] and r.cut_token(3) == 21
    seen = np.zeros(40, bool)
    seen[33] = True
    r2 = S.Row(x, seen, penalty=2.0, temperature=0.5)           # log 0.5 * 2 = log 0.25 < log 0.3
    assert r2.order.tolist() == [7, 33, 21, 2]
    assert r2.s[33] == np.float32(x[33] * np.float32(2.0)) and r2.z[33] == np.float32(r2.s[33] * np.float32(2.0))
    lo, hi, edge = r.interval(0, 0.85)
    assert lo == hi == 3 and abs(edge - 0.05) < 1e-6


def test_tie_tier_keeps_the_lower_ids():
    x = np.zeros(1000, np.float32)
    r = S.Row(x, temperature=0.7)
    assert r.order.tolist() == list(range(1000))
    assert (r.n_kept(0, 0.5), r.n_kept(0, 0.25), r.n_kept(100, 0.5), r.n_kept(100, 0.25)) == (500, 250, 50, 25)
    assert r.cut_token(500) == 499 and r.cut_token(25) == 24
    # two tiers: ids 5 and 9 lead, the rest tie below; -0.0 sorts below +0.0 as on the device
    x = np.full(10, -1.0, np.float32)
    x[[5, 9]] = 2.0
    x[3], x[4] = 0.0, -0.0
    assert S.Row(x).order.tolist()[:4] == [5, 9, 3, 4]
    assert S.Row(x).kept(3, 1.0).tolist() == [5, 9, 3]


def test_masked_row():
    x = np.full(64, -np.inf, np.float32)
    r = S.Row(x)
    assert r.candidates == 0 and r.n_kept(0, 0.8) == 0 and r.n_kept(5, 1.0) == 0 and r.cut_token(0) == -1
    assert r.interval(0, 0.8)[:2] == (0, 0)
    x[[17, 50, 63]] = [0.5, 2.0, -1.0]
    x[3] = np.nan
    r = S.Row(x)
    assert r.order.tolist() == [50, 17, 63]                     # NaN and -inf are no candidates
    assert r.n_kept(6, 1.0) == 3 and r.n_kept(2, 1.0) == 2


@pytest.mark.parametrize("T", [0.7, 1.5])
def test_against_transformers_warpers(T):
    """TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper(min_tokens_to_keep=1) on rows of distinct values
    (on exact ties at the k-th value HF keeps every tied token: the stated difference), in fp64 so that only the definition is
    compared.  HF divides the fp64 logit by T where the reference rounds s * (1 / T) to fp32: masses up to ~1e-6 apart, so a
    configuration whose edge lies within 1e-5 of top_p is not compared (few: the count is asserted)."""
    torch = pytest.importorskip("torch")
    tf = pytest.importorskip("transformers")
    compared = 0
    for seed in (11, 12, 13):
        x = chat_ref.grid_logits(1, 1000, seed, 0.01)[0]
        r = S.Row(x, temperature=T)
        for top_k in (0, 1, 2, 64, 100):
            for top_p in (0.1, 0.5, 0.8, 0.95, 1.0):
                if r.interval(top_k, top_p)[2] < 1e-5:
                    continue
                sc = torch.from_numpy(x.astype(np.float64))[None]
                ids = torch.zeros((1, 0), dtype=torch.long)
                sc = tf.TemperatureLogitsWarper(T)(ids, sc)
                if top_k:
                    sc = tf.TopKLogitsWarper(top_k=top_k)(ids, sc)
                if top_p < 1.0:
                    sc = tf.TopPLogitsWarper(top_p=top_p, min_tokens_to_keep=1)(ids, sc)
                hf = set(torch.nonzero(sc[0] > -float("inf")).flatten().tolist())
                assert hf == set(r.kept(top_k, top_p).tolist()), (seed, top_k, top_p)
                compared += 1
    assert compared >= 70                                       # of 75


def test_nucleus_sampling_checks():
    n = NucleusSampling()
    assert (n.top_p, n.top_k) == (0.8, 100)
    assert NucleusSampling(1.0, 0).top_k == 0
    with pytest.raises(Exception):
        n.top_p = 0.5                                           # frozen
    for bad in ((0.0, 10), (-0.1, 10), (1.0001, 10), (float("nan"), 10), (0.5, -1), (0.5, 2.5), (0.5, True)):
        with pytest.raises(ValueError):
            NucleusSampling(*bad)


def test_answer_generation_config_merge():
    """weighted_selection/MiniCPMV20/modeling_minicpmv.py:361-377: the mode's defaults, only THEIR keys overridden"""
    assert answer_chat_generation_config(True, {}) == {"top_p": 0.8, "top_k": 100, "temperature": 0.7, "do_sample": True,
                                                       "repetition_penalty": 1.05}
    assert answer_chat_generation_config(True, {"top_p": 0.5, "num_beams": 4, "seed": 3})["top_p"] == 0.5
    assert "num_beams" not in answer_chat_generation_config(True, {"num_beams": 4, "seed": 3})
    assert answer_chat_generation_config(False, {"top_p": 0.5, "repetition_penalty": 1.0}) == {"num_beams": 3, "repetition_penalty": 1.0}
    assert chat_generation_config(True, {}) == {"temperature": 0.7, "do_sample": True, "repetition_penalty": 1.02}   # untouched


class _NoChat:
    max_rows, max_slots, max_new = 3, 1, 32


def test_generate_items_nucleus_argument_rules():
    nuc = NucleusSampling(0.8, 100)
    for kw in ({"nucleus": nuc}, {"nucleus": nuc, "do_sample": False}, {"nucleus": nuc, "do_sample": True, "num_beams": 3},
               {"nucleus": nuc, "do_sample": True, "top_k": 100}, {"nucleus": nuc, "do_sample": True, "top_k": 0},
               {"nucleus": (0.8, 100), "do_sample": True}):
        with pytest.raises(ValueError):
            generate_items(_NoChat(), [], **kw)
    assert generate_items(_NoChat(), [], nucleus=nuc, do_sample=True) == []
    # the HF-named options stay refused next to a nucleus ...
    with pytest.raises(NotImplementedError):
        generate_items(_NoChat(), [], nucleus=nuc, do_sample=True, top_p=0.9)
    # ... and without one every old refusal still raises
    for kw in ({"top_p": 0.9}, {"do_sample": True, "top_k": 0}, {"do_sample": True, "top_k": 100}, {"do_sample": True, "top_k": 65},
               {"do_sample": True, "num_beams": 3}, {"typical_p": 0.5}):
        with pytest.raises(NotImplementedError):
            generate_items(_NoChat(), [], **kw)


def test_generate_items_sends_every_draw_to_sample():
    """A stand-in chat that records its calls: with a nucleus, every select of the lockstep round is ONE sample call over
    the pending items' rows, with the nucleus' top_k / top_p and step = 0, 1, 2, ...; select is never called."""
    calls = []

    class _Chat:
        max_rows, max_slots, max_new = 4, 4, 32

        def prefill(self, slot, row, item):
            calls.append(("prefill", slot, row))

        def step(self, slots, rows, tokens):
            calls.append(("step", list(rows), list(tokens)))

        def select(self, *a, **kw):
            raise AssertionError("select must not be called with a nucleus")

        def sample(self, rows, repetition_penalty, temperature, top_k, top_p, seed, step):
            calls.append(("sample", list(rows), repetition_penalty, temperature, top_k, top_p, seed, step))
            n = len(rows)
            # item of row 0 ends (eos = 2) at step 1, the others go on
            tok = np.array([2 if (r == 0 and step == 1) else 10 + r + step for r in rows], np.int32)
            return np.full(n, 0.5, np.float32), tok, np.full(n, 7, np.int32), np.full(n, 3, np.int32)

    class _Item:
        input_ids = [1, 5]

    out = generate_items(_Chat(), [_Item(), _Item(), _Item()], max_new_tokens=3, do_sample=True, temperature=0.7,
                         repetition_penalty=1.05, seed=9, nucleus=NucleusSampling(0.8, 100))
    assert out == [[10, 2], [11, 12, 13], [12, 13, 14]]
    samples = [c for c in calls if c[0] == "sample"]
    assert [c[1] for c in samples] == [[0, 1, 2], [0, 1, 2], [1, 2]]
    assert all(c[2:7] == (1.05, 0.7, 100, 0.8, 9) for c in samples) and [c[7] for c in samples] == [0, 1, 2]
