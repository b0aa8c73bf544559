"""MiniCPM-V 2.0 answer generation on the device (vr_chat_*, visrag_amd/generation.py) against the fp32 CPU oracle.

The oracle is the repository's restatement of the decoder (oracle/visrag_ret_oracle.py) plus the head of
modeling_minicpm.py:1411-1412, logits = lm_head(h / (hidden / dim_model_base)); the device runs the bf16 route."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import visrag_ret_oracle as O  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.config import full_config, tiny_config  # noqa: E402
from visrag_amd.engine import HipEncoder  # noqa: E402
from visrag_amd.generation import BEAM, GREEDY, SAMPLE, HipChat, generate_items  # noqa: E402
from visrag_amd.preprocess import PreparedItem, prepare_item  # noqa: E402
from visrag_amd.synth import iter_synth_weights, synth_lm_head, synth_pages, synth_state_dict  # noqa: E402
from visrag_amd.tokenizer import StandInTokenizer  # noqa: E402

DMB = 64.0          # tiny config: hidden 256 -> the head's input is h / 4
# bf16 route vs the fp32 oracle, relative to max |logit| (first MI355X run: prefill 5.9e-3 / 7.3e-3, steps 5.1e-3 .. 1.01e-2;
# full dims, step vs fresh prefill: 1.37e-2)
LOGIT_BAR = 2e-2


@pytest.fixture(scope="module")
def tiny():
    cfg = tiny_config()
    enc = HipEncoder(cfg, device=0, max_images=4, max_tokens=512, max_seqs=8)
    enc.load_state_dict(iter_synth_weights(cfg, 0, device="cuda"))
    W = synth_state_dict(cfg, 0)
    head = synth_lm_head(cfg, 0)
    chat = HipChat(enc, max_len=256, max_rows=9, dim_model_base=DMB, max_slots=3, max_new=200)
    chat.load_head(head.cuda())
    return cfg, enc, W, head, chat


def _text_item(cfg, text):
    return prepare_item(text, None, StandInTokenizer(cfg.vocab_size), cfg, 2048)


def _page_item(cfg, seed=0):
    from PIL import Image
    page = synth_pages(1, size=cfg.scale_resolution, seed=seed)[0]
    return prepare_item("<用户>what is shown here", Image.fromarray(page), StandInTokenizer(cfg.vocab_size), cfg, 2048)


def _oracle_logits(cfg, W, head, item, extra=()):
    ids = list(item.input_ids) + list(extra)
    taps = {}
    O.encode(W, cfg, [ids], [item.image_bound], [item.slices], taps=taps)
    h = taps["last_hidden"][0, len(ids) - 1]
    return (h / (cfg.hidden_size / DMB) @ head.T).numpy()


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_prefill_and_step_logits_match_oracle(tiny):
    cfg, enc, W, head, chat = tiny
    for item in (_page_item(cfg), _text_item(cfg, "<用户>a short question about the page")):
        chat.prefill(0, 0, item)
        got = chat.logits(0)
        ref = _oracle_logits(cfg, W, head, item)
        e0 = _rel(got, ref)
        print("prefill rel err", e0)
        assert e0 < LOGIT_BAR
        # teacher-forced steps: the oracle's argmax continues the prompt
        extra = []
        for t in range(4):
            tok = int(np.argmax(ref))
            extra.append(tok)
            chat.step([0], [0], [tok])
            got = chat.logits(0)
            ref = _oracle_logits(cfg, W, head, item, extra)
            e = _rel(got, ref)
            print("step", t, "rel err", e)
            assert e < LOGIT_BAR


def test_batch_invariance(tiny):
    cfg, enc, W, head, chat = tiny
    a = _text_item(cfg, "<用户>first prompt with several words in it")
    b = _text_item(cfg, "<用户>second")
    c = _page_item(cfg, seed=3)
    for nb in (1, 3):
        alone = generate_items(chat, [a], max_new_tokens=10, num_beams=nb, repetition_penalty=1.2)[0]
        batched = generate_items(chat, [b, a, c], max_new_tokens=10, num_beams=nb, repetition_penalty=1.2)
        assert batched[1] == alone, (nb, alone, batched)
        assert all(len(x) >= 1 for x in batched)


def test_beam_search_rules_on_device_candidates(tiny):
    """The beam candidates of the device equal log_softmax + penalty + beam score of its own logits (host restatement)."""
    cfg, enc, W, head, chat = tiny
    item = _text_item(cfg, "<用户>beam check")
    chat.prefill(0, 0, item)
    chat.reorder([1, 2], [0, 0])
    chat.step([0, 0, 0], [0, 1, 2], [7, 9, 7])
    chat.step([0, 0, 0], [0, 1, 2], [11, 7, 13])
    bs = [-0.5, -0.7, -1.1]
    sc, tk, pa = chat.select(BEAM, [[0, 1, 2]], 6, bs, repetition_penalty=1.2)
    seen = [{7, 11}, {9, 7}, {7, 13}]
    allsc = []
    for r in range(3):
        l = chat.logits(r).astype(np.float64)
        lp = l - (l.max() + np.log(np.exp(l - l.max()).sum()))
        for t in seen[r]:
            lp[t] = lp[t] * 1.2 if lp[t] < 0 else lp[t] / 1.2
        allsc.append(lp + bs[r])
    flat = np.concatenate(allsc)
    order = np.argsort(-flat, kind="stable")[:6]
    assert [(int(i) // cfg.vocab_size, int(i) % cfg.vocab_size) for i in order] == list(zip(pa[0].tolist(), tk[0].tolist()))
    np.testing.assert_allclose(sc[0], flat[order], rtol=0, atol=1e-4)
    g_sc, g_tk, _ = chat.select(GREEDY, [[1]], 1, repetition_penalty=1.2)
    l = chat.logits(1)
    for t in seen[1]:
        l[t] = l[t] * 1.2 if l[t] < 0 else l[t] / 1.2
    assert int(g_tk[0, 0]) == int(np.argmax(l))


def test_sampling_seeded_and_inside_top50(tiny):
    cfg, enc, W, head, chat = tiny
    item = _text_item(cfg, "<用户>sample something")
    runs = [generate_items(chat, [item], max_new_tokens=6, do_sample=True, temperature=0.7, repetition_penalty=1.02, seed=s)[0]
            for s in (5, 5, 6)]
    assert runs[0] == runs[1]
    # every drawn token lies in the top 50 of the penalised logits
    chat.prefill(0, 0, item)
    seen = set()
    for step, tok in enumerate(runs[0]):
        l = chat.logits(0)
        for t in seen:
            l[t] = l[t] * 1.02 if l[t] < 0 else l[t] / 1.02
        assert tok in set(np.argsort(-l)[:50].tolist())
        _, got, _ = chat.select(SAMPLE, [[0]], 1, repetition_penalty=1.02, temperature=0.7, top_k=50, seed=5, step=step)
        assert int(got[0, 0]) == tok
        if tok == 2 or step + 1 == len(runs[0]):
            break
        chat.step([0], [0], [tok])
        seen.add(tok)


def _three_rows(chat, item):
    """rows 0, 1, 2 on slot 0 with tails of 2, 5 and 9 tokens and different seen sets"""
    chat.prefill(0, 0, item)
    chat.reorder([1, 2], [0, 0])
    for t in range(9):
        rows = [r for r, n in ((0, 2), (1, 5), (2, 9)) if t < n]
        chat.step([0] * len(rows), rows, [20 + 37 * r + 3 * t for r in rows])
    assert [chat.row_state(r) for r in range(3)] == [(0, 2), (0, 5), (0, 9)]


def _next_step(chat, rows, tokens, beam_order):
    """step `rows` with `tokens`; -> per row (logits, greedy top-8 at penalty 1.2), and the beam candidates of the group"""
    chat.step([0] * len(rows), rows, tokens)
    per_row = [(chat.logits(r), chat.select(GREEDY, [[r]], 8, repetition_penalty=1.2)) for r in rows]
    beam = chat.select(BEAM, [beam_order], 6, [-0.5, -0.7, -1.1], repetition_penalty=1.2)
    return per_row, beam


WIDE_SCORES = [-0.5, -0.52, -0.55]       # close together: every row of the group has candidates among the 64 best


def _beam_by_parent(chat, scores):
    """the 64 best beam candidates of the group [0, 1, 2] at penalty 1.2 -> per parent row its (score, token) list, best first"""
    sc, tk, pa = chat.select(BEAM, [[0, 1, 2]], 64, scores, repetition_penalty=1.2)
    return [[(sc[0, i], tk[0, i]) for i in range(64) if pa[0, i] == r] for r in range(3)]


@pytest.mark.parametrize("parents", [[1, 2, 0], [2, 2, 0]])
def test_reorder_is_a_permutation(tiny, parents):
    """vr_chat_reorder with rows that are source AND destination (the two-pass copy of chat_tail_move / chat_seen_move):
    after reorder([0, 1, 2], parents) row r IS row parents[r] of an untouched twin run — next-step logits bit for bit, and
    the same greedy / beam candidates at penalty 1.2 (the seen sets moved with the tails)."""
    cfg, enc, W, head, chat = tiny
    item = _text_item(cfg, "<用户>three beams with tails of their own")
    tok = [301, 302, 303]
    _three_rows(chat, item)
    twin, twin_beam = _next_step(chat, [0, 1, 2], tok, [0, 1, 2])
    twin_wide = _beam_by_parent(chat, WIDE_SCORES)
    assert not np.array_equal(twin[0][0], twin[1][0]) and not np.array_equal(twin[1][0], twin[2][0])
    _three_rows(chat, item)
    chat.reorder([0, 1, 2], parents)
    assert [chat.row_state(r) for r in range(3)] == [(0, (2, 5, 9)[p]) for p in parents]
    got, _ = _next_step(chat, [0, 1, 2], [tok[p] for p in parents], [0, 1, 2])
    for r, p in enumerate(parents):
        assert np.array_equal(got[r][0], twin[p][0]), (r, p)
        for a, b in zip(got[r][1], twin[p][1]):
            assert np.array_equal(a, b), (r, p)
    # the beam select of the whole group, rows duplicated or not: row r carrying the twin's beam score of row parents[r]
    # contributes the twin row's candidates, bit for bit, as far as both lists reach into the 64 best
    wide = _beam_by_parent(chat, [WIDE_SCORES[p] for p in parents])
    for r, p in enumerate(parents):
        m = min(len(wide[r]), len(twin_wide[p]))
        assert m >= 1, (r, p)
        assert wide[r][:m] == twin_wide[p][:m], (r, p)
    if sorted(parents) == [0, 1, 2]:         # the group with its old rows in the old order: the same candidates, parents included
        where = [parents.index(p) for p in range(3)]
        beam = chat.select(BEAM, [where], 6, [-0.5, -0.7, -1.1], repetition_penalty=1.2)
        for a, b in zip(beam, twin_beam):
            assert np.array_equal(a, b)


def test_batch_mates_do_not_change_a_row(tiny):
    """A row's sums do not depend on its batch mates (the design rule stated at chat_attn_kernel's gsplit): the logits of a row
    stepped alone equal, bit for bit, those of the same row inside a 9-row step over 3 slots."""
    cfg, enc, W, head, chat = tiny
    items = [_text_item(cfg, "<用户>first prompt with several words in it"), _page_item(cfg, seed=3), _text_item(cfg, "<用户>second")]

    def setup():
        for s, it in enumerate(items):
            chat.prefill(s, 3 * s, it)
            chat.reorder([3 * s + 1, 3 * s + 2], [3 * s, 3 * s])
        chat.step([r // 3 for r in range(9)], list(range(9)), [40 + 11 * r for r in range(9)])

    setup()
    chat.step([r // 3 for r in range(9)], list(range(9)), [500 + r for r in range(9)])
    together = {r: chat.logits(r) for r in (0, 4, 8)}
    for r in (0, 4, 8):
        setup()
        chat.step([r // 3], [r], [500 + r])
        assert np.array_equal(chat.logits(r), together[r]), r


def test_tail_across_the_chunk_edge(tiny):
    """260 teacher-forced tokens with max_new = 300: the decode attention's tail loop crosses CHAT_KEYS = 256 keys.  Logits at
    255, 256, 257 and 260 generated tokens against the oracle's encode of the extended prompt (first MI355X run: 6.2e-3,
    5.5e-3, 8.0e-3, 7.8e-3)."""
    cfg, enc, W, head, _ = tiny
    chat = HipChat(enc, max_len=330, max_rows=1, dim_model_base=DMB, max_slots=1, max_new=300)
    chat.load_head(head.cuda())
    item = _text_item(cfg, "<用户>a long answer follows")
    toks = np.random.default_rng(7).integers(16, cfg.vocab_size, 260).tolist()
    chat.prefill(0, 0, item)
    errs = {}
    for n, t in enumerate(toks, start=1):
        chat.step([0], [0], [t])
        if n in (255, 256, 257, 260):
            errs[n] = _rel(chat.logits(0), _oracle_logits(cfg, W, head, item, toks[:n]))
    chat.close()
    print("tail across the chunk edge: rel err per generated length", errs)
    assert chat.max_new == 300 and all(e < LOGIT_BAR for e in errs.values()), errs


def test_capacity_errors_leave_state(tiny):
    cfg, enc, W, head, chat = tiny
    item = _text_item(cfg, "<用户>capacity")
    chat.prefill(0, 0, item)
    chat.step([0], [0], [5])
    before = chat.row_state(0), chat.logits(0)
    with pytest.raises(_lib.VisragHipError, match="status 4"):
        chat.step([0] * 10, list(range(10)), [5] * 10)             # more rows than max_rows
    long_item = PreparedItem(input_ids=[1] + [20] * 255, image_bound=[], slices=[])
    with pytest.raises(_lib.VisragHipError, match="status 4"):
        chat.prefill(1, 1, long_item)                              # a prompt of max_len tokens leaves no room
    assert chat.row_state(0) == before[0]
    assert np.array_equal(chat.logits(0), before[1])
    # filling the row up to max_new (its tail) and a second prompt up to max_len: the step past either fails, changes nothing
    for _ in range(chat.max_new - 1):
        chat.step([0], [0], [5])
    assert chat.row_state(0) == (0, chat.max_new)
    with pytest.raises(_lib.VisragHipError, match="status 4"):
        chat.step([0], [0], [5])
    assert chat.row_state(0) == (0, chat.max_new)
    long_item = PreparedItem(input_ids=[1] + [20] * 199, image_bound=[], slices=[])
    chat.prefill(1, 1, long_item)
    for _ in range(chat.max_len - 200):
        chat.step([1], [1], [5])
    with pytest.raises(_lib.VisragHipError, match="status 4"):
        chat.step([1], [1], [5])
    assert chat.row_state(1) == (1, chat.max_len - 200)


def test_encode_unchanged_by_chat(tiny):
    cfg, enc, W, head, chat = tiny
    items = [_page_item(cfg, seed=7), _text_item(cfg, "a query")]
    before = [enc.encode_items([it]).cpu().numpy() for it in items]
    chat.prefill(2, 3, items[0])
    chat.step([2], [3], [17])
    after = [enc.encode_items([it]).cpu().numpy() for it in items]
    for x, y in zip(before, after):
        assert np.array_equal(x, y)


def test_kv_cache_consistency_full_dims():
    """Production dims, synthetic weights: a decode step's logits equal a fresh prefill of the extended prompt (bf16)."""
    cfg = full_config()
    enc = HipEncoder(cfg, device=0, max_images=2, max_tokens=1024, max_seqs=2)
    enc.load_state_dict(iter_synth_weights(cfg, 1, device="cuda"))
    chat = HipChat(enc, max_len=800, max_rows=2, dim_model_base=256.0, max_slots=2, max_new=16)
    chat.load_head(synth_lm_head(cfg, 1, device="cuda"))
    rng = np.random.default_rng(0)
    ids = [1] + rng.integers(16, cfg.vocab_size, 600).tolist()
    item = PreparedItem(input_ids=ids, image_bound=[], slices=[])
    chat.prefill(0, 0, item)
    toks = [int(np.argmax(chat.logits(0)))]
    chat.step([0], [0], toks)
    toks.append(int(np.argmax(chat.logits(0))))
    chat.step([0], [0], toks[1:])
    step_logits = chat.logits(0)
    chat.prefill(1, 1, PreparedItem(input_ids=ids + toks, image_bound=[], slices=[]))
    fresh = chat.logits(1)
    e = _rel(step_logits, fresh)
    print("full-dims step vs prefill rel err", e)
    assert e < 2e-2
    chat.close()
    enc.close()


# ---- the reference model's recorded generation (tools/gen_golden_chat.py -> tests/golden/chat_tiny.npz) -------------------
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chat_tiny.npz")
QUESTIONS = ["What animal is in the picture?", "Describe the image.", "What is the capital of France?"]
# device vs the reference model's logits, relative to max |logit| (first MI355X run: worst 7.5e-3 over the three prompts'
# prefill + 19 teacher-forced steps)
REF_BAR = 1e-2
# decisions of the reference run whose margin exceeds 4 x REF_BAR x max|logit|, compared until the runs part (measured)
GREEDY_DECIDED = [0, 12, 14]
BEAM_DECIDED = [4, 0, 3]


class _Words(StandInTokenizer):
    def decode(self, ids):
        return " ".join(f"w{int(i)}" for i in ids) + " "


@pytest.fixture(scope="module")
def ref():
    from PIL import Image
    from visrag_amd.modeling import _prompt_item, chat_prompt
    cfg = tiny_config()
    F = np.load(FIX)
    enc = HipEncoder(cfg, device=0, max_images=4, max_tokens=1024, max_seqs=4)
    enc.load_state_dict(iter_synth_weights(cfg, 0, device="cuda"))
    head = synth_lm_head(cfg, 0)
    chat = HipChat(enc, max_len=720, max_rows=9, dim_model_base=float(F["dim_model_base"]), max_slots=3, max_new=32)
    chat.load_head(head.cuda())
    tok = _Words(cfg.vocab_size)
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs")
    items = []
    for p, name in enumerate(["cat.jpeg", "dog.jpg"]):
        img = Image.open(os.path.join(root, name)).convert("RGB")
        items.append(_prompt_item(*chat_prompt([{"role": "user", "content": QUESTIONS[p]}], img, tok, cfg), tok, 2048))
    items.append(_prompt_item("<用户>" + QUESTIONS[2], [], tok, 2048))
    for p, it in enumerate(items):
        assert it.input_ids == F[f"p{p}_ids"].tolist()
    return cfg, enc, head, chat, F, items, tok


def test_reference_logits_prefill_and_steps(ref):
    """Prefill logits of the last prompt token and teacher-forced step logits along the reference's greedy path."""
    cfg, enc, head, chat, F, items, tok = ref
    worst = 0.0
    for p, it in enumerate(items):
        ids, vals, toks = F[f"p{p}_greedy_top_ids"], F[f"p{p}_greedy_top_logits"], F[f"p{p}_greedy_tokens"]
        chat.prefill(0, 0, it)
        for s in range(len(toks)):
            got = chat.logits(0)[ids[s]]
            e = float(np.abs(got - vals[s]).max() / F[f"p{p}_greedy_absmax"][s])
            worst = max(worst, e)
            assert e < REF_BAR, (p, s, e)
            if s + 1 < len(toks):
                chat.step([0], [0], [int(toks[s])])
    print("reference logits: worst relative error", worst)


def _seqs(tokens, parents):
    """running beam sequences after every step, from the per-step (next tokens, parents)"""
    cur, out = [[]], []
    for t, p in zip(tokens, parents):
        cur = [cur[q] + [int(x)] for x, q in zip(t, p)]
        out.append(sorted(map(tuple, cur)))
    return out


def _beam_set_margins(F, p):
    """Per reference beam step: the score gap that decides the step's running set — between the last kept candidate and
    the next one, or, with an eos among the first num_beams + 1, the smallest gap among them (it decides the eos's rank).
    Candidates from the recorded per-prefix log-probs, penalty and beam scores as the reference applies them."""
    nb, V, pen = int(F["num_beams"]), 1000, np.float32(F["pen_beam"])
    pre, ln = F[f"p{p}_beam_q_prefix"], F[f"p{p}_beam_q_len"]
    table = {tuple(pre[i, :ln[i]].tolist()): (F[f"p{p}_beam_q_ids"][i], F[f"p{p}_beam_q_logprobs"][i]) for i in range(len(ln))}
    seqs, scores, out = [[]], [np.float32(0)], []
    for t, par in zip(F[f"p{p}_beam_next_tokens"], F[f"p{p}_beam_next_parents"]):
        cand = []
        for b, q in enumerate(seqs):
            ids, lp = table[tuple(q)]
            v = lp.copy()
            m = np.isin(ids, q)
            v[m] = np.where(v[m] < 0, v[m] * pen, v[m] / pen)
            cand += [(float(x + scores[b]), int(i), b) for x, i in zip(v, ids)]
        cand.sort(key=lambda c: (-c[0], c[2] * V + c[1]))
        top = cand[:nb + 1]
        gaps = [top[i][0] - top[i + 1][0] for i in range(nb)]
        out.append(min(gaps) if any(c[1] == 2 for c in top) else gaps[nb - 1])
        new = {(par[j], t[j]): j for j in range(nb)}
        scores = [np.float32(next(c[0] for c in cand if (c[2], c[1]) == (int(par[j]), int(t[j])))) for j in range(nb)]
        seqs = [seqs[int(par[j])] + [int(t[j])] for j in range(nb)]
    return out


def test_reference_greedy_and_beam_tokens(ref):
    """Greedy and beam (3, penalty 1.2) against the reference run, step by step until the two runs part: every step they
    share whose reference margin exceeds 4 x REF_BAR x max|logit| must decide alike; a parting step must be a narrow one."""
    cfg, enc, head, chat, F, items, tok = ref
    n_new = int(F["max_new"])
    g = generate_items(chat, items, max_new_tokens=n_new, num_beams=1, repetition_penalty=float(F["pen_greedy"]), details=True)
    b = generate_items(chat, items, max_new_tokens=n_new, num_beams=int(F["num_beams"]), repetition_penalty=float(F["pen_beam"]),
                       details=True)
    g_counts, b_counts = [], []
    for p in range(len(items)):
        ref_g, got = F[f"p{p}_greedy_tokens"].tolist(), g[p]["tokens"]
        n = 0
        for s, (m, a) in enumerate(zip(F[f"p{p}_greedy_margin"], F[f"p{p}_greedy_absmax"])):
            decisive = m > 4 * REF_BAR * a
            if s >= len(got) or got[s] != ref_g[s]:
                assert not decisive, (p, s, got, ref_g)
                break
            n += decisive
        g_counts.append(n)
        ref_b = _seqs(F[f"p{p}_beam_next_tokens"], F[f"p{p}_beam_next_parents"])
        margins = _beam_set_margins(F, p)
        steps = b[p]["steps"]
        got_b = _seqs([[t for _, t, _ in st[1]] for st in steps], [[q for _, _, q in st[1]] for st in steps])
        n = 0
        for s, (m, a) in enumerate(zip(margins, F[f"p{p}_beam_absmax"])):
            decisive = m > 4 * REF_BAR * a
            if s >= len(got_b) or got_b[s] != ref_b[s]:
                assert not decisive, (p, s)
                break
            n += decisive
        else:
            if b[p]["tokens"] == F[f"p{p}_beam_tokens"].tolist():
                assert abs(b[p]["score"] - float(F[f"p{p}_beam_score"])) < REF_BAR * float(F[f"p{p}_beam_absmax"].max()), p
        b_counts.append(n)
    g_counts, b_counts = [int(x) for x in g_counts], [int(x) for x in b_counts]
    print("decisive decisions compared: greedy", g_counts, "beam", b_counts)
    assert g_counts == GREEDY_DECIDED and b_counts == BEAM_DECIDED


def test_public_chat_and_generate(ref):
    """VisRAGRet.chat / generate (attach_generator) on the reference's cat prompt."""
    from PIL import Image
    from visrag_amd.generation import GenerationConfig, decode_text
    from visrag_amd.modeling import DRModelForInference
    cfg, enc, head, chat, F, items, tok = ref
    model = DRModelForInference(cfg, enc).lm_q.attach_generator(head.cuda(), GenerationConfig(dim_model_base=256.0),
                                                                max_inp_length=700, max_new_tokens=20, num_beams=3)
    img = Image.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inputs", "cat.jpeg")).convert("RGB")
    msgs = [[{"role": "user", "content": QUESTIONS[0]}]]
    ans = model.chat([img], msgs, tok, sampling=False, max_new_tokens=20)
    want = decode_text(generate_items(chat, items[:1], max_new_tokens=20, num_beams=3, repetition_penalty=1.2), tok)
    assert ans == want
    s1 = model.chat([img], msgs, tok, sampling=True, max_new_tokens=8, seed=11)
    assert s1 == model.chat([img], msgs, tok, sampling=True, max_new_tokens=8, seed=11)
    with pytest.raises(NotImplementedError):
        model.generate(data_list=["<用户>hi"], tokenizer=tok, top_p=0.5)
