"""Answer scoring on the device (vr_chat_score through HipChat.score, generation.score_items, VisRAGRet.score_answers /
choose / marginal_selection) against the fp32 CPU oracle, the reference model's recorded beams (tests/golden/chat_tiny.npz),
the device's own decode path, and the weighted-selection fixture's pages.

Bars.  LOGIT_BAR (bf16 route vs the fp32 oracle) and REF_BAR (vs the reference model) are the standing bars of
tests/test_gpu_chat.py, relative to a row's max |logit|.  A token log-prob is x_t - lse, 2-Lipschitz in the sup-norm of the
logits: its bar is twice the logit bar.  A sequence score is a mean of log-probs, each times 1 or the repetition penalty: the
mean of its tokens' bars times the penalty.  Where the rows' logits are not at hand the scale is the row's largest logit
(HipChat.score's top_logit), which never exceeds max |logit|: a bar never wider than the rule's."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import visrag_ret_oracle as O  # noqa: E402
from tests.answer_util import FIX as WFIX, Words, msgs_of, question_pages  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.config import tiny_config  # noqa: E402
from visrag_amd.engine import HipEncoder  # noqa: E402
from visrag_amd.generation import (BEAM, GenerationConfig, HipChat, beam_rule, generate_items, run_rule, score_items,  # noqa: E402
                                   sequence_score)
from visrag_amd.modeling import DRModelForInference, _prompt_item, chat_prompt  # noqa: E402
from visrag_amd.preprocess import PreparedItem, prepare_item  # noqa: E402
from visrag_amd.synth import iter_synth_weights, synth_lm_head, synth_pages, synth_state_dict  # noqa: E402
from visrag_amd.tokenizer import StandInTokenizer  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "chat_tiny.npz")
QUESTIONS = ["What animal is in the picture?", "Describe the image.", "What is the capital of France?"]
LOGIT_BAR = 2e-2        # tests/test_gpu_chat.py
REF_BAR = 1e-2          # tests/test_gpu_chat.py
PEN = 1.2


@pytest.fixture(scope="module")
def tiny():
    """tests/test_gpu_chat.py::tiny and ::ref in one: the encoder sized so that three reference prompts pack into one call"""
    from PIL import Image
    cfg = tiny_config()
    F = np.load(FIX)
    dmb = float(F["dim_model_base"])
    enc = HipEncoder(cfg, device=0, max_images=4, max_tokens=2304, max_seqs=4)
    enc.load_state_dict(iter_synth_weights(cfg, 0, device="cuda"))
    W = synth_state_dict(cfg, 0)
    head = synth_lm_head(cfg, 0)
    chat = HipChat(enc, max_len=720, max_rows=9, dim_model_base=dmb, max_slots=3, max_new=32)
    chat.load_head(head.cuda())
    tok = Words(cfg.vocab_size)
    root = os.path.join(HERE, "golden", "inputs")
    items = []
    for p, name in enumerate(["cat.jpeg", "dog.jpg"]):
        img = Image.open(os.path.join(root, name)).convert("RGB")
        items.append(_prompt_item(*chat_prompt([{"role": "user", "content": QUESTIONS[p]}], img, tok, cfg), tok, 2048))
    items.append(_prompt_item("<用户>" + QUESTIONS[2], [], tok, 2048))
    for p, it in enumerate(items):
        assert it.input_ids == F[f"p{p}_ids"].tolist()
    return types_ns(cfg=cfg, enc=enc, W=W, head=head, chat=chat, F=F, items=items, tok=tok, dmb=dmb)


def types_ns(**kw):
    import types
    return types.SimpleNamespace(**kw)


def _text_item(cfg, text):
    return prepare_item(text, None, StandInTokenizer(cfg.vocab_size), cfg, 2048)


def _page_item(cfg, seed=0):
    from PIL import Image
    page = synth_pages(1, size=cfg.scale_resolution, seed=seed)[0]
    return prepare_item("<用户>what is shown here", Image.fromarray(page), StandInTokenizer(cfg.vocab_size), cfg, 2048)


def _log_softmax64(logits):
    l = np.asarray(logits, dtype=np.float64)
    return l - (l.max() + np.log(np.exp(l - l.max()).sum()))


def _decode_path(chat, item, cont):
    """prefill + teacher-forced steps along `cont` -> per position (fp64 log-prob of the token, max |logit| of its row, argmax)"""
    chat.prefill(0, 0, item)
    out = []
    for t, tok in enumerate(cont):
        l = chat.logits(0)
        out.append((float(_log_softmax64(l)[tok]), float(np.abs(l).max()), int(np.argmax(l))))
        if t + 1 < len(cont):
            chat.step([0], [0], [int(tok)])
    return out


# ---- 1. the fp32 CPU oracle --------------------------------------------------------------------------------------------------
def test_token_logprobs_against_the_fp32_oracle(tiny):
    t = tiny
    rng = np.random.default_rng(3)
    for item in (_page_item(t.cfg), _text_item(t.cfg, "<用户>a short question about the page")):
        cont = rng.integers(16, t.cfg.vocab_size, 6).tolist()
        ids = list(item.input_ids) + cont
        taps = {}
        O.encode(t.W, t.cfg, [ids], [item.image_bound], [item.slices], taps=taps)
        hid = taps["last_hidden"][0]
        got = score_items(t.chat, [item], [cont])[0]
        worst = 0.0
        for j, tok in enumerate(cont):
            pos = len(item.input_ids) + j                   # the token's position: its row is the hidden state of pos - 1
            logits = (hid[pos - 1] / (t.cfg.hidden_size / t.dmb) @ t.head.T).numpy()
            ref = _log_softmax64(logits)
            bar = 2 * LOGIT_BAR * float(np.abs(logits).max())
            err = abs(got["token_logprobs"][j] - ref[tok])
            worst = max(worst, err / bar)
            assert err <= bar, (j, err, bar)
            if np.sort(logits)[-1] - np.sort(logits)[-2] > 2 * LOGIT_BAR * float(np.abs(logits).max()):
                assert got["top_tokens"][j] == int(np.argmax(logits))
        print("oracle: worst token log-prob error / bar", worst)


# ---- 2. the reference model ---------------------------------------------------------------------------------------------------
def test_reference_beam_logprobs_and_scores(tiny):
    t = tiny
    F = t.F
    n = int(F["n_prompts"])
    conts = [F[f"p{p}_beam_tokens"].tolist() for p in range(n)]
    res = score_items(t.chat, t.items, conts, repetition_penalty=float(F["pen_beam"]))      # one packed call of three sequences
    worst = 0.0
    for p in range(n):
        pre, ln = F[f"p{p}_beam_q_prefix"], F[f"p{p}_beam_q_len"]
        table = {tuple(pre[i, :ln[i]].tolist()): (F[f"p{p}_beam_q_ids"][i], F[f"p{p}_beam_q_logprobs"][i]) for i in range(len(ln))}
        assert len(conts[p]) == 20
        bars = 2 * REF_BAR * F[f"p{p}_beam_absmax"].astype(np.float64)
        for s, tok in enumerate(conts[p]):
            ids, lp = table[tuple(conts[p][:s])]
            (j,) = np.nonzero(ids == tok)[0]
            err = abs(res[p]["token_logprobs"][s] - float(lp[j]))
            worst = max(worst, err / bars[s])
            assert err <= bars[s], (p, s, err, bars[s])
        got = sequence_score(res[p]["token_logprobs"], conts[p], float(F["pen_beam"]))
        assert got == res[p]["score"]
        assert abs(got - float(F[f"p{p}_beam_score"])) <= float(F["pen_beam"]) * bars.mean(), p
    print("reference: worst token log-prob error / bar", worst)


# ---- 3. the device's own decode path ------------------------------------------------------------------------------------------
def test_decode_path_and_beam_hypotheses(tiny):
    t = tiny
    item = _page_item(t.cfg, seed=2)
    cont = np.random.default_rng(5).integers(16, t.cfg.vocab_size, 12).tolist()
    cont[7] = cont[2]                                       # a repeated token
    path = _decode_path(t.chat, item, cont)
    got = score_items(t.chat, [item], [cont], repetition_penalty=PEN)[0]
    for j, (lp, absmax, top) in enumerate(path):
        assert abs(got["token_logprobs"][j] - lp) <= 2 * LOGIT_BAR * absmax, j
    assert abs(got["score"] - sequence_score([p[0] for p in path], cont, PEN)) <= PEN * 2 * LOGIT_BAR * np.mean([p[1] for p in path])
    # every hypothesis the beam search returns: its score is the sequence score of its tokens
    for it in (item, _text_item(t.cfg, "<用户>a short question about the page")):
        det = generate_items(t.chat, [it], max_new_tokens=8, num_beams=3, repetition_penalty=PEN, details=True,
                             num_return_sequences=3)[0]
        assert 1 <= len(det["hyps"]) <= 3
        raw = t.chat.score([PreparedItem(input_ids=list(it.input_ids) + toks, image_bound=it.image_bound, slices=it.slices)
                            for _, toks in det["hyps"]], [len(toks) for _, toks in det["hyps"]])
        res = score_items(t.chat, [it] * len(det["hyps"]), [toks for _, toks in det["hyps"]], repetition_penalty=PEN)
        for (score, toks), r, rw in zip(det["hyps"], res, raw):
            bar = PEN * 2 * LOGIT_BAR * float(np.abs(rw["top_logit"]).mean())
            print("hypothesis", toks, "beam score", score, "scored", r["score"], "bar", bar)
            assert abs(r["score"] - score) <= bar


# ---- 4. packing ---------------------------------------------------------------------------------------------------------------
def test_packing_and_the_one_token_case(tiny):
    t = tiny
    a = _text_item(t.cfg, "<用户>first prompt with several words in it")
    b = _page_item(t.cfg, seed=3)
    c = _text_item(t.cfg, "<用户>second")
    rng = np.random.default_rng(9)
    conts = [rng.integers(16, t.cfg.vocab_size, n).tolist() for n in (5, 9, 1)]
    alone = score_items(t.chat, [b], [conts[1]])[0]
    packed = score_items(t.chat, [a, b, c], conts)
    raw = t.chat.score([PreparedItem(input_ids=list(b.input_ids) + conts[1], image_bound=b.image_bound, slices=b.slices)], [9])[0]
    bars = 2 * LOGIT_BAR * np.abs(raw["top_logit"]).astype(np.float64)
    assert (np.abs(alone["token_logprobs"] - packed[1]["token_logprobs"]) <= bars).all()
    assert [len(r["token_logprobs"]) for r in packed] == [5, 9, 1]
    # cont_len == 1: the log-softmax of the prompt's prefill logits
    for it, cont in ((c, conts[2]), (b, conts[1][:1])):
        t.chat.prefill(0, 0, it)
        l = t.chat.logits(0)
        one = score_items(t.chat, [it], [cont])[0]
        assert abs(one["token_logprobs"][0] - _log_softmax64(l)[cont[0]]) <= 2 * LOGIT_BAR * float(np.abs(l).max())
        if np.sort(l)[-1] - np.sort(l)[-2] > 2 * LOGIT_BAR * float(np.abs(l).max()):
            assert one["top_tokens"][0] == int(np.argmax(l))


# ---- 5. statelessness ---------------------------------------------------------------------------------------------------------
class _Beam:
    """One item's beam search by hand (prefill / select / reorder / step); `between` runs before every select."""

    def __init__(self, chat, item, between=None):
        self.chat, self.between = chat, between
        chat.prefill(0, 0, item)

    def select(self, n, scores, k):
        if self.between:
            self.between(n)
        sc, tk, pa = self.chat.select(BEAM, [list(range(n))], k, scores, repetition_penalty=PEN)
        return [(float(sc[0, j]), int(tk[0, j]), int(pa[0, j])) for j in range(k) if tk[0, j] >= 0]

    def advance(self, parents, tokens):
        dst = list(range(len(parents)))
        if list(parents) != dst:
            self.chat.reorder(dst, list(parents))
        self.chat.step([0] * len(dst), dst, list(tokens))


def test_scoring_leaves_a_generation_in_progress_alone(tiny):
    t = tiny
    item = _page_item(t.cfg, seed=4)
    other = [_text_item(t.cfg, "<用户>a bystander of the scoring call"), _page_item(t.cfg, seed=6)]
    conts = [[40, 41, 42], [50, 51, 52, 53, 54]]
    checked = []

    def between(n):
        before = [(t.chat.logits(r), t.chat.row_state(r)) for r in range(n)]
        res = score_items(t.chat, other, conts)
        assert all(np.isfinite(r["token_logprobs"]).all() for r in res)
        for r, (l, st) in enumerate(before):
            assert t.chat.row_state(r) == st and t.chat.logits(r).tobytes() == l.tobytes(), r
        checked.append(n)

    plain = run_rule(beam_rule(3, 8), _Beam(t.chat, item))
    disturbed = run_rule(beam_rule(3, 8), _Beam(t.chat, item, between))
    assert len(checked) >= 2 and max(checked) == 3
    assert disturbed["tokens"] == plain["tokens"] and disturbed["score"] == plain["score"]
    assert [s[1] for s in disturbed["steps"]] == [s[1] for s in plain["steps"]]


def test_encode_unchanged_by_scoring(tiny):
    t = tiny
    items = [_page_item(t.cfg, seed=7), _text_item(t.cfg, "a query")]
    before = [t.enc.encode_items([it]).cpu().numpy() for it in items]
    score_items(t.chat, items, [[17, 18], [19]])
    after = [t.enc.encode_items([it]).cpu().numpy() for it in items]
    for x, y in zip(before, after):
        assert np.array_equal(x, y)


# ---- 6. errors through the raw ABI --------------------------------------------------------------------------------------------
def _raw_score(chat, seqs, cont_lens, size=None):
    """vr_chat_score on token-only sequences with sentinel-filled outputs -> (status, outputs)"""
    ids = np.ascontiguousarray(np.concatenate([np.asarray(s, dtype=np.int32) for s in seqs]))
    off = np.zeros(len(seqs) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(s) for s in seqs])
    cl = np.asarray(cont_lens, dtype=np.int32)
    n = size or max(int(np.abs(cl).sum()), 1) + 4
    outs = [np.full(n, -7.5, dtype=np.float32) for _ in range(3)] + [np.full(n, -9, dtype=np.int32)]
    p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    pf = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    rc = chat.lib.vr_chat_score(chat._h, len(seqs), None, None, 0, 0, p32(ids), p32(off), None, p32(cl), pf(outs[0]), pf(outs[1]),
                                pf(outs[2]), p32(outs[3]), chat._stream())
    return rc, outs


def _untouched(outs):
    return all((o == np.float32(-7.5)).all() for o in outs[:3]) and (outs[3] == -9).all()


def test_argument_errors_leave_the_outputs(tiny):
    t = tiny
    V = t.cfg.vocab_size
    seq = [1] + list(range(20, 30))
    INVALID, STATE, CAPACITY = 1, 3, 4
    for seqs, cl, want in (([seq], [0], INVALID), ([seq], [len(seq)], INVALID), ([seq, seq], [2, -1], INVALID),
                           ([seq[:-1] + [V]], [3], INVALID), ([seq[:3] + [V] + seq[4:]], [2], INVALID),
                           ([seq] * 5, [1] * 5, CAPACITY),                                 # max_seqs = 4
                           ([[1] + [20] * 799] * 3, [4, 4, 4], CAPACITY)):                 # 2400 tokens > max_tokens = 2304
        rc, outs = _raw_score(t.chat, seqs, cl)
        assert rc == want and _untouched(outs), (cl, rc)
    bare = HipChat(t.enc, max_len=64, max_rows=1, dim_model_base=t.dmb)
    rc, outs = _raw_score(bare, [seq], [2])
    bare.close()
    assert rc == STATE and _untouched(outs)
    # NULL outputs, and a good call for contrast: exactly sum(cont_len) entries are written
    p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    ids, off, cl = np.asarray(seq, np.int32), np.asarray([0, len(seq)], np.int32), np.asarray([2], np.int32)
    assert t.chat.lib.vr_chat_score(t.chat._h, 1, None, None, 0, 0, p32(ids), p32(off), None, p32(cl), None, None, None, None,
                                    t.chat._stream()) == INVALID
    rc, outs = _raw_score(t.chat, [seq, seq], [2, 3])
    assert rc == 0
    for o in outs[:3]:
        assert np.isfinite(o[:5]).all() and (o[:5] != np.float32(-7.5)).all() and (o[5:] == np.float32(-7.5)).all()
    assert ((outs[3][:5] >= 0) & (outs[3][:5] < V)).all() and (outs[3][5:] == -9).all()
    assert (outs[2][:5] >= outs[0][:5]).all() and (outs[1][:5] >= outs[2][:5]).all()      # x_t <= top_x <= lse
    bar = 2 * LOGIT_BAR * float(np.abs(outs[2][:5]).max())                                # the same sequence twice: the same rows
    assert abs(outs[0][0] - outs[0][3]) <= bar and abs(outs[1][1] - outs[1][4]) <= bar and outs[3][0] == outs[3][3]


# ---- 7. the public surface ----------------------------------------------------------------------------------------------------
class _RoundTrip(Words):
    """Words whose encode reads its own decode back: "w<id>" is token <id>"""

    def _word_id(self, w):
        return int(w[1:]) if re.fullmatch(r"w\d+", w) else super()._word_id(w)


@pytest.fixture(scope="module")
def public(tiny):
    t = tiny
    F = np.load(WFIX)
    tok = _RoundTrip(t.cfg.vocab_size)
    model = DRModelForInference(t.cfg, t.enc).lm_q.attach_generator(t.head.cuda(), GenerationConfig(dim_model_base=float(F["dim_model_base"])),
                                                                    max_inp_length=720, max_new_tokens=8, num_beams=3, batch=3)
    return model, F, tok, question_pages(F, t.cfg, 0)


def test_score_answers_and_choose(tiny, public):
    model, F, tok, pages = public
    msgs = msgs_of(F, 0)
    out = model.score_answers(pages[:2], [msgs, msgs], [["w100 w200", "w300"], ["w100 w200 w400"]], tok)
    assert [len(o) for o in out] == [2, 1]
    assert [len(r["token_logprobs"]) for o in out for r in o] == [3, 2, 4]                 # the eos counts
    no_eos = model.score_answers(pages[:1], [msgs], [["w100 w200"]], tok, append_eos=False)[0][0]
    assert len(no_eos["token_logprobs"]) == 2
    raw_bar = 2 * LOGIT_BAR * 2 * float(F["q0_absmax"])       # two packings of the same rows: each within the bar of the truth
    assert (np.abs(no_eos["token_logprobs"] - out[0][0]["token_logprobs"][:2]) <= raw_bar).all()
    for r in (r for o in out for r in o):
        assert set(r) == {"token_logprobs", "sum", "score", "greedy_match", "top_tokens"}
        assert (r["token_logprobs"] <= 0).all() and abs(r["sum"] - r["token_logprobs"].sum()) < 1e-9
    # the model's own greedy output against two copies whose last token is another: the prefix log-probs are shared
    p, sl = chat_prompt(msgs, pages[0], tok, tiny.cfg)
    item = _prompt_item(p + "<AI>", sl, tok, 2048)
    greedy = generate_items(model._chat, [item], max_new_tokens=6, num_beams=1, repetition_penalty=1.0)[0]
    body = [g for g in greedy if g != tok.eos_id]
    assert len(body) >= 2
    text = lambda ids: " ".join(f"w{i}" for i in ids)  # noqa: E731
    wrong = [body[:-1] + [16 + (body[-1] + d) % (tiny.cfg.vocab_size - 16)] for d in (301, 602)]
    options = [text(wrong[0]), text(body), text(wrong[1])]
    index, scores = model.choose(pages[0], msgs, options, tok, append_eos=False)
    assert index == 1 and len(scores) == 3
    assert scores[1]["greedy_match"][-1] and not scores[0]["greedy_match"][-1]
    assert model.choose(pages[0], msgs, options, tok, normalise=False, append_eos=False)[0] == 1


def test_marginal_selection(tiny, public):
    model, F, tok, pages = public
    msgs, doc = msgs_of(F, 0), F["q0_doc_scores"].tolist()
    n_new = int(F["max_new"])
    answer, d = model.marginal_selection(pages, msgs, doc, tok, details=True, max_new_tokens=n_new)
    ws_answer, ws = d["weighted_selection"]
    k = len(pages)
    S = np.asarray(d["S"])
    assert S.shape == (len(d["candidates"]), k) and 1 <= len(d["candidates"]) <= k
    assert answer == d["answers"][d["index"]] and d["weights"][d["index"]] == max(d["weights"])
    bar = PEN * 2 * LOGIT_BAR * float(F["q0_absmax"])
    for i in range(k):
        a = d["candidates"].index(list(ws["tokens"][i]))
        beam = ws["results"][i]["score"]
        print("page", i, "candidate", a, "beam score", beam, "scored", S[a, i], "bar", bar)
        assert abs(S[a, i] - beam) <= bar, i
        assert d["weights"][a] >= ws["weights"][i], i
    np.testing.assert_allclose(d["doc_probs"], ws["doc_probs"], rtol=1e-12)
    for a in range(len(d["candidates"])):
        assert abs(d["weights"][a] - float(np.sum(np.asarray(d["doc_probs"]) * np.exp(S[a])))) < 1e-12
    assert model.marginal_selection(pages, msgs, doc, tok, max_new_tokens=n_new) == answer
    # the same image twice: one candidate, weight exp(S) averaged over the two (equal) pages
    _, d2 = model.marginal_selection([pages[0], pages[0]], msgs, [0.2, 0.2], tok, details=True, max_new_tokens=n_new)
    assert len(d2["candidates"]) == 1 and np.asarray(d2["S"]).shape == (1, 2)
