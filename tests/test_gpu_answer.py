"""From top-k pages to one answer on the device: the batched prefill (vr_chat_prefill_batch, its K / V scatter at op level),
generate_items(prefill="batched"), VisRAGRet.weighted_selection / chat(assistant_turn, return_scores) and
visrag_amd/answer.py, against the fp32 oracle and the reference run of tests/golden/weighted_tiny.npz."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.answer_util import FIX, REF_BAR, Words, msgs_of, question_pages, running_sets  # noqa: E402
from tests.gpu_util import P  # noqa: E402
from oracle import visrag_ret_oracle as O  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.answer import answer_page_concatenation, answer_weighted_selection, concat_pages  # noqa: E402
from visrag_amd.config import tiny_config  # noqa: E402
from visrag_amd.engine import HipEncoder  # noqa: E402
from visrag_amd.generation import BEAM, GenerationConfig, HipChat, beam_rule, decode_text, generate_items, run_rule  # noqa: E402
from visrag_amd.modeling import DRModelForInference, _prompt_item, chat_prompt  # noqa: E402
from visrag_amd.preprocess import PreparedItem, prepare_item  # noqa: E402
from visrag_amd.synth import iter_synth_weights, synth_lm_head, synth_pages, synth_state_dict  # noqa: E402
from visrag_amd.tokenizer import StandInTokenizer  # noqa: E402

DMB = 64.0
LOGIT_BAR = 2e-2        # bf16 route vs the fp32 oracle, relative to max |logit|: the bar tests/test_gpu_chat.py holds this route to


# ---- the scatter kernel at op level --------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [64, 192])
def test_prompt_scatter_op(E):
    lens, slots, n_slots, max_len = [1, 5, 70], [2, 0, 1], 4, 72
    ld, T = 3 * E + 8, sum(lens)
    g = torch.Generator().manual_seed(E)
    qkv = torch.randn((T, ld), generator=g).to(torch.bfloat16).cuda()
    sentinel = torch.tensor(-7.25, dtype=torch.bfloat16)
    kp = torch.full((n_slots, max_len, E), float(sentinel), dtype=torch.bfloat16, device="cuda")
    vp = torch.full((n_slots, max_len, E), float(sentinel), dtype=torch.bfloat16, device="cuda")
    off = np.cumsum([0] + lens).astype(np.int32)
    p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
    _lib.check(_lib.load().vr_op_chat_prompt_scatter(0, P(qkv), ld, E, len(lens), p32(off), p32(np.asarray(slots, dtype=np.int32)), n_slots,
                                                     max_len, P(kp), P(vp), None), "vr_op_chat_prompt_scatter")
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int16).cpu()
    for b, (n, sl) in enumerate(zip(lens, slots)):
        src = qkv[off[b]:off[b] + n]
        assert torch.equal(bits(kp[sl, :n]), bits(src[:, E:2 * E].contiguous())), (b, "K")
        assert torch.equal(bits(vp[sl, :n]), bits(src[:, 2 * E:3 * E].contiguous())), (b, "V")
        assert (kp[sl, n:] == sentinel).all() and (vp[sl, n:] == sentinel).all(), b        # rows past the prompt's length
    assert (kp[3] == sentinel).all() and (vp[3] == sentinel).all()                           # the unused slot
    # the entry's own checks: a repeated slot, a prompt longer than the plane
    bad = np.asarray([2, 2, 1], dtype=np.int32)
    assert _lib.load().vr_op_chat_prompt_scatter(0, P(qkv), ld, E, 3, p32(off), p32(bad), n_slots, max_len, P(kp), P(vp), None) != 0
    assert _lib.load().vr_op_chat_prompt_scatter(0, P(qkv), ld, E, 3, p32(off), p32(np.asarray(slots, dtype=np.int32)), n_slots, 69,
                                                 P(kp), P(vp), None) != 0


# ---- the library ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    cfg = tiny_config()
    enc = HipEncoder(cfg, device=0, max_images=4, max_tokens=512, max_seqs=8)
    enc.load_state_dict(iter_synth_weights(cfg, 0, device="cuda"))
    W = synth_state_dict(cfg, 0)
    head = synth_lm_head(cfg, 0)
    chat = HipChat(enc, max_len=256, max_rows=9, dim_model_base=DMB, max_slots=4, max_new=16)
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


def test_prefill_batch_logits_cache_and_bystander(tiny):
    """A page prompt, a text prompt and a one-token prompt in one pass, into permuted slots and non-adjacent rows; a row
    prefilled before on a fourth slot is a bystander.  Teacher-forced steps of all four rows in one call read every
    prompt's K / V back: a row in the wrong slot or at the wrong position would leave the bar."""
    cfg, enc, W, head, chat = tiny
    items = [_page_item(cfg), _text_item(cfg, "<用户>a short question about the page"), PreparedItem(input_ids=[1], image_bound=[], slices=[])]
    by = _text_item(cfg, "<用户>the bystander was here first")
    slots, rows = [2, 0, 1], [4, 0, 7]
    chat.prefill(3, 2, by)
    by_logits = chat.logits(2)
    chat.prefill_batch(slots, rows, items)
    assert np.array_equal(chat.logits(2), by_logits)
    assert [chat.row_state(r) for r in rows + [2]] == [(2, 0), (0, 0), (1, 0), (3, 0)]
    every = list(zip(items + [by], slots + [3], rows + [2]))
    every.sort(key=lambda x: x[1])
    refs = {r: _oracle_logits(cfg, W, head, it) for it, _, r in every}
    for it, _, r in every:
        e = _rel(chat.logits(r), refs[r])
        print("prefill_batch row", r, "tokens", len(it.input_ids), "rel err", e)
        assert e < LOGIT_BAR, r
    extra = {r: [] for _, _, r in every}
    for t in range(4):
        toks = [int(np.argmax(refs[r])) for _, _, r in every]
        for (_, _, r), tok in zip(every, toks):
            extra[r].append(tok)
        chat.step([s for _, s, _ in every], [r for _, _, r in every], toks)
        for it, _, r in every:
            refs[r] = _oracle_logits(cfg, W, head, it, extra[r])
            e = _rel(chat.logits(r), refs[r])
            print("step", t, "row", r, "rel err", e)
            assert e < LOGIT_BAR, (t, r)


def test_prefill_batch_failures_leave_state(tiny):
    cfg, enc, W, head, chat = tiny
    first = _text_item(cfg, "<用户>the earlier prompt")
    short = _text_item(cfg, "<用户>short")

    def start():
        chat.prefill(0, 0, first)
        chat.step([0], [0], [5])

    start()
    chat.step([0], [0], [9])
    twin = chat.logits(0)
    start()
    before = chat.row_state(0), chat.logits(0)
    long_ = PreparedItem(input_ids=[1] + [20] * 199, image_bound=[], slices=[])
    with pytest.raises(_lib.VisragHipError, match="status 4"):
        chat.prefill_batch([1, 2, 3], [3, 4, 5], [long_, long_, long_])               # 600 tokens > max_tokens = 512
    with pytest.raises(_lib.VisragHipError):
        chat.prefill_batch([1, 1], [3, 4], [short, short])                            # a repeated slot
    with pytest.raises(_lib.VisragHipError):
        chat.prefill_batch([1, 2], [3, 3], [short, short])                            # a repeated row
    with pytest.raises(_lib.VisragHipError, match="status 4"):
        chat.prefill_batch([0, 1], [0, 3], [short, PreparedItem(input_ids=[1] + [20] * 255, image_bound=[], slices=[])])   # max_len tokens
    assert chat.row_state(0) == before[0] and np.array_equal(chat.logits(0), before[1])
    assert chat.row_state(3) == (-1, 0)
    chat.step([0], [0], [9])
    assert np.array_equal(chat.logits(0), twin)


# ---- the reference run (tools/gen_golden_weighted.py) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref():
    cfg = tiny_config()
    F = np.load(FIX)
    enc = HipEncoder(cfg, device=0, max_images=4, max_tokens=1024, max_seqs=2)
    enc.load_state_dict(iter_synth_weights(cfg, 0, device="cuda"))
    head = synth_lm_head(cfg, 0)
    tok = Words(cfg.vocab_size)
    model = DRModelForInference(cfg, enc).lm_q.attach_generator(head.cuda(), GenerationConfig(dim_model_base=float(F["dim_model_base"])),
                                                                max_inp_length=720, max_new_tokens=8, num_beams=3, batch=3)
    k = int(F["k"])
    pages = {q: question_pages(F, cfg, q) for q in range(int(F["n_questions"]))}
    items = {}
    for q, imgs in pages.items():
        for i, img in enumerate(imgs):
            prompt, sl = chat_prompt(msgs_of(F, q), img, tok, cfg)
            items[q * k + i] = _prompt_item(prompt + "<AI>", sl, tok, 2048)
            assert items[q * k + i].input_ids == F[f"p{q * k + i}_ids"].tolist()
    return cfg, enc, model, F, tok, pages, items


def _sets(res):
    steps = res["steps"]
    return running_sets([[t for _, t, _ in st[1]] for st in steps], [[p for _, _, p in st[1]] for st in steps])


def _compare_to_reference(F, P, res):
    """Step by step until the runs part, as test_reference_greedy_and_beam_tokens does: a step the runs share whose reference
    margin exceeds 4 x REF_BAR x max|logit| decides alike; a parting step is a narrow one.  -> the runs never parted."""
    want, got = running_sets(F[f"p{P}_beam_next_tokens"], F[f"p{P}_beam_next_parents"]), _sets(res)
    for s, (m, a) in enumerate(zip(F[f"p{P}_beam_set_margin"], F[f"p{P}_beam_absmax"])):
        if s >= len(got) or got[s] != want[s]:
            assert not m > 4 * REF_BAR * a, (P, s, got, want)
            return False
    return True


def test_generate_items_batched_prefill_over_a_split_chunk(ref):
    """Chunks of three prompts against max_seqs = 2: every chunk's prefill splits.  "batched" equals "single" wherever the
    recorded margins decide; where the two part, the reference's margin of that step is narrow."""
    cfg, enc, model, F, tok, pages, items = ref
    chat = model._chat
    assert chat.max_rows // 3 > enc.max_seqs
    order = sorted(items)
    kw = dict(max_new_tokens=int(F["max_new"]), num_beams=3, repetition_penalty=float(F["pen_beam"]), details=True)
    single = generate_items(chat, [items[P] for P in order], **kw)
    batched = generate_items(chat, [items[P] for P in order], prefill="batched", **kw)
    n_equal = 0
    for P, a, b in zip(order, single, batched):
        sa, sb = _sets(a), _sets(b)
        on_path = _compare_to_reference(F, P, a)
        want = running_sets(F[f"p{P}_beam_next_tokens"], F[f"p{P}_beam_next_parents"])
        for s, (m, am) in enumerate(zip(F[f"p{P}_beam_set_margin"], F[f"p{P}_beam_absmax"])):
            if s >= len(sa) or sa[s] != want[s]:
                break                                   # "single" left the recorded path (at a narrow step): no margins beyond
            if s >= len(sb) or sb[s] != sa[s]:
                assert not m > 4 * REF_BAR * am, (P, s)
                break
        if bool(F[f"p{P}_decisive"]):
            assert on_path and a["tokens"] == b["tokens"] == F[f"p{P}_beam_tokens"].tolist(), P
        n_equal += a["tokens"] == b["tokens"]
    print("batched == single on", n_equal, "of", len(order), "prompts")


def test_weighted_selection_against_the_reference(ref):
    cfg, enc, model, F, tok, pages, items = ref
    k, n_new = int(F["k"]), int(F["max_new"])
    for q in range(int(F["n_questions"])):
        ds = F[f"q{q}_doc_scores"].tolist()
        answer, d = answer_weighted_selection(model, tok, msgs_of(F, q), pages[q], ds, max_new_tokens=n_new, details=True,
                                              prefill="batched")
        assert answer == d["answers"][d["index"]] and len(d["answers"]) == k
        bar = REF_BAR * float(F[f"q{q}_absmax"])
        same = [_compare_to_reference(F, q * k + i, d["results"][i]) for i in range(k)]
        for i in range(k):
            P = q * k + i
            if same[i] and d["tokens"][i] == F[f"p{P}_beam_tokens"].tolist():
                err = abs(d["scores"][i][0] - float(F[f"p{P}_beam_score"]))
                print("question", q, "page", i, "score error", err, "bar", bar)
                assert err < bar, (q, i)
        if bool(F[f"q{q}_decisive"]):
            assert all(same), q
            for i in range(k):
                assert d["tokens"][i] == F[f"p{q * k + i}_beam_tokens"].tolist(), (q, i)
                assert abs(d["scores"][i][1] - float(F[f"p{q * k + i}_beam_scores2"][1])) < bar, (q, i)
            assert d["index"] == int(F[f"q{q}_index"]), q
            assert answer == decode_text([F[f"p{q * k + int(F[f'q{q}_index'])}_beam_tokens"].tolist()], tok)[0]
            np.testing.assert_allclose(d["doc_probs"], F[f"q{q}_probs"], rtol=1e-6, atol=0)
            np.testing.assert_allclose(d["weights"], F[f"q{q}_weights"], rtol=0, atol=float(np.exp(bar) - 1) * max(F[f"q{q}_weights"]))
        if bool(F[f"q{q}_decisive"]):            # the default (one prefill per page) decides a decisive question alike
            assert answer_weighted_selection(model, tok, msgs_of(F, q), pages[q], ds, max_new_tokens=n_new) == answer


def test_chat_assistant_turn_and_scores(ref):
    cfg, enc, model, F, tok, pages, items = ref
    k, n_new = int(F["k"]), int(F["max_new"])
    decisive = [P for P in sorted(items) if bool(F[f"p{P}_decisive"])]
    assert len(decisive) >= 6
    for P in decisive[:3]:
        q, i = divmod(P, k)
        ans, scores = model.chat([pages[q][i]], [msgs_of(F, q)], tok, sampling=False, max_new_tokens=n_new, assistant_turn=True,
                                 return_scores=True)
        assert ans == decode_text([F[f"p{P}_beam_tokens"].tolist()], tok)
        bar = REF_BAR * float(F[f"p{P}_beam_absmax"].max())
        assert abs(scores[0][0] - float(F[f"p{P}_beam_score"])) < bar, P
        assert len(scores[0]) == 2 and abs(scores[0][1] - float(F[f"p{P}_beam_scores2"][1])) < bar, P
    with pytest.raises(NotImplementedError):
        model.chat([pages[1][0]], [msgs_of(F, 1)], tok, sampling=True, return_scores=True)


def test_page_concatenation_is_chat_on_the_concatenated_image(ref):
    cfg, enc, model, F, tok, pages, items = ref
    for kind in ("horizontal", "vertical"):
        got = answer_page_concatenation(model, tok, msgs_of(F, 1), pages[1], kind, max_new_tokens=4)
        img = concat_pages(pages[1], kind)
        want = model.chat([img], [msgs_of(F, 1)], tok, sampling=False, max_new_tokens=4, assistant_turn=True)[0]
        assert got == want and isinstance(got, str) and got
    plain = model.chat([concat_pages(pages[1], "horizontal")], [msgs_of(F, 1)], tok, sampling=False, max_new_tokens=4)[0]
    assert isinstance(plain, str)


class _DeviceBeam:
    """One item's beam search driven by hand through prefill / select / reorder / step: the path of generate_items' defaults."""

    def __init__(self, chat, item, pen):
        self.chat, self.pen = chat, pen
        chat.prefill(0, 0, item)

    def select(self, n, scores, k):
        sc, tk, pa = self.chat.select(BEAM, [list(range(n))], k, scores, repetition_penalty=self.pen)
        return [(float(sc[0, j]), int(tk[0, j]), int(pa[0, j])) for j in range(k) if tk[0, j] >= 0]

    def advance(self, parents, tokens):
        dst = list(range(len(parents)))
        if list(parents) != dst:
            self.chat.reorder(dst, list(parents))
        self.chat.step([0] * len(dst), dst, list(tokens))


def test_defaults_are_the_single_prefill_path(ref):
    """chat / generate / generate_items with their defaults: no "<AI>" turn, one prefill per item, the best hypothesis alone —
    the tokens of a beam search driven by hand over vr_chat_prefill."""
    from PIL import Image
    import os
    cfg, enc, model, F, tok, pages, items = ref
    chat = model._chat
    C_ = np.load(os.path.join(os.path.dirname(FIX), "chat_tiny.npz"))
    img = Image.open(os.path.join(os.path.dirname(FIX), "inputs", "cat.jpeg")).convert("RGB")
    question = "What animal is in the picture?"
    prompt, sl = chat_prompt([{"role": "user", "content": question}], img, tok, cfg)
    item = _prompt_item(prompt, sl, tok, 2048)
    assert item.input_ids == C_["p0_ids"].tolist()
    text = _prompt_item("<用户>What is the capital of France?", [], tok, 2048)
    assert text.input_ids == C_["p2_ids"].tolist()
    for it in (item, text):
        want = run_rule(beam_rule(3, 6), _DeviceBeam(chat, it, 1.2))
        got = generate_items(chat, [it], max_new_tokens=6, num_beams=3, repetition_penalty=1.2)
        assert got == [want["tokens"]]
        det = generate_items(chat, [it], max_new_tokens=6, num_beams=3, repetition_penalty=1.2, details=True)[0]
        assert det["tokens"] == want["tokens"] and det["score"] == want["score"] and len(det["hyps"]) == 1
    ans = model.chat([img], [[{"role": "user", "content": question}]], tok, sampling=False, max_new_tokens=6)
    assert ans == decode_text(generate_items(chat, [item], max_new_tokens=6, num_beams=3, repetition_penalty=1.2), tok)
    assert ans == model.generate(data_list=[prompt], img_list=[sl], tokenizer=tok, max_new_tokens=6, num_beams=3, repetition_penalty=1.2)
