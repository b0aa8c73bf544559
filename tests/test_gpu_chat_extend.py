"""Several given tokens appended to a cached prompt in one packed pass: vr_op_chat_extend_attention against the fp64
two-segment reference (tests/chat_extend_ref.py), vr_chat_extend / vr_chat_row_score / vr_chat_row_truncate through HipChat
against the fp32 CPU oracle and the device's other routes, and the public surface (score_answers / choose /
marginal_selection with shared_prefill=True, chat_session).

Bars.  Op level: the standing bar of the attention tests of tests/test_gpu_ops.py (rtol = atol = 2e-2) on bf16-rounded
inputs.  Model level: LOGIT_BAR = 2e-2 x the row's max |logit| against the fp32 oracle (tests/test_gpu_chat.py), twice that
between two device routes (each is within the bar of the truth); a token log-prob is 2-Lipschitz in the sup-norm of the
logits, so its bars are twice the logit's (2 x bar against the oracle, 4 x bar between two device routes); the sequence bar is
that of tests/test_gpu_answer_score.py."""
import ctypes as C
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import visrag_ret_oracle as O  # noqa: E402
from tests.answer_util import FIX as WFIX, Words, msgs_of, question_pages  # noqa: E402
from tests.chat_extend_ref import two_segment_attention, within_bar  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd.config import tiny_config  # noqa: E402
from visrag_amd.engine import HipEncoder  # noqa: E402
from visrag_amd.generation import (BEAM, GREEDY, GenerationConfig, HipChat, beam_rule, generate_items, run_rule,  # noqa: E402
                                   score_items, score_items_shared)
from visrag_amd.modeling import DRModelForInference, _prompt_item, chat_prompt  # noqa: E402
from visrag_amd.preprocess import PreparedItem, prepare_item  # noqa: E402
from visrag_amd.synth import iter_synth_weights, synth_lm_head, synth_pages, synth_state_dict  # noqa: E402
from visrag_amd.tokenizer import StandInTokenizer  # noqa: E402

LOGIT_BAR = 2e-2
PEN = 1.2
INVALID, STATE, CAPACITY = 1, 3, 4
DEV = "cuda:0"


def P(t):
    return C.c_void_p(t.data_ptr())


def _i32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


# =============================================================== op level ====================================================
class Arena:
    """The chat cache of the op: planes full of NaN, the rows a sequence may read filled by the caller; `out` sits between
    guard rows and carries guard columns."""

    def __init__(self, heads, seqs, L=2, l=1, slots=3, rows=4, slack_len=5, slack_new=3, seed=0):
        self.H, self.E, self.L, self.l, self.seqs = heads, heads * 64, L, l, seqs
        self.max_len = max(s["plen"] for s in seqs) + slack_len
        self.max_new = max(s["t0"] + s["n"] for s in seqs) + slack_new
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.prompt = torch.full((L, 2, slots, self.max_len, self.E), float("nan"), dtype=torch.bfloat16, device=DEV)
        self.tails = torch.full((L, 2, rows, self.max_new, self.E), float("nan"), dtype=torch.bfloat16, device=DEV)
        self.off = np.cumsum([0] + [s["n"] for s in seqs]).tolist()
        T = self.off[-1]
        self.q = torch.randn((T, self.E), generator=g, device=DEV).to(torch.bfloat16)
        for s in seqs:                                              # (a shared slot is filled once per sequence with the same seed)
            gs = torch.Generator(device=DEV).manual_seed(1000 + s["slot"])
            self.prompt[l, :, s["slot"], :s["plen"]] = torch.randn((2, s["plen"], self.E), generator=gs, device=DEV).to(torch.bfloat16)
            self.tails[l, :, s["row"], :s["t0"] + s["n"]] = torch.randn((2, s["t0"] + s["n"], self.E), generator=g, device=DEV).to(torch.bfloat16)
        self.ldo = self.E + 8
        self.buf = torch.full((T + 2, self.ldo), 7.0, dtype=torch.bfloat16, device=DEV)

    def run(self):
        lib = _lib.load()
        self.buf.fill_(7.0)
        out = self.buf[1:]
        s = self.seqs
        _lib.check(lib.vr_op_chat_extend_attention(0, P(self.q), self.E, P(self.prompt), P(self.tails), self.L, self.l, self.E, self.H,
                                                   self.prompt.shape[2], self.max_len, self.tails.shape[2], self.max_new, len(s),
                                                   _i32([x["row"] for x in s]), _i32([x["slot"] for x in s]), _i32([x["plen"] for x in s]),
                                                   _i32([x["t0"] for x in s]), _i32(self.off), P(out), self.ldo, None),
                   "vr_op_chat_extend_attention")
        torch.cuda.synchronize()
        got = self.buf.clone()
        T = self.off[-1]
        assert (got[0] == 7.0).all() and (got[T + 1] == 7.0).all() and (got[:, self.E:] == 7.0).all(), "guard words written"
        return got[1:T + 1, :self.E]

    def reference(self, b):
        s, H = self.seqs[b], self.H
        f = lambda t: t.float().cpu().numpy().astype(np.float64)  # noqa: E731
        q = f(self.q[self.off[b]:self.off[b + 1]]).reshape(s["n"], H, 64)
        pk, pv = (f(self.prompt[self.l, kv, s["slot"], :s["plen"]]).reshape(s["plen"], H, 64) for kv in (0, 1))
        m = s["t0"] + s["n"]
        tk, tv = (f(self.tails[self.l, kv, s["row"], :m]).reshape(m, H, 64) for kv in (0, 1))
        return two_segment_attention(q, pk, pv, tk, tv, s["t0"]).reshape(s["n"], H * 64)

    def check(self, what):
        got = self.run()
        assert torch.isfinite(got.float()).all(), what
        worst = 0.0
        for b in range(len(self.seqs)):
            ok, w = within_bar(got[self.off[b]:self.off[b + 1]].float().cpu().numpy(), self.reference(b))
            worst = max(worst, w)
            assert ok, (what, b, w)
        print(what, "worst error / bar", worst)
        return got


CASES = [(4, 1, 0, 1), (4, 63, 0, 15), (4, 64, 3, 16), (4, 65, 64, 17), (4, 257, 0, 63), (4, 700, 3, 64), (4, 1, 64, 65),
         (4, 64, 0, 130), (36, 65, 3, 1), (36, 257, 64, 16), (36, 63, 0, 65), (36, 700, 64, 130), (4, 1, 3, 130), (4, 700, 0, 17),
         (36, 1, 0, 64), (4, 65, 64, 63), (4, 257, 3, 15), (36, 64, 3, 17), (4, 63, 64, 64), (4, 64, 64, 1)]


@pytest.mark.parametrize("heads,plen,t0,n", CASES)
def test_op_against_the_fp64_reference(heads, plen, t0, n):
    a = Arena(heads, [dict(row=2, slot=1, plen=plen, t0=t0, n=n)], seed=plen + t0 + n)
    first = a.check(f"heads {heads} plen {plen} t0 {t0} n {n}:")
    assert torch.equal(first, a.run())


def test_op_three_sequences_two_on_one_slot():
    seqs = [dict(row=0, slot=2, plen=65, t0=3, n=17), dict(row=3, slot=0, plen=130, t0=0, n=70), dict(row=1, slot=2, plen=65, t0=0, n=1)]
    a = Arena(4, seqs, seed=5)
    a.check("three sequences:")


def test_op_dominant_keys_and_equal_scores():
    plen, t0, n = 70, 3, 20
    a = Arena(4, [dict(row=1, slot=0, plen=plen, t0=t0, n=n)], seed=9)
    g = torch.randn(a.E, generator=torch.Generator(device=DEV).manual_seed(3), device=DEV)
    a.q[:] = g.to(torch.bfloat16)                                 # every query row the same vector
    a.prompt[a.l, 0, 0, :plen] *= 0.05
    a.tails[a.l, 0, 1, :t0 + n] *= 0.05
    gh = a.q[0].float().view(4, 64)
    dom = (gh * (30 * 8 / (gh * gh).sum(-1, keepdim=True))).reshape(-1).to(torch.bfloat16)      # score 30 with every query
    a.prompt[a.l, 0, 0, 41] = dom
    got = a.check("a prompt key 30 above the rest:")
    v = a.prompt[a.l, 1, 0, 41].float()
    assert (got.float() - v).abs().max() <= 2e-2 + 2e-2 * v.abs().max()
    # a tail key like that one position AFTER query 7 must not move query 7 (or any earlier one): bit for bit
    a.prompt[a.l, 0, 0, 41] *= 0.001
    base = a.run()
    a.tails[a.l, 0, 1, t0 + 8] = dom
    a.tails[a.l, 1, 1, t0 + 8] = 100.0
    moved = a.check("a dominant tail key behind query 7:")
    assert torch.equal(moved[:8], base[:8]) and not torch.equal(moved[8:], base[8:])
    # all-equal scores: the plain mean of the visible values
    a.prompt[a.l, 0, 0, :plen] = 0
    a.tails[a.l, 0, 1, :t0 + n] = 0
    a.check("equal scores:")


def test_op_isolation():
    """NaN in every plane row no sequence may read (the Arena's fill), large finite values in a tail row that is in range but
    masked for every query except the last."""
    seqs = [dict(row=2, slot=1, plen=63, t0=3, n=66), dict(row=0, slot=1, plen=63, t0=0, n=5)]
    a = Arena(4, seqs, seed=11)
    assert torch.isnan(a.prompt[0]).all() and torch.isnan(a.prompt[a.l, :, 1, 63:]).all() and torch.isnan(a.tails[a.l, :, 2, 69:]).all()
    assert torch.isnan(a.prompt[a.l, :, 0]).all() and torch.isnan(a.tails[a.l, :, 1]).all() and torch.isnan(a.tails[a.l, :, 3]).all()
    sign = torch.where(torch.randn(a.E, device=DEV) > 0, 1.0, -1.0)
    a.tails[a.l, 0, 2, 68] = (1e4 * sign).to(torch.bfloat16)
    a.tails[a.l, 1, 2, 68] = 2e38
    first = a.check("isolation:")
    assert torch.equal(first, a.run())


def test_op_argument_checks():
    a = Arena(4, [dict(row=2, slot=1, plen=10, t0=2, n=3)])
    lib = _lib.load()

    def call(row=2, slot=1, plen=10, t0=2, off=(0, 3), B=1, heads=4, ldq=None, ldo=None, l=1):
        a.buf.fill_(7.0)
        rc = lib.vr_op_chat_extend_attention(0, P(a.q), ldq or a.E, P(a.prompt), P(a.tails), a.L, l, a.E, heads, 3, a.max_len, 4, a.max_new,
                                             B, _i32([row]), _i32([slot]), _i32([plen]), _i32([t0]), _i32(off), P(a.buf[1:]),
                                             ldo or a.ldo, None)
        torch.cuda.synchronize()
        assert rc == 0 or (a.buf == 7.0).all()
        return rc

    assert call() == 0
    for kw, want in ((dict(row=4), INVALID), (dict(slot=3), INVALID), (dict(plen=0), INVALID), (dict(plen=a.max_len + 1), CAPACITY),
                     (dict(t0=-1), INVALID), (dict(t0=a.max_new - 2), CAPACITY), (dict(off=(0, 0)), INVALID), (dict(off=(1, 4)), INVALID),
                     (dict(B=0), INVALID), (dict(B=17), CAPACITY), (dict(heads=5), INVALID), (dict(ldq=a.E + 4), INVALID),
                     (dict(ldo=a.E + 2), INVALID), (dict(l=2), INVALID)):
        assert call(**kw) == want, kw


# ============================================================== model level ==================================================
@pytest.fixture(scope="module")
def tiny():
    cfg = tiny_config()
    dmb = float(np.load(WFIX)["dim_model_base"])
    enc = HipEncoder(cfg, device=0, max_images=4, max_tokens=2304, max_seqs=4)
    enc.load_state_dict(iter_synth_weights(cfg, 0, device="cuda"))
    W = synth_state_dict(cfg, 0)
    head = synth_lm_head(cfg, 0)
    chat = HipChat(enc, max_len=720, max_rows=9, dim_model_base=dmb, max_slots=3, max_new=32)
    chat.load_head(head.cuda())
    from PIL import Image
    tokz = StandInTokenizer(cfg.vocab_size)
    page = prepare_item("<用户>what is shown here", Image.fromarray(synth_pages(1, size=cfg.scale_resolution, seed=0)[0]), tokz, cfg, 2048)
    text = prepare_item("<用户>a short question about the page", None, tokz, cfg, 2048)
    return SimpleNamespace(cfg=cfg, enc=enc, W=W, head=head, chat=chat, dmb=dmb, items=[page, text], cache={})


def _oracle(t, item, extra):
    """fp32 oracle logits [len(ids)][V] of item.input_ids + extra, cached per id list"""
    key = (id(item), tuple(extra))
    if key not in t.cache:
        taps = {}
        O.encode(t.W, t.cfg, [list(item.input_ids) + list(extra)], [item.image_bound], [item.slices], taps=taps)
        hid = taps["last_hidden"][0]
        t.cache[key] = (hid / (t.cfg.hidden_size / t.dmb) @ t.head.T).numpy()
    return t.cache[key]


def _close(got, ref, bars, what):
    """|got - ref| <= bars * LOGIT_BAR * max |ref|, printed"""
    bar = bars * LOGIT_BAR * float(np.abs(ref).max())
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)).max())
    print(what, "error / bar", err / bar)
    assert err <= bar, (what, err, bar)


def _plus(item, extra):
    return PreparedItem(input_ids=list(item.input_ids) + [int(x) for x in extra], image_bound=item.image_bound, slices=item.slices)


def _cont(seed, n, V):
    return np.random.default_rng(seed).integers(16, V, n).tolist()


@pytest.mark.parametrize("which", [0, 1])
def test_extend_against_the_oracle_a_full_prefill_and_step(tiny, which):
    t, item = tiny, tiny.items[which]
    c = _cont(3 + which, 7, t.cfg.vocab_size)
    t.chat.prefill(0, 0, item)
    assert t.chat.extend([0], [0], [c]) is None
    assert t.chat.row_state(0) == (0, 7)
    ext = t.chat.logits(0)
    _close(ext, _oracle(t, item, c)[-1], 1, "prefill + extend vs oracle:")
    t.chat.prefill(1, 1, _plus(item, c))
    _close(ext, t.chat.logits(1), 2, "prefill + extend vs prefill of the whole:")
    # n = 1 against a decode step with the same token
    t.chat.prefill(0, 0, item)
    t.chat.extend([0], [0], [c[:1]])
    one = t.chat.logits(0)
    t.chat.prefill(0, 0, item)
    t.chat.step([0], [0], c[:1])
    _close(one, t.chat.logits(0), 2, "extend of one token vs step:")
    _close(one, _oracle(t, item, c[:1])[-1], 1, "extend of one token vs oracle:")


@pytest.mark.parametrize("which", [0, 1])
def test_interleavings_of_extend_and_step(tiny, which):
    t, item = tiny, tiny.items[which]
    c = _cont(11 + which, 9, t.cfg.vocab_size)
    # extend 5 -> step 3
    t.chat.prefill(0, 0, item)
    t.chat.extend([0], [0], [c[:5]])
    for j in range(5, 8):
        t.chat.step([0], [0], [c[j]])
        _close(t.chat.logits(0), _oracle(t, item, c[:j + 1])[-1], 1, f"extend 5 -> step {j - 4}:")
    # step 3 -> extend 5 -> step 1
    t.chat.prefill(0, 0, item)
    for j in range(3):
        t.chat.step([0], [0], [c[j]])
    t.chat.extend([0], [0], [c[3:8]])
    assert t.chat.row_state(0) == (0, 8)
    _close(t.chat.logits(0), _oracle(t, item, c[:8])[-1], 1, "step 3 -> extend 5:")
    t.chat.step([0], [0], [c[8]])
    _close(t.chat.logits(0), _oracle(t, item, c)[-1], 1, "step 3 -> extend 5 -> step 1:")


def _log_softmax64(logits):
    l = np.asarray(logits, dtype=np.float64)
    return l - (l.max() + np.log(np.exp(l - l.max()).sum()))


@pytest.mark.parametrize("which", [0, 1])
def test_target_logprobs(tiny, which):
    t, item = tiny, tiny.items[which]
    c = _cont(21 + which, 6, t.cfg.vocab_size)
    ref = _oracle(t, item, c)
    plen = len(item.input_ids)
    t.chat.prefill(0, 0, item)
    first = t.chat.row_score([0], [c[0]])
    rest = t.chat.extend([0], [0], [c[:-1]], targets=[c[1:]])[0]
    f64 = lambda x: np.asarray(x, dtype=np.float64)  # noqa: E731
    lp = np.concatenate([f64(first["logit"]) - f64(first["lse"]), f64(rest["logit"]) - f64(rest["lse"])])
    top = np.concatenate([first["top_token"], rest["top_token"]])
    plain = score_items(t.chat, [item], [c])[0]
    worst = 0.0
    for j, tok in enumerate(c):
        row = ref[plen + j - 1]
        bar = LOGIT_BAR * float(np.abs(row).max())
        err = abs(lp[j] - _log_softmax64(row)[tok])
        worst = max(worst, err / (2 * bar))
        assert err <= 2 * bar, (j, err, bar)
        assert abs(lp[j] - plain["token_logprobs"][j]) <= 4 * bar, j
        srt = np.sort(row)
        if srt[-1] - srt[-2] > 2 * bar:
            assert top[j] == int(np.argmax(row)), j
    print("target log-probs vs oracle: worst error / (2 bar)", worst)
    # -1 targets leave their entries alone; the shared route returns what the two calls returned
    t.chat.prefill(0, 0, item)
    part = t.chat.extend([0], [0], [c[:-1]], targets=[[-1, c[2], -1, -1, c[5]]])[0]
    assert np.isnan(part["logit"][[0, 2, 3]]).all() and (part["top_token"][[0, 2, 3]] == -1).all()
    assert part["logit"][1] == rest["logit"][1] and part["lse"][4] == rest["lse"][4]
    shared = score_items_shared(t.chat, [item], [[c, c[:1]]])[0]
    tight = 4 * LOGIT_BAR * min(float(np.abs(ref[plen + j - 1]).max()) for j in range(len(c)))
    assert np.abs(shared[0]["token_logprobs"] - lp).max() <= tight and abs(shared[1]["token_logprobs"][0] - lp[0]) <= tight
    assert set(shared[0]) == set(plain) and len(shared[1]["token_logprobs"]) == 1


def test_three_rows_of_one_slot_in_one_call_and_the_prompt_planes(tiny):
    t, item = tiny, tiny.items[0]
    V = t.cfg.vocab_size
    conts = [_cont(31, 5, V), _cont(32, 17, V), _cont(33, 1, V)]
    for r in range(4):                                           # whatever earlier tests left on these rows: empty tails
        t.chat.truncate(r, 0)
    alone = []
    for c in conts:
        t.chat.prefill(1, 4, item)
        t.chat.extend([1], [0], [c])
        alone.append(t.chat.logits(0))
    t.chat.prefill(1, 4, item)
    t.chat.step([1], [3], [77])
    before = t.chat.logits(3)
    t.chat.truncate(3, 0)
    prompt_row = t.chat.logits(4)
    t.chat.extend([1, 1, 1], [0, 1, 2], conts)
    for r, (c, a) in enumerate(zip(conts, alone)):
        assert t.chat.row_state(r) == (1, len(c))
        _close(t.chat.logits(r), a, 2, f"row {r} of three vs alone:")
        _close(t.chat.logits(r), _oracle(t, item, c)[-1], 1, f"row {r} of three vs oracle:")
    assert t.chat.logits(4).tobytes() == prompt_row.tobytes() and t.chat.row_state(4) == (1, 0)     # the prompt's row is not named
    t.chat.step([1], [3], [77])
    assert t.chat.logits(3).tobytes() == before.tobytes(), "the prompt planes changed"


class _Beam:
    """tests/test_gpu_answer_score.py::_Beam"""

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


class _BeamOn(_Beam):
    """_Beam on a prompt that is already in slot 0 / row 0"""

    def __init__(self, chat):
        self.chat, self.between = chat, None


def test_extend_leaves_a_generation_in_progress_alone(tiny):
    t = tiny
    item, other = t.items[0], t.items[1]
    checked = []

    def between(n):
        before = [(t.chat.logits(r), t.chat.row_state(r)) for r in range(n)]
        t.chat.prefill(2, 8, other)
        res = t.chat.extend([2], [7], [[40, 41, 42, 43]], targets=[[41, 42, 43, 44]])
        assert np.isfinite(res[0]["logit"]).all()
        for r, (l, st) in enumerate(before):
            assert t.chat.row_state(r) == st and t.chat.logits(r).tobytes() == l.tobytes(), r
        checked.append(n)

    plain = run_rule(beam_rule(3, 8), _Beam(t.chat, item))
    disturbed = run_rule(beam_rule(3, 8), _Beam(t.chat, item, between))
    assert len(checked) >= 2 and max(checked) == 3
    assert disturbed["tokens"] == plain["tokens"] and disturbed["score"] == plain["score"]
    assert [s[1] for s in disturbed["steps"]] == [s[1] for s in plain["steps"]]


def test_slot_score_outlives_a_generation(tiny):
    t, item = tiny, tiny.items[0]
    for r in range(4):
        t.chat.truncate(r, 0)
    t.chat.prefill(0, 0, item)
    assert t.chat.slot_state(0) == (len(item.input_ids), True)
    want = t.chat.row_score([0, 0], [20, 500])
    run_rule(beam_rule(3, 6), _BeamOn(t.chat))                        # steps, reorders: row 0's logits move to another line
    got = t.chat.slot_score([0, 0], [20, 500])
    for k in want:
        assert want[k].tobytes() == got[k].tobytes(), k
    t.chat.truncate(0, 0)
    t.chat.extend([0], [1], [[30, 31]])                               # another row's line: the prompt's logits stay
    assert t.chat.slot_state(0)[1] and t.chat.slot_score([0], [20])["logit"][0] == want["logit"][0]
    t.chat.extend([0], [0], [[30]])                                   # the line the prefill named is rewritten
    assert t.chat.slot_state(0) == (len(item.input_ids), False)
    out = [np.full(1, -7.5, np.float32) for _ in range(3)] + [np.full(1, -9, np.int32)]
    pf = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    rc = t.chat.lib.vr_chat_slot_score(t.chat._h, 1, _i32([0]), _i32([20]), pf(out[0]), pf(out[1]), pf(out[2]),
                                       out[3].ctypes.data_as(C.POINTER(C.c_int32)), t.chat._stream())
    assert rc == STATE and out[0][0] == np.float32(-7.5)
    assert t.chat.lib.vr_chat_slot_score(t.chat._h, 1, _i32([3]), _i32([20]), pf(out[0]), pf(out[1]), pf(out[2]),
                                         out[3].ctypes.data_as(C.POINTER(C.c_int32)), t.chat._stream()) == INVALID


def test_truncate_then_extend(tiny):
    t, item = tiny, tiny.items[1]
    V = t.cfg.vocab_size
    a, b = _cont(41, 8, V), _cont(42, 5, V)
    t.chat.prefill(0, 0, item)
    t.chat.extend([0], [0], [a], seen="join")
    t.chat.truncate(0, 3)
    assert t.chat.row_state(0) == (0, 3)
    out = [np.full(1, -7.5, np.float32) for _ in range(3)] + [np.full(1, -9, np.int32)]
    pf = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    rc = t.chat.lib.vr_chat_row_score(t.chat._h, 1, _i32([0]), _i32([20]), pf(out[0]), pf(out[1]), pf(out[2]),
                                      out[3].ctypes.data_as(C.POINTER(C.c_int32)), t.chat._stream())
    assert rc == STATE and out[0][0] == np.float32(-7.5) and out[3][0] == -9
    with pytest.raises(_lib.VisragHipError):
        t.chat.logits(0)
    t.chat.extend([0], [0], [b])
    assert t.chat.row_state(0) == (0, 8)
    _close(t.chat.logits(0), _oracle(t, item, a[:3] + b)[-1], 1, "extend 8 -> truncate 3 -> extend 5:")
    for bad in (-1, 9):
        assert t.chat.lib.vr_chat_row_truncate(t.chat._h, 0, bad) == INVALID
    assert t.chat.lib.vr_chat_row_truncate(t.chat._h, 9, 0) == INVALID and t.chat.row_state(0) == (0, 8)


def _raw_extend(chat, slots, rows, token_lists, targets=None, seen=0, B=None):
    """vr_chat_extend with sentinel-filled outputs -> (status, outputs)"""
    off = np.zeros(len(token_lists) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(x) for x in token_lists])
    toks = np.asarray([x for tl in token_lists for x in tl] + [0], dtype=np.int32)
    n = int(off[-1]) + 4
    outs = [np.full(n, -7.5, dtype=np.float32) for _ in range(3)] + [np.full(n, -9, dtype=np.int32)]
    p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    pf = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    tg = np.asarray([x for tl in targets for x in tl] + [0], dtype=np.int32) if targets is not None else None
    rc = chat.lib.vr_chat_extend(chat._h, len(token_lists) if B is None else B, _i32(slots), _i32(rows), p32(off), p32(toks),
                                 p32(tg) if tg is not None else None, seen, pf(outs[0]), pf(outs[1]), pf(outs[2]), p32(outs[3]),
                                 chat._stream())
    return rc, outs


def _untouched(outs):
    return all((o == np.float32(-7.5)).all() for o in outs[:3]) and (outs[3] == -9).all()


def test_capacity_edges_and_argument_errors(tiny):
    t, item = tiny, tiny.items[1]
    V, plen = t.cfg.vocab_size, len(tiny.items[1].input_ids)
    small = HipChat(t.enc, max_len=plen + 9, max_rows=3, dim_model_base=t.dmb, max_slots=2, max_new=6)
    small.load_head(t.head.cuda())
    c = _cont(51, 9, V)
    # a tail filled exactly to max_new
    small.prefill(0, 0, item)
    small.extend([0], [0], [c[:2]])
    small.extend([0], [0], [c[2:6]])
    assert small.row_state(0) == (0, 6)
    _close(small.logits(0), _oracle(t, item, c[:6])[-1], 1, "tail filled to max_new:")
    keep = small.logits(0)
    rc, outs = _raw_extend(small, [0], [0], [[20]], targets=[[21]])
    assert rc == CAPACITY and _untouched(outs) and small.row_state(0) == (0, 6) and small.logits(0).tobytes() == keep.tobytes()
    rc, outs = _raw_extend(small, [0], [1], [c[:7]], targets=[c[1:8]])               # a fresh row: 7 > max_new
    assert rc == CAPACITY and _untouched(outs) and small.row_state(1) == (-1, 0)
    # a sequence that ends exactly at max_len: a prompt of plen + 4 tokens, then 5 more
    long = _plus(item, c[:4])
    small.prefill(1, 1, long)
    small.extend([1], [1], [c[4:9]])
    assert small.row_state(1) == (1, 5)
    _close(small.logits(1), _oracle(t, item, c)[-1], 1, "sequence ending at max_len:")
    keep = small.logits(1)
    rc, outs = _raw_extend(small, [1], [1], [[20]], targets=[[21]])
    assert rc == CAPACITY and _untouched(outs) and small.row_state(1) == (1, 5) and small.logits(1).tobytes() == keep.tobytes()
    assert _raw_extend(small, [0, 0, 0, 0], [0, 1, 2, 2], [[20]] * 4)[0] == CAPACITY                 # B > max_rows
    # VR_ERR_INVALID: state and outputs untouched
    small.prefill(0, 0, item)
    small.extend([0], [0], [c[:2]])
    state = [small.row_state(r) for r in range(3)]
    keep = small.logits(0)
    for kw in (dict(slots=[0], rows=[2], token_lists=[[]]), dict(slots=[0], rows=[2], token_lists=[[V]]),
               dict(slots=[0], rows=[2], token_lists=[[-1]]), dict(slots=[0], rows=[2], token_lists=[[20]], targets=[[V]]),
               dict(slots=[0], rows=[2], token_lists=[[20]], targets=[[-2]]), dict(slots=[2], rows=[2], token_lists=[[20]]),
               dict(slots=[0, 0], rows=[2, 2], token_lists=[[20], [21]]), dict(slots=[1], rows=[0], token_lists=[[20]]),
               dict(slots=[0], rows=[3], token_lists=[[20]]), dict(slots=[0], rows=[2], token_lists=[[20]], B=0),
               dict(slots=[0], rows=[2], token_lists=[[20]], seen=3)):
        kw.setdefault("targets", [[20] * len(x) for x in kw["token_lists"]])
        rc, outs = _raw_extend(small, **kw)
        assert rc == INVALID and _untouched(outs), kw
        assert [small.row_state(r) for r in range(3)] == state and small.logits(0).tobytes() == keep.tobytes(), kw
    p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    assert small.lib.vr_chat_extend(small._h, 1, _i32([0]), _i32([2]), None, None, None, 0, None, None, None, None, small._stream()) == INVALID
    one = np.asarray([20], np.int32)
    assert small.lib.vr_chat_extend(small._h, 1, _i32([0]), _i32([2]), p32(np.asarray([0, 1], np.int32)), p32(one), p32(one), 0, None, None,
                                    None, None, small._stream()) == INVALID                # targets without outputs
    bare = HipChat(t.enc, max_len=64, max_rows=1, dim_model_base=t.dmb)
    assert _raw_extend(bare, [0], [0], [[20]])[0] == STATE
    bare.close()
    small.close()


def test_seen_modes(tiny):
    t, item = tiny, tiny.items[1]
    V = t.cfg.vocab_size

    def greedy_with_penalty(row):
        sc, tk, _ = t.chat.select(GREEDY, [[row]], 1, repetition_penalty=PEN)
        return int(tk[0, 0])

    def host(logits, seen):
        l = logits.astype(np.float32).copy()
        ids = np.asarray(sorted(seen), dtype=np.int64)
        if len(ids):
            l[ids] = np.where(l[ids] < 0, l[ids] * np.float32(PEN), l[ids] / np.float32(PEN))
        return l

    t.chat.prefill(0, 0, item)
    l0 = t.chat.logits(0)
    order = np.argsort(-l0)
    # forced tokens: the prompt row's two best ids and a third — after "join" exactly these are penalised
    forced = [int(order[0]), int(order[1]), 500]
    for mode, seen_after in (("join", set(forced)), ("keep", set()), ("clear", set())):
        t.chat.prefill(0, 0, item)
        t.chat.extend([0], [0], [forced], seen=mode)
        l = t.chat.logits(0)
        pen = host(l, seen_after)
        top = np.sort(pen)[-2:]
        assert top[1] - top[0] > 0, "a tie: pick other forced tokens"
        assert greedy_with_penalty(0) == int(np.argmax(pen)), mode
        if mode == "join":
            # make the penalty bite: force the row's own argmax, then the penalised choice must differ from the plain one
            best = int(np.argmax(l))
            t.chat.extend([0], [0], [[best]], seen="join")
            l2 = t.chat.logits(0)
            want = int(np.argmax(host(l2, set(forced) | {best})))
            assert greedy_with_penalty(0) == want
            # "keep" afterwards leaves the set as it was, "clear" empties it
            t.chat.extend([0], [0], [[600]], seen="keep")
            l3 = t.chat.logits(0)
            assert greedy_with_penalty(0) == int(np.argmax(host(l3, set(forced) | {best})))
            t.chat.extend([0], [0], [[601]], seen="clear")
            assert greedy_with_penalty(0) == int(np.argmax(host(t.chat.logits(0), set())))
    # the penalty must BITE: put the row's own argmax into its seen set without changing the context — join it, truncate it
    # away again (the seen set stays) and feed the last token anew — then the penalised choice is another token
    t1, t2, big = 300, 301, 4.0
    t.chat.prefill(0, 0, item)
    t.chat.extend([0], [0], [[t1]], seen="keep")
    t.chat.extend([0], [0], [[t2]], seen="keep")                     # (the same call shape as below: the same bits)
    l = t.chat.logits(0)
    a = int(np.argmax(l))
    t.chat.extend([0], [0], [[a]], seen="join")
    t.chat.truncate(0, 1)
    t.chat.extend([0], [0], [[t2]], seen="keep")
    l2 = t.chat.logits(0)
    assert l2.tobytes() == l.tobytes(), "the same context, the same call: the same logits"
    pen = l2.copy()
    pen[a] = l2[a] * big if l2[a] < 0 else l2[a] / big
    assert int(np.argmax(pen)) != a, "the precondition: the penalty moves the argmax"
    sc, tk, _ = t.chat.select(GREEDY, [[0]], 1, repetition_penalty=big)
    assert int(tk[0, 0]) == int(np.argmax(pen)) != a                  # "join" marked the id, "keep" kept it
    t.chat.truncate(0, 1)
    t.chat.extend([0], [0], [[t2]], seen="clear")
    sc, tk, _ = t.chat.select(GREEDY, [[0]], 1, repetition_penalty=big)
    assert int(tk[0, 0]) == int(np.argmax(t.chat.logits(0))) == a     # "clear" emptied the set the join had changed the choice with


# ============================================================ public surface =================================================
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
                                                                    max_inp_length=720, max_new_tokens=32, num_beams=3, batch=3)
    return model, F, tok, question_pages(F, t.cfg, 0)


def test_score_answers_and_choose_shared(tiny, public):
    model, F, tok, pages = public
    msgs = msgs_of(F, 0)
    answers = [["w100 w200", "w300", "w100 w200 w400 w17"], ["w100 w200 w400"]]
    plain = model.score_answers(pages[:2], [msgs, msgs], answers, tok, repetition_penalty=PEN)
    shared = model.score_answers(pages[:2], [msgs, msgs], answers, tok, repetition_penalty=PEN, shared_prefill=True)
    bar = LOGIT_BAR * float(F["q0_absmax"])
    worst = 0.0
    assert [len(o) for o in shared] == [3, 1]
    for po, so in zip(plain, shared):
        for p, s in zip(po, so):
            assert set(p) == set(s) and len(p["token_logprobs"]) == len(s["token_logprobs"])
            err = float(np.abs(p["token_logprobs"] - s["token_logprobs"]).max())
            worst = max(worst, err / (4 * bar))
            assert err <= 4 * bar
            assert abs(p["score"] - s["score"]) <= PEN * 2 * bar
    print("score_answers shared vs default: worst token log-prob error / (4 bar)", worst)
    # choose: options whose default-route margin exceeds the sequence bar
    p, sl = chat_prompt(msgs, pages[0], tok, tiny.cfg)
    item = _prompt_item(p + "<AI>", sl, tok, 2048)
    greedy = generate_items(model._chat, [item], max_new_tokens=6, num_beams=1, repetition_penalty=1.0)[0]
    body = [g for g in greedy if g != tok.eos_id]
    text = lambda ids: " ".join(f"w{i}" for i in ids)  # noqa: E731
    wrong = [body[:-1] + [16 + (body[-1] + d) % (tiny.cfg.vocab_size - 16)] for d in (301, 602)]
    options = [text(wrong[0]), text(body), text(wrong[1])]
    index, scores = model.choose(pages[0], msgs, options, tok, append_eos=False)
    keys = sorted(float(s["score"]) for s in scores)
    assert keys[-1] - keys[-2] > 2 * bar, "the precondition: a margin above the sequence bar"
    assert model.choose(pages[0], msgs, options, tok, append_eos=False, shared_prefill=True)[0] == index


def test_marginal_selection_shared(tiny, public):
    model, F, tok, pages = public
    msgs, doc = msgs_of(F, 0), F["q0_doc_scores"].tolist()
    n_new = int(F["max_new"])
    chat = model._chat
    a0, d0 = model.marginal_selection(pages, msgs, doc, tok, details=True, max_new_tokens=n_new)
    # the pages fit one chunk of the generator's cache: the scoring reuses the slots the generation left behind — the only
    # prefills are the generation's own, one per page
    assert len(pages) <= chat.max_slots
    before = chat.prefills
    a1, d1 = model.marginal_selection(pages, msgs, doc, tok, details=True, max_new_tokens=n_new, shared_prefill=True)
    assert chat.prefills - before == len(pages), "the scoring pass prefilled a resident page again"
    assert d0["candidates"] == d1["candidates"] and d0["doc_probs"] == d1["doc_probs"]
    bar = PEN * 2 * LOGIT_BAR * float(F["q0_absmax"])
    err = float(np.abs(np.asarray(d0["S"]) - np.asarray(d1["S"])).max())
    print("marginal_selection: S shared vs default, error / bar", err / bar)
    assert err <= bar


def test_chat_session(tiny, public):
    model, F, tok, pages = public
    chat = model._chat
    # (the stand-in tokenizer splits at white space only: blanks around "<AI>" and the answers keep the turns' ids apart)
    q1, q2 = str(F["q0_question"]) + " ", "and what else is on the page "
    kw = dict(sampling=False, num_beams=1, repetition_penalty=1.0, max_new_tokens=3)
    sess = model.chat_session(pages[0], tok, **kw)
    a1 = sess.ask([{"role": "user", "content": q1}])
    assert sess.session.last_path == "prefill" and a1 == model.chat([pages[0]], [[{"role": "user", "content": q1}]], tok, assistant_turn=True, **kw)[0]
    # second turn: the logits along chat(full history)'s own greedy tokens, teacher-forced on both routes
    hist = [{"role": "user", "content": q1}, {"role": "assistant", "content": " " + a1 + " "}, {"role": "user", "content": q2}]
    item2 = sess.session.make_item(hist)
    greedy = generate_items(chat, [item2], max_new_tokens=4, num_beams=1, repetition_penalty=1.0)[0]
    chat_rows = []
    sess.session.chat.prefill(2, 8, item2)
    for g in greedy:
        chat_rows.append(chat.logits(8))
        chat.step([2], [8], [g])
    # (generate_items above prefilled slot 0: the session's cache is gone, so turn one is fed again first)
    sess = model.chat_session(pages[0], tok, **kw)
    assert sess.ask([{"role": "user", "content": q1}]) == a1
    path = sess.session.feed(item2)
    assert path == "extend" and sess.session.counts == {"prefill": 1, "extend": 1, "truncate": 0}
    base = chat.row_state(0)[1]
    for j, g in enumerate(greedy):
        _close(chat.logits(0), chat_rows[j], 2, f"session turn two, position {j}:")
        chat.step([0], [0], [g])
    chat.truncate(0, base)
    a2 = sess.ask(hist)
    assert isinstance(a2, str) and sess.session.counts["prefill"] == 1
    # an edited earlier answer: the ids part inside the tail
    edited = [{"role": "user", "content": q1}, {"role": "assistant", "content": " w333 w334 "}, {"role": "user", "content": q2}]
    before = dict(sess.session.counts)
    sess.ask(edited)
    assert sess.session.last_path == "truncate" and sess.session.counts["truncate"] == before["truncate"] + 1
    assert sess.session.fed[:len(sess.session.make_item(edited).input_ids)] == sess.session.make_item(edited).input_ids
    # another page: afresh
    sess.ask(edited, image=pages[1])
    assert sess.session.last_path == "prefill" and sess.session.counts["prefill"] == 2


def test_chat_session_defaults_foreign_use_and_beams(tiny, public):
    model, F, tok, pages = public
    chat = model._chat
    q1, q2 = str(F["q0_question"]) + " ", "and what else is on the page "
    sess = model.chat_session(pages[0], tok)                          # the defaults: max_new_tokens follows the generator's rows
    assert sess.session.max_new_tokens == chat.max_new
    # beams: rows 0..2 stay bound from the first turn; the second turn extends and decodes again
    kw = dict(sampling=False, num_beams=3, max_new_tokens=4)
    sess = model.chat_session(pages[0], tok, **kw)
    m1 = [{"role": "user", "content": q1}]
    a1 = sess.ask(m1)
    assert a1 == model.chat([pages[0]], [m1], tok, assistant_turn=True, **kw)[0]
    # ... which prefilled slot 0 behind the session's back: the next turn notices and prefills afresh
    hist = m1 + [{"role": "assistant", "content": " " + a1 + " "}, {"role": "user", "content": q2}]
    a2 = sess.ask(hist)
    assert sess.session.last_path == "prefill" and sess.session.counts["prefill"] == 2
    assert a2 == model.chat([pages[0]], [hist], tok, assistant_turn=True, **kw)[0]       # the same route: the same bits
    sess = model.chat_session(pages[0], tok, **kw)
    assert sess.ask(m1) == a1
    base = len(sess.session.fed) - sess.session.plen
    assert chat.row_state(0) == (0, base) and base == 0                # beams: the tail is cut back to what was fed
    a2x = sess.ask(hist)
    assert sess.session.last_path == "extend" and sess.session.counts == {"prefill": 1, "extend": 1, "truncate": 0}
    assert chat.row_state(0) == (0, len(sess.session.fed) - sess.session.plen) and isinstance(a2x, str)
    # the extended beam search against the fresh one: the best hypothesis' first token wherever the fresh route's top-2
    # margin at that position is beyond twice the bar (two bf16 routes)
    item2 = sess.session.make_item(hist)
    chat.prefill(2, 8, item2)
    fresh = chat.logits(8)
    sess2 = model.chat_session(pages[0], tok, **kw)
    sess2.ask(m1)
    sess2.session.feed(item2)
    _close(chat.logits(0), fresh, 2, "beam session, second turn's first position:")
