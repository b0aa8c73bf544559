"""CPU side of the chat-extend tests: the fp64 two-segment attention reference against plain causal attention (and against
deliberately wrong masks: the op bar can tell them apart), and the Python layer — generation.score_items_shared's packing,
row chunking and token-0 / rest split, generation.ChatSession's prefix / truncate / re-prefill decisions — over the host
stand-ins of tests/chat_extend_ref.py."""
import numpy as np
import pytest

from tests.chat_extend_ref import (FakeChat, FakeEnc, causal_concat_attention, fake_logprob, two_segment_attention,
                                   within_bar)
from visrag_amd.generation import ChatSession, resident_after_generation, score_items_shared, sequence_score
from visrag_amd.preprocess import PreparedItem


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plen,t0,n,H", [(1, 0, 1, 1), (3, 0, 4, 2), (5, 2, 3, 2), (2, 4, 1, 1), (7, 1, 6, 3)])
def test_two_segments_equal_causal_attention_over_the_concatenation(plen, t0, n, H):
    rng = np.random.default_rng(plen * 100 + t0 * 10 + n)
    T = plen + t0 + n
    q, k, v = (rng.standard_normal((T, H, 8)) for _ in range(3))
    # the tail planes hold MORE rows than the sequence may read: whatever they are must not matter
    tk = np.concatenate([k[plen:], 1e3 * rng.standard_normal((3, H, 8))])
    tv = np.concatenate([v[plen:], 1e3 * rng.standard_normal((3, H, 8))])
    got = two_segment_attention(q[T - n:], k[:plen], v[:plen], tk, tv, t0, scale=8 ** -0.5)
    ref = causal_concat_attention(q, k, v, n, scale=8 ** -0.5)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)


def test_a_wrong_mask_moves_the_result_past_the_op_bar():
    rng = np.random.default_rng(1)
    plen, t0, n, H = 5, 2, 6, 2
    q = rng.standard_normal((n, H, 64))
    pk, pv = rng.standard_normal((plen, H, 64)), rng.standard_normal((plen, H, 64))
    tk, tv = rng.standard_normal((t0 + n, H, 64)), rng.standard_normal((t0 + n, H, 64))
    ref = two_segment_attention(q, pk, pv, tk, tv, t0)
    assert within_bar(ref, ref)[0]
    for wrong in (dict(tail_shift=-1), dict(tail_shift=1), dict(hide_prompt=True)):
        ok, worst = within_bar(two_segment_attention(q, pk, pv, tk, tv, t0, **wrong), ref)
        assert not ok and worst > 2.0, (wrong, worst)


# ---- score_items_shared ----------------------------------------------------------------------------------------------------
def _item(ids):
    return PreparedItem(input_ids=list(ids), image_bound=[], slices=[])


def _expected(prompt, cont, pen=1.0, lpen=1.0):
    lp = []
    for j, t in enumerate(cont):
        x, lse, _, _ = fake_logprob(list(prompt) + list(cont[:j]), t)
        lp.append(np.float64(np.float32(x)) - np.float64(np.float32(lse)))
    return np.asarray(lp), sequence_score(lp, cont, pen, lpen)


def test_shared_scoring_packs_prefills_and_chunks_rows():
    chat = FakeChat(max_rows=4, max_slots=2, max_new=8, enc=FakeEnc(max_tokens=40, max_seqs=4))
    prompts = [[1, 20, 21, 22], [1, 30, 31], [1, 40, 41, 42, 43]]
    conts = [[[50, 51, 52], [60], [70, 71], [80, 81, 82, 83], [90, 91]], [[55]], [[65, 66, 66, 67], [75, 76]]]
    out = score_items_shared(chat, [_item(p) for p in prompts], conts, repetition_penalty=1.2, length_penalty=0.5)
    assert [len(o) for o in out] == [5, 1, 2]
    for p, cs, rs in zip(prompts, conts, out):
        for c, r in zip(cs, rs):
            lp, score = _expected(p, c, 1.2, 0.5)
            np.testing.assert_allclose(r["token_logprobs"], lp, rtol=0, atol=1e-12)
            assert abs(r["score"] - score) < 1e-12 and len(r["top_tokens"]) == len(c) == len(r["greedy_match"])
            assert set(r) == {"token_logprobs", "sum", "score", "greedy_match", "top_tokens"}
    kinds = [e[0] for e in chat.log]
    # one prefill per ITEM: two slots and half of the four rows per pack -> packs of two items, one packed pass each
    pre = [e for e in chat.log if e[0] == "prefill_batch"]
    assert [e[3] for e in pre] == [[4, 3], [5]] and "prefill" not in kinds
    # token 0 of all of an item's continuations is ONE row_score call on the prompt's row
    rs = [e for e in chat.log if e[0] == "row_score"]
    assert [e[2] for e in rs] == [[50, 60, 70, 80, 90], [55], [65, 75]] and all(len(set(e[1])) == 1 for e in rs)
    # the rest goes through extend: tokens c[:-1]; one-token continuations need none; rows never exceed those at hand
    ext = [e for e in chat.log if e[0] == "extend"]
    fed = [toks for e in ext for toks in e[3]]
    assert sorted(fed) == sorted(c[:-1] for cs in conts for c in cs if len(c) > 1)
    assert all(len(e[2]) <= 4 and len(set(e[1])) == 1 for e in ext)
    # item 0: four longer continuations on the two rows its pack leaves free -> two calls of two rows
    assert [len(e[2]) for e in ext[:2]] == [2, 2]


def test_shared_scoring_on_a_resident_prompt_and_its_errors():
    chat = FakeChat(max_rows=3, max_slots=2, max_new=4)
    chat.prefill(1, 2, _item([1, 20, 21]))
    chat.log.clear()
    out = score_items_shared(chat, [_item([1, 20, 21])], [[[50, 51], [60, 61, 62]]], prefilled={0: (1, 2)})
    assert not [e for e in chat.log if e[0].startswith("prefill")]
    for c, r in zip([[50, 51], [60, 61, 62]], out[0]):
        np.testing.assert_allclose(r["token_logprobs"], _expected([1, 20, 21], c)[0], atol=1e-12)
    assert chat.row_state(2) == (1, 0)                        # the prompt's row keeps its empty tail: rows 0 and 1 carried the tails
    with pytest.raises(ValueError):
        score_items_shared(chat, [_item([1, 2])], [[[5, 6, 7, 8, 9]]])          # longer than max_new = 4
    with pytest.raises(ValueError):
        score_items_shared(chat, [_item([1, 2])], [[[]]])
    with pytest.raises(ValueError):
        score_items_shared(chat, [_item([1, 2])], [[[5]]], prefilled={0: (0, 0)})   # row 0 does not hold slot 0's prompt
    # a single row: the prompt's own row carries the tails, one continuation per call
    one = FakeChat(max_rows=1, max_slots=1, max_new=4)
    out = score_items_shared(one, [_item([1, 20])], [[[50, 51], [60, 61]]])
    np.testing.assert_allclose(out[0][1]["token_logprobs"], _expected([1, 20], [60, 61])[0], atol=1e-12)
    assert [len(e[2]) for e in one.log if e[0] == "extend"] == [1, 1]


# ---- ChatSession -----------------------------------------------------------------------------------------------------------
class _Merging:
    """A tokenizer stand-in whose concatenation does NOT split alike: letters are ids 100 + index, but an adjacent "ab" is ONE
    token (id 300) — two generated tokens a, b read back as one."""
    eos_id = 2

    def encode(self, text):
        ids, i = [1], 0
        while i < len(text):
            if text.startswith("ab", i):
                ids.append(300); i += 2
            else:
                ids.append(100 + ord(text[i]) - ord("a")); i += 1
        return ids


def _session(chat, page="p", max_new_tokens=2):
    tok = _Merging()
    state = {"page": page}

    def make_item(history):
        return PreparedItem(input_ids=tok.encode("".join(history)), image_bound=[], slices=[np.frombuffer(state["page"].encode(), np.uint8)])

    return ChatSession(chat, make_item, eos=tok.eos_id, max_new_tokens=max_new_tokens), state, tok


def test_session_extends_truncates_and_prefills_afresh():
    chat = FakeChat(max_rows=1, max_slots=1, max_new=16, max_len=64)
    s, state, tok = _session(chat)
    first = s.ask_ids(["cde"])
    assert s.last_path == "prefill" and len(first) == 2
    assert chat.context(0) == s.fed == tok.encode("cde") + first[:1]       # the last generated token was never stepped
    # the fed ids are a prefix of the next turn's ids: only the remainder is appended, with an empty seen set
    turn2 = tok.encode("cde") + first[:1] + [105, 106]
    s.make_item = lambda h: PreparedItem(input_ids=list(h), image_bound=[], slices=[np.frombuffer(state["page"].encode(), np.uint8)])
    chat.log.clear()
    s.ask_ids(turn2)
    assert s.last_path == "extend" and s.counts == {"prefill": 1, "extend": 1, "truncate": 0}
    ext = [e for e in chat.log if e[0] == "extend"]
    assert len(ext) == 1 and ext[0][3] == [[105, 106]] and ext[0][4] == "clear" and not [e for e in chat.log if e[0] == "prefill"]
    assert chat.context(0)[:len(turn2)] == turn2 and chat.context(0) == s.fed
    # the history read back splits otherwise INSIDE the tail: truncate to the common prefix, then append
    fed = list(s.fed)
    edited = fed[:len(tok.encode("cde")) + 1] + [300, 107]
    chat.log.clear()
    s.ask_ids(edited)
    assert s.last_path == "truncate" and s.counts["truncate"] == 1
    tr = [e for e in chat.log if e[0] == "truncate"]
    assert tr == [("truncate", 0, 1)] and [e[3] for e in chat.log if e[0] == "extend"] == [[[300, 107]]]
    assert chat.context(0)[:len(edited)] == edited
    # ids equal to what is fed already: the last id is fed again so that the logits are current
    chat.log.clear()
    s.ask_ids(list(s.fed))
    assert s.last_path == "truncate" and chat.context(0)[:len(s.fed) - 1] == s.fed[:-1]
    # the prompt itself changed, then another page with the same ids: afresh both times
    changed = [1, 109] + edited[2:]
    s.ask_ids(changed)
    assert s.last_path == "prefill" and s.plen == len(changed)
    state["page"] = "q"
    s.ask_ids(changed)
    assert s.last_path == "prefill" and s.counts["prefill"] == 3
    # a tail that would not fit max_new: afresh
    small = FakeChat(max_rows=1, max_slots=1, max_new=4, max_len=64)
    s2, st2, _ = _session(small)
    s2.make_item = lambda h: PreparedItem(input_ids=list(h), image_bound=[], slices=[])
    s2.ask_ids([1, 5, 6])
    s2.ask_ids([1, 5, 6] + s2.fed[3:] + [7, 8])
    assert s2.last_path == "prefill"


def test_session_with_the_merging_tokenizer_is_right_either_way():
    """two generated tokens a, b come back as the single token "ab": the session must end up holding the NEW ids"""
    chat = FakeChat(max_rows=1, max_slots=1, max_new=16, max_len=64)
    s, state, tok = _session(chat)
    s.ask_ids(["cd"])
    gen = [100, 101]                                           # pretend the answer was "a", "b"
    chat.tail[0] = list(gen); s.fed = tok.encode("cd") + gen
    s.ask_ids(["cd", "ab", "e"])                               # reads back as [.., 300, 104]
    want = tok.encode("cdabe")
    assert 300 in want and s.last_path == "truncate"
    assert chat.context(0)[:len(want)] == want and s.fed[:len(want)] == want


def test_shared_scoring_reuses_prompts_a_generation_left_behind():
    """two pages generated with two beams each: rows carry tails, the prompts' logits are still readable -> no prefill"""
    chat = FakeChat(max_rows=4, max_slots=2, max_new=6)
    prompts = [[1, 20, 21], [1, 30, 31, 32]]
    for i, p in enumerate(prompts):
        chat.prefill(i, 2 * i, _item(p))
        chat.step([i], [2 * i], [90 + i])
        chat.tail[2 * i + 1], chat.row_slot[2 * i + 1] = [95 + i], i          # the second beam's row
    assert [chat.slot_state(i) for i in range(2)] == [(3, True), (4, True)] and chat.row_state(0) == (0, 1)
    chat.log.clear()
    conts = [[50, 51, 52], [60]]
    out = score_items_shared(chat, [_item(p) for p in prompts], [conts, conts], prefilled={0: (0, None), 1: (1, None)})
    assert not [e for e in chat.log if e[0].startswith("prefill")] and not [e for e in chat.log if e[0] == "row_score"]
    assert [e[1] for e in chat.log if e[0] == "slot_score"] == [[0, 0], [1, 1]]
    for p, rs in zip(prompts, out):
        for c, r in zip(conts, rs):
            np.testing.assert_allclose(r["token_logprobs"], _expected(p, c)[0], atol=1e-12)
    # the rows of the generation were truncated and carried the tails; an extend on the prompt's row ends the reuse
    assert chat.slot_state(0) == (3, False)
    with pytest.raises(ValueError):
        score_items_shared(chat, [_item(prompts[0])], [conts], prefilled={0: (0, None)})
    with pytest.raises(ValueError):
        score_items_shared(chat, [_item([1, 2, 3, 4, 5])], [conts], prefilled={0: (1, None)})      # another prompt length


def test_session_notices_a_foreign_prefill_and_a_moved_row():
    chat = FakeChat(max_rows=2, max_slots=2, max_new=16, max_len=64)
    s, state, tok = _session(chat)
    s.make_item = lambda h: PreparedItem(input_ids=list(h), image_bound=[], slices=[])
    s.ask_ids([1, 5, 6])
    nxt = list(s.fed) + [7]
    chat.prefill(0, 0, _item([1, 9, 9, 9]))                   # somebody else rewrites slot 0
    s.ask_ids(nxt)
    assert s.last_path == "prefill" and chat.context(0)[:len(nxt)] == nxt
    nxt = list(s.fed) + [8]
    chat.step([0], [0], [44])                                 # somebody else moves row 0 on
    s.ask_ids(nxt)
    assert s.last_path == "prefill" and chat.context(0)[:len(nxt)] == nxt
    nxt = list(s.fed) + [9]
    chat.prefill(1, 1, _item([1, 2]))                         # another slot, another row: none of the session's business
    s.ask_ids(nxt)
    assert s.last_path == "extend"
    # a remainder longer than the encoder's max_tokens: afresh, where the extend would have been refused
    chat.enc.max_tokens = 3
    s.ask_ids(list(s.fed) + [11, 12, 13, 14])
    assert s.last_path == "prefill"


def test_no_reuse_when_the_generation_ran_in_more_than_one_chunk():
    """max_rows 4, two beams: chunks of two pages.  Three pages of EQUAL prompt length: the second chunk leaves page 2 in slot
    0 and page 1 in slot 1 — a length match would score page 0 on page 2's prompt"""
    chat = FakeChat(max_rows=4, max_slots=3, max_new=6)
    prompts = [[1, 20, 21], [1, 30, 31], [1, 40, 41]]
    items = [_item(p) for p in prompts]
    for chunk in ([0, 1], [2]):                               # what generate_items does: item j of a chunk into slot j, row 2 j
        for j, i in enumerate(chunk):
            chat.prefill(j, 2 * j, items[i])
            chat.step([j], [2 * j], [90])
    assert chat.slot_state(0) == (3, True) and chat.slot_state(1) == (3, True)
    assert resident_after_generation(chat, items, 2) == {}
    assert resident_after_generation(chat, items[:2], 2) == {1: (1, None)}        # one chunk's worth: slot 0 holds ANOTHER page
    assert resident_after_generation(chat, [items[2], items[1]], 2) == {0: (0, None), 1: (1, None)}
    with pytest.raises(ValueError):                           # and the scoring refuses a slot that holds another prompt
        score_items_shared(chat, items, [[[50, 51]]] * 3, prefilled={0: (0, None)})
    chat.log.clear()
    conts = [[50, 51], [60]]
    out = score_items_shared(chat, items, [conts] * 3, prefilled=resident_after_generation(chat, items, 2))
    assert sum(len(e[3]) for e in chat.log if e[0] == "prefill_batch") == 3 and not [e for e in chat.log if e[0] == "slot_score"]
    for p, rs in zip(prompts, out):
        for c, r in zip(conts, rs):
            np.testing.assert_allclose(r["token_logprobs"], _expected(p, c)[0], atol=1e-12)
