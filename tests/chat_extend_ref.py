"""fp64 references and host stand-ins for the chat-extend tests (vr_chat_extend and the Python layer over it).

two_segment_attention is the definition the device kernel (csrc/chat_extend.hip) is held to: query j of a sequence with
plen prompt keys and t0 tail tokens already present sees every prompt key and the tail keys [0, t0 + j].  `tail_shift`
and `hide_prompt` are deliberately WRONG masks: the tests use them to show that the bar can tell them apart."""
import numpy as np


def _softmax_rows(s):
    s = s - s.max(axis=-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(axis=-1, keepdims=True)


def two_segment_attention(q, pk, pv, tk, tv, t0, scale=0.125, tail_shift=0, hide_prompt=False):
    """q [n][H][D]; prompt keys / values [plen][H][D]; tail keys / values [>= t0 + n][H][D] -> out [n][H][D], fp64.
    tail_shift = -1 hides each query's own key (causal off by one); hide_prompt drops the prompt segment."""
    q, pk, pv, tk, tv = (np.asarray(a, dtype=np.float64) for a in (q, pk, pv, tk, tv))
    n, H, D = q.shape
    plen, m = pk.shape[0], t0 + n
    vis = t0 + np.arange(n)[:, None] + 1 + tail_shift      # query j sees tail keys [0, vis[j])
    mask = np.concatenate([np.full((n, plen), not hide_prompt), np.arange(m)[None, :] < vis], axis=1)
    out = np.zeros((n, H, D))
    for h in range(H):
        k = np.concatenate([pk[:, h], tk[:m, h]], axis=0)
        v = np.concatenate([pv[:, h], tv[:m, h]], axis=0)
        s = np.where(mask, (q[:, h] @ k.T) * scale, -np.inf)
        out[:, h] = _softmax_rows(s) @ v
    return out


def causal_concat_attention(q_all, k_all, v_all, n_new, scale=0.125):
    """Plain causal attention over one sequence [T][H][D], restricted to its last n_new queries -> [n_new][H][D], fp64."""
    q_all, k_all, v_all = (np.asarray(a, dtype=np.float64) for a in (q_all, k_all, v_all))
    T, H, D = q_all.shape
    out = np.zeros((n_new, H, D))
    for j in range(n_new):
        t = T - n_new + j
        for h in range(H):
            p = _softmax_rows((k_all[:t + 1, h] @ q_all[t, h])[None, :] * scale)[0]
            out[j, h] = p @ v_all[:t + 1, h]
    return out


def within_bar(got, ref, rtol=2e-2, atol=2e-2):
    """-> (ok, worst |got - ref| / (atol + rtol |ref|)): the standing bar of the attention tests of tests/test_gpu_ops.py"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ratio = np.abs(got - ref) / (atol + rtol * np.abs(ref))
    worst = float(ratio.max()) if np.isfinite(ratio).all() else float("inf")
    return worst <= 1.0, worst


# ---- a host stand-in for HipChat: the cache is the id lists themselves, the "model" a deterministic function of the context
def fake_logprob(context, token):
    """(logit, lse, top_logit, top_token) of `token` after `context` — any deterministic function will do"""
    h = (sum((i + 1) * int(t) for i, t in enumerate(context)) * 2654435761 + 97 * int(token)) % 1000003
    top = (sum(int(t) for t in context) * 31 + len(context)) % 900 + 16
    return -(h % 997) / 100.0 - 0.5, 0.25, 3.0, top


class FakeEnc:
    def __init__(self, max_tokens=64, max_seqs=4):
        self.max_tokens, self.max_seqs = max_tokens, max_seqs


class FakeChat:
    """HipChat's prefill / prefill_batch / extend / row_score / truncate / row_state / select / step on id lists, with the
    library's binding rules and a log of the calls."""

    def __init__(self, max_rows=4, max_slots=2, max_new=8, max_len=64, enc=None):
        self.max_rows, self.max_slots, self.max_new, self.max_len = max_rows, max_slots, max_new, max_len
        self.enc = enc or FakeEnc()
        self.prompt = [None] * max_slots                  # per slot: (ids, slices key)
        self.row_slot, self.tail, self.has_logits = [-1] * max_rows, [[] for _ in range(max_rows)], [False] * max_rows
        self.seen = [set() for _ in range(max_rows)]
        self.slot_line = [None] * max_slots               # per slot: the row whose logits line still holds the prompt's logits
        self.prefills = 0
        self.gen = [0] * max_slots                        # per slot: prefills so far
        self.log = []

    def context(self, row):
        return list(self.prompt[self.row_slot[row]]) + list(self.tail[row])

    def _prefill(self, slot, row, item):
        for r in range(self.max_rows):
            if self.row_slot[r] == slot:
                self.row_slot[r], self.tail[r], self.has_logits[r] = -1, [], False
        self.prompt[slot] = [int(t) for t in item.input_ids]
        self.gen[slot] += 1
        self.slot_line = [None if l == row else l for l in self.slot_line]
        self.slot_line[slot] = row
        self.row_slot[row], self.tail[row], self.has_logits[row], self.seen[row] = slot, [], True, set()

    def prefill(self, slot, row, item):
        self.prefills += 1
        self.log.append(("prefill", slot, row, len(item.input_ids)))
        self._prefill(slot, row, item)

    def prefill_batch(self, slots, rows, items):
        assert len(set(slots)) == len(slots) and len(set(rows)) == len(rows)
        assert sum(len(it.input_ids) for it in items) <= self.enc.max_tokens or len(items) == 1
        assert len(items) <= self.enc.max_seqs
        self.prefills += 1
        self.log.append(("prefill_batch", list(slots), list(rows), [len(it.input_ids) for it in items]))
        for s, r, it in zip(slots, rows, items):
            self._prefill(s, r, it)

    def row_state(self, row):
        return self.row_slot[row], len(self.tail[row])

    def slot_state(self, slot):
        return (len(self.prompt[slot]) if self.prompt[slot] else 0), self.prompt[slot] is not None and self.slot_line[slot] is not None

    def slot_generation(self, slot):
        return self.gen[slot]

    def slot_holds(self, slot, item):
        return self.prompt[slot] is not None and self.prompt[slot] == [int(t) for t in item.input_ids]

    def slot_score(self, slots, targets):
        self.log.append(("slot_score", list(slots), list(targets)))
        assert all(self.slot_state(s)[1] for s in slots)
        vals = [fake_logprob(self.prompt[s], t) for s, t in zip(slots, targets)]
        return {"logit": np.asarray([v[0] for v in vals], np.float32), "lse": np.asarray([v[1] for v in vals], np.float32),
                "top_logit": np.asarray([v[2] for v in vals], np.float32), "top_token": np.asarray([v[3] for v in vals], np.int32)}

    def truncate(self, row, length):
        assert 0 <= length <= len(self.tail[row])
        self.log.append(("truncate", row, length))
        self.tail[row], self.has_logits[row] = self.tail[row][:length], False

    def row_score(self, rows, targets):
        self.log.append(("row_score", list(rows), list(targets)))
        assert all(self.has_logits[r] for r in rows)
        vals = [fake_logprob(self.context(r), t) for r, t in zip(rows, targets)]
        return {"logit": np.asarray([v[0] for v in vals], np.float32), "lse": np.asarray([v[1] for v in vals], np.float32),
                "top_logit": np.asarray([v[2] for v in vals], np.float32), "top_token": np.asarray([v[3] for v in vals], np.int32)}

    def extend(self, slots, rows, token_lists, targets=None, seen="keep"):
        assert len(set(rows)) == len(rows) and 1 <= len(rows) <= min(self.max_rows, self.enc.max_seqs)
        assert sum(len(t) for t in token_lists) <= self.enc.max_tokens
        self.log.append(("extend", list(slots), list(rows), [list(t) for t in token_lists], seen))
        out = []
        for b, (s, r, toks) in enumerate(zip(slots, rows, token_lists)):
            assert toks and self.prompt[s] is not None
            assert self.row_slot[r] == s or not self.tail[r], "a row with a tail must continue its slot"
            if self.row_slot[r] != s:
                self.row_slot[r], self.tail[r], self.seen[r] = s, [], set()
            assert len(self.tail[r]) + len(toks) <= self.max_new and len(self.context(r)) + len(toks) <= self.max_len
            vals = []
            for j, t in enumerate(toks):
                self.tail[r].append(int(t))
                if targets is not None and targets[b][j] >= 0:
                    vals.append(fake_logprob(self.context(r), targets[b][j]))
                else:
                    vals.append((np.nan, np.nan, np.nan, -1))
            self.has_logits[r] = True
            self.slot_line = [None if l == r else l for l in self.slot_line]
            if seen == "clear":
                self.seen[r] = set()
            elif seen == "join":
                self.seen[r] |= {int(t) for t in toks}
            out.append({"logit": np.asarray([v[0] for v in vals], np.float32), "lse": np.asarray([v[1] for v in vals], np.float32),
                        "top_logit": np.asarray([v[2] for v in vals], np.float32),
                        "top_token": np.asarray([v[3] for v in vals], np.int32)})
        return out if targets is not None else None

    # greedy decoding: the next token is a function of the context (never the eos of the tests)
    def select(self, mode, groups, k, beam_scores=None, **_):
        assert k == 1 and all(len(g) == 1 for g in groups)
        toks = [[fake_logprob(self.context(g[0]), 0)[3]] for g in groups]
        assert all(self.has_logits[g[0]] for g in groups)
        return np.zeros((len(groups), 1), np.float32), np.asarray(toks, np.int32), np.zeros((len(groups), 1), np.int32)

    def step(self, slots, rows, tokens):
        self.log.append(("step", list(slots), list(rows), list(tokens)))
        for s, r, t in zip(slots, rows, tokens):
            assert self.row_slot[r] == s
            self.tail[r].append(int(t))
            self.seen[r].add(int(t))
            self.has_logits[r] = True
