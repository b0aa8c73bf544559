"""Appending given tokens to a cached prompt (vr_chat_extend) next to the routes that rebuild the prompt, on one GPU,
alternating in one process:

    python tools/chat_extend_bench.py [--reps 10]

Full dims, synthetic weights, 448 x 448 pages, random answers:
  answers      one page, A = 1 / 9 answers of 32 / 256 tokens:   score_items (A packed sequences, each with its own tower
               pass and prompt rows)  vs  score_items_shared (one prefill, token 0 from the prompt row, the rest by extend)
  marginal     k = 3 pages x A = 3 candidates of 32 tokens (the shape of marginal_selection): the same two routes
  second_turn  a second question (12 tokens) about a resident page: truncate + extend on the cached prompt  vs  a fresh
               prefill of page + first turn + question
with the largest difference between the two routes' token log-probs (logits for second_turn).

Every measurement lies between two device events (host work between them included); `--reps` alternations, median
(min - max) in milliseconds.  Prints one JSON line.  Kernel times: run it under `rocprofv3 --kernel-trace --stats` on its own."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def spread_ms(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def alternate(todo, reps):
    for _, fn in todo:
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in todo}
    last = {}
    for _ in range(reps):
        for name, fn in todo:
            t, last[name] = timed(fn)
            ms[name].append(t)
    return {name: spread_ms(v) for name, v in ms.items()}, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chat_extend_bench needs a GPU: there is no CPU fallback")
    from PIL import Image

    from visrag_amd.config import full_config
    from visrag_amd.engine import HipEncoder
    from visrag_amd.generation import HipChat, score_items, score_items_shared
    from visrag_amd.preprocess import PreparedItem, prepare_item
    from visrag_amd.synth import iter_synth_weights, synth_lm_head, synth_pages
    from visrag_amd.tokenizer import StandInTokenizer
    cfg = full_config()
    enc = HipEncoder(cfg, device=0, max_images=9, max_tokens=3328, max_seqs=9)
    enc.load_state_dict(iter_synth_weights(cfg, 0, device="cuda"))
    chat = HipChat(enc, max_len=640, max_rows=10, dim_model_base=256.0, max_slots=3, max_new=260)
    chat.load_head(synth_lm_head(cfg, 0, device="cuda"))
    tok = StandInTokenizer(cfg.vocab_size)
    pages = [Image.fromarray(p) for p in synth_pages(3, size=448, seed=0)]
    items = [prepare_item("<用户>what is shown on this page", p, tok, cfg, 2048) for p in pages]
    rng = np.random.default_rng(0)
    res = {"reps": a.reps, "device": torch.cuda.get_device_name(0), "prompt_tokens": len(items[0].input_ids), "unit": "ms, device events"}

    def lps(rs):
        return [r["token_logprobs"] for r in rs]

    for A in (1, 9):
        for n_tok in (32, 256):
            conts = [rng.integers(16, cfg.vocab_size, n_tok).tolist() for _ in range(A)]
            t, last = alternate([("score_items", lambda: lps(score_items(chat, [items[0]] * A, conts))),
                                 ("score_items_shared", lambda: lps(score_items_shared(chat, [items[0]], [conts])[0]))], a.reps)
            t["max_abs_logprob_diff"] = float(max(np.abs(x - y).max() for x, y in zip(last["score_items"], last["score_items_shared"])))
            t["speedup_median"] = round(t["score_items"]["median"] / t["score_items_shared"]["median"], 2)
            res[f"answers{A}_tokens{n_tok}"] = t
            print(json.dumps({f"answers{A}_tokens{n_tok}": t}), file=sys.stderr, flush=True)

    cands = [rng.integers(16, cfg.vocab_size, 32).tolist() for _ in range(3)]
    t, last = alternate([("score_items", lambda: lps(score_items(chat, [it for _ in cands for it in items], [c for c in cands for _ in items]))),
                         ("score_items_shared", lambda: [r["token_logprobs"] for rs in score_items_shared(chat, items, [cands] * 3) for r in rs])],
                        a.reps)
    plain = {(ai, i): last["score_items"][ai * 3 + i] for ai in range(3) for i in range(3)}
    shared = {(ai, i): last["score_items_shared"][i * 3 + ai] for ai in range(3) for i in range(3)}
    t["max_abs_logprob_diff"] = float(max(np.abs(plain[k] - shared[k]).max() for k in plain))
    t["speedup_median"] = round(t["score_items"]["median"] / t["score_items_shared"]["median"], 2)
    res["marginal_pages3_answers3_tokens32"] = t
    print(json.dumps({"marginal": t}), file=sys.stderr, flush=True)

    first = rng.integers(16, cfg.vocab_size, 20).tolist()           # the first turn's answer, resident in the row's tail
    question = rng.integers(16, cfg.vocab_size, 12).tolist()
    whole = PreparedItem(input_ids=list(items[0].input_ids) + first + question, image_bound=items[0].image_bound, slices=items[0].slices)
    chat.prefill(0, 0, items[0])
    chat.extend([0], [0], [first])

    def resident():
        chat.truncate(0, len(first))
        chat.extend([0], [0], [question], seen="clear")
        return chat.logits(0)

    def fresh():
        chat.prefill(1, 1, whole)
        return chat.logits(1)

    t, last = alternate([("fresh_prefill", fresh), ("extend_resident", resident)], a.reps)
    t["max_abs_logit_diff"] = float(np.abs(last["fresh_prefill"] - last["extend_resident"]).max())
    t["max_abs_logit"] = float(np.abs(last["fresh_prefill"]).max())
    t["speedup_median"] = round(t["fresh_prefill"]["median"] / t["extend_resident"]["median"], 2)
    res["second_turn_tokens12"] = t
    chat.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
