"""MiniCPM-V 2.0 answer generation at production dims (synthetic weights): one A4 page (source + 8 slices at this aspect
ratio: 608 prompt tokens), beam search with 3 beams, 20 new tokens.  Prints prefill ms, ms per decode step, bytes per step
and the fraction of the HBM peak (8 TB/s) as one JSON line.  Measured on MI355X: prefill 23.3 ms, 3.34 ms per 3-beam step
(0.91 ms weight-stream floor at 6 TB/s), 0.23 ms per beam selection.

    python tools/chat_bench.py [--steps 20] [--beams 3]

--pages K (weighted selection over the top-K pages, K x beams <= 16 rows): K different A4 pages, in one process — K serial
vr_chat_prefill calls, then one vr_chat_prefill_batch of the same pages (each timed --reps times after a warm-up: median,
and max - min as the run-to-run spread), then the lockstep decode steps of all K x beams rows.

    python tools/chat_bench.py --pages 3
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from visrag_amd.config import full_config  # noqa: E402
from visrag_amd.engine import HipEncoder  # noqa: E402
from visrag_amd.generation import BEAM, HipChat  # noqa: E402
from visrag_amd.preprocess import prepare_item  # noqa: E402
from visrag_amd.synth import iter_synth_weights, synth_lm_head, synth_pages  # noqa: E402
from visrag_amd.tokenizer import StandInTokenizer  # noqa: E402

HBM_PEAK = 8.0e12


def a4_page(seed):
    page = np.concatenate([synth_pages(1, size=448, seed=3 * seed + s)[0] for s in range(3)], axis=0)      # 1344 x 448: a tall page
    return Image.fromarray(np.asarray(Image.fromarray(page).resize((1190, 1684))))                          # A4 at 144 dpi


def bench_pages(cfg, a):
    K, nb = a.pages, a.beams
    if K * nb > 16:
        raise SystemExit("--pages x --beams must not exceed 16 rows")
    enc = HipEncoder(cfg, device=0, max_images=10 * K, max_tokens=704 * K, max_seqs=K)
    enc.load_state_dict(iter_synth_weights(cfg, 0, device="cuda"))
    chat = HipChat(enc, max_len=768, max_rows=K * nb, dim_model_base=256.0, max_slots=K, max_new=a.steps + 2)
    chat.load_head(synth_lm_head(cfg, 0, device="cuda"))
    tok = StandInTokenizer(cfg.vocab_size)
    items = [prepare_item("<用户>What is the title of this page?", a4_page(k), tok, cfg, 2048) for k in range(K)]
    slots, first = list(range(K)), [k * nb for k in range(K)]

    def serial():
        for k in range(K):
            chat.prefill(k, first[k], items[k])

    def batched():
        chat.prefill_batch(slots, first, items)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), float(max(ms) - min(ms)), ms

    s_med, s_spread, s_all = timed(serial)
    b_med, b_spread, b_all = timed(batched)
    s2_med, s2_spread, s2_all = timed(serial)              # the serial path again: drift over the process
    batched()
    rows = list(range(K * nb))
    for k in range(K):
        if nb > 1:
            chat.reorder(rows[k * nb + 1:(k + 1) * nb], [k * nb] * (nb - 1))
    sl = [r // nb for r in rows]
    chat.step(sl, rows, [7] * len(rows))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        chat.step(sl, rows, [(17 + 31 * i + r) % cfg.vocab_size for r in rows])
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / a.steps
    r2 = lambda v: [round(x, 2) for x in v]
    print(json.dumps({"pages": K, "beams": nb, "prompt_tokens": [len(it.input_ids) for it in items], "reps": a.reps,
                      "serial_prefill_ms": round(s_med, 2), "serial_spread_ms": round(s_spread, 2), "serial_all_ms": r2(s_all),
                      "batched_prefill_ms": round(b_med, 2), "batched_spread_ms": round(b_spread, 2), "batched_all_ms": r2(b_all),
                      "serial_again_ms": round(s2_med, 2), "serial_again_spread_ms": round(s2_spread, 2),
                      "step_ms": round(step_ms, 3), "steps": a.steps,
                      "request_ms_serial": round(s_med + a.steps * step_ms, 2), "request_ms_batched": round(b_med + a.steps * step_ms, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--beams", type=int, default=3)
    ap.add_argument("--pages", type=int, default=0, help="K > 0: serial against batched prefill of K pages, then lockstep steps")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    cfg = full_config()
    if a.pages > 0:
        return bench_pages(cfg, a)
    enc = HipEncoder(cfg, device=0, max_images=10, max_tokens=1024, max_seqs=2)
    enc.load_state_dict(iter_synth_weights(cfg, 0, device="cuda"))
    chat = HipChat(enc, max_len=1024, max_rows=a.beams, dim_model_base=256.0)
    chat.load_head(synth_lm_head(cfg, 0, device="cuda"))
    page = np.concatenate([synth_pages(1, size=448, seed=s)[0] for s in range(3)], axis=0)      # 1344 x 448: a tall page
    page = np.asarray(Image.fromarray(page).resize((1190, 1684)))                                 # A4 at 144 dpi
    item = prepare_item("<用户>What is the title of this page?", Image.fromarray(page), StandInTokenizer(cfg.vocab_size), cfg, 2048)
    rows = list(range(a.beams))

    def prefill():
        chat.prefill(0, 0, item)
        torch.cuda.synchronize()

    prefill()
    t0 = time.perf_counter()
    prefill()
    prefill_ms = (time.perf_counter() - t0) * 1e3
    chat.reorder(rows[1:], [0] * (a.beams - 1))
    toks = [7] * a.beams
    chat.step([0] * a.beams, rows, toks)                 # warm-up step
    torch.cuda.synchronize()
    n = min(a.steps, chat.max_len - len(item.input_ids) - 2)
    t0 = time.perf_counter()
    for i in range(n):
        chat.step([0] * a.beams, rows, [(17 + 31 * i + r) % cfg.vocab_size for r in rows])
    torch.cuda.synchronize()
    step_ms = (time.perf_counter() - t0) * 1e3 / n
    t0 = time.perf_counter()
    for i in range(n):
        chat.select(BEAM, [rows], 2 * a.beams, [0.0] * a.beams, repetition_penalty=1.2)
    select_ms = (time.perf_counter() - t0) * 1e3 / n
    E, I, L, V = cfg.hidden_size, cfg.intermediate_size, cfg.num_layers, cfg.vocab_size
    weights = 2.0 * (L * (4 * E * E + 3 * E * I) + V * E)
    kv = 2.0 * L * 2 * len(item.input_ids) * E
    bytes_step = weights + kv
    print(json.dumps({"prompt_tokens": len(item.input_ids), "beams": a.beams, "prefill_ms": round(prefill_ms, 2),
                      "step_ms": round(step_ms, 3), "select_ms": round(select_ms, 3), "bytes_per_step": bytes_step,
                      "hbm_fraction": round(bytes_step / (step_ms * 1e-3) / HBM_PEAK, 3),
                      "weight_floor_ms_at_6TBps": round(weights / 6e12 * 1e3, 3)}))


if __name__ == "__main__":
    main()
