"""MiniCPM-V 2.0 answer generation at production dims (synthetic weights): one A4 page (source + 8 slices at this aspect
ratio: 608 prompt tokens), beam search with 3 beams, 20 new tokens.  Prints prefill ms, ms per decode step, bytes per step
and the fraction of the HBM peak (8 TB/s) as one JSON line.  Measured on MI355X: prefill 23.3 ms, 3.34 ms per 3-beam step
(0.91 ms weight-stream floor at 6 TB/s), 0.23 ms per beam selection.

    python tools/chat_bench.py [--steps 20] [--beams 3]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--beams", type=int, default=3)
    a = ap.parse_args()
    cfg = full_config()
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
