"""Does GemmArgs::warm pay, and what does it cost its carrier?  (tools/r6/mall_probe.py showed that a weight matrix READ by any
launch beforehand takes the HBM latency out of the half-height GEMM that uses it next; here the read is the cheap form: the
MFMA-bound launch in front of the projection requests one dword per line of the projection's matrix while it runs.)

Trains over 40 weight buffers, decoder shapes (T = 2176 rows), carriers' own weights cycling too:
    o:     [q|k|v + RoPE 2176 x 6912 x 2304 (variant 12, epilogue 5)  ;  o    2176 x 2304 x 2304 (variant 14) on W_i]
    down:  [gate|up + SwiGLU 2176 x 11520 x 2304 (variant 12, epilogue 4) ;  down 2176 x 2304 x 5760 (variant 14) on W_i]
each as: the projection alone (cold), the carrier alone without / with warm = W_i, the pair without / with.

    python tools/warm_probe.py [--lib PATH] [--label TEXT]

--lib: another build of the library (a tagged build with -DVR_WARM_LINE=64 requests one dword per 64 bytes instead of 128:
`python -m visrag_amd.build --tag warm64 -DVR_WARM_LINE=64`); --label goes into every output line."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from visrag_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--label", default="128 bytes per request")
args = ap.parse_args()
lib = _lib.load(args.lib)
s = torch.cuda.current_stream().cuda_stream
T, TP, POOL, E = 2176, 2304, 40, 2304


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def bf16(rows, cols, scale=1.0):
    return (torch.randn((rows, cols), device="cuda") * scale).to(torch.bfloat16)


pos = (torch.arange(T, device="cuda", dtype=torch.int32) % 68)
inv = 1.0 / (10000.0 ** (torch.arange(0, 64, 2, dtype=torch.float64) / 64))
fr = torch.outer(torch.arange(68, dtype=torch.float64), inv)
table = torch.cat([torch.cos(fr), torch.sin(fr)], dim=1).float().cuda()

for name, cN, epi, K in (("o", 3 * E, 5, E), ("down", 11520, 4, 5760)):
    xn = bf16(TP, E)                                          # the carrier's A rows (the norm's output)
    Wc = [bf16(cN, E, 0.05) for _ in range(POOL)]             # q|k|v / interleaved gate|up weights
    c_out = torch.zeros((TP, cN // 2 if epi == 4 else cN), device="cuda", dtype=torch.bfloat16)
    A = bf16(TP, K)                                           # the projection's A rows
    Wp = [bf16(E, K, 0.05) for _ in range(POOL)]              # o / down weights
    h = torch.zeros((TP, E), device="cuda", dtype=torch.float32)

    def carrier(i, warm):
        w = Wp[i % POOL] if warm else None
        _lib.check(lib.vr_op_gemm_warm(0, P(xn), E, P(Wc[i % POOL]), E, T, cN, E, epi, None, None, 1.0, P(c_out), c_out.stride(0),
                                       P(pos) if epi == 5 else None, P(table) if epi == 5 else None, 2 * E if epi == 5 else 0, 12, None,
                                       P(w), C.c_uint64(w.numel() * 2 if warm else 0), s))

    def proj(i):
        _lib.check(lib.vr_op_gemm(0, P(A), K, P(Wp[i % POOL]), K, T, E, K, 3, None, P(h), 0.0, P(h), E, None, None, 0, 14, s))

    def train(fn, n=3 * POOL):
        fn(0)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            fn(i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    r = {"case": name, "requests": args.label}
    for rep in range(2):                                      # (the second pass is the one to read: clocks and caches settled)
        r["proj_cold_us"] = round(train(proj), 1)
        r["carrier_us"] = round(train(lambda i: carrier(i, False)), 1)
        r["carrier_warm_us"] = round(train(lambda i: carrier(i, True)), 1)
        r["pair_us"] = round(train(lambda i: (carrier(i, False), proj(i))), 1)
        r["pair_warm_us"] = round(train(lambda i: (carrier(i, True), proj(i))), 1)
    r["carrier_pays_us"] = round(r["carrier_warm_us"] - r["carrier_us"], 1)
    r["proj_after_carrier_us"] = round(r["pair_us"] - r["carrier_us"], 1)
    r["proj_after_warm_us"] = round(r["pair_warm_us"] - r["carrier_warm_us"], 1)
    r["pair_saves_us"] = round(r["pair_us"] - r["pair_warm_us"], 1)
    print(json.dumps(r), flush=True)
    del Wc, Wp
    torch.cuda.empty_cache()
