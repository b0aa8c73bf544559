"""-m gpu: the bf16 attention kernels (attention.hip's tiled forms, attention_small.hip, attention_w.hip) on the guarded arena of
tests/attention_arena.py.  q, k and v are views into ONE allocation, no cu starts at 0, every row has pitch columns, and every
cell a launch has no business reading is a guard: 16 rows in front, 256 behind, 8 columns around each operand, the stale cache
rows outside the ranges of the decode form.  Each case first asserts the kernel it reaches (vr_op_attention_route — the switches
at max_q 64 | 65, 128 | 129, 80 | 81 and 223 | 224, 256 | 257, 447 | 448 all have a case on either side), then launches three
times through vr_op_attention_ex, with the guards zero, NaN, and the largest finite bf16:

  (a) the cells a launch must write are within rtol = atol = 2e-2 of fp64 attention of the (bf16) data — the bar
      tests/test_gpu_ops.py states — and lse within LSE_ATOL (tests/test_gpu_launch_args.py);
  (b) the nan and huge runs are BIT-identical to the clean one, out and lse: no guard cell reaches a result, not even as 0 * x;
  (c) every other cell of out and lse — the rows around an item, out's pitch columns, items without keys — still holds the
      sentinel's bits;
  (d) the arena itself is bitwise what it was.

The contract is written down at vr_op_attention in include/visrag_hip.h.  Its one exception, also there: the head_dim 72 route
of attention_w.hip stages a head's 72 columns as 80 and multiplies the extra 8 by zero, so k[row][H .. H+8) and v[row][H .. H+8)
(H = heads * 72: the 8 cells behind the LAST head; the other heads' 8 are the next head's data) of every key row of an item
must be finite.  On that route (the 72w_* cases) those cells hold the `huge` pattern in the nan run too; NaN goes everywhere else.
tests/test_cpu_attention_arena.py shows, on the host and at these shapes, that a kernel wrong by one key, one 16-byte column
chunk or one causal position would fail (a) or (b).

First run on an MI355X, worst |got - ref| / (atol + rtol |ref|) per case (out; lse where the case has one) — all three runs of
a case give the same bits, so one figure each.  All 29 cases passed (a) to (d) as the kernels stood: no finding.

    lens            head_dim 64   64 causal   72      80            case                 out     lse
    [64, 1, 63]     0.126         0.132       0.128   0.128         tiled72 [223]        0.173
    [65, 64]        0.136         0.124       0.130   0.128         tiled72 [257, 30]    0.177
    [128, 127]      0.221         0.196       0.153   0.183         hd128 resampler      0.208
    [129, 65, 1]    0.226         0.181       0.172   0.189         hd128 segments       0.237
    [129, 65, 1] causal                       0.131   0.164         small / causal       0.136 / 0.160
                                                                    72w [224]            0.903
                                                                    72w [256, 224, 1]    0.861
                                                                    72w [448, 33]        0.780
                                                                    decode shared q      0.131   0.001
                                                                    decode batched       0.145   0.000

The 72w figures are not a defect of that route's isolation: attention_w.hip multiplies q by scale * log2(e) and rounds it to bf16
a SECOND time before the score MFMAs (the engine hands it q already scaled, with one rounding: q_prescaled), a logit error of
2^-9 |q| |k| per term that grows with keys of size KEY_GAIN = 4 — test_vit_pair_scaled_q_columns_then_prescaled_attention
(test_gpu_launch_args.py) describes it.  The kernels have no atomics and a fixed summation order: the figures repeat.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import attention_arena as A  # noqa: E402
from tests.gpu_util import (ROUTE_72W, ROUTE_SMALL, attention_route_of, from_bf16_bits, op_attention_ex,  # noqa: E402
                            route_tiled)

DEV = "cuda:0"
CASES = A.cases()


def _route_code(route):
    return {A.SMALL: ROUTE_SMALL, A.W72: ROUTE_72W}.get(route) if isinstance(route, str) else route_tiled(*route[1:])


def _bits16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _i32(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.int32)).to(DEV) if x is not None else None


def _launch(c, a, fill, cu_q, cu_kv, kv_end, q_in, check_route):
    """one launch on the arena filled with `fill`: (out bits, lse values or None, the arena's bits after the call)"""
    arena = from_bf16_bits(a.filled(fill), DEV)
    q = arena[c.q_row0:, c.q_col:c.q_col + c.Wq]
    k = arena[:, c.k_col:c.k_col + c.Wkv]
    v = arena[:, c.v_col:c.v_col + c.Wkv]
    out_h, lse_h = a.out_sentinels()
    out = from_bf16_bits(out_h, DEV)
    lse = torch.from_numpy(lse_h).to(DEV) if c.lse else None
    kw = dict(B=c.B, ldq=c.ldq, kv_group=c.kv_group, kv_end=kv_end, q_in_rows=q_in, q_head_stride=c.q_head_stride, lse=lse)
    if check_route:
        assert attention_route_of(q, k, v, out, cu_q, cu_kv, c.heads, c.hd, c.max_q, c.causal, c.q_shared, c.scale, **kw) == \
            _route_code(c.route), "the case does not reach the kernel it is meant for"
    op_attention_ex(q, k, v, out, cu_q, cu_kv, c.heads, c.hd, c.max_q, c.causal, c.q_shared, c.scale, **kw)
    return _bits16(out), (lse.cpu().numpy() if c.lse else None), _bits16(arena)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_attention_reads_and_writes_only_its_own_cells(c):
    a = A.arena_of(c.name)
    ref, ref_lse = A.reference_of(c.name)
    om, lm = a.out_mask, a.lse_mask
    assert np.median(np.abs(ref[om[:, :c.Wo]])) > 0.1                       # outputs of the size of v: the tolerance means something
    cu_q = _i32(c.cu_q)
    cu_kv = cu_q if c.same_cu else _i32(c.cu_kv)
    kv_end, q_in = _i32(c.kv_end), _i32(c.q_in_rows)
    runs = {}
    for fill in A.FILLS:
        out, lse, after = _launch(c, a, fill, cu_q, cu_kv, kv_end, q_in, check_route=fill == "clean")
        assert np.array_equal(after, a.filled(fill)), f"(d) {fill}: the launch wrote into its inputs"
        runs[fill] = (out, lse)
    sent_out, sent_lse = a.out_sentinels()
    out, lse = runs["clean"]
    got = A.from_bits(out).astype(np.float64)[:, :c.Wo]
    ratio = A.worst_ratio(got, ref)
    ratio_lse = A.worst_ratio(lse.astype(np.float64), np.where(lm, ref_lse, np.nan), rtol=0, atol=A.LSE_ATOL) if c.lse else 0.0
    print(f"\n[isolation] {c.name:28s} worst |got - ref| / tol: out {ratio:.3f}" + (f"  lse {ratio_lse:.3f}" if c.lse else ""))
    for fill, (o, l) in runs.items():
        # (c) nothing outside the cells a launch must write has changed
        assert np.array_equal(o[~om], sent_out[~om]), f"(c) {fill}: out cells outside the items' rows x columns were written"
        if c.lse:
            assert np.array_equal(l.view(np.uint32)[~lm], sent_lse.view(np.uint32)[~lm]), f"(c) {fill}: lse rows of no item written"
            assert not np.any(l.view(np.uint32)[lm] == sent_lse.view(np.uint32)[lm]), f"{fill}: an lse cell of an item was not written"
        # (b) no guard cell reaches a result
        if fill != "clean":
            diff = np.argwhere(o != out)
            assert diff.size == 0, f"(b) {fill}: {len(diff)} out cells differ from the clean run, first at (row, col) {diff[0]}"
            if c.lse:
                assert np.array_equal(l.view(np.uint32), lse.view(np.uint32)), f"(b) {fill}: lse differs from the clean run"
    # (a) the values
    assert ratio <= 1.0, f"(a) out misses fp64 by {ratio:.3f} x the tolerance"
    assert ratio_lse <= 1.0, f"(a) lse misses fp64 by {ratio_lse:.3f} x the tolerance"
