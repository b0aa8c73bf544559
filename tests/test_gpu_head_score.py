"""The fused scoring head at op level (vr_op_head_score, csrc/head_score.hip) against the fp64 reference of
tests/head_score_ref.py, on inputs generated on the device.

Bars (none derived from the code under test).  bound[m][v] = K * 2^-24 * sum_k |a_mk * w_vk| covers fp32 accumulation of K
exact bf16 x bf16 products (gamma_K to first order):
  |x_t - ref| <= bound at the target;  top_x within bound of the reference maximum;
  |lse - ref| <= max_v bound + 2e-5: LSE is 1-Lipschitz in the sup-norm of the logits, and 2e-5 covers fp32 exp / log and
  the hierarchical sum (a few hundred roundings of 6e-8);
  top_id identical on every row: planted rows carry a top-two margin above twice the bound (asserted from the reference),
  tie rows hold exact dyadic logits, where the tie rule (lowest id) decides."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import head_score_ref as R  # noqa: E402
from tests.gpu_util import P  # noqa: E402
from visrag_amd import _lib  # noqa: E402

DEV = "cuda:0"
GUARD = 8
SENT_F, SENT_I = -12345.5, -54321
SHAPES = [(1, 1000, 256), (255, 1000, 256), (256, 1000, 256), (257, 1000, 256),      # row-tile edges, V % 256 != 0
          (5, 122753, 256),                                                          # 480 vocab tiles, 129 valid columns in the last
          (64, 1000, 2304),                                                          # the model's K
          (300, 2048, 256)]                                                          # no tail tile
LSE_SLACK = 2e-5


def _run(case):
    M, V, K = case["M"], case["V"], case["K"]
    tgt = torch.from_numpy(case["target"]).to(DEV)
    outs = [torch.full((M + GUARD,), SENT_F, dtype=torch.float32, device=DEV) for _ in range(3)]
    tok = torch.full((M + GUARD,), SENT_I, dtype=torch.int32, device=DEV)
    _lib.check(_lib.load().vr_op_head_score(0, P(case["A"]), K, P(case["W"]), K, M, V, K, P(tgt), P(outs[0]), P(outs[1]), P(outs[2]),
                                            P(tok), None), "vr_op_head_score")
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs] + [tok.cpu().numpy()]


@pytest.mark.parametrize("M,V,K", SHAPES)
def test_head_score_against_fp64(M, V, K):
    case = R.make_case(M, V, K, DEV)
    ref = R.head_score_ref(case["A"][:M], case["W"][:V], case["target"])
    x_t, lse, top_x, top_id = _run(case)
    # isolation: guard words behind entry M, the inputs (canary rows included) untouched, a second run bit-identical
    for o in (x_t, lse, top_x):
        assert (o[M:] == np.float32(SENT_F)).all()
    assert (top_id[M:] == SENT_I).all()
    again = _run(case)
    for a, b in zip((x_t, lse, top_x, top_id), again):
        assert a.tobytes() == b.tobytes()
    Mp, Vp = R.pad_to(M), R.pad_to(V)
    assert bool(torch.isnan(case["A"][Mp:].float()).all()) and bool(torch.isnan(case["W"][Vp:].float()).all())
    x_t, lse, top_x, top_id = x_t[:M], lse[:M], top_x[:M], top_id[:M]
    assert np.isfinite(x_t).all() and np.isfinite(lse).all() and np.isfinite(top_x).all()

    e_t = np.abs(x_t - ref["x_t"])
    e_lse = np.abs(lse - ref["lse"])
    e_top = np.abs(top_x - ref["top_x"])
    print(f"({M}, {V}, {K}): max |x_t err| {e_t.max():.3e} (bound {ref['bound_t'].max():.3e}), max |lse err| {e_lse.max():.3e} "
          f"(max bound {ref['bound_max'].max():.3e}), lse err - bound: {np.max(e_lse - ref['bound_max']):.3e}, "
          f"max |top err| {e_top.max():.3e}")
    assert (e_t <= ref["bound_t"]).all(), np.nonzero(e_t > ref["bound_t"])
    assert (e_lse <= ref["bound_max"] + LSE_SLACK).all(), np.nonzero(e_lse > ref["bound_max"] + LSE_SLACK)
    assert (e_top <= ref["bound_top"]).all()
    # every row's argmax: decided by margin (planted) or by the tie rule (exact logits)
    margin = ref["top_x"] - ref["second"]
    for m, k in enumerate(case["kinds"]):
        if k in ("all_equal", "tie_tiles", "tie_waves"):
            assert margin[m] == 0.0
        else:
            assert margin[m] > 2 * ref["bound_max"][m], (m, k)
    assert np.array_equal(top_id.astype(np.int64), ref["top_id"])

    kinds = case["kinds"]
    if "all_negative" in kinds:
        m = kinds.index("all_negative")
        assert ref["top_x"][m] <= -20 and lse[m] < -20             # the 24 pad columns (junk weights) did not count
        m = kinds.index("spike80")
        assert margin[m] >= 80 and abs(float(lse[m]) - float(top_x[m])) <= 1e-6
        m = kinds.index("magnitude300")
        assert 250 < top_x[m] < 400 and abs(lse[m] - top_x[m]) < 1e-3
        m = kinds.index("all_equal")
        assert top_id[m] == 0 and x_t[m] == 1.5 and top_x[m] == 1.5 and abs(lse[m] - (1.5 + np.log(V))) <= LSE_SLACK
        assert top_id[kinds.index("tie_tiles")] == R.TIE_A[0] and top_id[kinds.index("tie_waves")] == R.TIE_B[0]


def test_head_score_argument_errors():
    case = R.make_case(4, 1000, 256, DEV)
    lib = _lib.load()
    tgt = torch.from_numpy(case["target"]).to(DEV)
    o = torch.full((4 + GUARD,), SENT_F, dtype=torch.float32, device=DEV)
    t = torch.full((4 + GUARD,), SENT_I, dtype=torch.int32, device=DEV)
    call = lambda A, M, V, K: lib.vr_op_head_score(0, A, K, P(case["W"]), 256, M, V, K, P(tgt), P(o), P(o), P(o), P(t), None)  # noqa: E731
    assert call(None, 4, 1000, 256) == 1
    assert call(P(case["A"]), 0, 1000, 256) == 1
    assert call(P(case["A"]), 4, 0, 256) == 1
    assert call(P(case["A"]), 4, 1000, 200) == 2                  # K not a multiple of 64: the launcher refuses
    torch.cuda.synchronize()
    assert (o == SENT_F).all() and (t == SENT_I).all()
