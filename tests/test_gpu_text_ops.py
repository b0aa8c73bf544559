"""-m gpu: the kernels of the fp32 text path (csrc/hp_text.hip) and the encode glue kernels (csrc/misc.hip,
csrc/patch_embed.hip, csrc/norm.hip), one launch each through the vr_op_* entries, against the float64 references of
tests/text_ops_ref.py at the smallest shapes at which each kernel can still go wrong.  The bars are stated there, next to the
case tables; where a bar is a multiple of the float32 restatement's error, that error is computed here from the reference
alone and printed.  Outputs are the caller's buffers inside guard rows (and guard columns where a pitch leaves room),
prefilled with a sentinel; "not written" is a bitwise comparison with it.  A shape a launcher refuses comes back as status 2
(VR_ERR_HIP) with nothing written."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import text_ops_ref as R  # noqa: E402
from tests.gpu_util import (op_convert, op_embed_gather, op_gemm_ex, op_norm_ex, op_patch_embed, op_planes_sum, op_pool,  # noqa: E402
                            op_text_attention, op_text_rmsnorm_split, op_text_rope, op_text_swiglu_split)
from visrag_amd._lib import VisragHipError  # noqa: E402

DEV = "cuda:0"
EPI_F32 = 2
G = 3                                                     # guard rows in front of and behind every output
SENT = {torch.float32: -77.25, torch.bfloat16: 7.0, torch.int32: -7}       # exact in their formats, far from every output here
_BITS = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.int32: torch.int32}


def _dev(x, dtype=None):
    t = torch.from_numpy(np.array(x))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _dev_bf16(x):
    """bf16-valued float32 numpy -> bf16 on the device (exact)"""
    return torch.from_numpy(np.array(x, np.float32)).to(torch.bfloat16).to(DEV)


def _guarded(rows, cols, dtype):
    """(whole, inner): a sentinel-filled [G + rows + G][cols] buffer and the view of its middle rows"""
    whole = torch.full((rows + 2 * G, cols), SENT[dtype], dtype=dtype, device=DEV)
    return whole, whole[G:G + rows]


def _untouched(t):
    if t.numel() == 0:
        return True
    bits = t.contiguous().view(_BITS[t.dtype])
    want = torch.full((1,), SENT[t.dtype], dtype=t.dtype).view(bits.dtype).item()
    return bool((bits == want).all())


def _guards_kept(whole, rows):
    return _untouched(whole[:G]) and _untouched(whole[G + rows:])


def _f64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _bits(t):
    return t.contiguous().view(_BITS[t.dtype]).cpu().numpy()


def _refused(fn, *outs, launcher):
    with pytest.raises(VisragHipError, match=r"\(status 2\): " + launcher + r"\("):
        fn()
    torch.cuda.synchronize()
    for o in outs:
        assert _untouched(o)


# ------------------------------------------------------------------------ rmsnorm_split ---
def _rmsnorm_split(x, w, rows, dim, product_layout):
    """hi, lo (and the guarded buffers) of one launch: lo right behind the `rows` hi rows in ONE buffer (the encode path's
    layout), or in a buffer of its own"""
    if product_layout:
        whole, inner = _guarded(2 * rows, dim, torch.bfloat16)
        hi, lo = inner[:rows], inner[rows:]
        op_text_rmsnorm_split(x, rows, dim, w, R.RMS_EPS, hi, lo)
        assert _guards_kept(whole, 2 * rows)
    else:
        wh, hi = _guarded(rows, dim, torch.bfloat16)
        wl, lo = _guarded(rows, dim, torch.bfloat16)
        op_text_rmsnorm_split(x, rows, dim, w, R.RMS_EPS, hi, lo)
        assert _guards_kept(wh, rows) and _guards_kept(wl, rows)
    return hi, lo


@pytest.mark.parametrize("dim", R.RMSNORM_DIMS)
@pytest.mark.parametrize("rows", R.RMSNORM_ROWS)
def test_rmsnorm_split(rows, dim):
    """(a) hi + lo within 1.25 * 2^-16 of the float64 RMSNorm, (b) hi is the rounding of the value, (c) the encode path's layout
    and split buffers give the same bits; an all-zero row gives zeros, a row with one huge element stays finite"""
    X, w = R.rmsnorm_inputs(dim)
    wd = _dev(w)
    for x in ([X[:rows]] if rows > 1 else [X[0:1], X[1:2], X[2:3]]):
        ref = R.rms_norm(x, w, R.RMS_EPS)
        xd = _dev(x)
        hi, lo = _rmsnorm_split(xd, wd, rows, dim, True)
        hi2, lo2 = _rmsnorm_split(xd, wd, rows, dim, False)
        err, bar, ratio = R.split_errors(_f64(hi), _f64(lo), ref)
        rel = float(np.max(err[ref != 0] / np.abs(ref[ref != 0]), initial=0.0))
        print(f"rmsnorm_split rows {rows} dim {dim}: |hi + lo - ref| / |ref| <= {rel:.3g} (bar {R.SPLIT_REL:.3g}), |lo| / (2^-8 |hi|) <= {ratio:.3f}")
        assert (err <= bar).all()
        assert ratio <= 1.0
        np.testing.assert_array_equal(_bits(hi), _bits(hi2))
        np.testing.assert_array_equal(_bits(lo), _bits(lo2))
        zero = ~x.any(axis=1)
        assert (_f64(hi)[zero] == 0).all() and (_f64(lo)[zero] == 0).all()


@pytest.mark.parametrize("dim", R.RMSNORM_REFUSED)
def test_rmsnorm_split_refuses(dim):
    x, w = _dev(np.ones((4, dim), np.float32)), _dev(np.ones(dim, np.float32))
    wh, hi = _guarded(4, dim, torch.bfloat16)
    wl, lo = _guarded(4, dim, torch.bfloat16)
    _refused(lambda: op_text_rmsnorm_split(x, 4, dim, w, R.RMS_EPS, hi, lo), wh, wl, launcher="launch_rmsnorm_split")


# --------------------------------------------------------------------------------- rope ---
@pytest.mark.parametrize("E", R.ROPE_E)
def test_rope(E):
    """in place on rows of pitch 3 E + 8: q and k heads rotated to 4 fp32 ulps (at the magnitude of the two products and their
    sum) of the float64 rotation by the same fp32 table entries; rows at position 0, the v columns and the pad columns keep
    their bits"""
    qkv, pos, table = R.rope_inputs(E)
    T, ld = qkv.shape
    whole, inner = _guarded(T, ld, torch.float32)
    inner.copy_(_dev(qkv))
    op_text_rope(inner, T, ld, 2 * E, _dev(pos), _dev(table))
    assert _guards_kept(whole, T)
    got = inner.cpu().numpy()
    ref, mag = R.rope_ref(qkv, pos, table, 2 * E)
    np.testing.assert_array_equal(got[:, 2 * E:].view(np.int32), qkv[:, 2 * E:].view(np.int32))
    rows0 = pos == 0
    np.testing.assert_array_equal(got[rows0].view(np.int32), qkv[rows0].view(np.int32))
    ulps = np.abs(got.astype(np.float64) - ref) / R.ulp_f32(mag)
    print(f"rope E {E}: within {ulps.max():.2f} fp32 ulps of the float64 rotation")
    assert ulps.max() <= R.ROPE_ULPS
    # the rotation happened: the rotated rows moved by far more than that
    assert np.abs(got[~rows0, :2 * E] - qkv[~rows0, :2 * E]).mean() > 0.1


def test_rope_refuses():
    qkv, pos, table = R.rope_inputs(64)
    whole, inner = _guarded(5, qkv.shape[1], torch.float32)
    _refused(lambda: op_text_rope(inner, 5, qkv.shape[1], 96, _dev(pos), _dev(table)), whole, launcher="launch_rope_f32")


# ---------------------------------------------------------------------------- attention ---
def _attn(qkv, heads, lens, scale=0.125):
    """out f32 [T][E] of one launch; the input carries G readable rows behind its last token, the output guard rows"""
    T, ld = qkv.shape
    E = 64 * heads
    src = torch.zeros((T + G, ld), dtype=torch.float32, device=DEV)
    src[:T] = _dev(qkv)
    off = _dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
    whole, out = _guarded(T, E, torch.float32)
    op_text_attention(src, ld, E, off, len(lens), T, heads, scale, out)
    assert _guards_kept(whole, T)
    return out.cpu().numpy()


def _attn_check(name, qkv, heads, lens):
    ref = R.attn_ref(qkv, heads, lens, 0.125)
    bar, e32 = R.restatement_bar(ref, R.attn_ref(qkv, heads, lens, 0.125, np.float32))
    got = _attn(qkv, heads, lens)
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print(f"attn_f32 {name}: error {err:.3g}, float32 restatement {e32:.3g}, bar {bar:.3g}")
    assert np.isfinite(got).all()
    assert err <= bar
    return got


@pytest.mark.parametrize("gain", R.ATTN_QK_GAIN)
@pytest.mark.parametrize("lens", R.ATTN_SEQS, ids=lambda l: "-".join(map(str, l)))
@pytest.mark.parametrize("heads", R.ATTN_HEADS)
def test_attention(heads, lens, gain):
    """within 8 x the float32 restatement's error of the float64 causal attention; the first token of every sequence returns
    its own v row bit for bit (p = 1, l = 1)"""
    qkv = R.attn_inputs(heads, lens, gain)
    got = _attn_check(f"heads {heads} lens {lens} gain {gain}", qkv, heads, lens)
    first = np.concatenate([[0], np.cumsum(lens)])[:-1]
    E = 64 * heads
    np.testing.assert_array_equal(got[first].view(np.int32), qkv[first, 2 * E:3 * E].view(np.int32))


@pytest.mark.parametrize("case", R.ATTN_SCORE_CASES)
def test_attention_running_maximum(case):
    """the online softmax's rescale between the rounds of 64 keys: a dominant key in the second and in the third round, scores
    rising from round to round, all scores below -60, a huge first key — the same bar"""
    _attn_check(case, R.attn_score_case(case), 1, (200,))


@pytest.mark.parametrize("heads", R.ATTN_HEADS)
def test_attention_sequences_do_not_see_each_other(heads):
    lens = (63, 1, 66)
    qkv = R.attn_inputs(heads, lens)
    base = _attn(qkv, heads, lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    for b in range(len(lens)):
        other = qkv.copy()
        other[off[b]:off[b + 1]] = R.rng(31 + b).standard_normal((lens[b], qkv.shape[1])).astype(np.float32) * 3.0
        got = _attn(other, heads, lens)
        keep = np.ones(qkv.shape[0], bool)
        keep[off[b]:off[b + 1]] = False
        np.testing.assert_array_equal(got[keep].view(np.int32), base[keep].view(np.int32))
        assert (got[~keep] != base[~keep]).any()


@pytest.mark.parametrize("heads", R.ATTN_HEADS)
@pytest.mark.parametrize("lens,b,t", [((200, 3), 0, 62), ((200, 3), 0, 63), ((200, 3), 0, 127), ((63, 1, 66), 2, 0), ((200, 3), 1, 1)])
def test_attention_is_causal(heads, lens, b, t):
    """NaN in the k and v of every row after token t of sequence b: the rows up to t are unchanged and finite"""
    qkv = R.attn_inputs(heads, lens)
    E = 64 * heads
    base = _attn(qkv, heads, lens)
    off = np.concatenate([[0], np.cumsum(lens)])
    bad = qkv.copy()
    bad[off[b] + t + 1:off[b + 1], E:3 * E] = np.nan
    got = _attn(bad, heads, lens)
    keep = np.ones(qkv.shape[0], bool)
    keep[off[b] + t + 1:off[b + 1]] = False
    assert np.isfinite(got[keep]).all()
    np.testing.assert_array_equal(got[keep].view(np.int32), base[keep].view(np.int32))


def test_attention_refuses():
    qkv = _dev(R.attn_inputs(3, (5,)))
    off = _dev(np.array([0, 5], np.int32))
    whole, out = _guarded(5, 192, torch.float32)
    _refused(lambda: op_text_attention(qkv, qkv.shape[1], 192, off, 1, 5, 2, 0.125, out), whole, launcher="launch_attn_f32")


# ------------------------------------------------------------------------------- swiglu ---
def _swiglu(gu, T, ld_gu, I, ld_act):
    wh, hi = _guarded(T, ld_act, torch.bfloat16)
    wl, lo = _guarded(T, ld_act, torch.bfloat16)
    op_text_swiglu_split(_dev(gu), T, ld_gu, I, ld_act, hi, lo)
    assert _guards_kept(wh, T) and _guards_kept(wl, T)
    return hi, lo


@pytest.mark.parametrize("T", R.SWIGLU_T)
@pytest.mark.parametrize("I,ld_act,ld_gu", R.SWIGLU_SHAPES)
def test_swiglu_split(I, ld_act, ld_gu, T):
    """silu(gate) * up from the interleaved gate/up row, as hi + lo: (a) with the 2^-126 floor for the gates whose silu
    underflows, (b), and +0 in the columns [I, ld_act) of both halves"""
    g, u = R.swiglu_inputs(I, T)
    hi, lo = _swiglu(R.interleave_gu(g, u, ld_gu), T, ld_gu, I, ld_act)
    h64, l64 = _f64(hi), _f64(lo)
    assert np.isfinite(h64).all() and np.isfinite(l64).all()
    ref = R.swiglu_ref(g, u)
    err, bar, ratio = R.split_errors(h64[:, :I], l64[:, :I], ref, floor=R.TINY)
    print(f"swiglu_split I {I} T {T}: worst error / bar {np.max(err / bar):.3f}, |lo| / (2^-8 |hi|) <= {ratio:.3f}")
    assert (err <= bar).all()
    assert ratio <= 1.0
    assert (_bits(hi)[:, I:] == 0).all() and (_bits(lo)[:, I:] == 0).all()


@pytest.mark.parametrize("which", ["up", "gate"])
@pytest.mark.parametrize("I,ld_act,ld_gu", R.SWIGLU_SHAPES)
def test_swiglu_split_reads_the_right_columns(I, ld_act, ld_gu, which):
    """a gate/up matrix that encodes its own column index, one half at a time.  up: gate 30 everywhere (silu(30) is 30 in fp32)
    and up = the column's index: output i is exactly 30 i (below 2^15, so hi + lo holds it exactly).  gate: up 1 everywhere
    and gate rising strictly from -8 to 8 over the columns: output i is silu(gate_i) to check (a) — a gate read from any other
    column is off by a column's step or more, hundreds of times the bar"""
    T = 2
    col = np.tile(np.arange(I, dtype=np.float32), (T, 1))
    if which == "up":
        g, u = np.full((T, I), 30.0, np.float32), col
    else:
        g, u = (col * np.float32(16.0 / I) - np.float32(8.0)).astype(np.float32), np.ones((T, I), np.float32)
    hi, lo = _swiglu(R.interleave_gu(g, u, ld_gu), T, ld_gu, I, ld_act)
    if which == "up":
        np.testing.assert_array_equal((_f64(hi) + _f64(lo))[:, :I], 30.0 * u.astype(np.float64))
    else:
        ref = R.swiglu_ref(g, u)
        err, bar, _ = R.split_errors(_f64(hi)[:, :I], _f64(lo)[:, :I], ref, floor=R.TINY)
        assert (err <= bar).all()
        # the claim above, on the reference alone: the neighbouring column's value misses the bar (but where silu turns, at -1.28)
        miss = np.abs(ref[:, 1:] - ref[:, :-1]) > 100 * bar[:, 1:]
        assert miss.mean() > 0.97


@pytest.mark.parametrize("I,ld_act,ld_gu", R.SWIGLU_REFUSED)
def test_swiglu_split_refuses(I, ld_act, ld_gu):
    gu = _dev(np.ones((2, ld_gu), np.float32))
    wh, hi = _guarded(2, max(ld_act, I), torch.bfloat16)
    wl, lo = _guarded(2, max(ld_act, I), torch.bfloat16)
    _refused(lambda: op_text_swiglu_split(gu, 2, ld_gu, I, ld_act, hi, lo), wh, wl, launcher="launch_swiglu_split")


# ------------------------------------------------------------------------------- gather ---
@pytest.mark.parametrize("scale", R.GATHER_SCALES)
@pytest.mark.parametrize("dim", R.GATHER_DIMS)
def test_embed_gather(dim, scale):
    """both forms, bit-equal to float32 (hi + lo) * scale and hi * scale: one add and one multiply leave nothing to contract"""
    hi, lo, ids = R.gather_inputs(dim)
    T = len(ids)
    hd, ld, idd = _dev_bf16(hi), _dev_bf16(lo), _dev(ids)
    for low in (ld, None):
        whole, out = _guarded(T, dim, torch.float32)
        op_embed_gather(idd, T, hd, low, dim, scale, out)
        assert _guards_kept(whole, T)
        ref = R.gather_ref(hi, lo if low is not None else None, ids, scale)
        np.testing.assert_array_equal(out.cpu().numpy().view(np.int32), ref.view(np.int32))


def test_embed_gather_refuses():
    hi, lo, ids = R.gather_inputs(64)
    for low in (_dev_bf16(lo), None):
        whole, out = _guarded(len(ids), 64, torch.float32)
        _refused(lambda: op_embed_gather(_dev(ids), len(ids), _dev_bf16(hi), low, 62, 1.0, out), whole,
                 launcher="launch_embed_gather(_hp)?")


# --------------------------------------------------------------------------------- pool ---
@pytest.mark.parametrize("lens", R.POOL_LENS, ids=lambda l: "-".join(map(str, l)))
@pytest.mark.parametrize("dim", R.POOL_DIMS)
@pytest.mark.parametrize("mode", R.POOL_MODES)
def test_pool(mode, dim, lens):
    """final RMSNorm -> pooling -> L2 within 8 x the float32 restatement's error of float64; the tap holds the normed rows to
    the same kind of bar; asking for the tap does not change a bit of the pooled rows; an all-zero sequence gives zeros"""
    h, w, off = R.pool_inputs(dim, lens)
    B, T = len(lens), h.shape[0]
    ref, normed = R.pool_ref(h, w, off, R.RMS_EPS, mode)
    r32, n32 = R.pool_ref(h, w, off, R.RMS_EPS, mode, np.float32)
    bar, e32 = R.restatement_bar(ref, r32, R.POOL_BAR_FACTOR)
    tbar, t32 = R.restatement_bar(normed, n32, R.POOL_BAR_FACTOR)
    hd = torch.zeros((T + G, dim), dtype=torch.float32, device=DEV)       # (readable rows behind the last token)
    hd[:T] = _dev(h)
    wd = torch.zeros(dim + 64, dtype=torch.float32, device=DEV)
    wd[:dim] = _dev(w)
    od = _dev(off)
    wo, out = _guarded(B, dim, torch.float32)
    op_pool(hd, od, B, dim, wd, R.RMS_EPS, out, None, mode)
    wo2, out2 = _guarded(B, dim, torch.float32)
    wt, tap = _guarded(T, dim, torch.float32)
    op_pool(hd, od, B, dim, wd, R.RMS_EPS, out2, tap, mode)
    assert _guards_kept(wo, B) and _guards_kept(wo2, B) and _guards_kept(wt, T)
    got, gtap = out.cpu().numpy(), tap.cpu().numpy()
    err, terr = float(np.max(np.abs(got - ref))), float(np.max(np.abs(gtap - normed)))
    print(f"pool mode {mode} dim {dim} lens {lens}: pooled error {err:.3g} (float32 restatement {e32:.3g}, bar {bar:.3g}), "
          f"tap error {terr:.3g} (float32 restatement {t32:.3g}, bar {tbar:.3g})")
    assert np.isfinite(got).all() and np.isfinite(gtap).all()
    assert err <= bar
    assert terr <= tbar
    np.testing.assert_array_equal(got.view(np.int32), out2.cpu().numpy().view(np.int32))
    z = R.POOL_ZERO_SEQ[tuple(lens)]
    assert (got[z] == 0).all()


@pytest.mark.parametrize("dim,mode", [(2564, 0), (64, 4), (66, 1)])
def test_pool_refuses(dim, mode):
    h, off = _dev(np.ones((3, dim), np.float32)), _dev(np.array([0, 1, 3], np.int32))
    wo, out = _guarded(2, dim, torch.float32)
    wt, tap = _guarded(3, dim, torch.float32)
    _refused(lambda: op_pool(h, off, 2, dim, _dev(np.ones(dim, np.float32)), R.RMS_EPS, out, tap, mode), wo, wt, launcher="launch_pool")


# -------------------------------------------------------------------------- conversions ---
def _flat_guarded(n, dtype, pad=64):
    whole = torch.full((n + 2 * pad,), SENT[dtype], dtype=dtype, device=DEV)
    return whole, whole[pad:pad + n], pad


@pytest.mark.parametrize("n", R.CONVERT_N)
def test_f32_to_bf16(n):
    """bit-equal to torch's round-to-nearest-even on bit patterns around every rounding decision (ties to even and to odd, both
    neighbours, +-0, subnormals, overflow to inf, +-inf); NaN stays NaN"""
    u = R.convert_input(n)
    src = torch.from_numpy(u.view(np.float32).copy())
    want = src.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    whole, out, pad = _flat_guarded(n, torch.bfloat16)
    op_convert(0, src.to(DEV), out, n=n)
    assert _untouched(whole[:pad]) and _untouched(whole[pad + n:])
    got = _bits(out).view(np.uint16)
    nan = np.isnan(u.view(np.float32))
    np.testing.assert_array_equal(got[~nan], want[~nan])
    assert np.isnan(R.bf16_to_f32(got[nan])).all()


@pytest.mark.parametrize("with_word", [False, True])
@pytest.mark.parametrize("n,n_total", R.CONVERT_PAD)
def test_f32_to_bf16_pad(n, n_total, with_word):
    u = R.convert_input(max(n, 4))[:n]
    src = torch.from_numpy(np.concatenate([u, np.zeros(4, np.uint32)]).view(np.float32).copy())
    want = src[:n].to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    whole, out, pad = _flat_guarded(n_total, torch.bfloat16)
    words = torch.full((6,), SENT[torch.int32], dtype=torch.int32, device=DEV)
    op_convert(1, src.to(DEV), out, n=n, n_total=n_total, aux=words[2:4] if with_word else None)
    assert _untouched(whole[:pad]) and _untouched(whole[pad + n_total:])
    got = _bits(out).view(np.uint16)
    nan = np.isnan(u.view(np.float32))
    np.testing.assert_array_equal(got[:n][~nan], want[~nan])
    assert np.isnan(R.bf16_to_f32(got[:n][nan])).all()
    assert (got[n:] == 0).all()
    assert words.cpu().tolist() == ([-7, -7, 0, 0, -7, -7] if with_word else [-7] * 6)


def test_f32_to_bf16_pad_refuses():
    src = _dev(np.ones(16, np.float32))
    whole, out, _ = _flat_guarded(16, torch.bfloat16)
    for n, n_total in ((6, 8), (4, 10)):
        _refused(lambda: op_convert(1, src, out, n=n, n_total=n_total), whole, launcher="launch_f32_to_bf16_pad")


@pytest.mark.parametrize("n", R.SPLIT_N)
def test_split_bf16(n):
    """bit-equal to hi = bf16(v), lo = bf16(v - hi): v - hi is exact in fp32"""
    v = R.split_input(n)
    hi, lo = R.split_hi_lo(v)
    wh, oh, pad = _flat_guarded(n, torch.bfloat16)
    wl, ol, _ = _flat_guarded(n, torch.bfloat16)
    op_convert(2, _dev(v), oh, ol, n=n)
    for w in (wh, wl):
        assert _untouched(w[:pad]) and _untouched(w[pad + n:])
    np.testing.assert_array_equal(_bits(oh).view(np.uint16), R.bf16_bits(hi))
    np.testing.assert_array_equal(_bits(ol).view(np.uint16), R.bf16_bits(lo))


def _any_nonzero(words16, flag0):
    flags = torch.full((5,), SENT[torch.int32], dtype=torch.int32, device=DEV)
    flags[2] = flag0
    src = torch.from_numpy(words16.view(np.int16).copy()).to(DEV)
    op_convert(3, src, n=words16.size, aux=flags[2:3])
    got = flags.cpu().tolist()
    assert got[:2] == [-7, -7] and got[3:] == [-7, -7]
    return got[2]


@pytest.mark.parametrize("n", R.NONZERO_N + (R.NONZERO_FAR + 2,))
def test_any_nonzero16(n):
    """+0 and -0 count as zero; a lone 0x0001 is found at index 0, at n - 1 and (in the long array) at an index only the stride
    loop reaches; a flag that is already 1 stays 1"""
    zeros = np.zeros(n, np.uint16)
    mixed = zeros.copy()
    mixed[::2] = 0x8000
    assert _any_nonzero(zeros, 0) == 0
    assert _any_nonzero(mixed, 0) == 0
    assert _any_nonzero(mixed, 1) == 1
    for at in sorted({0, n - 1} | ({R.NONZERO_FAR} if n > R.NONZERO_FAR else set())):
        one = mixed.copy()
        one[at] = 0x0001
        assert _any_nonzero(one, 0) == 1, at
    top = zeros.copy()
    top[n - 1] = 0x8001            # the sign bit alone is zero, with any other bit it is not
    assert _any_nonzero(top, 0) == 1


@pytest.mark.parametrize("kind", [4, 5], ids=["iota_pos", "seq_of"])
def test_positions_and_sequence_ids(kind):
    off = np.array(R.SEQ_OFFSETS, np.int32)
    want = R.positions_ref(off, SENT[torch.int32])[kind - 4]
    whole, out, pad = _flat_guarded(want.size, torch.int32)
    op_convert(kind, _dev(off), out, n=len(off) - 1)
    assert _untouched(whole[:pad]) and _untouched(whole[pad + want.size:])
    np.testing.assert_array_equal(out.cpu().numpy(), want)


# --------------------------------------------------------------------------- planes_sum ---
@pytest.mark.parametrize("alpha", R.PLANES_ALPHA)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("N,ldp,ldo", R.PLANES_SHAPES)
@pytest.mark.parametrize("T", R.PLANES_T)
@pytest.mark.parametrize("n_parts", R.PLANES_N_PARTS)
def test_planes_sum(n_parts, T, N, ldp, ldo, accumulate, alpha):
    """bit-equal to the float32 sum in the kernel's order (planes in order, * alpha, + out); the columns [N, ldo) keep the
    sentinel"""
    parts, out0 = R.planes_inputs(n_parts, T, N, ldp)
    whole, out = _guarded(T, ldo, torch.float32)
    out[:, :N] = _dev(out0)
    op_planes_sum(_dev(parts), n_parts, parts.shape[1] * ldp, ldp, T, N, out, ldo, alpha, accumulate)
    assert _guards_kept(whole, T) and _untouched(out[:, N:])
    ref = R.planes_sum_ref(parts, T, N, out0, alpha, accumulate)
    np.testing.assert_array_equal(out[:, :N].cpu().numpy().view(np.int32), ref.view(np.int32))


@pytest.mark.parametrize("N,ldp,ldo", R.PLANES_REFUSED)
def test_planes_sum_refuses(N, ldp, ldo):
    parts = _dev(np.ones((2, 4, 256), np.float32))
    whole, out = _guarded(2, 256, torch.float32)
    _refused(lambda: op_planes_sum(parts, 2, 4 * 256, ldp, 2, N, out, ldo, 1.0, 0), whole, launcher="launch_planes_sum")


def test_planes_sum_closes_the_split_precision_gemm():
    """The text path's product in its own layout: A = [hi rows | lo rows] as ONE fp32 GEMM of 2 T rows against W_hi, A_hi W_lo
    as a second, planes_sum over the three planes — against float64 A W^T of the unsplit operands, within 2^-15 sum |a||w|
    (the dropped lo x lo term and the two splits are each <= 2^-16 of that sum; a bf16-only product misses by 2^-8)."""
    T, K, N = 20, 256, 256
    g = R.rng(77)
    A = g.standard_normal((T, K)).astype(np.float32)
    W = (g.standard_normal((N, K)) * 0.1).astype(np.float32)
    (ah, al), (wh, wl) = R.split_hi_lo(A), R.split_hi_lo(W)
    Ad = torch.zeros((256, K), dtype=torch.bfloat16, device=DEV)
    Ad[:T], Ad[T:2 * T] = _dev_bf16(ah), _dev_bf16(al)
    Wh, Wl = _dev_bf16(wh), _dev_bf16(wl)
    whole, planes = _guarded(3 * T, N, torch.float32)
    op_gemm_ex(Ad, Wh, 2 * T, N, EPI_F32, planes[:2 * T])
    op_gemm_ex(Ad, Wl, T, N, EPI_F32, planes[2 * T:])
    wo, out = _guarded(T, N, torch.float32)
    op_planes_sum(planes, 3, T * N, N, T, N, out, N, 1.0, 0)
    assert _guards_kept(whole, 3 * T) and _guards_kept(wo, T)
    ref = A.astype(np.float64) @ W.astype(np.float64).T
    mag = np.abs(A.astype(np.float64)) @ np.abs(W.astype(np.float64)).T
    err = np.abs(out.cpu().numpy() - ref)
    print(f"split-precision product: worst error / (2^-15 sum |a||w|) = {np.max(err / (R.HP_GEMM_BAR * mag)):.3f}")
    assert (err <= R.HP_GEMM_BAR * mag).all()
    # the bar separates: the hi x hi plane alone misses it almost everywhere
    assert (np.abs(planes[:T].cpu().numpy() - ref) > R.HP_GEMM_BAR * mag).mean() > 0.5


# -------------------------------------------------------------------------- patch embed ---
@functools.lru_cache(maxsize=None)
def _patch_case(n, gh, gw, D):
    imgs, w, b, pos = R.patch_inputs(n, gh, gw, D)
    ref, mag = R.patch_embed_ref(imgs, w, b, pos)
    frozen = R.frozen(ref, mag)
    return imgs, w, b, pos, frozen[0], frozen[1]


def _patch_embed(imgs, w, b, pos, D, H=None, W=None, K=R.PATCH_K):
    n, gh, gw = imgs.shape[0], imgs.shape[1] // R.PATCH_P, imgs.shape[2] // R.PATCH_P
    M = n * gh * gw
    whole, out = _guarded(M, D, torch.float32)
    dimgs = [_dev(imgs[i]) for i in range(n)]
    op_patch_embed(dimgs, H or imgs.shape[1], W or imgs.shape[2], R.PATCH_P, _dev(w), D, K, _dev(b), _dev(pos), D, out, D)
    return whole, out, M


@pytest.mark.parametrize("D", R.PATCH_D)
@pytest.mark.parametrize("n,gh,gw", R.PATCH_IMAGES)
def test_patch_embed(n, gh, gw, D):
    """pixels -> bf16((x / 255 - 0.5) / 0.5), conv with the bf16 weight, + bias + pos[(py, px)]: within 2^-20 sum |a||w| +
    2^-23 |ref| of float64 on the same rounded operands, for several images, non-square grids and an M that ends inside a
    128-row tile; the rows past M keep the sentinel; a row depends on its own image's bytes only"""
    imgs, w, b, pos, ref, mag = _patch_case(n, gh, gw, D)
    whole, out, M = _patch_embed(imgs, w, b, pos, D)
    assert _guards_kept(whole, M)
    got = out.cpu().numpy()
    err, bar = np.abs(got - ref), R.patch_bar(ref, mag)
    print(f"patch_embed n {n} grid {gh}x{gw} D {D}: worst error / bar {np.max(err / bar):.3f} (error {err.max():.3g})")
    assert np.isfinite(got).all()
    assert (err <= bar).all()
    if n >= 3:
        other = imgs.copy()
        other[0] = 255 - other[0]
        _, out2, _ = _patch_embed(other, w, b, pos, D)
        N = gh * gw
        got2 = out2.cpu().numpy()
        np.testing.assert_array_equal(got2[N:].view(np.int32), got[N:].view(np.int32))
        assert (got2[:N] != got[:N]).mean() > 0.9


@pytest.mark.parametrize("H,K", [(29, R.PATCH_K), (28, 576)], ids=["H % P", "3 P^2 > K"])
def test_patch_embed_refuses(H, K):
    _, w, b, pos, _, _ = _patch_case(1, 2, 2, 128)
    img = _dev(np.zeros((32, 28, 3), np.uint8))              # (rows enough for H = 29)
    whole, out = _guarded(4, 128, torch.float32)
    _refused(lambda: op_patch_embed([img], H, 28, R.PATCH_P, _dev(w), 128, K, _dev(b), _dev(pos), 128, out, 128), whole,
             launcher="launch_patch_embed")


# -------------------------------------------------------------------------------- norms ---
def _norm_ex(kind, x, w, b, dim, ldx, ldo, eps):
    """out bf16 [rows][ldo] of one launch on rows of pitch ldx whose pitch columns hold NaN"""
    rows = x.shape[0]
    xp = np.full((rows, ldx), np.nan, np.float32)
    xp[:, :dim] = x
    whole, out = _guarded(rows, ldo, torch.bfloat16)
    op_norm_ex(kind, _dev(xp), rows, dim, ldx, _dev(w), _dev(b) if b is not None else None, eps, out, ldo)
    assert _guards_kept(whole, rows)
    return out


def _norm_check(name, out, ref, dim):
    got = _f64(out)
    assert np.isfinite(got).all()
    ulps = np.abs(got[:, :dim] - ref) / R.ulp_bf16(ref)
    print(f"{name}: within {ulps.max():.3f} ulp_bf16 of float64")
    assert ulps.max() <= 1.0
    assert (_bits(out)[:, dim:] == 0).all()


@pytest.mark.parametrize("rows", R.LN_ROWS)
@pytest.mark.parametrize("dim,ldx,ldo", R.LN_SHAPES)
def test_layernorm_ex(dim, ldx, ldo, rows):
    """the three register forms (5 with two rows per wave, 10, 14), an input pitch wider than dim, odd row counts: within one
    bf16 ulp of float64, the columns [dim, ldo) zero"""
    x, w, b = R.norm_inputs(dim, rows)
    out = _norm_ex(0, x, w, b, dim, ldx, ldo, R.LN_EPS)
    _norm_check(f"layernorm dim {dim} ldx {ldx} rows {rows}", out, R.layer_norm(x, w, b, R.LN_EPS), dim)


@pytest.mark.parametrize("rows", R.RMS_ROWS)
@pytest.mark.parametrize("dim,ldx,ldo", R.RMS_SHAPES)
def test_rmsnorm_ex(dim, ldx, ldo, rows):
    x, w, _ = R.norm_inputs(dim, rows)
    out = _norm_ex(1, x, w, None, dim, ldx, ldo, R.RMS_EPS)
    _norm_check(f"rmsnorm dim {dim} rows {rows}", out, R.rms_norm(x, w, R.RMS_EPS), dim)


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("dim,ldx,ldo", R.NORM_REFUSED)
def test_norm_ex_refuses(dim, ldx, ldo, kind):
    x = _dev(np.ones((2, max(dim, ldx)), np.float32))
    w = _dev(np.ones(dim, np.float32))
    whole, out = _guarded(2, max(dim, ldo), torch.bfloat16)
    _refused(lambda: op_norm_ex(kind, x, 2, dim, ldx, w, w, 1e-6, out, ldo), whole,
             launcher="launch_layernorm" if kind == 0 else "launch_rmsnorm")
