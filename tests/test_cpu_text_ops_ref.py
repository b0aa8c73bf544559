"""The float64 references of tests/text_ops_ref.py pinned against independent implementations that are already trusted here
(oracle/visrag_ret_oracle.py, torch.nn.functional.conv2d, torch's bf16 rounding), the float32-restatement errors that the
x 8 bars of tests/test_gpu_text_ops.py rest on (printed, and bounded so that a drift of the yardstick shows), and the
conditions the case tables have to meet.  No GPU, no library."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import visrag_ret_oracle as O
from tests import text_ops_ref as R


def _t64(a):
    return torch.from_numpy(np.array(a, np.float64))


# ---------------------------------------------------------------------------------- bf16 ---
def test_bf16_rounding_is_torchs_round_to_nearest_even():
    u = np.concatenate([R.rounding_patterns(), R.convert_input(5000)])
    want = torch.from_numpy(u.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_bits(u.view(np.float32))
    nan = np.isnan(u.view(np.float32))
    np.testing.assert_array_equal(got[~nan], want[~nan])
    assert np.isnan(R.bf16_to_f32(got[nan])).all() and np.isnan(R.bf16_to_f32(want[nan])).all()
    # the patterns hold what they claim: exact ties (both parities), both neighbours, overflow to inf, subnormals
    p = R.rounding_patterns()
    low = p & 0xFFFF
    assert ((low == 0x8000) & ((p >> 16) & 1 == 0)).any() and ((low == 0x8000) & ((p >> 16) & 1 == 1)).any()
    assert (low == 0x7FFF).any() and (low == 0x8001).any()
    assert np.isinf(R.bf16_round(np.array([0x7F7FFFFF], np.uint32).view(np.float32))).all()
    assert np.isfinite(R.bf16_round(np.array([0x7F7F7FFF], np.uint32).view(np.float32))).all()


def test_split_is_exact_to_sixteen_bits_and_hi_is_a_rounding():
    v = R.split_input(R.SPLIT_N[-1])
    hi, lo = R.split_hi_lo(v)
    err, bar, ratio = R.split_errors(hi, lo, v.astype(np.float64), floor=R.TINY)
    assert (err <= 2.0 ** -16 * np.abs(v) + R.TINY).all() and (err <= bar).all() and ratio <= 1.0
    # v - hi is exact in float32 (what makes the kernel's lo bit-reproducible in numpy)
    np.testing.assert_array_equal((v - hi).astype(np.float64), v.astype(np.float64) - hi.astype(np.float64))
    # a truncated hi breaks (b), a dropped lo breaks (a): the two checks see what they are for
    trunc = (v.view(np.uint32) & 0xFFFF0000).view(np.float32)
    assert R.split_errors(trunc, R.bf16_round(v - trunc), v.astype(np.float64))[2] > 1.5
    e0, b0, _ = R.split_errors(hi, np.zeros_like(lo), v.astype(np.float64), floor=R.TINY)
    assert (e0 > b0).mean() > 0.9


# ------------------------------------------------------------------------------- rmsnorm ---
@pytest.mark.parametrize("dim", R.RMSNORM_DIMS)
def test_rmsnorm_reference_and_the_split_bar(dim):
    x, w = R.rmsnorm_inputs(dim)
    ref = R.rms_norm(x, w, R.RMS_EPS)
    np.testing.assert_allclose(ref, O.rms_norm(_t64(x), _t64(w), R.RMS_EPS).numpy(), rtol=1e-13, atol=0)
    assert (ref[1] == 0).all() and np.isfinite(ref).all() and np.abs(ref[2]).max() > 0.9 * np.sqrt(dim) * 0.5
    # the float32 restatement, split as the kernel splits: below 7.7e-6 relative (about 2^-17), inside the 1.25 * 2^-16 bar
    y32 = R.rms_norm(x, w, R.RMS_EPS, np.float32)
    hi, lo = R.split_hi_lo(y32)
    err, bar, ratio = R.split_errors(hi, lo, ref)
    rel = float(np.max(err[ref != 0] / np.abs(ref[ref != 0])))
    print(f"rmsnorm_split dim {dim}: float32 restatement relative error {rel:.3g} (bar {R.SPLIT_REL:.3g})")
    assert rel < 7.7e-6 and (err <= bar).all() and ratio <= 1.0


# ---------------------------------------------------------------------------------- rope ---
@pytest.mark.parametrize("E", R.ROPE_E)
def test_rope_reference_is_the_oracles_rotation(E):
    qkv, pos, table = R.rope_inputs(E)
    ref, mag = R.rope_ref(qkv, pos, table, 2 * E)
    T, heads = qkv.shape[0], E // 64
    cos, sin = O.rope_tables(64, 8, 10000.0)
    # the table is the oracle's (fp32 cos / sin of the same angles, to an ulp or two of their float32 evaluation)
    np.testing.assert_allclose(table[:, :32], cos[:, :32].numpy(), rtol=0, atol=3e-7)
    np.testing.assert_allclose(table[:, 32:], sin[:, :32].numpy(), rtol=0, atol=3e-7)
    t64 = _t64(table)[torch.from_numpy(np.array(pos)).long()]
    c, s = torch.cat([t64[:, :32]] * 2, -1)[:, None], torch.cat([t64[:, 32:]] * 2, -1)[:, None]
    q = _t64(qkv[:, :E]).view(T, heads, 64)
    k = _t64(qkv[:, E:2 * E]).view(T, heads, 64)
    qr, kr = O.apply_rope(q, k, c, s)
    np.testing.assert_allclose(ref[:, :E], qr.reshape(T, E).numpy(), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(ref[:, E:2 * E], kr.reshape(T, E).numpy(), rtol=1e-14, atol=1e-15)
    np.testing.assert_array_equal(ref[:, 2 * E:], qkv[:, 2 * E:].astype(np.float64))
    rows0 = np.array(R.ROPE_POS) == 0
    np.testing.assert_array_equal(ref[rows0], qkv[rows0].astype(np.float64))       # cos 0 = 1, sin 0 = 0: untouched
    # a float32 rotation (two products, one sum) stays within 1.5 ulps at the magnitude of its terms: 4 leaves room for nothing else
    x = qkv.astype(np.float32)
    tt = table[pos]
    got = x.copy()
    for h in range(2 * E // 64):
        a, b = x[:, h * 64:h * 64 + 32], x[:, h * 64 + 32:h * 64 + 64]
        got[:, h * 64:h * 64 + 32] = a * tt[:, :32] - b * tt[:, 32:]
        got[:, h * 64 + 32:h * 64 + 64] = b * tt[:, :32] + a * tt[:, 32:]
    assert np.max(np.abs(got - ref) / R.ulp_f32(mag)) <= 1.5


# ----------------------------------------------------------------------------- attention ---
def _oracle_attention(qkv, heads, lens, scale):
    E = 64 * heads
    out = np.zeros((qkv.shape[0], E))
    t0 = 0
    for L in lens:
        x = _t64(qkv[t0:t0 + L])
        q, k, v = (x[:, o:o + E].view(L, heads, 64).transpose(0, 1) for o in (0, E, 2 * E))
        mask = torch.full((L, L), -np.inf, dtype=torch.float64).triu(1)
        out[t0:t0 + L] = O.sdpa(q, k, v, mask=mask, scale=scale).transpose(0, 1).reshape(L, E).numpy()
        t0 += L
    return out


@pytest.mark.parametrize("gain", R.ATTN_QK_GAIN)
@pytest.mark.parametrize("heads", R.ATTN_HEADS)
def test_attention_reference_is_the_oracles_sdpa(heads, gain):
    worst = 0.0
    for lens in R.ATTN_SEQS:
        qkv = R.attn_inputs(heads, lens, gain)
        ref = R.attn_ref(qkv, heads, lens, 0.125)
        np.testing.assert_allclose(ref, _oracle_attention(qkv, heads, lens, 0.125), rtol=1e-12, atol=1e-13)
        bar, e32 = R.restatement_bar(ref, R.attn_ref(qkv, heads, lens, 0.125, np.float32))
        print(f"attn_f32 heads {heads} lens {lens} gain {gain}: float32 restatement error {e32:.3g}, bar {bar:.3g}")
        worst = max(worst, e32)
        assert e32 > 0 or sum(lens) == 1
        # the first token of a sequence sees itself only
        off = np.concatenate([[0], np.cumsum(lens)])[:-1]
        np.testing.assert_array_equal(ref[off], qkv[off, 2 * 64 * heads:3 * 64 * heads].astype(np.float64))
    # fp32-class: bf16 operands would sit at 6e-3 and above
    assert worst < (2e-6 if gain == 1.0 else 1e-4)


@pytest.mark.parametrize("case", R.ATTN_SCORE_CASES)
def test_attention_score_cases_are_what_they_say(case):
    qkv = R.attn_score_case(case)
    q, k = qkv[:, :64].astype(np.float64), qkv[:, 64:128].astype(np.float64)
    s = np.where(np.tril(np.ones((200, 200), bool)), q @ k.T * 0.125, -np.inf)
    if case == "dominant_second_group":
        assert 64 <= s[199].argmax() < 128 and s[199].max() > np.sort(s[199])[-2] + 20
    elif case == "dominant_third_group":
        assert 128 <= s[199].argmax() < 192 and s[199].max() > np.sort(s[199])[-2] + 20
    elif case == "rising":
        m = [s[199, g * 64:min(200, (g + 1) * 64)].max() for g in range(4)]
        assert m[0] < m[1] < m[2] < m[3]
    elif case == "all_below_minus_60":
        assert s[np.isfinite(s)].max() < -60
    else:
        assert (s[1:, 0] > np.where(np.isfinite(s[1:, 1:]), s[1:, 1:], -np.inf).max(axis=1) + 10).mean() > 0.9
    ref = R.attn_ref(qkv, 1, (200,), 0.125)
    np.testing.assert_allclose(ref, _oracle_attention(qkv, 1, (200,), 0.125), rtol=1e-11, atol=1e-13)
    bar, e32 = R.restatement_bar(ref, R.attn_ref(qkv, 1, (200,), 0.125, np.float32))
    print(f"attn_f32 score case {case}: float32 restatement error {e32:.3g}, bar {bar:.3g}")
    assert 0 < e32 < 1e-4


# -------------------------------------------------------------------------------- swiglu ---
@pytest.mark.parametrize("I,ld_act,ld_gu", R.SWIGLU_SHAPES)
def test_swiglu_reference_and_layout(I, ld_act, ld_gu):
    g, u = R.swiglu_inputs(I, 3)
    ref = R.swiglu_ref(g, u)
    want = (F.silu(_t64(g)) * _t64(u)).numpy()
    np.testing.assert_allclose(ref, want, rtol=1e-13, atol=1e-300)
    for gate in R.SWIGLU_GATES:
        assert (g == np.float32(gate)).any()
    assert np.isfinite(ref).all()
    # the interleave is the GEMM epilogue's: gate of column i at (i / 16) * 32 + i % 16, up 16 further
    gu = R.interleave_gu(g, u, ld_gu)
    i = np.arange(I)
    np.testing.assert_array_equal(gu[:, (i // 16) * 32 + i % 16], g)
    np.testing.assert_array_equal(gu[:, (i // 16) * 32 + 16 + i % 16], u)
    assert ld_gu >= 2 * I and ld_act >= I
    # the float32 restatement, split: inside (a) with the 2^-126 floor, and (b)
    y32 = R.swiglu_ref(g, u, np.float32)
    hi, lo = R.split_hi_lo(y32)
    err, bar, ratio = R.split_errors(hi, lo, ref, floor=R.TINY)
    assert (err <= bar).all() and ratio <= 1.0


# --------------------------------------------------------------------------- pool, norms ---
@pytest.mark.parametrize("lens", R.POOL_LENS)
@pytest.mark.parametrize("dim", R.POOL_DIMS)
def test_pool_reference_is_the_oracles_pooling(dim, lens):
    h, w, off = R.pool_inputs(dim, lens)
    B, Lmax = len(lens), max(lens)
    for mode in R.POOL_MODES:
        ref, normed = R.pool_ref(h, w, off, R.RMS_EPS, mode)
        np.testing.assert_allclose(normed, O.rms_norm(_t64(h), _t64(w), R.RMS_EPS).numpy(), rtol=1e-13, atol=0)
        hid = torch.zeros((B, Lmax, dim), dtype=torch.float64)
        mask = torch.zeros((B, Lmax), dtype=torch.int64)
        for b in range(B):
            hid[b, :lens[b]] = _t64(normed[off[b]:off[b + 1]])
            mask[b, :lens[b]] = 1
        want = O.pool_normalize(hid, mask, R.POOL_MODE_NAMES[mode]).numpy()
        np.testing.assert_allclose(ref, want, rtol=1e-12, atol=1e-15)
        z = R.POOL_ZERO_SEQ[tuple(lens)]
        assert (ref[z] == 0).all() and np.isfinite(ref).all()
        r32, n32 = R.pool_ref(h, w, off, R.RMS_EPS, mode, np.float32)
        bar, e32 = R.restatement_bar(ref, r32, R.POOL_BAR_FACTOR)
        tbar, t32 = R.restatement_bar(normed, n32, R.POOL_BAR_FACTOR)
        print(f"pool dim {dim} lens {lens} mode {mode}: float32 restatement error pooled {e32:.3g}, tap {t32:.3g}")
        assert 0 < e32 < 2e-7 and 0 < t32 < 2e-6


@pytest.mark.parametrize("rows", R.LN_ROWS)
@pytest.mark.parametrize("dim,ldx,ldo", R.LN_SHAPES)
def test_layer_norm_reference_and_the_one_ulp_bar(dim, ldx, ldo, rows):
    x, w, b = R.norm_inputs(dim, rows)
    ref = R.layer_norm(x, w, b, R.LN_EPS)
    np.testing.assert_allclose(ref, O.layer_norm(_t64(x), _t64(w), _t64(b), R.LN_EPS).numpy(), rtol=1e-12, atol=1e-14)
    # on the inputs the GPU test uses, a float32 layer_norm rounded to bf16 lands well inside the one-ulp bar
    out = R.bf16_round(R.layer_norm(x, w, b, R.LN_EPS, np.float32))
    worst = float(np.max(np.abs(out - ref) / R.ulp_bf16(ref)))
    print(f"layer_norm dim {dim} rows {rows}: float32 restatement rounded to bf16 within {worst:.3f} ulp_bf16")
    assert worst <= 0.6
    assert dim <= ldx and dim <= ldo
    # the inputs stay what they were drawn as, up to a few stepped biases
    assert np.abs(b).max() < 1.5 and 0.15 < b.std() < 0.25


def test_layer_norm_bar_needs_inputs_without_cancellation():
    """what norm_inputs steps away from: where a product cancels against its bias, float32 arithmetic itself misses one ulp"""
    g = R.rng(1000 + 1284 + 7)
    x = (g.standard_normal((7, 1284)) * 1.7 + 0.4).astype(np.float32)
    w = (1.0 + 0.3 * g.standard_normal(1284)).astype(np.float32)
    b = (0.2 * g.standard_normal(1284)).astype(np.float32)
    assert R.layer_norm_cancels(x, w, b).sum() >= 1
    ref = R.layer_norm(x, w, b, R.LN_EPS)
    out = R.bf16_round(R.layer_norm(x, w, b, R.LN_EPS, np.float32))
    assert float(np.max(np.abs(out - ref) / R.ulp_bf16(ref))) > 1.0


@pytest.mark.parametrize("dim,ldx,ldo", R.RMS_SHAPES)
def test_rms_norm_one_ulp_bar(dim, ldx, ldo):
    x, w, _ = R.norm_inputs(dim, 5)
    ref = R.rms_norm(x, w, R.RMS_EPS)
    out = R.bf16_round(R.rms_norm(x, w, R.RMS_EPS, np.float32))
    assert float(np.max(np.abs(out - ref) / R.ulp_bf16(ref))) <= 0.6


def test_ulp_helpers():
    np.testing.assert_array_equal(R.ulp_bf16(np.array([1.0, 1.99, 2.0, -0.75, 3.0e-3])), 2.0 ** np.array([-7.0, -7, -6, -8, -16]))
    np.testing.assert_array_equal(R.ulp_f32(np.array([1.0, -3.0])), 2.0 ** np.array([-23.0, -22]))
    v = np.float32(1.0) + np.float32(2.0 ** -23)
    assert float(v) - 1.0 == R.ulp_f32(1.0)


# ------------------------------------------------------------------- gather, planes, ids ---
def test_gather_and_planes_references():
    hi, lo, ids = R.gather_inputs(64)
    ref = R.gather_ref(hi, lo, ids, 12.0)
    assert ref.dtype == np.float32 and ref.shape == (len(R.GATHER_IDS), 64)
    np.testing.assert_array_equal(ref[0], ref[4])
    np.testing.assert_array_equal(ref[2], ref[3])
    np.testing.assert_allclose(ref, (hi.astype(np.float64) + lo)[ids] * 12.0, rtol=2.0 ** -23, atol=0)
    np.testing.assert_array_equal(R.gather_ref(hi, None, ids, 1.0), hi[ids])
    assert np.abs(lo).max() > 0 and max(R.GATHER_IDS) == R.GATHER_ROWS - 1
    parts, out0 = R.planes_inputs(9, 5, 1028, 1152)
    for alpha in R.PLANES_ALPHA:
        for acc in (0, 1):
            r = R.planes_sum_ref(parts, 5, 1028, out0, alpha, acc)
            want = parts[:, :5, :1028].astype(np.float64).sum(axis=0) * alpha + (out0 if acc else 0.0)
            np.testing.assert_allclose(r, want, rtol=0, atol=2e-6)
            assert r.dtype == np.float32
        # a power of two: the product is exact, so a contracted multiply-add has the bits of multiply, then add
        a = parts[0][:5, :1028]
        np.testing.assert_array_equal((a * np.float32(alpha)).astype(np.float64), a.astype(np.float64) * alpha)


def test_positions_reference():
    off = np.array(R.SEQ_OFFSETS)
    pos, seq = R.positions_ref(off, -7)
    assert pos[0] == 0 and list(pos[1:4]) == [0, 1, 2] and pos[299] == 298 and pos[300] == 0 and pos[301] == 0 and pos[562] == 261
    assert seq[0] == 0 and seq[1] == 1 and seq[299] == 1 and seq[300] == 2 and seq[301] == 3 and seq[562] == 3
    assert (pos[563:] == -7).all() and (seq[563:] == -7).all()
    assert max(np.diff(off)) > 256          # longer than the workgroup: the kernels' loops run twice


# --------------------------------------------------------------------------- patch embed ---
@pytest.mark.parametrize("n,gh,gw", R.PATCH_IMAGES)
def test_patch_embed_reference_is_conv2d(n, gh, gw):
    D = 128
    imgs, w, b, pos = R.patch_inputs(n, gh, gw, D)
    ref, mag = R.patch_embed_ref(imgs, w, b, pos)
    N = gh * gw
    assert ref.shape == (n * N, D)
    for i in range(n):
        px = O.to_pixel_tensor(imgs[i])                                    # f32 [3][H][W]
        # the kernel's operand is the bf16 rounding of exactly these float32 values
        a = torch.from_numpy(R.bf16_round(px.numpy())).double()
        y = F.conv2d(a[None], _t64(R.bf16_round(w)), _t64(b), stride=R.PATCH_P)[0]       # [D][gh][gw]
        want = y.reshape(D, N).T.numpy() + pos.astype(np.float64)
        np.testing.assert_allclose(ref[i * N:(i + 1) * N], want, rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(R.pixels_bf16(imgs[0]).transpose(2, 0, 1), R.bf16_round(O.to_pixel_tensor(imgs[0]).numpy()))
    ref32, _ = R.patch_embed_ref(imgs, w, b, pos, np.float32)
    bar = R.patch_bar(ref, mag)
    e = np.abs(ref32.astype(np.float64) - ref)
    print(f"patch_embed n {n} grid {gh}x{gw}: float32 restatement error {e.max():.3g}, {np.max(e / bar):.3f} of the bar")
    assert (e <= bar).all()
    for i, value in R.PATCH_CONST[n].items():
        assert (imgs[i] == value).all()
    assert len(np.unique(imgs[0])) == 256 and 0 not in R.PATCH_CONST[n]


def test_case_tables_reach_the_paths_they_name():
    assert 2560 in R.RMSNORM_DIMS and 260 in R.RMSNORM_DIMS and 2564 in R.RMSNORM_REFUSED
    Ms = [n * gh * gw for n, gh, gw in R.PATCH_IMAGES]
    assert Ms == [4, 45, 130, 144] and sum(128 < m < 256 for m in Ms) == 2
    consts = [v for n, _, _ in R.PATCH_IMAGES for v in R.PATCH_CONST[n].values()]
    assert 0 in consts and 255 in consts
    assert any(gh > gw for _, gh, gw in R.PATCH_IMAGES) and any(gh < gw for _, gh, gw in R.PATCH_IMAGES)
    assert R.CONVERT_N[-1] > 2048 * 256 * 4 and all(n % 4 == 0 and t % 4 == 0 for n, t in R.CONVERT_PAD)
    assert 3 * R.PATCH_P ** 2 <= R.PATCH_K and R.PATCH_K % 64 == 0
    assert any(ldo <= 1280 for _, _, ldo in R.LN_SHAPES) and any(1280 < ldo <= 2560 for _, _, ldo in R.LN_SHAPES)
    assert any(ldo > 2560 for _, _, ldo in R.LN_SHAPES) and any(ldx > d for d, ldx, _ in R.LN_SHAPES)
