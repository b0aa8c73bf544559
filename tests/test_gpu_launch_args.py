"""-m gpu: every launch argument of the GEMM and attention kernels, set on a single launch through vr_op_gemm_ex /
vr_op_attention_ex / vr_op_attn_combine, against the fp64 references of tests/launch_args_ref.py on the same (bf16-rounded)
inputs.  The rule under test (include/visrag_hip.h, vr_op_gemm_ex): a field is HONOURED by the kernel the launch reaches, or
the launch is REFUSED before anything runs — never silently ignored.  Outputs are the caller's buffers, prefilled with a
sentinel; "not written" is a bitwise comparison with it.

Tolerances are the ones tests/test_gpu_ops.py states for the same epilogue: fp32 outputs rtol 1e-5, atol 1e-4 * max(1, K / 512);
bf16 outputs rtol 1e-2, atol 2e-2 (3e-2 SwiGLU); attention rtol = atol = 2e-2."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import launch_args_ref as R  # noqa: E402
from tests.gpu_util import op_attention_ex, op_attn_combine, op_gemm_ex  # noqa: E402
from visrag_amd._lib import VisragHipError  # noqa: E402

DEV = "cuda:0"
BF16, GELU, F32, RESID, SWIGLU, ROPE = R.EPI_BF16, R.EPI_GELU, R.EPI_F32, R.EPI_RESID, R.EPI_SWIGLU, R.EPI_ROPE
EPI_NAME = {BF16: "bf16", GELU: "gelu", F32: "f32", RESID: "resid", SWIGLU: "swiglu", ROPE: "rope"}
SENT = {torch.float32: -77.25, torch.bfloat16: 7.0}       # exact in both formats, far from every output here
ALPHA = 0.2214


def _pad(n, mult=256):
    return (n + mult - 1) // mult * mult


def _dev_bf16(x, rows=None):
    """bf16-valued float32 numpy [r][c] -> bf16 on the device, rows zero-padded to `rows`"""
    t = torch.from_numpy(np.array(x)).to(torch.bfloat16)
    if rows is not None and rows > t.shape[0]:
        t = torch.cat([t, torch.zeros((rows - t.shape[0],) + tuple(t.shape[1:]), dtype=torch.bfloat16)])
    return t.to(DEV)


def _dev(x, dtype=None):
    t = torch.from_numpy(np.array(x))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _sentinel(shape, dtype):
    return torch.full(shape, SENT[dtype], dtype=dtype, device=DEV)


def _untouched(t):
    """every element still holds the sentinel's bits"""
    if t.numel() == 0:
        return True
    bits = t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    want = torch.full((1,), SENT[t.dtype], dtype=t.dtype).view(bits.dtype).item()
    return bool((bits == want).all())


def _tol(epi, K):
    if epi in (F32, RESID):
        return dict(rtol=1e-5, atol=1e-4 * max(1.0, K / 512))
    return dict(rtol=1e-2, atol=3e-2 if epi == SWIGLU else 2e-2)


def _out_dtype(epi):
    return torch.float32 if epi in (F32, RESID) else torch.bfloat16


def _np(t):
    return t.float().cpu().numpy().astype(np.float64)


def _refused(fn, out):
    """the LAUNCHERS refuse (status 2, VR_ERR_HIP: hipErrorInvalidValue came back from launch_gemm / launch_gemm_skinny — an
    argument check of the op entry itself would be status 1), and nothing has been launched: the output keeps the sentinel"""
    with pytest.raises(VisragHipError, match=r"\(status 2\): launch_gemm(_skinny)?\("):
        fn()
    torch.cuda.synchronize()
    assert _untouched(out)


# ---------------------------------------------------------------------- shared GEMM inputs ---
@functools.lru_cache(maxsize=None)
def _gemm_case(M, N, K, seed=0):
    """Host inputs and the fp64 accumulators every test of one shape shares (computed once, never modified):
    plain weights for epilogues 0..3 and 5, [16 gate | 16 up] interleaved ones for SwiGLU."""
    A, W, b = R.rand_bf16((M, K), 11 + seed), R.rand_bf16((N, K), 12 + seed, 0.1), R.rand_f32((N,), 13 + seed)
    Wi, bi = R.interleave16(W[:N // 2], W[N // 2:]), R.interleave16(b[:N // 2], b[N // 2:])
    pos = (np.arange(M) % 50).astype(np.int32)
    c = dict(A=A, W=W, b=b, Wi=Wi, bi=bi, pos=pos, table=R.rope_table(64))
    for a in c.values():
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _gemm_dev(M, N, K, seed=0):
    c = _gemm_case(M, N, K, seed)
    return dict(N=N, A=_dev_bf16(c["A"], _pad(M)), W=_dev_bf16(c["W"], _pad(N)), b=_dev(c["b"]), Wi=_dev_bf16(c["Wi"], _pad(N)),
                bi=_dev(c["bi"]), pos=_dev(c["pos"]), table=_dev(c["table"]))


def _epilogue_ref(c, epi, acc_kwargs, resid_rows=None):
    """fp64 value of every (m, n) the launch may write, BEFORE any row map: acc_kwargs go to launch_args_ref.gemm_acc"""
    if epi == SWIGLU:
        return R.swiglu_of_interleaved(R.gemm_acc(c["A"], c["Wi"], c["bi"], **acc_kwargs))
    acc = R.gemm_acc(c["A"], c["W"], None if epi == ROPE else c["b"], **acc_kwargs)
    if epi == GELU:
        return R.gelu(acc)
    if epi == ROPE:
        return R.rope(acc, c["pos"], c["table"], 128)
    if epi == RESID:
        return resid_rows + np.float64(np.float32(ALPHA)) * acc
    return acc


def _launch(d, M, epi, out, variant, resid=None, **extras):
    """one vr_op_gemm_ex call on the shared device inputs"""
    sw = epi == SWIGLU
    return op_gemm_ex(d["A"], d["Wi"] if sw else d["W"], M, d["N"], epi, out, bias=None if epi == ROPE else (d["bi"] if sw else d["b"]),
                      resid=resid, alpha=ALPHA, rope_pos=d["pos"] if epi == ROPE else None,
                      rope_table=d["table"] if epi == ROPE else None, rope_cols=128 if epi == ROPE else 0, variant=variant, **extras)


def _epis_of(variant):
    return {7: (BF16, GELU, F32, RESID), 13: (F32, RESID)}.get(variant, (BF16, GELU, F32, RESID, SWIGLU, ROPE))


# ------------------------------------------------------------------------------ row map ---
ROWMAP_CASES = [(v, N, e) for v in (0, 3, 9, 12, 7, 13) for N in (256, 384) if not (v in (7, 13) and N % 192)
                for e in _epis_of(v)]


def _check_rowmap(M, N, K, rows_map, variant, epi, seed):
    c, d = _gemm_case(M, N, K), _gemm_dev(M, N, K)
    rm = R.row_map(M, rows_map, seed)
    Mp = _pad(M)
    rows = max(Mp, rows_map) + Mp             # (a launch that ignored the map, or padded rows, would still be in bounds)
    cols = N // 2 if epi == SWIGLU else N
    out = _sentinel((rows, cols), _out_dtype(epi))
    resid_h = R.rand_f32((rows, cols), 17) if epi == RESID else None
    resid_at = None
    if epi == RESID:                          # the residual is read at the MAPPED row
        resid_at = np.asarray(resid_h, np.float64)[np.where(rm >= 0, rm, 0)]
    _launch(d, M, epi, out, variant, resid=_dev(resid_h) if epi == RESID else None, rowmap=_dev(rm))
    want, written = R.scatter_rows(_epilogue_ref(c, epi, {}, resid_at), rm, rows)
    got = _np(out)
    np.testing.assert_allclose(got[written], want[written], **_tol(epi, K))
    assert _untouched(out[torch.from_numpy(~written).to(DEV)]), "a row nobody maps to (or a dropped row's own index) was written"


@pytest.mark.parametrize("variant,N,epi", ROWMAP_CASES, ids=[f"v{v}-N{N}-{EPI_NAME[e]}" for v, N, e in ROWMAP_CASES])
def test_row_map_scatters_rows_and_drops(variant, N, epi):
    """GemmArgs::rowmap (the resampler's scatter into the decoder rows): 300 rows into 400, one in eight dropped; N = 384 is the
    column edge of the 256-wide tiles and the shape of the 192-wide ones."""
    _check_rowmap(300, N, 128, 400, variant, epi, 21)


def test_row_map_on_the_auto_route_to_the_256x192_tile():
    """M >= 4096, N = 384, EPI_RESID and a row map: the engine's own choice (variant 3) sends this to gemm192.hip."""
    _check_rowmap(4096 + 37, 384, 128, 4096 + 37 + 400, 3, RESID, 22)


# ----------------------------------------------------------------------------- row bias ---
RB_FORMS = [(256, 64), (512, 128), (100, 64), (256, 96)]
RB_M, RB_N, RB_K, RB_LD = 600, 256, 64, 128


@functools.lru_cache(maxsize=None)
def _rowbias(period):
    t = R.rand_f32((period, RB_LD), 31 + period)
    t.setflags(write=False)
    return t


@pytest.mark.parametrize("epi", [BF16, GELU, F32], ids=lambda e: EPI_NAME[e])
@pytest.mark.parametrize("period,cols", RB_FORMS)
@pytest.mark.parametrize("variant", [0, 9, 12, 3])
def test_row_bias_values(variant, period, cols, epi):
    """GemmArgs::rowbias (the ViT position embedding, pos_k): row m % period of the table, columns n < cols only.  (256, 64) and
    (512, 128) ride the one-wave kernel's descriptor form; a period a tile wraps around, or columns that are no whole 64-column
    block, take the general form."""
    c, d = _gemm_case(RB_M, RB_N, RB_K), _gemm_dev(RB_M, RB_N, RB_K)
    rb = _rowbias(period)
    out = _sentinel((_pad(RB_M), RB_N), _out_dtype(epi))
    _launch(d, RB_M, epi, out, variant, rowbias=_dev(rb), rowbias_period=period, rowbias_ld=RB_LD, rowbias_cols=cols)
    want = _epilogue_ref(c, epi, dict(rowbias=rb, period=period, cols=cols))
    np.testing.assert_allclose(_np(out[:RB_M]), want, **_tol(epi, RB_K))
    assert _untouched(out[RB_M:])


@pytest.mark.parametrize("epi", [RESID, SWIGLU, ROPE], ids=lambda e: EPI_NAME[e])
@pytest.mark.parametrize("variant", [0, 9, 12, 3])
def test_row_bias_is_refused_where_no_epilogue_adds_it(variant, epi):
    d = _gemm_dev(RB_M, RB_N, RB_K)
    cols = RB_N // 2 if epi == SWIGLU else RB_N
    out = _sentinel((_pad(RB_M), cols), _out_dtype(epi))
    resid = _dev(R.rand_f32((_pad(RB_M), cols), 33)) if epi == RESID else None
    _launch(d, RB_M, epi, out, variant, resid=resid)                      # (the same call without the table is legal)
    assert not _untouched(out[:RB_M])
    out = _sentinel((_pad(RB_M), cols), _out_dtype(epi))
    _refused(lambda: _launch(d, RB_M, epi, out, variant, resid=resid, rowbias=_dev(_rowbias(256)), rowbias_period=256,
                             rowbias_ld=RB_LD, rowbias_cols=64), out)


# ------------------------------------------------------------------------- column scale ---
@pytest.mark.parametrize("rb", [None, (256, 64), (100, 96)], ids=["norowbias", "rb256x64", "rb100x96"])
@pytest.mark.parametrize("col_scale_n", [64, 128, 256])
@pytest.mark.parametrize("variant", [0, 9, 12, 3])
def test_column_scale(variant, col_scale_n, rb):
    """GemmArgs::col_scale (the ViT's q columns): bf16((acc + bias [+ row bias]) * 0.17) for n < col_scale_n, the rest
    unscaled; with a row bias the general epilogue's per-column form (and the descriptor form on variant 12 for (256, 64))."""
    M, N, K = 300, 256, 128
    c, d = _gemm_case(M, N, K), _gemm_dev(M, N, K)
    kw, ex = dict(col_scale=0.17, col_scale_n=col_scale_n), dict(col_scale=0.17, col_scale_n=col_scale_n)
    if rb:
        t = _rowbias(rb[0])
        kw.update(rowbias=t, period=rb[0], cols=rb[1])
        ex.update(rowbias=_dev(t), rowbias_period=rb[0], rowbias_ld=RB_LD, rowbias_cols=rb[1])
    out = _sentinel((_pad(M), N), torch.bfloat16)
    _launch(d, M, BF16, out, variant, **ex)
    want = _epilogue_ref(c, BF16, kw)
    np.testing.assert_allclose(_np(out[:M]), want, **_tol(BF16, K))
    # ... and the columns past col_scale_n are the unscaled launch's, bit for bit
    plain = _sentinel((_pad(M), N), torch.bfloat16)
    _launch(d, M, BF16, plain, variant, **{k: v for k, v in ex.items() if not k.startswith("col_scale")})
    assert torch.equal(out[:M, col_scale_n:], plain[:M, col_scale_n:])
    if col_scale_n:
        assert not torch.equal(out[:M, :col_scale_n], plain[:M, :col_scale_n])
    assert _untouched(out[M:])


@pytest.mark.parametrize("variant", [0, 9, 12, 3])
def test_column_scale_refusals(variant):
    M, N, K = 300, 256, 128
    d = _gemm_dev(M, N, K)
    for n in (32, -64, 96):                                               # not a non-negative multiple of 64
        out = _sentinel((_pad(M), N), torch.bfloat16)
        _refused(lambda: _launch(d, M, BF16, out, variant, col_scale=0.17, col_scale_n=n), out)
    for epi in (GELU, F32, RESID, SWIGLU, ROPE):                          # only the plain bf16 epilogue scales
        cols = N // 2 if epi == SWIGLU else N
        out = _sentinel((_pad(M), cols), _out_dtype(epi))
        resid = _dev(R.rand_f32((_pad(M), cols), 34)) if epi == RESID else None
        _refused(lambda: _launch(d, M, epi, out, variant, resid=resid, col_scale=0.17, col_scale_n=64), out)


# ------------------------------------------------------------------------------ split K ---
@pytest.mark.parametrize("ksplit", [2, 3, 6])
@pytest.mark.parametrize("variant,N", [(9, 256), (12, 256), (13, 384)])
def test_split_k_planes(variant, N, ksplit):
    """GemmArgs::ksplit / split_stride on the 256-row tiles: plane s = A W^T over its own K range (+ bias on plane 0 only) at
    out + s * split_stride; the gap between the planes and the rows >= M keep the sentinel."""
    M, K = 300, 384
    c, d = _gemm_case(M, N, K), _gemm_dev(M, N, K)
    Mp = _pad(M)
    stride = Mp * N + 64
    buf = _sentinel((ksplit * stride,), torch.float32)
    _launch(d, M, F32, buf, variant, ldo=N, ksplit=ksplit, split_stride=stride)
    want = R.split_planes(c["A"], c["W"], ksplit, c["b"])
    for s in range(ksplit):
        plane = buf[s * stride:s * stride + Mp * N].view(Mp, N)
        np.testing.assert_allclose(_np(plane[:M]), want[s], **_tol(F32, K // ksplit))
        assert _untouched(plane[M:]) and _untouched(buf[s * stride + Mp * N:(s + 1) * stride])
    np.testing.assert_allclose(sum(_np(buf[s * stride:s * stride + Mp * N].view(Mp, N)[:M]) for s in range(ksplit)),
                               R.gemm_acc(c["A"], c["W"], c["b"]), **_tol(F32, K))


def test_split_k_refusals():
    M = 300
    stride = lambda N: _pad(M) * N + 64  # noqa: E731

    def refused(variant, N, K, epi=F32, ksplit=2, **extras):
        d = _gemm_dev(M, N, K)
        cols = N // 2 if epi == SWIGLU else N
        buf = _sentinel((ksplit * stride(N),), _out_dtype(epi))
        resid = _dev(R.rand_f32((_pad(M), cols), 35)) if epi == RESID else None
        _refused(lambda: _launch(d, M, epi, buf, variant, resid=resid, ldo=cols, ksplit=ksplit, split_stride=stride(N), **extras), buf)

    for variant, N in ((9, 256), (12, 256), (13, 384)):
        refused(variant, N, 320)                                          # K % (ksplit * 64) != 0
        rm = _dev(R.row_map(M, M, 23))
        refused(variant, N, 384, rowmap=rm)
        refused(variant, N, 384, rowbias=_dev(_rowbias(256)), rowbias_period=256, rowbias_ld=RB_LD, rowbias_cols=64)
    for variant in (0, 7, 14, 15):                                        # kernels without a split
        refused(variant, 768, 384)
        refused(variant, 768, 384, epi=RESID)
    for variant in (9, 12, 3):
        for epi in (BF16, GELU, RESID, SWIGLU, ROPE):                     # only fp32 planes can be split
            refused(variant, 256, 384, epi=epi)
    refused(13, 384, 384, epi=RESID)


# -------------------------------------------------------------------- device-side row count ---
@pytest.mark.parametrize("m_dev,m_sub", [(0, 0), (1, 0), (256, 0), (257, 0), (700, 0), (300, 43), (900, 200)])
def test_device_side_row_count(m_dev, m_sub):
    """GemmArgs::m_dev / m_sub (the search's band pass) on the 8-wave 256-tile kernel: rows below *m_dev - m_sub hold the
    product, tiles at or past the count are not computed; the rows between the count and the next multiple of 256 are
    unspecified."""
    M, N, K = 700, 256, 64
    c, d = _gemm_case(M, N, K), _gemm_dev(M, N, K)
    out = _sentinel((_pad(M), N), torch.float32)
    _launch(d, M, F32, out, 9, m_dev=torch.tensor([m_dev], dtype=torch.int32, device=DEV), m_sub=m_sub)
    valid, untouched_from = R.rows_left(m_dev - m_sub, M)
    np.testing.assert_allclose(_np(out[:valid]), R.gemm_acc(c["A"], c["W"], c["b"])[:valid], **_tol(F32, K))
    assert _untouched(out[untouched_from:])


@pytest.mark.parametrize("variant,N", [(0, 256), (12, 256), (7, 384), (13, 384)])
def test_device_side_row_count_is_refused_elsewhere(variant, N):
    M, K = 700, 64
    d = _gemm_dev(M, N, K)
    out = _sentinel((_pad(M), N), torch.float32)
    _refused(lambda: _launch(d, M, F32, out, variant, m_dev=torch.tensor([257], dtype=torch.int32, device=DEV)), out)


# ------------------------------------------------------------------------ rasterisation ---
@pytest.mark.parametrize("variant,epi", [(0, BF16), (9, BF16), (12, BF16), (7, BF16), (13, RESID), (14, RESID)],
                         ids=lambda x: str(x))
def test_raster_groups_do_not_change_a_bit(variant, epi):
    """GemmArgs::raster_gm only orders the tiles: any group height gives the bits of the launcher's own choice (5 m-tiles of 256
    rows, 9 of 128: heights 3, 5 and 7 leave a short last group)."""
    M, N, K = 1100, 768, 128
    d = _gemm_dev(M, N, K)
    resid = _dev(R.rand_f32((_pad(M), N), 36)) if epi == RESID else None
    base = _launch(d, M, epi, _sentinel((_pad(M), N), _out_dtype(epi)), variant, resid=resid)
    np.testing.assert_allclose(_np(base[:M]), _epilogue_ref(_gemm_case(M, N, K), epi, {}, None if resid is None else _np(resid[:M])),
                               **_tol(epi, K))
    for gm in (1, 2, 3, 5, 7):
        out = _launch(d, M, epi, _sentinel((_pad(M), N), _out_dtype(epi)), variant, resid=resid, raster_gm=gm)
        assert torch.equal(out.view(torch.int32 if epi == RESID else torch.int16), base.view(torch.int32 if epi == RESID else torch.int16)), gm


# ----------------------------------------------------------------------- the ViT's real pair ---
def _softmax_rows(s):
    p = np.exp(s - s.max(axis=1, keepdims=True))
    return p / p.sum(axis=1, keepdims=True)


def test_vit_pair_scaled_q_columns_then_prescaled_attention():
    """What the ViT runs: the qkv GEMM (one-wave 256-tile kernel) leaves its q columns as bf16((acc + bias) * head_dim^-0.5 *
    log2(e)) — ONE rounding — and attention_w.hip takes them as they are (q_prescaled).  8 heads of 72: D = 576 = 9 x 64, so the
    scaled blocks are exactly the q section."""
    hd, heads, lens = 72, 8, [1024, 300, 65]
    D, T = hd * heads, sum(lens)
    N = _pad(3 * D, 128)                                                   # 1792: the qkv rows, padded like the engine's
    qs = hd ** -0.5 * R.LOG2E
    x = R.rand_bf16((T, D), 41)
    W = np.zeros((N, D), np.float32)
    W[:3 * D] = R.rand_bf16((3 * D, D), 42, D ** -0.5)
    # keys 1.5 times the usual size: rows are carried by few keys (outputs not ~0) while the SECOND rounding of q that the
    # unscaled pair adds (2^-9 of every q element, so a logit error that grows with the keys) stays well inside the tolerance
    W[D:2 * D] = R.bf16_round(W[D:2 * D] * 1.5)
    b = np.zeros(N, np.float32)
    b[:3 * D] = R.rand_f32((3 * D,), 43, 0.2)
    xd, Wd, bd = _dev_bf16(x, _pad(T)), _dev_bf16(W, _pad(N)), _dev(b)
    cu = _dev(np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))

    def qkv(scaled):
        out = _sentinel((_pad(T), N), torch.bfloat16)
        op_gemm_ex(xd, Wd, T, N, BF16, out, bias=bd, variant=12, col_scale=qs if scaled else 0.0, col_scale_n=D if scaled else 0)
        want = R.gemm_acc(x, W, b, col_scale=qs, col_scale_n=D if scaled else 0)
        np.testing.assert_allclose(_np(out[:T]), want, **_tol(BF16, D))
        assert _untouched(out[T:])
        return out

    def attend(t, prescaled):
        att = _sentinel((T, D), torch.bfloat16)
        op_attention_ex(t[:, :D], t[:, D:2 * D], t[:, 2 * D:3 * D], att, cu, cu, heads, hd, max(lens), False, False, hd ** -0.5,
                        q_prescaled=prescaled)
        return _np(att)

    scaled, plain = qkv(True), qkv(False)
    got = attend(scaled, 1)
    h_scaled = _np(scaled[:T])                                             # the attention's own inputs: q rounded ONCE, by the GEMM
    lo = 0
    for L in lens:
        for h in range(heads):
            q, k, v = (h_scaled[lo:lo + L, o + h * hd:o + (h + 1) * hd] for o in (0, D, 2 * D))
            ref = _softmax_rows(q @ k.T * math.log(2.0)) @ v
            np.testing.assert_allclose(got[lo:lo + L, h * hd:(h + 1) * hd], ref, rtol=2e-2, atol=2e-2)
        lo += L
    assert np.median(np.abs(got)) > 0.1
    # the same tensors through the unscaled GEMM and a kernel that scales (and rounds) q itself
    np.testing.assert_allclose(attend(plain, 0), got, rtol=2e-2, atol=2e-2)


@pytest.mark.parametrize("lens", [[130, 68], [68, 13, 80]], ids=["tiled", "short"])
def test_prescaled_q_on_the_kernels_that_scale_scores(lens):
    """q_prescaled on a shape attention_w.hip does not take (head_dim 64, causal): launch_attention hands the other kernels the
    scale that makes their own factor 1."""
    hd, heads = 64, 2
    T, Wd = sum(lens), heads * hd
    qkv = R.rand_bf16((T, 3 * Wd), 44)
    qkv[:, Wd:2 * Wd] = R.bf16_round(qkv[:, Wd:2 * Wd] * 3.0)
    qkv[:, :Wd] = R.bf16_round(qkv[:, :Wd] * np.float32(hd ** -0.5 * R.LOG2E))       # the one rounding
    d = _dev_bf16(qkv)
    cu_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cu = _dev(cu_h)
    for cu_kv in (cu, cu.clone()):                 # (the same buffer twice: the one-wave-per-sequence kernel where it fits)
        att = _sentinel((T, Wd), torch.bfloat16)
        op_attention_ex(d[:, :Wd], d[:, Wd:2 * Wd], d[:, 2 * Wd:], att, cu, cu_kv, heads, hd, max(lens), True, False, hd ** -0.5,
                        q_prescaled=1)
        got = _np(att)
        for b in range(len(lens)):
            lo, hi = cu_h[b], cu_h[b + 1]
            for h in range(heads):
                ref = R.attn_range(qkv[lo:hi, h * hd:(h + 1) * hd], qkv[lo:hi, Wd + h * hd:Wd + (h + 1) * hd],
                                   qkv[lo:hi, 2 * Wd + h * hd:2 * Wd + (h + 1) * hd], math.log(2.0), causal_from=0)[0]
                np.testing.assert_allclose(got[lo:hi, h * hd:(h + 1) * hd], ref, rtol=2e-2, atol=2e-2)


# ------------------------------------------------------- grouped-query attention and ranges ---
LSE_ATOL = 4e-3     # a row's weights lose at most one bf16 rounding each (2^-9 relative), so does their sum: 2^-9 * log2(e) = 2.8e-3


def test_kv_group_prefill_form():
    """AttnArgs::kv_group: query head h reads K / V head h / kv_group (4 query heads on 2 KV heads, head_dim 128, causal)."""
    hd, heads, grp, lens = 128, 4, 2, [130, 1]
    T = sum(lens)
    q = R.rand_bf16((T, heads * hd), 51)
    k = R.rand_bf16((T, heads // grp * hd), 52, R.KEY_GAIN)
    v = R.rand_bf16((T, heads // grp * hd), 53)
    cu_h = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    cu = _dev(cu_h)
    att = _sentinel((T, heads * hd), torch.bfloat16)
    op_attention_ex(_dev_bf16(q), _dev_bf16(k), _dev_bf16(v), att, cu, cu.clone(), heads, hd, max(lens), True, False, hd ** -0.5,
                    kv_group=grp)
    got = _np(att)
    for b in range(len(lens)):
        lo, hi = cu_h[b], cu_h[b + 1]
        for h in range(heads):
            hk = h // grp
            ref = R.attn_range(q[lo:hi, h * hd:(h + 1) * hd], k[lo:hi, hk * hd:(hk + 1) * hd], v[lo:hi, hk * hd:(hk + 1) * hd],
                               hd ** -0.5, causal_from=0)[0]
            np.testing.assert_allclose(got[lo:hi, h * hd:(h + 1) * hd], ref, rtol=2e-2, atol=2e-2)


def _decode_attention(group, n_rows):
    """The generator's decode form on launch_args_ref's inputs: (part bf16 [n * 16 * group][KV * 128], lse f32
    [n * 16 * group][KV], the host inputs, the ranges).  n_rows 1: q_shared over one cache (cu_kv); else the batched form
    (q_in_rows, cu_kv / kv_end into n different caches)."""
    KV, HD, S16 = R.KV_HEADS, R.HD, R.GEN_ATT_SPLITS
    H = KV * group
    q, k, v = R.decode_case(group, 300 + group, n_rows=n_rows)
    kd, vd = _dev_bf16(k.reshape(-1, KV * HD)), _dev_bf16(v.reshape(-1, KV * HD))
    qd = _dev_bf16(q.reshape(-1, HD))                                      # 128-wide rows: row r's heads start at r * H
    items = n_rows * S16
    part = _sentinel((items * group, KV * HD), torch.bfloat16)
    lse = _sentinel((items * group, KV), torch.float32)
    cu_q = _dev((np.arange(items + 1) * group).astype(np.int32))           # as GenBatch lays it out
    common = dict(heads=KV, hd=HD, max_q=group, causal=False, scale=HD ** -0.5, ldq=HD, q_head_stride=group * HD, lse=lse)
    if n_rows == 1:
        lo, hi = R.range_bounds(R.RANGE_LENS)
        cu_kv = _dev(np.concatenate([lo, hi[-1:]]).astype(np.int32))
        op_attention_ex(qd, kd, vd, part, cu_q, cu_kv, q_shared=True, **common)
        counts = [sum(1 for x in R.RANGE_LENS if x > 0)]
    else:
        lo, hi, counts = R.batch_ranges(R.BATCH_LENS[:n_rows])
        q_in = _dev((np.repeat(np.arange(n_rows), S16) * H).astype(np.int32))
        op_attention_ex(qd, kd, vd, part, cu_q, _dev(lo), q_shared=False, B=items, kv_end=_dev(hi), q_in_rows=q_in, **common)
    return part, lse, (q, k, v), (lo, hi, counts)


def _check_ranges(group, n_rows, part, lse, qkv, ranges):
    """per-range outputs and lse against the reference; an empty range has written neither"""
    KV, HD, S16 = R.KV_HEADS, R.HD, R.GEN_ATT_SPLITS
    q, k, v = qkv
    lo, hi, _ = ranges
    wholes = []
    for r in range(n_rows):
        a = lo[r * S16:(r + 1) * S16] - r * R.CACHE_ROWS
        b = hi[r * S16:(r + 1) * S16] - r * R.CACHE_ROWS
        outs, lses, whole = R.decode_ref(q[r], k[r], v[r], group, a, b)
        wholes.append(whole)
        for t in range(S16):
            rows = slice((r * S16 + t) * group, (r * S16 + t + 1) * group)
            if outs[t] is None:
                assert _untouched(part[rows]) and _untouched(lse[rows]), (r, t)
                continue
            np.testing.assert_allclose(_np(part[rows]).reshape(group, KV, HD), outs[t], rtol=2e-2, atol=2e-2)
            np.testing.assert_allclose(_np(lse[rows]), lses[t], rtol=0, atol=LSE_ATOL)
    return wholes


@pytest.mark.parametrize("n_rows", [1, 3], ids=["shared_q", "batched"])
@pytest.mark.parametrize("group", [1, 4, 7])
def test_decode_ranges_and_their_merge(group, n_rows):
    """The generator's decode step: the `group` query heads of a KV head as the rows of a tile (q_head_stride), 16 KV ranges
    per sequence as batch items (lengths 1, 63, 64, 65, ..., 0), lse out — (a) one sequence, q_shared; (b) three sequences,
    q_in_rows and cu_kv / kv_end into three caches.  Then launch_attn_combine merges the first S ranges (S < 16; by value for
    one row, per row from the device for three) into attention over the whole cache."""
    H = R.KV_HEADS * group
    part, lse, qkv, ranges = _decode_attention(group, n_rows)
    wholes = _check_ranges(group, n_rows, part, lse, qkv, ranges)
    counts = ranges[2]
    assert max(counts) < R.GEN_ATT_SPLITS
    ld_out = H * R.HD + (64 if n_rows > 1 else 0)
    out = _sentinel((n_rows, ld_out), torch.bfloat16)
    if n_rows == 1:
        op_attn_combine(part, lse, H, group, out, S=counts[0], ld_out=ld_out)
    else:
        op_attn_combine(part, lse, H, group, out, S_dev=_dev(np.asarray(counts, np.int32)), n_rows=n_rows, ld_out=ld_out)
    for r in range(n_rows):
        np.testing.assert_allclose(_np(out[r, :H * R.HD]).reshape(H, R.HD), wholes[r], rtol=2e-2, atol=2e-2)
    assert _untouched(out[:, H * R.HD:])


@pytest.mark.parametrize("group,ksplit", [(1, 1), (1, 2), (4, 4), (4, 8)])
def test_merge_fused_into_the_o_projection(group, ksplit):
    """gemm_skinny.hip's SkinnyCombine form: the merged row never reaches memory — it is built as the A row of merged @ W^T
    (fp32 planes, at most four K-steps per split).  Reference: the fp64 merge of the SAME partial rows, rounded to bf16 like
    the kernel's A row."""
    H = R.KV_HEADS * group
    K, N = H * R.HD, 256
    part, lse, _, ranges = _decode_attention(group, 1)
    S = ranges[2][0]
    Wh = R.rand_bf16((N, K), 61, 0.1)
    Wd = _dev_bf16(Wh, _pad(N))
    planes = _sentinel((ksplit, 16, N), torch.float32)
    op_attn_combine(part, lse, H, group, planes, S=S, W=Wd, M=1, N=N, K=K, ksplit=ksplit, planes=ksplit, ldo=N, split_stride=16 * N)
    p, l = _np(part).reshape(R.GEN_ATT_SPLITS, group, R.KV_HEADS, R.HD)[:S], _np(lse).reshape(R.GEN_ATT_SPLITS, group, R.KV_HEADS)[:S]
    a_row = R.bf16_round(R.merged_to_heads(R.merge_ranges(list(p), list(l))).reshape(-1).astype(np.float32)).astype(np.float64)
    got = _np(planes[:, 0]).sum(axis=0)
    np.testing.assert_allclose(got, a_row @ np.asarray(Wh, np.float64).T, rtol=1e-5, atol=1e-4 * max(1.0, K / 512))
    per = (K // 64 + ksplit - 1) // ksplit * 64
    for s in range(ksplit):                                               # each plane is its own K range of the same row
        np.testing.assert_allclose(_np(planes[s, 0]), a_row[s * per:(s + 1) * per] @ np.asarray(Wh, np.float64)[:, s * per:(s + 1) * per].T,
                                   rtol=1e-5, atol=1e-4 * max(1.0, K / 512))
    assert _untouched(planes[:, 1:])


def test_fused_merge_refusals():
    """launch_gemm_skinny's own limits for the combine form: one row, K = heads * 128, at most four K-steps per split."""
    group = 1
    H = R.KV_HEADS * group
    K, N = H * R.HD, 256
    part = _sentinel((R.GEN_ATT_SPLITS * group, R.KV_HEADS * R.HD), torch.bfloat16)
    lse = _sentinel((R.GEN_ATT_SPLITS * group, R.KV_HEADS), torch.float32)
    Wd = _dev_bf16(R.rand_bf16((N, 2 * K), 62, 0.1), _pad(N))
    for kw in (dict(M=2, K=K), dict(M=1, K=2 * K), dict(M=1, K=K // 2)):
        planes = _sentinel((2, 16, N), torch.float32)
        _refused(lambda: op_attn_combine(part, lse, H, group, planes, S=3, W=Wd, N=N, ksplit=1, planes=2, ldo=N, split_stride=16 * N, **kw),
                 planes)
    # 8 heads are 16 K-steps: two splits would need eight stages each
    part8 = _sentinel((R.GEN_ATT_SPLITS * 4, R.KV_HEADS * R.HD), torch.bfloat16)
    lse8 = _sentinel((R.GEN_ATT_SPLITS * 4, R.KV_HEADS), torch.float32)
    W8 = _dev_bf16(R.rand_bf16((N, 8 * R.HD), 63, 0.1), _pad(N))
    planes = _sentinel((2, 16, N), torch.float32)
    _refused(lambda: op_attn_combine(part8, lse8, 8, 4, planes, S=3, W=W8, M=1, N=N, K=8 * R.HD, ksplit=2, planes=2, ldo=N,
                                     split_stride=16 * N), planes)
