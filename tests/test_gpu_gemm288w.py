"""-m gpu: the 256x288 tile of the one-wave GEMM (variant 16) through vr_op_gemm_ex / vr_op_gemm_warm.

The yardstick needs no tolerance: every output element accumulates its K-steps in the same order and through the same MFMA as on
the 256x192 tile (variant 13), and leaves through the same expression resid + alpha * (acc + bias).  So variant 16 must be
torch.equal to variant 13 on the same inputs.  (Variant 13 itself is held to the fp64 reference by tests/test_gpu_launch_args.py;
one loose comparison with a float64 product here only guards against the two being wrong together.)

Shapes, the smallest at which each mechanism can go wrong:
  (256, 576, 64)      one K-step: both prefetched steps point out of range; two tile columns
  (300, 576, 128)     two K-steps (one whole pair of the loop), a second row tile with 44 valid rows
  (515, 1152, 192)    an odd step count (the step behind the loop's pairs), 3 row tiles x 4 columns: raster groups and the XCD remap
  (300, 1152, 4352)   fc2's depth
  (4133, 1152, 1152)  17 x 4 tiles: more than one XCD block, a last raster group of one row tile
  N = 288 alone       a single tile column: W = the first 288 rows of an N = 576 case, against the first 288 columns of variant 13's
Rows >= M of the sentinel-filled output must stay untouched.  What the variant does not take is refused with VR_ERR_INVALID
(status 1) before anything runs."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_util import P, op_gemm_ex  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd._lib import VisragHipError  # noqa: E402

DEV = "cuda:0"
BF16, GELU, F32, RESID, SWIGLU, ROPE = range(6)
SENT, SENT_BF16 = -77.25, 7.0        # exact in their formats, far from every output here
SHAPES = [(256, 576, 64), (300, 576, 128), (515, 1152, 192), (300, 1152, 4352), (4133, 1152, 1152)]


def _pad(n, mult=256):
    return (n + mult - 1) // mult * mult


@functools.lru_cache(maxsize=None)
def _inputs(M, N, K):
    """device operands of one shape, shared and never modified; A's rows padded with zeros to the tile"""
    g = torch.Generator(device=DEV).manual_seed(1000 * M + N + K)
    A = torch.zeros((_pad(M), K), dtype=torch.bfloat16, device=DEV)
    A[:M] = torch.randn((M, K), generator=g, device=DEV).to(torch.bfloat16)
    W = (torch.randn((N, K), generator=g, device=DEV) * 0.1).to(torch.bfloat16)
    bias = torch.randn((N,), generator=g, device=DEV)
    resid = torch.full((_pad(M), N), SENT, device=DEV)
    resid[:M] = torch.randn((M, N), generator=g, device=DEV)
    return dict(A=A, W=W, bias=bias, resid=resid)


def _run(d, M, N, variant, with_bias, alpha, in_place, cols=None):
    """out [pad(M)][cols] after one launch; rows >= M hold the sentinel before it.  cols < N: the first tile columns only."""
    cols = cols or N
    W, bias = d["W"][:cols], (d["bias"][:cols].contiguous() if with_bias else None)
    resid = d["resid"][:, :cols].clone(memory_format=torch.contiguous_format)       # (a copy: in place, the launch writes into it)
    out = resid if in_place else torch.full_like(resid, SENT)
    op_gemm_ex(d["A"], W, M, cols, RESID, out, bias=bias, resid=resid, alpha=alpha, variant=variant)
    return out


@functools.lru_cache(maxsize=None)
def _want(M, N, K, with_bias, alpha):
    """variant 13, out of place: the bits variant 16 must give"""
    return _run(_inputs(M, N, K), M, N, 13, with_bias, alpha, False)


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_equals_the_192_column_tile(M, N, K, with_bias, alpha, in_place):
    d = _inputs(M, N, K)
    want = _want(M, N, K, with_bias, alpha)
    got = _run(d, M, N, 16, with_bias, alpha, in_place)
    assert _bits_equal(got[:M], want[:M])
    assert bool((got[M:] == SENT).all()) and bool((want[M:] == SENT).all())          # rows >= M: untouched
    assert not bool((want[:M] == SENT).any())                                         # ... and every row < M written


@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no_bias"])
@pytest.mark.parametrize("M,N,K", SHAPES[:2])
def test_one_tile_column(M, N, K, with_bias, alpha, in_place):
    d = _inputs(M, N, K)
    want = _want(M, N, K, with_bias, alpha)[:, :288]
    got = _run(d, M, N, 16, with_bias, alpha, in_place, cols=288)
    assert _bits_equal(got[:M], want[:M])
    assert bool((got[M:] == SENT).all())


@pytest.mark.parametrize("M,N,K", SHAPES[:3])
def test_both_tiles_near_a_float64_product(M, N, K):
    """(not the yardstick: both tiles wrong in the same way would pass the comparison above)  fp32 outputs of bf16 products:
    the bound tests/test_gpu_ops.py states for this epilogue, rtol 1e-5, atol 1e-4 * max(1, K / 512)"""
    d = _inputs(M, N, K)
    ref = d["resid"][:M].double() + 0.5 * (d["A"][:M].double() @ d["W"].double().T + d["bias"].double())
    torch.testing.assert_close(_want(M, N, K, True, 0.5)[:M].double(), ref, rtol=1e-5, atol=1e-4 * max(1.0, K / 512))


def test_auto_reaches_it_where_the_route_says_so():
    """16 384 rows of N = 1152: one round of 288-column tiles against two of 192 — AUTO's launch gives the same bits either way,
    so the route query is what tells them apart"""
    ex = _lib.VRGemmExtras()
    lib = _lib.load()
    assert lib.vr_op_gemm_route(16384, 1152, 1152, RESID, 3, 1152, 1152, 1152, C.byref(ex), 0) == 16
    assert lib.vr_op_gemm_route(16384, 1152, 64, RESID, 3, 64, 64, 1152, C.byref(ex), 0) == 16
    assert lib.vr_op_gemm_route(4133, 1152, 1152, RESID, 3, 1152, 1152, 1152, C.byref(ex), 0) == 13
    M, N, K = 16384, 1152, 64
    d = _inputs(M, N, K)
    got = _run(d, M, N, 3, True, 0.5, True)
    assert _bits_equal(got, _run(d, M, N, 13, True, 0.5, False)) and _bits_equal(got, _run(d, M, N, 16, True, 0.5, False))


# ---------------------------------------------------------------------------------- refusals ---
def _refused(fn, *outs):
    """VR_ERR_INVALID (status 1) from the entry, nothing launched: the outputs keep the sentinel"""
    with pytest.raises(VisragHipError, match=r"\(status 1\)"):
        fn()
    torch.cuda.synchronize()
    for out in outs:
        assert bool((out == SENT).all())


def _refusal_case(N=576, dtype=torch.float32):
    """the (300, 576, 128) operands (N < 576: their first rows), a sentinel-filled output and residual"""
    M, K = 300, 128
    d = _inputs(M, 576, K)
    out = torch.full((_pad(M), N), SENT if dtype == torch.float32 else SENT_BF16, dtype=dtype, device=DEV)
    resid = torch.full((_pad(M), N), SENT, dtype=torch.float32, device=DEV)
    return M, d, out, resid


def test_refuses_a_width_off_the_tile():
    M, d, out, resid = _refusal_case(N=384)
    _refused(lambda: op_gemm_ex(d["A"], d["W"], M, 384, RESID, out, bias=d["bias"], resid=resid, alpha=0.5, variant=16), out)


@pytest.mark.parametrize("extra", ["rowmap", "rowbias", "ksplit", "col_scale_n", "m_dev"])
def test_refuses_every_optional_field(extra):
    M, d, out, resid = _refusal_case()
    kw = dict(rowmap=dict(rowmap=torch.arange(M, dtype=torch.int32, device=DEV)),
              rowbias=dict(rowbias=torch.zeros((256, 576), device=DEV), rowbias_period=256, rowbias_cols=64),
              ksplit=dict(ksplit=2, split_stride=_pad(M) * 576),
              col_scale_n=dict(col_scale=0.5, col_scale_n=64),
              m_dev=dict(m_dev=torch.tensor([257], dtype=torch.int32, device=DEV)))[extra]
    _refused(lambda: op_gemm_ex(d["A"], d["W"], M, 576, RESID, out, bias=d["bias"], resid=resid, alpha=0.5, variant=16, **kw), out)


def test_refuses_a_region_to_warm():
    M, d, out, resid = _refusal_case()
    region = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    lib = _lib.load()

    def call():
        _lib.check(lib.vr_op_gemm_warm(0, P(d["A"]), 128, P(d["W"]), 128, M, 576, 128, RESID, P(d["bias"]), P(resid), 0.5, P(out), 576,
                                       None, None, 0, 16, None, P(region), C.c_uint64(4096), None), "vr_op_gemm_warm")
    _refused(call, out)
    assert bool((region == 0).all())


@pytest.mark.parametrize("epi", [BF16, GELU, F32, SWIGLU, ROPE])
def test_refuses_every_other_epilogue(epi):
    dtype = torch.float32 if epi == F32 else torch.bfloat16
    M, d, out, resid = _refusal_case(dtype=dtype)
    rope = dict(rope_pos=torch.zeros(M, dtype=torch.int32, device=DEV), rope_table=torch.zeros((64, 64), device=DEV), rope_cols=128) if epi == ROPE else {}
    with pytest.raises(VisragHipError, match=r"\(status 1\)"):
        op_gemm_ex(d["A"], d["W"], M, 576, epi, out, bias=d["bias"], variant=16, **rope)
    torch.cuda.synchronize()
    assert bool((out == (SENT if dtype == torch.float32 else SENT_BF16)).all())
