"""vr_op_gemm_route on made-up sizes: the variant a GEMM launch reaches.  The entry does host arithmetic on the shape and compares
the pointers of the extras with NULL, so it runs here, without a GPU; launch_gemm dispatches on the same function (gemm_route,
csrc/gemm.hip), so what is pinned here is what a launch does.

The rule for the residual GEMMs whose N is a multiple of both 192 and 288 (1152: the ViT's attention projection and fc2): the
one-wave kernel's 256x288 tile (16) or its 256x192 tile (13), whichever takes fewer rounds of the 256 CUs x tile columns, ties to
288."""
import ctypes as C

import pytest

from visrag_amd import _lib

BF16, GELU, F32, RESID, SWIGLU, ROPE = 0, 1, 2, 3, 4, 5
AUTO, REFUSED = 3, -1
ADDR = 0x7F0000001000           # a made-up "device address": compared with NULL, never dereferenced


def route(M, N, K, epi, variant=AUTO, lda=None, ldw=None, ldo=None, warm_bytes=0, **extras):
    ex = _lib.VRGemmExtras(**extras)
    return int(_lib.load().vr_op_gemm_route(M, N, K, epi, variant, lda or K, ldw or K, ldo or N, C.byref(ex), warm_bytes))


def cost(M, cols, N=1152):
    """rounds of 256 CUs x tile columns"""
    tiles = -(-M // 256) * (N // cols)
    return -(-tiles // 256) * cols


@pytest.mark.parametrize("M,want", [(32768, 16), (16384, 16), (10260, 13), (4096, 13)])
@pytest.mark.parametrize("K", [1152, 4352])
def test_n1152_residual_by_rounds_times_columns(M, want, K):
    assert (16 if cost(M, 288) <= cost(M, 192) else 13) == want          # 2x288 = 3x192 (tie), 288 < 384, 288 > 192, 288 > 192
    assert route(M, 1152, K, RESID) == want
    # the same launch asked for by number reaches that number
    assert route(M, 1152, K, RESID, variant=16) == 16 and route(M, 1152, K, RESID, variant=13) == 13


def test_the_tie_goes_to_288_and_the_rule_is_not_one_shape():
    assert cost(32768, 288) == cost(32768, 192) == 576
    assert route(32768, 1152, 1152, RESID) == 16
    assert route(32768 + 1, 1152, 1152, RESID) == 13                   # 129 row tiles: 3 x 288 against 4 x 192
    assert cost(32769, 288) == 864 and cost(32769, 192) == 768
    assert route(65536, 1152, 1152, RESID) == 16 and cost(65536, 288) == 1152 == cost(65536, 192)
    # N = 576 = 2 x 288 = 3 x 192 is either tile's by number; the entry asks N % 128 == 0 of the engine's choice
    assert route(16384, 576, 1152, RESID) == REFUSED
    assert route(16384, 576, 1152, RESID, variant=16) == 16 and route(16384, 576, 1152, RESID, variant=13) == 13


def test_small_m_is_unchanged():
    # M <= 4095 never reaches the N % 192 rule: the 128^2 / 256^2 choice of every other shape
    for M in (4095, 2048, 300):
        got = route(M, 1152, 1152, RESID)
        assert got in (0, 9, 12) and got == route(M, 1152, 1152, F32), M


def test_other_n_go_where_they_went():
    assert route(32768, 384, 1152, RESID) == 13                         # N % 192 == 0, not % 288
    assert route(32768, 1536, 1152, RESID) == 12                        # N % 256 == 0: the 256^2 tile
    assert route(32768, 1536, 1152, F32) == 12
    assert route(32768, 384, 1152, RESID, rowmap=ADDR) == 7             # a row map: the 8-wave 256x192 kernel
    assert route(32768, 1152, 1152, RESID, rowmap=ADDR) == 7


@pytest.mark.parametrize("epi", [BF16, GELU, F32, SWIGLU, ROPE])
@pytest.mark.parametrize("M", [32768, 16384, 4096, 300])
def test_other_epilogues_never_reach_16(epi, M):
    assert route(M, 1152, 1152, epi) not in (16, REFUSED)
    assert route(M, 1152, 1152, epi, variant=16) == REFUSED


def test_what_16_refuses():
    ok = dict(M=300, N=576, K=128, epi=RESID, variant=16)
    assert route(**ok) == 16
    assert route(**{**ok, "N": 384}) == REFUSED and route(**{**ok, "N": 1152 + 128}) == REFUSED
    assert route(**{**ok, "K": 96}) == REFUSED and route(**{**ok, "M": 0}) == REFUSED
    for extra in (dict(rowmap=ADDR), dict(rowbias=ADDR, rowbias_period=256, rowbias_ld=576, rowbias_cols=64), dict(ksplit=2),
                  dict(col_scale=0.5, col_scale_n=64), dict(m_dev=ADDR)):
        assert route(**ok, **extra) == REFUSED, extra
    assert route(**ok, warm_bytes=4096) == REFUSED
    assert route(**ok, raster_gm=2) == 16 and route(**ok, ksplit=1) == 16     # the order of the tiles is the caller's to choose
    # AUTO is judged as the variant it lands on: neither 16 nor 13 takes a region to warm
    assert route(32768, 1152, 1152, RESID, warm_bytes=4096) == REFUSED
    assert route(32768, 1152, 1152, 99) == REFUSED and route(32768, 1152, 1152, RESID, variant=5) == REFUSED
