"""-m gpu: GemmArgs::warm through vr_op_gemm_warm — a region the one-wave 256-tile GEMM (variant 12) only REQUESTS while it runs,
so that the launch behind it finds the region in the memory-side cache.  A request computes nothing: every output must keep
the bits of the launch without it, the region and its surroundings must stay what they were, and every other variant must
refuse the field before anything runs (the rule of include/visrag_hip.h, vr_op_gemm_ex).  Whether the requests pay is a
timing question: tools/warm_probe.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import launch_args_ref as R  # noqa: E402
from tests.gpu_util import P  # noqa: E402
from visrag_amd import _lib  # noqa: E402
from visrag_amd._lib import VisragHipError  # noqa: E402

DEV = "cuda:0"
BF16, GELU, F32, RESID, SWIGLU, ROPE = range(6)
EPI_NAME = ["bf16", "gelu", "f32", "resid", "swiglu", "rope"]
SENT = {torch.float32: -77.25, torch.bfloat16: 7.0}
GUARD = 4096
MIB = 1 << 20


def op_gemm_warm(A, W, M, N, K, epi, out, ldo, bias=None, resid=None, alpha=1.0, rope_pos=None, rope_table=None, rope_cols=0,
                 variant=12, warm=None, warm_bytes=0):
    """one vr_op_gemm_warm call; `warm` is a device ADDRESS (int) or None"""
    lib = _lib.load()
    _lib.check(lib.vr_op_gemm_warm(0, P(A), A.stride(0), P(W), W.stride(0), M, N, K, epi, P(bias), P(resid), float(alpha), P(out), ldo,
                                   P(rope_pos), P(rope_table), rope_cols, variant, None, C.c_void_p(warm), C.c_uint64(warm_bytes), None),
               "vr_op_gemm_warm")
    torch.cuda.synchronize()
    return out


def _pad(n, mult=256):
    return (n + mult - 1) // mult * mult


def _dev_bf16(x, rows):
    t = torch.from_numpy(np.array(x)).to(torch.bfloat16)
    if rows > t.shape[0]:
        t = torch.cat([t, torch.zeros((rows - t.shape[0], t.shape[1]), dtype=torch.bfloat16)])
    return t.to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _out_dtype(epi):
    return torch.float32 if epi in (F32, RESID) else torch.bfloat16


@functools.lru_cache(maxsize=None)
def _inputs(M, N, K):
    """device operands of one shape, shared and never modified: plain W for epilogues 0..3 and 5, [16 gate | 16 up] interleaved for 4"""
    A, W, b = R.rand_bf16((M, K), 51), R.rand_bf16((N, K), 52, 0.1), R.rand_f32((N,), 53)
    Wi, bi = R.interleave16(W[:N // 2], W[N // 2:]), R.interleave16(b[:N // 2], b[N // 2:])
    dev = lambda x: torch.from_numpy(np.array(x)).to(DEV)  # noqa: E731
    return dict(A=_dev_bf16(A, _pad(M)), W=_dev_bf16(W, _pad(N)), b=dev(b), Wi=_dev_bf16(Wi, _pad(N)), bi=dev(bi),
                pos=dev((np.arange(M) % 50).astype(np.int32)), table=dev(R.rope_table(64)),
                resid=dev(R.rand_f32((_pad(M), N), 54)))


def _launch(d, M, N, K, epi, variant=12, **warm):
    cols = N // 2 if epi == SWIGLU else N
    out = torch.full((_pad(M), cols), SENT[_out_dtype(epi)], dtype=_out_dtype(epi), device=DEV)
    sw, rp = epi == SWIGLU, epi == ROPE
    op_gemm_warm(d["A"], d["Wi"] if sw else d["W"], M, N, K, epi, out, cols, bias=None if rp else (d["bi"] if sw else d["b"]),
                 resid=d["resid"] if epi == RESID else None, alpha=0.2214, rope_pos=d["pos"] if rp else None,
                 rope_table=d["table"] if rp else None, rope_cols=128 if rp else 0, variant=variant, **warm)
    return out


@functools.lru_cache(maxsize=None)
def _region():
    """(buffer, clone): GUARD bytes, 3 MiB + 2 that get warmed, GUARD bytes — one allocation of arbitrary bytes"""
    g = torch.Generator(device="cpu").manual_seed(55)
    buf = torch.randint(0, 256, (GUARD + 3 * MIB + 2 + GUARD,), dtype=torch.uint8, generator=g).to(DEV)
    return buf, buf.clone()


# (offset into the region's allocation behind the front guard, bytes): absent with a pointer, below / at / above one line, one
# wave-instruction (64 lines) and a dword more, several instructions per wave on the four workgroups; then base and end off a dword
WARM_CASES = [(0, 0), (0, 4), (0, 127), (0, 128), (0, 129), (0, 8192 + 4), (0, 3 * MIB), (2, 127), (2, 8192 + 4), (2, 3 * MIB)]


@pytest.mark.parametrize("epi", range(6), ids=EPI_NAME)
def test_warm_changes_no_output_bit_and_no_byte_of_the_region(epi):
    """M = 300, N = 512, K = 192: 2 x 2 tiles with a ragged last row tile, three K-steps, every epilogue of the kernel."""
    M, N, K = 300, 512, 192
    d = _inputs(M, N, K)
    base = _launch(d, M, N, K, epi)
    assert not bool((_bits(base[:M]) == _bits(torch.full((1,), SENT[base.dtype], dtype=base.dtype, device=DEV))).all())
    buf, clone = _region()
    for off, nbytes in WARM_CASES:
        out = _launch(d, M, N, K, epi, warm=buf.data_ptr() + GUARD + off, warm_bytes=nbytes)
        assert torch.equal(_bits(out), _bits(base)), (off, nbytes)
    assert torch.equal(buf, clone)                      # the warmed bytes, and the 4 KiB in front of and behind them
    assert torch.equal(buf[:GUARD], clone[:GUARD]) and torch.equal(buf[-GUARD:], clone[-GUARD:])


def test_warm_on_the_decoder_shape():
    """The decoder's q|k|v + RoPE launch carrying the o projection's weights: M = 2176, N = 6912, K = 2304, 243 workgroups, two
    requests per wave."""
    M, N, K = 2176, 6912, 2304
    g = torch.Generator(device=DEV).manual_seed(56)
    A = torch.randn((_pad(M), K), device=DEV, generator=g).to(torch.bfloat16)
    W = (torch.randn((N, K), device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    Wo = (torch.randn((K, K), device=DEV, generator=g) * 0.05).to(torch.bfloat16)
    Wo_clone = Wo.clone()
    pos = (torch.arange(M, device=DEV, dtype=torch.int32) % 68)
    table = torch.from_numpy(np.array(R.rope_table(68))).to(DEV)
    outs = []
    for warm in (dict(), dict(warm=Wo.data_ptr(), warm_bytes=Wo.numel() * 2)):
        out = torch.full((_pad(M), N), SENT[torch.bfloat16], dtype=torch.bfloat16, device=DEV)
        outs.append(op_gemm_warm(A, W, M, N, K, ROPE, out, N, rope_pos=pos, rope_table=table, rope_cols=2 * K, **warm))
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    assert float(outs[0][:M].float().abs().max()) > 0 and torch.equal(Wo, Wo_clone)


@pytest.mark.parametrize("variant", [0, 7, 9, 13, 14, 15])
def test_warm_is_refused_by_every_other_variant(variant):
    """honoured or refused, never ignored: the launchers return hipErrorInvalidValue (status 2) and nothing is launched"""
    M, N, K = 300, 768, 128
    d = _inputs(M, N, K)
    plain = _launch(d, M, N, K, RESID, variant=variant)             # (the same call without the field is legal)
    assert not torch.equal(_bits(plain[:M]), _bits(torch.full_like(plain[:M], SENT[torch.float32])))
    buf, clone = _region()
    out = torch.full((_pad(M), N), SENT[torch.float32], dtype=torch.float32, device=DEV)
    with pytest.raises(VisragHipError, match=r"\(status 2\): launch_gemm\("):
        op_gemm_warm(d["A"], d["W"], M, N, K, RESID, out, N, bias=d["b"], resid=d["resid"], alpha=0.2214, variant=variant,
                     warm=buf.data_ptr() + GUARD, warm_bytes=8192)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(torch.full_like(out, SENT[torch.float32]))) and torch.equal(buf, clone)
