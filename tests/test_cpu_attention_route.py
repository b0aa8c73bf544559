"""vr_op_attention_route on made-up addresses: which kernel a bf16 attention launch reaches, at every switch of
launch_attention (csrc/attention.hip), attention_small_ok (attention_small.hip) and attention72w_ok (attention_w.hip).  The entry
compares pointers and strides and dereferences none, so it runs here, without a GPU; launch_attention dispatches on the same
function (attention_route), so what is pinned here is what a launch does."""
import pytest

from tests.gpu_util import ROUTE_72W, ROUTE_NONE, ROUTE_REFUSED, ROUTE_SMALL, op_attention_route, route_tiled

BASE = 0x7F0000000000          # a made-up, 16-byte aligned "device address"
CU_A, CU_B, OUT, OTHER = BASE + 0x1000, BASE + 0x2000, BASE + 0x100000, BASE + 0x40000000
KV_END, Q_IN, LSE = BASE + 0x3000, BASE + 0x4000, BASE + 0x5000


def route(hd, max_q, heads=2, same_cu=False, ld=None, B=3, **kw):
    """q | k | v as columns of the same rows (row pitch ld = 3 W unless given), like every self-attention of the engine"""
    W = heads * hd
    ld = ld or 3 * W
    args = dict(q=BASE, ldq=ld, k=BASE + 2 * W, ldk=ld, v=BASE + 4 * W, ldv=ld, out=OUT, ldo=W, cu_q=CU_A, cu_kv=CU_A if same_cu else CU_B,
                B=B, heads=heads, hd=hd, max_q=max_q)
    args.update(kw)
    return op_attention_route(**args)


@pytest.mark.parametrize("hd", [64, 72, 80])
def test_tiled_forms_switch_at_64_and_128(hd):
    for max_q, qf, pipe in ((1, 1, 0), (64, 1, 0), (65, 2, 0), (128, 2, 0), (129, 2, 3), (191, 2, 3), (4096, 2, 3)):
        assert route(hd, max_q, causal=True) == route_tiled(hd, qf, pipe), max_q
        if hd != 72 or max_q < 192:         # (72 non-causal in nearly full 256-row tiles is attention_w.hip's: below)
            assert route(hd, max_q) == route_tiled(hd, qf, pipe), max_q


@pytest.mark.parametrize("max_q", [1, 64, 65, 128, 129, 240, 5000])
def test_head_dim_128_has_one_form(max_q):
    assert route(128, max_q) == route_tiled(128, 1, 0)
    assert route(128, max_q, causal=True, kv_group=2, q_shared=True, lse=LSE, kv_end=KV_END, q_in_rows=Q_IN, q_head_stride=512) == \
        route_tiled(128, 1, 0)


def test_nothing_to_do_and_refusals():
    assert route(64, 0) == ROUTE_NONE and route(64, -1) == ROUTE_NONE and route(64, 64, B=0) == ROUTE_NONE
    assert route(96, 64) == ROUTE_REFUSED and route(0, 64) == ROUTE_REFUSED                  # a head_dim nobody implements
    assert route(96, 0) == ROUTE_NONE                                                          # (an empty launch asks nothing)
    for bad in (dict(ldq=3 * 128 + 4), dict(ldk=3 * 128 + 4), dict(ldv=3 * 128 + 4), dict(ldo=130)):
        assert route(64, 64, **bad) == ROUTE_REFUSED, bad
    assert route(64, 64, ldo=132) == route_tiled(64, 1, 0)                                    # out rows: 8-byte stores
    for null in ("q", "k", "v", "out", "cu_q", "cu_kv"):                                       # vr_op_attention_ex refuses these
        assert route(64, 64, **{null: None}) == ROUTE_REFUSED, null


def test_small_kernel_up_to_80_rows_of_one_cu_buffer():
    for causal in (False, True):
        assert route(64, 1, same_cu=True, causal=causal) == ROUTE_SMALL
        assert route(64, 80, same_cu=True, causal=causal, heads=5) == ROUTE_SMALL
        assert route(64, 81, same_cu=True, causal=causal) == route_tiled(64, 2, 0)
        # cu_q and cu_kv in different buffers (even with equal contents) are a cross-attention as far as the launch can tell
        assert route(64, 80, same_cu=False, causal=causal) == route_tiled(64, 2, 0)
        assert route(64, 64, same_cu=False, causal=causal) == route_tiled(64, 1, 0)
    assert route(72, 80, same_cu=True) == route_tiled(72, 2, 0) and route(80, 80, same_cu=True) == route_tiled(80, 2, 0)
    # every extra sends it to the tiled kernel, which honours them; q_prescaled is honoured by the small kernel (through the scale)
    for extra in (dict(lse=LSE), dict(kv_end=KV_END), dict(q_in_rows=Q_IN), dict(q_head_stride=128), dict(kv_group=2), dict(q_shared=True)):
        assert route(64, 80, same_cu=True, **extra) == route_tiled(64, 2, 0), extra
    assert route(64, 80, same_cu=True, kv_group=1) == ROUTE_SMALL and route(64, 80, same_cu=True, q_prescaled=1) == ROUTE_SMALL


# attention72w_ok: max_q >= 192 and at most 1/8 of the 256-row query tiles wasted
W72_SWITCHES = [(191, False), (192, False), (223, False), (224, True), (256, True), (257, False), (447, False), (448, True), (512, True),
                (513, False), (671, False), (672, True), (1024, True), (1025, False)]


@pytest.mark.parametrize("max_q,taken", W72_SWITCHES)
def test_72w_needs_nearly_full_256_row_tiles(max_q, taken):
    other = route_tiled(72, 2, 3)
    assert route(72, max_q) == (ROUTE_72W if taken else other)
    assert route(72, max_q, same_cu=True, q_prescaled=1, heads=16) == (ROUTE_72W if taken else other)
    assert route(64, max_q) == route_tiled(64, 2, 3) and route(80, max_q) == route_tiled(80, 2, 3)


def test_the_192_row_floor_never_decides():
    """attention72w_ok asks for max_q >= 192 AND at most 1/8 of the tiles wasted; the second is the stricter one everywhere
    ((256 - 223) * 8 = 264 > 256): the first tile's window is 224..256, not 192..256"""
    taken = [m for m in range(1, 300) if route(72, m) == ROUTE_72W]
    assert taken == list(range(224, 257))


@pytest.mark.parametrize("max_q", [224, 256, 448])
def test_72w_preconditions(max_q):
    W = 2 * 72
    tiled = route_tiled(72, 2, 3)
    assert route(72, max_q) == ROUTE_72W
    assert route(72, max_q, ld=3 * W + 32, q=BASE + 16, k=BASE + 2 * (W + 16), v=BASE + 2 * (2 * W + 24)) == ROUTE_72W     # the arena's columns
    # v in another allocation (in front of k or a row or more behind it), or overlapping k's heads: k and v are not columns of one row
    assert route(72, max_q, v=OTHER) == tiled and route(72, max_q, v=BASE - 4 * W) == tiled
    assert route(72, max_q, v=BASE + 2 * W + 2 * 3 * W) == tiled                              # exactly one row behind k
    assert route(72, max_q, v=BASE + 2 * W + 2 * 3 * W - 16) == ROUTE_72W                     # the last 16-byte step inside the row
    assert route(72, max_q, v=BASE + 2 * W + 2 * W - 16) == tiled and route(72, max_q, v=BASE + 2 * W) == tiled
    # one row stride for both
    assert route(72, max_q, ldv=3 * W + 8) == tiled and route(72, max_q, ldk=3 * W + 8) == tiled
    assert route(72, max_q, ldq=3 * W + 8) == ROUTE_72W                                        # q may live elsewhere
    # causal, a shared q, ranges of a cache, and every other extra: attention.hip's
    for extra in (dict(causal=True), dict(q_shared=True), dict(kv_end=KV_END), dict(q_in_rows=Q_IN), dict(q_head_stride=72), dict(kv_group=2),
                  dict(lse=LSE)):
        assert route(72, max_q, **extra) == tiled, extra
    assert route(72, max_q, kv_group=1) == ROUTE_72W
