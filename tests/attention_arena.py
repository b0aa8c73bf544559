"""A guarded arena for the bf16 attention kernels (attention.hip, attention_small.hip, attention_w.hip), pure numpy.

The kernels walk K and V in 64-key tiles that run past a sequence's last row and rely on buffer descriptors, masks and "P is
exactly 0" to make what lies there harmless.  Here q, k and v are views into ONE allocation in which every cell a launch has no
business reading — the guard cells — can be filled with zeros, NaNs or the largest finite bf16:

    rows      16 guard rows | T rows | 256 guard rows          (so every cu starts at 16, and an over-read by a whole tile — or
                                                                a 256-row query tile — stays inside memory the test owns)
    columns   8 | q (Wq) | 8 | k (Wkv) | 8 | v (Wkv) | 8       (ld = Wq + 2 Wkv + 32; every offset a multiple of 8 elements; v - k
                                                                stays inside a row and is Wkv + 8 >= heads * head_dim elements)

`out` is [16 + rows + 256][W + 8] and `lse` [16 + rows + 256][heads], prefilled with the sentinels of test_gpu_launch_args.py.
WHICH cells are data follows from the launch arguments alone: `addresses()` spells out AttnArgs' addressing (csrc/kernels.h) in
flat element offsets, the data masks and the fp64 reference (launch_args_ref.attn_range) are both built from it, and
tests/test_cpu_attention_arena.py checks them against plain slices of the views.  Nothing here needs a GPU or the library."""
import functools
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from tests import launch_args_ref as R

FRONT, BACK, GUTTER = 16, 256, 8
FILLS = ("clean", "nan", "huge")
FILL_BITS = {"clean": (0x0000, 0x0000), "nan": (0x7FC0, 0xFFC0), "huge": (0x7F7F, 0xFF7F)}     # alternating over the cells
SENT_OUT_BITS = 0x40E0          # bf16 7.0
SENT_LSE = np.float32(-77.25)
RTOL = ATOL = 2e-2              # the attention bar of tests/test_gpu_ops.py
LSE_ATOL = 4e-3                 # tests/test_gpu_launch_args.py: one bf16 rounding of a row's weights, 2^-9 log2(e) = 2.8e-3

SMALL, W72 = "small", "72w"


def tiled(hd, qf, pipe):
    return ("tiled", hd, qf, pipe)


def to_bits(x):
    """bf16-valued float32 -> uint16 bit patterns"""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def from_bits(b):
    return (np.ascontiguousarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


@dataclass
class Case:
    """One launch: AttnArgs in arena rows.  cu_* / kv_end / q_in_rows are ABSOLUTE arena rows (q, k, v, out point at row 0 of
    their columns; a shared q points at row 16, as a launch reads it from its own row 0)."""
    name: str
    route: object
    hd: int
    heads: int
    cu_q: np.ndarray
    cu_kv: np.ndarray
    max_q: int
    rows: int                              # T: data rows of the arena
    causal: bool = False
    q_shared: bool = False
    scale: float = 0.0
    same_cu: bool = False                  # cu_q and cu_kv are the SAME device buffer
    kv_group: int = 0
    kv_end: Optional[np.ndarray] = None
    q_in_rows: Optional[np.ndarray] = None
    q_rows_per_head: int = 0               # q_head_stride = this many ROWS of the arena (0: heads side by side in a row)
    q_heads: int = 0                       # width of the q section in heads (0: `heads`)
    kv_heads: int = 0                      # width of the k / v sections in heads (0: `heads`)
    lse: bool = False
    seed: int = 0
    B: int = field(init=False)

    def __post_init__(self):
        self.B = len(self.cu_q) - 1
        self.scale = self.scale or self.hd ** -0.5
        self.cu_q, self.cu_kv = np.asarray(self.cu_q, np.int32), np.asarray(self.cu_kv, np.int32)

    # ---- geometry
    @property
    def Wq(self): return (self.q_heads or self.heads) * self.hd
    @property
    def Wkv(self): return (self.kv_heads or self.heads) * self.hd
    @property
    def Wo(self): return self.heads * self.hd
    @property
    def ld(self): return self.Wq + 2 * self.Wkv + 4 * GUTTER
    @property
    def q_col(self): return GUTTER
    @property
    def k_col(self): return 2 * GUTTER + self.Wq
    @property
    def v_col(self): return 3 * GUTTER + self.Wq + self.Wkv
    @property
    def arena_rows(self): return FRONT + self.rows + BACK
    @property
    def out_rows(self): return FRONT + int(self.cu_q[-1] - FRONT) + BACK
    @property
    def ldo(self): return self.Wo + GUTTER
    @property
    def ldq(self): return self.ld
    @property
    def q_head_stride(self): return self.q_rows_per_head * self.ld
    @property
    def q_row0(self): return FRONT if self.q_shared and self.q_in_rows is None else 0     # the row the q pointer points at

    def kv_range(self, b):
        return int(self.cu_kv[b]), int(self.kv_end[b] if self.kv_end is not None else self.cu_kv[b + 1])

    def live(self, b):
        lo, hi = self.kv_range(b)
        return hi > lo and self.cu_q[b + 1] > self.cu_q[b]


def addresses(c: Case, b: int, h: int, extra_keys=0, col_shift=0):
    """AttnArgs' addressing of item b, head h, as flat element offsets into the arena: (q [nq][hd], k [L][hd], v [L][hd]).
    extra_keys / col_shift: what a kernel that is wrong by that many rows / columns would read instead."""
    d = np.arange(c.hd)
    nq = int(c.cu_q[b + 1] - c.cu_q[b])
    first = int(c.q_in_rows[b]) if c.q_in_rows is not None else (0 if c.q_shared else int(c.cu_q[b]))
    qptr = c.q_row0 * c.ld + c.q_col
    q = qptr + (first + np.arange(nq))[:, None] * c.ldq + h * (c.q_head_stride or c.hd) + d[None, :]
    hkv = h // c.kv_group if c.kv_group > 1 else h
    lo, hi = c.kv_range(b)
    rows = np.arange(lo, hi + extra_keys)
    k = c.k_col + rows[:, None] * c.ld + hkv * c.hd + col_shift + d[None, :]
    v = c.v_col + rows[:, None] * c.ld + hkv * c.hd + col_shift + d[None, :]
    return q, k, v


@dataclass
class Arena:
    case: Case
    bits: np.ndarray            # uint16 [arena_rows][ld], guard cells zero (the clean fill)
    q_mask: np.ndarray          # bool [arena_rows][ld]: the cells each operand's addressing reaches
    k_mask: np.ndarray
    v_mask: np.ndarray
    finite_only: np.ndarray     # guard cells the 72w route reads and multiplies by zero: `huge` in the nan fill too
    out_mask: np.ndarray        # bool [out_rows][ldo]: the cells a launch must write
    lse_mask: np.ndarray        # bool [out_rows][heads]

    @property
    def data(self): return self.q_mask | self.k_mask | self.v_mask
    @property
    def guard(self): return ~self.data

    def filled(self, fill):
        """the arena's bits with every guard cell set to `fill`'s pattern"""
        r, col = np.indices(self.bits.shape)
        odd = ((r + col) & 1).astype(bool)
        pat = lambda f: np.where(odd, np.uint16(FILL_BITS[f][1]), np.uint16(FILL_BITS[f][0]))  # noqa: E731
        out = np.where(self.guard, pat(fill), self.bits)
        if fill == "nan":
            out = np.where(self.finite_only, pat("huge"), out)
        return out.astype(np.uint16)

    def views(self, bits):
        """(q, k, v) as the launch gets them: slices of one array, first row = the row its pointer points at"""
        c = self.case
        return (bits[c.q_row0:, c.q_col:c.q_col + c.Wq], bits[:, c.k_col:c.k_col + c.Wkv], bits[:, c.v_col:c.v_col + c.Wkv])

    def out_sentinels(self):
        c = self.case
        return (np.full((c.out_rows, c.ldo), SENT_OUT_BITS, np.uint16), np.full((c.out_rows, c.heads), SENT_LSE, np.float32))


def _mask_of(c, pick):
    m = np.zeros(c.arena_rows * c.ld, bool)
    for b in range(c.B):
        if c.live(b):
            for h in range(c.heads):
                m[pick(addresses(c, b, h)).ravel()] = True
    return m.reshape(c.arena_rows, c.ld)


def build(c: Case) -> Arena:
    q_mask, k_mask, v_mask = (_mask_of(c, lambda a, i=i: a[i]) for i in range(3))
    assert not (q_mask & k_mask).any() and not (q_mask & v_mask).any() and not (k_mask & v_mask).any()
    vals = np.zeros((c.arena_rows, c.ld), np.float32)
    shape = vals.shape
    vals[q_mask] = R.rand_bf16(shape, 1000 + c.seed)[q_mask]
    vals[k_mask] = R.rand_bf16(shape, 2000 + c.seed, R.KEY_GAIN)[k_mask]      # a few keys carry a row: outputs of the size of v
    vals[v_mask] = R.rand_bf16(shape, 3000 + c.seed)[v_mask]
    finite_only = np.zeros(shape, bool)
    if c.route == W72:
        # attention_w.hip stages a head's 72 columns as 80: the 8 columns behind the LAST head of k and of v, in every key row of an
        # item (the other heads' 8 are the next head's data)
        for b in range(c.B):
            if c.live(b):
                lo, hi = c.kv_range(b)
                finite_only[lo:hi, c.k_col + c.Wkv:c.k_col + c.Wkv + GUTTER] = True
                finite_only[lo:hi, c.v_col + c.Wkv:c.v_col + c.Wkv + GUTTER] = True
    out_mask = np.zeros((c.out_rows, c.ldo), bool)
    lse_mask = np.zeros((c.out_rows, c.heads), bool)
    for b in range(c.B):
        if c.live(b):
            out_mask[c.cu_q[b]:c.cu_q[b + 1], :c.Wo] = True
            lse_mask[c.cu_q[b]:c.cu_q[b + 1], :] = c.lse
    return Arena(c, to_bits(vals), q_mask, k_mask, v_mask, finite_only, out_mask, lse_mask)


def reference(c: Case, bits, extra_keys=0, col_shift=0, causal_shift=0):
    """fp64 attention of the launch on the arena `bits`: (out [out_rows][Wo], lse [out_rows][heads]), NaN where nothing is
    written.  extra_keys, col_shift, causal_shift: the WRONG kernels of tests/test_cpu_attention_arena.py."""
    flat = from_bits(bits).astype(np.float64).ravel()
    out = np.full((c.out_rows, c.Wo), np.nan)
    lse = np.full((c.out_rows, c.heads), np.nan)
    with np.errstate(all="ignore"):
        for b in range(c.B):
            if not c.live(b):
                continue
            for h in range(c.heads):
                qa, ka, va = addresses(c, b, h, extra_keys, col_shift)
                o, l = R.attn_range(flat[qa], flat[ka], flat[va], c.scale, causal_from=causal_shift if c.causal else None)
                out[c.cu_q[b]:c.cu_q[b + 1], h * c.hd:(h + 1) * c.hd] = o
                lse[c.cu_q[b]:c.cu_q[b + 1], h] = l
    return out, lse


def worst_ratio(got, ref, rtol=RTOL, atol=ATOL):
    """max |got - ref| / (atol + rtol |ref|) over the cells where ref is a number; NaN / inf in `got` there counts as inf"""
    m = ~np.isnan(ref)
    if not m.any():
        return 0.0
    with np.errstate(all="ignore"):
        r = np.abs(got[m] - ref[m]) / (atol + rtol * np.abs(ref[m]))
    return float(np.inf if not np.isfinite(r).all() else r.max())


# ------------------------------------------------------------------------------------ cases ---
def _packed(lens):
    return (FRONT + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32)


def _self(name, route, hd, lens, causal=False, heads=2, same_cu=False, seed=0, **kw):
    cu = _packed(lens)
    return Case(name=name, route=route, hd=hd, heads=heads, cu_q=cu, cu_kv=cu.copy(), max_q=max(lens), rows=sum(lens), causal=causal,
                same_cu=same_cu, seed=seed, **kw)


def _lens_id(lens):
    return "_".join(str(x) for x in lens)


def _decode(n_rows, group=4):
    """The inputs of test_gpu_launch_args._decode_attention (the generator's decode step), rebuilt on an arena: the `group` query
    heads of a KV head as the rows of a tile, 16 KV ranges per sequence as items.  Cache r occupies arena rows
    [16 + 333 r, 16 + 333 (r + 1)); cache rows outside every range of their sequence are guards (cache 2 of BATCH_LENS: 200..332)."""
    KV, S16 = R.KV_HEADS, R.GEN_ATT_SPLITS
    H = KV * group
    items = n_rows * S16
    cu_q = (FRONT + np.arange(items + 1) * group).astype(np.int32)
    common = dict(route=tiled(128, 1, 0), hd=R.HD, heads=KV, cu_q=cu_q, max_q=group, rows=n_rows * R.CACHE_ROWS, q_rows_per_head=group,
                  q_heads=1, lse=True, seed=70 + n_rows)
    if n_rows == 1:
        lo, hi = R.range_bounds(R.RANGE_LENS)
        return Case(name="decode_shared_q", cu_kv=FRONT + np.concatenate([lo, hi[-1:]]), q_shared=True, **common)
    lo, hi, _ = R.batch_ranges(R.BATCH_LENS[:n_rows])
    q_in = FRONT + np.repeat(np.arange(n_rows), S16) * H
    return Case(name="decode_batched", cu_kv=np.concatenate([FRONT + lo, [FRONT + hi[-1]]]), kv_end=(FRONT + hi).astype(np.int32),
                q_in_rows=q_in.astype(np.int32), **common)


TILED_LENS = [[64, 1, 63], [65, 64], [128, 127], [129, 65, 1]]


def _tiled_route(hd, lens):
    m = max(lens)
    return tiled(hd, 1, 0) if m <= 64 else tiled(hd, 2, 0) if m <= 128 else tiled(hd, 2, 3)


@functools.lru_cache(maxsize=None)
def cases() -> Tuple[Case, ...]:
    out = []
    seed = 0
    for hd in (64, 72, 80):
        for lens in TILED_LENS:
            for causal in (False, True):
                if causal and hd != 64 and lens != TILED_LENS[-1]:
                    continue
                seed += 1
                out.append(_self(f"tiled{hd}_{_lens_id(lens)}{'_causal' if causal else ''}", _tiled_route(hd, lens), hd, lens, causal,
                                 seed=seed))
    # the tiled sides of the 72w switch: 223 wastes more than 1/8 of a 256-row tile, 257 of two
    out.append(_self("tiled72_223", tiled(72, 2, 3), 72, [223], seed=31))
    out.append(_self("tiled72_257_30", tiled(72, 2, 3), 72, [257, 30], seed=32))
    # head_dim 128: the resampler form (64 shared q rows against every item's keys) and the segment form (the EVisRAG vision
    # tower: head_dim 80 padded to 128, scale 80^-0.5, one cu buffer)
    keys = [1, 63, 64, 65, 130]
    out.append(Case(name="hd128_resampler", route=tiled(128, 1, 0), hd=128, heads=2, cu_q=FRONT + 64 * np.arange(len(keys) + 1),
                    cu_kv=_packed(keys), max_q=64, rows=sum(keys), q_shared=True, seed=41))
    out.append(_self("hd128_segments", tiled(128, 1, 0), 128, [64, 32, 4, 240], same_cu=True, kv_group=1, scale=80 ** -0.5, seed=42))
    for causal in (False, True):
        out.append(_self(f"small{'_causal' if causal else ''}", SMALL, 64, [80, 1, 16, 17, 79, 33], causal, heads=5, same_cu=True,
                         seed=51 + causal))
    for i, lens in enumerate([[224], [256, 224, 1], [448, 33]]):
        out.append(_self(f"72w_{_lens_id(lens)}", W72, 72, lens, seed=61 + i))
    out.append(_decode(1))
    out.append(_decode(3))
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def arena_of(name: str) -> Arena:
    return build(next(c for c in cases() if c.name == name))


@functools.lru_cache(maxsize=None)
def reference_of(name: str):
    """the fp64 reference of a case on its clean arena — computed once, shared, never written to"""
    a = arena_of(name)
    out, lse = reference(a.case, a.filled("clean"))
    out.setflags(write=False); lse.setflags(write=False)
    return out, lse
