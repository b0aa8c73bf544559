"""Thin Python owners of the two C-ABI objects: the VisRAG-Ret encoder (`HipEncoder`) and the
HBM-resident index (`HipIndex`).  torch tensors are used only as device-memory containers
and for the current HIP stream; all arithmetic happens in libvisrag_hip.so."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .config import VisRAGRetConfig
from .preprocess import PreparedItem


def _stream_ptr(device: int = 0) -> int:
    """HIP stream handle of torch's CURRENT stream ON `device` (the device the C side launches on)."""
    return int(torch.cuda.current_stream(int(device)).cuda_stream) if torch.cuda.is_available() else 0


def _require_gpu():
    if not torch.cuda.is_available():
        raise _lib.VisragHipError("no HIP device visible: visrag_amd has no CPU fallback")


def streams_overlap(a: "torch.cuda.Stream", b: "torch.cuda.Stream") -> bool:
    """Do kernels on the two streams run side by side (vr_streams_overlap: two spin kernels), or did the runtime put the
    streams on one hardware queue?"""
    _require_gpu()
    got = C.c_int32(0)
    _lib.check(_lib.load().vr_streams_overlap(int(a.device.index), C.c_void_p(int(a.cuda_stream)), C.c_void_p(int(b.cuda_stream)),
                                              C.byref(got)), "vr_streams_overlap")
    return bool(got.value)


def overlapping_streams(device, n: int = 2, tries: int = 12) -> List["torch.cuda.Stream"]:
    """`n` torch streams on `device` whose kernels overlap pairwise.  torch hands its pool streams out round-robin and
    HIP maps them onto four hardware queues: two NEIGHBOURING pool streams can share a queue (streams 2 and 3 of a fresh
    process do), and two batches "in flight" on them run at the single-stream rate — 661 against 711 pages/s.  Streams are
    drawn from the pool until `n` are found that overlap pairwise (probed, ~2.5 ms a pair); if the pool cannot deliver
    within `tries` draws the last draws fill the list — slower, still correct."""
    dev = torch.device(device) if not isinstance(device, int) else torch.device(f"cuda:{device}")
    chosen: List[torch.cuda.Stream] = []
    spare: List[torch.cuda.Stream] = []
    for _ in range(max(tries, n)):
        s = torch.cuda.Stream(device=dev)
        if all(streams_overlap(s, c) for c in chosen):
            chosen.append(s)
            if len(chosen) == n:
                return chosen
        else:
            spare.append(s)
    return (chosen + spare)[:n]


class HipEncoder:
    """Device-resident VisRAG-Ret weights + workspace (vr_model_*)."""

    def __init__(self, cfg: VisRAGRetConfig, device: int = 0, max_images: int = 32,
                 max_patches: Optional[int] = None, max_tokens: int = 4096, max_seqs: int = 64):
        _require_gpu()
        self.lib = _lib.load()
        self.cfg = cfg
        self.device = int(device)
        if max_patches is None:
            g = cfg.scale_resolution // cfg.patch_size
            max_patches = int(g * g * 1.1) + 8       # sliced pages reach ~1064 patches per slice
        self.max_images, self.max_tokens, self.max_seqs = max_images, max_tokens, max_seqs
        self._c = _lib.make_config(cfg, max_images, max_patches, max_tokens, max_seqs)
        self._h = C.c_void_p()
        _lib.check(self.lib.vr_model_create(self.device, C.byref(self._c), C.byref(self._h)), "vr_model_create")
        self.finalized = False

    def clone(self) -> "HipEncoder":
        """A second encoder on the SAME device weights with its own workspace (vr_model_clone): run it on
        another torch stream to keep two batches in flight.  Keeps a reference to its source."""
        if not self.finalized:
            raise RuntimeError("clone() needs a finalized encoder")
        other = object.__new__(HipEncoder)
        other.lib, other.cfg, other.device = self.lib, self.cfg, self.device
        other.max_images, other.max_tokens, other.max_seqs = self.max_images, self.max_tokens, self.max_seqs
        other._c = self._c
        other._h = C.c_void_p()
        other._src = self
        _lib.check(self.lib.vr_model_clone(self._h, C.byref(other._h)), "vr_model_clone")
        other.finalized = True
        return other

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.lib.vr_model_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    POOLINGS = {"wmean": 0, "mean": 1, "lasttoken": 2, "cls": 3}

    def set_pooling(self, pooling: str) -> None:
        """DRModel.encode's pooling (dense_retrieval_model.py:172-220); clones made afterwards inherit it."""
        if pooling not in self.POOLINGS:
            raise ValueError("Unknown pooling type: {}".format(pooling))
        _lib.check(self.lib.vr_model_set_pooling(self._h, self.POOLINGS[pooling]), "vr_model_set_pooling")

    # ---- weights --------------------------------------------------------------------------
    def load_weight(self, name: str, t: torch.Tensor) -> None:
        if t.dtype == torch.bfloat16:
            dt = _lib.VR_DTYPE_BF16
        else:
            t = t.to(torch.float32)
            dt = _lib.VR_DTYPE_F32
        t = t.contiguous()
        shape = (C.c_int64 * t.dim())(*t.shape)
        _lib.check(self.lib.vr_model_load_weight(self._h, name.encode(), C.c_void_p(t.data_ptr()), shape,
                                                 t.dim(), dt, 1 if t.is_cuda else 0), f"load {name}")
        self.finalized = False

    def load_state_dict(self, items: Iterable[Tuple[str, torch.Tensor]]) -> None:
        """items: (HF key, tensor) pairs — a dict's .items() or a generator (tensors may be
        released by the caller as soon as the call returns)."""
        if isinstance(items, dict):
            items = items.items()
        for name, t in items:
            self.load_weight(name, t)
        self.finalize()

    def finalize(self) -> None:
        _lib.check(self.lib.vr_model_finalize(self._h), "vr_model_finalize")
        self.finalized = True

    # ---- encode ---------------------------------------------------------------------------
    def encode_items(self, items: Sequence[PreparedItem], device_slices: Optional[List[torch.Tensor]] = None,
                     out: Optional[torch.Tensor] = None, hidden_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """items -> unit-norm embeddings [B, hidden] float32 on the device.
        `device_slices`: optional uint8 HWC cuda tensors replacing the host slices of the items
        (same order: item 0's slices first, ...).
        `hidden_out`: optional float32 cuda tensor [B, L, hidden] (L >= the longest item) that receives the last hidden
        states, right-padded with zeros (vr_encode_hidden: the HF-style forward's `last_hidden_state`)."""
        cfg = self.cfg
        B = len(items)
        if B == 0:
            raise ValueError("empty batch")
        Q = cfg.query_num
        seq = np.zeros(B + 1, dtype=np.int32)
        for i, it in enumerate(items):
            seq[i + 1] = seq[i] + len(it.input_ids)
        ids = np.concatenate([np.asarray(it.input_ids, dtype=np.int32) for it in items])
        slices: List = []
        hw: List[int] = []
        rows: List[np.ndarray] = []
        di = 0
        for i, it in enumerate(items):
            for k, s in enumerate(it.slices):
                if device_slices is not None:     # shapes come from the device tensors (host slice may be None)
                    s = device_slices[di]
                di += 1
                slices.append(s)
                hw += [int(s.shape[0]), int(s.shape[1])]
                r = np.full(Q, -1, dtype=np.int32)
                if k < len(it.image_bound):       # bound k <-> slice k (scatter_ semantics)
                    b0, b1 = it.image_bound[k]
                    n = max(0, min(Q, b1 - b0))
                    r[:n] = seq[i] + b0 + np.arange(n, dtype=np.int32)
                rows.append(r)
        n_slices = len(slices)
        if device_slices is None and n_slices and all(isinstance(t, torch.Tensor) and t.is_cuda for t in slices):
            device_slices = slices            # items prepared on the GPU (gpu_resize.prepare_item_gpu)
        on_dev = 0
        keep = []
        if n_slices:
            if device_slices is not None:
                if len(device_slices) != n_slices:
                    raise ValueError("device_slices must match the items' slices")
                ptrs = (C.c_void_p * n_slices)(*[C.c_void_p(t.data_ptr()) for t in device_slices])
                on_dev = 1
            else:
                keep = [np.ascontiguousarray(s, dtype=np.uint8) for s in slices]
                ptrs = (C.c_void_p * n_slices)(*[C.c_void_p(a.ctypes.data) for a in keep])
            hw_arr = (C.c_int32 * (2 * n_slices))(*hw)
            vr = np.ascontiguousarray(np.concatenate(rows), dtype=np.int32)
            vr_p = vr.ctypes.data_as(C.POINTER(C.c_int32))
        else:
            ptrs, hw_arr, vr_p = None, None, None
        if out is None:
            out = torch.empty((B, cfg.hidden_size), dtype=torch.float32, device=f"cuda:{self.device}")
        if hidden_out is not None:
            if not (hidden_out.is_cuda and hidden_out.dtype == torch.float32 and hidden_out.is_contiguous() and hidden_out.dim() == 3
                    and hidden_out.shape[0] == B and hidden_out.shape[2] == cfg.hidden_size):
                raise ValueError("hidden_out must be a contiguous float32 cuda tensor [B, L, hidden_size]")
            _lib.check(self.lib.vr_encode_hidden(
                self._h, ptrs, hw_arr, n_slices, on_dev,
                ids.ctypes.data_as(C.POINTER(C.c_int32)), seq.ctypes.data_as(C.POINTER(C.c_int32)), B,
                vr_p, C.c_void_p(out.data_ptr()), 1, C.c_void_p(hidden_out.data_ptr()), int(hidden_out.shape[1]),
                C.c_void_p(_stream_ptr(self.device))), "vr_encode_hidden")
            return out
        _lib.check(self.lib.vr_encode(
            self._h, ptrs, hw_arr, n_slices, on_dev,
            ids.ctypes.data_as(C.POINTER(C.c_int32)), seq.ctypes.data_as(C.POINTER(C.c_int32)), B,
            vr_p, C.c_void_p(out.data_ptr()), 1, C.c_void_p(_stream_ptr(self.device))), "vr_encode")
        return out

    # ---- profiling (HIP events around kernel classes, see include/visrag_hip.h) -------------
    PROF_CLASSES = ("vit_qkv", "vit_attn", "vit_proj", "vit_fc1", "vit_fc2", "resampler", "decoder",
                    "dec_qkv_rope", "dec_attn", "dec_o", "dec_gate_up", "dec_down", "dec_norms")

    def set_profile(self, on) -> None:
        """False / 0: off; True / 1: the seven phase classes; 2: the decoder's sub-phases (dec_*) instead."""
        _lib.check(self.lib.vr_model_set_profile(self._h, int(on)))

    def get_profile(self) -> Dict[str, Dict[str, float]]:
        out = {}
        for i, name in enumerate(self.PROF_CLASSES):
            ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
            _lib.check(self.lib.vr_model_get_profile(self._h, i, C.byref(ms), C.byref(n), C.byref(fl)))
            out[name] = {"ms": ms.value, "launches": int(n.value), "flops": fl.value}
        return out

    # ---- debug taps -----------------------------------------------------------------------
    def set_taps(self, on: bool) -> None:
        _lib.check(self.lib.vr_model_set_taps(self._h, 1 if on else 0))

    def tap(self, name: str, rows: int, cols: int) -> np.ndarray:
        out = np.empty((rows, cols), dtype=np.float32)
        _lib.check(self.lib.vr_model_tap(self._h, name.encode(), C.c_void_p(out.ctypes.data), rows, cols),
                   f"tap {name}")
        return out


class HipIndex:
    """HBM-resident embedding index (fp32 rows + a bf16 copy for the MFMA sweep)."""

    def __init__(self, dim: int, capacity: int, device: int = 0):
        _require_gpu()
        self.lib = _lib.load()
        self.dim, self.capacity, self.device = int(dim), int(capacity), int(device)
        self._h = C.c_void_p()
        _lib.check(self.lib.vr_index_create(self.device, self.dim, self.capacity, C.byref(self._h)),
                   "vr_index_create")
        self.n_groups = 0          # groups set for the rows present (set_groups); add / reset drop them
        self.n_filters = 0         # filters set for the rows present (set_filters); add / reset drop them

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self.lib.vr_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = C.c_int64()
        _lib.check(self.lib.vr_index_size(self._h, C.byref(n)))
        return int(n.value)

    def reset(self) -> None:
        _lib.check(self.lib.vr_index_reset(self._h))
        self.n_groups = 0
        self.n_filters = 0

    def add(self, reps) -> None:
        self.n_groups = 0
        self.n_filters = 0
        if isinstance(reps, torch.Tensor):
            t = reps.to(torch.float32).contiguous()
            assert t.dim() == 2 and t.shape[1] == self.dim
            _lib.check(self.lib.vr_index_add(self._h, C.c_void_p(t.data_ptr()), t.shape[0],
                                             1 if t.is_cuda else 0, C.c_void_p(_stream_ptr(self.device))), "vr_index_add")
        else:
            a = np.ascontiguousarray(reps, dtype=np.float32)
            assert a.ndim == 2 and a.shape[1] == self.dim
            _lib.check(self.lib.vr_index_add(self._h, C.c_void_p(a.ctypes.data), a.shape[0], 0,
                                             C.c_void_p(_stream_ptr(self.device))), "vr_index_add")

    # ---- editing in place (include/visrag_hip.h: vr_index_remove / vr_index_update / vr_index_get_rows) ----
    @staticmethod
    def _row_ids(ids) -> np.ndarray:
        if isinstance(ids, torch.Tensor):
            ids = ids.detach().cpu().numpy()
        return np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))

    def remove(self, ids) -> np.ndarray:
        """Remove the rows `ids` (any int sequence or tensor, any order, duplicates count once).  The rows that remain keep their
        order and close up; every search then answers as on an index freshly built from them.  The filters are carried along
        (`n_filters` stays), the grouping is dropped (`n_groups = 0`: set the offsets of the rows that remain).
        -> new_id_of_old, int64 [len before]: the new id of every old row, -1 for a removed one (documents.remap_rows carries
        ids across it, documents.compact_filters states what became of the filters)."""
        from .documents import new_id_of_old
        a = self._row_ids(ids)
        n_old = len(self)
        removed = C.c_int64(0)
        _lib.check(self.lib.vr_index_remove(self._h, a.ctypes.data_as(C.POINTER(C.c_int64)), len(a), C.byref(removed),
                                            C.c_void_p(_stream_ptr(self.device))), "vr_index_remove")
        if len(a):
            self.n_groups = 0
        return new_id_of_old(n_old, a)

    def update(self, ids, reps) -> None:
        """Rows `ids` (distinct) become `reps` [len(ids)][dim]: numpy, a cpu tensor or a cuda tensor.  No row moves: groups and
        filters stay."""
        a = self._row_ids(ids)
        if isinstance(reps, torch.Tensor) and reps.is_cuda:
            r = reps.to(torch.float32).contiguous()
            ptr, dev = r.data_ptr(), 1
        else:
            r = np.ascontiguousarray(reps.numpy() if isinstance(reps, torch.Tensor) else reps, dtype=np.float32)
            ptr, dev = r.ctypes.data, 0
        if r.ndim != 2 or tuple(r.shape) != (len(a), self.dim):
            raise ValueError(f"reps must be [{len(a)}][{self.dim}]")
        _lib.check(self.lib.vr_index_update(self._h, a.ctypes.data_as(C.POINTER(C.c_int64)), C.c_void_p(ptr), len(a), dev,
                                            C.c_void_p(_stream_ptr(self.device))), "vr_index_update")

    def rows(self, ids=None, bf16: bool = False, device: bool = False):
        """The rows `ids` (None: all; duplicates allowed) as stored: float32 [n][dim], or with `bf16` the MFMA copy as its raw
        bits, uint16 [n][dim] (int16 of the same bits on the device).  -> numpy, or a cuda tensor with `device=True`."""
        a = self._row_ids(np.arange(len(self)) if ids is None else ids)
        n = len(a)
        if device:
            out = torch.empty((n, self.dim), dtype=torch.int16 if bf16 else torch.float32, device=f"cuda:{self.device}")
            ptr = out.data_ptr()
        else:
            out = np.empty((n, self.dim), dtype=np.uint16 if bf16 else np.float32)
            ptr = out.ctypes.data
        if n == 0:
            return out
        _lib.check(self.lib.vr_index_get_rows(self._h, a.ctypes.data_as(C.POINTER(C.c_int64)), n,
                                              C.c_void_p(None if bf16 else ptr), C.c_void_p(ptr if bf16 else None),
                                              1 if device else 0, C.c_void_p(_stream_ptr(self.device))), "vr_index_get_rows")
        return out

    def _queries(self, queries, ndim: int = 2, shape: Optional[str] = None):
        """`queries` as contiguous float32 where they live -> (q, cuda): a cuda tensor stays one, a cpu tensor or anything else
        becomes numpy.  They have `ndim` axes, `dim` the last (`shape`: how the ValueError names that)."""
        cuda = isinstance(queries, torch.Tensor) and queries.is_cuda
        if cuda:
            q = queries.to(torch.float32).contiguous()
        else:
            q = np.ascontiguousarray(queries.numpy() if isinstance(queries, torch.Tensor) else queries, dtype=np.float32)
        if q.ndim != ndim or q.shape[-1] != self.dim:
            raise ValueError(f"queries must be {shape or f'[nq][{self.dim}]'}")
        return q, cuda

    def _grouped_queries(self, queries, lims):
        """the sub-queries of search_multi / search_multi_groups / search_rrf -> (q flat [n_sub][dim] where it lives, cuda, lims
        int64 host, n_groups, n_sub): flat `queries` with `lims` [n_groups + 1], or [n_groups][m][dim] with `lims=None`"""
        if lims is None:
            q, cuda = self._queries(queries, 3, f"[n_groups][m][{self.dim}] when lims is None")
            lim = np.arange(q.shape[0] + 1, dtype=np.int64) * q.shape[1]
            q = q.reshape(-1, self.dim)
        else:
            q, cuda = self._queries(queries, 2, f"[n_sub][{self.dim}] with lims")
            lim = np.ascontiguousarray(self._row_ids(lims), dtype=np.int64)
            if len(lim) < 1:
                raise ValueError("lims must hold n_groups + 1 entries")
        return q, cuda, lim, len(lim) - 1, int(q.shape[0])

    def _filter_of_group(self, q, cuda: bool, ng: int, filter_of_group):
        """`filter_of_group` of those searches, one entry per group, where the queries live -> (keep-alive, pointer); None: no filter"""
        if filter_of_group is None:
            return None, C.c_void_p(None)
        return self._filter_of_query(torch.empty((ng, 0), device=q.device) if cuda else np.empty((ng, 0)), filter_of_group)

    def _stats3(self, fn, names, reset: bool) -> Dict[str, int]:
        """the three counters of one search's `*_search_stats` under `names`, cleared with `reset`"""
        out = (C.c_int64 * 3)()
        _lib.check(fn(self._h, out, 1 if reset else 0))
        return {name: int(v) for name, v in zip(names, out)}

    def _search(self, fn, what: str, queries, k: int, n_int_out: int):
        """One call of a library search that writes scores [nq,k] f32 and `n_int_out` arrays [nq,k] i64: torch cuda tensors in ->
        cuda tensors out, numpy / cpu in -> numpy out (sized with max(k, 0): a negative k reaches the library's own error)."""
        cuda = isinstance(queries, torch.Tensor) and queries.is_cuda
        if cuda:
            q = queries.to(torch.float32).contiguous()
            outs = [torch.empty((q.shape[0], k), dtype=d, device=q.device) for d in [torch.float32] + [torch.int64] * n_int_out]
            ptrs = [x.data_ptr() for x in [q] + outs]
        else:
            q = np.ascontiguousarray(queries.numpy() if isinstance(queries, torch.Tensor) else queries, dtype=np.float32)
            outs = [np.empty((q.shape[0], max(k, 0)), dtype=d) for d in [np.float32] + [np.int64] * n_int_out]
            ptrs = [x.ctypes.data for x in [q] + outs]
        _lib.check(fn(self._h, C.c_void_p(ptrs[0]), q.shape[0], k, *[C.c_void_p(p) for p in ptrs[1:]], 1 if cuda else 0,
                      C.c_void_p(_stream_ptr(self.device))), what)
        return tuple(outs)

    def search(self, queries, k: int):
        """-> (scores [nq,k] f32, ids [nq,k] i64); torch cuda tensors in -> cuda tensors out,
        numpy / cpu in -> numpy out."""
        return self._search(self.lib.vr_index_search, "vr_index_search", queries, k, 1)

    def set_groups(self, offsets) -> None:
        """Partition the rows present into groups (documents) of adjacent rows: group g = rows offsets[g] .. offsets[g + 1] - 1
        (offsets[0] == 0, strictly increasing, offsets[-1] == len(self)).  `add` and `reset` drop the grouping."""
        off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        _lib.check(self.lib.vr_index_set_groups(self._h, off.ctypes.data_as(C.POINTER(C.c_int64)), len(off) - 1),
                   "vr_index_set_groups")
        self.n_groups = len(off) - 1

    def search_groups(self, queries, k: int):
        """The k best groups per query, each by its best row (include/visrag_hip.h: vr_index_search_groups)
        -> (scores [nq,k] f32, best row ids [nq,k] i64, groups [nq,k] i64); cuda in -> cuda out, numpy / cpu in -> numpy out."""
        return self._search(self.lib.vr_index_search_groups, "vr_index_search_groups", queries, k, 2)

    def group_search_stats(self, reset: bool = False) -> Dict[str, int]:
        """Grouped-search queries since the last reset by outcome: certified from the first candidate set / after widening it /
        redone from exact fp32 scores of every row."""
        return self._stats3(self.lib.vr_index_group_search_stats, ("certified", "certified_widened", "exact"), reset)

    def set_filters(self, masks) -> None:
        """Row filters for `search_filtered` over the rows present: `masks` is bool [n_filters][len(self)] (True = the row is
        allowed) or already packed uint32 [n_filters][ceil(len(self) / 32)] (documents.pack_filters: bit r & 31 of word r >> 5;
        bits beyond the last row are ignored), numpy or torch, host or cuda — a cuda tensor is packed and handed over on the
        device.  The library keeps its own copy.  `add` and `reset` drop the filters; filters and groups are independent."""
        n, words = len(self), (len(self) + 31) // 32
        if isinstance(masks, torch.Tensor) and masks.is_cuda:
            m = masks
            if m.dtype == torch.bool:
                if m.dim() != 2 or m.shape[1] != n:
                    raise ValueError(f"bool masks must be [n_filters][{n}]")
                m = torch.nn.functional.pad(m, (0, words * 32 - n)).reshape(m.shape[0], words, 32).to(torch.int64)
                m = (m << torch.arange(32, device=m.device)).sum(-1)                 # 0 .. 2^32 - 1: the word's value
                m = torch.where(m >= 2 ** 31, m - 2 ** 32, m).to(torch.int32)        # ... as the int32 of the same bits
            elif m.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                raise ValueError("cuda masks must be bool, or packed words as int32 / uint32")
            m = m.contiguous()
            if m.dim() != 2 or m.shape[1] != words:
                raise ValueError(f"packed masks must be [n_filters][{words}]")
            ptr, nf, dev = m.data_ptr(), m.shape[0], 1
        else:
            from .documents import pack_filters
            m = np.asarray(masks.numpy() if isinstance(masks, torch.Tensor) else masks)
            m = pack_filters(m) if m.dtype == np.bool_ and m.ndim == 2 and m.shape[1] == n else m
            if m.dtype == np.int32:
                m = m.view(np.uint32)
            if m.dtype != np.uint32 or m.ndim != 2 or m.shape[1] != words:
                raise ValueError(f"masks must be bool [n_filters][{n}] or packed uint32 [n_filters][{words}]")
            m = np.ascontiguousarray(m)
            ptr, nf, dev = m.ctypes.data, m.shape[0], 0
        _lib.check(self.lib.vr_index_set_filters(self._h, C.c_void_p(ptr), nf, dev, C.c_void_p(_stream_ptr(self.device))),
                   "vr_index_set_filters")
        self.n_filters = int(nf)

    def _filter_of_query(self, queries, filter_of_query):
        """`filter_of_query` of search_filtered / search_diverse as int32 [nq] where the queries live -> (keep-alive, pointer)"""
        nq = int(queries.shape[0])
        if filter_of_query is None:
            filter_of_query = -1
        if isinstance(filter_of_query, (int, np.integer)):
            fq = np.full(nq, int(filter_of_query), dtype=np.int64)
        elif isinstance(filter_of_query, torch.Tensor):
            fq = filter_of_query.detach().cpu().numpy().astype(np.int64).reshape(-1)
        else:
            fq = np.asarray(filter_of_query, dtype=np.int64).reshape(-1)
        if len(fq) != nq:
            raise ValueError(f"{len(fq)} filter_of_query entries for {nq} queries")
        if self.n_filters and ((fq < -1) | (fq >= self.n_filters)).any():
            raise ValueError(f"filter_of_query entries must lie in [-1, {self.n_filters})")
        fq = np.ascontiguousarray(fq, dtype=np.int32)
        cuda = isinstance(queries, torch.Tensor) and queries.is_cuda
        keep = torch.from_numpy(fq).to(queries.device) if cuda else fq
        return keep, C.c_void_p(keep.data_ptr() if cuda else keep.ctypes.data)

    def search_filtered(self, queries, k: int, filter_of_query=None):
        """The k best rows per query among the rows its filter allows (include/visrag_hip.h: vr_index_search_filtered)
        -> (scores [nq,k] f32, ids [nq,k] i64), tail (-inf, -1) where fewer than k rows are allowed; cuda in -> cuda out, numpy / cpu
        in -> numpy out.  `filter_of_query`: one filter index per query (any int sequence or tensor), an int = that filter for
        every query, None or -1 = no filter (all rows).  Entries outside [-1, n_filters) raise ValueError."""
        keep, fptr = self._filter_of_query(queries, filter_of_query)

        def fn(h, q, n, kk, out_scores, out_ids, on_device, stream):
            return self.lib.vr_index_search_filtered(h, q, n, kk, fptr, out_scores, out_ids, on_device, stream)

        return self._search(fn, "vr_index_search_filtered", queries, k, 1)

    def search_diverse(self, queries, k: int, pool: Optional[int] = None, lambda_: float = 0.5, filter_of_query=None):
        """k rows per query picked by maximal marginal relevance from the pool of its `pool` best rows (include/visrag_hip.h:
        vr_index_search_diverse): pick 0 is the best row, every later pick maximises lambda_ * score - (1 - lambda_) * (largest
        dot product with a row already picked).  -> (scores [nq,k] f32 the picks' relevance, ids [nq,k] i64) in PICK order — the
        scores are not monotone — tail (-inf, -1) where the pool has fewer than k rows; cuda in -> cuda out, numpy / cpu in ->
        numpy out.  `pool=None`: min(1000, max(4 * k, 32)).  `filter_of_query` as in `search_filtered`, None = the pool of the
        plain search (no filters need to be set)."""
        if pool is None:
            pool = min(1000, max(4 * k, 32))
        keep, fptr = (None, C.c_void_p(None)) if filter_of_query is None else self._filter_of_query(queries, filter_of_query)

        def fn(h, q, n, kk, out_scores, out_ids, on_device, stream):
            return self.lib.vr_index_search_diverse(h, q, n, kk, int(pool), float(lambda_), fptr, out_scores, out_ids, on_device, stream)

        return self._search(fn, "vr_index_search_diverse", queries, k, 1)

    def filter_search_stats(self, reset: bool = False) -> Dict[str, int]:
        """Filtered-search queries since the last reset by outcome: certified from the first candidate set (or no row allowed) /
        after widening it / redone from exact fp32 scores of every row."""
        return self._stats3(self.lib.vr_index_filter_search_stats, ("certified", "certified_widened", "exact"), reset)

    def search_range(self, queries, threshold, filter_of_query=None, max_total: Optional[int] = None, sort: bool = True):
        """Every row whose fp32 score is >= the query's threshold (include/visrag_hip.h: vr_index_search_range) -> (lims int64
        [nq + 1], scores f32 [total], ids i64 [total]): entries lims[q] .. lims[q + 1] - 1 are query q's; cuda in -> cuda out,
        numpy / cpu in -> numpy out.  `threshold`: a scalar or one per query.  `filter_of_query` as in `search_filtered`, None =
        no filter (none need to be set).  `max_total=None`: min(nq * rows, 2 ** 26) entries; a larger result raises
        (VR_ERR_CAPACITY).  `sort=True`: every segment by score descending, then id ascending — the library's ranking order;
        `sort=False`: the ABI's ascending-id order."""
        return self._range_call(False, queries, threshold, filter_of_query, max_total, sort)

    def _range_call(self, grouped: bool, queries, threshold, filter_of_query, max_total, sort):
        """search_range, or with `grouped` search_groups_range: the thresholds, `max_total`, the search and its `*_results` call,
        then every segment sorted by the search's own key"""
        q, cuda = self._queries(queries)
        nq = int(q.shape[0])
        if isinstance(threshold, torch.Tensor):
            threshold = threshold.detach().cpu().numpy()
        thr = np.array(threshold, dtype=np.float32).reshape(-1)          # (a copy: the caller's array may be read-only)
        thr = np.full(nq, thr[0], dtype=np.float32) if thr.size == 1 else np.ascontiguousarray(thr)
        if len(thr) != nq:
            raise ValueError(f"{len(thr)} thresholds for {nq} queries")
        keep, fptr = (None, C.c_void_p(None)) if filter_of_query is None else self._filter_of_query(q, filter_of_query)
        if max_total is None:
            max_total = max(1, min(nq * (self.n_groups if grouped else len(self)), 2 ** 26))
        search, results = ("vr_index_search_groups_range", "vr_index_group_range_results") if grouped else \
                          ("vr_index_search_range", "vr_index_range_results")
        total = C.c_int64(0)
        stream = C.c_void_p(_stream_ptr(self.device))
        if cuda:
            thr_d = torch.from_numpy(thr).to(q.device)
            lims = torch.empty(nq + 1, dtype=torch.int64, device=q.device)
            ptrs = (q.data_ptr(), thr_d.data_ptr(), lims.data_ptr())
        else:
            lims = np.empty(nq + 1, dtype=np.int64)
            ptrs = (q.ctypes.data, thr.ctypes.data, lims.ctypes.data)
        _lib.check(getattr(self.lib, search)(self._h, C.c_void_p(ptrs[0]), nq, C.c_void_p(ptrs[1]), fptr, int(max_total),
                                             C.c_void_p(ptrs[2]), C.byref(total), 1 if cuda else 0, stream), search)
        n = int(total.value)
        if cuda:       # scores, (best) rows and with `grouped` groups
            outs = [torch.empty(n, dtype=d, device=q.device) for d in (torch.float32, torch.int64, torch.int64)[:3 if grouped else 2]]
            optrs = [C.c_void_p(x.data_ptr()) for x in outs]
        else:
            outs = [np.empty(n, dtype=d) for d in (np.float32, np.int64, np.int64)[:3 if grouped else 2]]
            optrs = [C.c_void_p(x.ctypes.data) for x in outs]
        _lib.check(getattr(self.lib, results)(self._h, *optrs, n, 1 if cuda else 0, stream), results)
        del keep
        if sort and n > 1:
            scores = outs[0]
            if cuda:
                seg = torch.repeat_interleave(torch.arange(nq, device=q.device), lims[1:] - lims[:-1])
                key = scores
                if grouped:     # the ranking's order of floats is that of the keys' orderable bits (-0.0 < +0.0)
                    bits = scores.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
                    key = torch.where(bits >= 0x80000000, 0xFFFFFFFF - bits, bits + 0x80000000)
                o1 = torch.sort(key, descending=True, stable=True)[1]        # ids (groups) ascend already: the stable sorts keep that
                order = o1[torch.sort(seg[o1], stable=True)[1]]
            else:
                seg = np.repeat(np.arange(nq), np.diff(lims))
                if grouped:
                    bits = scores.view(np.uint32).astype(np.int64)
                    order = np.lexsort((outs[2], -np.where(bits >= 0x80000000, 0xFFFFFFFF - bits, bits + 0x80000000), seg))
                else:
                    order = np.lexsort((outs[1], -scores.astype(np.float64), seg))
            outs = [x[order] for x in outs]
        return (lims, *outs)

    def range_search_stats(self, reset: bool = False) -> Dict[str, int]:
        """Range searches since the last reset: queries, candidate rows re-scored in fp32 (the rows inside the error band below
        the thresholds and everything above), rows returned."""
        return self._stats3(self.lib.vr_index_range_search_stats, ("queries", "candidates", "returned"), reset)

    # ---- rank search (include/visrag_hip.h: vr_index_rank_rows / vr_index_count_range) ----
    @staticmethod
    def _pairs(values, lims, nq: int, dtype, what: str):
        """The targets / thresholds of nq queries -> (flat [pairs] of `dtype`, lims int64 [nq + 1], shape of the outputs).  `values`:
        a scalar (one for every query), [nq], [nq][T], or flat with `lims`."""
        if isinstance(values, torch.Tensor):
            values = values.detach().cpu().numpy()
        v = np.asarray(values)
        if lims is not None:
            if isinstance(lims, torch.Tensor):
                lims = lims.detach().cpu().numpy()
            lims = np.ascontiguousarray(np.asarray(lims, dtype=np.int64).reshape(-1))
            v = v.reshape(-1)
            if len(lims) != nq + 1 or lims[-1] != len(v):
                raise ValueError(f"lims must hold {nq + 1} entries and end at the {len(v)} {what}")
            shape = (len(v),)
        else:
            if v.ndim == 0:
                v = np.full(nq, v)
            if v.ndim not in (1, 2) or v.shape[0] != nq:
                raise ValueError(f"{what} must be [{nq}] or [{nq}][T], or flat with lims")
            shape = v.shape
            lims = np.arange(nq + 1, dtype=np.int64) * (1 if v.ndim == 1 else v.shape[1])
        return np.ascontiguousarray(v.reshape(-1), dtype=dtype), lims, shape

    def _rank_call(self, grouped: bool, queries, flat, lims, shape, filter_of_query, strict):
        """The rank search of rows (vr_index_rank_rows / vr_index_count_range) or with `grouped` of documents (vr_index_rank_groups /
        vr_index_count_groups_range): int64 targets -> (scores, best rows — documents only — and ranks), float32 thresholds ->
        counts"""
        q, cuda = self._queries(queries)
        nq, n = int(q.shape[0]), len(flat)
        ranks = flat.dtype == np.int64
        keep, fptr = (None, C.c_void_p(None)) if filter_of_query is None else self._filter_of_query(q, filter_of_query)
        if cuda:
            outs = [torch.empty(n, dtype=d, device=q.device) for d in (torch.float32, torch.int64, torch.int64)]
            ptrs = [C.c_void_p(x.data_ptr()) for x in [q] + outs]
        else:
            outs = [np.empty(n, dtype=d) for d in (np.float32, np.int64, np.int64)]
            ptrs = [C.c_void_p(x.ctypes.data) for x in [q] + outs]
        if ranks:
            name = "vr_index_rank_groups" if grouped else "vr_index_rank_rows"
            args = [fptr, ptrs[1]] + ([ptrs[2]] if grouped else []) + [ptrs[3]]
        else:
            name = "vr_index_count_groups_range" if grouped else "vr_index_count_range"
            args = [1 if strict else 0, fptr, ptrs[3]]
        _lib.check(getattr(self.lib, name)(self._h, ptrs[0], nq, C.c_void_p(lims.ctypes.data), C.c_void_p(flat.ctypes.data), *args,
                                           1 if cuda else 0, C.c_void_p(_stream_ptr(self.device))), name)
        del keep
        if not ranks:
            return outs[2].reshape(shape)
        return tuple(x.reshape(shape) for x in (outs if grouped else (outs[0], outs[2])))

    def rank_rows(self, queries, ids, lims=None, filter_of_query=None):
        """Where the named rows stand (include/visrag_hip.h: vr_index_rank_rows) -> (scores f32, ranks i64) shaped as `ids`: the
        fp32 score `search` returns for that (query, row) and the number of rows ahead of it — score descending, then lower id
        first — so a row of rank r is at position r of `search(k)` for every k > r.  `ids`: [nq] (one target per query), [nq][T],
        or flat with `lims` [nq + 1] (query q's targets are ids[lims[q]:lims[q + 1]]); duplicates allowed.  `filter_of_query`
        as in `search_filtered`: the rank among the rows the filter allows — for a target the filter forbids, the position it
        WOULD take.  cuda queries -> cuda tensors, numpy / cpu -> numpy."""
        flat, lims, shape = self._pairs(ids, lims, int(queries.shape[0]), np.int64, "ids")
        return self._rank_call(False, queries, flat, lims, shape, filter_of_query, False)

    def count_range(self, queries, thresholds, lims=None, filter_of_query=None, strict: bool = False):
        """How many rows reach a threshold (include/visrag_hip.h: vr_index_count_range) -> counts i64 shaped as `thresholds`
        (a scalar: [nq]): rows with fp32 score >= t, with `strict` > t — exactly `np.diff(search_range(queries, t)[0])`, without
        the rows.  `thresholds`: a scalar, [nq], [nq][T], or flat with `lims`.  `filter_of_query` as in `search_filtered`.
        cuda queries -> a cuda tensor, numpy / cpu -> numpy."""
        flat, lims, shape = self._pairs(thresholds, lims, int(queries.shape[0]), np.float32, "thresholds")
        return self._rank_call(False, queries, flat, lims, shape, filter_of_query, strict)

    def rank_search_stats(self, reset: bool = False) -> Dict[str, int]:
        """Rank searches and counts since the last reset: (query, bar) pairs, rows of the error bands re-scored in fp32, rows counted."""
        return self._stats3(self.lib.vr_index_rank_search_stats, ("pairs", "candidates", "counted"), reset)

    # ---- windowed search (include/visrag_hip.h: vr_index_search_window) ----
    def _offsets(self, offset, nq: int) -> np.ndarray:
        """`offset` of the window searches as int64 [nq]: an int is every query's"""
        off = self._row_ids(offset)
        if off.size == 1 and nq != 1:
            off = np.full(nq, off[0], dtype=np.int64)
        if len(off) != nq:
            raise ValueError(f"{len(off)} offsets for {nq} queries")
        if (off < 0).any():
            raise ValueError("offsets must be >= 0")
        return off

    def search_window(self, queries, offset, k: int, filter_of_query=None):
        """The rows at ranks [offset, offset + k) of every query's fp32 ranking (include/visrag_hip.h: vr_index_search_window)
        -> (scores [nq,k] f32, ids [nq,k] i64): entry j is the row of rank offset + j — score descending, then lower id first,
        among the rows the query's filter allows — so `search_window(q, o, k)` is `search(q, o + k)[..., o:]` wherever `search`
        reaches, and `rank_rows` of the ids returned is `offset + arange(k)`.  `offset`: an int (every query's) or one per query
        (any int sequence or tensor), each >= 0, however deep; slots at or past the number of allowed rows are (-inf, -1).
        1 <= k <= 1000: page for more.  `filter_of_query` as in `search_filtered`, None = no filter (none need to be set).
        cuda in -> cuda out, numpy / cpu in -> numpy out."""
        off = self._offsets(offset, int(queries.shape[0]))
        keep, fptr = (None, C.c_void_p(None)) if filter_of_query is None else self._filter_of_query(queries, filter_of_query)

        def fn(h, q, n, kk, out_scores, out_ids, on_device, stream):
            return self.lib.vr_index_search_window(h, q, n, C.c_void_p(off.ctypes.data), kk, fptr, out_scores, out_ids, on_device, stream)

        return self._search(fn, "vr_index_search_window", queries, k, 1)

    def window_search_stats(self, reset: bool = False) -> Dict[str, int]:
        """Windowed searches since the last reset: queries, rows of the bands re-scored in fp32, rows certainly ahead of their
        query's window (decided by the bf16 score alone)."""
        return self._stats3(self.lib.vr_index_window_search_stats, ("queries", "candidates", "ahead"), reset)

    # ---- document window search (include/visrag_hip.h: vr_index_search_groups_window) ----
    def search_groups_window(self, queries, offset, k: int, filter_of_query=None):
        """The documents at ranks [offset, offset + k) of every query's document ranking, under its filter (include/visrag_hip.h:
        vr_index_search_groups_window) -> (scores [nq,k] f32, best row ids [nq,k] i64, groups [nq,k] i64).  A group (`set_groups`)
        is present if the query's filter allows one of its rows; it scores as its best ALLOWED row does, that row — the lowest
        among equals — is its best row, and present groups rank score descending, then lower group first.  Entry j is the group
        of rank offset + j; slots at or past the number of present groups are (-inf, -1, -1).  `search_groups_window(q, 0, k)` is
        `search_groups(q, k)` bit for bit.  `offset`: an int (every query's) or one per query (any int sequence or tensor), each
        >= 0, however deep.  1 <= k <= 1000: page for more.  `filter_of_query` as in `search_filtered`, None = no filter (none
        need to be set).  cuda in -> cuda out, numpy / cpu in -> numpy out."""
        off = self._offsets(offset, int(queries.shape[0]))
        keep, fptr = (None, C.c_void_p(None)) if filter_of_query is None else self._filter_of_query(queries, filter_of_query)

        def fn(h, q, n, kk, out_scores, out_ids, out_groups, on_device, stream):
            return self.lib.vr_index_search_groups_window(h, q, n, C.c_void_p(off.ctypes.data), kk, fptr, out_scores, out_ids,
                                                          out_groups, on_device, stream)

        return self._search(fn, "vr_index_search_groups_window", queries, k, 2)

    def group_window_search_stats(self, reset: bool = False) -> Dict[str, int]:
        """Document window searches since the last reset: queries, documents of the bands re-scored, fp32 page dot products."""
        return self._stats3(self.lib.vr_index_group_window_search_stats, ("queries", "documents", "page_dots"), reset)

    # ---- document rank search (include/visrag_hip.h: vr_index_rank_groups / vr_index_count_groups_range) ----
    def rank_groups(self, queries, groups, lims=None, filter_of_query=None):
        """Where the named documents stand (include/visrag_hip.h: vr_index_rank_groups) -> (scores f32, best rows i64, ranks i64)
        shaped as `groups`.  The ranking is `search_groups_window`'s: a group (`set_groups`) is present if the query's filter
        allows one of its rows, it scores as its best ALLOWED row does, that row — the lowest among equals — is its best row, and
        present groups rank score descending, then lower group first.  The rank is the number of present groups ahead, so a group
        of rank r is entry r - o of `search_groups_window(q, o, k, f)` for every o <= r < o + k, with the same score bits and the
        same best row.  A target the filter leaves no row of is NOT in the ranking: it gets (-inf, -1, -1) — unlike `rank_rows`,
        where a forbidden row gets the position it would take: a group's score is defined over its allowed rows, an absent group
        has none (`documents.never_retrieved` turns the -1 into a rank no cut-off reaches).  `groups`: host ints, [nq] (one
        target per query), [nq][T], or flat with `lims` [nq + 1]; duplicates allowed.  `filter_of_query` as in `search_filtered`,
        None = no filter.  cuda queries -> cuda tensors, numpy / cpu -> numpy."""
        flat, lims, shape = self._pairs(groups, lims, int(queries.shape[0]), np.int64, "groups")
        return self._rank_call(True, queries, flat, lims, shape, filter_of_query, False)

    def count_groups_range(self, queries, thresholds, lims=None, filter_of_query=None, strict: bool = False):
        """How many documents reach a threshold (include/visrag_hip.h: vr_index_count_groups_range) -> counts i64 shaped as
        `thresholds` (a scalar: [nq]): present groups whose score — that of their best allowed row — is >= t, with `strict` > t.
        `thresholds`: a scalar, [nq], [nq][T], or flat with `lims`; finite; -0.0 counts as +0.0.  `filter_of_query` as in
        `search_filtered`.  cuda queries -> a cuda tensor, numpy / cpu -> numpy."""
        flat, lims, shape = self._pairs(thresholds, lims, int(queries.shape[0]), np.float32, "thresholds")
        return self._rank_call(True, queries, flat, lims, shape, filter_of_query, strict)

    def group_rank_search_stats(self, reset: bool = False) -> Dict[str, int]:
        """Document rank searches and counts since the last reset: (query, bar) pairs, documents of the error bands re-scored (a
        rank's own target among them), fp32 page dot products."""
        return self._stats3(self.lib.vr_index_group_rank_search_stats, ("pairs", "documents", "page_dots"), reset)

    # ---- document range search (include/visrag_hip.h: vr_index_search_groups_range) ----
    def search_groups_range(self, queries, threshold, filter_of_query=None, max_total: Optional[int] = None, sort: bool = True):
        """Every document whose score reaches the query's threshold, under its filter (include/visrag_hip.h:
        vr_index_search_groups_range) -> (lims int64 [nq + 1], scores f32 [total], best rows i64 [total], groups i64 [total]):
        entries lims[q] .. lims[q + 1] - 1 are query q's; cuda in -> cuda out, numpy / cpu in -> numpy out.  The semantics are
        `search_groups_window`'s and `count_groups_range`'s: a group (`set_groups`) is present if the query's filter allows one of
        its rows, it scores as its best ALLOWED row does, that row — the lowest among equals — is its best row; the result is every
        present group with score >= t (-0.0 counts as +0.0), so `np.diff(lims)` is `count_groups_range(queries, t, ...)`.
        `threshold`: a scalar or one per query.  `filter_of_query` as in `search_filtered`, None = no filter (none need to be
        set).  `max_total=None`: min(nq * groups, 2 ** 26) entries, at least 1; a larger result raises (VR_ERR_CAPACITY).
        `sort=True`: every segment in `search_groups_window`'s order, score descending, then lower group first; `sort=False`: the
        ABI's ascending-group order."""
        return self._range_call(True, queries, threshold, filter_of_query, max_total, sort)

    def group_range_search_stats(self, reset: bool = False) -> Dict[str, int]:
        """Document range searches since the last reset: queries, documents of the error bands re-scored (everything that can
        reach its threshold), fp32 page dot products."""
        return self._stats3(self.lib.vr_index_group_range_search_stats, ("queries", "documents", "page_dots"), reset)

    # ---- fused search (include/visrag_hip.h: vr_index_search_multi) ----
    def search_multi(self, queries, lims, k: int, fuse: str = "max", filter_of_group=None):
        """The k rows of largest fused score per group of sub-queries (include/visrag_hip.h: vr_index_search_multi) -> (scores
        [n_groups,k] f32, ids [n_groups,k] i64, which [n_groups,k] i32).  A row's fused score is the max (`fuse="max"`, "any-of")
        or the min (`fuse="min"`, "all-of") of its fp32 scores — the bits `search` returns — over the group's sub-queries; rows
        come score descending, then lower id first, among the rows the group's filter allows, slots past them are (-inf, -1, -1);
        `which` is the lowest in-group index of a sub-query whose score IS the fused score.  `queries`: flat [n_sub][dim] with
        `lims` [n_groups + 1] (group g = sub-queries lims[g] .. lims[g + 1] - 1; documents.group_rows makes it from labels), or
        [n_groups][m][dim] with `lims=None`.  Groups hold 1..256 sub-queries, 1 <= k <= 1000.  `filter_of_group` as
        `filter_of_query` in `search_filtered`, one entry per group; None = no filter (none need to be set).  cuda in -> cuda
        out, numpy / cpu in -> numpy out."""
        if fuse not in ("max", "min"):
            raise ValueError("fuse must be 'max' or 'min'")
        q, cuda, lim, ng, n_sub = self._grouped_queries(queries, lims)
        keep, fptr = self._filter_of_group(q, cuda, ng, filter_of_group)
        if cuda:
            outs = [torch.empty((ng, k), dtype=d, device=q.device) for d in (torch.float32, torch.int64, torch.int32)]
            ptrs = [x.data_ptr() for x in [q] + outs]
        else:
            outs = [np.empty((ng, max(k, 0)), dtype=d) for d in (np.float32, np.int64, np.int32)]
            ptrs = [x.ctypes.data for x in [q] + outs]
        _lib.check(self.lib.vr_index_search_multi(self._h, C.c_void_p(ptrs[0]), n_sub, C.c_void_p(lim.ctypes.data), ng, k,
                                                  0 if fuse == "max" else 1, fptr, C.c_void_p(ptrs[1]), C.c_void_p(ptrs[2]),
                                                  C.c_void_p(ptrs[3]), 1 if cuda else 0, C.c_void_p(_stream_ptr(self.device))),
                   "vr_index_search_multi")
        del keep
        return tuple(outs)

    def multi_search_stats(self, reset: bool = False) -> Dict[str, int]:
        """Fused searches since the last reset: groups, columns of the bands re-scored in fp32, fp32 row dot products (every
        band column against every sub-query of its group)."""
        return self._stats3(self.lib.vr_index_multi_search_stats, ("groups", "candidates", "dots"), reset)

    # ---- fused document search (include/visrag_hip.h: vr_index_search_multi_groups) ----
    def search_multi_groups(self, queries, lims, k: int, fuse: str = "max", filter_of_group=None, evidence: bool = False):
        """The k documents (`set_groups`) of largest fused score per question (include/visrag_hip.h:
        vr_index_search_multi_groups) -> (scores [n_questions,k] f32, best rows [n_questions,k] i64, docs [n_questions,k] i64,
        which [n_questions,k] i32).  A document is present if the question's filter allows one of its pages; per sub-query j it
        scores E_j(D) = its best ALLOWED page's fp32 score — the bits `search` returns — and its fused score is the max
        (`fuse="max"`, "any-of") or the min (`fuse="min"`, "all-of") of them over the question's sub-queries.  Documents come
        score descending, then lower document first; slots past the present documents are (-inf, -1, -1, -1).  `which` is the
        lowest sub-query whose E_j(D) IS the fused score, the best row that sub-query's best page (the lowest among equals).
        With `evidence=True` two more arrays follow: (ev_scores f32, ev_rows i64), flat [n_sub * k]; question g's block starts at
        k * lims[g] and reads as [k][m_g] — per returned document the best page of EVERY sub-query and its score, (-inf, -1) in a
        tail slot (documents.evidence_pages makes a generator's page list of one question's block).  `queries`, `lims` and
        `filter_of_group` as in `search_multi`; with [n_questions][m][dim] and `lims=None` the evidence comes as
        [n_questions][k][m].  1 <= k <= 1000.  cuda in -> cuda out, numpy / cpu in -> numpy out."""
        if fuse not in ("max", "min"):
            raise ValueError("fuse must be 'max' or 'min'")
        q, cuda, lim, ng, n_sub = self._grouped_queries(queries, lims)
        keep, fptr = self._filter_of_group(q, cuda, ng, filter_of_group)
        kk = max(k, 0)
        if cuda:
            outs = [torch.empty((ng, kk), dtype=d, device=q.device) for d in (torch.float32, torch.int64, torch.int64, torch.int32)]
            if evidence:
                outs += [torch.empty(n_sub * kk, dtype=d, device=q.device) for d in (torch.float32, torch.int64)]
            ptrs = [x.data_ptr() for x in [q] + outs]
        else:
            outs = [np.empty((ng, kk), dtype=d) for d in (np.float32, np.int64, np.int64, np.int32)]
            if evidence:
                outs += [np.empty(n_sub * kk, dtype=d) for d in (np.float32, np.int64)]
            ptrs = [x.ctypes.data for x in [q] + outs]
        ev = [C.c_void_p(ptrs[5]), C.c_void_p(ptrs[6])] if evidence else [C.c_void_p(None), C.c_void_p(None)]
        _lib.check(self.lib.vr_index_search_multi_groups(self._h, C.c_void_p(ptrs[0]), n_sub, C.c_void_p(lim.ctypes.data), ng, k,
                                                         0 if fuse == "max" else 1, fptr, C.c_void_p(ptrs[1]), C.c_void_p(ptrs[2]),
                                                         C.c_void_p(ptrs[3]), C.c_void_p(ptrs[4]), *ev, 1 if cuda else 0,
                                                         C.c_void_p(_stream_ptr(self.device))),
                   "vr_index_search_multi_groups")
        del keep
        if evidence and lims is None:
            outs[4:] = [x.reshape(ng, kk, n_sub // max(ng, 1)) for x in outs[4:]]
        return tuple(outs)

    def multi_group_search_stats(self, reset: bool = False) -> Dict[str, int]:
        """Fused document searches since the last reset: questions, documents of the error bands re-scored, fp32 page dot
        products."""
        return self._stats3(self.lib.vr_index_multi_group_search_stats, ("questions", "documents", "page_dots"), reset)

    # ---- rank-fusion search (include/visrag_hip.h: vr_index_search_rrf) ----
    def search_rrf(self, queries, lims, k: int, depth: int = 100, c: float = 60.0, weights=None, filter_of_group=None,
                   documents: bool = False):
        """The k ids of largest reciprocal-rank-fusion score per group of sub-queries (include/visrag_hip.h: vr_index_search_rrf)
        -> (scores [n_groups,k] f32, ids [n_groups,k] i64, hits [n_groups,k] i32).  Every sub-query's list is what
        `search(k=depth)` returns for it (under `filter_of_group`: `search_filtered`; with `documents=True`: the groups of
        `search_groups_window(offset 0, k=depth)`, and the ids are documents); an id scores float32(sum of w_j / (c + 1 + r) over
        the lists j that hold it at 0-based position r), `hits` is the number of those lists; ids come score descending, then
        lower id first, slots past the distinct ids are (-inf, -1, 0) (documents.rrf_runs is the definition, bit for bit).
        `queries` and `lims` as in `search_multi`: flat [n_sub][dim] with `lims` [n_groups + 1], or [n_groups][m][dim] with
        `lims=None`.  `weights`: one float per sub-query, None = 1.  Groups hold 1..256 sub-queries and at most
        `rrf_max_entries()` list slots, 1 <= k, depth <= 1000.  `filter_of_group` as in `search_multi`.  cuda in -> cuda out,
        numpy / cpu in -> numpy out."""
        q, cuda, lim, ng, n_sub = self._grouped_queries(queries, lims)
        w, wptr = _rrf_weights(weights, n_sub)
        keep, fptr = self._filter_of_group(q, cuda, ng, filter_of_group)
        if cuda:
            outs = [torch.empty((ng, k), dtype=d, device=q.device) for d in (torch.float32, torch.int64, torch.int32)]
            ptrs = [x.data_ptr() for x in [q] + outs]
        else:
            outs = [np.empty((ng, max(k, 0)), dtype=d) for d in (np.float32, np.int64, np.int32)]
            ptrs = [x.ctypes.data for x in [q] + outs]
        _lib.check(self.lib.vr_index_search_rrf(self._h, C.c_void_p(ptrs[0]), n_sub, C.c_void_p(lim.ctypes.data), ng, k, int(depth),
                                                float(c), wptr, fptr, 1 if documents else 0, C.c_void_p(ptrs[1]),
                                                C.c_void_p(ptrs[2]), C.c_void_p(ptrs[3]), 1 if cuda else 0,
                                                C.c_void_p(_stream_ptr(self.device))), "vr_index_search_rrf")
        del keep, w
        return tuple(outs)

    def rrf_max_entries(self) -> int:
        """The most list slots (sub-queries x depth) one group of `search_rrf` / `rrf_fuse` may hold."""
        return int(self.lib.vr_rrf_max_entries())

    def rrf_search_stats(self, reset: bool = False) -> Dict[str, int]:
        """Rank-fusion searches since the last reset: groups, non-empty list entries, distinct ids."""
        return self._stats3(self.lib.vr_index_rrf_search_stats, ("groups", "entries", "distinct"), reset)

    def search_keys(self, queries: torch.Tensor, k: int, id_offset: int = 0) -> torch.Tensor:
        """The same search with each result packed into ONE 64-bit word (include/visrag_hip.h:
        vr_index_search_keys): orderable(score) << 32 | ~(row + id_offset); 0 = empty slot.  -> int64 [nq, k]
        on the queries' device — the buffer the ranks all-gather (retriever.sharded_search)."""
        q = queries.to(torch.float32).contiguous()
        if not q.is_cuda:
            raise ValueError("search_keys works on device tensors (the exchange buffer lives in HBM)")
        nq = q.shape[0]
        keys = torch.empty((nq, k), dtype=torch.int64, device=q.device)
        _lib.check(self.lib.vr_index_search_keys(self._h, C.c_void_p(q.data_ptr()), nq, k, int(id_offset),
                                                 C.c_void_p(keys.data_ptr()), 1, C.c_void_p(_stream_ptr(self.device))),
                   "vr_index_search_keys")
        return keys

    def set_search_eps(self, eps_rel: Optional[float]) -> None:
        """Error model of the top-k certification: None = the rigorous data-dependent default, >= 0 = eps_rel * |q| * max|d|,
        < 0 = certification off."""
        _lib.check(self.lib.vr_index_set_search_eps(self._h, float("nan") if eps_rel is None else float(eps_rel)))

    def search_stats(self, reset: bool = False) -> Dict[str, int]:
        """Queries since the last reset by outcome: certified from the sweep's candidates at once / after re-scoring more of
        them; `flagged` = redone behind the sweep, of which `band_pass` by re-scoring every row inside the error band and
        `exact_pass` = band beyond 8192 rows (the fp32 pass over the whole index, or — the first such queries of an index — one workgroup's walk); `uncertified` = searched with certification off."""
        out = (C.c_int64 * 6)()
        _lib.check(self.lib.vr_index_search_stats(self._h, out, 1 if reset else 0))
        return {"certified": int(out[0]), "certified_extended": int(out[1]), "flagged": int(out[2]),
                "band_pass": int(out[2]) - int(out[5]), "exact_pass": int(out[5]),
                "uncertified": int(out[3]), "regathered": int(out[4])}

    def search_plan(self, nq: int) -> Dict[str, int]:
        """How a search of `nq` queries (k <= 26) is laid out over the rows added so far (include/visrag_hip.h:
        vr_index_search_plan): `prepass_chunks` > 0 = the threshold pre-pass owns its sampled tiles, the sweep skips them."""
        out = (C.c_int32 * 5)()
        _lib.check(self.lib.vr_index_search_plan(self._h, int(nq), out))
        return {"list_chunks": int(out[0]), "prepass_chunks": int(out[1]), "sweep_chunks": int(out[2]), "tiles_per_chunk": int(out[3]),
                "exact_pass_launched": int(out[4])}

    def error_model(self) -> Dict[str, float]:
        """What the default certification bound is made of (include/visrag_hip.h: vr_index_set_search_eps)."""
        out = (C.c_float * 4)()
        _lib.check(self.lib.vr_index_error_model(self._h, out))
        return {"max_row_norm": float(out[0]), "max_row_bf16_residual": float(out[1]), "acc_rel": float(out[2]),
                "worst_case_eps_rel": float(out[3])}

    SEARCH_STAGES = ("convert", "thresholds", "sweep", "merge", "exact_pass")

    def set_search_profile(self, on: bool) -> None:
        _lib.check(self.lib.vr_index_set_search_profile(self._h, 1 if on else 0))

    def get_search_profile(self) -> Dict[str, float]:
        ms, calls = (C.c_double * 5)(), C.c_int64()
        _lib.check(self.lib.vr_index_get_search_profile(self._h, ms, C.byref(calls)))
        n = max(int(calls.value), 1)
        out = {name: ms[i] / n for i, name in enumerate(self.SEARCH_STAGES)}
        out["calls"] = int(calls.value)
        return out


def _rrf_weights(weights, n_lists: int):
    """`weights` of a rank fusion as a host float32 [n_lists] -> (keep-alive, pointer); None: no array (every weight 1)"""
    if weights is None:
        return None, C.c_void_p(None)
    if isinstance(weights, torch.Tensor):
        weights = weights.detach().cpu().numpy()
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float32).reshape(-1))
    if len(w) != n_lists:
        raise ValueError(f"{len(w)} weights for {n_lists} lists")
    return w, C.c_void_p(w.ctypes.data)


def rrf_fuse(ids, lims, k: int, c: float = 60.0, weights=None, device: int = 0):
    """Reciprocal-rank fusion of lists from anywhere — two indexes built with different models, pages and documents, lists
    under different filters (include/visrag_hip.h: vr_rrf_fuse) -> (scores [n_groups,k] f32, ids [n_groups,k] i64, hits
    [n_groups,k] i32), as `HipIndex.search_rrf` returns them.  `ids` [n_lists][depth] int64: slot r of list j, -1 = an empty slot;
    group g holds lists lims[g] .. lims[g + 1] - 1 (`lims=None`: [n_groups][m][depth]).  cuda in -> cuda out (on the tensor's
    device), numpy / cpu in -> numpy out (computed on `device`)."""
    _require_gpu()
    lib = _lib.load()
    cuda = isinstance(ids, torch.Tensor) and ids.is_cuda
    if cuda:
        a = ids.to(torch.int64).contiguous()
        device = a.device.index or 0
    else:
        a = np.ascontiguousarray(ids.numpy() if isinstance(ids, torch.Tensor) else ids, dtype=np.int64)
    if lims is None:
        if a.ndim != 3:
            raise ValueError("ids must be [n_groups][m][depth] when lims is None")
        lim = np.arange(a.shape[0] + 1, dtype=np.int64) * a.shape[1]
        a = a.reshape(-1, a.shape[2])
    else:
        if a.ndim != 2:
            raise ValueError("ids must be [n_lists][depth] with lims")
        lim = np.ascontiguousarray(HipIndex._row_ids(lims), dtype=np.int64)
        if len(lim) < 1:
            raise ValueError("lims must hold n_groups + 1 entries")
    ng, n_lists, depth = len(lim) - 1, int(a.shape[0]), int(a.shape[1])
    w, wptr = _rrf_weights(weights, n_lists)
    if cuda:
        outs = [torch.empty((ng, k), dtype=d, device=a.device) for d in (torch.float32, torch.int64, torch.int32)]
        ptrs = [x.data_ptr() for x in [a] + outs]
    else:
        outs = [np.empty((ng, max(k, 0)), dtype=d) for d in (np.float32, np.int64, np.int32)]
        ptrs = [x.ctypes.data for x in [a] + outs]
    _lib.check(lib.vr_rrf_fuse(int(device), C.c_void_p(ptrs[0]), n_lists, depth, C.c_void_p(lim.ctypes.data), ng, k, float(c), wptr,
                               C.c_void_p(ptrs[1]), C.c_void_p(ptrs[2]), C.c_void_p(ptrs[3]), 1 if cuda else 0,
                               C.c_void_p(_stream_ptr(int(device)))), "vr_rrf_fuse")
    del w
    return tuple(outs)


def topk_merge_keys(keys: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[n_parts, nq, k] packed keys (HipIndex.search_keys of every shard, e.g. the all-gather's output as it is)
    -> merged (scores [nq, k] f32, global ids [nq, k] i64) on the device."""
    _require_gpu()
    lib = _lib.load()
    n_parts, nq, k = keys.shape
    keys = keys.contiguous()
    os_ = torch.empty((nq, k), dtype=torch.float32, device=keys.device)
    oi = torch.empty((nq, k), dtype=torch.int64, device=keys.device)
    dev = keys.device.index or 0
    _lib.check(lib.vr_topk_merge_keys(dev, C.c_void_p(keys.data_ptr()), n_parts, nq, k, C.c_void_p(os_.data_ptr()),
                                      C.c_void_p(oi.data_ptr()), C.c_void_p(_stream_ptr(dev))), "vr_topk_merge_keys")
    return os_, oi


def topk_merge(scores: torch.Tensor, ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[n_parts, nq, k] per-shard (score, global id) lists -> merged [nq, k] (device tensors)."""
    _require_gpu()
    lib = _lib.load()
    n_parts, nq, k = scores.shape
    scores = scores.contiguous().to(torch.float32)
    ids = ids.contiguous().to(torch.int64)
    os_ = torch.empty((nq, k), dtype=torch.float32, device=scores.device)
    oi = torch.empty((nq, k), dtype=torch.int64, device=scores.device)
    dev = scores.device.index or 0
    _lib.check(lib.vr_topk_merge(dev, C.c_void_p(scores.data_ptr()), C.c_void_p(ids.data_ptr()),
                                 n_parts, nq, k, C.c_void_p(os_.data_ptr()), C.c_void_p(oi.data_ptr()),
                                 C.c_void_p(_stream_ptr(dev))), "vr_topk_merge")
    return os_, oi
