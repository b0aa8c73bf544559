"""Helpers for the -m gpu tests: call the op-level C-ABI entry points on torch containers."""
import ctypes as C

import torch

from visrag_amd import _lib


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def pad_rows(t, mult=256):
    r = (t.shape[0] + mult - 1) // mult * mult
    if r == t.shape[0]:
        return t.contiguous()
    out = torch.zeros((r,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
    out[: t.shape[0]] = t
    return out


def op_gemm(A, W, epi, bias=None, resid=None, alpha=1.0, out_dtype=torch.bfloat16, out_cols=None,
            rope_pos=None, rope_table=None, rope_cols=0, variant=0):
    """A [M,K] bf16, W [N,K] bf16 (cuda) -> out [M, out_cols]."""
    lib = _lib.load()
    M, K = A.shape
    N = W.shape[0]
    Ap = pad_rows(A)
    out_cols = out_cols or N
    out = torch.zeros((Ap.shape[0], out_cols), dtype=out_dtype, device=A.device)
    if resid is not None:
        resid = pad_rows(resid.to(torch.float32))
    _lib.check(lib.vr_op_gemm(A.device.index or 0, P(Ap), K, P(W.contiguous()), K, M, N, K, epi, P(bias), P(resid),
                              float(alpha), P(out), out_cols, P(rope_pos), P(rope_table), rope_cols, variant, None),
               "vr_op_gemm")
    torch.cuda.synchronize()
    return out[:M]


def op_norm(kind, x, w, b, eps, ldo=None):
    lib = _lib.load()
    rows, dim = x.shape
    ldo = ldo or dim
    out = torch.full((rows, ldo), 7.0, dtype=torch.bfloat16, device=x.device)
    _lib.check(lib.vr_op_norm(x.device.index or 0, kind, P(x.contiguous()), rows, dim, P(w), P(b), float(eps), P(out),
                              ldo, None), "vr_op_norm")
    torch.cuda.synchronize()
    return out


def op_attention(q, k, v, cu_q, cu_kv, heads, hd, max_q, causal, q_shared, scale, rows_out):
    lib = _lib.load()
    out = torch.zeros((rows_out, heads * hd), dtype=torch.bfloat16, device=q.device)
    B = cu_kv.numel() - 1
    _lib.check(lib.vr_op_attention(q.device.index or 0, P(q), q.stride(0), P(k), k.stride(0), P(v), v.stride(0),
                                   P(out), out.stride(0), P(cu_q), P(cu_kv), B, heads, hd, max_q, int(causal),
                                   int(q_shared), float(scale), None), "vr_op_attention")
    torch.cuda.synchronize()
    return out


def from_bf16_bits(bits, device="cuda:0"):
    """uint16 bf16 bit patterns (numpy) -> torch.bfloat16 on the device"""
    import numpy as np
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(device).view(torch.bfloat16)


def _i32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


def op_gemm_skinny(A, W, M, N, K, ksplit=1, bias=None, swiglu=False, out=None, ldo=None, split_stride=None):
    """A bf16 [>= 16 / 32 rows][K], W bf16 [multiple of 256 rows][K] (the caller pads) -> `out`, written in place: fp32
    planes [ksplit][rows][ldo], or bf16 act [rows][ldo] with swiglu."""
    lib = _lib.load()
    ldo = ldo or out.shape[-1]
    split_stride = split_stride if split_stride is not None else (out.shape[-2] * out.shape[-1] if out.dim() == 3 else 0)
    _lib.check(lib.vr_op_gemm_skinny(A.device.index or 0, P(A), A.stride(0), P(W), W.stride(0), M, N, K, ksplit, P(bias), int(swiglu),
                                     P(out), ldo, split_stride, None), "vr_op_gemm_skinny")
    torch.cuda.synchronize()
    return out


def op_plane_sum(kind, parts, rows, dim, x=None, alpha=1.0, weight=None, eps=1e-5, out=None):
    """parts fp32 [nsplit][rows_alloc][ldp]; kind 0: x fp32 [rows][ldx] updated in place, out bf16 [rows][ldo] or None;
    kind 1: out bf16 [rows][ldo] = SwiGLU of the summed planes."""
    lib = _lib.load()
    nsplit, ldp = parts.shape[0], parts.shape[2]
    _lib.check(lib.vr_op_plane_sum(parts.device.index or 0, kind, P(parts), nsplit, parts.stride(0), ldp, rows, dim, P(x),
                                   x.stride(0) if x is not None else 0, float(alpha), P(weight), float(eps), P(out),
                                   out.stride(0) if out is not None else 0, None), "vr_op_plane_sum")
    torch.cuda.synchronize()
    return out


def op_chat_attention(q, prompt, tails, l, step_row, step_slot, step_tail, slot_plen, force_splits=0):
    """q bf16 [n][E]; prompt bf16 [L][2][slots][max_len][E]; tails bf16 [L][2][rows][max_new][E] -> att bf16 [n][E]"""
    lib = _lib.load()
    n, E = q.shape
    L, _, slots, max_len, _ = prompt.shape
    rows, max_new = tails.shape[2], tails.shape[3]
    att = torch.full((n, E), 7.0, dtype=torch.bfloat16, device=q.device)
    _lib.check(lib.vr_op_chat_attention(q.device.index or 0, P(q), P(prompt), P(tails), L, l, E, slots, max_len, rows, max_new, n,
                                        _i32(step_row), _i32(step_slot), _i32(step_tail), _i32(slot_plen), force_splits, P(att),
                                        None), "vr_op_chat_attention")
    torch.cuda.synchronize()
    return att


def op_chat_select(mode, logits, seen, V, group_offsets, K, kout, beam_scores=None, penalty=1.0, temperature=1.0, seed=0, step=0):
    """logits fp32 [n][ld], seen int32 words [n][words] (cuda) -> (scores, tokens, parents), numpy [groups][kout]"""
    import numpy as np
    lib = _lib.load()
    G = len(group_offsets) - 1
    n = group_offsets[-1]
    sc = np.zeros((G, kout), dtype=np.float32)
    tk = np.zeros((G, kout), dtype=np.int32)
    pa = np.zeros((G, kout), dtype=np.int32)
    bs = (C.c_float * n)(*[float(x) for x in beam_scores]) if beam_scores is not None else None
    p32 = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    _lib.check(lib.vr_op_chat_select(logits.device.index or 0, int(mode), P(logits), logits.stride(0), V, P(seen), seen.stride(0), G,
                                     _i32(group_offsets), bs, K, kout, float(penalty), float(temperature),
                                     C.c_uint64(int(seed) & (2 ** 64 - 1)), int(step), sc.ctypes.data_as(C.POINTER(C.c_float)), p32(tk),
                                     p32(pa), None), "vr_op_chat_select")
    return sc, tk, pa


# ---- every launch argument (tests/test_gpu_launch_args.py).  The caller owns the output tensor and prefills it with a sentinel:
#      a zero fill here would hide a row that was never written.
def op_gemm_ex(A, W, M, N, epi, out, bias=None, resid=None, alpha=1.0, rope_pos=None, rope_table=None, rope_cols=0, variant=0,
               ldo=None, rowmap=None, rowbias=None, rowbias_period=0, rowbias_ld=None, rowbias_cols=0, col_scale=0.0,
               col_scale_n=0, ksplit=0, split_stride=0, m_dev=None, m_sub=0, raster_gm=0):
    """A bf16 [M padded by the caller][K], W bf16 [N padded by the caller][K] -> `out`, written in place (row pitch ldo);
    resid f32 with out's row pitch; rowmap / m_dev int32 and rowbias f32 on the device."""
    lib = _lib.load()
    K = W.shape[1]
    ex = _lib.VRGemmExtras(rowmap=rowmap.data_ptr() if rowmap is not None else None,
                           rowbias=rowbias.data_ptr() if rowbias is not None else None, rowbias_period=rowbias_period,
                           rowbias_ld=(rowbias_ld if rowbias_ld is not None else (rowbias.stride(0) if rowbias is not None else 0)),
                           rowbias_cols=rowbias_cols, col_scale=float(col_scale), col_scale_n=col_scale_n, ksplit=ksplit,
                           split_stride=split_stride, m_dev=m_dev.data_ptr() if m_dev is not None else None, m_sub=m_sub,
                           raster_gm=raster_gm)
    ldo = ldo if ldo is not None else out.stride(-2)
    _lib.check(lib.vr_op_gemm_ex(A.device.index or 0, P(A), A.stride(0), P(W), W.stride(0), M, N, K, epi, P(bias), P(resid),
                                 float(alpha), P(out), ldo, P(rope_pos), P(rope_table), rope_cols, variant, C.byref(ex), None),
               "vr_op_gemm_ex")
    torch.cuda.synchronize()
    return out


def op_attention_ex(q, k, v, out, cu_q, cu_kv, heads, hd, max_q, causal, q_shared, scale, B=None, ldq=None, kv_group=0,
                    kv_end=None, q_in_rows=None, q_head_stride=0, q_prescaled=0, lse=None):
    """`out` bf16 (and `lse` f32 [rows_q][heads]) are the caller's, prefilled with a sentinel"""
    lib = _lib.load()
    ex = _lib.VRAttnExtras(kv_group=kv_group, kv_end=kv_end.data_ptr() if kv_end is not None else None,
                           q_in_rows=q_in_rows.data_ptr() if q_in_rows is not None else None, q_head_stride=q_head_stride,
                           q_prescaled=int(q_prescaled), lse=lse.data_ptr() if lse is not None else None)
    B = B if B is not None else cu_kv.numel() - 1
    _lib.check(lib.vr_op_attention_ex(q.device.index or 0, P(q), ldq if ldq is not None else q.stride(0), P(k), k.stride(0), P(v),
                                      v.stride(0), P(out), out.stride(0), P(cu_q), P(cu_kv), B, heads, hd, max_q, int(causal),
                                      int(q_shared), float(scale), C.byref(ex), None), "vr_op_attention_ex")
    torch.cuda.synchronize()
    return out


# the values of vr_op_attention_route (include/visrag_hip.h)
ROUTE_REFUSED, ROUTE_NONE, ROUTE_SMALL, ROUTE_72W = -1, 0, 1, 2


def route_tiled(hd, qf, pipe):
    return 100000 + hd * 100 + qf * 10 + pipe


def op_attention_route(q, ldq, k, ldk, v, ldv, out, ldo, cu_q, cu_kv, B, heads, hd, max_q, causal=False, q_shared=False, scale=1.0,
                       kv_group=0, kv_end=None, q_in_rows=None, q_head_stride=0, q_prescaled=0, lse=None):
    """The kernel vr_op_attention_ex reaches with these arguments.  Pointers are plain integers (addresses): the entry compares
    them and dereferences none, so it runs without a GPU and on made-up values."""
    lib = _lib.load()
    ex = _lib.VRAttnExtras(kv_group=kv_group, kv_end=kv_end, q_in_rows=q_in_rows, q_head_stride=q_head_stride,
                           q_prescaled=int(q_prescaled), lse=lse)
    return int(lib.vr_op_attention_route(0, q, ldq, k, ldk, v, ldv, out, ldo, cu_q, cu_kv, B, heads, hd, max_q, int(causal),
                                         int(q_shared), float(scale), C.byref(ex)))


def attention_route_of(q, k, v, out, cu_q, cu_kv, heads, hd, max_q, causal, q_shared, scale, B=None, ldq=None, kv_group=0,
                       kv_end=None, q_in_rows=None, q_head_stride=0, q_prescaled=0, lse=None):
    """op_attention_route with the arguments of op_attention_ex (tensors)"""
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    return op_attention_route(ptr(q), ldq if ldq is not None else q.stride(0), ptr(k), k.stride(0), ptr(v), v.stride(0), ptr(out),
                              out.stride(0), ptr(cu_q), ptr(cu_kv), B if B is not None else cu_kv.numel() - 1, heads, hd, max_q,
                              causal, q_shared, scale, kv_group=kv_group, kv_end=ptr(kv_end), q_in_rows=ptr(q_in_rows),
                              q_head_stride=q_head_stride, q_prescaled=q_prescaled, lse=ptr(lse))


def op_attn_combine(part, lse, heads, group, out, S=0, S_dev=None, n_rows=1, ld_out=0, W=None, M=1, N=0, K=0, ksplit=1,
                    planes=1, ldo=0, split_stride=0):
    """part bf16 / lse f32: a decode attention's partial rows (layout: SkinnyCombine, csrc/kernels.h).  W None: `out` bf16
    [n_rows][ld_out] merged rows; W bf16 [N padded to 256][K]: `out` fp32 planes [planes][M][ldo] of merged @ W^T."""
    lib = _lib.load()
    _lib.check(lib.vr_op_attn_combine(part.device.index or 0, P(part), P(lse), S, P(S_dev), heads, group, n_rows, P(out), ld_out,
                                      P(W), W.stride(0) if W is not None else 0, M, N, K, ksplit, planes, ldo, split_stride, None),
               "vr_op_attn_combine")
    torch.cuda.synchronize()
    return out


# ---- the fp32 text path and the encode glue kernels (tests/test_gpu_text_ops.py).  As above the outputs are the caller's,
#      prefilled with a sentinel; pointers are passed as they are, so a view into a larger guarded buffer can be handed in.
def op_norm_ex(kind, x, rows, dim, ldx, w, b, eps, out, ldo):
    lib = _lib.load()
    _lib.check(lib.vr_op_norm_ex(x.device.index or 0, kind, P(x), rows, dim, ldx, P(w), P(b), float(eps), P(out), ldo, None), "vr_op_norm_ex")
    torch.cuda.synchronize()
    return out


def op_text_rmsnorm_split(x, rows, dim, w, eps, hi, lo):
    lib = _lib.load()
    _lib.check(lib.vr_op_text_rmsnorm_split(x.device.index or 0, P(x), rows, dim, P(w), float(eps), P(hi), P(lo), None), "vr_op_text_rmsnorm_split")
    torch.cuda.synchronize()


def op_text_rope(qkv, T, ld, rope_cols, pos, table):
    lib = _lib.load()
    _lib.check(lib.vr_op_text_rope(qkv.device.index or 0, P(qkv), T, ld, rope_cols, P(pos), P(table), None), "vr_op_text_rope")
    torch.cuda.synchronize()
    return qkv


def op_text_attention(qkv, ld, E, seq_offsets, B, T, heads, scale, out):
    lib = _lib.load()
    _lib.check(lib.vr_op_text_attention(qkv.device.index or 0, P(qkv), ld, E, P(seq_offsets), B, T, heads, float(scale), P(out), None),
               "vr_op_text_attention")
    torch.cuda.synchronize()
    return out


def op_text_swiglu_split(gu, T, ld_gu, I, ld_act, hi, lo):
    lib = _lib.load()
    _lib.check(lib.vr_op_text_swiglu_split(gu.device.index or 0, P(gu), T, ld_gu, I, ld_act, P(hi), P(lo), None), "vr_op_text_swiglu_split")
    torch.cuda.synchronize()


def op_embed_gather(ids, T, table, table_lo, dim, scale, out):
    lib = _lib.load()
    _lib.check(lib.vr_op_embed_gather(ids.device.index or 0, P(ids), T, P(table), P(table_lo), dim, float(scale), P(out), None), "vr_op_embed_gather")
    torch.cuda.synchronize()
    return out


def op_pool(h, seq_offsets, B, dim, w, eps, out, tap, mode):
    lib = _lib.load()
    _lib.check(lib.vr_op_pool(h.device.index or 0, P(h), P(seq_offsets), B, dim, P(w), float(eps), P(out), P(tap), mode, None), "vr_op_pool")
    torch.cuda.synchronize()
    return out


def op_convert(kind, src, out=None, out2=None, n=0, n_total=0, aux=None):
    """kind 0 f32 -> bf16, 1 the same + zeros up to n_total (aux: two i32 cleared), 2 hi / lo split, 3 *aux |= any non-zero 16-bit
    word, 4 / 5 positions / sequence index of the tokens of src = seq_offsets [n + 1]"""
    lib = _lib.load()
    _lib.check(lib.vr_op_convert(src.device.index or 0, kind, P(src), P(out), P(out2), int(n), int(n_total), P(aux), None), "vr_op_convert")
    torch.cuda.synchronize()


def op_planes_sum(parts, n_parts, stride, ldp, T, N, out, ldo, alpha, accumulate):
    lib = _lib.load()
    _lib.check(lib.vr_op_planes_sum(parts.device.index or 0, P(parts), n_parts, int(stride), ldp, T, N, P(out), ldo, float(alpha), int(accumulate),
                                    None), "vr_op_planes_sum")
    torch.cuda.synchronize()
    return out


def op_patch_embed(imgs, H, W, patch, weight, D, K, bias, pos, ld_pos, out, ldo):
    """imgs: a list of u8 HWC device tensors; weight f32 [D][3][patch][patch]; out f32 [>= n (H / patch)(W / patch)][ldo]"""
    lib = _lib.load()
    ptrs = (C.c_void_p * len(imgs))(*[t.data_ptr() for t in imgs])
    _lib.check(lib.vr_op_patch_embed(weight.device.index or 0, ptrs, len(imgs), H, W, patch, P(weight), D, K, P(bias), P(pos), ld_pos, P(out), ldo,
                                     None), "vr_op_patch_embed")
    torch.cuda.synchronize()
    return out


# ---- the EVisRAG generator's small kernels (tests/test_gpu_gen_ops.py).  Outputs are the caller's, prefilled with a sentinel.
def op_gen_mrope_cache(T, H, KV, pos3, pos_stride, sections, inv_freq, q_out, ldq, k_cache, v_cache, ld_cache, ld, src=None, parts=None,
                       n_parts=0, plane_stride=0, bias=None, cache_row0=0, row0_dev=None, cache_rows=None, cu_kv=None):
    lib = _lib.load()
    _lib.check(lib.vr_op_gen_mrope_cache(k_cache.device.index or 0 if k_cache is not None else 0, P(src), P(parts), n_parts, int(plane_stride), P(bias), ld, T, H, KV, P(pos3),
                                         pos_stride, sections[0], sections[1], P(inv_freq), P(q_out), ldq, P(k_cache), P(v_cache), ld_cache,
                                         cache_row0, P(row0_dev), P(cache_rows), P(cu_kv), None), "vr_op_gen_mrope_cache")
    torch.cuda.synchronize()


def op_gen_rope2d(qkv, ld, T, n_slots, hh, pos_h, pos_w, sec_h, freq):
    lib = _lib.load()
    dev = freq.device.index or 0 if freq is not None else 0
    _lib.check(lib.vr_op_gen_rope2d(dev, P(qkv), ld, T, n_slots, hh, P(pos_h), P(pos_w), sec_h, P(freq), None), "vr_op_gen_rope2d")
    torch.cuda.synchronize()
    return qkv


def op_gen_sample(logits, vocab, seen, penalty=1.0, temperature=0.0, seed=0, step=0, state=None, step_from_state=False, advance=False):
    """logits f32 [>= vocab], seen int32 words, state int32 [42] or None (all cuda) -> the pick (also marked in `seen`)"""
    lib = _lib.load()
    tok = C.c_int32(-7)
    dev = seen.device.index or 0 if seen is not None else 0
    _lib.check(lib.vr_op_gen_sample(dev, P(logits), vocab, P(seen), float(penalty), float(temperature), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                    int(step), P(state), int(step_from_state), int(advance), C.byref(tok), None), "vr_op_gen_sample")
    return int(tok.value)


def op_gen_mark_seen(ids, n, seen, vocab):
    lib = _lib.load()
    dev = seen.device.index or 0 if seen is not None else 0
    _lib.check(lib.vr_op_gen_mark_seen(dev, P(ids), n, P(seen), vocab, None), "vr_op_gen_mark_seen")
    torch.cuda.synchronize()
    return seen


def op_gen_decode_begin(state, q_rows):
    lib = _lib.load()
    _lib.check(lib.vr_op_gen_decode_begin(state.device.index or 0 if state is not None else 0, P(state), q_rows, None), "vr_op_gen_decode_begin")
    torch.cuda.synchronize()
    return state


def op_gen_rows(kind, n, dst, ld, src=None, row_idx=None, dim=0, pages=None, page_w=None, img=None, ph=None, pw=None, patch=0, tp=0,
                mean=None, std=None):
    """kind 0 scatter f32 rows, 1 gather to bf16 + zero pad, 2 u8 patch rows (pages: a list of u8 HWC device tensors)"""
    lib = _lib.load()
    ptrs = (C.c_void_p * len(pages))(*[t.data_ptr() if t is not None else None for t in pages]) if pages is not None else None
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v]) if v is not None else None  # noqa: E731
    dev = dst.device.index or 0 if dst is not None else 0
    _lib.check(lib.vr_op_gen_rows(dev, kind, P(src), P(row_idx), n, dim, P(dst), ld, ptrs, _i32(page_w) if page_w is not None else None,
                                  len(pages) if pages is not None else 0, P(img), P(ph), P(pw), patch, tp, f3(mean), f3(std), None),
               "vr_op_gen_rows")
    torch.cuda.synchronize()
    return dst
