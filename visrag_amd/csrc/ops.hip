// Stand-alone entry points of libvisrag_hip.so: page resize, synthetic pages, the stream-overlap probe and the op-level
// calls (vr_op_*) the kernel tests drive.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "engine_common.h"

// -------------------------------------------------------------------------------- resize ---
// coefficient tables are cached per (device, in, out): a corpus has a handful of page sizes
struct ResizeTab { DevBuf bounds, kk; int ksize = 0; };
static std::map<std::tuple<int, int, int>, ResizeTab> g_resize_tabs;

static int get_resize_tab(int dev, int in_size, int out_size, ResizeTab** out) {
    auto key = std::make_tuple(dev, in_size, out_size);
    auto it = g_resize_tabs.find(key);
    if (it == g_resize_tabs.end()) {
        std::vector<int> b, k;
        ResizeTab t;
        t.ksize = resize_coeffs(in_size, out_size, b, k);
        VRCHK(t.bounds.alloc(b.size() * 4));
        VRCHK(t.kk.alloc(k.size() * 4));
        HIPCHK(hipMemcpy(t.bounds.p, b.data(), b.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(t.kk.p, k.data(), k.size() * 4, hipMemcpyHostToDevice));
        it = g_resize_tabs.emplace(key, std::move(t)).first;
    }
    *out = &it->second;
    return VR_OK;
}

// grow-only staging buffers per (device, stream): the resize of a page costs no allocation, no
// clear and no stream synchronisation, so it stays asynchronous next to another stream's batch
struct ResizeScratch { DevBuf in, tmp; };
static std::map<std::pair<int, void*>, ResizeScratch> g_resize_scratch;

extern "C" int vr_resize_bicubic(int device_id, const uint8_t* src, int32_t src_on_device, int32_t H, int32_t W,
                                 uint8_t* dst, int32_t out_h, int32_t out_w, void* stream) {
    if (!src || !dst || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0) return fail(VR_ERR_INVALID, "bad resize arguments");
    VRCHK(set_dev(device_id));
    hipStream_t s = (hipStream_t)stream;
    ResizeScratch& sc = g_resize_scratch[std::make_pair(device_id, stream)];
    const uint8_t* in = src;
    if (!src_on_device) {
        VRCHK(sc.in.reserve((size_t)H * W * 3));
        HIPCHK(hipMemcpyAsync(sc.in.p, src, (size_t)H * W * 3, hipMemcpyHostToDevice, s));
        in = sc.in.as<uint8_t>();
    }
    const bool need_h = out_w != W, need_v = out_h != H;
    if (!need_h && !need_v) {
        HIPCHK(hipMemcpyAsync(dst, in, (size_t)H * W * 3, hipMemcpyDeviceToDevice, s));
    } else {
        const uint8_t* mid = in;
        if (need_h) {
            ResizeTab* th = nullptr;
            VRCHK(get_resize_tab(device_id, W, out_w, &th));
            uint8_t* hout = dst;
            if (need_v) { VRCHK(sc.tmp.reserve((size_t)H * out_w * 3)); hout = sc.tmp.as<uint8_t>(); }
            HIPCHK(launch_resize_h(in, W, H, hout, out_w, th->bounds.as<int>(), th->kk.as<int>(), th->ksize, s));
            mid = hout;
        }
        if (need_v) {
            ResizeTab* tv = nullptr;
            VRCHK(get_resize_tab(device_id, H, out_h, &tv));
            HIPCHK(launch_resize_v(mid, out_w, dst, out_h, tv->bounds.as<int>(), tv->kk.as<int>(), tv->ksize, s));
        }
    }
    if (!src_on_device) HIPCHK(hipStreamSynchronize(s));     // the caller may reuse its host buffer
    return VR_OK;
}

// ------------------------------------------------------------------------- synthetic input ---
extern "C" int vr_synth_pages(int device_id, uint8_t* out, int32_t n, int32_t size, int64_t seed, int64_t first, void* stream) {
    if (!out || n < 0 || size < 64 || size > 4096) return fail(VR_ERR_INVALID, "bad synth_pages arguments");
    VRCHK(set_dev(device_id));
    HIPCHK(launch_synth_pages(out, n, size, seed, first, (hipStream_t)stream));
    return VR_OK;
}

// ------------------------------------------------------------------- streams and queues ---
// HIP maps a process's streams onto a handful of hardware queues (four by default); two streams that land on ONE queue
// run their kernels one behind the other, and a caller keeping two batches in flight on them gets the single-stream
// rate plus the bookkeeping (measured, round 4: streams 2 and 3 of torch's pool in a fresh process, 661 against 711
// pages/s for every other neighbouring pair).  The mapping is the runtime's business, so it is PROBED: a one-thread
// kernel spins for `usec` on each stream; together they take `usec` if the streams overlap and twice that if not.
__global__ void spin_kernel(long long ticks) {
    const long long t0 = wall_clock64();                     // (the constant 100 MHz counter)
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

extern "C" int vr_streams_overlap(int device_id, void* stream_a, void* stream_b, int32_t* overlap) {
    if (!overlap) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    const hipStream_t a = (hipStream_t)stream_a, b = (hipStream_t)stream_b;
    constexpr int usec = 400;
    int votes = 0;
    for (int rep = 0; rep < 3; ++rep) {                      // (first round: also the kernel's load)
        HIPCHK(hipStreamSynchronize(a));
        HIPCHK(hipStreamSynchronize(b));
        const auto t0 = std::chrono::steady_clock::now();
        hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(1), 0, a, (long long)usec * 100);
        hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(1), 0, b, (long long)usec * 100);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(a));
        HIPCHK(hipStreamSynchronize(b));
        const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        if (rep > 0) votes += us < 1.6 * usec ? 1 : 0;
    }
    *overlap = votes == 2 ? 1 : 0;
    return VR_OK;
}

// ------------------------------------------------------------------------------ op-level ---
// the shape test of the GEMM entries: the tile columns of the variant asked for divide N (AUTO: 128), K whole steps, rows
static bool gemm_shape_refused(int32_t M, int32_t N, int32_t K, int32_t variant) {
    const int cols = variant == GEMM_VARIANT_288W ? 288 : (variant == GEMM_VARIANT_192 || variant == GEMM_VARIANT_192W || variant == GEMM_VARIANT_128W_192) ? 192 : 128;
    return N % cols || K % 64 || M <= 0;
}

// (extras: the fields of GemmArgs beyond vr_op_gemm's arguments, copied as they are — what is legal is the launchers' decision)
extern "C" int vr_op_gemm_warm(int device_id, const void* A, int32_t lda, const void* W, int32_t ldw, int32_t M, int32_t N,
                               int32_t K, int32_t epilogue, const float* bias, const float* resid, float alpha, void* out,
                               int32_t ldo, const int32_t* rope_pos, const float* rope_table, int32_t rope_cols,
                               int32_t variant, const vr_gemm_extras_t* extras, const void* warm, uint64_t warm_bytes, void* stream) {
    if (!A || !W || !out) return fail(VR_ERR_INVALID, "NULL argument");
    if (variant != GEMM_VARIANT_GLDS && variant != GEMM_VARIANT_AUTO && variant != GEMM_VARIANT_192 && variant != GEMM_VARIANT_256IL && variant != GEMM_VARIANT_256W && variant != GEMM_VARIANT_192W &&
        variant != GEMM_VARIANT_128W_192 && variant != GEMM_VARIANT_128W_256 && variant != GEMM_VARIANT_288W)
        return fail(VR_ERR_INVALID, "variant %d: 0 (128^2 tile), 3 (auto), 7 (256x192 tile), 9 (256^2 tile), 12 / 13 / 16 (256^2 / 256x192 / 256x288 tile, one wave per SIMD), 14 / 15 (128x192 / 128x256 tile, one wave per SIMD)", variant);
    if (gemm_shape_refused(M, N, K, variant)) return fail(VR_ERR_INVALID, "need N %% 128 == 0 (192 for variants 7, 13 and 14, 288 for variant 16), K %% 64 == 0");
    if (epilogue == EPI_RESID && !resid) return fail(VR_ERR_INVALID, "EPI_RESID needs resid");
    if (epilogue == EPI_ROPE && (!rope_pos || !rope_table)) return fail(VR_ERR_INVALID, "EPI_ROPE needs tables");
    VRCHK(set_dev(device_id));
    GemmArgs a{};
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.M = M; a.N = N; a.K = K; a.bias = bias; a.resid = resid;
    a.alpha = alpha; a.out = out; a.ldo = ldo; a.rope_pos = rope_pos; a.rope_table = rope_table; a.rope_cols = rope_cols;
    if (extras) {
        a.rowmap = extras->rowmap;
        a.rowbias = extras->rowbias; a.rowbias_period = extras->rowbias_period; a.rowbias_ld = extras->rowbias_ld; a.rowbias_cols = extras->rowbias_cols;
        a.col_scale = extras->col_scale; a.col_scale_n = extras->col_scale_n;
        a.ksplit = extras->ksplit; a.split_stride = (size_t)extras->split_stride;
        a.m_dev = extras->m_dev; a.m_sub = extras->m_sub;
        a.raster_gm = extras->raster_gm;
    }
    a.warm = warm; a.warm_bytes = (size_t)warm_bytes;
    // (the 256x288 tile is one epilogue form and no optional field: what it does not take is an argument error of this entry)
    if (variant == GEMM_VARIANT_288W && gemm_route(a, epilogue, variant) == GEMM_ROUTE_REFUSED)
        return fail(VR_ERR_INVALID, "variant 16 takes the residual epilogue without a row map, row bias, split K, column scale, device-side row count or region to warm");
    HIPCHK(launch_gemm(a, epilogue, variant, (hipStream_t)stream));
    return VR_OK;
}

extern "C" int vr_op_gemm_ex(int device_id, const void* A, int32_t lda, const void* W, int32_t ldw, int32_t M, int32_t N,
                             int32_t K, int32_t epilogue, const float* bias, const float* resid, float alpha, void* out,
                             int32_t ldo, const int32_t* rope_pos, const float* rope_table, int32_t rope_cols,
                             int32_t variant, const vr_gemm_extras_t* extras, void* stream) {
    return vr_op_gemm_warm(device_id, A, lda, W, ldw, M, N, K, epilogue, bias, resid, alpha, out, ldo, rope_pos, rope_table, rope_cols,
                           variant, extras, nullptr, 0, stream);
}

extern "C" int vr_op_gemm(int device_id, const void* A, int32_t lda, const void* W, int32_t ldw, int32_t M, int32_t N,
                          int32_t K, int32_t epilogue, const float* bias, const float* resid, float alpha, void* out,
                          int32_t ldo, const int32_t* rope_pos, const float* rope_table, int32_t rope_cols,
                          int32_t variant, void* stream) {
    return vr_op_gemm_ex(device_id, A, lda, W, ldw, M, N, K, epilogue, bias, resid, alpha, out, ldo, rope_pos, rope_table, rope_cols,
                         variant, nullptr, stream);
}

// the variant that call reaches (AUTO resolved), or VR_GEMM_ROUTE_REFUSED: no device is selected, nothing is launched, no
// pointer is dereferenced (those of `extras` are compared with null); launch_gemm dispatches on the same function
extern "C" int vr_op_gemm_route(int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t variant, int32_t lda, int32_t ldw,
                                int32_t ldo, const vr_gemm_extras_t* extras, uint64_t warm_bytes) {
    if (variant != GEMM_VARIANT_GLDS && variant != GEMM_VARIANT_AUTO && variant != GEMM_VARIANT_192 && variant != GEMM_VARIANT_256IL && variant != GEMM_VARIANT_256W && variant != GEMM_VARIANT_192W &&
        variant != GEMM_VARIANT_128W_192 && variant != GEMM_VARIANT_128W_256 && variant != GEMM_VARIANT_288W)
        return VR_GEMM_ROUTE_REFUSED;
    if (gemm_shape_refused(M, N, K, variant)) return VR_GEMM_ROUTE_REFUSED;
    GemmArgs a{};
    a.lda = lda; a.ldw = ldw; a.M = M; a.N = N; a.K = K; a.ldo = ldo;
    if (extras) {
        a.rowmap = extras->rowmap;
        a.rowbias = extras->rowbias; a.rowbias_period = extras->rowbias_period; a.rowbias_ld = extras->rowbias_ld; a.rowbias_cols = extras->rowbias_cols;
        a.col_scale = extras->col_scale; a.col_scale_n = extras->col_scale_n;
        a.ksplit = extras->ksplit; a.split_stride = (size_t)extras->split_stride;
        a.m_dev = extras->m_dev; a.m_sub = extras->m_sub;
        a.raster_gm = extras->raster_gm;
    }
    if (warm_bytes) { a.warm = &a; a.warm_bytes = (size_t)warm_bytes; }      // (any non-null address: the launchers compare it with null)
    const int r = gemm_route(a, epilogue, variant);
    return r == GEMM_ROUTE_REFUSED ? VR_GEMM_ROUTE_REFUSED : r;
}

extern "C" int vr_op_norm(int device_id, int32_t kind, const float* x, int32_t rows, int32_t dim, const float* weight,
                          const float* bias, float eps, void* out, int32_t ldo, void* stream) {
    if (!x || !weight || !out || (kind == 0 && !bias)) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    if (kind == 0) HIPCHK(launch_layernorm(x, rows, dim, dim, weight, bias, eps, out, ldo, (hipStream_t)stream));
    else HIPCHK(launch_rmsnorm(x, rows, dim, dim, weight, eps, out, ldo, (hipStream_t)stream));
    return VR_OK;
}

static AttnArgs attn_args_of(const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v, int32_t ldv, void* out,
                             int32_t ldo, const int32_t* cu_q, const int32_t* cu_kv, int32_t B, int32_t heads, int32_t head_dim,
                             int32_t max_q, int32_t causal, int32_t q_shared, float scale, const vr_attn_extras_t* extras) {
    AttnArgs a{};
    a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv; a.out = out; a.ldo = ldo; a.cu_q = cu_q;
    a.cu_kv = cu_kv; a.B = B; a.heads = heads; a.head_dim = head_dim; a.max_q = max_q; a.causal = causal;
    a.q_shared = q_shared; a.scale = scale;
    if (extras) {
        a.kv_group = extras->kv_group; a.kv_end = extras->kv_end; a.q_in_rows = extras->q_in_rows;
        a.q_head_stride = extras->q_head_stride; a.q_prescaled = extras->q_prescaled; a.lse = extras->lse;
    }
    return a;
}

extern "C" int vr_op_attention_ex(int device_id, const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v,
                                  int32_t ldv, void* out, int32_t ldo, const int32_t* cu_q, const int32_t* cu_kv, int32_t B,
                                  int32_t heads, int32_t head_dim, int32_t max_q, int32_t causal, int32_t q_shared,
                                  float scale, const vr_attn_extras_t* extras, void* stream) {
    if (!q || !k || !v || !out || !cu_q || !cu_kv) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    const AttnArgs a = attn_args_of(q, ldq, k, ldk, v, ldv, out, ldo, cu_q, cu_kv, B, heads, head_dim, max_q, causal, q_shared, scale,
                                    extras);
    HIPCHK(launch_attention(a, (hipStream_t)stream));
    return VR_OK;
}

// the kernel that call would reach: no device is selected, nothing is launched, no pointer is dereferenced
extern "C" int vr_op_attention_route(int device_id, const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v,
                                     int32_t ldv, void* out, int32_t ldo, const int32_t* cu_q, const int32_t* cu_kv, int32_t B,
                                     int32_t heads, int32_t head_dim, int32_t max_q, int32_t causal, int32_t q_shared,
                                     float scale, const vr_attn_extras_t* extras) {
    (void)device_id;
    if (!q || !k || !v || !out || !cu_q || !cu_kv) return VR_ATTN_ROUTE_REFUSED;
    const AttnRoute r = attention_route(attn_args_of(q, ldq, k, ldk, v, ldv, out, ldo, cu_q, cu_kv, B, heads, head_dim, max_q, causal,
                                                     q_shared, scale, extras));
    switch (r.kind) {
        case ATTN_ROUTE_NONE:  return VR_ATTN_ROUTE_NONE;
        case ATTN_ROUTE_SMALL: return VR_ATTN_ROUTE_SMALL;
        case ATTN_ROUTE_72W:   return VR_ATTN_ROUTE_72W;
        case ATTN_ROUTE_TILED: return VR_ATTN_ROUTE_TILED(r.head_dim, r.qf, r.pipe);
        default:               return VR_ATTN_ROUTE_REFUSED;
    }
}

extern "C" int vr_op_attention(int device_id, const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v,
                               int32_t ldv, void* out, int32_t ldo, const int32_t* cu_q, const int32_t* cu_kv, int32_t B,
                               int32_t heads, int32_t head_dim, int32_t max_q, int32_t causal, int32_t q_shared,
                               float scale, void* stream) {
    return vr_op_attention_ex(device_id, q, ldq, k, ldk, v, ldv, out, ldo, cu_q, cu_kv, B, heads, head_dim, max_q, causal, q_shared,
                              scale, nullptr, stream);
}

// the merge of a decode step's KV ranges: on its own (gen_kernels.hip) or inside the o projection (gemm_skinny.hip, COMBINE)
extern "C" int vr_op_attn_combine(int device_id, const void* part, const float* lse, int32_t S, const int32_t* S_dev, int32_t heads,
                                  int32_t group, int32_t n_rows, void* out, int32_t ld_out, const void* W, int32_t ldw, int32_t M,
                                  int32_t N, int32_t K, int32_t ksplit, int32_t planes, int32_t ldo, int64_t split_stride, void* stream) {
    if (!part || !lse || !out) return fail(VR_ERR_INVALID, "NULL argument");
    if (heads < 1 || n_rows < 1 || n_rows > 16) return fail(VR_ERR_INVALID, "need heads >= 1 and 1..16 rows");
    if (!S_dev && (S < 1 || S > GEN_ATT_SPLITS)) return fail(VR_ERR_INVALID, "S must be 1..%d", GEN_ATT_SPLITS);
    VRCHK(set_dev(device_id));
    if (!W) {
        if (ld_out < heads * 128 && n_rows > 1) return fail(VR_ERR_INVALID, "ld_out must cover heads * 128");
        HIPCHK(launch_attn_combine(part, lse, S, heads, group, out, (hipStream_t)stream, S_dev, n_rows, ld_out));
        return VR_OK;
    }
    // (what keeps the launch inside the caller's buffers is checked here; what the kernel can do is the launcher's to refuse)
    if (n_rows != 1) return fail(VR_ERR_INVALID, "the fused form merges one row");
    if (N < 1 || N % 4 || K < 64 || K % 64 || ldw < K || ldw % 8) return fail(VR_ERR_INVALID, "need N %% 4 == 0, K %% 64 == 0, ldw >= K, ldw %% 8 == 0");
    if (ksplit < 1 || ksplit > planes) return fail(VR_ERR_INVALID, "ksplit must be 1..planes");
    if (ldo < N || ldo % 4 || (ksplit > 1 && (split_stride < (int64_t)(M > 0 ? M : 1) * ldo || split_stride % 4)))
        return fail(VR_ERR_INVALID, "ldo must cover N, split_stride a plane of M x ldo; both multiples of 4");
    if (((uintptr_t)W | (uintptr_t)out) & 15) return fail(VR_ERR_INVALID, "pointers must be 16-byte aligned");
    GemmArgs a{};
    a.A = nullptr; a.lda = K; a.W = W; a.ldw = ldw; a.M = M; a.N = N; a.K = K; a.out = out; a.ldo = ldo;
    a.ksplit = ksplit; a.split_stride = (size_t)split_stride;
    const SkinnyCombine cb{part, lse, S, heads, group, S_dev};
    HIPCHK(launch_gemm_skinny(a, (hipStream_t)stream, false, &cb));
    return VR_OK;
}

// ---- the decode step's kernels (gemm_skinny.hip, norm.hip, chat_kernels.hip) ---
extern "C" int vr_op_gemm_skinny(int device_id, const void* A, int32_t lda, const void* W, int32_t ldw, int32_t M, int32_t N,
                                 int32_t K, int32_t ksplit, const float* bias, int32_t swiglu, void* out, int32_t ldo,
                                 int64_t split_stride, void* stream) {
    if (!A || !W || !out) return fail(VR_ERR_INVALID, "NULL argument");
    if (M < 1 || N < 1 || K < 64 || K % 64 || N % 4) return fail(VR_ERR_INVALID, "need M >= 1, N %% 4 == 0, K %% 64 == 0");
    if (M > 32 || (swiglu && M > 16)) return fail(VR_ERR_CAPACITY, "%d rows: at most 32 (16 with swiglu)", M);
    if (ksplit < 1 || ksplit > 64) return fail(VR_ERR_INVALID, "ksplit must be 1..64");
    if (lda < K || ldw < K || lda % 8 || ldw % 8) return fail(VR_ERR_INVALID, "lda / ldw must cover K and be multiples of 8");
    if (((uintptr_t)A | (uintptr_t)W | (uintptr_t)out | (uintptr_t)bias) & 15) return fail(VR_ERR_INVALID, "pointers must be 16-byte aligned");
    if (swiglu) {
        if (ksplit != 1 || N % 32) return fail(VR_ERR_INVALID, "swiglu needs ksplit 1 and N %% 32 == 0");
        if (ldo < N / 2 || ldo % 8) return fail(VR_ERR_INVALID, "swiglu: ldo must cover N / 2 and be a multiple of 8");
    } else {
        if (ldo < N || ldo % 4) return fail(VR_ERR_INVALID, "ldo must cover N and be a multiple of 4");
        if (ksplit > 1 && (split_stride < (int64_t)M * ldo || split_stride % 4)) return fail(VR_ERR_INVALID, "split_stride must cover a plane of M x ldo and be a multiple of 4");
    }
    VRCHK(set_dev(device_id));
    GemmArgs a{};
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.M = M; a.N = N; a.K = K; a.bias = bias; a.out = out; a.ldo = ldo;
    a.ksplit = ksplit; a.split_stride = (size_t)split_stride;
    HIPCHK(launch_gemm_skinny(a, (hipStream_t)stream, swiglu != 0));
    return VR_OK;
}

extern "C" int vr_op_plane_sum(int device_id, int32_t kind, const float* parts, int32_t nsplit, int64_t split_stride, int32_t ldp,
                               int32_t rows, int32_t dim, float* x, int32_t ldx, float alpha, const float* weight, float eps,
                               void* out, int32_t ldo, void* stream) {
    if (!parts) return fail(VR_ERR_INVALID, "NULL argument");
    if (kind != 0 && kind != 1) return fail(VR_ERR_INVALID, "kind %d: 0 (residual + RMSNorm), 1 (SwiGLU)", kind);
    if (rows < 1 || dim < 1 || nsplit < 1 || nsplit > 64) return fail(VR_ERR_INVALID, "need rows, dim >= 1 and nsplit 1..64");
    if (split_stride % 4 || (nsplit > 1 && split_stride < (int64_t)rows * ldp)) return fail(VR_ERR_INVALID, "split_stride must cover a plane of rows x ldp and be a multiple of 4");
    VRCHK(set_dev(device_id));
    if (kind == 0) {
        if (!x || (out && !weight)) return fail(VR_ERR_INVALID, "NULL argument");
        if (dim > 3584 || (out && ldo > 3584)) return fail(VR_ERR_CAPACITY, "rows of at most 3584 columns");
        if (dim % 4 || ldx % 4 || ldp % 4 || ldx < dim || ldp < dim || (out && (ldo % 4 || ldo < dim)))
            return fail(VR_ERR_INVALID, "dim, ldx, ldp, ldo must be multiples of 4 and the strides cover dim");
        if (((uintptr_t)parts | (uintptr_t)x | (uintptr_t)weight) & 15 || (uintptr_t)out & 7) return fail(VR_ERR_INVALID, "misaligned pointer");
        HIPCHK(launch_rmsnorm_accum(x, rows, dim, ldx, parts, nsplit, (size_t)split_stride, ldp, alpha, weight, eps, out, ldo, (hipStream_t)stream));
    } else {
        if (!out) return fail(VR_ERR_INVALID, "NULL argument");
        if (dim % 16 || ldp < 2 * dim || ldo < dim) return fail(VR_ERR_INVALID, "swiglu: dim %% 16 == 0, ldp >= 2 dim, ldo >= dim");
        HIPCHK(launch_swiglu_sum(parts, nsplit, (size_t)split_stride, ldp, rows, dim, out, ldo, (hipStream_t)stream));
    }
    return VR_OK;
}

// grow-only scratch of the two entries below, per device (the sampler test calls vr_op_chat_select thousands of times)
static std::map<int, DevBuf> g_chat_op_scratch;

extern "C" int vr_op_chat_attention(int device_id, const void* q, const void* prompt, const void* tails, int32_t layers, int32_t l,
                                    int32_t E, int32_t slots, int32_t max_len, int32_t rows, int32_t max_new, int32_t n,
                                    const int32_t* step_row, const int32_t* step_slot, const int32_t* step_tail,
                                    const int32_t* slot_plen, int32_t force_splits, void* att, void* stream) {
    if (!q || !prompt || !tails || !step_row || !step_slot || !step_tail || !slot_plen || !att) return fail(VR_ERR_INVALID, "NULL argument");
    if (E < 64 || E % 64) return fail(VR_ERR_INVALID, "E must be a multiple of the head dim 64");
    if (layers < 1 || l < 0 || l >= layers) return fail(VR_ERR_INVALID, "layer %d of %d", l, layers);
    if (slots < 1 || max_len < 1 || rows < 1 || max_new < 1) return fail(VR_ERR_INVALID, "bad cache geometry");
    if (force_splits < 0 || force_splits > CHAT_ATT_SPLITS) return fail(VR_ERR_INVALID, "force_splits must be 0..%d", CHAT_ATT_SPLITS);
    if (n < 1) return fail(VR_ERR_INVALID, "n must be positive");
    if (n > CHAT_MAX_ROWS) return fail(VR_ERR_CAPACITY, "%d rows exceed %d", n, CHAT_MAX_ROWS);
    if (((uintptr_t)q | (uintptr_t)prompt | (uintptr_t)tails | (uintptr_t)att) & 15) return fail(VR_ERR_INVALID, "pointers must be 16-byte aligned");
    ChatStep st{};
    st.n = n;
    std::vector<char> used(rows, 0);
    for (int i = 0; i < n; ++i) {
        const int r = step_row[i], sl = step_slot[i], t = step_tail[i];
        if (sl < 0 || sl >= slots || slot_plen[sl] < 1) return fail(VR_ERR_INVALID, "step row %d: slot %d holds no prompt", i, sl);
        if (slot_plen[sl] > max_len) return fail(VR_ERR_CAPACITY, "slot %d: %d prompt keys exceed max_len=%d", sl, slot_plen[sl], max_len);
        if (r < 0 || r >= rows || used[r]) return fail(VR_ERR_INVALID, "step row %d: row %d out of range or repeated", i, r);
        if (t < 0) return fail(VR_ERR_INVALID, "step row %d: negative tail index", i);
        if (t >= max_new) return fail(VR_ERR_CAPACITY, "step row %d: tail index %d exceeds max_new=%d", i, t, max_new);
        used[r] = 1;
        st.row[i] = r; st.slot[i] = sl; st.tail[i] = t; st.pos[i] = slot_plen[sl] + t;
    }
    const int S = chat_step_groups(st, slot_plen, slots, force_splits);
    if (!S) return fail(VR_ERR_INVALID, "the rows of a slot must be adjacent");
    VRCHK(set_dev(device_id));
    hipStream_t s = (hipStream_t)stream;
    const int H = E / 64;
    const size_t po = (size_t)CHAT_MAX_ROWS * H * CHAT_ATT_SPLITS * 64 * 4, pml = (size_t)CHAT_MAX_ROWS * H * CHAT_ATT_SPLITS * 2 * 4;
    DevBuf& sc = g_chat_op_scratch[device_id];
    if (sc.bytes < po + pml) { HIPCHK(hipStreamSynchronize(s)); VRCHK(sc.reserve(po + pml)); }
    const ChatCaps caps{slots, max_len, rows, max_new};
    HIPCHK(launch_chat_attn(st, q, prompt, tails, l, E, H, caps, S, sc.as<float>(), (float*)((char*)sc.p + po), att, s));
    HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_op_chat_extend_attention(int device_id, const void* q, int32_t ldq, const void* prompt, const void* tails, int32_t layers,
                                           int32_t l, int32_t E, int32_t heads, int32_t slots, int32_t max_len, int32_t rows,
                                           int32_t max_new, int32_t B, const int32_t* seq_row, const int32_t* seq_slot,
                                           const int32_t* seq_plen, const int32_t* seq_t0, const int32_t* seq_off, void* out,
                                           int32_t ldo, void* stream) {
    if (!q || !prompt || !tails || !seq_row || !seq_slot || !seq_plen || !seq_t0 || !seq_off || !out) return fail(VR_ERR_INVALID, "NULL argument");
    if (E < 64 || E % 8 || heads < 1 || heads * 64 > E) return fail(VR_ERR_INVALID, "need E %% 8 == 0 and 1 <= heads <= E / 64");
    if (layers < 1 || l < 0 || l >= layers) return fail(VR_ERR_INVALID, "layer %d of %d", l, layers);
    if (slots < 1 || max_len < 1 || rows < 1 || max_new < 1) return fail(VR_ERR_INVALID, "bad cache geometry");
    if (ldq % 8 || ldq < heads * 64 || ldo % 4 || ldo < heads * 64) return fail(VR_ERR_INVALID, "ldq (multiple of 8) / ldo (of 4) must cover heads * 64");
    if (B < 1) return fail(VR_ERR_INVALID, "B must be positive");
    if (B > CHAT_MAX_ROWS) return fail(VR_ERR_CAPACITY, "%d sequences exceed %d", B, CHAT_MAX_ROWS);
    if (((uintptr_t)q | (uintptr_t)prompt | (uintptr_t)tails | (uintptr_t)out) & 15) return fail(VR_ERR_INVALID, "pointers must be 16-byte aligned");
    if (seq_off[0] != 0) return fail(VR_ERR_INVALID, "seq_off[0] must be 0");
    ChatExtend ex{};
    ex.n = B;
    std::vector<char> used(rows, 0);
    for (int b = 0; b < B; ++b) {
        const int r = seq_row[b], sl = seq_slot[b], pl = seq_plen[b], t0 = seq_t0[b], n = seq_off[b + 1] - seq_off[b];
        if (sl < 0 || sl >= slots || pl < 1) return fail(VR_ERR_INVALID, "sequence %d: slot %d out of range or without a prompt key", b, sl);
        if (pl > max_len) return fail(VR_ERR_CAPACITY, "sequence %d: %d prompt keys exceed max_len=%d", b, pl, max_len);
        if (r < 0 || r >= rows || used[r]) return fail(VR_ERR_INVALID, "sequence %d: row %d out of range or repeated", b, r);
        if (t0 < 0 || n < 1) return fail(VR_ERR_INVALID, "sequence %d: negative tail index or no query row", b);
        if ((int64_t)t0 + n > max_new) return fail(VR_ERR_CAPACITY, "sequence %d: tail of %lld rows exceeds max_new=%d", b, (long long)t0 + n, max_new);
        used[r] = 1;
        ex.row[b] = r; ex.slot[b] = sl; ex.plen[b] = pl; ex.t0[b] = t0; ex.off[b] = seq_off[b];
    }
    ex.off[B] = seq_off[B];
    VRCHK(set_dev(device_id));
    hipStream_t s = (hipStream_t)stream;
    const ChatCaps caps{slots, max_len, rows, max_new};
    HIPCHK(launch_chat_extend_attn(ex, q, ldq, prompt, tails, l, E, heads, caps, out, ldo, s));
    HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_op_chat_select(int device_id, int32_t mode, const float* logits, int32_t ld, int32_t V, const uint32_t* seen,
                                 int32_t words, int32_t n_groups, const int32_t* group_offsets, const float* beam_scores, int32_t K,
                                 int32_t kout, float repetition_penalty, float temperature, uint64_t seed, int32_t step,
                                 float* out_scores, int32_t* out_tokens, int32_t* out_parents, void* stream) {
    if (!logits || !seen || !group_offsets || !out_scores || !out_tokens || !out_parents) return fail(VR_ERR_INVALID, "NULL argument");
    if (mode < VR_CHAT_GREEDY || mode > VR_CHAT_SAMPLE) return fail(VR_ERR_INVALID, "mode %d", mode);
    if (V < 1 || ld < V || words < (V + 31) / 32) return fail(VR_ERR_INVALID, "need V >= 1, ld >= V, words >= ceil(V / 32)");
    if (n_groups < 1 || n_groups > CHAT_MAX_ROWS || group_offsets[0] != 0) return fail(VR_ERR_INVALID, "bad groups");
    const int n = group_offsets[n_groups];
    if (n > CHAT_MAX_ROWS) return fail(VR_ERR_CAPACITY, "%d rows exceed %d", n, CHAT_MAX_ROWS);
    if (K < 1 || kout < 1) return fail(VR_ERR_INVALID, "K / kout must be positive");
    if (K > CHAT_TOPK_MAX || kout > CHAT_TOPK_MAX) return fail(VR_ERR_CAPACITY, "K / kout exceed %d", CHAT_TOPK_MAX);
    if (!(repetition_penalty > 0.f)) return fail(VR_ERR_INVALID, "repetition_penalty must be positive");
    if (mode == VR_CHAT_SAMPLE && !(temperature > 0.f)) return fail(VR_ERR_INVALID, "sampling: temperature must be positive");
    ChatSel sel{};
    sel.n = n; sel.groups = n_groups;
    for (int g = 0; g <= n_groups; ++g) sel.g_lo[g] = group_offsets[g];
    for (int g = 0; g < n_groups; ++g) {
        const int nb = group_offsets[g + 1] - group_offsets[g];
        if (nb < 1) return fail(VR_ERR_INVALID, "empty group %d", g);
        if (mode != VR_CHAT_BEAM && nb != 1) return fail(VR_ERR_INVALID, "greedy / sampling groups hold one row");
    }
    for (int i = 0; i < n; ++i) {
        sel.lrow[i] = i; sel.srow[i] = i;
        sel.bscore[i] = mode == VR_CHAT_BEAM && beam_scores ? beam_scores[i] : 0.f;
    }
    VRCHK(set_dev(device_id));
    hipStream_t s = (hipStream_t)stream;
    const size_t b_lse = CHAT_MAX_ROWS * 4, b_part = (size_t)CHAT_MAX_ROWS * CHAT_SEL_WGS * CHAT_TOPK_MAX * 8, b_out = (size_t)CHAT_MAX_ROWS * CHAT_TOPK_MAX * 4;
    DevBuf& sc = g_chat_op_scratch[device_id];
    if (sc.bytes < b_part + b_lse + 3 * b_out) { HIPCHK(hipStreamSynchronize(s)); VRCHK(sc.reserve(b_part + b_lse + 3 * b_out)); }
    unsigned long long* part = sc.as<unsigned long long>();
    float* lse = (float*)((char*)sc.p + b_part);
    float* o_score = (float*)((char*)lse + b_lse);
    int* o_tok = (int*)((char*)o_score + b_out);
    int* o_par = (int*)((char*)o_tok + b_out);
    const int cm = mode == VR_CHAT_BEAM ? CHAT_SEL_BEAM : mode == VR_CHAT_SAMPLE ? CHAT_SEL_SAMPLE : CHAT_SEL_GREEDY;
    HIPCHK(launch_chat_select(sel, cm, logits, ld, V, (const unsigned*)seen, words, repetition_penalty, temperature, K, kout,
                              (unsigned long long)seed, (unsigned)step, lse, part, o_score, o_tok, o_par, s));
    const size_t cnt = (size_t)n_groups * kout;
    HIPCHK(hipMemcpyAsync(out_scores, o_score, cnt * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_tokens, o_tok, cnt * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(out_parents, o_par, cnt * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_op_chat_sample(int device_id, const float* logits, int32_t ld, int32_t V, const uint32_t* seen, int32_t words, int32_t n,
                                 float repetition_penalty, float temperature, int32_t top_k, double top_p, uint64_t seed, int32_t step,
                                 float* out_scores, int32_t* out_tokens, int32_t* out_kept, int32_t* out_cut, void* stream) {
    if (!logits || !seen || !out_scores || !out_tokens || !out_kept || !out_cut) return fail(VR_ERR_INVALID, "NULL argument");
    if (V < 1 || ld < V || words < (V + 31) / 32) return fail(VR_ERR_INVALID, "need V >= 1, ld >= V, words >= ceil(V / 32)");
    if (n < 1) return fail(VR_ERR_INVALID, "n must be positive");
    if (n > CHAT_MAX_ROWS) return fail(VR_ERR_CAPACITY, "%d rows exceed %d", n, CHAT_MAX_ROWS);
    if (!(repetition_penalty > 0.f)) return fail(VR_ERR_INVALID, "repetition_penalty must be positive");
    if (!(temperature > 0.f)) return fail(VR_ERR_INVALID, "temperature must be positive");
    if (top_k < 0) return fail(VR_ERR_INVALID, "top_k must be 0 (off) or positive");
    if (!(top_p > 0.0 && top_p <= 1.0)) return fail(VR_ERR_INVALID, "top_p must be in (0, 1]");
    ChatSel sel{};
    sel.n = n; sel.groups = n;
    for (int i = 0; i < n; ++i) { sel.lrow[i] = i; sel.srow[i] = i; sel.g_lo[i] = i; }
    sel.g_lo[n] = n;
    VRCHK(set_dev(device_id));
    hipStream_t s = (hipStream_t)stream;
    const size_t b_out = (size_t)4 * CHAT_MAX_ROWS * 4;
    DevBuf& sc = g_chat_op_scratch[device_id];
    if (sc.bytes < b_out) { HIPCHK(hipStreamSynchronize(s)); VRCHK(sc.reserve(b_out)); }
    float* o_score = sc.as<float>();
    int* o_tok = (int*)(o_score + CHAT_MAX_ROWS);
    HIPCHK(launch_chat_sample(sel, logits, ld, V, (const unsigned*)seen, words, repetition_penalty, temperature, top_k, top_p,
                              (unsigned long long)seed, (unsigned)step, o_score, o_tok, o_tok + CHAT_MAX_ROWS, o_tok + 2 * CHAT_MAX_ROWS, s));
    int32_t host[4 * CHAT_MAX_ROWS];                          // one copy for the four runs
    HIPCHK(hipMemcpyAsync(host, o_score, sizeof(host), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    memcpy(out_scores, host, (size_t)n * 4);
    memcpy(out_tokens, host + CHAT_MAX_ROWS, (size_t)n * 4);
    memcpy(out_kept, host + 2 * CHAT_MAX_ROWS, (size_t)n * 4);
    memcpy(out_cut, host + 3 * CHAT_MAX_ROWS, (size_t)n * 4);
    return VR_OK;
}

extern "C" int vr_op_chat_prompt_scatter(int device_id, const void* qkv, int32_t ld, int32_t E, int32_t B, const int32_t* seq_offsets,
                                         const int32_t* slots, int32_t n_slots, int32_t max_len, void* kplane, void* vplane, void* stream) {
    if (!qkv || !seq_offsets || !slots || !kplane || !vplane) return fail(VR_ERR_INVALID, "NULL argument");
    if (E < 8 || E % 8 || ld % 8 || ld < 3 * E) return fail(VR_ERR_INVALID, "E and ld must be multiples of 8 and ld >= 3 E");
    if (n_slots < 1 || max_len < 1) return fail(VR_ERR_INVALID, "bad cache geometry");
    if (B < 1) return fail(VR_ERR_INVALID, "B must be positive");
    if (B > CHAT_MAX_ROWS || B > n_slots) return fail(VR_ERR_CAPACITY, "%d prompts exceed %d / the %d slots", B, CHAT_MAX_ROWS, n_slots);
    if (((uintptr_t)qkv | (uintptr_t)kplane | (uintptr_t)vplane) & 15) return fail(VR_ERR_INVALID, "pointers must be 16-byte aligned");
    if (seq_offsets[0] != 0) return fail(VR_ERR_INVALID, "seq_offsets[0] must be 0");
    ChatBatch bt{};
    bt.n = B;
    std::vector<char> used(n_slots, 0);
    for (int b = 0; b < B; ++b) {
        const int T = seq_offsets[b + 1] - seq_offsets[b], sl = slots[b];
        if (T < 1) return fail(VR_ERR_INVALID, "empty prompt %d", b);
        if (T > max_len) return fail(VR_ERR_CAPACITY, "prompt %d: %d rows exceed max_len=%d", b, T, max_len);
        if (sl < 0 || sl >= n_slots || used[sl]) return fail(VR_ERR_INVALID, "prompt %d: slot %d out of range or repeated", b, sl);
        used[sl] = 1;
        bt.off[b] = seq_offsets[b]; bt.idx[b] = sl;
    }
    bt.off[B] = seq_offsets[B];
    VRCHK(set_dev(device_id));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(launch_chat_prompt_scatter(bt, qkv, ld, E, max_len, kplane, vplane, s));
    HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// grow-only scratch per (device, stream) for the head's partials
static std::map<std::pair<int, void*>, DevBuf> g_head_score_scratch;

extern "C" int vr_op_head_score(int device_id, const void* A, int32_t lda, const void* W, int32_t ldw, int32_t M, int32_t V,
                                int32_t K, const int32_t* targets, float* out_logit, float* out_lse, float* out_top_logit,
                                int32_t* out_top_token, void* stream) {
    if (!A || !W || !targets || !out_logit || !out_lse || !out_top_logit || !out_top_token) return fail(VR_ERR_INVALID, "NULL argument");
    if (M < 1 || V < 1) return fail(VR_ERR_INVALID, "need M >= 1 and V >= 1");
    VRCHK(set_dev(device_id));
    hipStream_t s = (hipStream_t)stream;
    DevBuf& sc = g_head_score_scratch[std::make_pair(device_id, stream)];
    const size_t need = head_score_part_words(M, V) * 4;
    if (sc.bytes < need) { HIPCHK(hipStreamSynchronize(s)); VRCHK(sc.reserve(need)); }
    HIPCHK(launch_head_score(A, lda, W, ldw, M, V, K, targets, sc.p, out_logit, out_lse, out_top_logit, out_top_token, s));
    HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

// ---- the fp32 text path (hp_text.hip) and the encode glue kernels (misc.hip, patch_embed.hip, norm.hip) ---
// Thin forwards: only NULL pointers are checked here; what a kernel cannot do is the launcher's to refuse (VR_ERR_HIP).
extern "C" int vr_op_norm_ex(int device_id, int32_t kind, const float* x, int32_t rows, int32_t dim, int32_t ldx, const float* weight,
                             const float* bias, float eps, void* out, int32_t ldo, void* stream) {
    if (!x || !weight || !out || (kind == 0 && !bias)) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    if (kind == 0) HIPCHK(launch_layernorm(x, rows, dim, ldx, weight, bias, eps, out, ldo, (hipStream_t)stream));
    else HIPCHK(launch_rmsnorm(x, rows, dim, ldx, weight, eps, out, ldo, (hipStream_t)stream));
    return VR_OK;
}

extern "C" int vr_op_text_rmsnorm_split(int device_id, const float* x, int32_t rows, int32_t dim, const float* weight, float eps,
                                        void* hi, void* lo, void* stream) {
    if (!x || !weight || !hi || !lo) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    HIPCHK(launch_rmsnorm_split(x, rows, dim, weight, eps, hi, lo, (hipStream_t)stream));
    return VR_OK;
}

extern "C" int vr_op_text_rope(int device_id, float* qkv, int32_t T, int32_t ld, int32_t rope_cols, const int32_t* pos,
                               const float* table, void* stream) {
    if (!qkv || !pos || !table) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    HIPCHK(launch_rope_f32(qkv, T, ld, rope_cols, pos, table, (hipStream_t)stream));
    return VR_OK;
}

extern "C" int vr_op_text_attention(int device_id, const float* qkv, int32_t ld, int32_t E, const int32_t* seq_offsets, int32_t B,
                                    int32_t T, int32_t heads, float scale, float* out, void* stream) {
    if (!qkv || !seq_offsets || !out) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    hipStream_t s = (hipStream_t)stream;
    DevBuf seq_of;                                          // (freed on return: the stream is drained first)
    VRCHK(seq_of.alloc((size_t)(T > 0 ? T : 1) * 4));
    HIPCHK(launch_seq_of(seq_offsets, B, seq_of.as<int>(), s));
    HIPCHK(launch_attn_f32(qkv, ld, E, seq_of.as<int>(), seq_offsets, T, heads, scale, out, s));
    HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_op_text_swiglu_split(int device_id, const float* gu, int32_t T, int32_t ld_gu, int32_t I, int32_t ld_act, void* hi,
                                       void* lo, void* stream) {
    if (!gu || !hi || !lo) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    HIPCHK(launch_swiglu_split(gu, T, ld_gu, I, ld_act, hi, lo, (hipStream_t)stream));
    return VR_OK;
}

extern "C" int vr_op_embed_gather(int device_id, const int32_t* ids, int32_t T, const void* table, const void* table_lo, int32_t dim,
                                  float scale, float* out, void* stream) {
    if (!ids || !table || !out) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    if (!table_lo) HIPCHK(launch_embed_gather(ids, T, table, dim, scale, out, (hipStream_t)stream));
    else HIPCHK(launch_embed_gather_hp(ids, T, table, table_lo, dim, scale, out, (hipStream_t)stream));
    return VR_OK;
}

extern "C" int vr_op_pool(int device_id, const float* h, const int32_t* seq_offsets, int32_t B, int32_t dim, const float* norm_w,
                          float eps, float* out, float* tap, int32_t mode, void* stream) {
    if (!h || !seq_offsets || !norm_w || !out) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    HIPCHK(launch_pool(h, seq_offsets, B, dim, norm_w, eps, out, tap, (hipStream_t)stream, mode));
    return VR_OK;
}

extern "C" int vr_op_convert(int device_id, int32_t kind, const void* in, void* out, void* out2, int64_t n, int64_t n_total,
                             int32_t* aux, void* stream) {
    if (kind < 0 || kind > 5) return fail(VR_ERR_INVALID, "kind %d: 0 f32->bf16, 1 f32->bf16 + zero pad, 2 hi/lo split, 3 any non-zero, 4 positions, 5 sequence of a token", kind);
    if (!in || (kind != 3 && !out) || (kind == 2 && !out2) || (kind == 3 && !aux)) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    hipStream_t s = (hipStream_t)stream;
    switch (kind) {
        case 0: HIPCHK(launch_f32_to_bf16((const float*)in, out, (size_t)n, s)); break;
        case 1: HIPCHK(launch_f32_to_bf16_pad((const float*)in, out, (size_t)n, (size_t)n_total, s, aux)); break;
        case 2: HIPCHK(launch_split_bf16((const float*)in, out, out2, (size_t)n, s)); break;
        case 3: HIPCHK(launch_any_nonzero16(in, (size_t)n, aux, s)); break;
        case 4: HIPCHK(launch_iota_pos((const int*)in, (int)n, (int*)out, s)); break;
        default: HIPCHK(launch_seq_of((const int*)in, (int)n, (int*)out, s)); break;
    }
    return VR_OK;
}

extern "C" int vr_op_planes_sum(int device_id, const float* parts, int32_t n_parts, int64_t stride, int32_t ldp, int32_t T, int32_t N,
                                float* out, int32_t ldo, float alpha, int32_t accumulate, void* stream) {
    if (!parts || !out) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    HIPCHK(launch_planes_sum(parts, n_parts, (size_t)stride, ldp, T, N, out, ldo, alpha, accumulate != 0, (hipStream_t)stream));
    return VR_OK;
}

extern "C" int vr_op_patch_embed(int device_id, const void* const* imgs, int32_t n, int32_t H, int32_t W, int32_t P, const float* weight,
                                 int32_t D, int32_t K, const float* bias, const float* pos, int32_t ld_pos, float* out, int32_t ldo,
                                 void* stream) {
    if (!imgs || !weight || !bias || !pos || !out) return fail(VR_ERR_INVALID, "NULL argument");
    for (int i = 0; i < n; ++i)
        if (!imgs[i]) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    hipStream_t s = (hipStream_t)stream;
    const int Kreal = 3 * P * P, patches = P > 0 ? (H / P) * (W / P) : 0;
    // the packed weight as vr_model_load_weight keeps it: bf16 [D padded to 256 rows][K], zero where nothing is packed (the
    // row pitch of the ALLOCATION also covers Kreal, so that the pack of a K the launcher will refuse stays inside it)
    DevBuf wp, ptrs;
    VRCHK(wp.alloc((size_t)pad256(D > 0 ? D : 1) * (size_t)std::max(std::max(K, Kreal), 1) * 2));
    VRCHK(ptrs.alloc((size_t)(n > 0 ? n : 1) * sizeof(void*)));
    HIPCHK(launch_pack_patch_weight(weight, 0, D, P, wp.p, K, s));
    if (n > 0) HIPCHK(hipMemcpyAsync(ptrs.p, imgs, (size_t)n * sizeof(void*), hipMemcpyHostToDevice, s));
    GemmArgs a{};
    a.W = wp.p; a.ldw = K; a.M = n * patches; a.N = D; a.K = K; a.bias = bias; a.out = out; a.ldo = ldo; a.alpha = 1.0f;
    a.rowbias = pos; a.rowbias_period = patches; a.rowbias_ld = ld_pos; a.rowbias_cols = D;
    const hipError_t e = launch_patch_embed((const uint8_t* const*)ptrs.p, n, H, W, P, a, Kreal, s);
    HIPCHK(hipStreamSynchronize(s));                        // (the temporaries are freed on return)
    if (e != hipSuccess) return fail(VR_ERR_HIP, "launch_patch_embed(...) failed: %s", hipGetErrorString(e));
    return VR_OK;
}

// ---- the EVisRAG generator's small kernels (gen_kernels.hip) ---
// Thin forwards like the block above: NULL pointers and counts are checked here, what a kernel cannot do is the launcher's to
// refuse (VR_ERR_HIP).  Entries that own a temporary drain the stream before they return.
extern "C" int vr_op_gen_mrope_cache(int device_id, const void* src_bf16, const float* parts, int32_t n_parts, int64_t plane_stride,
                                     const float* bias, int32_t ld, int32_t T, int32_t H, int32_t KV, const int32_t* pos3,
                                     int32_t pos_stride, int32_t sec_t, int32_t sec_h, const float* inv_freq, void* q_out, int32_t ldq,
                                     void* k_cache, void* v_cache, int32_t ld_cache, int32_t cache_row0, const int32_t* row0_dev,
                                     const int32_t* cache_rows, int32_t* cu_kv, void* stream) {
    if ((!src_bf16 && !parts) || !pos3 || !inv_freq || !q_out || !k_cache || !v_cache) return fail(VR_ERR_INVALID, "NULL argument");
    if (T < 1 || H < 1 || KV < 1 || (parts && n_parts < 1)) return fail(VR_ERR_INVALID, "need T, H, KV >= 1 (and n_parts >= 1 with planes)");
    VRCHK(set_dev(device_id));
    HIPCHK(launch_mrope_cache(parts ? nullptr : src_bf16, parts, n_parts, (size_t)plane_stride, bias, ld, T, H, KV, pos3, pos_stride,
                              sec_t, sec_h, inv_freq, q_out, ldq, k_cache, v_cache, ld_cache, cache_row0, cu_kv, (hipStream_t)stream,
                              row0_dev, cache_rows));
    return VR_OK;
}

extern "C" int vr_op_gen_rope2d(int device_id, void* qkv, int32_t ld, int32_t T, int32_t n_slots, int32_t hh, const int32_t* pos_h,
                                const int32_t* pos_w, int32_t sec_h, const float* freq, void* stream) {
    if (!qkv || !pos_h || !pos_w || !freq) return fail(VR_ERR_INVALID, "NULL argument");
    if (T < 1 || n_slots < 1) return fail(VR_ERR_INVALID, "need T, n_slots >= 1");
    VRCHK(set_dev(device_id));
    hipStream_t s = (hipStream_t)stream;
    DevBuf cs;                                              // f32 [T][64][2] (freed on return: the stream is drained first)
    VRCHK(cs.alloc((size_t)T * 64 * 8));
    hipError_t e = launch_rope2d_table(pos_h, pos_w, T, sec_h, freq, cs.p, s);
    if (e == hipSuccess) e = launch_rope2d_inplace(qkv, ld, T, n_slots, hh, cs.p, s);
    HIPCHK(hipStreamSynchronize(s));
    if (e != hipSuccess) return fail(VR_ERR_HIP, "launch_rope2d_table / launch_rope2d_inplace(...) failed: %s", hipGetErrorString(e));
    return VR_OK;
}

// the words of `state` (include/visrag_hip.h) are GenState's
static_assert(sizeof(GenState) == 42 * 4 && GEN_ATT_SPLITS == 16, "vr_op_gen_sample / vr_op_gen_decode_begin document 42 words");
static std::map<int, DevBuf> g_gen_op_scratch;              // 64 partial keys + the token, per device

extern "C" int vr_op_gen_sample(int device_id, const float* logits, int32_t vocab, uint32_t* seen, float repetition_penalty,
                                float temperature, uint64_t seed, int32_t step, int32_t* state, int32_t step_from_state,
                                int32_t advance, int32_t* out_token, void* stream) {
    if (!logits || !seen || !out_token || ((step_from_state || advance) && !state)) return fail(VR_ERR_INVALID, "NULL argument");
    if (vocab < 1) return fail(VR_ERR_INVALID, "vocab must be positive");
    VRCHK(set_dev(device_id));
    hipStream_t s = (hipStream_t)stream;
    DevBuf& sc = g_gen_op_scratch[device_id];
    if (sc.bytes < 64 * 8 + 16) { HIPCHK(hipStreamSynchronize(s)); VRCHK(sc.reserve(64 * 8 + 16)); }
    int* tok = (int*)((char*)sc.p + 64 * 8);
    HIPCHK(launch_sample(logits, vocab, (unsigned*)seen, repetition_penalty, temperature, (unsigned long long)seed, (unsigned)step, tok,
                         sc.as<unsigned long long>(), s, (GenState*)state, step_from_state, advance));
    HIPCHK(hipMemcpyAsync(out_token, tok, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return VR_OK;
}

extern "C" int vr_op_gen_mark_seen(int device_id, const int32_t* ids, int32_t n, uint32_t* seen, int32_t vocab, void* stream) {
    if (!ids || !seen) return fail(VR_ERR_INVALID, "NULL argument");
    if (n < 1 || vocab < 1) return fail(VR_ERR_INVALID, "need n, vocab >= 1");
    VRCHK(set_dev(device_id));
    HIPCHK(launch_mark_seen(ids, n, (unsigned*)seen, vocab, (hipStream_t)stream));
    return VR_OK;
}

extern "C" int vr_op_gen_decode_begin(int device_id, int32_t* state, int32_t q_rows, void* stream) {
    if (!state) return fail(VR_ERR_INVALID, "NULL argument");
    if (q_rows < 1) return fail(VR_ERR_INVALID, "q_rows must be positive");
    VRCHK(set_dev(device_id));
    HIPCHK(launch_decode_begin((GenState*)state, q_rows, (hipStream_t)stream));
    return VR_OK;
}

extern "C" int vr_op_gen_rows(int device_id, int32_t kind, const float* src, const int32_t* row_idx, int32_t n, int32_t dim, void* dst,
                              int32_t ld, const void* const* pages, const int32_t* page_w, int32_t n_pages, const int32_t* img,
                              const int32_t* ph, const int32_t* pw, int32_t P, int32_t tp, const float* mean3, const float* std3,
                              void* stream) {
    if (kind < 0 || kind > 2) return fail(VR_ERR_INVALID, "kind %d: 0 scatter f32 rows, 1 gather to bf16 + zero pad, 2 u8 patch rows", kind);
    if (!dst || n < 1) return fail(VR_ERR_INVALID, "NULL argument or n < 1");
    hipStream_t s = (hipStream_t)stream;
    if (kind < 2) {
        if (!src || !row_idx) return fail(VR_ERR_INVALID, "NULL argument");
        if (dim < 1) return fail(VR_ERR_INVALID, "dim must be positive");
        VRCHK(set_dev(device_id));
        if (kind == 0) HIPCHK(launch_scatter_rows(src, row_idx, n, dim, (float*)dst, ld, s));
        else HIPCHK(launch_gather_rows_bf16(src, row_idx, n, dim, dst, ld, s));
        return VR_OK;
    }
    if (!pages || !page_w || !img || !ph || !pw || !mean3 || !std3) return fail(VR_ERR_INVALID, "NULL argument");
    if (n_pages < 1 || P < 1 || tp < 1) return fail(VR_ERR_INVALID, "need n_pages, P, tp >= 1");
    for (int i = 0; i < n_pages; ++i)
        if (!pages[i]) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    DevBuf tab;                                             // the page pointers, then their widths (freed on return: the stream is drained first)
    VRCHK(tab.alloc((size_t)n_pages * 12));
    HIPCHK(hipMemcpyAsync(tab.p, pages, (size_t)n_pages * 8, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync((char*)tab.p + (size_t)n_pages * 8, page_w, (size_t)n_pages * 4, hipMemcpyHostToDevice, s));
    const hipError_t e = launch_patch_rows_u8((const uint8_t* const*)tab.p, (const int*)((const char*)tab.p + (size_t)n_pages * 8), img, ph, pw,
                                              n, P, tp, mean3, std3, dst, ld, s);
    HIPCHK(hipStreamSynchronize(s));
    if (e != hipSuccess) return fail(VR_ERR_HIP, "launch_patch_rows_u8(...) failed: %s", hipGetErrorString(e));
    return VR_OK;
}
