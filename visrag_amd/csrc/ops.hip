// Stand-alone entry points of libvisrag_hip.so: page resize, synthetic pages, the stream-overlap probe and the op-level
// calls (vr_op_*) the kernel tests drive.
#include <hip/hip_runtime.h>

#include <chrono>
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
extern "C" int vr_op_gemm(int device_id, const void* A, int32_t lda, const void* W, int32_t ldw, int32_t M, int32_t N,
                          int32_t K, int32_t epilogue, const float* bias, const float* resid, float alpha, void* out,
                          int32_t ldo, const int32_t* rope_pos, const float* rope_table, int32_t rope_cols,
                          int32_t variant, void* stream) {
    if (!A || !W || !out) return fail(VR_ERR_INVALID, "NULL argument");
    if (variant != GEMM_VARIANT_GLDS && variant != GEMM_VARIANT_AUTO && variant != GEMM_VARIANT_192 && variant != GEMM_VARIANT_256IL && variant != GEMM_VARIANT_256W && variant != GEMM_VARIANT_192W &&
        variant != GEMM_VARIANT_128W_192 && variant != GEMM_VARIANT_128W_256)
        return fail(VR_ERR_INVALID, "variant %d: 0 (128^2 tile), 3 (auto), 7 (256x192 tile), 9 (256^2 tile), 12 / 13 (256^2 / 256x192 tile, one wave per SIMD), 14 / 15 (128x192 / 128x256 tile, one wave per SIMD)", variant);
    if (((variant == 7 || variant == 13 || variant == 14) ? N % 192 : N % 128) || K % 64 || M <= 0) return fail(VR_ERR_INVALID, "need N %% 128 == 0 (192 for variant 7), K %% 64 == 0");
    if (epilogue == EPI_RESID && !resid) return fail(VR_ERR_INVALID, "EPI_RESID needs resid");
    if (epilogue == EPI_ROPE && (!rope_pos || !rope_table)) return fail(VR_ERR_INVALID, "EPI_ROPE needs tables");
    VRCHK(set_dev(device_id));
    GemmArgs a{};
    a.A = A; a.lda = lda; a.W = W; a.ldw = ldw; a.M = M; a.N = N; a.K = K; a.bias = bias; a.resid = resid;
    a.alpha = alpha; a.out = out; a.ldo = ldo; a.rope_pos = rope_pos; a.rope_table = rope_table; a.rope_cols = rope_cols;
    HIPCHK(launch_gemm(a, epilogue, variant, (hipStream_t)stream));
    return VR_OK;
}

extern "C" int vr_op_norm(int device_id, int32_t kind, const float* x, int32_t rows, int32_t dim, const float* weight,
                          const float* bias, float eps, void* out, int32_t ldo, void* stream) {
    if (!x || !weight || !out || (kind == 0 && !bias)) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    if (kind == 0) HIPCHK(launch_layernorm(x, rows, dim, dim, weight, bias, eps, out, ldo, (hipStream_t)stream));
    else HIPCHK(launch_rmsnorm(x, rows, dim, dim, weight, eps, out, ldo, (hipStream_t)stream));
    return VR_OK;
}

extern "C" int vr_op_attention(int device_id, const void* q, int32_t ldq, const void* k, int32_t ldk, const void* v,
                               int32_t ldv, void* out, int32_t ldo, const int32_t* cu_q, const int32_t* cu_kv, int32_t B,
                               int32_t heads, int32_t head_dim, int32_t max_q, int32_t causal, int32_t q_shared,
                               float scale, void* stream) {
    if (!q || !k || !v || !out || !cu_q || !cu_kv) return fail(VR_ERR_INVALID, "NULL argument");
    VRCHK(set_dev(device_id));
    AttnArgs a{};
    a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv; a.out = out; a.ldo = ldo; a.cu_q = cu_q;
    a.cu_kv = cu_kv; a.B = B; a.heads = heads; a.head_dim = head_dim; a.max_q = max_q; a.causal = causal;
    a.q_shared = q_shared; a.scale = scale;
    HIPCHK(launch_attention(a, (hipStream_t)stream));
    return VR_OK;
}
