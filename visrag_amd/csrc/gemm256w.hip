// 256 x 256 x 64 bf16 GEMM tile with ONE WAVE PER SIMD: 4 waves (2 x 2), 128 x 128 outputs per wave.
//
// Why: the 8-wave 256^2 kernel (gemm.hip) reads 12 fragments per 32 MFMAs and keeps two waves per
// SIMD in lockstep behind one barrier per K-step; PMC puts its main loop at ~67 % matrix-pipe use
// with the LDS ~75 % busy.  A 128 x 128 register tile reads 16 fragments per 64 MFMAs (a third less
// LDS traffic per flop) and leaves the SIMD to a single wave whose instruction stream is laid out
// by hand, so nothing has to be hidden by a second wave:
//
//   * the 256 fp32 accumulators of a lane live in the accumulation registers (a wave alone on its
//     SIMD owns all 512 registers), the 32 operand fragments of a whole K-step in VGPRs;
//   * software pipeline over K-steps (two LDS stages of A 32 KiB + W 32 KiB):
//       phase 1: 64 MFMAs on the k-half-0 fragments; under them the 16 fragment reads of k-half 1,
//                then `lgkmcnt(0) + barrier` (every wave has the whole stage in registers: the stage
//                is free) and the first LDS-DMA loads of K-step kt+2 INTO THE STAGE BEING COMPUTED;
//       phase 2: 64 MFMAs on the k-half-1 fragments; under them `vmcnt(5) + barrier` (K-step kt+1
//                has landed; the loads of kt+2 issued so far stay in flight), the rest of the loads
//                of kt+2 and the 16 k-half-0 fragment reads of K-step kt+1.
//     Loads run two K-steps ahead with two LDS stages because the registers hold the step being
//     computed; the MFMA stream never stops at a step boundary.
//   * the 16 LDS-DMA loads a wave issues per K-step are SPREAD, one per five MFMAs.  In-kernel clock
//     counts per K-step (2048 = the 128 MFMAs alone): MFMAs + barriers 2100, + fragment reads 2094,
//     + the 16 loads issued back to back 2777, + the same loads spread 2201.  The CU moves one 1 KiB
//     LDS-DMA instruction per ~16 clocks; four waves issuing theirs in one burst queue behind each
//     other and, being alone on their SIMDs, stall their MFMA streams while they wait.
//   * LDS-DMA through a buffer descriptor: per-lane offset in a VGPR (constant + K offset: two VALU
//     adds per K-step), row-group offsets in SGPRs, the two K-steps past the end of K are pointed
//     out of the descriptor's range (zeros written to the dead stage, no memory traffic), so every
//     K-step runs the same code and the `vmcnt(5)` count always holds.
//
//   * the epilogue stages through 16 KiB of LDS above the two stages, so it does not wait for the last
//     (out-of-range) loads to land.  A PERSISTENT form of this kernel (one workgroup per CU walking its
//     XCD's tile range, the load pipeline running on across tile boundaries: no prologue, no workgroup
//     launch between tiles) was built and measured in round 2 — tile period 28.7 instead of 30.1 us, but
//     the kernel no faster: with a static split the slowest workgroup sets the end (CUs differ by 8 %,
//     XCDs by 2.5 %), and per-XCD atomic cursors cost as much (index arithmetic and the LDS mailbox between
//     K-steps) as they balance: ViT qkv 227 vs 221 us, proj 109 vs 102.  The hardware dispatcher already
//     does that balancing for a one-tile-per-workgroup grid.  Round 5 tried the middle: PAIRS of tiles per workgroup for
//     whole rounds of the CUs, the rest one tile each — correct, qkv -1.7 %, but the step +1.6 % (the residual GEMMs' first
//     epilogue queues behind the second tile's HBM operand loads; and a prologue is a wait, not work: under the power cap the
//     clock takes such cycles back — DESIGN.md 5.2, ledger 50).  What did pay in round 5 was executing less in the epilogues
//     (buffer descriptors instead of predicates, branches and 64-bit address arithmetic: gemm256w_kernel.h, gemm_epilogue.h).
//
// NJ = 16-column fragments per wave: 8 -> 256 x 256 tile, 6 -> 256 x 192 tile (N = 1152 = 6 x 192: SigLIP proj / fc2,
// residual and fp32 epilogues), 9 -> 256 x 288 tile (1152 = 4 x 288: 512 tiles at 32 768 rows, two full rounds of the
// 256 CUs where 192 columns take three; the lookup-free residual epilogue only).  Slot s = strip * NJ + fragment numbers
// the MFMAs of a phase; the numbers in the schedule above are those of NJ = 8, the others are scaled (see the constants
// in the kernel: NJ = 9 has 72 slots, 17 loads, barriers at slots 45 and 9, five loads in phase 1, vmcnt(17) / vmcnt(5)).
// NJ = 9 per K-step and wave: 144 MFMAs on 17 LDS-DMA instructions and 34 fragment reads (0.35 auxiliaries per MFMA; NJ = 6:
// 0.44, NJ = 8: 0.375), (256 + 288) / (256 * 288) operand bytes per output (0.81 of NJ = 6's).  Its 288 accumulators do not
// fit the accumulation-register file: strip i's ninth fragment is eight "+v" operands (W_MFMA_V, gemm256w_acc.h) in arch
// VGPRs — 136 fragment registers + 32 + addressing = 204, no scratch.  The K-loop of that instantiation runs whole PAIRS of
// steps and the odd step behind them: with an exit between the two steps of the loop hipcc copied the 32 registers to
// another set in one step and back in the next (16 v_mov_b64 per step, each reading an MFMA result the hardware does not
// interlock); build.py walks the listing for such reads (mfma_operand_hazards).  A stage is A 32 KiB + W 36 KiB; two
// stages + staging + dump slots = 156 672 B of the 160 KiB a workgroup may declare.  Epilogue pieces of 32 rows x 48
// columns, twelve per wave, through the same descriptors, register ring and expression as NJ = 6: bit-identical outputs.
//
// LDS image, swizzle and epilogues are those of the 8-wave kernel (gemm_core.h, gemm_epilogue.h);
// the accumulators are kept as two 64-column halves so the epilogue helpers apply unchanged.
// Roofline: MFMA (2*M*N*K flops per launch).
#include <type_traits>

#include "gemm_core.h"
#include "gemm_epilogue.h"
#include "gemm256w_acc.h"

namespace vr {

bool gemm256w_fits(const GemmArgs& a, int bn);

namespace {

constexpr int W_STAGE = 2 * G256_TILE_BYTES;       // A tile + W tile = 64 KiB
// ... of a tile of 32 nj columns: the 288-column tile's W rows take 36 KiB, the 192-column tile keeps the 256-column stride
constexpr int w_stage_bytes(int nj) { return nj > 8 ? G256_TILE_BYTES + nj * 32 * GEMM_BK * 2 : W_STAGE; }
constexpr unsigned W_OOB = 0x80000000u;            // per-lane offset beyond the descriptor's range

}  // namespace

// PLAIN: the host has checked that the bf16-output epilogue needs no per-row lookups (no row map / row bias,
// N and ldo multiples of 8) — the kernel then carries only the lookup-free staged epilogue.
constexpr int W_STAGING = 4096;                            // epilogue staging per wave: one piece of 32 rows x 64 bf16
constexpr int W_WARM_DUMP = 256;                           // where a wave's GemmArgs::warm requests land: 64 lanes x 4 bytes nobody reads
constexpr int W_SMEM_BYTES = 2 * W_STAGE + 4 * W_STAGING + 4 * W_WARM_DUMP;  // two stages + staging + dump slots = 145 KiB
constexpr int w_smem_bytes(int nj) { return 2 * w_stage_bytes(nj) + 4 * W_STAGING + 4 * W_WARM_DUMP; }
static_assert(w_smem_bytes(8) == W_SMEM_BYTES && w_smem_bytes(6) == W_SMEM_BYTES && w_smem_bytes(9) == 156672 && w_smem_bytes(9) <= 160 * 1024, "LDS a workgroup may declare");

// GemmArgs::warm: walking the workgroups and their waves in order, each share starts where the one before ended (ordered, disjoint,
// no gap) and the last one ends with the region's last line — every line is requested exactly once, whatever the grid
constexpr bool warm_shares_tile(size_t bytes, unsigned total) {
    unsigned at = 0;
    for (unsigned w = 0; w < total; ++w)
        for (unsigned v = 0; v < WARM_WAVES; ++v) {
            const WarmShare s = warm_share(bytes, w, total, v);
            if (s.first != at || s.end < s.first) return false;
            at = s.end;
        }
    return at == warm_lines(bytes) && (size_t)at * WARM_LINE >= bytes && (bytes == 0 || (size_t)(at - 1) * WARM_LINE < bytes);
}
static_assert(warm_shares_tile(0, 1) && warm_shares_tile(0, 243), "no lines");
static_assert(warm_shares_tile(1, 1) && warm_shares_tile(WARM_LINE, 4) && warm_shares_tile(WARM_LINE + 1, 4), "1 and 2 lines");
static_assert(warm_shares_tile(63 * WARM_LINE, 1) && warm_shares_tile(64 * WARM_LINE, 1) && warm_shares_tile(65 * WARM_LINE, 1), "63 / 64 / 65 lines, one workgroup");
static_assert(warm_shares_tile(63 * WARM_LINE, 4) && warm_shares_tile(64 * WARM_LINE, 4) && warm_shares_tile(65 * WARM_LINE - 3, 4), "63 / 64 / 65 lines, four");
static_assert(warm_shares_tile(100 * WARM_LINE, 243) && warm_shares_tile(5 * WARM_LINE, 405), "a region of fewer lines than the grid has waves");
static_assert(warm_shares_tile((size_t)2304 * 2304 * 2, 243), "W_o (10.6 MB) over the decoder's q|k|v grid");
static_assert(warm_shares_tile((size_t)2304 * 5760 * 2, 405), "W_down (26.5 MB) over the decoder's gate|up grid");
static_assert(warm_shares_tile(WARM_MAX_BYTES - 1, 1021), "the largest region");
static_assert(warm_cut((1u << 24) - 1, 65534, 65535) == (unsigned)(((1ull << 24) - 1) * 65534 / 65535) && warm_cut(65534, 65534, 65535) == 65533 &&
              warm_cut((1u << 24) - 1, 65535, 65535) == (1u << 24) - 1, "the largest grid of the 32-bit form");
static_assert(warm_part(0, warm_lines(WARM_MAX_BYTES - 1), 65536, 65537).end == warm_lines(WARM_MAX_BYTES - 1) &&
              warm_cut(1u << 24, 70001, 70003) == (unsigned)((1ull << 24) * 70001 / 70003) && warm_cut(82944, 100, 243) == 82944ull * 100 / 243, "both forms of the cut");
#if VR_WARM_LINE == 128
static_assert(warm_instructions(warm_share((size_t)2304 * 2304 * 2, 0, 243, 0)) == 2 &&
              warm_instructions(warm_share((size_t)2304 * 5760 * 2, 404, 405, 3)) == 2, "two requests per wave in the decoder");
#endif

#define W_KERNEL_TEMPLATE template <int EPI, bool PLAIN, int NJ>
#define W_KERNEL_NAME gemm256w_bf16_kernel
#include "gemm256w_kernel.h"
#undef W_KERNEL_TEMPLATE
#undef W_KERNEL_NAME

template <int EPI, bool PLAIN, int NJ>
static hipError_t launch_wp(GemmArgs a, hipStream_t s) {
    constexpr int BN = 32 * NJ;
    const int tn = (a.N + BN - 1) / BN, tm = (a.M + G256_BM - 1) / G256_BM;
    // (four tile columns of 288: the 32 tiles an XCD runs together as 8 rows x 4 columns — the least operand rows, r * 256 + c * 288,
    // among the r x c = 32 blocks of whole tile columns)
    if (a.raster_gm <= 0) a.raster_gm = tm <= 16 ? tm : (NJ == 9 ? 8 : 4);
    if (!gemm256w_fits(a, BN)) return hipErrorInvalidValue;
    if (gemm_args_refused(a, EPI, NJ == 9 ? GEMM_VARIANT_288W : NJ == 6 ? GEMM_VARIANT_192W : GEMM_VARIANT_256W)) return hipErrorInvalidValue;
    int total = tn * tm;
    if (a.ksplit > 1) total *= a.ksplit;
    auto k = gemm256w_bf16_kernel<EPI, PLAIN, NJ>;
    static unsigned long long attr = 0;     // bit d: set on device d
    set_max_dynamic_lds((const void*)k, w_smem_bytes(NJ), attr);
    hipLaunchKernelGGL(k, dim3(total), dim3(256), w_smem_bytes(NJ), s, a);
    return hipGetLastError();
}

template <int EPI>
static hipError_t launch_w(const GemmArgs& a, hipStream_t s) {
    if constexpr (EPI == EPI_BF16 || EPI == EPI_GELU || EPI == EPI_SWIGLU || EPI == EPI_ROPE) {
        // (a row bias rides the lookup-free bf16 form when no tile can wrap around its period and it covers whole 64-column blocks:
        // the resampler's k | v in-projection, pos_k[row % 1024] on the k half)
        const bool rb_ok = !a.rowbias || (EPI == EPI_BF16 && a.rowbias_period > 0 && a.rowbias_period % G256_BM == 0 && a.rowbias_cols % 64 == 0 && a.rowbias_cols <= a.rowbias_ld &&
                                          (size_t)a.rowbias_period * a.rowbias_ld * 4 < (1ull << 32));
        if (!a.rowmap && rb_ok && (a.N & 7) == 0 && (a.ldo & 7) == 0) return launch_wp<EPI, true, 8>(a, s);
    }
    return launch_wp<EPI, false, 8>(a, s);
}

// the LDS-DMA addresses whole matrices through 32-bit offsets: both operands (rows padded to the tile) below 2 GiB
bool gemm256w_fits(const GemmArgs& a, int bn) {
    const size_t tm = (a.M + G256_BM - 1) / G256_BM, tn = (a.N + bn - 1) / bn;
    // ... and the buffer-descriptor epilogues count a tile's output rows (and the row-bias table) in 32-bit byte offsets whose
    // out-of-range marker is +2^31: 256 rows of fp32 at pitch ldo must stay below that
    return tm * G256_BM * (size_t)a.lda * 2 < (1ull << 31) && tn * bn * (size_t)a.ldw * 2 < (1ull << 31) &&
           (size_t)G256_BM * (size_t)a.ldo * 4 < (1ull << 31) && (!a.rowbias || (size_t)G256_BM * (size_t)a.rowbias_ld * 4 < (1ull << 31));
}

hipError_t launch_gemm256w(const GemmArgs& a, int epi, hipStream_t s) {
    switch (epi) {
        case EPI_BF16: return launch_w<EPI_BF16>(a, s);
        case EPI_GELU: return launch_w<EPI_GELU>(a, s);
        case EPI_F32: return launch_w<EPI_F32>(a, s);
        case EPI_RESID: return launch_w<EPI_RESID>(a, s);
        case EPI_SWIGLU: return launch_w<EPI_SWIGLU>(a, s);
        case EPI_ROPE: return launch_w<EPI_ROPE>(a, s);
        default: return hipErrorInvalidValue;
    }
}

// 256 x 192 tile: N % 192 == 0, residual (the SigLIP proj / fc2 GEMMs) and fp32 (split-K partial products of the
// decoder's o / down projections) epilogues; W rows readable up to the next multiple of 192 (N itself)
hipError_t launch_gemm192w(const GemmArgs& a, int epi, hipStream_t s) {
    if (a.N % 192) return hipErrorInvalidValue;
    if (epi == EPI_RESID && a.ksplit <= 1) return launch_wp<EPI_RESID, false, 6>(a, s);
    if (epi == EPI_F32) return launch_wp<EPI_F32, false, 6>(a, s);          // incl. split-K partial products
    return hipErrorInvalidValue;
}

// 256 x 288 tile: N % 288 == 0 (1152 = 4 x 288: two full rounds of 256 CUs at 32 768 rows where 192 columns take three), the
// lookup-free residual epilogue and nothing else (gemm_args_refused): no tile has a column edge, no row is mapped
hipError_t launch_gemm288w(const GemmArgs& a, int epi, hipStream_t s) {
    if (a.N % 288 || epi != EPI_RESID) return hipErrorInvalidValue;
    return launch_wp<EPI_RESID, false, 9>(a, s);
}

}  // namespace vr
