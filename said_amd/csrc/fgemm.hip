// fgemm.hip — the K-split 64-row tile of the token-major GEMMs (fgemm_kernel): fp32 operands on v_mfma_f32_32x32x2_f32, their split-fp16 variants, and the same
// workgroup on bf16 operands (the UNet's batch-as-rows GEMMs).  launch_tgemm (tgemm.hip) decides which launches come here.
#include <algorithm>
#include <type_traits>

#include "gemm_common.h"
#include "tgemm.h"
#include "tgemm_dev.h"
#include "split_f16.h"

namespace said {

// ------------------------------------------------------------------------------------------------------------------
// fp32 token-major GEMM (fp32 mode, large batches: BASELINE configs[3]'s per-GPU work) on v_mfma_f32_32x32x2_f32.
// Same operand geometry in BYTES as the bf16 kernels — a k-tile is 128 bytes per row (32 floats), LDS rows 144 bytes, 16-byte
// fragment reads — and the same epilogue.  A lane's 16-byte fragment holds k = 8 s + 4 (l >> 5) + {0..3}; MFMA i of step s
// multiplies element i of the A and W fragments, i.e. the k pair (8 s + i, 8 s + 4 + i) — a permutation of k both operands share.
//
// Workgroup: tile 64 rows x 32 NJ columns, ONE LDS operand buffer (23-28 KB), FOUR waves = 2 row halves x 2 K HALVES: wave
// (r, kh) multiplies rows 32 r .. 32 r + 31 by k = 16 kh .. 16 kh + 15 of every 32-k tile; the two K halves are added through
// LDS once, after the loop (12-16 KB per pair), and wave (r, 0) runs the epilogue.  3-4 workgroups share a CU, each in its own
// phase, so one's prologue / barriers / epilogue hide under the others' MFMAs.
//
// Why this shape (every step measured on the MI355X, scripts/gpu_r2_m.sh ... gpu_r2_u.sh):
//  * the channel-major ugemm family splits K over the 8 waves of a 32-token tile and pays a 64 KB LDS reduction per tile: 40 % of
//    the fp32 MFMA roof at Be = 64.  A first token-major shape (64 x 192 tile, 4 waves, each 32 x 96 over the whole K, double-
//    buffered) ran the 192-wide convolutions at 144 us where the MFMAs alone need 55.
//  * these GEMMs are MFMA-bound, and an MFMA-bound launch is a bin-packing of indivisible wave-tiles onto 1024 SIMDs: 38912 rows
//    x 192 columns in 32 x 96 wave-tiles over the whole K are 2432 units = 2.375 per SIMD -> 3 on the busiest, 79 % at best,
//    whatever the workgroup shape.  Halving K per wave halves the unit (4.75 -> 5 per SIMD: 95 %) WITHOUT extra operand traffic
//    — all four waves read the same LDS tiles.  (Smaller output tiles would also balance, but cost L2 bandwidth, see below.)
//  * knock-outs of this kernel's loop: no barriers -0 %, no LDS stores -3 %, no global loads -22 %.  The loads are not waited
//    for (average L2 latency seen by the L1 is 219 clocks, TCP_TCC_READ_REQ_LATENCY / TCP_TCC_READ_REQ; a second register set,
//    PF = 2, buys 5 %); what they cost is the MFMA RATE itself (power-managed clock, or register-file / issue contention — not
//    separated): scripts/ubench/mfma_with_loads.hip — pure fp32 MFMA loops on all CUs — sustains
//    150 TFLOP/s alone, 135 with 3.2 TB/s of independent L2 loads beside them, 114 with 5.4 TB/s, 112 with 10.5 TB/s.  A 64 x 96
//    tile needs 20 KB per 48 MFMA-times: ~5 TB/s at the rate it runs.  So ~115 TFLOP/s is the practical roof of an fp32 GEMM at
//    these tile sizes, and this kernel's 93-98 (convolutions), 87 (q/k/v, K = 192) and 93 (GEGLU) sit at 75-85 % of it.
// ------------------------------------------------------------------------------------------------------------------
// NJ = 3: 64 x 96 tile (N = 192 / 576), NJ = 4: 64 x 128 (GEGLU, value / gate column tiles interleaved as for the bf16 kernel).
// PF = 2: two register sets, the tile two k-steps ahead is in flight while the current one multiplies.
// BF: the same workgroup on bf16 operands (bf16 mode's UNet GEMMs): a k-tile is again 128 bytes per row (64 halfs), each K half
// two v_mfma_f32_32x32x16_bf16 per column tile.  There the point is not MFMA balance but spread: the 256-row bf16 tiles put a
// 192-wide convolution on 152 workgroups of a 256-CU chip, and its time is the fp32 epilogue traffic (§7.3).
constexpr int FGEMM_PK_LDS3 = 2 * (64 + 96) * 144 > fgemm_lds_bytes<3>() ? 2 * (64 + 96) * 144 : fgemm_lds_bytes<3>();   // packed mode: two operand buffers
constexpr int fgemm_occ(int NJ, int PF, bool BF) { return NJ == 3 ? 4 : 3; }   // workgroups per CU the registers are budgeted for
// SP (round 4, fp32 operands only): the products run on SPLIT-fp16 operands (split_f16.h: x = h + 2^-11 l, three v_mfma_f32_32x32x16_f16 per eight
// v_mfma_f32_32x32x2_f32, fp32 accumulation, the cross terms in a second accumulator set).  The LDS tiles stay fp32 — staging, K halves, exchange and
// epilogue are untouched; a wave's lane half takes the EIGHT consecutive k (16 kh + 8 lh ...) of the 32-k tile as two 16-byte reads per operand row and
// splits them in registers (A once, W once per column tile — ALL of a k-tile's operands in distinct registers: two workgroups per CU), then operand_fence(), then the
// 3 NJ MFMAs, then a second fence.  A variant that split one column tile at a time (three workgroups per CU) — its conversions rewriting the operand registers of
// MFMAs issued 16 idle slots earlier — was not bit-stable from one run to the next (profiles/r04i_attn_split_hazard.txt).
// PK (round 6, SP only): the operands ARRIVE split — every element of A / A2 / W is one dword h | l << 16 (prep_kernel's pack mode, engine.cpp's packed weight copies) — and a
// fragment is unpacked with eight v_perm_b32 instead of ~40 VALU instructions of conversion: with one k16 step (9 MFMAs of 8 passes) per k-tile and wave, the splits of A and of
// three W fragments were 2.4 x the matrix time.  Same planes, same products: bit-identical to the in-kernel split.
template <int NJ, int PF, bool BF, int OCC = fgemm_occ(NJ, PF, BF), bool SP = false, bool PK = false>
__global__ __launch_bounds__(256, OCC) void fgemm_kernel(const TGemmArgs a) {
    static_assert(!(SP && BF), "the split mode reads fp32 operands");
    static_assert(!PK || SP, "packed operands are split operands");
    extern __shared__ __attribute__((aligned(16))) unsigned short lds[];   // [A 64 rows | W BN rows] x 144 bytes
    float* const ldsf = reinterpret_cast<float*>(lds);
    typedef typename std::conditional<BF, unsigned short, float>::type elt_t;
    constexpr int EPC = BF ? 8 : 4;              // elements per 16-byte chunk
    constexpr int FBK = 8 * EPC, FLP = 9 * EPC;  // k per tile (128 bytes), LDS row pitch (144 bytes), in elements
    elt_t* const ldse = reinterpret_cast<elt_t*>(lds);
    constexpr int BM = 64, BN = 32 * NJ, NTH = 256;
    constexpr int ACH = BM * 8 / NTH, WCH = BN * 8 / NTH;   // 16-byte chunks per thread and tile: 2, NJ
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    const int wr = w & 1, kh = w >> 1;
    const int rows_tot = a.batch * a.seg_rows;   // batch-as-rows addressing only (tgemm_supports)
    const int NT = a.N / BN, MT = (rows_tot + BM - 1) / BM;
    // (xcd_tile, tgemm_dev.h, written out: the call, although inlined, changes this kernel's instruction stream — integer range facts derived in a different order)
    const unsigned L = blockIdx.x, xcd = L & 7u, slot = L >> 3;
    const int nt = (int)(slot % (unsigned)NT);
    const int mg = (int)(slot / (unsigned)NT) * 8 + (int)xcd;
    if (mg >= MT) return;   // padding of the tile count to a multiple of 8 (the whole workgroup exits together)
    const int m0 = mg * BM, n0 = nt * BN;
    const elt_t* A = reinterpret_cast<const elt_t*>(a.a);
    const elt_t* A2 = reinterpret_cast<const elt_t*>(a.a2);
    const elt_t* W = reinterpret_cast<const elt_t*>(a.w);
    const int nk = a.K / FBK;
    const int nk1 = (a.a2 ? a.K1 : a.K) / FBK;

    f32x4 ra[ACH], rw[WCH], ra1[PF == 2 ? ACH : 1], rw1[PF == 2 ? WCH : 1];
    int aoff[ACH], a2off[ACH], woff[WCH];   // element offsets: < 2^31 (host-checked)
    int loff[ACH], lwoff[WCH];
#pragma unroll
    for (int i = 0; i < ACH; ++i) {
        const int c = tid + NTH * i, row = c >> 3, kp = c & 7;
        const int m = min(m0 + row, rows_tot - 1);
        aoff[i] = m * a.lda + kp * EPC;
        a2off[i] = m * a.lda2 + kp * EPC;
        loff[i] = row * FLP + kp * EPC;
    }
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
        const int c = tid + NTH * i, row = c >> 3, kp = c & 7;
        woff[i] = (n0 + row) * a.K + kp * EPC;
        lwoff[i] = BM * FLP + row * FLP + kp * EPC;
    }
    auto gload_tile = [&](f32x4* xa, f32x4* xw, int kt) {
        const bool first = kt < nk1;
#pragma unroll
        for (int i = 0; i < ACH; ++i) {
            const elt_t* p = first ? A + (aoff[i] + kt * FBK) : A2 + (a2off[i] + (kt - nk1) * FBK);
            xa[i] = *reinterpret_cast<const f32x4*>(p);
        }
#pragma unroll
        for (int i = 0; i < WCH; ++i) xw[i] = *reinterpret_cast<const f32x4*>(W + (woff[i] + kt * FBK));
    };
    // PK: TWO operand buffers in LDS — the next tile is parked in the other buffer before the one barrier of a k-step (the single-buffer loop pays two barriers per
    // nine MFMAs of a wave); the other variants keep one buffer (their k loop is bound elsewhere, and their occupancy is budgeted on 23-28 KB)
    constexpr int BUFE = PK ? (BM + BN) * FLP : 0;   // elements between the two buffers
    auto lds_store = [&](const f32x4* xa, const f32x4* xw, int buf = 0) {
#pragma unroll
        for (int i = 0; i < ACH; ++i) *reinterpret_cast<f32x4*>(ldse + buf * BUFE + loff[i]) = xa[i];
#pragma unroll
        for (int i = 0; i < WCH; ++i) *reinterpret_cast<f32x4*>(ldse + buf * BUFE + lwoff[i]) = xw[i];
    };
    f32x16 acc[NJ], accx[SP ? NJ : 1];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[j][r] = 0.f;
            if (SP) accx[SP ? j : 0][r] = 0.f;
        }
    // fragment of step ks: bytes 64 kh + 32 ks + 16 (l >> 5) of the row — the same byte offsets for both element types
    const int frow = l & 31, fk = EPC * (l >> 5) + 4 * EPC * kh;
    const elt_t* const pa = ldse + (wr * 32 + frow) * FLP + fk;
    const elt_t* const pw = ldse + BM * FLP + frow * FLP + fk;
    // (split mode: floats 16 kh + 8 lh .. + 7 of the row)
    const float* const paS = ldsf + (wr * 32 + frow) * 36 + 16 * kh + 8 * (l >> 5);
    const float* const pwS = ldsf + BM * 36 + frow * 36 + 16 * kh + 8 * (l >> 5);
    auto compute = [&](int buf = 0) {
        if constexpr (SP) {
            const float* const pa2 = paS + buf * BUFE;
            const float* const pw2 = pwS + buf * BUFE;
            const SplitH sa = PK ? unpack_f16x8(*reinterpret_cast<const f32x4*>(pa2), *reinterpret_cast<const f32x4*>(pa2 + 4))
                                 : split_f16x8(*reinterpret_cast<const f32x4*>(pa2), *reinterpret_cast<const f32x4*>(pa2 + 4));
            SplitH sb[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                sb[j] = PK ? unpack_f16x8(*reinterpret_cast<const f32x4*>(pw2 + j * 32 * 36), *reinterpret_cast<const f32x4*>(pw2 + j * 32 * 36 + 4))
                           : split_f16x8(*reinterpret_cast<const f32x4*>(pw2 + j * 32 * 36), *reinterpret_cast<const f32x4*>(pw2 + j * 32 * 36 + 4));
            operand_fence();
            // two MFMAs on the same accumulator are NJ - 1 or more apart (never back to back: attn.hip)
#pragma unroll
            for (int j = 0; j < NJ; ++j) accx[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(sa.l, sb[j].h, accx[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(sa.h, sb[j].h, acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NJ; ++j) accx[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(sa.h, sb[j].l, accx[j], 0, 0, 0);
            operand_fence();   // (the next k-tile's split reuses these operand registers)
            return;
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            if constexpr (BF) {
                const bf16x8 fa = *reinterpret_cast<const bf16x8*>(pa + ks * 16);
                bf16x8 fb[NJ];
#pragma unroll
                for (int j = 0; j < NJ; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(pw + j * 32 * FLP + ks * 16);
#pragma unroll
                for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb[j], acc[j], 0, 0, 0);
            } else {
                const f32x4 fa = *reinterpret_cast<const f32x4*>(pa + ks * 8);
                f32x4 fb[NJ];
#pragma unroll
                for (int j = 0; j < NJ; ++j) fb[j] = *reinterpret_cast<const f32x4*>(pw + j * 32 * FLP + ks * 8);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j][i], acc[j], 0, 0, 0);
            }
        }
    };
    // Every load and LDS store of the loop is unconditional, as in tgemm_kernel (steps past the end re-request the last tile).
    // One k-step: request a later tile -> multiply the tile in LDS -> barrier (all four waves have read it) -> park the next
    // tile -> barrier.
    gload_tile(ra, rw, 0);
    if constexpr (PF == 2) gload_tile(ra1, rw1, min(1, nk - 1));
    lds_store(ra, rw);
    __syncthreads();
    if constexpr (PF == 2) {
        for (int kt = 0; kt < nk; kt += 2) {
            gload_tile(ra, rw, min(kt + 2, nk - 1));
            __builtin_amdgcn_sched_barrier(0);
            compute();
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
            lds_store(ra1, rw1);
            __syncthreads();
            gload_tile(ra1, rw1, min(kt + 3, nk - 1));
            __builtin_amdgcn_sched_barrier(0);
            if (kt + 1 < nk) compute();
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
            lds_store(ra, rw);
            __syncthreads();
        }
    } else if constexpr (PK) {
        // tile kt multiplies from buffer kt & 1 while tile kt + 1 (in registers since the previous step) is parked in the other one — free since every wave passed the
        // previous barrier behind its products on it — and tile kt + 2 is requested: ONE barrier per k-step
        gload_tile(ra, rw, min(1, nk - 1));
        for (int kt = 0; kt < nk; ++kt) {
            __builtin_amdgcn_sched_barrier(0);
            compute(kt & 1);
            __builtin_amdgcn_sched_barrier(0);
            lds_store(ra, rw, (kt + 1) & 1);
            gload_tile(ra, rw, min(kt + 2, nk - 1));
            __syncthreads();
        }
    } else {
        for (int kt = 0; kt < nk; ++kt) {
            gload_tile(ra, rw, min(kt + 1, nk - 1));
            __builtin_amdgcn_sched_barrier(0);
            compute();
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
            lds_store(ra, rw);
            __syncthreads();
        }
    }
    // ---- add the two K halves.  NJ = 4 (GEGLU: the epilogue is 18 % of the kernel, mostly erf) splits the epilogue as well: wave
    // (r, 0) finishes column tiles [0, 2), wave (r, 1) tiles [2, 4) — each parks the tiles the OTHER one finishes in the exchange
    // area (lane-linear, region r), a barrier, each adds its partner's half to its own; a second barrier frees the area, which
    // then serves as the waves' transposition scratch (245 -> 235 us).  NJ = 3: wave (r, 1) parks everything, wave (r, 0) finishes
    // all three tiles (the 2 : 1 split measured slower: 122.5 -> 126.7 us).
    if constexpr (SP) {
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = fmaf(accx[j][r], 0x1p-11f, acc[j][r]);
    }
    constexpr int NJ0 = NJ == 4 ? 2 : NJ, NJ1 = NJ - NJ0;
    // (unsplit: region r is also wave (r, 0)'s scratch, so the regions are spaced by the scratch size and never overlap)
    float* const xr = ldsf + wr * (NJ1 > 0 ? NJ * 16 * 64 : 32 * (32 * NJ + 4));
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if ((kh == 1) == (j < NJ0)) {
#pragma unroll
            for (int r = 0; r < 16; ++r) xr[(j * 16 + r) * 64 + l] = acc[j][r];
        }
    }
    __syncthreads();
    if (NJ1 > 0 || kh == 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if ((kh == 0) == (j < NJ0)) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] += xr[(j * 16 + r) * 64 + l];
            }
        }
    }
    if constexpr (NJ1 > 0) {
        __syncthreads();
        float* sc = ldsf + w * (32 * (32 * NJ0 + 4));
        if (kh == 0) tg_epilogue<NJ, 0, NJ0>(a, acc, 0, m0 + wr * 32, n0, l, sc);
        else tg_epilogue<NJ, NJ0, (NJ1 > 0 ? NJ1 : 1)>(a, acc, 0, m0 + wr * 32, n0 + 32 * NJ0, l, sc);
    } else {
        // region r holds only wave (r, 0)'s partner data, which it has just consumed: the row half's transposition scratch (in-order
        // LDS).  Round 3: wave (r, 0) runs phase 1 alone, then BOTH waves of the row half share phase 2 — half the channels (channel-
        // major results) or half the rows (token-major ones) each; before, wave (r, 1) had exited and two of the workgroup's four
        // waves carried the whole memory-facing half of the kernel.
        if (kh == 0) {
            __builtin_amdgcn_wave_barrier();
            tg_epilogue<NJ, 0, NJ, -1, 1>(a, acc, 0, m0 + wr * 32, n0, l, xr);
        }
        __syncthreads();
        tg_epilogue<NJ, 0, NJ, -1, 2>(a, acc, 0, m0 + wr * 32, n0, l, xr, nullptr, kh);
    }
}

// ---- host side: the fp32 and the bf16 batch-as-rows launches of launch_tgemm (which has checked tgemm_supports and filled in a.batch)
void configure_fgemm_kernels() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fgemm_kernel<3, 2, false>), hipFuncAttributeMaxDynamicSharedMemorySize, fgemm_lds_bytes<3>());
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fgemm_kernel<4, 1, false>), hipFuncAttributeMaxDynamicSharedMemorySize, fgemm_lds_bytes<4>());
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fgemm_kernel<3, 1, false, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, fgemm_lds_bytes<3>());
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fgemm_kernel<3, 1, false, 2, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, FGEMM_PK_LDS3);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fgemm_kernel<4, 1, false, 2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, fgemm_lds_bytes<4>());
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fgemm_kernel<3, 1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, fgemm_lds_bytes<3>());
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&fgemm_kernel<4, 1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, fgemm_lds_bytes<4>());
}
bool launch_fgemm(const TGemmArgs& a, hipStream_t s) {
    const long long rows_tot = (long long)a.batch * a.seg_rows;   // batch-as-rows addressing only
    const long long mt8 = ((rows_tot + 63) / 64 + 7) / 8 * 8;   // 64-row tiles, padded to the 8 XCDs
    constexpr int LDS3 = fgemm_lds_bytes<3>(), LDS4 = fgemm_lds_bytes<4>();
    if (a.f32) {
        if (a.grp > 1) return false;
        if ((rows_tot + 2) * (long long)std::max(a.lda, a.lda2) >= 0x7fffffffLL) return false;   // 32-bit operand offsets
        if (a.f32_split) {   // products on split-fp16 operands (TGemmArgs::f32_split)
            if (a.f32_packed) {   // ... which arrive split (NJ = 3 shapes: the ResBlock convolutions and q / k / v)
                if (a.N % 96 || a.geglu) return false;
                hipLaunchKernelGGL((fgemm_kernel<3, 1, false, 2, true, true>), dim3((unsigned)(mt8 * (a.N / 96))), dim3(256), FGEMM_PK_LDS3, s, a);
                return true;
            }
            if (a.N % 128 == 0 && (a.geglu || a.N % 96)) hipLaunchKernelGGL((fgemm_kernel<4, 1, false, 2, true>), dim3((unsigned)(mt8 * (a.N / 128))), dim3(256), LDS4, s, a);
            else hipLaunchKernelGGL((fgemm_kernel<3, 1, false, 2, true>), dim3((unsigned)(mt8 * (a.N / 96))), dim3(256), LDS3, s, a);
            return true;
        }
        if (a.N % 128 == 0 && (a.geglu || a.N % 96)) hipLaunchKernelGGL((fgemm_kernel<4, 1, false>), dim3((unsigned)(mt8 * (a.N / 128))), dim3(256), LDS4, s, a);
        else hipLaunchKernelGGL((fgemm_kernel<3, 2, false>), dim3((unsigned)(mt8 * (a.N / 96))), dim3(256), LDS3, s, a);   // (one register
        // set at five workgroups per CU — the bf16 variant's choice — spills and measured 344 vs 328 ms here)
        return true;
    }
    const bool wide_n = a.N % 128 == 0 && (a.geglu || a.N % 96);
    // (the GEGLU tile squeezed to 128 VGPRs for four per CU spills five registers and measured no better: 121.7 vs 120.1 ms)
    if (wide_n) hipLaunchKernelGGL((fgemm_kernel<4, 1, true>), dim3((unsigned)(mt8 * (a.N / 128))), dim3(256), LDS4, s, a);
    // one register set at FIVE workgroups per CU (96 VGPRs): the 1216 workgroups of a 192-wide launch at Be = 64 are all
    // resident at once instead of 1024 + a tail of 192 (two register sets at four per CU) — 124.5 -> 121.0 ms per 32 clips x 50 steps,
    // three alternating runs on one box (scripts/gpu_r2_ar.sh)
    else hipLaunchKernelGGL((fgemm_kernel<3, 1, true>), dim3((unsigned)(mt8 * (a.N / 96))), dim3(256), LDS3, s, a);
    return true;
}

}  // namespace said
