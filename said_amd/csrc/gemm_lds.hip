// gemm_lds.hip — the UNet GEMM: channel-major fp32 MFMA GEMM / Conv1d(k=1|3, stride 1) with the X operand
// staged ONCE per wave through LDS.
//
// Why (measured on MI355X, scripts/ubench/load_issue.hip): a CU sustains only ~20 B/clk of dword
// buffer loads (~44 B/clk as dwordx4), so the first version of this kernel — two dword loads per MFMA,
// X re-fetched for each of the three conv taps — spent 3-7k clocks just issuing its 72 loads per wave.
// Here a wave
//   * fetches its 24-channel x 32-token slice of X with three dwordx4 loads (+ one dword load for the
//     two halo columns of a k=3 conv), applies the fused operand transform (GroupNorm+SiLU /
//     LayerNorm / GroupNorm->LayerNorm / SiLU) ONCE per element, and parks the result in a wave-private
//     LDS tile — no cross-wave synchronisation is needed for it;
//   * fetches its weight fragments as dwordx4 (host packing puts a lane's four consecutive k-pairs side
//     by side): 9 loads instead of 36 for a conv slice;
//   * runs a main loop that is nothing but ds_read_b32 + v_mfma_f32_32x32x2_f32.
// LayerNorm statistics come from the very registers that were loaded for staging; GroupNorm statistics
// are finalised per wave for its own channel slice from the producer's Welford partials (gemm_common.h).
// Work split, reduction and epilogues are those of gemm.hip: NB output tiles x 32 tokens per workgroup,
// KS waves splitting K by input channel, fixed-order LDS reduction, fused epilogues.
// Here: the kernel, the LDS sizing, and the table of instantiations with its one lookup (configure_ugemm_kernels walks it, launch_ugemm calls the row's launch).
// ugemm_plan.h (host only): the shape lists, the launch variants, ugemm_supports and plan_gemm, which picks a launch's row; ugemm_dev.h: tile constants, header;
// ugemm_body.h, kconv_body.h: the two bodies.
#include <cstdio>
#include <cstdlib>

#include "ugemm_dev.h"
#include "ugemm_body.h"
#include "kconv_body.h"

namespace said {

template <int NB, int KS, int EPI, int VAR, bool BF, bool MT, bool SP = false>
// multi-tile single-n-tile store kernels are compiled for <= 128 VGPRs (4 waves per SIMD): two workgroups share a CU, so one's
// staging / reduction / epilogue phases overlap the other's MFMA stream (large batches)
__global__ __launch_bounds__(64 * KS, (MT && NB == 1 && EPI == EPI_STORE) ? 4 : 1) void ugemm_kernel(const float* hx, const float* hw4, int hpack, int hTN, int hpitch_gv, int hbstride,
                                                        int hbmod_b0, int hgx, const float* hgn_part, int hgn_bstride, int hgn_cfg,
                                                        const GemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // the leading dwords are the preloaded header; `a` only reserves the kernarg layout for arg_view_hs()
    const int hN = (int)((unsigned)hTN >> 16), hgate_vft = (int)((unsigned)hpitch_gv >> 16);
    const FastHdr hd = {hx, hw4, hpack, hpitch_gv & 0xffff, hTN & 0xffff, hbstride, hbmod_b0, hN, hgate_vft, hgn_part, hgn_bstride, hgn_cfg};
    // XCD-aware block order.  Hardware places block id on XCD id % 8; with the natural order every XCD's L2 ends up
    // fetching ALL weights and ALL activations of the launch (rocprofv3 FETCH_SIZE: 4x the algorithmic bytes).  Here
    // each XCD gets a contiguous run of the logical order (n-tile fastest, then t-tile), i.e. a few whole token tiles:
    // it still needs every weight tile but only its own slice of X.  Placement affects speed only.
    // The grid is (token-tile runs x n-tile groups, samples): blocks of one sample with equal blockIdx.x & 7 share an
    // XCD whatever the row's phase, so the decode needs no division by the batch count; the one division left, by the
    // number of n-tile groups, is by one of a few small constants (a run-time integer division is ~25 dependent
    // instructions, and this sits in front of the first load request of every wave).
    const unsigned ny = (unsigned)(((hN + 31) >> 5) / NB), gx = (unsigned)hgx;
    const unsigned cls = blockIdx.x & 7u, slot = blockIdx.x >> 3, q = gx >> 3, r = gx & 7u;
    const unsigned L = (cls < r ? cls * (q + 1) : r * (q + 1) + (cls - r) * q) + slot;
    // L / ny as a multiply-shift with the host's magic number (exact for every L < grid width: the host checks)
    const unsigned ubx = (L * ((unsigned)hbmod_b0 & 0x1ffffu)) >> 16;
    const int bx = (int)ubx, by = (int)(L - ubx * ny), bz = (int)blockIdx.y;
    if constexpr (is_kconv_shape(SP, MT, NB, KS, EPI, VAR)) {
        if (!(hpack & (1 << 27))) {   // (bit 27: said_debug_option "kconv" = 0 — the block loop of ugemm_body, the A/B reference)
            kconv_body<(VAR & UV_GN1) != 0>(hd, smem, bx, by, bz);
            return;
        }
    }
    if constexpr (EPI == EPI_QKV) {
        if (by * NB < hgate_vft) {
            ugemm_body<NB, KS, EPI, VAR, true, BF, MT, SP>(hd, smem, bx, by, bz);
            return;
        }
    }
    ugemm_body<NB, KS, EPI, VAR, false, BF, MT, SP>(hd, smem, bx, by, bz);
}

template <int NB, int EPI>
static int ugemm_smem_floats(const GemmArgs& a, int KS, bool mt = false) {
    constexpr int NACC = (EPI == EPI_GEGLU) ? 2 * NB : NB;
    int coef = 0;
    for (int s = 0; s < a.nseg; ++s) coef += seg_coef_floats(a.seg[s]);
    const int stage = coef + KS * 64 + KS * 8 * NRMAX * XP;
    const int red = (KS * NACC * 16 * 64 * 4 > 128 * 1024) ? KS * (NACC / 2) * 16 * 64 : KS * NACC * 16 * 64;
    const int red_end = mt ? coef + red : red;   // multi-tile: the reduction buffer sits behind the coefficient tables
    return epi_scratch_floats<NACC>(EPI, KS) + KS * GN_SCRATCH + (stage > red_end ? stage : red_end);
}

constexpr int kMaxLds = 160 * 1024;
template <int NB, int KS, int EPI, int VAR, bool BF, bool MT, bool SP>
static void ulaunch_one(const GemmArgs& a, int batch, hipStream_t s, int tt) {
    int smem = ugemm_smem_floats<NB, EPI>(a, KS, MT) * (int)sizeof(float);
    constexpr bool KCONV = is_kconv_shape(SP, MT, NB, KS, EPI, VAR);
    if (KCONV && !a.kconv_off) {   // kconv_body's own carve (separate tiles per block, reduction buffer beside them)
        const int ks = kconv_smem_floats(a.seg[0].C, (VAR & UV_GN1) ? a.seg[1].C : 0, (VAR & UV_GN1) ? 2 : 3) * (int)sizeof(float);
        if (ks > smem) smem = ks;
    }
    if (smem > kMaxLds) { launch_fault("ugemm needs %d B of LDS", smem); return; }
    const int ntt = (a.T + 31) / 32;
    dim3 grid(((MT ? (ntt + tt - 1) / tt : ntt)) * (a.ntiles_per_group / NB), batch);   // x: decoded XCD-aware in the kernel
    const Seg& s0 = a.seg[0];
    const bool gn0 = s0.xform == XF_GN_SILU || s0.xform == XF_GN_LN;
    const int pack = s0.C | (s0.taps << 16) | (s0.xform << 20) | (a.nseg << 24) | ((gn0 && s0.gn_eps == 1e-6f) ? (1 << 26) : 0) |
                     ((MT ? tt : 0) << 28) | ((KCONV && a.kconv_off) ? (1 << 27) : 0);
    const unsigned ny_host = (unsigned)(a.ntiles_per_group / NB), magic = 65536u / ny_host + 1u;
    for (unsigned L = 0; L < grid.x; ++L)   // exactness of the multiply-shift over this launch's range (a few thousand at most)
        if (((L * magic) >> 16) != L / ny_host) { launch_fault("block decode magic inexact (grid %u, ny %u)", grid.x, ny_host); return; }
    const int bmod_b0 = (int)(magic & 0x1ffffu) | (a.b0 << 17);
    const int gate_vft = (EPI == EPI_GEGLU) ? a.geglu_gate_tiles : (EPI == EPI_QKV ? a.tm_tiles : 0);   // tm_tiles shares a union
    hipLaunchKernelGGL((ugemm_kernel<NB, KS, EPI, VAR, BF, MT, SP>), grid, dim3(64 * KS), smem, s, s0.x, SP ? s0.ws : (BF ? s0.w2 : s0.w4), pack,
                       a.T | (a.N << 16), s0.x_pitch | (gate_vft << 16), (int)s0.x_bstride, bmod_b0, (int)grid.x,
                       gn0 ? s0.gn_part : nullptr, (int)s0.gn_part_bstride, s0.gn_cpg | (s0.gn_nparts << 16), a);
}
template <int NB, int KS, int EPI, int VAR, bool BF, bool MT, bool SP>
static void uconfigure_one() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ugemm_kernel<NB, KS, EPI, VAR, BF, MT, SP>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
}

// The instantiations: ugemm_plan.h's three shape lists, expanded once, each row with its launch and configure functions
#define SAID_UGEMM_ROW_FNS(NB, KS, EPI, VAR, BF, MT, SP) &ulaunch_one<NB, KS, EPI, VAR, BF, MT, SP>, &uconfigure_one<NB, KS, EPI, VAR, BF, MT, SP>
static const URow kRows[] = {SAID_UGEMM_ROWS};

const URow* ugemm_row(int epi, int NB, int KS, int var, UMode mode, bool mt) {
    for (const URow& r : kRows)
        if (r.epi == epi && r.NB == NB && r.KS == KS && r.var == var && r.mode == mode && r.mt == mt) return &r;
    return nullptr;
}

void configure_ugemm_kernels() { for (const URow& r : kRows) r.configure(); }

void launch_ugemm(const GemmArgs& a, int epi, int batch, int NB, int KS, hipStream_t s, UMode mode, int tt) {
    if (const URow* r = ugemm_row(epi, NB, KS, uvar_of(a, epi), mode, tt > 1)) r->launch(a, batch, s, tt);
    else launch_fault("unsupported ugemm config epi=%d NB=%d KS=%d mode=%d tt=%d", epi, NB, KS, (int)mode, tt);
}

}  // namespace said
