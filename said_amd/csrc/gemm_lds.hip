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
// Here: the kernel, the LDS sizing, the shape tables and the launch dispatch; ugemm_dev.h: tile constants, header, variants; ugemm_body.h, kconv_body.h: the two bodies.
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
template <int NB, int KS, int EPI, int VAR, bool BF, bool MT, bool SP = false>
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
template <int NB, int KS, int EPI, int VAR, bool BF, bool MT, bool SP = false>
static void uconfigure_one() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&ugemm_kernel<NB, KS, EPI, VAR, BF, MT, SP>), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds);
}

// (epilogue, NB, KS, variant): small-batch tile shapes; large batches use the generic kernel's NB = 3..6 shapes
#define SAID_UGEMM_CONFIGS(X)                                                                                    \
    X(EPI_STORE, 1, 8, 0) X(EPI_STORE, 1, 8, UV_DEEP) X(EPI_STORE, 1, 8, UV_T3 | UV_GN0)                         \
    X(EPI_STORE, 1, 8, UV_MULTI) X(EPI_STORE, 2, 8, UV_MULTI)                                                    \
    X(EPI_STORE, 1, 8, UV_RGN | UV_DUP) X(EPI_STORE, 1, 8, UV_T3 | UV_GN0 | UV_DUP) X(EPI_STORE, 2, 8, UV_T3 | UV_GN0 | UV_DUP) \
    X(EPI_STORE, 1, 8, UV_T3 | UV_GN0 | UV_MULTI)                                                                \
    X(EPI_STORE, 1, 8, UV_T3 | UV_GN0 | UV_GN1 | UV_MULTI) X(EPI_STORE, 1, 8, UV_RGN)                            \
    X(EPI_STORE, 2, 8, 0) X(EPI_STORE, 2, 8, UV_DEEP) X(EPI_STORE, 2, 8, UV_T3 | UV_GN0)                         \
    X(EPI_STORE, 2, 8, UV_T3 | UV_GN0 | UV_MULTI)                                                                \
    X(EPI_STORE, 2, 8, UV_T3 | UV_GN0 | UV_GN1 | UV_MULTI)                                                       \
    X(EPI_STORE, 3, 8, 0) X(EPI_STORE, 3, 8, UV_DEEP) X(EPI_STORE, 3, 8, UV_T3 | UV_GN0) X(EPI_STORE, 3, 8, UV_MULTI) \
    X(EPI_STORE, 3, 8, UV_T3 | UV_GN0 | UV_DUP)                                                                  \
    X(EPI_QKV, 1, 8, UV_GN0) X(EPI_QKV, 2, 8, UV_GN0) X(EPI_QKV, 3, 8, UV_GN0)                                   \
    X(EPI_GEGLU, 1, 8, 0) X(EPI_GEGLU, 2, 8, 0) X(EPI_GEGLU, 4, 8, 0)                                            \
    X(EPI_BAND, 1, 8, 0)

// split-fp16 product shapes (SP; fp32 mode, single-tile workgroups): the small-batch step's launches.  Not built: the shapes that spill with the second
// accumulator set (NB = 2 with two or three K segments of 3-tap blocks, NB = 3 DEEP / MULTI: 148-180 bytes of scratch per lane) and GEGLU other than the one-tile-per-wave
// NB = 4 shape (its weights use the flat step layout) — those launches stay on the fp32 MFMAs.
#define SAID_UGEMM_SP_CONFIGS(X)                                                                                 \
    X(EPI_STORE, 1, 8, 0) X(EPI_STORE, 1, 8, UV_DEEP) X(EPI_STORE, 1, 8, UV_T3 | UV_GN0)                         \
    X(EPI_STORE, 1, 8, UV_MULTI) X(EPI_STORE, 2, 8, UV_MULTI)                                                    \
    X(EPI_STORE, 1, 8, UV_RGN | UV_DUP) X(EPI_STORE, 1, 8, UV_T3 | UV_GN0 | UV_DUP) X(EPI_STORE, 2, 8, UV_T3 | UV_GN0 | UV_DUP) \
    X(EPI_STORE, 1, 8, UV_T3 | UV_GN0 | UV_MULTI)                                                                \
    X(EPI_STORE, 1, 8, UV_T3 | UV_GN0 | UV_GN1 | UV_MULTI) X(EPI_STORE, 1, 8, UV_RGN)                            \
    X(EPI_STORE, 2, 8, 0) X(EPI_STORE, 2, 8, UV_DEEP) X(EPI_STORE, 2, 8, UV_T3 | UV_GN0)                         \
    X(EPI_STORE, 3, 8, 0) X(EPI_STORE, 3, 8, UV_T3 | UV_GN0)                                                     \
    X(EPI_STORE, 3, 8, UV_T3 | UV_GN0 | UV_DUP)                                                                  \
    X(EPI_QKV, 1, 8, UV_GN0) X(EPI_QKV, 2, 8, UV_GN0) X(EPI_QKV, 3, 8, UV_GN0)                                   \
    X(EPI_GEGLU, 4, 8, 0)                                                                                        \
    X(EPI_BAND, 1, 8, 0)

// multi-tile shapes (large batches; single-block launches).  (Round 2's single-n-tile store shapes at two workgroups per CU — an
// experiment that measured slower, two of whose instantiations spilled 6 VGPRs — are gone.)  fp32 GEGLU uses NB = 2: with 8 accumulator tiles the
// weight fragments only fit by rolling them through the registers, which a multi-tile workgroup cannot do.
#define SAID_UGEMM_MT_CONFIGS(X)                                                                   \
    X(EPI_STORE, 2, 8, 0, 0) X(EPI_STORE, 2, 8, UV_T3 | UV_GN0, 0) X(EPI_STORE, 1, 8, UV_RGN, 0)   \
    X(EPI_STORE, 2, 8, 0, 1) X(EPI_STORE, 2, 8, UV_T3 | UV_GN0, 1) X(EPI_STORE, 1, 8, UV_RGN, 1)   \
    X(EPI_STORE, 2, 8, UV_T3 | UV_GN0 | UV_DUP, 0) X(EPI_STORE, 1, 8, UV_RGN | UV_DUP, 0)          \
    X(EPI_STORE, 2, 8, UV_T3 | UV_GN0 | UV_DUP, 1) X(EPI_STORE, 1, 8, UV_RGN | UV_DUP, 1)          \
    X(EPI_QKV, 3, 8, UV_GN0, 0) X(EPI_QKV, 3, 8, UV_GN0, 1)                                        \
    X(EPI_GEGLU, 2, 8, 0, 0) X(EPI_GEGLU, 2, 8, 0, 1)                                              \
    X(EPI_BAND, 1, 8, 0, 0) X(EPI_BAND, 1, 8, 0, 1)

void configure_ugemm_kernels() {
#define X(E, nb, ks, var) uconfigure_one<nb, ks, E, var, false, false>(); uconfigure_one<nb, ks, E, var, true, false>();
    SAID_UGEMM_CONFIGS(X)
#undef X
#define X(E, nb, ks, var) uconfigure_one<nb, ks, E, var, false, false, true>();
    SAID_UGEMM_SP_CONFIGS(X)
#undef X
#define X(E, nb, ks, var, bf) uconfigure_one<nb, ks, E, var, bf != 0, true>();
    SAID_UGEMM_MT_CONFIGS(X)
#undef X
}

static inline bool is_gn(int xf) { return xf == XF_GN_SILU || xf == XF_GN_LN; }
static int uvar_of(const GemmArgs& a, int epi) {
    int v = 0;
    if (a.seg[0].taps == 3) v |= UV_T3;
    if (is_gn(a.seg[0].xform)) v |= UV_GN0;
    if (a.nseg > 1 && is_gn(a.seg[1].xform)) v |= UV_GN1;
    if (epi == EPI_STORE && a.res_kind == RES_GN) v |= UV_RGN;
    if (epi == EPI_STORE && a.y2) v |= UV_DUP;
    if (a.nseg > 1) v |= UV_MULTI;
    else if (a.seg[0].C > 24 * 8) v |= UV_DEEP;   // KS = 8 everywhere: more than one 24-channel block per wave
    return v;
}

// The LDS-staged kernel covers stride-1, k in {1,3}, ungrouped GEMMs whose per-wave channel slice is a
// multiple of 24 (or 8 / 16); everything else stays on the generic kernel.
bool ugemm_supports(const GemmArgs& a, int epi, int NB, int KS, int pm, int tt) {
    const bool bf16 = pm == 1, sp = pm == 2;
    bool cfg = false;
    const int var = uvar_of(a, epi);
    if (tt > 1) {   // multi-tile: own shape list, one K block per wave, at most 15 tiles per workgroup
        bool mt = false;
#define X(E, nb, ks, v, bf) mt = mt || (epi == E && NB == nb && KS == ks && var == (v) && bf16 == (bf != 0));
        SAID_UGEMM_MT_CONFIGS(X)
#undef X
        const int cw = a.seg[0].C / KS;
        if (!mt || tt > 15 || a.nseg != 1 || cw != 24) return false;
    }
#define X(E, nb, ks, v) cfg = cfg || (epi == E && NB == nb && KS == ks && var == (v));
    SAID_UGEMM_CONFIGS(X)
#undef X
    if (!cfg || a.groups != 1 || a.ntiles_per_group % NB) return false;
    if (sp) {   // split-fp16 products: single-tile workgroups, every segment packed for them, the flat layout exactly where the kernel expects it
        bool spc = false;
#define X(E, nb, ks, v) spc = spc || (epi == E && NB == nb && KS == ks && var == (v));
        SAID_UGEMM_SP_CONFIGS(X)
#undef X
        if (tt > 1 || !spc) return false;
        const bool flat_shape = epi == EPI_GEGLU && NB == 4 && KS == 8 && !(var & (UV_MULTI | UV_DEEP));
        for (int s = 0; s < a.nseg; ++s) if (!a.seg[s].ws || (a.seg[s].ws_flat != 0) != flat_shape) return false;
        if (is_kconv_shape(sp, tt > 1, NB, KS, epi, var) && !a.kconv_off) {
            // kconv_body's shapes: every segment 8 x 24 channels; [3-tap GN + SiLU] x 2, or 3-tap GN + SiLU followed by one or two plain 1-tap segments
            const bool gn1 = (var & UV_GN1) != 0;
            if (a.res_kind != RES_NONE || a.y2 || (gn1 ? a.nseg != 2 : (a.nseg < 2 || a.nseg > 3))) return false;
            for (int s = 0; s < a.nseg; ++s) {
                const Seg& sg = a.seg[s];
                const bool gn3 = (s == 0) || gn1;
                if (sg.C != 24 * 8 || sg.taps != (gn3 ? 3 : 1) || sg.xform != (gn3 ? XF_GN_SILU : XF_NONE) || sg.Tin != a.T) return false;
                if (sg.x_bstride > 0x7fffffffLL || sg.gn_part_bstride > 0x7fffffffLL) return false;
            }
            if (a.emb && (long long)a.N * a.emb_pitch * 4 > 0x7fffffffLL) return false;
        }
    }
    {   // what the compile-time variant assumes about the arguments
        const int xf0 = a.seg[0].xform;
        if (epi == EPI_QKV && (xf0 != XF_GN_LN || a.vt_dim <= 0 || (a.vt_dim & (a.vt_dim - 1)))) return false;
        if ((epi == EPI_GEGLU || epi == EPI_BAND) && xf0 != XF_LN) return false;
        if (epi == EPI_STORE && !(xf0 == XF_NONE || xf0 == XF_SILU || xf0 == XF_GN_SILU)) return false;
        if (a.nseg > 2 && is_gn(a.seg[2].xform)) return false;
        if ((xf0 == XF_LN || xf0 == XF_GN_LN) && !(a.seg[0].w4_ln_tail && a.seg[0].ln_eps == 1e-5f)) return false;
        const int nacc = (epi == EPI_GEGLU) ? 2 * NB : NB;
        if (nacc >= 8 && !(a.nseg == 1 && a.seg[0].C == 24 * KS)) return false;   // rolling weight rounds: one block only
        if (epi != EPI_STORE && a.res_kind != RES_NONE) return false;
        if (!(var & UV_T3))
            for (int s = 0; s < a.nseg; ++s) if (a.seg[s].taps != 1) return false;
        if (var & UV_RGN) {   // one residual GroupNorm group per wave
            const int c_span = NB * 32;
            if (a.res_gn_cpg <= 0 || (c_span + a.res_gn_cpg - 1) / a.res_gn_cpg + 1 > KS) return false;
        }
    }
    if (a.seg[0].x_bstride > 0x7fffffffLL || a.b0 > 0x3fff || a.seg[0].C > 0xffff) return false;
    for (int s = 0; s < a.nseg; ++s) if (a.seg[s].b_mod != 0) return false;   // sample aliasing (b % b_mod) stays on the generic kernel
    if (a.seg[0].Tin != a.T || a.ntiles_per_group != (a.N + 31) / 32) return false;
    if (a.T > 0xffff || a.N > 0xffff || a.seg[0].x_pitch > 0xffff || a.geglu_gate_tiles > 0xffff || (epi == EPI_QKV && a.tm_tiles > 0xffff)) return false;   // packed header fields
    {   // header-only GroupNorm path of segment 0: parameters behind the weights, eps one of two known values
        const Seg& s0 = a.seg[0];
        if (s0.xform == XF_GN_SILU || s0.xform == XF_GN_LN) {
            if (!s0.w4_gn_tail || !(s0.gn_eps == 1e-5f || s0.gn_eps == 1e-6f)) return false;
            if (s0.gn_part_bstride > 0x7fffffffLL || s0.gn_cpg > 0xffff || s0.gn_nparts > 0x7fff) return false;
        }
    }
    for (int s = 0; s < a.nseg; ++s) {
        const Seg& sg = a.seg[s];
        if (bf16 && !sg.w2) return false;
        if (!sg.w4 || sg.stride != 1 || !(sg.taps == 1 || sg.taps == 3) || sg.pad != (sg.taps - 1) / 2) return false;
        if (sg.taps == 3 && epi != EPI_STORE) return false;
        if (sg.C % KS) return false;
        const int cw = sg.C / KS;
        if (cw % 24 != 0) return false;   // blocks of three 8-channel rounds; narrower slices stay on the generic kernel
        if ((sg.xform == XF_GN_SILU || sg.xform == XF_GN_LN) && (cw % sg.gn_cpg || cw > 64)) return false;
        if ((sg.xform == XF_LN || sg.xform == XF_GN_LN) && (sg.taps != 1 || cw > 24 || s != 0)) return false;
    }
    return true;
}

void launch_ugemm(const GemmArgs& a, int epi, int batch, int NB, int KS, hipStream_t s, int pm, int tt) {
    const int var = uvar_of(a, epi);
    const bool bf16 = pm == 1, sp = pm == 2;
    if (tt > 1) {
#define X(E, nb, ks, v, bf) \
        if (epi == E && NB == nb && KS == ks && var == (v) && bf16 == (bf != 0)) { ulaunch_one<nb, ks, E, v, bf != 0, true>(a, batch, s, tt); return; }
        SAID_UGEMM_MT_CONFIGS(X)
#undef X
    }
    if (sp) {
#define X(E, nb, ks, v) \
        if (epi == E && NB == nb && KS == ks && var == (v)) { ulaunch_one<nb, ks, E, v, false, false, true>(a, batch, s, 1); return; }
        SAID_UGEMM_SP_CONFIGS(X)
#undef X
        launch_fault("unsupported split-fp16 ugemm config epi=%d NB=%d KS=%d", epi, NB, KS);
        return;
    }
#define X(E, nb, ks, v) \
    if (epi == E && NB == nb && KS == ks && var == (v)) {                   \
        if (bf16) ulaunch_one<nb, ks, E, v, true, false>(a, batch, s, 1);   \
        else ulaunch_one<nb, ks, E, v, false, false>(a, batch, s, 1);       \
        return;                                                             \
    }
    SAID_UGEMM_CONFIGS(X)
#undef X
    launch_fault("unsupported ugemm config epi=%d NB=%d KS=%d", epi, NB, KS);
}

}  // namespace said
