// ugemm_plan.h — everything about a UNet GEMM launch that is decided on the host and needs no GPU: which instantiations of ugemm_kernel (gemm_lds.hip) exist,
// what each assumes about its arguments (ugemm_supports), the column-tile rules of the schedules, and plan_gemm — the ONE place that turns a launch's
// arguments into (NB, KS, token tiles per workgroup, kernel).  Host code only: gemm_lds.hip attaches the kernels to the rows, unet_sched.cpp launches by the
// plan, tests/ugemm_plan_main.cpp prints the plans without a device.
#pragma once
#include <algorithm>

#include "kernels.h"

namespace said {

// ---- the instantiations: three lists, expanded ONCE into a table (SAID_UGEMM_ROWS) ----
// (epilogue, NB, KS, variant): small-batch tile shapes, each built for fp32 and for bf16 products; large batches use the generic kernel's NB = 3..6 shapes
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

// multi-tile shapes (large batches; single-block launches; last column: bf16).  (Round 2's single-n-tile store shapes at two workgroups per CU — an
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

// One instantiation ugemm_kernel<NB, KS, epi, var, mode == U_BF16, mt, mode == U_SP>.  launch / configure: set by whoever defines
// SAID_UGEMM_ROW_FNS(NB, KS, EPI, VAR, BF, MT, SP) before expanding the table (gemm_lds.hip: ulaunch_one, uconfigure_one); a host program leaves them null.
struct URow {
    int epi, NB, KS, var;
    UMode mode;
    bool mt, kconv;   // multi-tile workgroups; launches run kconv_body (is_kconv_shape)
    void (*launch)(const GemmArgs& a, int batch, hipStream_t s, int tt);
    void (*configure)();
};
#define SAID_UGEMM_ROW(E, nb, ks, v, m, mt) \
    {E, nb, ks, v, m, mt, is_kconv_shape(m == U_SP, mt, nb, ks, E, v), SAID_UGEMM_ROW_FNS(nb, ks, E, v, m == U_BF16, mt, m == U_SP)},
#define SAID_UGEMM_ROW_BASE(E, nb, ks, v) SAID_UGEMM_ROW(E, nb, ks, v, U_F32, false) SAID_UGEMM_ROW(E, nb, ks, v, U_BF16, false)
#define SAID_UGEMM_ROW_SP(E, nb, ks, v) SAID_UGEMM_ROW(E, nb, ks, v, U_SP, false)
#define SAID_UGEMM_ROW_MT(E, nb, ks, v, bf) SAID_UGEMM_ROW(E, nb, ks, v, (bf ? U_BF16 : U_F32), true)
#define SAID_UGEMM_ROWS SAID_UGEMM_CONFIGS(SAID_UGEMM_ROW_BASE) SAID_UGEMM_SP_CONFIGS(SAID_UGEMM_ROW_SP) SAID_UGEMM_MT_CONFIGS(SAID_UGEMM_ROW_MT)
// the table's one lookup (defined beside the table: gemm_lds.hip); nullptr: not built
const URow* ugemm_row(int epi, int NB, int KS, int var, UMode mode, bool mt);

inline bool is_gn(int xf) { return xf == XF_GN_SILU || xf == XF_GN_LN; }
inline int uvar_of(const GemmArgs& a, int epi) {
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
// True when ugemm_kernel serves the launch: the instantiation (epi, NB, KS, uvar_of(a), mode, tt > 1) is built and the arguments are what it assumes.
inline bool ugemm_supports(const GemmArgs& a, int epi, int NB, int KS, UMode mode, int tt = 1) {
    const int var = uvar_of(a, epi);
    const URow* r = ugemm_row(epi, NB, KS, var, mode, tt > 1);
    if (!r || a.groups != 1 || a.ntiles_per_group % NB) return false;
    // multi-tile: one K block per wave, at most 15 tiles per workgroup
    if (tt > 1 && (tt > 15 || a.nseg != 1 || a.seg[0].C / KS != 24)) return false;
    if (mode == U_SP) {   // split-fp16 products: every segment packed for them, the flat layout exactly where the kernel expects it
        const bool flat_shape = epi == EPI_GEGLU && NB == 4 && KS == 8 && !(var & (UV_MULTI | UV_DEEP));
        for (int s = 0; s < a.nseg; ++s) if (!a.seg[s].ws || (a.seg[s].ws_flat != 0) != flat_shape) return false;
        if (r->kconv && !a.kconv_off) {
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
        if (mode == U_BF16 && !sg.w2) return false;
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

namespace host {

// UNet GEMMs with 6 output tiles (192 channels): the LDS-staged kernel at every batch size — two tiles per workgroup
// as soon as that still fills the chip (measured at Be=32: 47 TFLOP/s against 34 for the generic NB=6 shape)
// Column tiles per workgroup (NB) of the UNet's 192-wide channel-major GEMMs.  A launch is t_tiles x 6 / NB workgroups on 256 CUs; its
// time is that of the busiest CU: ceil(workgroups / 256) workgroups of (F + NB) units each, F = 0.45 the per-workgroup fixed part
// (GroupNorm finalisation, operand tile; fitted on T = 1800: NB = 1 14.8 us, NB = 2 25.0 us at 342 workgroups each).  Round 2's rule
// (NB = 2 from 64 tiles) put 342 workgroups on 256 CUs at T = 1800: two rounds of three units where NB = 3 is one round of 3.45.
inline int best_nb(long long token_tiles, int column_tiles) {
    int best = 1;
    double cost = 1e30;
    for (int nb = 1; nb <= 3; ++nb) {
        const long long wgs = token_tiles * (column_tiles / nb);
        const double k = (double)((wgs + 255) / 256) * (0.45 + nb);
        if (k < cost - 1e-9) { cost = k; best = nb; }
    }
    return best;
}
inline int pick_unet_nb(long long t_tiles_total) {
    if (t_tiles_total * 6 > 1024) return t_tiles_total * 3 >= 192 ? 2 : 1;   // (large launches: multi-tile NB = 2 shapes)
    return best_nb(t_tiles_total, 6);
}
// q/k/v (18 column tiles): the largest shape that still gives every CU a workgroup in ONE round (at Be=2, T=600:
// NB=3 -> 228 workgroups, 27.5 -> 13.8 us per launch against NB=1's 684 workgroups in 2.7 rounds)
// pick_unet_nb's busiest-CU model over the 18 column tiles where it applies (19 tiles: NB 1 -> 2, 342 -> 171 workgroups)
inline int qkv_nb(long long tt1) { return tt1 * 18 <= 1024 ? best_nb(tt1, 18) : (tt1 * 6 >= 192 ? 3 : (tt1 * 9 >= 192 ? 2 : 1)); }
inline int geglu_nb(long long tt) { return tt * 6 >= 192 ? 4 : (tt * 12 >= 192 ? 2 : 1); }   // one round of workgroups, as for qkv

// what plan_gemm reads of the context (unet_sched.cpp plan_switches): bf16 mode, sp_on(ugemm_split), said_debug_option "kconv", clk_on, cur_concurrent
struct PlanSwitches { bool bf16, split; int kconv; bool clk, concurrent; };
enum class GemmKernel { cgemm /* the generic kernel, gemm.hip */, ugemm_f32, ugemm_bf16, ugemm_sp /* ugemm_kernel by product mode */ };
struct GemmPlan {
    int NB, KS, tt; GemmKernel kernel;   // tt > 1: multi-tile workgroups
    bool on_ugemm() const { return kernel != GemmKernel::cgemm; }
    UMode mode() const { return kernel == GemmKernel::ugemm_bf16 ? U_BF16 : (kernel == GemmKernel::ugemm_sp ? U_SP : U_F32); }
};

// Multi-tile workgroups (gemm_lds.hip, MT): once a launch would have several thousand workgroups, each workgroup walks
// over `tt` consecutive token tiles instead, keeping its weights in registers; tt is chosen so that ~4 workgroups per
// CU remain.  Returns 1 when the launch is not eligible.
constexpr long long KCONV_MAX_TILES = 4096;   // plan_gemm: launches of at most this many (sample, token tile) pairs may run the K-long convolutions as NB = 1 kconv_body workgroups
constexpr long long MT_WGS_PER_TILE = 1024;   // workgroups per extra token tile of a large launch
constexpr long long MT_MID_WGS = 228;         // ... of a mid-size one
inline int pick_tt(const GemmArgs& a, int epi, int batch, int NB, int KS, UMode mode) {
    if (a.step_inc || epi == EPI_GEGLU || epi == EPI_BAND) return 1;   // GEGLU, band: measured slower multi-tile (B=32: GEGLU NB=2 x tt vs NB=4, band)
    const long long ntt = (a.T + 31) / 32;
    const long long wgs = ntt * (a.ntiles_per_group / NB) * batch;
    long long want = wgs / MT_WGS_PER_TILE;
    // mid-size launches (one to four rounds of one workgroup per CU, e.g. q/k/v at T = 1800: 684 workgroups): as many token tiles per
    // workgroup as there would be rounds, so that ONE round of <= 256 workgroups remains (configs[4]: 16.87k -> 17.34k frames/s)
    if (want <= 1) want = wgs / MT_MID_WGS;
    const int tt = (int)std::min<long long>(std::min<long long>(8, want), ntt);
    return (tt <= 1 || !ugemm_supports(a, epi, NB, KS, mode, tt)) ? 1 : tt;
}

// The decision of one UNet GEMM launch, from the schedule's (NB, KS) request; rules in this order: NB 3 -> 2 where NB = 3 is not built, the kconv NB = 1
// switch, tiles per workgroup (pick_tt), split-fp16 products, then bf16 -> fp32 -> the generic kernel.  Pure: same inputs, same plan.
inline GemmPlan plan_gemm(const PlanSwitches& sw, const GemmArgs& args, int epi, int batch, int NB, int KS) {
    GemmArgs a = args;
    a.kconv_off = (sw.kconv == 0) ? 1 : 0;
    const UMode m = sw.bf16 ? U_BF16 : U_F32;
    if (NB == 3 && epi == EPI_STORE && !ugemm_supports(a, epi, 3, KS, m)) NB = 2;   // (the two-segment fp32 shapes spill at NB = 3: not built)
    // K-long up-path convolutions (two / three K segments): the split-fp16 shapes exist for one column tile per workgroup only (kconv_body; with two the second accumulator
    // set spills).  Where that takes at most 1.5 x the rounds of the chosen shape on the fp32 matrix instructions it wins (a round of NB = 1 split ~11 us, of NB = 2 fp32 ~21 us:
    // configs[4] 24.3k -> 25.5k frames/s, 3 clips +6 %; 76 tiles — 2 rounds against 1 — loses 2 %: profiles/r06g_kconv_ab.txt)
    if (!sw.bf16 && epi == EPI_STORE && NB > 1 && a.nseg >= 2 && sw.kconv != 0 && sw.split && !a.step_inc && !sw.clk && (!sw.concurrent || sw.kconv == 2)) {   // (concurrent clip groups share the CUs: fewer workgroups win there — 5 clips -1.9 %; "kconv" = 2: there too)
        const long long tiles = (long long)batch * ((a.T + 31) / 32), r1 = (tiles * 6 + 255) / 256, rn = (tiles * (6 / NB) + 255) / 256;
        if (tiles <= KCONV_MAX_TILES && 2 * r1 <= 3 * rn && !ugemm_supports(a, epi, NB, KS, U_SP) && ugemm_supports(a, epi, 1, 8, U_SP)) { NB = 1; KS = 8; }
    }
    const int tt = pick_tt(a, epi, batch, NB, KS, m);
    GemmKernel k = GemmKernel::cgemm;
    if (tt > 1) k = sw.bf16 ? GemmKernel::ugemm_bf16 : GemmKernel::ugemm_f32;
    else if (!a.step_inc) {   // (the launch that advances the loop's step counter stays on the generic kernel)
        // fp32 mode, single-tile workgroups: split-fp16 products wherever the shape is built for them (gemm_lds.hip SP) and the weights carry the packing
        if (!sw.bf16 && sw.split && ugemm_supports(a, epi, NB, KS, U_SP)) k = GemmKernel::ugemm_sp;
        else if (sw.bf16 && ugemm_supports(a, epi, NB, KS, U_BF16)) k = GemmKernel::ugemm_bf16;
        else if (ugemm_supports(a, epi, NB, KS, U_F32)) k = GemmKernel::ugemm_f32;   // (bf16 mode too, where a segment has no Seg::w2)
    }
    return {NB, KS, tt, k};
}

}  // namespace host
}  // namespace said
