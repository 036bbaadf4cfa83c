// rgemm_plan.h — the host-side decisions of rgemm_kernel (rgemm.hip), host-only: which launches it serves (rg_plan), the template instantiation of a served
// launch (RG_VARIANTS, rg_variant), and the persistent tile walk's geometry — row tiles per range (`per`), workgroups (`grid`), column groups.  A header of its own
// so that tests can ask it without a GPU (tests/rgemm_plan_main.cpp), as ugemm_plan.h is for the channel-major GEMMs.
#pragma once
#include <algorithm>

#include "tgemm.h"

namespace said {

struct RgPlan { int ntap, ek, mode, res, dup, stats, nch, per, grid, groups; };
inline bool rg_plan(const TGemmArgs& a, RgPlan& p) {
    if (a.f32 || a.seg_rows <= 0 || a.seg_rows % 32 || a.M < 1 || a.M > a.seg_rows) return false;
    if (a.ra[1] || a.sk[2] || a.y_cm) return false;
    p.nch = 1;
    if (a.ra[0]) {
        if (a.sk[0] || a.sk[1] || (a.rtaps != 1 && a.rtaps != 3) || a.K != a.rtaps * 192) return false;
        if (a.rmode < 1 || a.rmode > 3) return false;
        if ((a.rmode == 1 || a.rmode == 3) && (!a.gn_part[0] || !a.gn_gamma || !a.gn_beta || a.res_gn)) return false;
        if (a.rmode >= 2 && (!a.ln_gamma || !a.ln_beta || a.rtaps != 1)) return false;
        p.ntap = a.rtaps; p.mode = a.rmode;
    } else {
        if (!a.sa[0]) return false;
        if (a.sk[0] == 768) { if (a.sld[0] != 768 || a.sk[1] || a.K != 768) return false; p.nch = 4; }
        else if (a.sk[0] != 192 || a.sld[0] != 192) return false;
        else if (a.sk[1]) { if (a.sk[1] != 192 || a.sld[1] != 192 || !a.sa[1] || a.K != 384) return false; p.nch = 2; }
        else if (a.K != 192) return false;
        p.ntap = 1; p.mode = 0;
    }
    p.res = 0; p.dup = 0; p.stats = 0; p.groups = 1;
    if (a.geglu) {
        if (a.N % 384 || a.N / 384 > 32 || !a.yb || a.ldy % 8 || !a.ra[0] || p.ntap != 1 || a.band_k || a.qk) return false;
        if ((long long)a.batch * a.seg_rows * a.ldy * 2 > 0x7ffffff0LL) return false;
        p.ek = 2; p.groups = a.N / 384;
    } else if (a.band_k) {
        if (a.N != 192 || !a.ra[0] || !a.y_tm || !a.band_lo || !a.band_hi || a.band_wmax < 1 || a.band_wmax > 8 || p.ntap != 1) return false;
        p.ek = 4;
    } else if (a.qk) {
        if (a.N != 576 || a.qk_n != 384 || a.head_dim != 32 || a.heads2 != 12 || !a.vt || p.ntap != 1) return false;
        p.ek = 1;
    } else if (a.y_tm) {
        if (a.N != 192 || a.ldy != 192 || (a.res_tm && a.ldr_tm != 192)) return false;
        if (a.res_gn && (!a.res_tm || !a.res_part || !a.res_gamma || !a.res_beta)) return false;
        p.ek = 0;
        p.res = a.res_tm ? (a.res_gn ? 2 : 1) : 0;
        p.dup = a.y2_tm ? 1 : 0;
        p.stats = a.stats ? 1 : 0;
    } else return false;
    if ((long long)a.batch * a.seg_rows * (p.nch == 4 ? 768 : 192) * 2 > 0x7ffffff0LL) return false;   // 32-bit byte offsets into the activation tensors
    if (a.qk) {   // ... and into the q / k / v outputs: the fp32 q / k layout is 1536 B per token, four times the bf16 activations' 384
        const long long el = a.qkv_bf16 ? 2 : 4;
        if ((long long)a.batch * a.heads2 * a.rows * 32 * el > 0x7ffffff0LL) return false;
        if ((long long)a.batch * a.v_bs * el > 0x7ffffff0LL) return false;
    }
    const int total = a.batch * ((a.M + 31) / 32);
    const int wpg = std::max(8, 256 / p.groups / 8 * 8);          // workgroups per column group: one workgroup per CU in all
    p.per = (total + wpg - 1) / wpg;
    const int ranges = (total + p.per - 1) / p.per;
    p.grid = 8 * p.groups * ((ranges + 7) / 8);
    return true;
}
// the instantiations the UNet schedule needs (engine.cpp: run_resblock_tm, run_transformer_tm)
#define RG_VARIANTS(X)                                                                                     \
    X(3, 0, 1, 0, false, true, 1)   /* conv1: silu(GN(x)) -> conv3 + emb, statistics                       */ \
    X(3, 0, 1, 1, false, true, 1)   /* conv2 + identity skip                                              */ \
    X(3, 0, 1, 1, true, true, 1)    /* ... written to both guidance halves                                 */ \
    X(1, 0, 0, 2, false, false, 1)  /* attn1.to_out + GroupNorm(x_in)                                      */ \
    X(1, 0, 0, 2, true, false, 1)   /* ... + the unconditional half's x2 = x1 + c2                         */ \
    X(1, 0, 0, 1, false, false, 1)  /* attn2.to_out + x1                                                   */ \
    X(1, 1, 3, 0, false, false, 1)  /* q/k/v of LayerNorm(GroupNorm(x))                                    */ \
    X(1, 4, 2, 0, false, false, 1)  /* q of LayerNorm(x1) + banded cross-attention                         */ \
    X(1, 2, 2, 0, false, false, 1)  /* GEGLU of LayerNorm(x2): four column groups of six (value, gate) pairs */ \
    X(3, 0, 1, 0, false, false, 1)  /* one source of a concatenated-input convolution -> partial sum        */ \
    X(1, 0, 0, 0, false, false, 2)  /* 1x1 skip convolution over the concatenated raw input (two chunks)    */ \
    X(1, 0, 0, 1, false, false, 4)  /* folded proj_out o ff.net.2, the GEGLU product's 768 columns + x_in -> partial sum */ \
    X(1, 0, 0, 1, false, true, 1)   /* ... x2's 192 columns + bias + the partial sum, statistics            */
inline int rg_variant(const RgPlan& p) {
    int i = 0;
#define X(NT_, EK_, MO_, RE_, DU_, ST_, NC_) if (p.ntap == NT_ && p.ek == EK_ && p.mode == MO_ && p.res == RE_ && (p.dup != 0) == DU_ && (p.stats != 0) == ST_ && p.nch == NC_) return i; ++i;
    RG_VARIANTS(X)
#undef X
    return -1;
}

}  // namespace said
