// unet_sched.cpp — the UNet1D launch schedules: the per-block ResBlock / SpatialTransformer launch sequences of every precision mode and
// batch size, time embedding, cross-attention K/V and the alignment band.  Every launch of run_unet goes through counted(); a channel-major
// GEMM (do_gemm) runs on whatever ugemm_plan.h's plan_gemm decides — the column-tile rules and the rule order are written there, once.
#include "engine_internal.h"
#include "ugemm_plan.h"

namespace said {
namespace host {

namespace {

constexpr float ATTN_SCALE = 0.17677669529663687f;   // dim_head ** -0.5 = 32 ** -0.5 (attention.py:101)
constexpr float LOG2E = 1.4426950408889634f;

}  // namespace

Seg mkseg(const float* x, long long bstride, int pitch, int C, int taps, int pad, int stride, int Tin, int xform, const float* w) {
    Seg s;
    memset(&s, 0, sizeof s);
    s.x = x; s.w = w; s.x_bstride = bstride; s.x_pitch = pitch; s.C = C; s.taps = taps; s.pad = pad; s.stride = stride;
    s.Tin = Tin; s.xform = xform; s.gn_cpg = 1; s.gn_nparts = 1;
    return s;
}

namespace {

inline Seg with_w4(Seg s, const float* w4, bool gn_tail = false, bool ln_tail = false) { s.w4 = w4; s.w4_gn_tail = gn_tail ? 1 : 0; s.w4_ln_tail = ln_tail ? 1 : 0; return s; }
// attach K-segment k of a packed weight: both packings for the LDS-staged kernel and what follows them
inline Seg with_pw(Seg s, const PW& pw, int k) {
    s.w4 = pw.w4[k]; s.w2 = pw.w2[k]; s.ws = pw.ws[k]; s.ws_flat = pw.ws_flat ? 1 : 0; s.w4_gn_tail = pw.gn_tail ? 1 : 0; s.w4_ln_tail = pw.ln_tail ? 1 : 0;
    return s;
}
void seg_gn(Seg& s, const float* part, long long part_bstride, int cpg, int nparts, float eps, const float* g, const float* b) {
    s.gn_part = part; s.gn_part_bstride = part_bstride; s.gn_cpg = cpg; s.gn_nparts = nparts; s.gn_eps = eps; s.gn_gamma = g; s.gn_beta = b;
}

}  // namespace

GemmArgs mkargs(int T, int N) {
    GemmArgs a;
    memset(&a, 0, sizeof a);
    a.T = T; a.N = N; a.groups = 1; a.ntiles_per_group = (N + 31) / 32;
    return a;
}

namespace {

// One counted launch of the schedule.  Every launch of run_unet takes exactly one number from dbg_count, in launch order: said_profile_unet replays number
// dbg_only alone, said_debug_stop_after issues the numbers below dbg_stop.  `log` adds the launch's stage_log entry (called only while logging), `launch` issues it
// (called only when its number is wanted); -DSAID_TRACE builds report the launch (fmt, args) before it and how it ended after it.  Returns whether it ran.
template <class Log, class Launch, class... A>
bool counted(said_ctx* c, hipStream_t s, Log&& log, Launch&& launch, const char* fmt, A... args) {
    if (c->log_on) log();
    const int k = c->dbg_count++;
    if (c->dbg_only >= 0 ? k != c->dbg_only : (c->dbg_stop >= 0 && k >= c->dbg_stop)) return false;
    if (trace_on()) { fprintf(stderr, "[said] #%d ", k); fprintf(stderr, fmt, args...); fputc('\n', stderr); fflush(stderr); }
    launch();
    if (trace_on()) { hipError_t e = hipStreamSynchronize(s); fprintf(stderr, "[said]   -> %s\n", hipGetErrorString(e)); fflush(stderr); }
    return true;
}
// (a helper launch that is not a node of the counted schedule: runs whenever the NEXT counted launch would)
inline bool dbg_go_peek(const said_ctx* c) { return c->dbg_only >= 0 ? c->dbg_count == c->dbg_only : (c->dbg_stop < 0 || c->dbg_count < c->dbg_stop); }

inline PlanSwitches plan_switches(const said_ctx* c) { return {c->bf16_mode, sp_on(c, c->ugemm_split), c->kconv, c->clk_on, c->cur_concurrent}; }

// One channel-major UNet GEMM: planned (ugemm_plan.h plan_gemm — the schedule's NB / KS are a request), logged, launched by the plan.
// returns true when the launch went to ugemm_kernel (gemm_lds.hip) — the only kernel that honours GemmCommon::gn_coef_out / kv_split
bool do_gemm(said_ctx* c, const GemmArgs& a, int epi, int batch, int NB, int KS, hipStream_t s) {
    const GemmPlan p = plan_gemm(plan_switches(c), a, epi, batch, NB, KS);
    GemmArgs a2 = a;
    a2.kconv_off = (c->kconv == 0) ? 1 : 0;
    if (c->clk_on && c->dbg_count < 64) a2.clk = c->clk_dev + (long long)c->dbg_count * 128;
    auto log = [&] {   // algorithmic HBM bytes / flops of the launch: weights + operands in + residual + result out
        double w = 0, in = 0, fl = 0;
        const double nout = (double)a.groups * a.N * (epi == EPI_GEGLU ? 2 : 1);
        for (int i = 0; i < a.nseg; ++i) {
            const Seg& sg = a.seg[i];
            w += nout * sg.C * sg.taps * 4.0;
            in += (double)batch * a.groups * sg.C * sg.Tin * 4.0;
            fl += 2.0 * batch * nout * sg.C * sg.taps * a.T;
        }
        double out = (double)batch * a.groups * a.N * a.T * 4.0;
        if (a.res_kind != RES_NONE) in += out;
        if (epi == EPI_BAND) in += 2.0 * batch * a.N * a.T * 4.0;  // this block's K and V rows
        c->stage_log.push_back({p.on_ugemm() ? 2 : 0, epi, p.NB, p.KS, w + in + out, fl});
    };
    auto launch = [&] {
        if (p.on_ugemm()) launch_ugemm(a2, epi, batch, p.NB, p.KS, s, p.mode(), p.tt);
        else if (epi == EPI_QKV && a2.kv_split) c->launch_err = "q/k/v GEMM asked for pre-split k / v but does not run on ugemm_kernel";
        else launch_gemm(a2, epi, batch, p.NB, p.KS, s);
    };
    return counted(c, s, log, launch, "gemm epi=%d NB=%d KS=%d T=%d N=%d batch=%d tt=%d kernel=%d", epi, p.NB, p.KS, a.T, a.N, batch, p.tt, (int)p.kernel) && p.on_ugemm();
}
void do_attn(said_ctx* c, const AttnArgs& a, int batch, int head_dim, int KS, hipStream_t s, bool presplit = false) {
    const double e = (double)batch * a.heads * head_dim * a.T;
    counted(c, s, [&] { c->stage_log.push_back({1, -1, head_dim / 32, KS, 4.0 * e * 4.0, 4.0 * e * a.T}); },
            [&] { launch_attn(a, batch, head_dim, KS, s, c->bf16_mode ? 1 : (sp_on(c, c->attn_split) ? (presplit ? 3 : 2) : 0)); },
            "attn D=%d KS=%d T=%d batch=%d", head_dim, KS, a.T, batch);
}
// battn_kernel (attn.hip): bf16 q / k / v as the token-major q/k/v projection leaves them (TGemmArgs::qkv_bf16)
void do_battn(said_ctx* c, const AttnArgs& a, int batch, hipStream_t s) {
    const double e = (double)batch * a.heads * HD * a.T;
    counted(c, s, [&] { c->stage_log.push_back({9, -1, 1, 1, 4.0 * e * 2.0, 4.0 * e * a.T}); }, [&] { launch_battn(a, batch, s); }, "battn T=%d batch=%d", a.T, batch);
}
// the self-attention of one block over q / k (QK) and v (VT) as every q/k/v projection leaves them; o_mode as AttnArgs has it
AttnArgs mk_attn(const said_ctx* c, const UGeo& g, float* o, long long o_bstride, int o_mode) {
    AttnArgs a;
    a.qk = c->QK; a.v = c->VT; a.o = o;
    a.v_bstride = (long long)MC * g.Tp; a.o_bstride = o_bstride; a.o_mode = o_mode;
    a.pitch = g.Tp; a.T = g.T; a.heads = HEADS; a.rows = rup(g.T, 32); a.b0 = 0;
    a.scale = ATTN_SCALE;
    return a;
}

inline int tm_seg(const UGeo& g) { return rup(g.T, 64); }   // sample pitch in tokens: a 64-row tile never straddles samples
// Sample ranges of one SpatialTransformer block.  shared: guidance-shared prefix (first transformer under classifier-free guidance): self-attention and
// everything before it run once per clip on samples [0, g.Bc).  With g.Bc > 0 the cross-attention (q projection, band softmax, to_out) runs on the
// conditional half only — the unconditional half attends to one repeated key/value, so its attn2 output is the per-channel constant c2[blk] and
// attn1's to_out emits its x2 = x1 + c2 directly.
struct StRange {
    int n1, n2;      // samples through self-attention / through cross-attention
    int x_off;       // first sample of the cross-attention range in the activations (X1, O): the conditional half, unless the prefix is
                     // shared (then X1 exists once per clip, in slots [0, Bc))
    int kv_off;      // ... in X2 and the K/V: always the conditional half's
    long long seg;   // sample pitch of the token-major activations (tm_seg)
    int vt_rows;     // padded T of the q / k rows
};
inline StRange st_range(const UGeo& g, bool shared) {
    return {shared ? g.Bc : g.Be, g.Bc > 0 ? g.Bc : g.Be, (g.Bc > 0 && !shared) ? g.Bc : 0, g.Bc > 0 ? g.Bc : 0, tm_seg(g), rup(g.T, 32)};
}
// cross-attention K (v = false) / V rows of block blk in the precomputed KV [sample][NST x (K | V) x 192][Sp], from sample kv_off on
inline long long kv_bs(const UGeo& g) { return (long long)NST * 2 * MC * g.Sp; }
inline const float* band_kv(const said_ctx* c, const UGeo& g, int blk, int kv_off, bool v) {
    return c->KV + (long long)(blk * 2 * MC + (v ? MC : 0)) * g.Sp + (long long)kv_off * kv_bs(g);
}
// the timestep-embedding term of ResBlock rb_index (GemmArgs and TGemmArgs spell the fields alike)
template <class Args> void set_emb(Args& a, const said_ctx* c, const UGeo& g, int rb_index) {
    a.emb = c->EO + (long long)rb_index * MC * c->maxNp; a.emb_pitch = c->maxNp; a.step_ptr = g.step_ptr; a.emb_b_stride = g.emb_b_stride;
}

// ---- fp32 / bf16: everything behind a block's self-attention as ONE launch (stchain.hip) ------------------------------------
// the fields both precisions share; the caller adds the output (y, y_bs) and what its kernel alone reads
ChainArgs mkchain(const said_ctx* c, const UGeo& g, const STW& sw, int blk, const ActBuf& in, const ActBuf& out, const float* wstream) {
    ChainArgs ca;
    memset(&ca, 0, sizeof ca);
    ca.wstream = wstream; ca.vec = sw.chain_vec;
    ca.xin_part = in.st; ca.part_bs = g.sts; ca.gn_gamma = sw.gn_g; ca.gn_beta = sw.gn_b;
    ca.kvt = c->KVT; ca.kvt_bs = (long long)g.S * (NST * 2 * MC); ca.lo = c->band_lo; ca.hi = c->band_hi;
    ca.stats_out = out.st; ca.stats_bs = g.sts;
    ca.S = g.S; ca.np = g.np; ca.koff = blk * 2 * MC; ca.wmax = c->band_wmax; ca.scale = ATTN_SCALE;
    return ca;
}
// o / xin: the attention output and the block input, sample strides o_bs / x_bs
void do_stchain(said_ctx* c, const UGeo& g, const StRange& r, ChainArgs ca, const void* o, const void* xin, long long o_bs, long long x_bs, bool shared, bool bf, hipStream_t s) {
    if ((bf ? c->xclk_on : c->clk_on) && c->dbg_count < 64) ca.clk = c->clk_dev + (long long)c->dbg_count * 128;   // (bf16: said_debug_option "xgemm_clk": -DSAID_CLK_STAMPS builds)
    auto log = [&] {
        const double eb = bf ? 2.0 : 4.0;   // element size of the weights and the activations (the K / V windows are fp32 in the log of both modes)
        const int n1 = r.n1, n2 = r.n2;
        const double w = eb * ((double)3 * MC * MC + 2.0 * FFI * MC + (double)(FFI + MC) * MC);
        const double io = eb * MC * g.T * ((double)n1 * 2 + g.Be) + 4.0 * 2 * MC * g.T * (double)n2;
        const double fl = 2.0 * g.T * ((double)n1 * MC * MC + (double)n2 * 2 * MC * MC + (double)g.Be * (2.0 * FFI * MC + (double)(FFI + MC) * MC)) + 4.0 * n2 * MC * g.T * c->band_wmax;
        c->stage_log.push_back({10, EPI_STORE, 6, 8, w + io, fl});
    };
    counted(c, s, log, [&] {
        launch_stchain(ca, static_cast<const float*>(o), static_cast<const float*>(xin), g.T, g.Tp, o_bs, x_bs, shared ? g.Bc : 0, g.Bc > 0 ? g.Bc : 0, g.Be, s, bf);
        ++c->n_stchain;
    }, "stchain T=%d samples=%d shared=%d", g.T, g.Be, (int)shared);
}

// ---- bf16 mode, large batches: UNet GEMMs on the token-major bf16 kernel (tgemm.hip) ------------------------------------
// The channel-major fp32 activations stay as they are between kernels (GroupNorm statistics, residuals, attention operands);
// what changes is the GEMM itself: a prep kernel applies the fused operand transform once and writes the operand token-major
// in bf16, and the GEMM runs as 128-token tiles on v_mfma_f32_32x32x16_bf16 without any split-K reduction.
bool use_tg(said_ctx* c, const UGeo& g, int nsamples) {
    // (the token-major kernels address their operands with 32-bit element offsets: beyond that the channel-major kernels run)
    const long long widest = ((long long)nsamples * rup(g.T + 2, 32) + 2) * FFI;
    if (c->band_wmax > 8) return false;   // wide alignment windows: the channel-major schedule (its generic band kernel)
    return !c->clk_on && widest < 0x7fffffffLL &&
           (long long)nsamples * g.T >= (c->bf16_mode ? c->unet_tgemm_min_tokens : (c->cur_concurrent ? std::min(c->unet_fgemm_min_tokens, c->unet_fgemm_min_concurrent) : c->unet_fgemm_min_tokens));
}
// weight of the token-major GEMM in the context's precision mode
inline const void* tw(const said_ctx* c, const void* bf, const void* f32) { return c->bf16_mode ? bf : f32; }
// conv_in_kernel (conv_in.hip): one result per clip, stored for its in_copies samples; tm: token-major bf16 (H0.t) instead of channel-major fp32 (H0.p)
void do_conv_in(said_ctx* c, const UGeo& g, int in_copies, bool tm, hipStream_t s) {
    counted(c, s, [&] {
        c->stage_log.push_back({11 /* conv_in_kernel */, EPI_STORE, 1, 4, 4.0 * ((double)MC * c->cin * 3 + (double)g.B_lat * c->cin * g.T + (double)g.Be * MC * g.T),
                                2.0 * g.B_lat * MC * c->cin * 3 * g.T});
    }, [&] {
        if (tm) launch_conv_in_tm(c->x_cm, c->conv_in.w4[0], c->conv_in.bias, c->H0.t, tm_seg(g), c->H0.st, g.step_inc, g.B_lat, in_copies, g.T, g.Tp, s);
        else launch_conv_in(c->x_cm, c->conv_in.w4[0], c->conv_in.bias, c->H0.p, c->H0.st, g.step_inc, g.B_lat, in_copies, g.T, g.Tp, MC, s);
    }, "conv_in T=%d clips=%d copies=%d tm=%d", g.T, g.B_lat, in_copies, (int)tm);
}
void do_prep(said_ctx* c, const PrepArgs& a, int batch, hipStream_t s) {
    PrepArgs a2 = a;
    a2.f32 = c->bf16_mode ? 0 : 1;
    if (!a2.f32) a2.pack = 0;
    counted(c, s, [&] { c->stage_log.push_back({5, -2, 0, 0, (double)batch * a.C * a.T * (4.0 + (c->bf16_mode ? 2.0 : 4.0)) * (a.dst2 ? 1.5 : 1.0), 0.0}); },
            [&] { if (!launch_prep(a2, batch, s)) c->launch_err = "operand preparation kernel: unsupported shape"; }, "prep mode=%d C=%d T=%d batch=%d", a.mode, a.C, a.T, batch);
}
void do_tgemm(said_ctx* c, const TGemmArgs& a, int batch, hipStream_t s) {
    TGemmArgs a2 = a;
    a2.f32 = c->bf16_mode ? 0 : 1;
    if (a2.f32 && a2.yb) { a2.yf = reinterpret_cast<float*>(a2.yb); a2.yb = nullptr; }   // token-major intermediate (GEGLU product) in fp32
    a2.f32_split = (a2.f32 && sp_on(c, c->gemm_split)) ? 1 : 0;
    if (!a2.f32_split) a2.f32_packed = 0;
    auto log = [&] {
        const double eb = c->bf16_mode ? 2.0 : 4.0;   // operand element size; KS = 32 marks the fp32 kernel (fgemm_kernel) in the log
        const double out_b = a.geglu ? a.N / 2 * eb : (a.y_cm ? 4.0 * a.N * (a.res_cm ? 2 : 1) : 4.0 * a.N);
        const int tile_n = c->bf16_mode ? (a.N % 128 == 0 ? 128 : 64) : ((a.N % 128 == 0 && (a.geglu || a.N % 96)) ? 128 : 96);
        c->stage_log.push_back({4, a.geglu ? EPI_GEGLU : (a.qk ? EPI_QKV : EPI_STORE), tile_n, c->bf16_mode ? 4 : 32,
                                eb * a.N * a.K + (double)batch * a.M * (eb * a.K + out_b), 2.0 * batch * (double)a.M * a.N * a.K});
    };
    counted(c, s, log, [&] {
        if (launch_tgemm(a2, batch, s)) return;
        char b[160]; snprintf(b, sizeof b, "token-major GEMM: shape M=%d N=%d K=%d (batch %d) is not served by any kernel", a.M, a.N, a.K, batch);
        c->launch_err = b;
    }, "tgemm M=%d N=%d K=%d batch=%d", a.M, a.N, a.K, batch);
}
// per-sample row pitch of the token-major operands: a multiple of 32 that holds the T tokens plus the two Conv1d padding rows, so
// that all samples form ONE row axis for the 256-row GEMM tiles (tgemm.h: seg_rows) and 32-row MFMA tiles never straddle samples
inline int tg_rows(const UGeo& g) { return rup(g.T + 2, 32); }
PrepArgs mkprep(const UGeo& g, const float* x, int mode, void* dst, long long dst_bs, int ldd, int coff) {
    PrepArgs p;
    memset(&p, 0, sizeof p);
    p.x = x; p.x_bs = g.hs; p.pitch = g.Tp; p.T = g.T; p.C = MC; p.mode = mode;
    p.dst = dst; p.dst_bs = dst_bs; p.ldd = ldd; p.coff = coff;
    return p;
}
// GroupNorm of the operand: its coefficients are finalised inside the preparation kernel from the producer's partials
void prep_gn(PrepArgs& p, const UGeo& g, const float* part, int cpg, float eps, const float* gamma, const float* beta) {
    p.part = part; p.part_bs = g.sts; p.gn_cpg = cpg; p.gn_nparts = g.np; p.gn_eps = eps; p.gn_gamma = gamma; p.gn_beta = beta;
}
TGemmArgs mktg(const UGeo& g, const void* a, int lda, const void* w, int N, int K) {
    TGemmArgs t;
    memset(&t, 0, sizeof t);
    t.a = a; t.a_bs = 0; t.lda = lda; t.w = w; t.M = g.T; t.N = N; t.K = K; t.seg_rows = tg_rows(g);
    return t;
}
void tg_cm_out(TGemmArgs& t, const UGeo& g, const ActBuf& out) {
    t.y_cm = out.p; t.cm_bs = g.hs; t.cm_pitch = g.Tp; t.stats = out.st; t.stats_bs = g.sts;
}

// ---- round 3, large batches: token-major activations between the kernels, operand transforms inside the GEMMs (xgemm_kernel) ----
// (32-bit element offsets inside the kernels: the widest token-major tensor here is the GEGLU product, sample pitch tm_seg — up to 4/3 of
// the rup(T + 2, 32) pitch use_tg's guard is written for)
inline bool use_tm(said_ctx* c, const UGeo& g) {
    return c->bf16_mode && c->tm_acts != 0 && use_tg(c, g, g.Be) && ((long long)g.Be * tm_seg(g) + 2) * FFI < 0x7fffffffLL;
}
// `rows` tokens further into a token-major tensor of row width `ld` (element size by precision mode)
inline void* tm_at(const said_ctx* c, void* base, long long rows, int ld) { return static_cast<char*>(base) + rows * ld * (c->bf16_mode ? 2 : 4); }
void do_xgemm(said_ctx* c, const TGemmArgs& a, int batch, hipStream_t s) {
    TGemmArgs a2 = a;
    a2.f32 = c->bf16_mode ? 0 : 1;
    if (c->xclk_on && c->dbg_count < 64) a2.clk = c->clk_dev + (long long)c->dbg_count * 128;
    if (a2.f32 && a2.yb) { a2.yf = reinterpret_cast<float*>(a2.yb); a2.yb = nullptr; }
    // kernel family: 7 = rgemm_kernel (round 4: register-stationary weights, helper waves), 6 = round 3's xgemm_kernel
    const int fam = (!a2.f32 && rgemm_supports(a2, batch)) ? 7 : 6;
    // a launch over a COLUMN RANGE of the packed weights (the split concatenated-input ResBlocks / folded proj_out probe only their first launch) is
    // something only rgemm_kernel understands: falling through to xgemm_kernel would silently multiply the wrong columns
    if (fam == 6 && (a2.w_k0 != 0 || (a2.w_ld != 0 && a2.w_ld != a2.K) || a2.w_seg != 0)) {
        c->launch_err = "token-major GEMM over a weight column range is not served by rgemm_kernel for this shape";
        return;
    }
    auto log = [&] {
        const double eb = c->bf16_mode ? 2.0 : 4.0;
        const double out_n = a.geglu ? a.N / 2 : a.N;
        const double out_b = a.y_cm ? 4.0 * out_n : (a.qk ? 4.0 * out_n : eb * out_n * (a.y2_tm ? 2 : 1));
        const double in_k = (a.ra[0] ? (a.ra[1] ? 384.0 : 192.0) : 0.0) + a.sk[0] + a.sk[1] + a.sk[2];   // source channels read per token (a conv reads its tile once)
        const double res_b = a.res_tm ? eb * a.N : 0.0;
        const double band_b = a.band_k ? 2.0 * 4.0 * a.N : 0.0;
        c->stage_log.push_back({fam, a.geglu ? EPI_GEGLU : (a.qk ? EPI_QKV : (a.band_k ? EPI_BAND : EPI_STORE)), a.N % 128 == 0 && (a.geglu || a.N % 96) ? 128 : 96, c->bf16_mode ? 4 : 32,
                                eb * a.N * a.K + (double)batch * a.M * (eb * in_k + out_b + res_b + band_b), 2.0 * batch * (double)a.M * a.N * a.K});
    };
    if (fam == 6) ++c->n_xgemm;   // (every xgemm launch of the schedule, issued or not; n_rgemm: the issued ones)
    counted(c, s, log, [&] {
        if (fam == 7) {
            if (!launch_rgemm(a2, batch, s)) c->launch_err = "rgemm_kernel refused a launch its own rgemm_supports() had accepted";
            ++c->n_rgemm;
        } else if (!launch_xgemm(a2, batch, s)) {
            char b[160]; snprintf(b, sizeof b, "token-major activation GEMM: shape M=%d N=%d K=%d (batch %d) is not served by any kernel", a.M, a.N, a.K, batch);
            c->launch_err = b;
        }
    }, "xgemm family=%d M=%d N=%d K=%d batch=%d", fam, a.M, a.N, a.K, batch);
}
TGemmArgs mkx(const UGeo& g, const void* w, int N, int K) {
    TGemmArgs t;
    memset(&t, 0, sizeof t);
    t.w = w; t.M = g.T; t.N = N; t.K = K; t.seg_rows = tm_seg(g);
    t.gn_part_bs = g.sts; t.gn_nparts = g.np; t.stats_bs = g.sts; t.ldy = MC; t.ldr_tm = MC;
    return t;
}
// a ResBlock convolution: GroupNorm (eps 1e-5, gamma / beta of src's channels) -> SiLU -> conv3 of `src` as the resident operand, 192 outputs
TGemmArgs mkx_conv3(const UGeo& g, const void* w, int K, const ActBuf& src, int cpg, const float* gamma, const float* beta) {
    TGemmArgs t = mkx(g, w, MC, K);
    t.ra[0] = src.t; t.rmode = 1; t.rtaps = 3;
    t.gn_part[0] = src.st; t.gn_cpg = cpg; t.gn_eps = 1e-5f; t.gn_gamma = gamma; t.gn_beta = beta;
    return t;
}
// in_layers of a concatenated-input ResBlock over ONE of its sources: input channels [off, off + 192), i.e. that range of every tap's weight columns
TGemmArgs res_in_range(const UGeo& g, const ResW& rw, const ActBuf& src, int off) {
    TGemmArgs t = mkx_conv3(g, rw.t_conv1, 3 * MC, src, rw.cin / 32, rw.g1 + off, rw.b1 + off);
    t.w_ld = 3 * rw.cin; t.w_k0 = off; t.w_seg = rw.cin;
    return t;
}
void run_resblock_tm(said_ctx* c, const UGeo& g, const ResW& rw, int rb_index, const ActBuf& in0, const ActBuf* in1, const ActBuf& out, hipStream_t s, bool shared) {
    const int nb = shared ? g.Bc : g.Be;
    // Round 4 (bf16 mode): a concatenated-input ResBlock (K = 1152 / 576 + 384) runs as launches of rgemm_kernel over COLUMN RANGES of the
    // same packed weights — its register-stationary weight fragments hold 576 columns per wave — with a bf16 partial sum in between (one extra
    // rounding of a quantity the next kernel rounds anyway): conv1 = [source 0 -> P] + [source 1 + bias + emb + P], and the 1x1 skip over
    // the raw input becomes the residual of conv2.  The partial / skip tensor lives in tX1 (idle until the block's SpatialTransformer).
    if (in1 && c->bf16_mode && rw.has_skip) {
        // in_layers, source 0: GN -> SiLU -> conv3 over the first 192 input channels -> P
        TGemmArgs p0 = res_in_range(g, rw, in0, 0);
        p0.y_tm = c->tX1;
        if (rgemm_supports(p0, nb)) {
            do_xgemm(c, p0, nb, s);
            {   // in_layers, source 1 (the skip connection's channels) + bias + emb term + P
                TGemmArgs t = res_in_range(g, rw, *in1, MC);
                t.bias = rw.conv1.bias;
                set_emb(t, c, g, rb_index);
                t.res_tm = c->tX1;
                t.y_tm = c->M.t; t.stats = c->M.st;
                do_xgemm(c, t, nb, s);
            }
            {   // skip_connection: Conv1d 1x1 over the concatenated raw input (openaimodel.py:194) -> tX1
                TGemmArgs t = mkx(g, rw.t_conv2, MC, 2 * MC);
                t.sa[0] = in0.t; t.sld[0] = MC; t.sk[0] = MC;
                t.sa[1] = in1->t; t.sld[1] = MC; t.sk[1] = MC;
                t.w_ld = 3 * MC + 2 * MC; t.w_k0 = 3 * MC;
                t.y_tm = c->tX1;
                do_xgemm(c, t, nb, s);
            }
            {   // out_layers: GN -> SiLU -> conv3 + (both biases) + skip(x)
                TGemmArgs t = mkx_conv3(g, rw.t_conv2, 3 * MC, c->M, 6, rw.g2, rw.b2);
                t.w_ld = 3 * MC + 2 * MC; t.w_k0 = 0;
                t.bias = rw.bias2;
                t.res_tm = c->tX1;
                t.y_tm = out.t; t.stats = out.st;
                do_xgemm(c, t, nb, s);
            }
            return;
        }
    }
    {   // in_layers: GN -> SiLU -> conv3 + emb term   (openaimodel.py:205-225)
        TGemmArgs t = mkx_conv3(g, tw(c, rw.t_conv1, rw.tf_conv1), 3 * rw.cin, in0, rw.cin / 32, rw.g1, rw.b1);
        if (in1) { t.ra[1] = in1->t; t.gn_part[1] = in1->st; }
        t.bias = rw.conv1.bias;
        set_emb(t, c, g, rb_index);
        t.y_tm = c->M.t; t.stats = c->M.st;
        do_xgemm(c, t, nb, s);
    }
    {   // out_layers: GN -> SiLU -> conv3 ; + skip(x)   (openaimodel.py:226-227)
        TGemmArgs t = mkx_conv3(g, tw(c, rw.t_conv2, rw.tf_conv2), 3 * MC + (rw.has_skip ? 2 * MC : 0), c->M, 6, rw.g2, rw.b2);
        if (rw.has_skip) {   // 1x1 conv over the concatenated raw input: two streamed K segments behind the resident one
            t.sa[0] = in0.t; t.sld[0] = MC; t.sk[0] = MC;
            t.sa[1] = in1->t; t.sld[1] = MC; t.sk[1] = MC;
            t.bias = rw.bias2;
        } else {
            t.bias = rw.conv2.bias;
            t.res_tm = in0.t;
        }
        t.y_tm = out.t; t.stats = out.st;
        if (shared) { t.y2_tm = out.t; t.y2_row_off = (long long)g.Bc * tm_seg(g); }
        do_xgemm(c, t, nb, s);
    }
}
// ---- the SpatialTransformer steps behind the self-attention on token-major activations (do_xgemm), shared by the two bf16 large-batch schedules ----
// q / k / v of a token-major GEMM in attn.hip's operand layout: q and k token-major into QK [Be][2*heads][rows][32], v channel-major into VT [Be][192][Tp]
void tg_qkv_out(TGemmArgs& t, const said_ctx* c, const UGeo& g, const StRange& r) {
    t.qk = c->QK; t.vt = c->VT; t.v_bs = (long long)MC * g.Tp; t.qk_n = 2 * MC; t.head_dim = HD; t.rows = r.vt_rows; t.heads2 = 2 * HEADS; t.v_pitch = g.Tp;
}
TGemmArgs tm_out1(said_ctx* c, const UGeo& g, const STW& sw, int blk, const ActBuf& in) {   // x1 = to_out(attn) + GroupNorm(x_in)   (attention.py:127, 168); under guidance also x2 of the unconditional half = x1 + c2
    TGemmArgs t = mkx(g, tw(c, sw.t_out1, sw.tf_out1), MC, MC);
    t.sa[0] = c->tO; t.sld[0] = MC; t.sk[0] = MC;
    t.bias = sw.out1.bias;
    t.res_tm = in.t; t.res_gn = 1; t.res_part = in.st; t.res_gamma = sw.gn_g; t.res_beta = sw.gn_b; t.res_eps = 1e-6f; t.gn_cpg = 6;
    t.y_tm = c->tX1;
    if (g.Bc > 0) { t.y2_tm = c->tX2; t.y2_row_off = 0; t.y2_add = c->c2[blk]; }
    return t;
}
TGemmArgs tm_q2_band(said_ctx* c, const UGeo& g, const STW& sw, int blk, const StRange& r) {   // attn2: q = to_q(norm2(x1)); banded softmax over the precomputed audio K/V   (attention.py:170-191)
    TGemmArgs t = mkx(g, tw(c, sw.t_q2, sw.tf_q2), MC, MC);
    t.ra[0] = tm_at(c, c->tX1, r.x_off * r.seg, MC); t.rmode = 2; t.rtaps = 1;
    t.ln_gamma = sw.l2g; t.ln_beta = sw.l2b;
    t.band_k = band_kv(c, g, blk, r.kv_off, false);
    t.band_v = band_kv(c, g, blk, r.kv_off, true);
    t.band_kv_bs = kv_bs(g); t.band_kv_pitch = g.Sp; t.band_lo = c->band_lo; t.band_hi = c->band_hi; t.band_wmax = c->band_wmax;
    t.band_scale = ATTN_SCALE;
    t.y_tm = tm_at(c, c->tO, r.x_off * r.seg, MC);
    return t;
}
TGemmArgs tm_out2(said_ctx* c, const UGeo& g, const STW& sw, const StRange& r) {   // x2 = to_out(attn2) + x1   (conditional half only under guidance: its rows are [Bc, 2 Bc) of X2)
    TGemmArgs t = mkx(g, tw(c, sw.t_out2, sw.tf_out2), MC, MC);
    t.sa[0] = tm_at(c, c->tO, r.x_off * r.seg, MC); t.sld[0] = MC; t.sk[0] = MC;
    t.bias = sw.out2.bias;
    t.res_tm = tm_at(c, c->tX1, r.x_off * r.seg, MC);
    t.y_tm = tm_at(c, c->tX2, r.kv_off * r.seg, MC);
    return t;
}
TGemmArgs tm_geglu(said_ctx* c, const UGeo& g, const STW& sw, const StRange& r) {   // GEGLU: proj(norm3(x2)) -> a * gelu(gate)   (attention.py:25-32): the GEMM normalises its operand itself
    TGemmArgs t = mkx(g, tw(c, sw.t_ff1, sw.tf_ff1), 2 * FFI, MC);
    t.ra[0] = c->tX2; t.rmode = 2; t.rtaps = 1;
    t.ln_gamma = sw.l3g; t.ln_beta = sw.l3b;
    t.bias = sw.t_ff1_bias; t.geglu = 1;
    t.yb = c->tF; t.y_bs = r.seg * FFI; t.ldy = FFI;
    return t;
}
// proj_out o ff.net.2 over [h ; x2] + x_in   (attention.py:193, 232-234); cm: channel-major fp32 + GroupNorm partials (for a channel-major
// ResBlock or out_sched_kernel), else token-major
TGemmArgs tm_proj_out(said_ctx* c, const UGeo& g, const STW& sw, const ActBuf& in, const ActBuf& out, bool cm) {
    TGemmArgs t = mkx(g, tw(c, sw.t_ffproj, sw.tf_ffproj), MC, FFI + MC);
    t.sa[0] = c->tF; t.sld[0] = FFI; t.sk[0] = FFI;
    t.sa[1] = c->tX2; t.sld[1] = MC; t.sk[1] = MC;
    t.bias = sw.ffproj.bias;
    t.res_tm = in.t;
    if (cm) { t.y_cm = out.p; t.cm_bs = g.hs; t.cm_pitch = g.Tp; t.stats = out.st; }
    else { t.y_tm = out.t; t.stats = out.st; }
    return t;
}
// attn1.to_out, attn2 (q + band), attn2.to_out, GEGLU, folded proj_out.  last: the result goes out channel-major
void run_tm_tail(said_ctx* c, const UGeo& g, const STW& sw, int blk, const ActBuf& in, const ActBuf& out, const StRange& r, hipStream_t s, bool last) {
    do_xgemm(c, tm_out1(c, g, sw, blk, in), r.n1, s);
    do_xgemm(c, tm_q2_band(c, g, sw, blk, r), r.n2, s);
    do_xgemm(c, tm_out2(c, g, sw, r), r.n2, s);
    do_xgemm(c, tm_geglu(c, g, sw, r), g.Be, s);
    if (!last && c->bf16_mode) {   // round 4: as two rgemm launches over column ranges of the folded weight (see run_resblock_tm)
        TGemmArgs h = mkx(g, sw.t_ffproj, MC, FFI);   // (P F2) h + x_in -> tX1 (x1 is dead by now)
        h.sa[0] = c->tF; h.sld[0] = FFI; h.sk[0] = FFI; h.w_ld = FFI + MC; h.w_k0 = 0;
        h.res_tm = in.t; h.y_tm = c->tX1;
        if (rgemm_supports(h, g.Be)) {
            do_xgemm(c, h, g.Be, s);
            TGemmArgs t = mkx(g, sw.t_ffproj, MC, MC);   // + P x2 + (P b2 + bp)
            t.sa[0] = c->tX2; t.sld[0] = MC; t.sk[0] = MC; t.w_ld = FFI + MC; t.w_k0 = FFI;
            t.bias = sw.ffproj.bias;
            t.res_tm = c->tX1; t.y_tm = out.t; t.stats = out.st;
            do_xgemm(c, t, g.Be, s);
            return;
        }
    }
    do_xgemm(c, tm_proj_out(c, g, sw, in, out, last), g.Be, s);
}

// last: this block feeds the `out` convolution, which reads channel-major fp32 + GroupNorm partials (out_sched.hip)
void run_transformer_tm(said_ctx* c, const UGeo& g, const STW& sw, int blk, const ActBuf& in, const ActBuf& out, hipStream_t s, bool shared, bool last) {
    const StRange r = st_range(g, shared);
    // softmax(q k^T * scale) v -> token-major   (attention.py:99-126)
    const AttnArgs at = mk_attn(c, g, static_cast<float*>(c->tO), r.seg, c->bf16_mode ? 2 : 1);
    bool battn = false;
    {   // x = norm(x); q, k, v = to_{q,k,v}(norm1(x)) into attn.hip's operand layout   (attention.py:227, 168, 93-97)
        TGemmArgs t = mkx(g, tw(c, sw.t_qkv, sw.tf_qkv), 3 * MC, MC);
        t.ra[0] = in.t; t.rmode = 3; t.rtaps = 1;
        t.gn_part[0] = in.st; t.gn_cpg = 6; t.gn_eps = 1e-6f; t.gn_gamma = sw.gn_g; t.gn_beta = sw.gn_b;
        t.ln_gamma = sw.l1g; t.ln_beta = sw.l1b;
        tg_qkv_out(t, c, g, r);
        // round 4 (bf16 mode, T <= 640): the projection writes bf16 q / k / v in battn_kernel's operand layout (attn.hip)
        t.qkv_bf16 = (c->bf16_mode && battn_supports(at, HD)) ? 1 : 0;
        if (t.qkv_bf16 && !rgemm_supports(t, r.n1)) t.qkv_bf16 = 0;
        battn = t.qkv_bf16 != 0;
        t.q_scale = ATTN_SCALE * LOG2E;
        do_xgemm(c, t, r.n1, s);
    }
    if (battn) do_battn(c, at, r.n1, s);
    else do_attn(c, at, r.n1, HD, -4, s);
    // round 5: everything behind the attention as ONE launch on bf16 operands (stchain_kernel<true>; the token-major bf16 tensors are its operands as they are)
    if (c->bf16_mode && c->st_chain_bf16 != 0 && !last && sw.chain_wb && sw.chain_vec && c->band_chain_ok && c->kvt_S == g.S && c->kvt_bf16 && g.S == c->band_S && g.T == c->band_T &&
        (long long)g.Be * r.seg * MC < 0x7fffffffLL) {
        ChainArgs ca = mkchain(c, g, sw, blk, in, out, static_cast<const float*>(sw.chain_wb));
        ca.y = static_cast<float*>(out.t); ca.y_bs = r.seg * MC;
        do_stchain(c, g, r, ca, c->tO, in.t, r.seg * MC, r.seg * MC, shared, true, s);
        return;
    }
    run_tm_tail(c, g, sw, blk, in, out, r, s, last);
}

// ---- round 3, bf16 mode at large batch when the token-major activations are off (tm_acts = 0, or beyond their 32-bit offsets): the HYBRID SpatialTransformer.  The ResBlocks and q/k/v keep round 2's kernels
// (channel-major fp32 between them, prep_kernel + token-major GEMM), everything from the attention output on runs on round 3's
// token-major-activation kernels, where they are faster in situ: attention writes token-major bf16, attn1.to_out / band / attn2.to_out /
// GEGLU / folded proj_out are xgemm launches (no second preparation kernel: GEGLU applies norm3 itself), and the folded proj_out writes
// channel-major fp32 + GroupNorm partials again for the next ResBlock.  The token-major copy of the block's input (the residual of
// attn1.to_out and of proj_out) is a by-product of the q/k/v operand preparation.  8 launches per block instead of 9.
void run_transformer_hybrid(said_ctx* c, const UGeo& g, const STW& sw, int blk, const ActBuf& in, const ActBuf& out, hipStream_t s, bool shared) {
    const StRange r = st_range(g, shared);
    {   // q, k, v on round 2's token-major GEMM; the preparation kernel also leaves the raw input token-major (in.t)
        PrepArgs p = mkprep(g, in.p, 1, c->uPL, (long long)tg_rows(g) * MC, MC, 0);
        prep_gn(p, g, in.st, 6, 1e-6f, sw.gn_g, sw.gn_b);
        p.ln_gamma = sw.l1g; p.ln_beta = sw.l1b;
        p.dst2 = in.t; p.dst2_bs = r.seg * MC; p.ldd2 = MC; p.coff2 = 0;
        do_prep(c, p, g.Be, s);   // (all samples: the second half's rows are the residual of proj_out)
        TGemmArgs t = mktg(g, c->uPL, MC, tw(c, sw.t_qkv, sw.tf_qkv), 3 * MC, MC);
        tg_qkv_out(t, c, g, r);
        do_tgemm(c, t, r.n1, s);
    }
    do_attn(c, mk_attn(c, g, static_cast<float*>(c->tO), r.seg, c->bf16_mode ? 2 : 1), r.n1, HD, -4, s);   // softmax(q k^T * scale) v -> token-major
    run_tm_tail(c, g, sw, blk, in, out, r, s, true);
}

// shared: guidance-shared prefix — only the first g.Bc samples are computed, and the result is ALSO written into the
// conditional half's slots (values only; its statistics are consumed by kernels that run on the first half alone)
void run_resblock(said_ctx* c, const UGeo& g, const ResW& rw, int rb_index, const ActBuf& in0, const ActBuf* in1, const ActBuf& out, hipStream_t s,
                  bool shared = false) {
    const int cpg = rw.cin / 32;
    const int nb = shared ? g.Bc : g.Be;
    const long long tt = (long long)nb * ((g.T + 31) / 32);
    if (use_tg(c, g, nb)) {
        const long long T2 = tg_rows(g);
        // fp32 mode: the operands reach fgemm_kernel already split (packed h | l pairs: prep_kernel's pack mode + the packed weight copies)
        const int pk = (!c->bf16_mode && sp_on(c, c->gemm_split) && c->gemm_presplit != 0 && rw.tp_conv1 && rw.tp_conv2) ? 1 : 0;
        {   // in_layers: GN -> SiLU -> conv3 + emb term   (openaimodel.py:205-225)
            for (int off = 0; off < (in1 ? 2 * MC : MC); off += MC) {   // one preparation launch per source: its channels [off, off + 192) of the operand
                const ActBuf& src = off ? *in1 : in0;
                PrepArgs p = mkprep(g, src.p, 0, c->uPA, T2 * rw.cin, rw.cin, off);
                p.pack = pk;
                prep_gn(p, g, src.st, cpg, 1e-5f, rw.g1 + off, rw.b1 + off);
                if (rw.has_skip) { p.dst2 = c->uPB; p.dst2_bs = T2 * 2 * MC; p.ldd2 = 2 * MC; p.coff2 = off; }   // raw copy for the 1x1 skip conv
                do_prep(c, p, nb, s);
            }
            TGemmArgs t = mktg(g, c->uPA, rw.cin, pk ? rw.tp_conv1 : tw(c, rw.t_conv1, rw.tf_conv1), MC, 3 * rw.cin);
            t.f32_packed = pk;
            t.bias = rw.conv1.bias;
            set_emb(t, c, g, rb_index);
            tg_cm_out(t, g, c->M);
            do_tgemm(c, t, nb, s);
        }
        {   // out_layers: GN -> SiLU -> conv3 ; + skip(x)   (openaimodel.py:226-227)
            PrepArgs p = mkprep(g, c->M.p, 0, c->uPA, T2 * MC, MC, 0);
            p.pack = pk;
            prep_gn(p, g, c->M.st, 6, 1e-5f, rw.g2, rw.b2);
            do_prep(c, p, nb, s);
            TGemmArgs t = mktg(g, c->uPA, MC, pk ? rw.tp_conv2 : tw(c, rw.t_conv2, rw.tf_conv2), MC, 3 * MC);
            t.f32_packed = pk;
            if (rw.has_skip) {   // 1x1 conv over the concatenated raw input as a second K segment
                // (the raw copies of the two inputs were written into uPB by the in_layers operand preparation above)
                t.a2 = c->uPB; t.a2_bs = 0; t.lda2 = 2 * MC; t.K1 = 3 * MC; t.K = 5 * MC;
                t.bias = rw.bias2;
            } else {
                t.bias = rw.conv2.bias;
                t.res_cm = in0.p; t.res_cm_bs = g.hs;
            }
            tg_cm_out(t, g, out);
            if (shared) { t.y2_cm = out.p + (long long)g.Bc * g.hs; t.y2_bs = g.hs; }
            do_tgemm(c, t, nb, s);
        }
        return;
    }
    {   // in_layers: GN -> SiLU -> conv3 ; + emb_layers(emb)   (openaimodel.py:205-225)
        GemmArgs a = mkargs(g.T, MC);
        a.nseg = in1 ? 2 : 1;
        for (int k = 0; k < a.nseg; ++k) {
            const ActBuf& src = k ? *in1 : in0;
            a.seg[k] = with_pw(mkseg(src.p, g.hs, g.Tp, MC, 3, 1, 1, g.T, XF_GN_SILU, rw.conv1.w[k]), rw.conv1, k);
            seg_gn(a.seg[k], src.st, g.sts, cpg, g.np, 1e-5f, rw.g1 + k * MC, rw.b1 + k * MC);
        }
        a.bias = rw.conv1.bias;
        set_emb(a, c, g, rb_index);
        a.y = c->M.p; a.y_bstride = g.hs; a.y_pitch = g.Tp;
        a.stats_out = c->M.st; a.stats_bstride = g.sts;
        do_gemm(c, a, EPI_STORE, nb, pick_unet_nb(tt), 8, s);
    }
    {   // out_layers: GN -> SiLU -> conv3 ; + skip(x)   (openaimodel.py:226-227)
        GemmArgs a = mkargs(g.T, MC);
        a.nseg = 1;
        a.seg[0] = with_pw(mkseg(c->M.p, g.hs, g.Tp, MC, 3, 1, 1, g.T, XF_GN_SILU, rw.conv2.w[0]), rw.conv2, 0);
        seg_gn(a.seg[0], c->M.st, g.sts, 6, g.np, 1e-5f, rw.g2, rw.b2);
        if (rw.has_skip) {  // 1x1 conv over the concatenated input folded in as two extra K segments
            a.seg[1] = with_pw(mkseg(in0.p, g.hs, g.Tp, MC, 1, 0, 1, g.T, XF_NONE, rw.skip.w[0]), rw.skip, 0);
            a.seg[2] = with_pw(mkseg(in1->p, g.hs, g.Tp, MC, 1, 0, 1, g.T, XF_NONE, rw.skip.w[1]), rw.skip, 1);
            a.nseg = 3;
            a.bias = rw.bias2;
        } else {
            a.bias = rw.conv2.bias;
            a.res_kind = RES_PLAIN; a.res = in0.p; a.res_bstride = g.hs; a.res_pitch = g.Tp;
        }
        a.y = out.p; a.y_bstride = g.hs; a.y_pitch = g.Tp;
        a.stats_out = out.st; a.stats_bstride = g.sts;
        if (shared) { a.y2 = out.p + (long long)g.Bc * g.hs; a.y2_bstride = g.hs; a.y2_add = nullptr; }
        do_gemm(c, a, EPI_STORE, nb, pick_unet_nb(tt), 8, s);
    }
}

// the channel-major schedule (shared: see StRange)
void run_transformer(said_ctx* c, const UGeo& g, const STW& sw, int blk, const ActBuf& in, const ActBuf& out, hipStream_t s,
                     bool shared = false) {
    const StRange r = st_range(g, shared);
    const int n1 = r.n1, n2 = r.n2, x_off = r.x_off, kv_off = r.kv_off;
    const long long tt1 = (long long)n1 * ((g.T + 31) / 32), tt2 = (long long)n2 * ((g.T + 31) / 32);
    const long long tt = (long long)g.Be * ((g.T + 31) / 32);
    const long long obs = 2LL * MC * g.Tp;   // batch stride of O (shared with QK so attention uses one stride)
    const bool tg = use_tg(c, g, n1);
    if (c->bf16_mode && tg && use_tg(c, g, g.Be)) { run_transformer_hybrid(c, g, sw, blk, in, out, s, shared); return; }
    // fp32 mode: attn1.to_out on the token-major fp32 GEMM too (the attention kernel writes its operand token-major into the free q/k/v
    // operand buffer; the GroupNorm'ed residual uses the coefficients the q/k/v preparation finalised): 59 -> ~30 us per launch at Be = 64
    // fp32 mode: everything behind the self-attention as ONE launch (stchain.hip) — at small batches beside the channel-major GEMMs, at large ones
    // beside the token-major GEMMs' q / k / v (the attention kernel then writes channel-major, as the small-batch schedule has it)
    const bool chain = !c->bf16_mode && sp_on(c, c->st_chain) && sw.chain_w && sw.chain_vec && c->band_chain_ok && c->kvt_S == g.S && !c->kvt_bf16 &&
                       g.S == c->band_S && g.T == c->band_T;
    const bool out1_tm = tg && !chain && !c->bf16_mode && tt1 * HEADS >= 2048 && sw.tf_out1;
    bool presplit = false;   // k and v stored as packed split-fp16 pairs for attn_kernel<PM = 3> (see below)
    bool coef_ready = false; // the q/k/v GEMM left the block input's GroupNorm coefficients in gn_coef (small-batch ugemm_kernel only)
    if (tg) {   // q, k, v on the bf16 token-major GEMM: operand = LayerNorm(GroupNorm(x)) prepared once
        const int pk = (!c->bf16_mode && sp_on(c, c->gemm_split) && c->gemm_presplit != 0 && sw.tp_qkv) ? 1 : 0;   // operands arrive split (see run_resblock)
        PrepArgs p = mkprep(g, in.p, 1, c->uPL, (long long)tg_rows(g) * MC, MC, 0);
        p.pack = pk;
        prep_gn(p, g, in.st, 6, 1e-6f, sw.gn_g, sw.gn_b);
        p.ln_gamma = sw.l1g; p.ln_beta = sw.l1b;
        if ((out1_tm || (chain && c->chain_coef != 0)) && p.part) { p.coef_out = c->gn_coef; p.coef_out_bs = 2 * MC; coef_ready = chain; }   // (the fp32 fused tail reads them too: round 6)
        do_prep(c, p, n1, s);
        TGemmArgs t = mktg(g, c->uPL, MC, pk ? sw.tp_qkv : tw(c, sw.t_qkv, sw.tf_qkv), 3 * MC, MC);
        t.f32_packed = pk;
        tg_qkv_out(t, c, g, r);
        // round 6: this GEMM's epilogue stores k and v pre-split too (as ugemm_kernel's does at small batch), for every attention shape that unpacks them: the
        // key-split ones and the four-query-tile one of large batches (each wave of which used to split all of K and V for itself)
        presplit = !c->bf16_mode && sp_on(c, c->attn_split) && c->attn_presplit != 0 && sp_on(c, c->gemm_split) &&
                   !c->clk_on;   // (then the attention shape below is -4, 8 or 4: all unpack)
        t.kv_pack = presplit ? 1 : 0;
        do_tgemm(c, t, n1, s);
    } else
    {   // x = norm(x) (GroupNorm eps 1e-6); q,k,v = to_{q,k,v}(norm1(x))   (attention.py:227, 168, 93-97)
        GemmArgs a = mkargs(g.T, 3 * MC);
        a.nseg = 1;
        a.seg[0] = with_pw(mkseg(in.p, g.hs, g.Tp, MC, 1, 0, 1, g.T, XF_GN_LN, sw.qkv.w[0]), sw.qkv, 0);
        seg_gn(a.seg[0], in.st, g.sts, 6, g.np, 1e-6f, sw.gn_g, sw.gn_b);
        a.seg[0].ln_gamma = sw.l1g; a.seg[0].ln_beta = sw.l1b; a.seg[0].ln_eps = 1e-5f;
        // q and k tiles (0..11) token-major into QK [Be][2*heads][rows][32]; v tiles channel-major into VT [Be][192][Tp]
        // (y is biased so that output channel n = 384 + c lands on row c)
        a.tm_tiles = 2 * MC / 32;
        a.vt = c->QK; a.vt_heads = 2 * HEADS; a.vt_dim = HD; a.vt_rows = r.vt_rows;
        a.y = c->VT - (long long)a.tm_tiles * 32 * g.Tp; a.y_bstride = (long long)MC * g.Tp; a.y_pitch = g.Tp;
        const int nb = qkv_nb(tt1);   // tiles per workgroup (ugemm_plan.h)
        // k and v pre-split for the key-split attention shapes (same rule as below), when this GEMM runs on ugemm_kernel (the only epilogue that packs): ask the plan
        const bool key_split = tt1 * HEADS < 2048;
        presplit = !c->bf16_mode && sp_on(c, c->attn_split) && c->attn_presplit != 0 && key_split && !c->clk_on &&
                   plan_gemm(plan_switches(c), a, EPI_QKV, n1, nb, 8).on_ugemm();
        a.kv_split = presplit ? 1 : 0;
        // round 6: this GEMM finalises the block input's GroupNorm coefficients anyway (its operand is LayerNorm(GroupNorm(x))): the first workgroup of every sample
        // leaves them for stchain_kernel, whose GroupNorm'ed residual then needs 2 loads per wave instead of 23 and no finalisation in front of its first barrier
        if (chain && c->chain_coef != 0 && c->gn_coef) { a.gn_coef_out = c->gn_coef; a.gn_coef_bs = 2 * MC; }
        coef_ready = do_gemm(c, a, EPI_QKV, n1, nb, 8, s) && a.gn_coef_out != nullptr;
    }
    bool out1_done = false;
    {   // softmax(q k^T * scale) v   (attention.py:99-126)
        AttnArgs a = mk_attn(c, g, c->O, obs, 0);
        // waves per workgroup = ways the key tiles are split: 8 only pays while a wave would otherwise hold a single
        // tile (T <= 256); from there 4 waves with ~5 tiles each merge half as many partial states (B=1: -0.5 % per step)
        // large batches: four query tiles per workgroup sharing each K / V tile through the CU's L1 (-4), see attn.hip
        int ks_run = tt1 * HEADS >= 2048 ? -4 : (g.T <= 256 ? 8 : 4);
        if (out1_tm && ks_run == -4) { a.o = static_cast<float*>(c->uPL); a.o_bstride = tg_rows(g); a.o_mode = 1; }
        // long sequences at small batch (configs[4]): three query tiles per wave share every K / V fragment (attn2q.hip; bit-identical) where a third of the
        // launch is most of ONE round of workgroups (101 KB of LDS, 264 registers: one workgroup per CU)
        if (presplit && ks_run == 4 && a.o_mode == 0 && (c->attn_2q > 0 || (c->attn_2q < 0 && tt1 * HEADS >= 512 && (long long)n1 * HEADS * ((((g.T + 31) / 32) + 2) / 3) <= 256))) ks_run = 34;   // (one round of one workgroup per CU)
        do_attn(c, a, n1, HD, ks_run, s, presplit && (ks_run == 4 || ks_run == 8 || ks_run == -4 || ks_run == 34));
        out1_done = a.o_mode == 1;
    }
    if (chain && !out1_done) {
        ChainArgs ca = mkchain(c, g, sw, blk, in, out, sw.chain_w);
        ca.y = out.p; ca.y_bs = g.hs;
        // small launches: three workgroups per token tile, each streaming a third of the GEGLU / folded proj_out weights (38 workgroups on 256 CUs were bound by
        // one CU's L2 port each: 2.36 MB per workgroup) — while the launch still is one round of the chip
        ca.slices = 1;
        if (c->st_chain_slices != 1 && sw.chain_w3 && sw.chain_w2) {
            if (tt <= CHAIN3_MAX_TILES && c->st_chain_slices != 2) ca.slices = 3;
            else if (tt <= CHAIN2_MAX_TILES) ca.slices = 2;
        }
        if (ca.slices > 1) { ca.wstream = ca.slices == 3 ? sw.chain_w3 : sw.chain_w2; ca.part = c->chain_part; ca.ticket = c->chain_ticket; }
        // the fp32 kernels read the block input's GroupNorm coefficients (round 6): left by the q/k/v GEMM (ugemm_kernel) or its operand preparation (prep_kernel), else made here
        if (!coef_ready && dbg_go_peek(c)) launch_gn_coef(in.st, g.sts, 6, g.np, g.T, 1e-6f, sw.gn_g, sw.gn_b, c->gn_coef, 2 * MC, n1, s);
        ca.gn_coef = c->gn_coef; ca.coef_bs = 2 * MC;
        do_stchain(c, g, r, ca, c->O, in.p, obs, g.hs, shared, false, s);
        return;
    }
    if (out1_done) {   // x1 = to_out(attn) + GroupNorm(x_in) on fgemm_kernel; under guidance also x2 of the unconditional half = x1 + c2
        TGemmArgs t = mktg(g, c->uPL, MC, sw.tf_out1, MC, MC);
        t.bias = sw.out1.bias;
        t.res_cm = in.p; t.res_cm_bs = g.hs; t.res_cm_coef = c->gn_coef; t.res_cm_coef_bs = 2 * MC;
        t.y_cm = c->X1; t.cm_bs = g.hs; t.cm_pitch = g.Tp;
        if (g.Bc > 0) { t.y2_cm = c->X2; t.y2_bs = g.hs; t.y2_add_cm = c->c2[blk]; }
        do_tgemm(c, t, n1, s);
    } else
    {   // x1 = to_out(attn) + x, with x = GroupNorm(in) recomputed on the fly   (attention.py:127, 168)
        GemmArgs a = mkargs(g.T, MC);
        a.nseg = 1;
        a.seg[0] = with_pw(mkseg(c->O, obs, g.Tp, MC, 1, 0, 1, g.T, XF_NONE, sw.out1.w[0]), sw.out1, 0);
        a.bias = sw.out1.bias;
        a.res_kind = RES_GN; a.res = in.p; a.res_bstride = g.hs; a.res_pitch = g.Tp;
        a.res_gn_part = in.st; a.res_gn_part_bstride = g.sts; a.res_gn_cpg = 6; a.res_gn_nparts = g.np; a.res_gn_eps = 1e-6f;
        a.res_gn_gamma = sw.gn_g; a.res_gn_beta = sw.gn_b;
        a.y = c->X1; a.y_bstride = g.hs; a.y_pitch = g.Tp;
        if (g.Bc > 0) {   // x2 of the unconditional half: x1 + const (written for every sample of this launch; the
                          // conditional slots — when this launch covers them — are overwritten by attn2's to_out below)
            a.y2 = c->X2; a.y2_bstride = g.hs; a.y2_add = c->c2[blk];
        }
        do_gemm(c, a, EPI_STORE, n1, 1, 8, s);   // the GroupNorm'ed-residual variant exists for NB = 1
    }
    {   // attn2: q = to_q(norm2(x1)); banded softmax over the precomputed audio K/V   (attention.py:170-191)
        GemmArgs a = mkargs(g.T, MC);
        a.nseg = 1;
        a.seg[0] = with_pw(mkseg(c->X1 + (long long)x_off * g.hs, g.hs, g.Tp, MC, 1, 0, 1, g.T, XF_LN, sw.q2.w[0]), sw.q2, 0);
        a.seg[0].ln_gamma = sw.l2g; a.seg[0].ln_beta = sw.l2b; a.seg[0].ln_eps = 1e-5f;
        a.y = c->O + (long long)x_off * obs; a.y_bstride = obs; a.y_pitch = g.Tp;
        a.band.k = band_kv(c, g, blk, kv_off, false);
        a.band.v = band_kv(c, g, blk, kv_off, true);
        a.band.kv_bstride = kv_bs(g); a.band.kv_pitch = g.Sp;
        a.band.lo = c->band_lo; a.band.hi = c->band_hi; a.band.wmax = c->band_wmax; a.band.scale = ATTN_SCALE;
        if (c->band_wmax > 8) {   // windows wider than the fused epilogue's eight keys (S >> T through SAID.forward): plain q projection, then the
                                  // generic band kernel in place (misc.hip; never on SAID.inference's path)
            const BandArgs bd = a.band;
            memset(&a.band, 0, sizeof a.band);
            do_gemm(c, a, EPI_STORE, n2, 1, 8, s);
            counted(c, s, [&] { c->stage_log.push_back({5, -2, 0, 0, 0.0, 0.0}); },
                    [&] { launch_band_wide(a.y, obs, g.Tp, bd.k, bd.v, bd.kv_bstride, bd.kv_pitch, bd.lo, bd.hi, g.T, HEADS, n2, bd.scale, s); }, "band_wide T=%d batch=%d", g.T, n2);
        } else
        do_gemm(c, a, EPI_BAND, n2, 1, 8, s);
    }
    {   // x2 = to_out(attn2) + x1   (conditional half only under guidance: its slots are [Bc, 2 Bc) of X2)
        GemmArgs a = mkargs(g.T, MC);
        a.nseg = 1;
        a.seg[0] = with_pw(mkseg(c->O + (long long)x_off * obs, obs, g.Tp, MC, 1, 0, 1, g.T, XF_NONE, sw.out2.w[0]), sw.out2, 0);
        a.bias = sw.out2.bias;
        a.res_kind = RES_PLAIN; a.res = c->X1 + (long long)x_off * g.hs; a.res_bstride = g.hs; a.res_pitch = g.Tp;
        a.y = c->X2 + (long long)kv_off * g.hs; a.y_bstride = g.hs; a.y_pitch = g.Tp;
        do_gemm(c, a, EPI_STORE, n2, pick_unet_nb(tt2), 8, s);
    }
    if (use_tg(c, g, g.Be)) {
        {   // GEGLU: operand norm3(x2) (and raw x2 for the folded proj_out), value/gate pairs multiplied in the epilogue
            const long long P = tg_rows(g);
            PrepArgs p = mkprep(g, c->X2, 2, c->uPL, P * MC, MC, 0);
            p.ln_gamma = sw.l3g; p.ln_beta = sw.l3b;
            p.dst2 = c->uPX; p.dst2_bs = P * MC; p.ldd2 = MC; p.coff2 = 0;
            do_prep(c, p, g.Be, s);
            TGemmArgs t = mktg(g, c->uPL, MC, tw(c, sw.t_ff1, sw.tf_ff1), 2 * FFI, MC);
            t.bias = sw.t_ff1_bias; t.geglu = 1;
            t.yb = c->uPH; t.y_bs = P * FFI; t.ldy = FFI;
            do_tgemm(c, t, g.Be, s);
        }
        {   // proj_out o ff.net.2 over [h ; x2] + x_in, channel-major result + GroupNorm partials
            TGemmArgs t = mktg(g, c->uPH, FFI, tw(c, sw.t_ffproj, sw.tf_ffproj), MC, FFI + MC);
            t.a2 = c->uPX; t.a2_bs = 0; t.lda2 = MC; t.K1 = FFI;
            t.bias = sw.ffproj.bias;
            t.res_cm = in.p; t.res_cm_bs = g.hs;
            tg_cm_out(t, g, out);
            do_tgemm(c, t, g.Be, s);
        }
        return;
    }
    {   // GEGLU: proj(norm3(x2)) -> a * gelu(gate)   (attention.py:25-32)
        GemmArgs a = mkargs(g.T, FFI);
        a.nseg = 1;
        a.seg[0] = with_pw(mkseg(c->X2, g.hs, g.Tp, MC, 1, 0, 1, g.T, XF_LN, sw.ff1.w[0]), sw.ff1, 0);
        a.seg[0].ln_gamma = sw.l3g; a.seg[0].ln_beta = sw.l3b; a.seg[0].ln_eps = 1e-5f;
        a.bias = sw.ff1.bias; a.geglu_gate_tiles = FFI / 32;
        a.y = c->F; a.y_bstride = (long long)FFI * g.Tp; a.y_pitch = g.Tp;
        do_gemm(c, a, EPI_GEGLU, g.Be, geglu_nb(tt), 8, s);
    }
    {
        // x3 = net.2(h) + x2 and out = proj_out(x3) + x_in as ONE GEMM over the K segments [h ; x2] with the host-folded
        // weights (P F2 | P) — both maps are per-token linear, so nothing but rounding order changes
        GemmArgs a = mkargs(g.T, MC);
        a.nseg = 2;
        a.seg[0] = with_pw(mkseg(c->F, (long long)FFI * g.Tp, g.Tp, FFI, 1, 0, 1, g.T, XF_NONE, sw.ffproj.w[0]), sw.ffproj, 0);
        a.seg[1] = with_pw(mkseg(c->X2, g.hs, g.Tp, MC, 1, 0, 1, g.T, XF_NONE, sw.ffproj.w[1]), sw.ffproj, 1);
        a.bias = sw.ffproj.bias;
        a.res_kind = RES_PLAIN; a.res = in.p; a.res_bstride = g.hs; a.res_pitch = g.Tp;
        a.y = out.p; a.y_bstride = g.hs; a.y_pitch = g.Tp;
        a.stats_out = out.st; a.stats_bstride = g.sts;
        do_gemm(c, a, EPI_STORE, g.Be, pick_unet_nb(tt), 8, s);
    }
}

}  // namespace

// UNetModel.forward (openaimodel.py:677-709): x_cm (latents) -> eps_cm.  Needs KV, band tables and EO ready.
void run_unet(said_ctx* c, const UGeo& g, hipStream_t s) {
    const long long tt = (long long)g.Be * ((g.T + 31) / 32);
    const int in_copies = (g.B_lat > 0 && g.Be % g.B_lat == 0) ? g.Be / g.B_lat : 0;   // samples sharing one clip's latents
    bool conv_in_tm = false;
    if (in_copies >= 1 && c->conv_in.w4[0] && !c->clk_on &&
        conv_in_supports(c->cin, MC, c->conv_in.taps, g.T, g.Tp, in_copies)) {
        // input_blocks.0: Conv1d(32 -> 192, k3), computed once per clip (conv_in.hip)
        // (large batches in bf16 mode: straight into the token-major bf16 layout the persistent GEMMs read — no channel-major copy, no transposition)
        conv_in_tm = c->bf16_mode && use_tm(c, g) && tm_seg(g) <= 0xffff;
        do_conv_in(c, g, in_copies, conv_in_tm, s);
    } else {   // input_blocks.0: Conv1d(32 -> 192, k3)
        GemmArgs a = mkargs(g.T, MC);
        a.nseg = 1;
        a.seg[0] = with_pw(mkseg(c->x_cm, (long long)c->cin * g.Tp, g.Tp, c->cin, 3, 1, 1, g.T, XF_NONE, c->conv_in.w[0]), c->conv_in, 0);
        a.seg[0].b_mod = g.B_lat;
        a.step_inc = g.step_inc;   // the loop's device step counter is advanced by the first kernel of the step
        a.bias = c->conv_in.bias;
        a.y = c->H0.p; a.y_bstride = g.hs; a.y_pitch = g.Tp; a.stats_out = c->H0.st; a.stats_bstride = g.sts;
        do_gemm(c, a, EPI_STORE, g.Be, pick_unet_nb(tt), 8, s);
    }
    const bool sh = g.Bc > 0;   // guidance-shared prefix: the two halves first differ at input_blocks.1.1's cross-attention
    // round 4: the loop's last kernel reads the token-major bf16 hidden state itself (out_sched.hip: out_sched_tm_kernel)
    OutSchedArgs osa_tm;
    bool out_tm = false;
    if (g.out_sched && c->out_tm != 0 && c->bf16_mode && use_tm(c, g) && c->bw_out) {
        osa_tm = *g.out_sched;
        osa_tm.x_tm = c->P.t; osa_tm.wb = c->bw_out; osa_tm.seg = tm_seg(g);
        out_tm = out_sched_tm_supports(osa_tm);
    }
    const bool tm = use_tm(c, g);
    if (tm && !conv_in_tm) {   // conv_in's result (channel-major fp32 + GroupNorm partials) -> token-major, raw
        PrepArgs p = mkprep(g, c->H0.p, 3, c->H0.t, (long long)tm_seg(g) * MC, MC, 0);
        do_prep(c, p, g.Be, s);
    }
    auto res = [&](int i, const ActBuf& in0, const ActBuf* in1, const ActBuf& out, bool shared = false) {
        if (tm) run_resblock_tm(c, g, c->res[i], i, in0, in1, out, s, shared);
        else run_resblock(c, g, c->res[i], i, in0, in1, out, s, shared);
    };
    // last: -> channel-major for out_sched_kernel unless out_tm
    auto st = [&](int i, const ActBuf& in, const ActBuf& out, bool shared = false, bool last = false) {
        if (tm) run_transformer_tm(c, g, c->st[i], i, in, out, s, shared, last && !out_tm);
        else run_transformer(c, g, c->st[i], i, in, out, s, shared);
    };
    res(0, c->H0, nullptr, c->P, sh);    // input_blocks.1.0
    st(0, c->P, c->H1, sh);              // input_blocks.1.1   (hs: H0, H1)
    res(1, c->H1, nullptr, c->P);        // middle_block.0
    st(1, c->P, c->Q);                   // middle_block.1
    res(2, c->Q, nullptr, c->P);         // middle_block.2
    res(3, c->P, &c->H1, c->Q);          // output_blocks.0.0  cat([h, H1])
    st(2, c->Q, c->P);                   // output_blocks.0.1
    res(4, c->P, &c->H0, c->Q);          // output_blocks.1.0  cat([h, H0])
    st(3, c->Q, c->P, false, true);      // output_blocks.1.1
    if (g.out_sched) {   // out conv + guidance + DDIM update in one kernel (out_sched.hip)
        counted(c, s, [] {} /* (the loop is never logged) */, [&] {
            if (out_tm) { launch_out_sched_tm(osa_tm, s); ++c->n_out_sched_tm; }
            else { launch_out_sched(*g.out_sched, s); ++c->n_out_sched; }
        }, "out_sched tm=%d", (int)out_tm);
    } else {   // out: GN -> SiLU -> Conv1d(192 -> 32, k3)
        GemmArgs a = mkargs(g.T, c->cin);
        a.nseg = 1;
        a.seg[0] = with_pw(mkseg(c->P.p, g.hs, g.Tp, MC, 3, 1, 1, g.T, XF_GN_SILU, c->conv_out.w[0]), c->conv_out, 0);
        seg_gn(a.seg[0], c->P.st, g.sts, 6, g.np, 1e-5f, c->out_g, c->out_b);
        a.bias = c->conv_out.bias;
        a.y = c->eps_cm; a.y_bstride = (long long)c->cin * g.Tp; a.y_pitch = g.Tp;
        do_gemm(c, a, EPI_STORE, g.Be, 1, 8, s);
        if (c->log_on && !c->stage_log.empty()) c->stage_log.back().kind = 12;   // the `out` convolution alone (forward(), profiling): in the loop it is out_sched_kernel's first half
    }
}

// time_embed + the five emb_layers for `n` timesteps already in ts_dev -> EO [5*192][Np]
void run_time_embed(said_ctx* c, int n, hipStream_t s) {
    const int Np = c->maxNp;
    launch_timestep_embedding(c->ts_dev, c->freqs, c->E0, n, MC, Np, s);
    const long long tt = (n + 31) / 32;
    // y [N][Np] = act(W xform(x) + b) over the n columns
    auto linear = [&](const float* x, int K, int xform, const PW& pw, int N, int act, float* y) {
        GemmArgs a = mkargs(n, N);
        a.nseg = 1;
        a.seg[0] = with_pw(mkseg(x, 0, Np, K, 1, 0, 1, n, xform, pw.w[0]), pw, 0);
        a.bias = pw.bias; a.act = act;
        a.y = y; a.y_pitch = Np;
        const LaunchCfg lc = pick_cfg(tt, N / 32);
        launch_gemm(a, EPI_STORE, 1, lc.NB, lc.KS, s);
    };
    linear(c->E0, MC, XF_NONE, c->te1, TE, ACT_SILU, c->E1);
    linear(c->E1, TE, XF_NONE, c->te2, TE, ACT_NONE, c->E2);
    linear(c->E2, TE, XF_SILU, c->emb_all, NRES * MC, ACT_NONE, c->EO);
}

// cross-attention K/V of all four transformer blocks from the channel-major context (step-invariant)
// for samples [b0, b0 + nb): under guidance with the shared schedule only the conditional half's are ever read
void run_kv(said_ctx* c, int b0, int nb, int S, int Sp, hipStream_t s) {
    GemmArgs a = mkargs(S, NST * 2 * MC);
    a.nseg = 1;
    const long long cbs = (long long)c->ctx_dim * Sp, ybs = (long long)NST * 2 * MC * Sp;
    a.seg[0] = with_pw(mkseg(c->CTX + b0 * cbs, cbs, Sp, c->ctx_dim, 1, 0, 1, S, XF_NONE, c->kv_all.w[0]), c->kv_all, 0);
    a.y = c->KV + b0 * ybs; a.y_bstride = ybs; a.y_pitch = Sp;
    const LaunchCfg lc = pick_cfg((long long)nb * ((S + 31) / 32), NST * 2 * MC / 32);
    launch_gemm(a, EPI_STORE, nb, lc.NB, lc.KS, s);
    // the key-major copy the fused SpatialTransformer tail reads its window tiles from (once per loop; fp32 mode's small-batch schedule only)
    c->kvt_S = -1;
    if ((c->bf16_mode ? c->st_chain_bf16 != 0 : sp_on(c, c->st_chain)) && (long long)S * NST * 2 * MC <= (long long)NST * 2 * MC * c->maxTp)
    {
        c->kvt_S = S; c->kvt_bf16 = c->bf16_mode ? 1 : 0;
        // (bf16 mode: the copy itself is bf16 — the kernels round the window tiles to bf16 anyway, and at 32 clips the windows are 64 of a launch's 117 MB of HBM traffic in fp32)
        if (c->bf16_mode) launch_cm_to_tm_bf16(c->KV + b0 * ybs, ybs, Sp, reinterpret_cast<unsigned short*>(c->KVT) + (long long)b0 * S * (NST * 2 * MC), (long long)S * (NST * 2 * MC), nb, S, NST * 2 * MC, s);
        else launch_cm_to_tm(c->KV + b0 * ybs, c->KVT + (long long)b0 * S * (NST * 2 * MC), nb, S, NST * 2 * MC, Sp, ybs, s);
    }
}

// alignment band of ldm/attention.py:170-189 with Python's banker's rounding on doubles
int set_band(said_ctx* ctx, int T, int S, hipStream_t s) {
    if (ctx->band_T == T && ctx->band_S == S) return 0;
    std::vector<int> lo(T), hi(T);
    const double ratio = (double)S / (double)T, kh = ratio / 2 + 1;
    int wmax = 0;
    for (int i = 0; i < T; ++i) {
        const double mid = (i + 0.5) * ratio;
        const int a = std::max((int)std::nearbyint(mid - kh), 0);
        const int b = std::min((int)std::nearbyint(mid + kh), S);
        lo[i] = a; hi[i] = b;
        wmax = std::max(wmax, b - a);
        if (b <= a) return fail(ctx, "empty alignment window at query %d (T=%d, S=%d)", i, T, S);
    }
    // work queued earlier on the caller's stream may still read the previous tables: drain it before they change
    // (only happens when the clip length changes)
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipMemcpy(ctx->band_lo, lo.data(), T * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(ctx->band_hi, hi.data(), T * sizeof(int), hipMemcpyHostToDevice));
    ctx->band_T = T; ctx->band_S = S; ctx->band_wmax = wmax;
    {   // stchain.hip keeps the windows of a 32-token tile as CHAIN_KW key rows starting at lo[first token]: needs a non-decreasing band of that span
        bool ok = wmax <= 8;
        for (int i = 1; i < T && ok; ++i) ok = lo[i] >= lo[i - 1];
        for (int t0 = 0; t0 < T && ok; t0 += 32) {
            int hmax = 0;
            for (int i = t0; i < std::min(T, t0 + 32); ++i) hmax = std::max(hmax, hi[i]);
            ok = hmax - lo[t0] <= CHAIN_KW;
        }
        ctx->band_chain_ok = ok;
    }
    return 0;
}

UGeo make_geo(said_ctx* c, int Be, int B_lat, int T, int S) {
    UGeo g;
    g.Be = Be; g.B_lat = B_lat; g.T = T; g.Tp = rup(T, 32); g.np = (T + 31) / 32; g.S = S; g.Sp = rup(S, 32);
    g.hs = (long long)MC * g.Tp; g.sts = (long long)MC * g.np * 2;
    g.step_ptr = nullptr; g.emb_b_stride = 0; g.step_inc = nullptr; g.out_sched = nullptr; g.Bc = 0;
    return g;
}

}  // namespace host
}  // namespace said
