// ugemm_plan_main — said_amd/csrc/ugemm_plan.h behind a command line for tests/test_ugemm_plan_cpu.py: the plan of every GEMM the channel-major UNet schedule issues
// (the GemmArgs of run_resblock, run_transformer and run_unet in unet_sched.cpp, with the packings weights.cpp gives each weight), over every setting of the
// switches plan_gemm reads and every batch size of a scan.  No device is touched; the table here has no kernels attached.
//   (no arguments)  -> one line per (case, T, distinct result): `case T=<T> <switch codes> : b<first batch>=<plan> ...`, a plan printed where it changes along the scan.
//                      switch code: f|b (fp32 | bf16 mode), ugemm_split, kconv, concurrent, clk.  plan: kernel/NB/KS/tt, for q/k/v also /p<run_transformer's old presplit term>
//   rows            -> checks that every split-fp16 and multi-tile row of the table is also a base row; prints the row counts
//   plan <batch> <T> [<split>] -> one line per case at that batch and frame count with fp32 mode's default switches (ugemm_split on, kconv -1, no clip groups, no
//                      clocks), or with ugemm_split as given (0: what strict fp32 plans with): `case kernel/NB/KS/tt body`, body = kconv for launches that run
//                      kconv_body, else block
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#define SAID_UGEMM_ROW_FNS(NB, KS, EPI, VAR, BF, MT, SP) nullptr, nullptr
#include "ugemm_plan.h"

using namespace said;
using namespace said::host;

#ifdef SAID_UGEMM_ROWS
static const URow kRows[] = {SAID_UGEMM_ROWS};
const URow* said::ugemm_row(int epi, int NB, int KS, int var, UMode mode, bool mt) {
    for (const URow& r : kRows)
        if (r.epi == epi && r.NB == NB && r.KS == KS && r.var == var && r.mode == mode && r.mt == mt) return &r;
    return nullptr;
}
static int check_rows() {
    int n[3] = {0, 0, 0}, bad = 0;
    for (const URow& r : kRows) {
        const int list = r.mt ? 2 : (r.mode == U_SP ? 1 : 0);
        ++n[list];
        if (list && !(ugemm_row(r.epi, r.NB, r.KS, r.var, U_F32, false) && ugemm_row(r.epi, r.NB, r.KS, r.var, U_BF16, false))) {
            printf("row epi=%d NB=%d KS=%d var=%d mode=%d mt=%d has no base row\n", r.epi, r.NB, r.KS, r.var, (int)r.mode, (int)r.mt);
            ++bad;
        }
        if (r.kconv != is_kconv_shape(r.mode == U_SP, r.mt, r.NB, r.KS, r.epi, r.var)) ++bad;
    }
    printf("rows base=%d split=%d multi_tile=%d bad=%d\n", n[0], n[1], n[2], bad);
    return bad ? 1 : 0;
}
#endif

namespace {

constexpr int MC = 192, FFI = 768, HD = 32, HEADS = 6, CIN = 32;
float mem[4];   // every pointer the plan only tests for null
int counter[1];

enum Pack { PK_PLAIN /* make_pw: w, w4, w2 */, PK_BLOCK /* + ws */, PK_FLAT /* + ws in the flat step layout */ };
Seg seg(int C, int taps, int T, int xform, Pack pk, bool gn_tail = false, bool ln_tail = false) {
    Seg s;
    memset(&s, 0, sizeof s);
    s.x = s.w = s.w4 = s.w2 = mem;
    if (pk != PK_PLAIN && C % 192 == 0) s.ws = mem;
    s.ws_flat = pk == PK_FLAT;
    s.w4_gn_tail = gn_tail; s.w4_ln_tail = ln_tail;
    s.x_pitch = (T + 31) / 32 * 32; s.x_bstride = (long long)C * s.x_pitch; s.C = C; s.taps = taps; s.pad = (taps - 1) / 2; s.stride = 1;
    s.Tin = T; s.xform = xform; s.gn_cpg = 1; s.gn_nparts = 1;
    if (xform == XF_LN || xform == XF_GN_LN) { s.ln_gamma = s.ln_beta = mem; s.ln_eps = 1e-5f; }
    return s;
}
void gn(Seg& s, int T, int cpg, float eps) {
    s.gn_part = s.gn_gamma = s.gn_beta = mem; s.gn_cpg = cpg; s.gn_nparts = (T + 31) / 32; s.gn_eps = eps; s.gn_part_bstride = (long long)MC * s.gn_nparts * 2;
}
GemmArgs args(int T, int N) {
    GemmArgs a;
    memset(&a, 0, sizeof a);
    a.T = T; a.N = N; a.groups = 1; a.ntiles_per_group = (N + 31) / 32;
    a.y = mem; a.y_pitch = (T + 31) / 32 * 32; a.y_bstride = (long long)N * a.y_pitch;
    return a;
}
void res_plain(GemmArgs& a) { a.res_kind = RES_PLAIN; a.res = mem; a.res_bstride = a.y_bstride; a.res_pitch = a.y_pitch; }

struct Case {
    const char* name;
    int epi;
    GemmArgs (*make)(int T, int batch);
    int (*nb)(long long tiles);   // the schedule's request (KS = 8 everywhere)
};
int nb_one(long long) { return 1; }
int nb_unet(long long t) { return pick_unet_nb(t); }
int nb_qkv(long long t) { return qkv_nb(t); }
int nb_geglu(long long t) { return geglu_nb(t); }

template <bool STEP> GemmArgs conv_in(int T, int batch) {
    GemmArgs a = args(T, MC);
    a.nseg = 1;
    a.seg[0] = seg(CIN, 3, T, XF_NONE, PK_PLAIN);
    a.seg[0].b_mod = batch;
    if (STEP) a.step_inc = counter;
    a.bias = mem; a.stats_out = mem;
    return a;
}
template <int NSEG> GemmArgs in_layers(int T, int) {
    GemmArgs a = args(T, MC);
    a.nseg = NSEG;
    for (int k = 0; k < NSEG; ++k) {
        a.seg[k] = seg(MC, 3, T, XF_GN_SILU, PK_BLOCK, true);
        gn(a.seg[k], T, NSEG * MC / 32, 1e-5f);
    }
    a.bias = mem; a.emb = mem; a.emb_pitch = 64; a.stats_out = mem;
    return a;
}
template <bool SKIP, bool DUP> GemmArgs out_layers(int T, int) {
    GemmArgs a = args(T, MC);
    a.nseg = SKIP ? 3 : 1;
    a.seg[0] = seg(MC, 3, T, XF_GN_SILU, PK_BLOCK, true);
    gn(a.seg[0], T, 6, 1e-5f);
    if (SKIP) a.seg[1] = a.seg[2] = seg(MC, 1, T, XF_NONE, PK_BLOCK);
    else res_plain(a);
    a.bias = mem; a.stats_out = mem;
    if (DUP) { a.y2 = mem; a.y2_bstride = a.y_bstride; }
    return a;
}
// PK_PLAIN: a weight without the split-fp16 packing; DIM = 24: a head size the epilogue does not serve
template <Pack PK, int DIM> GemmArgs qkv(int T, int) {
    GemmArgs a = args(T, 3 * MC);
    a.nseg = 1;
    a.seg[0] = seg(MC, 1, T, XF_GN_LN, PK, true, true);
    gn(a.seg[0], T, 6, 1e-6f);
    a.tm_tiles = 2 * MC / 32; a.vt = mem; a.vt_heads = 2 * HEADS; a.vt_dim = DIM; a.vt_rows = a.y_pitch;
    return a;
}
template <bool DUP> GemmArgs to_out1(int T, int) {
    GemmArgs a = args(T, MC);
    a.nseg = 1;
    a.seg[0] = seg(MC, 1, T, XF_NONE, PK_BLOCK);
    a.bias = mem;
    a.res_kind = RES_GN; a.res = mem; a.res_bstride = a.y_bstride; a.res_pitch = a.y_pitch;
    a.res_gn_part = a.res_gn_gamma = a.res_gn_beta = mem; a.res_gn_cpg = 6; a.res_gn_nparts = (T + 31) / 32; a.res_gn_eps = 1e-6f;
    if (DUP) { a.y2 = mem; a.y2_bstride = a.y_bstride; a.y2_add = mem; }
    return a;
}
template <bool BAND> GemmArgs q2(int T, int) {   // BAND = false: the plain q projection in front of the generic band kernel (wide alignment windows)
    GemmArgs a = args(T, MC);
    a.nseg = 1;
    a.seg[0] = seg(MC, 1, T, XF_LN, PK_BLOCK, false, true);
    if (BAND) { a.band.k = a.band.v = mem; a.band.wmax = 4; a.band.scale = 1.f; }
    return a;
}
template <bool W2> GemmArgs to_out2(int T, int) {   // W2 = false: no bf16 packing — bf16 mode then multiplies in fp32
    GemmArgs a = args(T, MC);
    a.nseg = 1;
    a.seg[0] = seg(MC, 1, T, XF_NONE, PK_BLOCK);
    if (!W2) a.seg[0].w2 = nullptr;
    a.bias = mem;
    res_plain(a);
    return a;
}
GemmArgs geglu(int T, int) {
    GemmArgs a = args(T, FFI);
    a.nseg = 1;
    a.seg[0] = seg(MC, 1, T, XF_LN, PK_FLAT, false, true);
    a.bias = mem; a.geglu_gate_tiles = FFI / 32;
    return a;
}
GemmArgs proj_out(int T, int) {
    GemmArgs a = args(T, MC);
    a.nseg = 2;
    a.seg[0] = seg(FFI, 1, T, XF_NONE, PK_BLOCK);
    a.seg[1] = seg(MC, 1, T, XF_NONE, PK_BLOCK);
    a.bias = mem; a.stats_out = mem;
    res_plain(a);
    return a;
}
GemmArgs out_conv(int T, int) {
    GemmArgs a = args(T, CIN);
    a.nseg = 1;
    a.seg[0] = seg(MC, 3, T, XF_GN_SILU, PK_BLOCK, true);
    gn(a.seg[0], T, 6, 1e-5f);
    a.bias = mem;
    return a;
}

const Case CASES[] = {
    {"conv_in", EPI_STORE, conv_in<false>, nb_unet}, {"conv_in_step", EPI_STORE, conv_in<true>, nb_unet},
    {"in_layers", EPI_STORE, in_layers<1>, nb_unet}, {"in_layers_cat", EPI_STORE, in_layers<2>, nb_unet},
    {"out_layers", EPI_STORE, out_layers<false, false>, nb_unet}, {"out_layers_dup", EPI_STORE, out_layers<false, true>, nb_unet},
    {"out_layers_skip", EPI_STORE, out_layers<true, false>, nb_unet},
    {"qkv", EPI_QKV, qkv<PK_BLOCK, HD>, nb_qkv}, {"qkv_no_ws", EPI_QKV, qkv<PK_PLAIN, HD>, nb_qkv}, {"qkv_dim24", EPI_QKV, qkv<PK_BLOCK, 24>, nb_qkv},
    {"to_out1", EPI_STORE, to_out1<false>, nb_one}, {"to_out1_dup", EPI_STORE, to_out1<true>, nb_one},
    {"q2_band", EPI_BAND, q2<true>, nb_one}, {"q2_plain", EPI_STORE, q2<false>, nb_one},
    {"to_out2", EPI_STORE, to_out2<true>, nb_unet}, {"to_out2_no_w2", EPI_STORE, to_out2<false>, nb_unet},
    {"geglu", EPI_GEGLU, geglu, nb_geglu},
    {"proj_out", EPI_STORE, proj_out, nb_unet},
    {"out_conv", EPI_STORE, out_conv, nb_one},
};
// T = 32: the token-tile total is the batch, every total up to 400 (best_nb's rounds at 43 / 86 / 128 / 171, pick_unet_nb's 1024 / 6, the 192-workgroup rules of q/k/v
// and GEGLU, the kconv window 86 .. 128); T = 64: totals to 2800 in twos, where a workgroup can take two tiles; T = 1800 (57 tiles, 114 at two samples): pick_tt's
// 228- and 1024-workgroup divisors and its cap of 8 (q/k/v: 8 from 24 samples; the store shapes: 8 from 48)
const struct { int T, max_batch; } SCANS[] = {{32, 400}, {64, 1400}, {1800, 50}};
const char* KERNEL[] = {"cgemm", "f32", "bf16", "sp"};

}  // namespace

int main(int argc, char** argv) {
#ifdef SAID_UGEMM_ROWS
    if (argc > 1 && !strcmp(argv[1], "rows")) return check_rows();
#endif
#ifdef SAID_UGEMM_ROWS
    if (argc > 3 && !strcmp(argv[1], "plan")) {
        const int batch = atoi(argv[2]), T = atoi(argv[3]);
        const PlanSwitches sw = {false, argc > 4 ? atoi(argv[4]) != 0 : true, -1, false, false};
        for (const Case& cs : CASES) {
            const GemmArgs a = cs.make(T, batch);
            const GemmPlan p = plan_gemm(sw, a, cs.epi, batch, cs.nb((long long)batch * ((T + 31) / 32)), 8);
            const URow* r = p.on_ugemm() ? ugemm_row(cs.epi, p.NB, p.KS, uvar_of(a, cs.epi), p.mode(), p.tt > 1) : nullptr;
            printf("%s %s/%d/%d/%d %s\n", cs.name, KERNEL[(int)p.kernel], p.NB, p.KS, p.tt, (r && r->kconv) ? "kconv" : "block");
        }
        return 0;
    }
#endif
    for (const Case& cs : CASES)
        for (const auto& sc : SCANS) {
            std::map<std::string, std::string> by_result;   // scan -> switch codes
            std::vector<std::string> order;
            for (int code = 0; code < 48; ++code) {
                const PlanSwitches sw = {code >= 24, (code / 12) % 2 != 0, (code / 4) % 3, (code / 2) % 2 != 0, code % 2 != 0};
                std::string scan, last;
                for (int batch = 1; batch <= sc.max_batch; ++batch) {
                    const GemmArgs a = cs.make(sc.T, batch);
                    const long long tiles = (long long)batch * ((sc.T + 31) / 32);
                    const int nb = cs.nb(tiles);
                    const GemmPlan p = plan_gemm(sw, a, cs.epi, batch, nb, 8);
                    char buf[96];
                    int n = snprintf(buf, sizeof buf, "%s/%d/%d/%d", KERNEL[(int)p.kernel], p.NB, p.KS, p.tt);
                    if (cs.epi == EPI_QKV) snprintf(buf + n, sizeof buf - n, "/p%d", (int)(ugemm_supports(a, EPI_QKV, nb, 8, U_SP) || ugemm_supports(a, EPI_QKV, nb, 8, U_F32)));
                    if (last != buf) { scan += " b" + std::to_string(batch) + "=" + buf; last = buf; }
                }
                char sc5[8];
                snprintf(sc5, sizeof sc5, "%c%d%d%d%d", sw.bf16 ? 'b' : 'f', (int)sw.split, sw.kconv, (int)sw.concurrent, (int)sw.clk);
                if (!by_result.count(scan)) order.push_back(scan);
                by_result[scan] += std::string(by_result[scan].empty() ? "" : ",") + sc5;
            }
            for (const std::string& scan : order) printf("%s T=%d %s :%s\n", cs.name, sc.T, by_result[scan].c_str(), scan.c_str());
        }
    return 0;
}
