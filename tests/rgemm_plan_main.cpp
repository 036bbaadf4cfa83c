// rgemm_plan_main — said_amd/csrc/rgemm_plan.h behind a command line for tests/test_rgemm_plan_cpu.py: the plan of every rgemm_kernel launch of the token-major bf16
// schedule (the TGemmArgs of run_resblock_tm, run_transformer_tm and run_tm_tail in unet_sched.cpp), without a device.
//   <Be> <Bc> <T> <six>  -> one line per launch in schedule order: `name v<variant> <ntap>,<ek>,<mode>,<res>,<dup>,<stats>,<nch> per=<row tiles per range> grid=<workgroups>
//                           groups=<column groups> batch=<samples> spr=<samples a range touches at most>`
//                           Be samples (Bc > 0: the guided step, Bc clips, Be = 2 Bc), T frames, six = 1: the six-launch tail instead of the fused one.  forward() (Bc = 0)
//                           ends its last block on xgemm_kernel, the loop on the fused tail (or, six, on the proj_out pair): those launches are not rgemm's and not listed.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rgemm_plan.h"

using namespace said;

namespace {

constexpr int MC = 192, FFI = 768, HD = 32, HEADS = 6;
float mem[4];   // every pointer the plan only tests for null
int imem[4];
int rup(int a, int b) { return (a + b - 1) / b * b; }

struct Geo { int Be, Bc, T; };
int seg(const Geo& g) { return rup(g.T, 64); }

TGemmArgs mkx(const Geo& g, int N, int K) {
    TGemmArgs t;
    memset(&t, 0, sizeof t);
    t.w = mem; t.M = g.T; t.N = N; t.K = K; t.seg_rows = seg(g);
    t.gn_part_bs = (long long)MC * ((g.T + 31) / 32) * 2; t.gn_nparts = (g.T + 31) / 32; t.stats_bs = t.gn_part_bs; t.ldy = MC; t.ldr_tm = MC;
    return t;
}
TGemmArgs conv3(const Geo& g, int cpg) {
    TGemmArgs t = mkx(g, MC, 3 * MC);
    t.ra[0] = mem; t.rmode = 1; t.rtaps = 3;
    t.gn_part[0] = mem; t.gn_cpg = cpg; t.gn_eps = 1e-5f; t.gn_gamma = t.gn_beta = mem;
    return t;
}
void emit(const char* name, const TGemmArgs& a_in, int batch) {
    TGemmArgs a = a_in;
    a.batch = batch;
    RgPlan p;
    if (!rg_plan(a, p)) { printf("%s unserved\n", name); return; }
    const int ntv = (a.M + 31) / 32;
    // samples a range of `per` consecutive tiles touches at most (ranges start at multiples of per)
    int spr = 0;
    for (int tb = 0; tb < batch * ntv; tb += p.per) {
        const int last = (tb + p.per < batch * ntv ? tb + p.per : batch * ntv) - 1;
        const int n = last / ntv - tb / ntv + 1;
        if (n > spr) spr = n;
    }
    printf("%s v%d %d,%d,%d,%d,%d,%d,%d per=%d grid=%d groups=%d batch=%d spr=%d\n", name, rg_variant(p), p.ntap, p.ek, p.mode, p.res, p.dup, p.stats, p.nch, p.per, p.grid, p.groups,
           batch, spr);
}

void resblock(const Geo& g, int i, bool shared) {
    const int nb = shared ? g.Bc : g.Be;
    char nm[32];
    if (i >= 3) {   // concatenated input: launches over column ranges of the packed weights
        TGemmArgs p0 = conv3(g, 12);
        p0.w_ld = 3 * 2 * MC; p0.w_k0 = 0; p0.w_seg = 2 * MC; p0.y_tm = mem;
        snprintf(nm, sizeof nm, "res%d.conv1a", i); emit(nm, p0, nb);
        TGemmArgs t = conv3(g, 12);
        t.w_ld = 3 * 2 * MC; t.w_k0 = MC; t.w_seg = 2 * MC; t.bias = mem; t.emb = mem; t.emb_pitch = 64; t.res_tm = mem; t.y_tm = mem; t.stats = mem;
        snprintf(nm, sizeof nm, "res%d.conv1b", i); emit(nm, t, nb);
        TGemmArgs s = mkx(g, MC, 2 * MC);
        s.sa[0] = s.sa[1] = mem; s.sld[0] = s.sld[1] = MC; s.sk[0] = s.sk[1] = MC; s.w_ld = 5 * MC; s.w_k0 = 3 * MC; s.y_tm = mem;
        snprintf(nm, sizeof nm, "res%d.skip", i); emit(nm, s, nb);
        TGemmArgs c = conv3(g, 6);
        c.w_ld = 5 * MC; c.w_k0 = 0; c.bias = mem; c.res_tm = mem; c.y_tm = mem; c.stats = mem;
        snprintf(nm, sizeof nm, "res%d.conv2", i); emit(nm, c, nb);
        return;
    }
    TGemmArgs t = conv3(g, 6);
    t.bias = mem; t.emb = mem; t.emb_pitch = 64; t.y_tm = mem; t.stats = mem;
    snprintf(nm, sizeof nm, "res%d.conv1", i); emit(nm, t, nb);
    TGemmArgs c = conv3(g, 6);
    c.bias = mem; c.res_tm = mem; c.y_tm = mem; c.stats = mem;
    if (shared) { c.y2_tm = mem; c.y2_row_off = (long long)g.Bc * seg(g); }
    snprintf(nm, sizeof nm, "res%d.conv2", i); emit(nm, c, nb);
}

void transformer(const Geo& g, int j, bool shared, bool six, bool last) {
    const int n1 = shared ? g.Bc : g.Be, n2 = g.Bc > 0 ? g.Bc : g.Be;
    char nm[32];
    TGemmArgs q = mkx(g, 3 * MC, MC);
    q.ra[0] = mem; q.rmode = 3; q.rtaps = 1;
    q.gn_part[0] = mem; q.gn_cpg = 6; q.gn_eps = 1e-6f; q.gn_gamma = q.gn_beta = q.ln_gamma = q.ln_beta = mem;
    q.qk = mem; q.vt = mem; q.v_bs = (long long)MC * rup(g.T, 32); q.qk_n = 2 * MC; q.head_dim = HD; q.rows = rup(g.T, 32); q.heads2 = 2 * HEADS; q.v_pitch = rup(g.T, 32);
    q.qkv_bf16 = g.T <= 640 ? 1 : 0; q.q_scale = 1.f;
    snprintf(nm, sizeof nm, "st%d.qkv", j); emit(nm, q, n1);
    const bool forward_last = last && g.Bc == 0;
    if (!six && !forward_last) return;   // the fused tail (stchain_kernel)
    TGemmArgs o1 = mkx(g, MC, MC);
    o1.sa[0] = mem; o1.sld[0] = MC; o1.sk[0] = MC; o1.bias = mem;
    o1.res_tm = mem; o1.res_gn = 1; o1.res_part = o1.res_gamma = o1.res_beta = mem; o1.res_eps = 1e-6f; o1.gn_cpg = 6; o1.y_tm = mem;
    if (g.Bc > 0) { o1.y2_tm = mem; o1.y2_add = mem; }
    snprintf(nm, sizeof nm, "st%d.out1", j); emit(nm, o1, n1);
    TGemmArgs b = mkx(g, MC, MC);
    b.ra[0] = mem; b.rmode = 2; b.rtaps = 1; b.ln_gamma = b.ln_beta = mem;
    b.band_k = b.band_v = mem; b.band_lo = b.band_hi = imem; b.band_wmax = 4; b.band_scale = 1.f; b.y_tm = mem;
    snprintf(nm, sizeof nm, "st%d.band", j); emit(nm, b, n2);
    TGemmArgs o2 = mkx(g, MC, MC);
    o2.sa[0] = mem; o2.sld[0] = MC; o2.sk[0] = MC; o2.bias = mem; o2.res_tm = mem; o2.y_tm = mem;
    snprintf(nm, sizeof nm, "st%d.out2", j); emit(nm, o2, n2);
    TGemmArgs ge = mkx(g, 2 * FFI, MC);
    ge.ra[0] = mem; ge.rmode = 2; ge.rtaps = 1; ge.ln_gamma = ge.ln_beta = mem; ge.bias = mem; ge.geglu = 1; ge.yb = mem; ge.y_bs = (long long)seg(g) * FFI; ge.ldy = FFI;
    snprintf(nm, sizeof nm, "st%d.geglu", j); emit(nm, ge, g.Be);
    if (forward_last) return;       // (the channel-major folded proj_out: xgemm_kernel)
    TGemmArgs h = mkx(g, MC, FFI);
    h.sa[0] = mem; h.sld[0] = FFI; h.sk[0] = FFI; h.w_ld = FFI + MC; h.w_k0 = 0; h.res_tm = mem; h.y_tm = mem;
    snprintf(nm, sizeof nm, "st%d.proj_h", j); emit(nm, h, g.Be);
    TGemmArgs x = mkx(g, MC, MC);
    x.sa[0] = mem; x.sld[0] = MC; x.sk[0] = MC; x.w_ld = FFI + MC; x.w_k0 = FFI; x.bias = mem; x.res_tm = mem; x.y_tm = mem; x.stats = mem;
    snprintf(nm, sizeof nm, "st%d.proj_x", j); emit(nm, x, g.Be);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: rgemm_plan_main <Be> <Bc> <T> <six>\n"); return 2; }
    const Geo g = {atoi(argv[1]), atoi(argv[2]), atoi(argv[3])};
    const bool six = atoi(argv[4]) != 0, sh = g.Bc > 0;
    resblock(g, 0, sh); transformer(g, 0, sh, six, false);
    resblock(g, 1, false); transformer(g, 1, false, six, false);
    resblock(g, 2, false);
    resblock(g, 3, false); transformer(g, 2, false, six, false);
    resblock(g, 4, false); transformer(g, 3, false, six, true);
    return 0;
}
