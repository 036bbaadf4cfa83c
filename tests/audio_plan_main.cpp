// audio_plan_main — said_amd/csrc/audio_plan.h behind a command line for tests/test_audio_plan_cpu.py: the launch plan of the fp32 audio encoder
// (audio_enc.cpp, fp32 branch) without a device.
//   plan <clips per pass> <samples> <frames, 0 = none given>
//       -> one line per launch site of one pass: `site tiles=<token tiles> asked=<NB>/<KS> runs=<NB>/<KS>` (asked: what the site requests of launch_gemm,
//          runs: the instantiation launch_gemm resolves it to), and `attn tiles=<..> ks=<key slices> ks_train=<with attention dropout>`
//   fallback <max token tiles>
//       -> per GEMM site, the token-tile counts 1 .. max at which launch_gemm would fall back to (1, 8) from another request:
//          `site n=<how many> first=<first such count or 0>`
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "audio_plan.h"

using namespace said;

namespace {

struct Site { const char* name; int epi; LaunchCfg (*ask)(long long); };
const Site SITES[] = {
    {"conv", EPI_STORE, audio_plan::conv},   {"fproj", EPI_STORE, audio_plan::hidden}, {"pos", EPI_STORE, audio_plan::posconv},
    {"qkv", EPI_QKV, audio_plan::qkv},       {"out", EPI_STORE, audio_plan::hidden},   {"ff1", EPI_STORE, audio_plan::ffn},
    {"ff2", EPI_STORE, audio_plan::hidden},  {"proj", EPI_STORE, audio_plan::proj},
};
const int CONV_K[7] = {10, 3, 3, 3, 3, 2, 2}, CONV_S[7] = {5, 2, 2, 2, 2, 2, 2};

void line(const char* name, int idx, const Site& st, long long tt) {
    const LaunchCfg a = st.ask(tt), r = cgemm_resolve(st.epi, a.NB, a.KS);
    if (idx >= 0) printf("%s%d tiles=%lld asked=%d/%d runs=%d/%d\n", name, idx, tt, a.NB, a.KS, r.NB, r.KS);
    else printf("%s tiles=%lld asked=%d/%d runs=%d/%d\n", name, tt, a.NB, a.KS, r.NB, r.KS);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "plan")) {
        const int nb = atoi(argv[2]), Ta = atoi(argv[3]), nf = atoi(argv[4]);
        int L[7], len = Ta;
        for (int i = 0; i < 7; ++i) {
            len = (len - CONV_K[i]) / CONV_S[i] + 1;
            if (len < 1) { fprintf(stderr, "too short\n"); return 2; }
            L[i] = len;
        }
        const int Fr = nf > 0 ? nf : L[6];
        printf("frames=%d pitch=%d\n", Fr, (Fr + 31) / 32 * 32);
        for (int i = 1; i < 7; ++i) line("conv", i, SITES[0], audio_plan::token_tiles(nb, L[i]));
        const long long tt = audio_plan::token_tiles(nb, Fr);
        for (size_t i = 1; i < sizeof SITES / sizeof SITES[0]; ++i) line(SITES[i].name, -1, SITES[i], tt);
        printf("attn tiles=%lld ks=%d ks_train=%d\n", tt, audio_plan::attn_slices(tt), audio_plan::attn_slices(tt, true));
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "fallback")) {
        const long long mx = atoll(argv[2]);
        for (const Site& st : SITES) {
            long long n = 0, first = 0;
            for (long long tt = 1; tt <= mx; ++tt) {
                const LaunchCfg a = st.ask(tt), r = cgemm_resolve(st.epi, a.NB, a.KS);
                if (r.NB != a.NB || r.KS != a.KS) { if (!n) first = tt; ++n; }
            }
            printf("%s n=%lld first=%lld\n", st.name, n, first);
        }
        return 0;
    }
    fprintf(stderr, "usage: audio_plan_main plan <clips> <samples> <frames> | fallback <max token tiles>\n");
    return 2;
}
