// ut_gemm_plan_main — said_amd/csrc/ut_gemm_plan.h behind a command line for tests/test_ut_gemm_plan_cpu.py: the K-split plan of the training
// step's weight gradients (Gm::ksplit, EncGm::split_small and the partial-tile buffer's size in unet_trainer.cpp), without a device.
//   sweep <Kmax>          -> one line per K in 1 .. Kmax: `K KS kchunk empty` for a weight gradient of one 192 x 192 tile set in the default
//                            context (empty: chunks with ks kchunk >= K), then `total <K with an empty chunk> first <the first such K>`
//   products <F> <L> <B> <T>
//                         -> `cap <gpart_n>`, then one line per K-split product of the (F, L) context's step at B x T, in the order of
//                            enqueue_backward / enqueue_enc_backward: `tensor kind M N Z K KS kchunk want need`
//                            kind w: a weight gradient (ut_ksplit), want = its chunk count before the capacity is looked at, need = want Z M N;
//                            kind s: the positional convolution's forward / data gradient (ut_split_small), want = need = 0
//   ksplit <K> <M> <N> <Z> <capacity>
//                         -> `KS kchunk` of one weight gradient with a partial-tile buffer of `capacity` floats
#include <cstdio>
#include <cstdlib>
#include <string>

#include "ut_gemm_plan.h"

using namespace said::ut;

namespace {

constexpr int CH = 192, TEd = 768, FF = 768, XC = 32, AUD = 768, EH = 768, ECONV = 512, EFFN = 3072;
size_t cap;

void wgrad(const std::string& name, int M, int N, int Z, int K) {
    const UtSplit p = ut_ksplit(K, M, N, Z, cap);
    const int want = ut_ksplit_want(K);
    printf("%s w %d %d %d %d %d %d %d %zu\n", name.c_str(), M, N, Z, K, p.KS, p.kchunk, want, (size_t)want * Z * M * N);
}
void small(const std::string& name, int M, int N, int Z, int K) {
    const UtSplit p = ut_split_small(K, M, N, Z, cap);
    printf("%s s %d %d %d %d %d %d 0 0\n", name.c_str(), M, N, Z, K, p.KS, p.kchunk);
}
// lin_wgrad: dW (N, K) over `rows`; conv_wgrad: dW (Co, Ci 3) over B T
void lin(const std::string& name, int rows, int N, int K) { wgrad(name, N, K, 1, rows); }
void conv(const std::string& name, int Co, int Ci, int rows) { wgrad(name, Co, Ci * 3, 1, rows); }

void res(const std::string& q, int ci, int B, int M) {
    conv(q + ".out_layers.3.weight", CH, CH, M);
    lin(q + ".emb_layers.1.weight", B, CH, TEd);
    conv(q + ".in_layers.2.weight", CH, ci, M);
    if (ci != CH) lin(q + ".skip_connection.weight", M, CH, ci);
}
void st(const std::string& q, int CTX, int M) {
    const std::string b = q + ".transformer_blocks.0";
    lin(q + ".proj_out.weight", M, CH, CH);
    lin(b + ".ff.net.2.weight", M, CH, FF);
    lin(b + ".ff.net.0.proj.weight", M, 2 * FF, CH);
    lin(b + ".attn2.to_out.0.weight", M, CH, CH);
    lin(b + ".attn2.to_q.weight", M, CH, CH);
    lin(b + ".attn2.to_k.weight", M, CH, CTX);
    lin(b + ".attn2.to_v.weight", M, CH, CTX);
    lin(b + ".attn1.to_out.0.weight", M, CH, CH);
    lin(b + ".attn1.to_q.weight", M, CH, CH);
    lin(b + ".attn1.to_k.weight", M, CH, CH);
    lin(b + ".attn1.to_v.weight", M, CH, CH);
}

}  // namespace

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "sweep" && argc == 3) {
        const int kmax = atoi(argv[2]);
        cap = ut_gpart_n(-1, 0);
        int total = 0, first = 0;
        for (int K = 1; K <= kmax; ++K) {
            const UtSplit p = ut_ksplit(K, CH, CH, 1, cap);
            int empty = 0;
            for (int ks = 0; ks < p.KS; ++ks) empty += (long long)ks * p.kchunk >= K;
            if (empty) { ++total; if (!first) first = K; }
            printf("%d %d %d %d\n", K, p.KS, p.kchunk, empty);
        }
        printf("total %d first %d\n", total, first);
        return 0;
    }
    if (cmd == "products" && argc == 6) {
        const int F = atoi(argv[2]), L = atoi(argv[3]), B = atoi(argv[4]), T = atoi(argv[5]), M = B * T, CTX = F > 0 ? F : AUD;
        cap = ut_gpart_n(F, L);
        printf("cap %zu\n", cap);
        const std::string m = "denoiser.model.";
        conv(m + "out.2.weight", XC, CH, M);
        st(m + "output_blocks.1.1", CTX, M); res(m + "output_blocks.1.0", 2 * CH, B, M);
        st(m + "output_blocks.0.1", CTX, M); res(m + "output_blocks.0.0", 2 * CH, B, M);
        res(m + "middle_block.2", CH, B, M);
        st(m + "middle_block.1", CTX, M); res(m + "middle_block.0", CH, B, M);
        st(m + "input_blocks.1.1", CTX, M); res(m + "input_blocks.1.0", CH, B, M);
        conv(m + "input_blocks.0.0.weight", CH, XC, M);
        lin(m + "time_embed.2.weight", B, TEd, TEd);
        lin(m + "time_embed.0.weight", B, TEd, CH);
        if (F > 0) lin("audio_proj_layer.weight", M, CTX, AUD);
        if (L > 0) {
            const std::string e = "audio_encoder.";
            small("pos_fwd", M, UT_EPC, UT_EPG, UT_EPK * UT_EPC);
            for (int l = L - 1; l >= 0; --l) {
                const std::string p = e + "encoder.layers." + std::to_string(l);
                lin(p + ".feed_forward.output_dense.weight", M, EH, EFFN);
                lin(p + ".feed_forward.intermediate_dense.weight", M, EFFN, EH);
                lin(p + ".attention.out_proj.weight", M, EH, EH);
                lin(p + ".attention.q_proj.weight", M, EH, EH);
                lin(p + ".attention.k_proj.weight", M, EH, EH);
                lin(p + ".attention.v_proj.weight", M, EH, EH);
            }
            small("pos_dgrad", M, UT_EPC, UT_EPG, UT_EPK * UT_EPC);
            wgrad(e + "encoder.pos_conv_embed.conv.weight_v", UT_EPC, UT_EPC * UT_EPK, UT_EPG, M);
            lin(e + "feature_projection.projection.weight", M, EH, ECONV);
        }
        return 0;
    }
    if (cmd == "ksplit" && argc == 7) {
        const UtSplit p = ut_ksplit(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), (size_t)atoll(argv[6]));
        printf("%d %d\n", p.KS, p.kchunk);
        return 0;
    }
    fprintf(stderr, "usage: ut_gemm_plan_main sweep <Kmax> | products <F> <L> <B> <T> | ksplit <K> <M> <N> <Z> <capacity>\n");
    return 2;
}
