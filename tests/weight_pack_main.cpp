// weight_pack_main — command-line front of said_amd/csrc/weight_pack.h for tests/test_weight_pack_cpu.py: raw fp32 files in, packed buffers out.
//   frag  W.f32 Ctot taps N row0 c_begin C PREFIX   -> PREFIX.rows .rows4 .bf16 [.split_block] [.split_flat]   (rows_dense(N, row0), channels [c_begin, c_begin + C))
//   tm    W.f32 N C taps PREFIX                     -> PREFIX.tm .bf16 .words                                  (the token-major GEMM operands)
//   chain DIR                                       -> DIR/stream1 stream3 stream2 stream_bf16 vec .bin        (the fused tail, from DIR/<operand>.f32)
#include <cstdio>
#include <cstdlib>
#include <string>

#include "weight_pack.h"

using namespace said;
using namespace said::pack;

static std::vector<float> rd(const std::string& path) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
    fseek(f, 0, SEEK_END);
    std::vector<float> v((size_t)ftell(f) / 4);
    fseek(f, 0, SEEK_SET);
    if (fread(v.data(), 4, v.size(), f) != v.size()) exit(2);
    fclose(f);
    return v;
}
template <typename T>
static void wr(const std::string& path, const std::vector<T>& v) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
}
static std::vector<float> need(const std::string& path, size_t n) {
    std::vector<float> v = rd(path);
    if (v.size() != n) { fprintf(stderr, "%s: %zu floats, expected %zu\n", path.c_str(), v.size(), n); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "frag" && argc == 10) {
        const int Ctot = atoi(argv[3]), taps = atoi(argv[4]), N = atoi(argv[5]), row0 = atoi(argv[6]), c_begin = atoi(argv[7]), C = atoi(argv[8]);
        const std::string out = argv[9];
        const std::vector<float> W = rd(argv[2]);
        if (W.size() < (size_t)(row0 + N) * Ctot * taps || c_begin + C > Ctot) { fprintf(stderr, "frag: W too small\n"); return 2; }
        const Rows rows = rows_dense(W.data(), Ctot, taps, N, row0);
        wr(out + ".rows", pack_rows(rows, c_begin, C));
        wr(out + ".rows4", pack_rows4(rows, c_begin, C));
        wr(out + ".bf16", pack_rows_bf16(rows, c_begin, C));
        if (C % 24 == 0 && (taps == 1 || taps == 3)) wr(out + ".split_block", pack_rows_split(rows, c_begin, C, false));
        if (C % 16 == 0 && taps == 1) wr(out + ".split_flat", pack_rows_split(rows, c_begin, C, true));
        return 0;
    }
    if (cmd == "tm" && argc == 7) {
        const size_t N = atoi(argv[3]), C = atoi(argv[4]), taps = atoi(argv[5]);
        const std::string out = argv[6];
        const std::vector<float> W = need(argv[2], N * C * taps), tm = tap_major(W.data(), N, C, taps);
        wr(out + ".tm", tm);
        wr(out + ".bf16", to_bf16(tm));
        wr(out + ".words", to_split_words(tm));
        return 0;
    }
    if (cmd == "chain" && argc == 3) {
        const std::string d = std::string(argv[2]) + "/";
        const int MC = CHAIN_MC, FFI = CHAIN_FFI;
        const auto w1 = need(d + "out1.f32", MC * MC), q = need(d + "q.f32", MC * MC), g2 = need(d + "g2.f32", MC), be2 = need(d + "be2.f32", MC);
        const auto w3 = need(d + "out2.f32", MC * MC), ff = need(d + "ff.f32", 2 * FFI * MC), g3 = need(d + "g3.f32", MC), be3 = need(d + "be3.f32", MC);
        const auto ffb = need(d + "ffb.f32", 2 * FFI), b1 = need(d + "b1.f32", MC), b3 = need(d + "b3.f32", MC), c2 = need(d + "c2.f32", MC);
        const auto fp = need(d + "ffproj.f32", MC * (FFI + MC)), fpb = need(d + "ffproj_b.f32", MC);
        const auto qf = fold_gamma(q.data(), MC, MC, g2.data()), fff = fold_gamma(ff.data(), 2 * FFI, MC, g3.data());
        const ChainMats m{{w1.data(), qf.data(), w3.data(), fff.data(), fp.data()}};
        const auto s1 = chain_stream_f16(chain_plan(1), m), s3 = chain_stream_f16(chain_plan(3), m), s2 = chain_stream_f16(chain_plan(2), m);
        const auto sb = chain_stream_bf16(chain_plan(1), m);
        if (s1.size() * 2 != CHAIN_STREAM_BYTES || s3.size() * 2 != CHAIN3_STREAM_BYTES || s2.size() * 2 != CHAIN2_STREAM_BYTES || sb.size() != CHAIN_STREAM_UNITS * 512) {
            fprintf(stderr, "chain: stream size mismatch\n");
            return 3;
        }
        wr(d + "stream1.bin", s1);
        wr(d + "stream3.bin", s3);
        wr(d + "stream2.bin", s2);
        wr(d + "stream_bf16.bin", sb);
        const auto bq = fold_beta(q.data(), MC, MC, be2.data(), nullptr), bff = fold_beta(ff.data(), 2 * FFI, MC, be3.data(), ffb.data());
        wr(d + "vec.bin", chain_vec(b1.data(), bq.data(), b3.data(), c2.data(), fpb.data(), bff.data()));
        return 0;
    }
    fprintf(stderr, "usage: weight_pack_main frag|tm|chain ... (see the head of tests/weight_pack_main.cpp)\n");
    return 1;
}
