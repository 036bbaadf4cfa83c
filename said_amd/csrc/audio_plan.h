// audio_plan.h — the host-side launch decisions of the fp32 audio encoder (audio_enc.cpp, fp32 branch; kernels: cgemm_kernel in gemm.hip, attn_kernel in
// attn.hip), host-only: which (NB, KS) tile shape each channel-major GEMM asks for (pick_cfg and the sites that do not use it), which shape launch_gemm
// then really runs (cgemm_resolve: a shape gemm.hip does not instantiate goes back to one tile x eight waves), and how many key slices attention takes.
// A header of its own so that tests can ask it without a GPU (tests/audio_plan_main.cpp), as ugemm_plan.h, rgemm_plan.h and ut_gemm_plan.h are for
// the other GEMMs.
#pragma once
#include "kernels.h"

namespace said {

struct LaunchCfg { int NB, KS; };

// tile shape of a channel-major GEMM over t_tiles_total 32-token tiles (all samples of the launch) and ntiles 32-column tiles
inline LaunchCfg pick_cfg(long long t_tiles_total, int ntiles, bool allow6 = true) {
    // small problems: maximise workgroups (split K over 8 waves, one tile each);
    // large problems: amortise the operand transform over more tiles per workgroup.
    if (t_tiles_total * ntiles <= 1536 || ntiles % 2) return {1, 8};
    if (t_tiles_total * ntiles <= 4096) return {2, 8};
    if (allow6 && ntiles % 6 == 0) return {6, 4};
    if (ntiles % 4 == 0) return {4, 4};
    if (ntiles % 3 == 0) return {3, 4};
    return {2, 8};
}

// ---- the instantiations of cgemm_kernel<NB, KS, EPI> (gemm.hip expands the same list into its launchers) ----
#define SAID_GEMM_CONFIGS(X)                                                                   \
    X(EPI_STORE, 1, 8) X(EPI_STORE, 2, 8) X(EPI_STORE, 3, 4) X(EPI_STORE, 6, 4) X(EPI_STORE, 4, 4) \
    X(EPI_QKV, 1, 8) X(EPI_QKV, 2, 8) X(EPI_QKV, 3, 4) X(EPI_QKV, 6, 4)                        \
    X(EPI_GEGLU, 1, 8) X(EPI_GEGLU, 3, 4)                                                      \
    X(EPI_BAND, 1, 8) X(EPI_BAND, 1, 4)

inline bool cgemm_instantiated(int epi, int NB, int KS) {
#define X(E, nb, ks) if (epi == E && NB == nb && KS == ks) return true;
    SAID_GEMM_CONFIGS(X)
#undef X
    return false;
}
// The shape launch_gemm runs when (NB, KS) is asked for: the shape itself where it is instantiated; else one tile x eight waves (a tile shape chosen for
// the LDS-staged kernel that this kernel does not instantiate: every epilogue exists as (1, 8), and the q/k/v token-major split needs tm_tiles % NB == 0,
// which NB = 1 always satisfies); {0, 0}: not even that (an unknown epilogue).
inline LaunchCfg cgemm_resolve(int epi, int NB, int KS) {
    if (cgemm_instantiated(epi, NB, KS)) return {NB, KS};
    if (cgemm_instantiated(epi, 1, 8)) return {1, 8};
    return {0, 0};
}

// ---- the fp32 audio encoder's launch sites ----
namespace audio_plan {

constexpr int AP_CONV = 512, AP_H = 768, AP_FFN = 3072, AP_HEADS = 12;

// token tiles of one pass: nb clips of `frames` tokens each (a clip's tiles are its own: the pitch is a multiple of 32)
inline long long token_tiles(int nb, int frames) { return (long long)nb * ((frames + 31) / 32); }

// strided convolutions 1-6 of the feature extractor (tt: tiles of the convolution's OUTPUT length)
inline LaunchCfg conv(long long tt) { return pick_cfg(tt, AP_CONV / 32, false); }
// feature projection, out_proj, ff2: 768 columns
inline LaunchCfg hidden(long long tt) { return pick_cfg(tt, AP_H / 32); }
// ff1: 3072 columns
inline LaunchCfg ffn(long long tt) { return pick_cfg(tt, AP_FFN / 32); }
// q/k/v (EPI_QKV, 72 column tiles)
inline bool qkv_big(long long tt) { return tt * 72 > 4096; }
inline LaunchCfg qkv(long long tt) { return qkv_big(tt) ? LaunchCfg{6, 4} : LaunchCfg{2, 8}; }
// grouped positional convolution: 16 groups of two column tiles
inline LaunchCfg posconv(long long tt) { return LaunchCfg{tt * 32 <= 2048 ? 1 : 2, 8}; }
// audio_proj_layer
inline LaunchCfg proj(long long) { return LaunchCfg{1, 8}; }
// key slices of attn_kernel<2, KS, PM>: one workgroup per (clip, head, token tile).  with_dropout: the train-mode kernel (attn_drop_kernel) has no
// key-split-free form — training batches are small
inline int attn_slices(long long tt, bool with_dropout = false) {
    const long long wgs = tt * AP_HEADS;
    if (wgs <= 2048) return 8;
    if (with_dropout) return 4;
    return wgs <= 8192 ? 4 : 1;
}

}  // namespace audio_plan
}  // namespace said
