// ut_gemm_plan.h — the host-side K-split decisions of the training step's gemm_kernel (unet_train.hip; launched by unet_trainer.cpp), host-only:
// how many k chunks a weight gradient runs on and how long a chunk is (ut_ksplit), the short-batch split of the positional convolution
// (ut_split_small), and the size of the partial-tile buffer both write (ut_gpart_n).  A header of its own so that tests can ask it without a
// GPU (tests/ut_gemm_plan_main.cpp), as rgemm_plan.h and ugemm_plan.h are for the inference GEMMs.
//
// Chunk ks of a split product covers k in [ks kchunk, min(K, (ks + 1) kchunk)).  kchunk is a multiple of the kernel's 16-wide k tile, so
// rounding it up can leave the LAST chunk empty (first at K = 1281: 10 chunks of 144 cover 1296 in nine).  gemm_kernel then runs no k tile
// and stores an all-zero partial tile, which gemm_reduce_kernel adds like every other.
#pragma once
#include <algorithm>
#include <cstddef>

namespace said {
namespace ut {

constexpr int UT_MAXKS = 16;        // chunks of a weight gradient at most
constexpr int UT_KS_PER = 128;      // one chunk per 128 of K
constexpr int UT_SMALL_KS = 8;      // the positional convolution's split at a short batch
constexpr int UT_SMALL_M = 256;     // ... taken up to this many tokens
// the widths gpart is sized for: the UNet's widest weight gradient is (max(768, F), 768); the fine-tuned encoder's positional convolution
// is 16 groups of (48, 48 x 128)
constexpr int UT_TED = 768, UT_EH = 768, UT_EPG = 16, UT_EPC = UT_EH / UT_EPG, UT_EPK = 128;

struct UtSplit { int KS, kchunk; };

inline int ut_rup(int a, int b) { return (a + b - 1) / b * b; }
inline int ut_kchunk(int K, int ks) { return ut_rup((std::max(K, 1) + ks - 1) / ks, 16); }
inline UtSplit ut_unsplit(int K) { return UtSplit{1, ut_kchunk(K, 1)}; }

// the chunk count of a weight gradient before the capacity is looked at
inline int ut_ksplit_want(int K) { return std::min(UT_MAXKS, std::max(1, K / UT_KS_PER)); }
// the weight gradients: few tiles, long K.  KS chunks write KS Z M N partial floats; KS is lowered until they fit into `capacity` floats
// (no product of any tensor table needs that: tests/test_ut_gemm_plan_cpu.py)
inline UtSplit ut_ksplit(int K, int M, int N, int Z, size_t capacity) {
    int ks = ut_ksplit_want(K);
    while (ks > 1 && (size_t)ks * Z * M * N > capacity) --ks;
    return UtSplit{ks, ut_kchunk(K, ks)};
}
// a short batch of the grouped positional convolution (M tokens): split K = 128 x 48 eight ways so that more than 16 workgroups run
inline UtSplit ut_split_small(int K, int M, int N, int Z, size_t capacity) {
    if (M <= UT_SMALL_M && (size_t)UT_SMALL_KS * Z * M * N <= capacity) return UtSplit{UT_SMALL_KS, ut_kchunk(K, UT_SMALL_KS)};
    return ut_unsplit(K);
}
// floats of the partial-tile buffer of a context with feature_dim F (<= 0: none) and L fine-tuned encoder layers (<= 0: frozen encoder)
inline size_t ut_gpart_n(int F, int L) {
    if (L > 0) return (size_t)UT_MAXKS * UT_EH * UT_EPC * UT_EPK;
    return (size_t)UT_MAXKS * std::max(UT_TED, F) * UT_TED;
}

}  // namespace ut
}  // namespace said
