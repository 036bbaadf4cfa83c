// enc_gemm.h — the launcher of the fine-tuned audio encoder's dense products on split-fp16 operands (enc_gemm.hip), called by the trainer
// context (unet_trainer.cpp) when the context's encoder products are SAID_UT_PRODUCTS_SPLIT_F16 (said_unet_train_products.h).  The launcher
// only enqueues on `s`.  Everything is row-major fp32 with a leading dimension.  No atomics, fixed reduction orders: equal inputs give
// equal bits, whatever `part` and `amax` held before.
#pragma once
#include <hip/hip_runtime.h>

namespace said {
namespace eg __attribute__((visibility("hidden"))) {

// W is (N, K); M token rows
//   EG_FWD    c (M, N) = a (M, K) W^T + bias[n] (+ res) (+ c)        a = x,  b = W
//   EG_DGRAD  c (M, K) (+)= a (M, N) W                               a = dy, b = W       (a scaled, see below)
//   EG_WGRAD  c (N, K) = a^T (M, N) b (M, K), contraction over M     a = dy, b = x       (a scaled; K-split into `part` when KS > 1)
enum { EG_FWD = 0, EG_DGRAD = 1, EG_WGRAD = 2 };
constexpr int EG_TILE = 64;          // N and K must be multiples of it; M is arbitrary
constexpr int EG_AMAX_BLOCKS = 256;  // partial maxima of the gradient operand: `amax` holds this many

struct EncGemm {
    int layout;
    const float* a; int lda;
    const float* b; int ldb;
    float* c; int ldc;
    int M, N, K;
    const float* bias;          // EG_FWD only
    const float* res; int ldr;  // EG_FWD only
    int accumulate;             // EG_FWD, EG_DGRAD
    // EG_WGRAD: KS chunks of kchunk token rows (ut_gemm_plan.h ut_ksplit); KS > 1: partial tiles part[ks][n][k], added in ascending chunk
    // order by unet_train.hip's gemm_reduce
    int KS, kchunk;
    float* part;
    // the gradient operand a of EG_DGRAD / EG_WGRAD (dense: lda == N) is multiplied by a power of two before it is split, so that its largest
    // magnitude lies in [2^14, 2^15), and the result by the inverse; amax: EG_AMAX_BLOCKS words of scratch
    unsigned* amax;
};
// whether the kernel takes the weight's shape
constexpr bool enc_gemm_takes(int N, int K) { return N > 0 && K > 0 && N % EG_TILE == 0 && K % EG_TILE == 0; }
void enc_gemm(hipStream_t s, const EncGemm& g);

}  // namespace eg
}  // namespace said
