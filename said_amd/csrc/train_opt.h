// train_opt.h — the optimizer update both trainers run (train_opt.hip): the global gradient-norm clip, AdamW and the EMA shadow over one flat
// parameter array (train_store.h).  The launchers only enqueue on `s`: the BCVAE's step is captured into a hipGraph with them in it.
#pragma once
#include <hip/hip_runtime.h>

namespace said {
namespace opt __attribute__((visibility("hidden"))) {

// the optimizer's slots of a step record: the same in SAID_TRAIN_S_* (include/said_train.h) and SAID_UT_S_* (include/said_unet_train.h)
enum { S_WD_FACTOR = 1, S_STEP_SIZE, S_BC2_SQRT, S_EMA_OMD, S_OMB1 = 7, S_B2, S_OMB2, S_EPS, S_USE_EMA };
// static_assert(OPT_SLOTS_MATCH(SAID_TRAIN_S_)): a trainer's public record has the optimizer's slots where the kernel reads them
#define OPT_SLOTS_MATCH(P)                                                                                                              \
    (P##WD_FACTOR == said::opt::S_WD_FACTOR && P##STEP_SIZE == said::opt::S_STEP_SIZE && P##BC2_SQRT == said::opt::S_BC2_SQRT &&         \
     P##EMA_OMD == said::opt::S_EMA_OMD && P##OMB1 == said::opt::S_OMB1 && P##B2 == said::opt::S_B2 && P##OMB2 == said::opt::S_OMB2 &&   \
     P##EPS == said::opt::S_EPS && P##USE_EMA == said::opt::S_USE_EMA)

// squared 2-norms of the gradient segments (seg[3 s + 0..2]: start, length, tensor; the segments of one tensor are consecutive), then the clip
// factor min(1, 1 / (norm + 1e-6)) into clip[0] (clip[1]: the norm)
void grad_norm(hipStream_t s, int nseg, const long long* seg, const float* G, double* part, float* clip);
// AdamW (torch.optim.AdamW, single-tensor form) on clip[0] * G, then the EMA shadow
void adamw_ema(hipStream_t s, long long n, float* P, const float* G, float* M, float* V, float* E, const float* clip, const float* rec);

}  // namespace opt
}  // namespace said
