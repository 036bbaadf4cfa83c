// train_store.h — what the two trainer contexts (vae_trainer.cpp, unet_trainer.cpp) keep alike: the trainable tensors in one flat array with
// their gradients, AdamW moments and EMA shadow, the gradient-norm segments, the loss accumulators, and the update on them (train_opt.hip).
// The functions are called with the context's device current; a failure sets the owning context's error and returns -1.
#pragma once
#include "engine_internal.h"
#include "train_opt.h"

namespace said {
namespace host __attribute__((visibility("hidden"))) {

constexpr int TS_SEG = 8192;               // gradient-norm segment length
constexpr int TS_NACC = 8, TS_A_BAD = 5;   // doubles per accumulator set; the count of steps with a non-finite loss (both public headers)

struct TrainStore {
    HostCtx* ctx = nullptr;   // the owner of every allocation below (free_allocs releases them)
    long long nparam = 0;
    float *P = nullptr, *G = nullptr, *M = nullptr, *V = nullptr, *E = nullptr, *S = nullptr;   // S: the stash of EMAModel.store, optional
    long long* seg = nullptr;   // [nseg][3]: start, length, tensor; the segments of one tensor are consecutive
    int nseg = 0;
    double* part = nullptr;     // [nseg]
    float* clip = nullptr;      // factor, norm
    double* acc = nullptr;      // [2][TS_NACC]: training, validation
    float* last = nullptr;      // the 4 losses of the last step
};

// Lays tensors of `sizes` elements out one after the other (a size of 0: not a parameter; off[i]: tensor i's offset), cuts them into the
// gradient norm's segments and allocates everything.  Ends with a synchronous copy.
inline int store_build(TrainStore* st, HostCtx* ctx, const std::vector<long long>& sizes, bool stash, std::vector<long long>* off) {
    st->ctx = ctx;
    std::vector<long long> seg;
    off->assign(sizes.size(), 0);
    for (size_t i = 0; i < sizes.size(); ++i) {
        (*off)[i] = st->nparam;
        for (long long s0 = 0; s0 < sizes[i]; s0 += TS_SEG)
            seg.insert(seg.end(), {st->nparam + s0, std::min<long long>(TS_SEG, sizes[i] - s0), (long long)i});
        st->nparam += sizes[i];
    }
    st->nseg = (int)seg.size() / 3;
    const size_t n = (size_t)st->nparam;
    if (dalloc(ctx, &st->P, n) || dalloc(ctx, &st->G, n) || dalloc(ctx, &st->M, n) || dalloc(ctx, &st->V, n) || dalloc(ctx, &st->E, n) ||
        (stash && dalloc(ctx, &st->S, n)) || dalloc(ctx, &st->seg, seg.size()) || dalloc(ctx, &st->part, (size_t)st->nseg) ||
        dalloc(ctx, &st->clip, 2) || dalloc(ctx, &st->acc, (size_t)2 * TS_NACC) || dalloc(ctx, &st->last, 4))
        return -1;
    HIPCHK(hipMemcpy(st->seg, seg.data(), seg.size() * sizeof(long long), hipMemcpyHostToDevice));
    return 0;
}

// zero gradients and moments, the EMA shadow a copy of the parameters; synchronises s
inline int store_reset_optimizer(TrainStore* st, hipStream_t s) {
    HostCtx* ctx = st->ctx;
    const size_t bytes = (size_t)st->nparam * sizeof(float);
    HIPCHK(hipMemsetAsync(st->G, 0, bytes, s));
    HIPCHK(hipMemsetAsync(st->M, 0, bytes, s));
    HIPCHK(hipMemsetAsync(st->V, 0, bytes, s));
    HIPCHK(hipMemcpyAsync(st->E, st->P, bytes, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// copy `which` (STATE, EMA, GRAD, EXP_AVG, EXP_AVG_SQ, STASH, as both public headers number them) at offset `off`; nullptr if there is none
inline float* store_copy_of(const TrainStore* st, int which, long long off) {
    float* base[6] = {st->P, st->E, st->G, st->M, st->V, st->S};
    return (which >= 0 && which < 6 && base[which]) ? base[which] + off : nullptr;
}

// n floats dst <- src (a tensor's upload or download, or a whole copy onto another), enqueued on s; sync: wait for it
inline int store_copy(TrainStore* st, hipStream_t s, float* dst, const float* src, long long n, hipMemcpyKind kind, bool sync) {
    HostCtx* ctx = st->ctx;
    HIPCHK(hipMemcpyAsync(dst, src, n * sizeof(float), kind, s));
    if (sync) HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// clip, AdamW, EMA with the optimizer's slots of the device record `rec` (train_opt.h), enqueued on s
inline void store_enqueue_update(const TrainStore* st, hipStream_t s, const float* rec) {
    opt::grad_norm(s, st->nseg, st->seg, st->G, st->part, st->clip);
    opt::adamw_ema(s, st->nparam, st->P, st->G, st->M, st->V, st->E, st->clip, rec);
}

// the accumulators of the training steps (val = 0) or of the validation (val = 1) to acc_host, zeroed afterwards when reset; *status
// (nullable) = 1 when a step's loss was not finite, else 0; synchronises s
inline int store_read_losses(TrainStore* st, hipStream_t s, int val, double* acc_host, int* status, int reset) {
    HostCtx* ctx = st->ctx;
    double* a = st->acc + (val ? TS_NACC : 0);
    HIPCHK(hipMemcpyAsync(acc_host, a, TS_NACC * sizeof(double), hipMemcpyDeviceToHost, s));
    if (reset) HIPCHK(hipMemsetAsync(a, 0, TS_NACC * sizeof(double), s));
    HIPCHK(hipStreamSynchronize(s));
    if (status) *status = acc_host[TS_A_BAD] > 0;
    return 0;
}

}  // namespace host
}  // namespace said
