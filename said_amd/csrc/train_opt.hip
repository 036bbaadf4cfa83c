// train_opt.hip — the optimizer update of both trainers (vae_trainer.cpp, unet_trainer.cpp through train_store.h): the global gradient-norm
// clip (torch.nn.utils.clip_grad_norm_), AdamW (torch.optim.AdamW, single-tensor form) and the EMA shadow (diffusers EMAModel.step).  fp32 state,
// the norm in double.  No atomics; every sum runs in a fixed order (train_dev.h), so equal inputs give bit-identical outputs.
#include "train_opt.h"

#include <math.h>

#include <algorithm>

#include "train_dev.h"

namespace said {
namespace opt {
namespace {

// seg[3 s + 0..2] = start, length, tensor; segments of one tensor are consecutive
__global__ void __launch_bounds__(NT) grad_sq_kernel(const long long* __restrict__ seg, const float* __restrict__ G, double* __restrict__ part) {
    __shared__ double sh[NT];
    const long long st = seg[3 * blockIdx.x], n = seg[3 * blockIdx.x + 1];
    double q = 0.0;
    for (long long i = threadIdx.x; i < n; i += NT) {
        const double g = G[st + i];
        q += g * g;
    }
    q = block_sum(q, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = q;
}

// torch.nn.utils.clip_grad_norm_(max_norm=1): total = |(|g_0|, |g_1|, ...)|, factor min(1, 1 / (total + 1e-6)), applied always
__global__ void __launch_bounds__(64) clip_kernel(int nseg, const long long* __restrict__ seg, const double* __restrict__ part, float* __restrict__ clip) {
    if (threadIdx.x != 0) return;
    double tot = 0.0, cur = 0.0;
    for (int s = 0; s < nseg; ++s) {
        cur += part[s];
        if (s + 1 == nseg || seg[3 * (s + 1) + 2] != seg[3 * s + 2]) {
            const float nt = (float)sqrt(cur);   // per-tensor norm in fp32
            tot += (double)nt * (double)nt;
            cur = 0.0;
        }
    }
    const float total = (float)sqrt(tot);
    const float f = 1.f / (total + 1e-6f);
    clip[0] = f < 1.f ? f : 1.f;
    clip[1] = total;
}

__global__ void __launch_bounds__(NT) adamw_ema_kernel(long long n, float* __restrict__ P, const float* __restrict__ G, float* __restrict__ M,
                                                       float* __restrict__ V, float* __restrict__ E, const float* __restrict__ clip,
                                                       const float* __restrict__ rec) {
    const float cf = clip[0], wdf = rec[S_WD_FACTOR], ss = rec[S_STEP_SIZE], bc2 = rec[S_BC2_SQRT], omb1 = rec[S_OMB1], b2 = rec[S_B2],
                omb2 = rec[S_OMB2], eps = rec[S_EPS], omd = rec[S_EMA_OMD];
    const bool ema = rec[S_USE_EMA] != 0.f;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT) {
        const float g = G[i] * cf;
        float p = P[i] * wdf;                         // param.mul_(1 - lr wd)
        const float m = M[i] + omb1 * (g - M[i]);     // exp_avg.lerp_(grad, 1 - beta1)
        const float v = V[i] * b2 + (omb2 * g) * g;   // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
        const float den = sqrtf(v) / bc2 + eps;       // exp_avg_sq.sqrt() / bias_correction2_sqrt + eps
        p = p + (-ss) * (m / den);                    // param.addcdiv_(exp_avg, denom, -lr / bias_correction1)
        P[i] = p;
        M[i] = m;
        V[i] = v;
        if (ema) E[i] = E[i] - omd * (E[i] - p);      // diffusers EMAModel.step: s -= (1 - decay)(s - p)
    }
}

}  // namespace

void grad_norm(hipStream_t s, int nseg, const long long* seg, const float* G, double* part, float* clip) {
    grad_sq_kernel<<<nseg, NT, 0, s>>>(seg, G, part);
    clip_kernel<<<1, 64, 0, s>>>(nseg, seg, part, clip);
}
void adamw_ema(hipStream_t s, long long n, float* P, const float* G, float* M, float* V, float* E, const float* clip, const float* rec) {
    adamw_ema_kernel<<<std::min(nblk(n), 1024), NT, 0, s>>>(n, P, G, M, V, E, clip, rec);
}

}  // namespace opt
}  // namespace said
