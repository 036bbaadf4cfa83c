// train_dev.h — device code shared by the training kernels (vae_train.hip, unet_train.hip, train_opt.hip): the workgroup size and the
// fixed-order sums.  A thread's own sum runs in index order, a wave's lanes are combined by a fixed xor butterfly, a workgroup's threads by
// a fixed LDS tree: equal inputs give equal bits.
#pragma once
#include <hip/hip_runtime.h>

namespace said {

constexpr int NT = 256;   // threads per workgroup of every training kernel

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum of one value per thread of a 256-thread workgroup, the same order every call; every thread gets the result
template <typename F>
__device__ __forceinline__ F block_sum(F v, F* sh) {
    const int t = threadIdx.x;
    __syncthreads();
    sh[t] = v;
    __syncthreads();
    for (int w = NT / 2; w >= 1; w >>= 1) {
        if (t < w) sh[t] = sh[t] + sh[t + w];
        __syncthreads();
    }
    return sh[0];
}

inline int nblk(long long n, int per = NT) { return (int)((n + per - 1) / per); }

}  // namespace said
