// vae_dec.hip — BCVAE decoder (said/model/vae.py:115-170) as one fused launch, eval mode, fp32 VALU throughout.
//
//   z (64) -> Linear 64->240 [+BN folded] -> LeakyReLU(0.01) -> Linear 240->480 -> Unflatten (4, 120)
//          -> ConvT 4->32 k3 [+BN] -> LReLU(0.2) -> ConvT 32->32 k3 [+BN] -> LReLU(0.2) -> Conv 32->32 k3 -> Conv 32->32 k3
//          -> ReLU -> Tanh -> (120, 32) token-major
//
// The host (engine.cpp, said_vae_finalize_weights) folds the BatchNorms and rewrites each stride-1 ConvTranspose1d as a Conv1d
// with the kernel transposed and flipped over an input zero-padded by k-1 = 2 on each side, so all four convolutions are the
// same "valid" Conv1d below.  Weight layouts (packed on the host):
//   fc1_w [64][240], fc2_w [240][480]   (input-major: thread o reads column o, coalesced across the workgroup)
//   conv_w[l] [cin][32][3]              (cin-major: the 8 output channels x 3 taps one wave needs for one cin are 24
//                                        consecutive floats at a wave-uniform address -> scalar loads)
//
// One workgroup = 256 threads = 4 waves owns VD_WPB windows; their activations stay in LDS from the FC output to the final
// store (two ping-pong buffers of 32 channels x VD_PITCH positions per window).  In a convolution wave q computes output
// channels 8q..8q+7 and lane l positions l and l + 64 of every window; weights come from the scalar cache, inputs are
// conflict-free ds_read_b32 of consecutive positions.  Positions >= L_out are computed (their reads stay inside the row
// pitch) and discarded.  The last convolution's ReLU/tanh results are staged in LDS token-major (pitch 33: conflict-free)
// and leave as whole 16-byte rows of the (n, 120, 32) output.
#include "kernels.h"

namespace said {

namespace {

constexpr int VD_WPB = 2;                  // windows per workgroup
constexpr int VD_PITCH = 132;              // LDS row pitch (floats): >= 128 + 2 (widest tap read of a discarded lane)
constexpr int VD_BUF = 32 * VD_PITCH;      // one window's 32-channel buffer
constexpr int VD_TM = 33;                  // token-major staging pitch of the last layer (120 x 33 <= VD_BUF)
constexpr int VD_Z = 64, VD_H1 = 240, VD_H2 = 480, VD_L = 120;

enum VdAct { VD_LRELU02 = 0, VD_NONE = 1, VD_RELU_TANH = 2 };

// valid Conv1d, 32 output channels, kernel 3: out[w][co][off + t] = act(b[co] + sum_ci sum_k W[ci][co][k] in[w][ci][t + k]),
// t < Lout.  TM: store token-major into out[w][t * VD_TM + co] instead.
template <int CIN, int ACT, bool TM>
__device__ __forceinline__ void conv3(const float* __restrict__ W, const float* __restrict__ B, const float* in, float* out, int off, int Lout) {
    const int q = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int co0 = q * 8;
    float acc[VD_WPB][2][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float b = B[co0 + j];
#pragma unroll
        for (int w = 0; w < VD_WPB; ++w) {
            acc[w][0][j] = b;
            acc[w][1][j] = b;
        }
    }
#pragma unroll 2
    for (int ci = 0; ci < CIN; ++ci) {
        const float* wr = W + (ci * 32 + co0) * 3;
        float wv[24];
#pragma unroll
        for (int i = 0; i < 24; ++i) wv[i] = wr[i];
#pragma unroll
        for (int w = 0; w < VD_WPB; ++w) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float* x = in + w * VD_BUF + ci * VD_PITCH + lane + 64 * h;
                const float x0 = x[0], x1 = x[1], x2 = x[2];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float a = acc[w][h][j];
                    a = __builtin_fmaf(wv[j * 3 + 0], x0, a);
                    a = __builtin_fmaf(wv[j * 3 + 1], x1, a);
                    a = __builtin_fmaf(wv[j * 3 + 2], x2, a);
                    acc[w][h][j] = a;
                }
            }
        }
    }
#pragma unroll
    for (int w = 0; w < VD_WPB; ++w) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int t = lane + 64 * h;
            if (t < Lout) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float v = acc[w][h][j];
                    if (ACT == VD_LRELU02) v = v > 0.f ? v : 0.2f * v;
                    if (ACT == VD_RELU_TANH) v = tanhf(fmaxf(v, 0.f));
                    if (TM) out[w * VD_BUF + t * VD_TM + co0 + j] = v;
                    else out[w * VD_BUF + (co0 + j) * VD_PITCH + off + t] = v;
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void vae_decode_kernel(VaeDecWeights P, const float* __restrict__ mean, const float* __restrict__ logvar,
                                                         const float* __restrict__ eps, int n, float* __restrict__ out) {
    __shared__ float A[VD_WPB * VD_BUF];
    __shared__ float Bf[VD_WPB * VD_BUF];
    __shared__ float Z[VD_WPB * VD_Z];
    __shared__ float H1[VD_WPB * VD_H1];
    const int tid = threadIdx.x;
    const long long win0 = (long long)blockIdx.x * VD_WPB;
    const int nw = (int)min((long long)VD_WPB, (long long)n - win0);

    // zero padding of the two transposed convolutions' inputs: Bf channels 0..3 at positions 0, 1, 122, 123 (FC2 output,
    // length 120 at offset 2); A all channels at 0, 1, 124, 125 (ConvT1 output, length 122 at offset 2)
    for (int i = tid; i < VD_WPB * 32 * 4; i += 256) {
        const int w = i / 128, c = (i >> 2) & 31, p = i & 3;
        A[w * VD_BUF + c * VD_PITCH + (p < 2 ? p : 122 + p)] = 0.f;
        if (c < 4) Bf[w * VD_BUF + c * VD_PITCH + (p < 2 ? p : 120 + p)] = 0.f;
    }
    // latent, with the reparametrisation z = mean + exp(0.5 log_var) eps when eps is given (vae.py:106-110)
    for (int i = tid; i < VD_WPB * VD_Z; i += 256) {
        const int w = i / VD_Z;
        float z = 0.f;
        if (w < nw) {
            const long long g = (win0 + w) * VD_Z + (i % VD_Z);
            z = mean[g];
            if (eps) z = z + expf(0.5f * logvar[g]) * eps[g];
        }
        Z[i] = z;
    }
    __syncthreads();
    // Linear 64 -> 240 (+BN folded) + LeakyReLU(0.01)
    if (tid < VD_H1) {
        float acc[VD_WPB];
        const float b = P.fc1_b[tid];
#pragma unroll
        for (int w = 0; w < VD_WPB; ++w) acc[w] = b;
        for (int i = 0; i < VD_Z; ++i) {
            const float wt = P.fc1_w[i * VD_H1 + tid];
#pragma unroll
            for (int w = 0; w < VD_WPB; ++w) acc[w] = __builtin_fmaf(wt, Z[w * VD_Z + i], acc[w]);
        }
#pragma unroll
        for (int w = 0; w < VD_WPB; ++w) H1[w * VD_H1 + tid] = acc[w] > 0.f ? acc[w] : 0.01f * acc[w];
    }
    __syncthreads();
    // Linear 240 -> 480, Unflatten (4, 120): output o -> channel o / 120, position 2 + o % 120 of Bf
    {
        const int o0 = tid, o1 = tid + 256;
        const int o1c = o1 < VD_H2 ? o1 : VD_H2 - 1;   // lanes past 480 read a valid column and discard it
        float a0[VD_WPB], a1[VD_WPB];
        const float b0 = P.fc2_b[o0], b1 = P.fc2_b[o1c];
#pragma unroll
        for (int w = 0; w < VD_WPB; ++w) { a0[w] = b0; a1[w] = b1; }
#pragma unroll 4
        for (int i = 0; i < VD_H1; ++i) {
            const float w0 = P.fc2_w[i * VD_H2 + o0], w1 = P.fc2_w[i * VD_H2 + o1c];
#pragma unroll
            for (int w = 0; w < VD_WPB; ++w) {
                const float h = H1[w * VD_H1 + i];
                a0[w] = __builtin_fmaf(w0, h, a0[w]);
                a1[w] = __builtin_fmaf(w1, h, a1[w]);
            }
        }
#pragma unroll
        for (int w = 0; w < VD_WPB; ++w) {
            Bf[w * VD_BUF + (o0 / VD_L) * VD_PITCH + 2 + o0 % VD_L] = a0[w];
            if (o1 < VD_H2) Bf[w * VD_BUF + (o1 / VD_L) * VD_PITCH + 2 + o1 % VD_L] = a1[w];
        }
    }
    __syncthreads();
    conv3<4, VD_LRELU02, false>(P.conv_w[0], P.conv_b[0], Bf, A, 2, 122);    // ConvT 4->32 (+BN) + LReLU(0.2), into A[2, 124)
    __syncthreads();
    conv3<32, VD_LRELU02, false>(P.conv_w[1], P.conv_b[1], A, Bf, 0, 124);   // ConvT 32->32 (+BN) + LReLU(0.2)
    __syncthreads();
    conv3<32, VD_NONE, false>(P.conv_w[2], P.conv_b[2], Bf, A, 0, 122);      // Conv 32->32
    __syncthreads();
    conv3<32, VD_RELU_TANH, true>(P.conv_w[3], P.conv_b[3], A, Bf, 0, VD_L); // Conv 32->32, ReLU, Tanh, token-major staging
    __syncthreads();
    // (120, 32) per window, 16-byte stores (the host checks `out`'s alignment; a window is 15360 bytes)
    float4* o4 = reinterpret_cast<float4*>(out + win0 * (VD_L * 32));
    for (int i = tid; i < nw * (VD_L * 8); i += 256) {
        const int w = i / (VD_L * 8), r = i % (VD_L * 8);
        const int t = r >> 3, c = (r & 7) * 4;
        const float* s = Bf + w * VD_BUF + t * VD_TM + c;
        o4[i] = make_float4(s[0], s[1], s[2], s[3]);
    }
}

}  // namespace

void launch_vae_decode(const VaeDecWeights& w, const float* mean, const float* logvar, const float* eps, int n, float* out, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(vae_decode_kernel, dim3((n + VD_WPB - 1) / VD_WPB), dim3(256), 0, s, w, mean, logvar, eps, n, out);
}

}  // namespace said
