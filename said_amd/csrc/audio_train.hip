// audio_train.hip — the kernels of the audio encoder's train mode (include/said_audio_train.h): self-attention with dropout on the
// probabilities, LayerNorm over a residual sum with dropout in front of or behind it, and the in-place dropout (+ SpecAugment span
// replacement) of a channel-major activation.  All on the fp32 channel-major route of audio_enc.cpp; the inference kernels are not touched.
//
// Dropout masks are never stored: Philox4x32-10 (sched_math.h) with key = the call's seed, one call per four elements, the rule of
// unet_train.hip's drop_factor: u = (word >> 8) 2^-24, kept iff u >= p, a kept element times the fp32 value of 1 / (1 - p).
//   element-wise sites: e = logical index in (B, T, C); counter (site, e >> 2, 0, 0), word e & 3
//   probabilities:      counter (site, (b 12 + head) T + i, j >> 2, 0), word j & 3
// Both depend on logical indices only, so a mask is independent of the chunking over clips, the key split and every tile shape.
#include "audio_train.h"
#include "sched_math.h"
#include "split_f16.h"

namespace said {

// the keep factors of the four elements that Philox counter (site, c1, c2, 0) serves
static __device__ __forceinline__ void drop4(unsigned k0, unsigned k1, int site, unsigned c1, unsigned c2, float p, float keep, float (&f)[4]) {
    unsigned r[4];
    philox4x32_10((unsigned)site, c1, c2, 0u, k0, k1, r);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = ((float)(r[e] >> 8) * 5.9604644775390625e-8f >= p) ? keep : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------
// attn_drop_kernel — attn.hip's attn_kernel<2, KS, PM> (head_dim 64, keys split over the workgroup's KS waves, states merged through
// LDS in wave order) with dropout on the normalised probabilities.  The scores are computed transposed, S^T[j][i], so a lane owns ONE
// query (i = i0 + (lane & 31)) and accumulator register r of key tile j0 is key j0 + (r & 3) + 8 (r >> 2) + 4 (lane >> 5): the four
// registers of quadruple r >> 2 are the four words of Philox counter (site, row(b, head, i), (j0 >> 2) + 2 (r >> 2) + (lane >> 5), 0).
// The running sum takes the UNDROPPED exp (the softmax denominator is over all keys); the masked, rescaled value is what the second
// product multiplies with V.  A kernel of its own rather than another template parameter of attn_kernel: that file is compiled with
// kernarg preloading and register budgets that inference depends on.
struct AttnDropParams {
    const float* qk; const float* v; float* o;
    int v_bstride, o_bstride, pitch, T, heads, rows;
    float scale;
    int b_global;
    unsigned k0, k1;
    int site;
    float p, keep;
};
template <int KS, int PM>
__global__ __launch_bounds__(64 * KS, (64 * KS <= 256) ? 2 : 1) void attn_drop_kernel(const AttnDropParams a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int ND = 2, D = 64, NQ = D / 8;
    constexpr bool SP = PM == 2;
    const int tid = threadIdx.x, l = tid & 63, lt = l & 31, lh = l >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i0 = blockIdx.x * 32, h = blockIdx.y, b = blockIdx.z;
    const int T = a.T, pitch = a.pitch, H = a.heads, rows = a.rows;
    const float* qb = a.qk + (((long long)b * 2 * H + h) * rows) * D + lh * (D / 2);
    const float* kb = a.qk + (((long long)b * 2 * H + H + h) * rows) * D + lh * (D / 2);
    const float* vb = a.v + (long long)b * a.v_bstride + (long long)(h * D + lt) * pitch + 4 * lh;
    const unsigned prow = ((unsigned)(a.b_global + b) * (unsigned)H + (unsigned)h) * (unsigned)T + (unsigned)(i0 + lt);   // (< 2^32 for i < T: checked by the host)

    f32x4 qf[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) qf[q] = *reinterpret_cast<const f32x4*>(qb + (long long)min(i0 + lt, rows - 1) * D + 4 * q);
    SplitH qs[NQ / 2];
#pragma unroll
    for (int q = 0; q < NQ / 2; ++q) qs[q] = split_f16x8(qf[2 * q], qf[2 * q + 1]);
    float m = -1.0e30f, lsum = 0.f;
    f32x16 o[ND], ox[SP ? ND : 1];
#pragma unroll
    for (int nd = 0; nd < ND; ++nd)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            o[nd][r] = 0.f;
            if (SP) ox[SP ? nd : 0][r] = 0.f;
        }

    const int nkt = (T + 31) >> 5;
    for (int kt = w; kt < nkt; kt += KS) {
        const int j0 = kt * 32;
        f32x4 kf[NQ], vf[ND][4];
#pragma unroll
        for (int q = 0; q < NQ; ++q) kf[q] = *reinterpret_cast<const f32x4*>(kb + (long long)(j0 + lt) * D + 4 * q);
#pragma unroll
        for (int nd = 0; nd < ND; ++nd)
#pragma unroll
            for (int q = 0; q < 4; ++q) vf[nd][q] = *reinterpret_cast<const f32x4*>(vb + (long long)(nd * 32) * pitch + j0 + 8 * q);
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        if constexpr (SP) {
            SplitH ks[NQ / 2];
#pragma unroll
            for (int q = 0; q < NQ / 2; ++q) ks[q] = split_f16x8(kf[2 * q], kf[2 * q + 1]);
            operand_fence();
            f32x16 sxa;
#pragma unroll
            for (int r = 0; r < 16; ++r) sxa[r] = 0.f;
#pragma unroll
            for (int q = 0; q < NQ / 2; ++q) {
                sxa = __builtin_amdgcn_mfma_f32_32x32x16_f16(ks[q].l, qs[q].h, sxa, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_32x32x16_f16(ks[q].h, qs[q].h, s, 0, 0, 0);
                sxa = __builtin_amdgcn_mfma_f32_32x32x16_f16(ks[q].h, qs[q].l, sxa, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = fmaf(sxa[r], 0x1p-11f, s[r]);
        } else {
#pragma unroll
            for (int dp = 0; dp < ND * 16; ++dp) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[dp >> 2][dp & 3], qf[dp >> 2][dp & 3], s, 0, 0, 0);
        }
        // online softmax in the reference's op order (scale, subtract the maximum, exp); keys past T only exist in the last tile
        float mx = -1.0e30f;
        const bool tail = j0 + 32 > T;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            s[r] = (!tail || j < T) ? s[r] * a.scale : -1.0e30f;
            mx = fmaxf(mx, s[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(m, mx);
        const float alpha = __expf(m - mn);
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __expf(s[r] - mn);
            ps += s[r];
        }
        lsum = lsum * alpha + ps;   // the undropped terms
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {
#pragma unroll
            for (int nd = 0; nd < ND; ++nd)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    o[nd][r] *= alpha;
                    if (SP) ox[SP ? nd : 0][r] *= alpha;
                }
        }
        // dropout: one Philox call per register quadruple (four consecutive keys)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float f[4];
            drop4(a.k0, a.k1, a.site, prow, (unsigned)(j0 >> 2) + 2 * q + lh, a.p, a.keep, f);
#pragma unroll
            for (int e = 0; e < 4; ++e) s[4 * q + e] *= f[e];
        }
        // never-written columns of v (keys past T) are zeroed: their probabilities are 0, but 0 x NaN is NaN
        if (tail) {
#pragma unroll
            for (int nd = 0; nd < ND; ++nd)
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) vf[nd][q][e] = (j0 + 8 * q + 4 * lh + e < T) ? vf[nd][q][e] : 0.f;
        }
        if constexpr (SP) {
            SplitH psa[2], vsa[2][ND];
#pragma unroll
            for (int m8 = 0; m8 < 2; ++m8) {
                const f32x4 p0 = {s[8 * m8], s[8 * m8 + 1], s[8 * m8 + 2], s[8 * m8 + 3]}, p1 = {s[8 * m8 + 4], s[8 * m8 + 5], s[8 * m8 + 6], s[8 * m8 + 7]};
                psa[m8] = split_f16x8(p0, p1);
#pragma unroll
                for (int nd = 0; nd < ND; ++nd) vsa[m8][nd] = split_f16x8(vf[nd][2 * m8], vf[nd][2 * m8 + 1]);
            }
            operand_fence();
#pragma unroll
            for (int m8 = 0; m8 < 2; ++m8)
#pragma unroll
                for (int nd = 0; nd < ND; ++nd) {
                    ox[nd] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vsa[m8][nd].l, psa[m8].h, ox[nd], 0, 0, 0);
                    o[nd] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vsa[m8][nd].h, psa[m8].h, o[nd], 0, 0, 0);
                    ox[nd] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vsa[m8][nd].h, psa[m8].l, ox[nd], 0, 0, 0);
                }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int nd = 0; nd < ND; ++nd) o[nd] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[nd][r >> 2][r & 3], s[r], o[nd], 0, 0, 0);
        }
    }
    lsum += __shfl_xor(lsum, 32);
    if constexpr (SP) {
#pragma unroll
        for (int nd = 0; nd < ND; ++nd)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[nd][r] = fmaf(ox[nd][r], 0x1p-11f, o[nd][r]);
    }

    // ---- merge the KS partial states, in wave order ----
    float* ml = smem;                 // [KS][2][32]
    float* ob = smem + KS * 64;       // [KS][ND][16][64]
    if (lh == 0) {
        ml[(w * 2 + 0) * 32 + lt] = m;
        ml[(w * 2 + 1) * 32 + lt] = lsum;
    }
#pragma unroll
    for (int nd = 0; nd < ND; ++nd)
#pragma unroll
        for (int r = 0; r < 16; ++r) ob[((w * ND + nd) * 16 + r) * 64 + l] = o[nd][r];
    __syncthreads();
    float M = -1.0e30f;
#pragma unroll
    for (int w2 = 0; w2 < KS; ++w2) M = fmaxf(M, ml[(w2 * 2) * 32 + lt]);
    float f[KS];
    float L = 0.f;
#pragma unroll
    for (int w2 = 0; w2 < KS; ++w2) {
        f[w2] = __expf(ml[(w2 * 2) * 32 + lt] - M);
        L += ml[(w2 * 2 + 1) * 32 + lt] * f[w2];
    }
    const float invL = 1.0f / L;
    constexpr int NV = ND * 16;
    static_assert(NV % KS == 0, "");
    float* ob_out = a.o + (long long)b * a.o_bstride + (long long)(h * D) * pitch;
#pragma unroll
    for (int jv = 0; jv < NV / KS; ++jv) {
        const int v = w + jv * KS;
        const int nd = v >> 4, r = v & 15;
        float acc = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < KS; ++w2) acc += ob[((w2 * ND + nd) * 16 + r) * 64 + l] * f[w2];
        const int d = nd * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const int i = i0 + lt;
        if (i < T) ob_out[(long long)d * pitch + i] = acc * invL;
    }
}

template <int KS, int PM>
static void launch_attn_drop_one(const AttnDropParams& p, int batch, hipStream_t s) {
    const int smem = (KS * 64 + KS * 2 * 16 * 64) * (int)sizeof(float);
    dim3 grid((p.T + 31) / 32, p.heads, batch);
    hipLaunchKernelGGL((attn_drop_kernel<KS, PM>), grid, dim3(64 * KS), smem, s, p);
}
template <int KS, int PM>
static void configure_attn_drop_one() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_drop_kernel<KS, PM>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}
void configure_audio_train_kernels() {
    configure_attn_drop_one<8, 0>(); configure_attn_drop_one<4, 0>(); configure_attn_drop_one<8, 2>(); configure_attn_drop_one<4, 2>();
}
void launch_attn_drop(const AttnArgs& a, int batch, int KS, hipStream_t s, int mode, int b_global, const DropSite& d) {
    if (a.v_bstride > 0x7fffffffLL || a.o_bstride > 0x7fffffffLL) { launch_fault("attention batch stride exceeds 31 bits"); return; }
    if (a.b0 != 0 || a.o_mode != 0 || (KS != 8 && KS != 4) || (mode != 0 && mode != 2) || !(d.p > 0.f)) {
        launch_fault("attention with dropout: unsupported config KS=%d mode=%d", KS, mode);
        return;
    }
    const AttnDropParams p = {a.qk, a.v, a.o, (int)a.v_bstride, (int)a.o_bstride, a.pitch, a.T, a.heads, a.rows, a.scale, b_global,
                              (unsigned)(d.seed & 0xFFFFFFFFull), (unsigned)(d.seed >> 32), d.site, d.p, d.keep};
    if (KS == 8) mode == 2 ? launch_attn_drop_one<8, 2>(p, batch, s) : launch_attn_drop_one<8, 0>(p, batch, s);
    else mode == 2 ? launch_attn_drop_one<4, 2>(p, batch, s) : launch_attn_drop_one<4, 0>(p, batch, s);
}

// ------------------------------------------------------------------------------------------------------------------
// ln_drop_cm_kernel — misc.hip's layernorm_cm_kernel (one workgroup = 16 tokens x all C channels, the tile kept in LDS, exact mean
// first, then the shifted second moment) over v = res + pre(x), the result through post().  A thread takes four consecutive channels
// per pass, the four words of one Philox call.  Serves the encoder front (res = the positional embedding, post = the hidden dropout)
// and both LayerNorms of a layer (pre = the hidden dropout on the out_proj / FFN output, whose GEMMs then run without their residual).
constexpr int LND_TT = 16;
struct DropK { unsigned k0, k1; int site; float p, keep; };
static DropK drop_k(const DropSite& d) { return DropK{(unsigned)(d.seed & 0xFFFFFFFFull), (unsigned)(d.seed >> 32), d.site, d.p, d.keep}; }

__global__ __launch_bounds__(256) void ln_drop_cm_kernel(const float* __restrict__ x, const float* __restrict__ res, float* __restrict__ y,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, int C, int T, int pitch,
                                                         long long bstride, float eps, int b_global, const DropK pre, const DropK post) {
    extern __shared__ float tile[];            // [C][LND_TT + 1]
    __shared__ float red[16][LND_TT];
    __shared__ float stat[2][LND_TT];
    const int b = blockIdx.y, t0 = blockIdx.x * LND_TT;
    const int tx = threadIdx.x & (LND_TT - 1), cy = threadIdx.x / LND_TT;   // 16 channel quadruples per pass
    const int t = min(t0 + tx, T - 1);
    const float* xb = x + (long long)b * bstride + t;
    const float* rb = res + (long long)b * bstride + t;
    const unsigned e4 = ((unsigned)(b_global + b) * (unsigned)T + (unsigned)t) * (unsigned)(C >> 2);   // (logical index of channel 0) >> 2
    float s = 0.f;
    for (int c4 = cy; c4 < (C >> 2); c4 += 16) {
        float f[4] = {1.f, 1.f, 1.f, 1.f};
        if (pre.p > 0.f) drop4(pre.k0, pre.k1, pre.site, e4 + c4, 0u, pre.p, pre.keep, f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * c4 + e;
            float v = xb[(long long)c * pitch];
            if (pre.p > 0.f) v *= f[e];
            v = rb[(long long)c * pitch] + v;
            tile[c * (LND_TT + 1) + tx] = v;
            s += v;
        }
    }
    red[cy][tx] = s;
    __syncthreads();
    if (threadIdx.x < LND_TT) {
        float tot = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) tot += red[g][threadIdx.x];
        stat[0][threadIdx.x] = tot / (float)C;
    }
    __syncthreads();
    const float mean = stat[0][tx];
    float q = 0.f;
    for (int c4 = cy; c4 < (C >> 2); c4 += 16)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = tile[(4 * c4 + e) * (LND_TT + 1) + tx] - mean;
            q = fmaf(d, d, q);
        }
    red[cy][tx] = q;
    __syncthreads();
    if (threadIdx.x < LND_TT) {
        float tot = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) tot += red[g][threadIdx.x];
        stat[1][threadIdx.x] = 1.0f / sqrtf(tot / (float)C + eps);
    }
    __syncthreads();
    const float rstd = stat[1][tx];
    if (t0 + tx < T) {
        float* yb = y + (long long)b * bstride + t0 + tx;
        for (int c4 = cy; c4 < (C >> 2); c4 += 16) {
            float f[4] = {1.f, 1.f, 1.f, 1.f};
            if (post.p > 0.f) drop4(post.k0, post.k1, post.site, e4 + c4, 0u, post.p, post.keep, f);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 4 * c4 + e;
                float v = fmaf((tile[c * (LND_TT + 1) + tx] - mean) * rstd, gamma[c], beta[c]);
                if (post.p > 0.f) v *= f[e];
                yb[(long long)c * pitch] = v;
            }
        }
    }
}
void launch_ln_drop_cm(const float* x, const float* res, float* y, const float* gamma, const float* beta, int B, int C, int T, int pitch,
                       long long bstride, float eps, int b_global, const DropSite& pre, const DropSite& post, hipStream_t s) {
    if (C % 4 != 0 || !res) { launch_fault("LayerNorm with dropout: C = %d is not a multiple of 4, or no residual", C); return; }
    dim3 grid((T + LND_TT - 1) / LND_TT, B);
    const size_t smem = (size_t)C * (LND_TT + 1) * sizeof(float);   // 52 KB at C = 768
    hipLaunchKernelGGL(ln_drop_cm_kernel, grid, dim3(256), smem, s, x, res, y, gamma, beta, C, T, pitch, bstride, eps, b_global, drop_k(pre), drop_k(post));
}

// ------------------------------------------------------------------------------------------------------------------
// drop_cm_kernel — in place: x = dropout(x); then the SpecAugment span replacement x[b][:][t] = embed[:] where mask[b][t] (after the
// dropout, as Wav2Vec2Model does it).  One thread = one token x four consecutive channels (one Philox call); a wave reads 64
// consecutive tokens of a channel row.
__global__ __launch_bounds__(256) void drop_cm_kernel(float* __restrict__ x, int C4, int T, int pitch, long long bstride, int b_global, const DropK d,
                                                      const unsigned char* __restrict__ mask, const float* __restrict__ embed) {
    const int t = blockIdx.x * 64 + (threadIdx.x & 63), c4 = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
    if (t >= T || c4 >= C4) return;
    float* xp = x + (long long)b * bstride + (long long)(4 * c4) * pitch + t;
    const bool masked = mask && mask[(long long)b * T + t] != 0;
    float f[4] = {1.f, 1.f, 1.f, 1.f};
    if (d.p > 0.f && !masked) drop4(d.k0, d.k1, d.site, ((unsigned)(b_global + b) * (unsigned)T + (unsigned)t) * (unsigned)C4 + (unsigned)c4, 0u, d.p, d.keep, f);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float* p = xp + (long long)e * pitch;
        if (masked) *p = embed[4 * c4 + e];
        else if (d.p > 0.f) *p = *p * f[e];
    }
}
void launch_drop_cm(float* x, int B, int C, int T, int pitch, long long bstride, int b_global, const DropSite& d, const unsigned char* mask,
                    const float* embed, hipStream_t s) {
    if (C % 4 != 0 || (mask && !embed)) { launch_fault("dropout: C = %d is not a multiple of 4, or a mask without its embedding", C); return; }
    if (!(d.p > 0.f) && !mask) return;
    dim3 grid((T + 63) / 64, (C / 4 + 3) / 4, B);
    hipLaunchKernelGGL(drop_cm_kernel, grid, dim3(256), 0, s, x, C / 4, T, pitch, bstride, b_global, drop_k(d), mask, embed);
}

}  // namespace said
