// tm_kernels.hip — the small token-major kernels around the GEMMs: GroupNorm coefficients, UNet operand preparation, the two layout converters and the
// token-major LayerNorms of the audio encoder.
#include "gemm_common.h"
#include "tgemm.h"
#include "tgemm_dev.h"
#include "split_f16.h"

namespace said {

// ------------------------------------------------------------------------------------------------------------------
// GroupNorm coefficients (a, b) per (sample, channel) from the producer's Welford partials, once per tensor: the same
// combination code as inside the GEMM kernels (gemm_common.h), one workgroup per sample, 48 channels per wave.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gn_coef_kernel(const float* __restrict__ part, long long part_bs, int cpg, int nparts, int T, float eps,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ coef_out,
                                                      long long coef_bs) {
    __shared__ float coef[2 * 192];
    __shared__ float gns[4 * GN_SCRATCH];
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, b = blockIdx.x;
    const GnP gp = {cpg, nparts, T, eps, gamma, beta, 192};
    const rsrc_t rp = make_rsrc(part + (long long)b * part_bs, 192u * (unsigned)nparts * 8u);
    GnLoads gl;
    gn_issue(gp, rp, w * 48, 48, l, gl);
    gn_finish(gp, rp, w * 48, 48, l, gl, gns + w * GN_SCRATCH, coef);
    __syncthreads();
    for (int i = tid; i < 2 * 192; i += 256) coef_out[(long long)b * coef_bs + i] = coef[i];
}
void launch_gn_coef(const float* part, long long part_bs, int cpg, int nparts, int T, float eps, const float* gamma, const float* beta,
                    float* coef_out, long long coef_bs, int batch, hipStream_t s) {
    hipLaunchKernelGGL(gn_coef_kernel, dim3(batch), dim3(256), 0, s, part, part_bs, cpg, nparts, T, eps, gamma, beta, coef_out, coef_bs);
}

// ------------------------------------------------------------------------------------------------------------------
// UNet operand preparation: one workgroup = 32 tokens x 192 channels of one sample.  The tile is read with six 16-byte
// loads per thread (all in flight at once), transformed once (GroupNorm affine from the precomputed coefficients, SiLU,
// LayerNorm over channels), transposed through LDS and written token-major in bf16 with 16-byte stores (a token's 384
// bytes are contiguous).  HBM-bound by construction: 24.6 KB in, 12.3 KB out per workgroup.
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 5) void prep_kernel(const PrepArgs a) {   // five workgroups per CU: 84 VGPRs, 31 KB LDS
    __shared__ float tile[192][33];     // RAW values [channel][token]
    __shared__ float coefS[192][2];     // GroupNorm (a, b) per channel (modes 0, 1)
    // one scratch area: first the GroupNorm finalisation's per-wave scratch, then (after the tile barrier) the LayerNorm partials —
    // 31.4 KB of LDS in all, so FIVE workgroups share a CU and the 1216 workgroups of a Be = 64 launch are resident at once
    // (with the two areas separate it was four: a second round of 0.75 workgroups per CU, 12 -> 21 us)
    __shared__ float gns[4 * GN_SCRATCH];
    float (*lnp)[32][2] = reinterpret_cast<float (*)[32][2]>(gns);          // [8][32][2]
    float (*lnst)[2] = reinterpret_cast<float (*)[2]>(gns + 8 * 32 * 2);     // [32][2]
    static_assert(4 * GN_SCRATCH >= 8 * 32 * 2 + 32 * 2, "LayerNorm partials alias the GroupNorm scratch");
    const int tid = threadIdx.x;
    const int t0 = blockIdx.x * 32, b = blockIdx.y;
    const int T = a.T;
    const bool gn = a.mode <= 1, ln = a.mode == 1 || a.mode == 2;
    const float* xb = a.x + (long long)b * a.x_bs;
    // ---- load the raw tile -> LDS [channel][token]; GroupNorm coefficients -> LDS
    float4 v[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int idx = tid + 256 * i, row = idx >> 3, q = idx & 7;
        v[i] = (t0 + 4 * q < a.pitch) ? *reinterpret_cast<const float4*>(xb + (long long)row * a.pitch + t0 + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (gn && a.part) {   // finalise the GroupNorm coefficients here: 4 waves x 48 channels, as gn_coef_kernel
        const int l = tid & 63, w = tid >> 6;
        const GnP gp = {a.gn_cpg, a.gn_nparts, T, a.gn_eps, a.gn_gamma, a.gn_beta, 192};
        const rsrc_t rp = make_rsrc(a.part + (long long)b * a.part_bs, 192u * (unsigned)a.gn_nparts * 8u);
        GnLoads gl;   // (20 loads up front — one round trip instead of two at T = 600 — cost 96 VGPRs + spills: 118.5 vs 116.4 ms in situ)
        gn_issue(gp, rp, w * 48, 48, l, gl);
        gn_finish(gp, rp, w * 48, 48, l, gl, gns + w * GN_SCRATCH, &coefS[0][0]);
        if (a.coef_out && blockIdx.x == 0) {   // the tensor's coefficients for a later consumer (the GroupNorm'ed residual of attn1.to_out)
            __syncthreads();
            float* co = a.coef_out + (long long)b * a.coef_out_bs;
            for (int i = tid; i < 2 * 192; i += 256) co[i] = (&coefS[0][0])[i];
        }
    } else if (gn) {
        const float* cf = a.coef + (long long)b * a.coef_bs;
        for (int i = tid; i < 2 * 192; i += 256) (&coefS[0][0])[i] = cf[i];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int idx = tid + 256 * i, row = idx >> 3, q = idx & 7;
        const float e[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
        for (int k = 0; k < 4; ++k) tile[row][4 * q + k] = (t0 + 4 * q + k < T) ? e[k] : 0.f;
    }
    __syncthreads();
    // ---- LayerNorm statistics per token (modes 1, 2), over the GroupNorm'ed values in mode 1
    float mu = 0.f, rs = 1.f;
    if (ln) {
        const int tt = tid & 31, part = tid >> 5;   // 8 parts x 24 channels
        // (mean, M2) of this part's 24 channels in two passes, merged over the eight parts with Chan's update (round 6: the shifted one-pass sums of rounds 2-5 —
        // d = x - x[channel 0] — lose digits when channel 0 is an outlier channel: gains of 10 on trained-like weights)
        float xs[24];
        float sm = 0.f;
#pragma unroll
        for (int i = 0; i < 24; ++i) {
            const int c = part * 24 + i;
            float x = tile[c][tt];
            if (gn) x = fmaf(x, coefS[c][0], coefS[c][1]);
            xs[i] = x;
            sm += x;
        }
        const float mp = sm * (1.0f / 24.0f);
        float qp = 0.f;
#pragma unroll
        for (int i = 0; i < 24; ++i) { const float d = xs[i] - mp; qp = fmaf(d, d, qp); }
        lnp[part][tt][0] = mp;
        lnp[part][tt][1] = qp;
        __syncthreads();
        if (tid < 32) {
            float mean = lnp[0][tid][0], M2 = lnp[0][tid][1];
#pragma unroll
            for (int p = 1; p < 8; ++p) {
                const float d = lnp[p][tid][0] - mean;
                const float n = 24.f * (float)p, nn = n + 24.f;
                mean = fmaf(d, 24.f / nn, mean);
                M2 += lnp[p][tid][1] + d * d * (n * 24.f / nn);
            }
            lnst[tid][0] = mean;
            lnst[tid][1] = 1.0f / sqrtf(M2 * (1.0f / 192.0f) + 1e-5f);
        }
        __syncthreads();
    }
    // ---- transform + write token-major.  A token's 192 channels are one contiguous row of the destination (768 B in fp32, 384 B in
    // bf16) and the tile's 32 rows are 16-byte chunk g = token * (chunks per row) + chunk: thread tid takes chunks tid, tid + 256, ...,
    // so the 64 lanes of every store instruction write 1 KB of consecutive bytes (with 24 channels per thread each instruction
    // scattered 64 16-byte pieces at a 96-byte stride: six partial writes per cache line).
    const int row_off = a.mode == 0 ? 1 : 0;   // conv operand: row 0 is the left padding
    if (a.f32) {   // fp32 operands (fgemm_kernel): 48 chunks of 4 channels per token
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const int g = i * 256 + tid, tt = g / 48, c0 = 4 * (g - tt * 48);
            const int t = t0 + tt;
            const bool tv = t < T;
            if (!(tv || (a.mode == 0 && t == T))) continue;   // the conv operand's right padding row (token T) is written as zeros
            if (ln) { mu = lnst[tt][0]; rs = lnst[tt][1]; }
            f32x4 o, r;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c0 + k;
                const float raw = tile[c][tt];
                float x = raw;
                if (gn) x = fmaf(x, coefS[c][0], coefS[c][1]);
                if (a.mode == 0) x = silu_f(x);
                if (ln) x = fmaf((x - mu) * rs, a.ln_gamma[c], a.ln_beta[c]);
                o[k] = tv ? x : 0.f;
                r[k] = raw;
                if (a.pack) { o[k] = pack_split_f16(o[k]); r[k] = pack_split_f16(r[k]); }   // (0 packs to 0: the padding rows stay all-zero bits)
            }
            *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.dst) + (long long)b * a.dst_bs + (long long)(t + row_off) * a.ldd + a.coff + c0) = o;
            if (a.dst2 && tv)   // raw copy (1x1 skip conv over the ResBlock input; x2 for the folded proj_out)
                *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.dst2) + (long long)b * a.dst2_bs + (long long)t * a.ldd2 + a.coff2 + c0) = r;
        }
        if (a.mode == 0 && t0 == 0 && tid < 48) {   // left padding row
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(a.dst) + (long long)b * a.dst_bs + a.coff + 4 * tid) = zero;
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {   // bf16 operands: 24 chunks of 8 channels per token
        const int g = i * 256 + tid, tt = g / 24, c0 = 8 * (g - tt * 24);
        const int t = t0 + tt;
        const bool tv = t < T;
        if (!(tv || (a.mode == 0 && t == T))) continue;
        if (ln) { mu = lnst[tt][0]; rs = lnst[tt][1]; }
        __attribute__((aligned(16))) __bf16 o[8];
        __attribute__((aligned(16))) __bf16 r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int c = c0 + k;
            const float raw = tile[c][tt];
            float x = raw;
            if (gn) x = fmaf(x, coefS[c][0], coefS[c][1]);
            if (a.mode == 0) x = silu_f(x);
            if (ln) x = fmaf((x - mu) * rs, a.ln_gamma[c], a.ln_beta[c]);
            o[k] = (__bf16)(tv ? x : 0.f);
            r[k] = (__bf16)raw;
        }
        *reinterpret_cast<u32x4*>(reinterpret_cast<__bf16*>(a.dst) + (long long)b * a.dst_bs + (long long)(t + row_off) * a.ldd + a.coff + c0) = *reinterpret_cast<const u32x4*>(o);
        if (a.dst2 && tv)
            *reinterpret_cast<u32x4*>(reinterpret_cast<__bf16*>(a.dst2) + (long long)b * a.dst2_bs + (long long)t * a.ldd2 + a.coff2 + c0) = *reinterpret_cast<const u32x4*>(r);
    }
    if (a.mode == 0 && t0 == 0 && tid < 24) {   // left padding row
        const u32x4 zero = {0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(reinterpret_cast<__bf16*>(a.dst) + (long long)b * a.dst_bs + a.coff + 8 * tid) = zero;
    }
}
bool launch_prep(const PrepArgs& a, int batch, hipStream_t s) {
    if (a.C != 192 || a.T < 1 || a.ldd % 8 || a.coff % 8 || a.dst_bs % 8 || (a.dst2 && (a.ldd2 % 8 || a.coff2 % 8 || a.dst2_bs % 8)) || a.pitch % 4) return false;
    dim3 grid(a.T / 32 + 1, batch);   // one tile past ceil(T / 32) when T % 32 == 0: the conv operand's right padding row
    hipLaunchKernelGGL(prep_kernel, grid, dim3(256), 0, s, a);
    return true;
}

// ------------------------------------------------------------------------------------------------------------------
// channel-major fp32 [b][C][pitch] -> token-major bf16 [b][T][C]   (conv0 activation, attention output)
// ------------------------------------------------------------------------------------------------------------------
__global__ void cm_to_tm_bf16_kernel(const float* __restrict__ src, long long src_bs, int pitch, unsigned short* __restrict__ dst, long long dst_bs,
                                     int T, int C) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, t = t0 + tx;
        tile[r][tx] = (t < T && c < C) ? src[(long long)b * src_bs + (long long)c * pitch + t] : 0.f;
    }
    __syncthreads();
    __bf16* d = reinterpret_cast<__bf16*>(dst) + (long long)b * dst_bs;
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, c = c0 + tx;
        if (c < C && t < T) d[(long long)t * C + c] = (__bf16)tile[tx][r];
    }
}
__global__ void tm_to_group_bf16_kernel(const float* __restrict__ src, long long src_bs, unsigned short* __restrict__ dst, int T, int G, int CG, int R,
                                        int lpad) {
    const int r = blockIdx.x, b = blockIdx.y, C = G * CG;
    const int t = r - lpad;
    const bool live = t >= 0 && t < T;
    __bf16* d = reinterpret_cast<__bf16*>(dst);
    for (int i = threadIdx.x; i < C; i += blockDim.x) {
        const int g = i / CG, c = i - g * CG;
        const float v = live ? src[(long long)b * src_bs + (long long)t * C + i] : 0.f;
        d[(((long long)b * G + g) * R + r) * CG + c] = (__bf16)v;
    }
}
void launch_tm_to_group_bf16(const float* src, long long src_bs, void* dst, int B, int T, int G, int CG, int R, int lpad, hipStream_t s) {
    hipLaunchKernelGGL(tm_to_group_bf16_kernel, dim3(R, B), dim3(256), 0, s, src, src_bs, reinterpret_cast<unsigned short*>(dst), T, G, CG, R, lpad);
}
void launch_cm_to_tm_bf16(const float* src, long long src_bs, int pitch, void* dst, long long dst_bs, int B, int T, int C, hipStream_t s) {
    dim3 grid((T + 31) / 32, (C + 31) / 32, B);
    hipLaunchKernelGGL(cm_to_tm_bf16_kernel, grid, dim3(256), 0, s, src, src_bs, pitch, reinterpret_cast<unsigned short*>(dst), dst_bs, T, C);
}

// ------------------------------------------------------------------------------------------------------------------
// token-major LayerNorm over C channels, one wave per token: y = LN(x [+ add]) -> fp32 and/or bf16 copies
// ------------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void ln_tm_kernel(const float* __restrict__ x, const float* __restrict__ add, float* __restrict__ yf,
                                                    unsigned short* __restrict__ yb, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, long long ntok, float eps) {
    constexpr int PER = C / 64;
    const long long tok = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tok >= ntok) return;
    const int l = threadIdx.x & 63;
    float v[PER];
    float s1 = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        v[i] = x[tok * C + l + 64 * i];
        if (add) v[i] += add[tok * C + l + 64 * i];
        s1 += v[i];
    }
    const float mean = wave_sum(s1) * (1.0f / C);
    float s2 = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) { const float d = v[i] - mean; s2 = fmaf(d, d, s2); }
    const float rstd = 1.0f / sqrtf(wave_sum(s2) * (1.0f / C) + eps);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int c = l + 64 * i;
        const float o = fmaf((v[i] - mean) * rstd, gamma[c], beta[c]);
        if (yf) yf[tok * C + c] = o;
        if (yb) reinterpret_cast<__bf16*>(yb)[tok * C + c] = (__bf16)o;
    }
}
void launch_ln_tm(const float* x, const float* add, float* yf, void* yb, const float* gamma, const float* beta, long long ntok, int C, float eps,
                  hipStream_t s) {
    const dim3 grid((unsigned)((ntok + 3) / 4));
    if (C == 768) hipLaunchKernelGGL(ln_tm_kernel<768>, grid, dim3(256), 0, s, x, add, yf, reinterpret_cast<unsigned short*>(yb), gamma, beta, ntok, eps);
    else if (C == 512) hipLaunchKernelGGL(ln_tm_kernel<512>, grid, dim3(256), 0, s, x, add, yf, reinterpret_cast<unsigned short*>(yb), gamma, beta, ntok, eps);
    else launch_fault("ln_tm for C=%d not instantiated", C);
}

// ------------------------------------------------------------------------------------------------------------------
// F.interpolate(linear, align_corners=True) along t of token-major bf16 features (wav2vec2.py:41-44), then the feature
// projection's LayerNorm(512) — one wave per output frame -> bf16 token-major [b][Tout][C]
// ------------------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void interp_ln_tm_kernel(const unsigned short* __restrict__ src, long long src_bs, int Tin,
                                                           unsigned short* __restrict__ dst, long long dst_bs, int Tout, float scale,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta, float eps) {
    constexpr int PER = C / 64;
    const int b = blockIdx.y;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= Tout) return;
    const int l = threadIdx.x & 63;
    const float pos = __fmul_rn(scale, (float)i);
    int i0 = min((int)pos, Tin - 1);
    const int i1 = i0 + ((i0 < Tin - 1) ? 1 : 0);
    const float l1 = __fsub_rn(pos, (float)i0), l0 = __fsub_rn(1.0f, l1);
    const __bf16* s0 = reinterpret_cast<const __bf16*>(src) + (long long)b * src_bs + (long long)i0 * C;
    const __bf16* s1p = reinterpret_cast<const __bf16*>(src) + (long long)b * src_bs + (long long)i1 * C;
    float v[PER];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        v[k] = __fadd_rn(__fmul_rn(l0, (float)s0[l + 64 * k]), __fmul_rn(l1, (float)s1p[l + 64 * k]));
        sum += v[k];
    }
    const float mean = wave_sum(sum) * (1.0f / C);
    float s2 = 0.f;
#pragma unroll
    for (int k = 0; k < PER; ++k) { const float d = v[k] - mean; s2 = fmaf(d, d, s2); }
    const float rstd = 1.0f / sqrtf(wave_sum(s2) * (1.0f / C) + eps);
    __bf16* d = reinterpret_cast<__bf16*>(dst) + (long long)b * dst_bs + (long long)i * C;
#pragma unroll
    for (int k = 0; k < PER; ++k) d[l + 64 * k] = (__bf16)fmaf((v[k] - mean) * rstd, gamma[l + 64 * k], beta[l + 64 * k]);
}
void launch_interp_ln_tm(const void* src, long long src_bs, int Tin, void* dst, long long dst_bs, int Tout, int B, int C, const float* gamma,
                         const float* beta, float eps, hipStream_t s) {
    if (C != 512) { launch_fault("interp_ln_tm for C=%d not instantiated", C); return; }
    const float scale = (Tout > 1) ? (float)(Tin - 1) / (float)(Tout - 1) : 0.f;
    dim3 grid((Tout + 3) / 4, B);
    hipLaunchKernelGGL(interp_ln_tm_kernel<512>, grid, dim3(256), 0, s, reinterpret_cast<const unsigned short*>(src), src_bs, Tin,
                       reinterpret_cast<unsigned short*>(dst), dst_bs, Tout, scale, gamma, beta, eps);
}

}  // namespace said
