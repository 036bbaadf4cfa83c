// enc_gemm.hip — the fine-tuned audio encoder's dense products (q / k / v / out_proj / the two FFN layers / the feature projection; forward,
// data gradient, weight gradient) on split-fp16 operands: x ~= h + 2^-11 l (split_f16.h), a . b ~= h_a . h_b + 2^-11 (h_a . l_b + l_a . h_b)
// on v_mfma_f32_32x32x16_f16, three products per 16 contraction steps, fp32 accumulation, the cross terms in an accumulator of their own.
//
// One kernel family: C (R, S) = sum_k A(r, k) B(s, k), an operand either contiguous along the contraction (element (r, k) at r ld + k) or
// across it (at k ld + r):
//   forward          A = x  (along),  B = W  (along)    R = M tokens, S = N, contraction K
//   data gradient    A = dy (along),  B = W  (across)   R = M tokens, S = K, contraction N
//   weight gradient  A = dy (across), B = x  (across)   R = N,        S = K, contraction M tokens, K-split
// The weight's two dimensions are multiples of the 64 x 64 tile; the token count is arbitrary: a ragged row edge of the operand that lies
// along the contraction, a ragged contraction of the operands that lie across it.
//
// Every workgroup splits its own fp32 operands: a 64 x 32 tile goes from global memory through registers (requested four tiles ahead, under the
// matrix instructions of the tiles in between) into the two fp16 planes in LDS, [row][k] with 80-byte rows, from where a lane's eight
// contraction steps of a plane are one ds_read_b128.  Both planes of an operand come from one conversion (split_f16x4).
//
// The gradient operand (A of the two gradients) is first multiplied by a power of two taken from its largest magnitude (amax_kernel: per-block
// maxima of the magnitudes' bit patterns, an exact and order-independent reduction; every GEMM workgroup combines the 256 partial maxima
// itself), and the epilogue multiplies by the inverse; both multiplications are exact.  Zero and non-finite maxima take scale 1.
//
// Reduction orders: an element is summed over the contraction in ascending 32-wide tiles, each as two matrix instructions per product; the
// K-split weight gradient writes one partial tile per chunk, which gemm_reduce (unet_train.hip) adds in ascending chunk order.  No atomics.
#include "enc_gemm.h"

#include "split_f16.h"
#include "unet_train.h"
#include "vec_types.h"

namespace said {
namespace eg {
namespace {

constexpr int NT = 256, BM = 64, BN = 64, BK = 32, NS = 4, LDH = BK + 8;   // LDH: halves per LDS row (80 bytes: 16-byte aligned, off the 64-byte stride)
static_assert(BM == EG_TILE && BN == EG_TILE, "enc_gemm.h states the tile");

struct Args {
    const float *A, *B;
    int lda, ldb, a_vec, b_vec;   // *_vec: the operand's address and leading dimension allow vector loads
    int R, S, Kc;
    float* C;
    int ldc;
    const float* bias;
    const float* res;
    int ldr, accumulate, KS, kchunk;
    float* part;
    const unsigned* amax;   // null: A is not scaled
};

// the largest magnitude of x[0 .. n) as a bit pattern (a NaN is above infinity, so it survives): one word per block
__global__ void __launch_bounds__(NT) amax_kernel(const float* __restrict__ x, long long n, unsigned* __restrict__ out) {
    __shared__ unsigned sh[NT / 64];
    unsigned m = 0;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n; i += (long long)gridDim.x * NT)
        m = max(m, __builtin_bit_cast(unsigned, x[i]) & 0x7fffffffu);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = max(max(sh[0], sh[1]), max(sh[2], sh[3]));
}

// what a thread holds of an operand tile between global memory and LDS
struct Stage { f32x4 v[2]; };

// KC: the operand is contiguous along the contraction: thread items e = tid, tid + 256: row e / 8, k = 4 (e % 8) .. + 3 (rows past `rows` read as 0;
// the contraction is a multiple of 32 there).  Else: k = 4 (tid / 32) + j, rows 2 (tid % 32), + 1 (k past kend reads as 0; the rows are a multiple
// of 64 there)
template <bool KC>
__device__ __forceinline__ Stage load_tile(const float* __restrict__ p, int ld, int vec, int rows, int r0, int k0, int kend, int tid) {
    Stage st;
    if (KC) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + NT * i, row = r0 + (e >> 3), k = k0 + 4 * (e & 7);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (row < rows) {
                const float* q = p + (long long)row * ld + k;
                if (vec) v = *reinterpret_cast<const f32x4*>(q);
                else { v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3]; }
            }
            st.v[i] = v;
        }
    } else {
        const int kg = tid >> 5, rp = tid & 31;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + 4 * kg + j;
            f32x2 w = {0.f, 0.f};
            if (k < kend) {
                const float* q = p + (long long)k * ld + r0 + 2 * rp;
                if (vec) w = *reinterpret_cast<const f32x2*>(q);
                else { w[0] = q[0]; w[1] = q[1]; }
            }
            st.v[j >> 1][2 * (j & 1)] = w[0];
            st.v[j >> 1][2 * (j & 1) + 1] = w[1];
        }
    }
    return st;
}

template <bool KC>
__device__ __forceinline__ void store_tile(const Stage& st, float sc, _Float16 (*H)[LDH], _Float16 (*L)[LDH], int tid) {
    f16x4 h, l;
    if (KC) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = tid + NT * i, row = e >> 3, k = 4 * (e & 7);
            split_f16x4(st.v[i][0] * sc, st.v[i][1] * sc, st.v[i][2] * sc, st.v[i][3] * sc, h, l);
            *reinterpret_cast<f16x4*>(&H[row][k]) = h;
            *reinterpret_cast<f16x4*>(&L[row][k]) = l;
        }
    } else {
        const int k = 4 * (tid >> 5), row = 2 * (tid & 31);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            split_f16x4(st.v[0][i] * sc, st.v[0][2 + i] * sc, st.v[1][i] * sc, st.v[1][2 + i] * sc, h, l);
            *reinterpret_cast<f16x4*>(&H[row + i][k]) = h;
            *reinterpret_cast<f16x4*>(&L[row + i][k]) = l;
        }
    }
}

template <bool AKC, bool BKC>
__global__ void __launch_bounds__(NT) enc_gemm_kernel(const Args g) {
    __shared__ __attribute__((aligned(16))) _Float16 Ah[BM][LDH], Al[BM][LDH], Bh[BN][LDH], Bl[BN][LDH];
    __shared__ unsigned red[NT / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, wm = wave & 1, wn = wave >> 1;
    const int r0 = blockIdx.x * BM, s0 = blockIdx.y * BN, ks = blockIdx.z;
    const int kbeg = ks * g.kchunk, kend = min(g.Kc, kbeg + g.kchunk);

    // the gradient operand's scale 2^s and its inverse
    float sc = 1.f, inv = 1.f;
    if (g.amax) {
        unsigned m = g.amax[tid];   // EG_AMAX_BLOCKS == NT words
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
        if (lane == 0) red[wave] = m;
        __syncthreads();
        m = max(max(red[0], red[1]), max(red[2], red[3]));
        const int e = (int)(m >> 23);
        if (m != 0u && e != 255) {
            const int s = min(14 - (max(e, 1) - 127), 126);
            sc = __builtin_bit_cast(float, (unsigned)(127 + s) << 23);
            inv = __builtin_bit_cast(float, (unsigned)(127 - s) << 23);
        }
    }

    f32x16 hh, xx;
#pragma unroll
    for (int i = 0; i < 16; ++i) { hh[i] = 0.f; xx[i] = 0.f; }
    // NS tiles are in flight between global memory and LDS: a forward product of the 768-wide layers is 180 workgroups, fewer than the chip
    // has CUs, so nothing but the workgroup's own earlier requests hides a load's latency
    Stage ra[NS], rb[NS];
    const int nt = kbeg < kend ? (kend - kbeg + BK - 1) / BK : 0;
#pragma unroll
    for (int i = 0; i < NS; ++i)
        if (i < nt) {
            ra[i] = load_tile<AKC>(g.A, g.lda, g.a_vec, g.R, r0, kbeg + i * BK, kend, tid);
            rb[i] = load_tile<BKC>(g.B, g.ldb, g.b_vec, g.S, s0, kbeg + i * BK, kend, tid);
        }
    const int fr = lane & 31, fk = 8 * (lane >> 5);
    for (int t0 = 0; t0 < nt; t0 += NS) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            const int t = t0 + i;
            if (t >= nt) break;   // uniform over the workgroup
            __syncthreads();      // the previous tile's operand reads are done
            store_tile<AKC>(ra[i], sc, Ah, Al, tid);
            store_tile<BKC>(rb[i], 1.f, Bh, Bl, tid);
            __syncthreads();
            if (t + NS < nt) {
                ra[i] = load_tile<AKC>(g.A, g.lda, g.a_vec, g.R, r0, kbeg + (t + NS) * BK, kend, tid);
                rb[i] = load_tile<BKC>(g.B, g.ldb, g.b_vec, g.S, s0, kbeg + (t + NS) * BK, kend, tid);
            }
#pragma unroll
            for (int q = 0; q < BK / 16; ++q) {
                const f16x8 ah = *reinterpret_cast<const f16x8*>(&Ah[wm * 32 + fr][16 * q + fk]);
                const f16x8 al = *reinterpret_cast<const f16x8*>(&Al[wm * 32 + fr][16 * q + fk]);
                const f16x8 bh = *reinterpret_cast<const f16x8*>(&Bh[wn * 32 + fr][16 * q + fk]);
                const f16x8 bl = *reinterpret_cast<const f16x8*>(&Bl[wn * 32 + fr][16 * q + fk]);
                xx = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, xx, 0, 0, 0);
                hh = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, hh, 0, 0, 0);
                xx = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, xx, 0, 0, 0);
            }
        }
    }
    // lane l, register v: row 8 (v / 4) + 4 (l / 32) + v % 4, column l % 32
    const int s = s0 + wn * 32 + (lane & 31);
    if (s >= g.S) return;
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int r = r0 + wm * 32 + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
        if (r >= g.R) continue;
        float y = __builtin_fmaf(xx[v], 0x1p-11f, hh[v]) * inv;
        if (g.KS > 1) {
            g.part[((long long)ks * g.R + r) * g.S + s] = y;
            continue;
        }
        if (g.bias) y += g.bias[s];
        if (g.res) y += g.res[(long long)r * g.ldr + s];
        float* c = g.C + (long long)r * g.ldc + s;
        if (g.accumulate) y += *c;
        *c = y;
    }
}

bool vec_ok(const float* p, int ld, int n) { return reinterpret_cast<uintptr_t>(p) % (sizeof(float) * n) == 0 && ld % n == 0; }

}  // namespace

void enc_gemm(hipStream_t s, const EncGemm& e) {
    Args g{};
    g.A = e.a; g.lda = e.lda; g.B = e.b; g.ldb = e.ldb;
    g.C = e.c; g.ldc = e.ldc; g.bias = e.bias; g.res = e.res; g.ldr = e.ldr; g.accumulate = e.accumulate;
    g.KS = 1; g.part = e.part;
    if (e.layout != EG_FWD) {
        amax_kernel<<<EG_AMAX_BLOCKS, NT, 0, s>>>(e.a, (long long)e.M * e.N, e.amax);
        g.amax = e.amax;
    }
    if (e.layout == EG_FWD) {
        g.R = e.M; g.S = e.N; g.Kc = e.K; g.kchunk = e.K;
        g.a_vec = vec_ok(e.a, e.lda, 4); g.b_vec = vec_ok(e.b, e.ldb, 4);
        enc_gemm_kernel<true, true><<<dim3((g.R + BM - 1) / BM, g.S / BN, 1), NT, 0, s>>>(g);
    } else if (e.layout == EG_DGRAD) {
        g.R = e.M; g.S = e.K; g.Kc = e.N; g.kchunk = e.N;
        g.a_vec = vec_ok(e.a, e.lda, 4); g.b_vec = vec_ok(e.b, e.ldb, 2);
        enc_gemm_kernel<true, false><<<dim3((g.R + BM - 1) / BM, g.S / BN, 1), NT, 0, s>>>(g);
    } else {
        g.R = e.N; g.S = e.K; g.Kc = e.M; g.KS = e.KS; g.kchunk = e.kchunk;
        g.a_vec = vec_ok(e.a, e.lda, 2); g.b_vec = vec_ok(e.b, e.ldb, 2);
        enc_gemm_kernel<false, false><<<dim3(g.R / BM, g.S / BN, g.KS), NT, 0, s>>>(g);
        if (g.KS > 1) {
            ut::UGemm u{};
            u.C = e.c; u.ldc = e.ldc; u.M = e.N; u.N = e.K; u.Z = 1; u.ZH = 1; u.alpha = 1.f; u.rbT = 1; u.KS = e.KS; u.part = e.part;
            ut::gemm_reduce(s, u);
        }
    }
}

}  // namespace eg
}  // namespace said
