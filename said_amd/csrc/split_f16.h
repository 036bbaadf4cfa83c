// split_f16.h — fp32-accurate matrix products on the fp16 matrix pipe (round 4).
#pragma once
#include "vec_types.h"

namespace said {

// Split-fp16 operands (attn_kernel PM == 2, fgemm_kernel SP): x ~= h + 2^-11 l with h = RN16(x), l = RN16((x - h) * 2^11) — the remainder is stored at h's own
// magnitude, so both halves are normal fp16 numbers for 2^-14 <= |x| < 65504 and x is represented to 2^-22 relative (22 significand bits + the
// remainder's sign; below 2^-14 the pair still resolves 2^-36 absolute where the matrix pipe keeps fp16 denormals) — and
//   a . b ~= h_a . h_b + 2^-11 (h_a . l_b + l_a . h_b)
// on v_mfma_f32_32x32x16_f16: three 8-pass MFMAs per 16 contraction steps against eight 16-pass v_mfma_f32_32x32x2_f32 (5.3 x fewer
// matrix-pipe clocks).  Accumulation is fp32 as before; the cross terms have their own accumulator (merged with one fma per element).  The
// dropped term 2^-22 l_a . l_b is below the representation error.  Domain: |x| < 65504 (q, k, v are projections of LayerNorm'ed rows; an
// overflow shows as inf / NaN).
struct SplitH { f16x8 h, l; };
// The low plane must be computed from the very bits that are stored as the high plane.  Round 5 (stchain.hip bring-up): hipcc converts the stored vector
// with v_cvt_pk_f16_f32 and, left to itself, the (float)h inside the remainder with a separate v_cvt_f16_f32 — and the two disagree when x lies exactly
// half-way between two fp16 numbers (one element in 2^13): h from one rounding, l from the other, i.e. an operand off by a whole fp16 ulp (2^-11 relative; seen
// as 1e-4 errors of single tokens).  The empty asm makes the packed result opaque, so every later use reads those bits.
static __device__ __forceinline__ void split_f16x4(const float x0, const float x1, const float x2, const float x3, f16x4& h, f16x4& l) {
    h[0] = (_Float16)x0; h[1] = (_Float16)x1; h[2] = (_Float16)x2; h[3] = (_Float16)x3;
    asm volatile("" : "+v"(h));
    l[0] = (_Float16)((x0 - (float)h[0]) * 2048.f);   // (x - h is exact in fp32)
    l[1] = (_Float16)((x1 - (float)h[1]) * 2048.f);
    l[2] = (_Float16)((x2 - (float)h[2]) * 2048.f);
    l[3] = (_Float16)((x3 - (float)h[3]) * 2048.f);
}
static __device__ __forceinline__ SplitH split_f16x8(const f32x4 a, const f32x4 b) {
    SplitH r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r.h[i] = (_Float16)a[i];
        r.h[4 + i] = (_Float16)b[i];
    }
    asm volatile("" : "+v"(r.h));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r.l[i] = (_Float16)((a[i] - (float)r.h[i]) * 2048.f);      // (a - h is exact in fp32)
        r.l[4 + i] = (_Float16)((b[i] - (float)r.h[4 + i]) * 2048.f);
    }
    return r;
}
// A split operand element as ONE dword (h in the low half, l in the high half): what a producer stores when every consumer would split the value again
// (the q/k/v GEMM's k and v tiles: each of a sample's 19 query-tile workgroups used to split all of K and V for itself — attn.hip PM = 3).
static __device__ __forceinline__ float pack_split_f16(float x) {
    _Float16 h = (_Float16)x;
    asm volatile("" : "+v"(h));
    const _Float16 lo = (_Float16)((x - (float)h) * 2048.f);
    const unsigned u = (unsigned)__builtin_bit_cast(unsigned short, h) | ((unsigned)__builtin_bit_cast(unsigned short, lo) << 16);
    return __builtin_bit_cast(float, u);
}
// eight packed elements -> the two MFMA operand planes: one v_perm_b32 per two elements and plane
static __device__ __forceinline__ SplitH unpack_f16x8(const f32x4 a, const f32x4 b) {
    const u32x4 ua = __builtin_bit_cast(u32x4, a), ub = __builtin_bit_cast(u32x4, b);
    const u32x4 hh = {__builtin_amdgcn_perm(ua[1], ua[0], 0x05040100u), __builtin_amdgcn_perm(ua[3], ua[2], 0x05040100u),
                       __builtin_amdgcn_perm(ub[1], ub[0], 0x05040100u), __builtin_amdgcn_perm(ub[3], ub[2], 0x05040100u)};
    const u32x4 ll = {__builtin_amdgcn_perm(ua[1], ua[0], 0x07060302u), __builtin_amdgcn_perm(ua[3], ua[2], 0x07060302u),
                       __builtin_amdgcn_perm(ub[1], ub[0], 0x07060302u), __builtin_amdgcn_perm(ub[3], ub[2], 0x07060302u)};
    SplitH r;
    r.h = __builtin_bit_cast(f16x8, hh);
    r.l = __builtin_bit_cast(f16x8, ll);
    return r;
}
// Only a scheduling fence (the conversions stay in front of the MFMA group): the issue order of the split products is free.  The corruption round 4 chased
// here was other kernels' crossed packed-fp32 operands beside fp16 / bf16 MFMAs (said_amd/build.py NO_SLP and its ISA scan).
static __device__ __forceinline__ void operand_fence() { __builtin_amdgcn_sched_barrier(0); }

}  // namespace said
