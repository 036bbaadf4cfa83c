// weight_pack.h — the weight layouts the kernels read, as pure host functions: fp32 matrices in, std::vectors out.  No context, no HIP call, no device
// allocation (weights.cpp validates, folds and uploads); plain C++17 for a compiler that has _Float16, so the layouts are testable without a GPU
// (tests/test_weight_pack_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "stchain.h"

namespace said {
namespace pack {

// ---- conversions ----
inline uint16_t f16_bits(_Float16 v) { uint16_t b; memcpy(&b, &v, 2); return b; }
// The split-fp16 pair of split_f16.h: w = h + 2^-11 l with h = RN16(w), l = RN16((w - h) * 2^11) — l from the very bits stored as h.  The ONE host copy.
struct SplitPair { uint16_t h, l; };
inline SplitPair split_pair(float w) {
    const _Float16 h = (_Float16)w;
    return {f16_bits(h), f16_bits((_Float16)((w - (float)h) * 2048.f))};
}
// round-to-nearest-even fp32 -> bf16 (finite inputs)
inline uint16_t bf16_rne(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    x += 0x7fffu + ((x >> 16) & 1u);
    return (uint16_t)(x >> 16);
}
// 16- / 32-bit elements as the float storage the device arrays are declared with
template <typename T>
std::vector<float> as_floats(const std::vector<T>& v) {
    std::vector<float> out(v.size() * sizeof(T) / 4);
    memcpy(out.data(), v.data(), out.size() * 4);
    return out;
}

// ---- fragment packing ----
// A weight W[rows][Ctot][taps] and the rows its 32-row tiles hold: row_of[32 tile + r] is a row of W, or -1 (zeros).
struct Rows {
    const float* W;
    int Ctot, taps;
    std::vector<int> row_of;
    int ntiles() const { return (int)row_of.size() / 32; }
};
inline Rows rows_dense(const float* W, int Ctot, int taps, int N, int row0 = 0) {
    Rows m{W, Ctot, taps, std::vector<int>((size_t)(N + 31) / 32 * 32, -1)};
    for (int i = 0; i < N; ++i) m.row_of[i] = row0 + i;
    return m;
}
struct Src { int c, tap; };   // the (channel, tap) an element comes from; c < 0: padding
// Every MFMA operand layout is out[tile][unit][lane][e]: lane l holds row 32 tile + (l & 31), and a layout says how many units a tile has, how many elements a
// lane holds per unit, where element (unit, l >> 5, e) comes from and how it is converted (conv(value, unit)).  Rows past N and padding are conv(0).
template <typename T, typename Where, typename Conv>
std::vector<T> pack_fragments(const Rows& m, int units, int per_lane, Where where, Conv conv) {
    std::vector<T> out((size_t)m.ntiles() * units * 64 * per_lane);
    size_t o = 0;
    for (int tile = 0; tile < m.ntiles(); ++tile)
        for (int u = 0; u < units; ++u)
            for (int l = 0; l < 64; ++l)
                for (int e = 0; e < per_lane; ++e) {
                    const int row = m.row_of[tile * 32 + (l & 31)];
                    const Src s = where(u, l >> 5, e);
                    out[o++] = conv(row < 0 || s.c < 0 ? 0.f : m.W[((size_t)row * m.Ctot + s.c) * m.taps + s.tap], u);
                }
    return out;
}
// MFMA A-fragment order of channels [c_begin, c_begin + C): Wp[tile][tap][cpair][lane],
// lane l <-> (n = tile*32 + (l & 31), c = c_begin + 2*cpair + (l >> 5)); rows beyond N are zero.
inline std::vector<float> pack_rows(const Rows& m, int c_begin, int C) {
    return pack_fragments<float>(m, m.taps * (C / 2), 1, [=](int u, int hi, int) { return Src{c_begin + 2 * (u % (C / 2)) + hi, u / (C / 2)}; },
                                 [](float v, int) { return v; });
}
// dwordx4 packing: Wq[tile][tap][c/8][lane][4]; value j of lane l = W[tile*32 + (l & 31)][c_begin + 8*cq + 2*j + (l >> 5)][tap]
inline std::vector<float> pack_rows4(const Rows& m, int c_begin, int C) {
    return pack_fragments<float>(m, m.taps * (C / 8), 4, [=](int u, int hi, int j) { return Src{c_begin + 8 * (u % (C / 8)) + 2 * j + hi, u / (C / 8)}; },
                                 [](float v, int) { return v; });
}
// bf16 packing for v_mfma_f32_32x32x8_bf16_1k: Wb[tile][tap][c/8][lane][4]; value j of lane l =
// W[tile*32 + (l & 31)][c_begin + 8*cq + 4*(l >> 5) + j][tap].  Returned as float storage (2 bf16 per float).
inline std::vector<float> pack_rows_bf16(const Rows& m, int c_begin, int C) {
    return as_floats(pack_fragments<uint16_t>(m, m.taps * (C / 8), 4, [=](int u, int hi, int j) { return Src{c_begin + 8 * (u % (C / 8)) + 4 * hi + j, u / (C / 8)}; },
                                              [](float v, int) { return bf16_rne(v); }));
}
// split-fp16 packing for v_mfma_f32_32x32x16_f16 (gemm_lds.hip SP; kernels.h Seg::ws): w = h + 2^-11 l (split_pair).
// Per 24-channel block: NS = 5 (3 taps) / 2 (1 tap) k16 steps x 2 planes (h, l) x 64 lanes x 8 halfs; the 8 halfs of lane l in step s are K-group
// g = 2 s + (l >> 5) of the block's tap-major K slice (tap = g / 3, channels 8 (g % 3) .. + 7), zeros past the slice's 9 / 3 groups.  flat: C / 16 steps over
// the whole K (taps == 1), no padding.  Returned as float storage (2 halfs per float).
inline std::vector<float> pack_rows_split(const Rows& m, int c_begin, int C, bool flat) {
    const int nblk = flat ? 1 : C / 24, ns = flat ? C / 16 : (m.taps == 3 ? 5 : 2), ng = flat ? C / 8 : 3 * m.taps;
    return as_floats(pack_fragments<uint16_t>(   // unit = (block, step, plane)
        m, nblk * ns * 2, 8,
        [=](int u, int hi, int j) {
            const int blk = u / (2 * ns), g = 2 * (u / 2 % ns) + hi;
            if (g >= ng) return Src{-1, 0};
            return flat ? Src{c_begin + 8 * g + j, 0} : Src{c_begin + 24 * blk + 8 * (g % 3) + j, g / 3};
        },
        [](float v, int u) { const SplitPair p = split_pair(v); return u & 1 ? p.l : p.h; }));
}

// ---- the token-major GEMM operands (tgemm.hip, fgemm.hip) ----
// a Conv1d weight [N][C][taps] with its K axis reordered tap-major: [N][taps][C] (the token-major im2col order)
inline std::vector<float> tap_major(const float* W, size_t N, size_t C, size_t taps) {
    std::vector<float> h(N * C * taps);
    for (size_t n = 0; n < N; ++n)
        for (size_t t = 0; t < taps; ++t)
            for (size_t c = 0; c < C; ++c) h[(n * taps + t) * C + c] = W[(n * C + c) * taps + t];
    return h;
}
inline std::vector<uint16_t> to_bf16(const std::vector<float>& w) {
    std::vector<uint16_t> h(w.size());
    for (size_t i = 0; i < w.size(); ++i) h[i] = bf16_rne(w[i]);
    return h;
}
// split-fp16 pairs, one dword h | l << 16 per element (split_f16.h pack_split_f16) — fgemm_kernel's packed mode unpacks them with v_perm
inline std::vector<uint32_t> to_split_words(const std::vector<float>& w) {
    std::vector<uint32_t> pk(w.size());
    for (size_t i = 0; i < w.size(); ++i) {
        const SplitPair p = split_pair(w[i]);
        pk[i] = (uint32_t)p.h | ((uint32_t)p.l << 16);
    }
    return pk;
}

// ---- LayerNorm folds (formed in double, rounded once) ----
// W' = W diag(gamma), W[N][K]
inline std::vector<float> fold_gamma(const float* W, int N, int K, const float* gamma) {
    std::vector<float> f((size_t)N * K);
    for (int n = 0; n < N; ++n)
        for (int k = 0; k < K; ++k) f[(size_t)n * K + k] = (float)((double)W[(size_t)n * K + k] * (double)gamma[k]);
    return f;
}
// bias' = bias + W beta (bias may be null)
inline std::vector<float> fold_beta(const float* W, int N, int K, const float* beta, const float* bias) {
    std::vector<float> f(N);
    for (int n = 0; n < N; ++n) {
        double a = bias ? bias[n] : 0.0;
        for (int k = 0; k < K; ++k) a += (double)W[(size_t)n * K + k] * (double)beta[k];
        f[n] = (float)a;
    }
    return f;
}

// ---- the fused SpatialTransformer tail's operands (stchain.hip) ----
constexpr int CHAIN_MC = 192, CHAIN_FFI = 768;   // the tail's layout is fixed to the model's sizes
// The matrices a unit of the weight stream may come from, all row-major: LayerNorm2 / LayerNorm3 are folded into to_q and the GEGLU projection
// (fold_gamma), proj_out o ff.net.2 is one matrix over [h (768) ; x2 (192)].
enum ChainKind { CK_OUT1, CK_Q, CK_OUT2, CK_GEGLU, CK_FFPROJ, CK_COUNT };
struct ChainMats {
    const float* w[CK_COUNT];   // to_out1 [192][192], to_q' [192][192], to_out2 [192][192], GEGLU' [1536][192] (value rows, then gate rows), [P F2 | P] [192][960]
    static int ld(int kind) { return kind == CK_FFPROJ ? CHAIN_FFI + CHAIN_MC : CHAIN_MC; }
};
// A unit is one k16 step of a 32-row tile: the v_mfma_f32_32x32x16_f16 A operand whose lane l holds row row0 + (l & 31), k = 16 step + 8 (l >> 5) .. + 7.
struct ChainUnit { int kind, row0, step; };
// The units of the stream for `slices` workgroups per token tile (1, 2 or 3; stchain.hip CU<>), slice after slice, within a slice wave after wave, in the order
// the wave consumes them.  Waves 0-5 (column owner j = output columns [32 j, 32 j + 32)): to_out1, to_q, to_out2 (12 steps each, in every slice), the wave's
// GEGLU pairs (12 steps each, value then gate unit per step), then the slice's steps of the folded proj_out — all of them for j < 4, the first half for j = 4, 5;
// waves 6, 7: their GEGLU pairs, then the second half for column tiles 4, 5.
//  * A slice owns 24 / slices GEGLU pairs (hidden tiles): with 1 or 3 slices wave w has the slice's pairs w, w + 8, ...; with 2 (twelve pairs) waves 0-3 have
//    two (w, w + 4) and waves 4-7 one (w + 4).
//  * A slice owns 48 / slices k16 steps of the folded proj_out's GEGLU segment and 12 / slices of its x2 segment (steps 48 .. 59 of the 60).
inline std::vector<ChainUnit> chain_plan(int slices) {
    std::vector<ChainUnit> plan;
    const int npair = 24 / slices, nff = 48 / slices, nx2 = 12 / slices, nstep = nff + nx2;
    for (int c = 0; c < slices; ++c) {
        auto geglu = [&](int w) {   // wave w's pairs of slice c
            std::vector<int> mine;
            if (slices == 2) mine = w < 4 ? std::vector<int>{w, w + 4} : std::vector<int>{w + 4};
            else for (int p = w; p < npair; p += 8) mine.push_back(p);
            for (int p : mine)
                for (int s = 0; s < 12; ++s) {
                    plan.push_back({CK_GEGLU, 32 * (npair * c + p), s});
                    plan.push_back({CK_GEGLU, CHAIN_FFI + 32 * (npair * c + p), s});
                }
        };
        auto ffproj = [&](int tile, int first, int last) {
            for (int i = first; i < last; ++i) plan.push_back({CK_FFPROJ, 32 * tile, i < nff ? nff * c + i : 48 + nx2 * c + (i - nff)});
        };
        for (int w = 0; w < 6; ++w) {
            for (int kind : {CK_OUT1, CK_Q, CK_OUT2})
                for (int s = 0; s < 12; ++s) plan.push_back({kind, 32 * w, s});
            geglu(w);
            ffproj(w, 0, w < 4 ? nstep : nstep / 2);
        }
        for (int w = 6; w < 8; ++w) {
            geglu(w);
            ffproj(w - 2, nstep / 2, nstep);
        }
    }
    return plan;
}
inline float chain_elem(const ChainMats& m, const ChainUnit& u, int l, int i) {
    return m.w[u.kind][(size_t)(u.row0 + (l & 31)) * ChainMats::ld(u.kind) + 16 * u.step + 8 * (l >> 5) + i];
}
// the fp16 stream: 2 KB per unit, the h plane (64 lanes x 8 halfs) and then the l plane
inline std::vector<uint16_t> chain_stream_f16(const std::vector<ChainUnit>& plan, const ChainMats& m) {
    std::vector<uint16_t> st(plan.size() * 1024);
    size_t o = 0;
    for (const ChainUnit& u : plan) {
        for (int e = 0; e < 512; ++e) {
            const SplitPair p = split_pair(chain_elem(m, u, e >> 3, e & 7));
            st[o + e] = p.h;
            st[o + 512 + e] = p.l;
        }
        o += 1024;
    }
    return st;
}
// the bf16 stream: the same units in the same order, ONE plane of bf16 (RNE) — 1 KB per unit
inline std::vector<uint16_t> chain_stream_bf16(const std::vector<ChainUnit>& plan, const ChainMats& m) {
    std::vector<uint16_t> st(plan.size() * 512);
    size_t o = 0;
    for (const ChainUnit& u : plan)
        for (int e = 0; e < 512; ++e) st[o++] = bf16_rne(chain_elem(m, u, e >> 3, e & 7));
    return st;
}
// the vectors b1, bq = Wq beta2, bo2, c2, bffp (192 each), bff' (1536): CHAIN_VEC_FLOATS
inline std::vector<float> chain_vec(const float* b1, const float* bq, const float* bo2, const float* c2, const float* bffp, const float* bff) {
    std::vector<float> vec(CHAIN_VEC_FLOATS);
    const float* part[5] = {b1, bq, bo2, c2, bffp};
    for (int p = 0; p < 5; ++p) std::copy(part[p], part[p] + CHAIN_MC, vec.begin() + p * CHAIN_MC);
    std::copy(bff, bff + 2 * CHAIN_FFI, vec.begin() + 5 * CHAIN_MC);
    return vec;
}

}  // namespace pack
}  // namespace said
