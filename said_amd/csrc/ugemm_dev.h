// ugemm_dev.h — what the bodies of the LDS-staged UNet GEMM (ugemm_body.h, kconv_body.h) and its host side (gemm_lds.hip) share: the tile constants, the
// preloaded header and a wave's block descriptor.  (The compile-time launch variants and which instantiations are kconv_body's: kernels.h; the shape lists: ugemm_plan.h.)
#pragma once
#include "gemm_common.h"
#include "ugemm_plan.h"

namespace said {

constexpr int XP = 40;        // LDS tile pitch (floats): col = tin - t0 + 4  (halo at 3 and 36)
// bf16 MFMA mode (BF): the tile is kept token-major in bf16, X[col = tin - t0 + 1][channel], pitch PB halfs, so that the
// B operand of v_mfma_f32_32x32x8_bf16_1k — 4 consecutive channels of one token — is a single ds_read_b64
constexpr int PB = 28;
constexpr int NRMAX = 3;      // row rounds per block: CB = 8 * NR <= 24 channels

template <int XF>
__device__ __forceinline__ float xf1(float v, float2 gn, float mu, float rs, float2 ln) { return xform_apply<XF>(v, gn, mu, rs, ln); }

// 16 dwords of launch-invariant scalars passed as LEADING kernel parameters: with -amdgpu-kernarg-preload-count=16
// the command processor delivers them in SGPRs, so the first operand loads need no memory round trip at all.
struct FastHdr {       // unpacked view of the preloaded kernel parameters
    const float* x;    // segment 0 source (batch 0)
    const float* w4;   // segment 0 packed weights (+ GroupNorm / LayerNorm affine tails)
    int pack;          // C | taps << 16 | xform << 20 | nseg << 24 | (gn_eps == 1e-6) << 26 | tiles per workgroup << 28
    int pitch, T, bstride;   // segment 0 pitch, length (stride-1 conv: Tin == T), batch stride (floats)
    int bmod_b0;       // ny_magic (17 bits) | b0 << 17  (ny_magic = floor(65536 / ny) + 1: block decode without a division)
    int N;
    int gate_vft;      // EPI_GEGLU: gate tile offset; EPI_QKV: number of leading token-major tiles
    // GroupNorm statistics of segment 0: with these the partial loads — the head of the longest dependent chain of
    // a GroupNorm'ed GEMM — go out at kernel entry instead of one memory round trip later
    const float* gn_part;
    int gn_bstride;    // floats between batches of the partials
    int gn_cfg;        // gn_cpg | gn_nparts << 16
};
// The header travels as the 14 leading dwords of the kernel parameters: that is how many the hardware preloads into
// SGPRs (2 of the 16 user SGPRs hold the kernarg pointer).  Anything beyond — and implicit arguments such as gridDim —
// costs a scalar-memory round trip before the first request can be issued, so T|N and pitch|gate_vft share dwords
// and the grid width is passed explicitly.
constexpr int kHdrDwords = 14;

// dwords of one output tile's split-fp16 weights (Seg::ws): per-block layout [C / 24][5 | 2 steps][2 planes][64 lanes][4 dwords]; the flat layout of the
// one-tile-per-wave GEGLU shape, [C / 16][2][64][4], has the same size as the fp32 packing
__host__ __device__ constexpr unsigned sp_tile_dwords(int C, int taps, bool flat = false) {
    return flat ? (unsigned)(C / 16) * 2u * 256u : (unsigned)(C / 24) * (taps == 3 ? 5u : 2u) * 2u * 256u;
}
struct UBlock {   // one (segment, channel block) of this wave
    rsrc_t rx, rw;
    int c0;        // first channel of the block (segment-relative)
    int taps, Tin, pitch4, C8 /* C / 8 */;
    int xform;
    const float2* cGN;   // LDS coefficient tables, indexed by segment channel
    const float2* cLN;
};

}  // namespace said
