// tgemm.hip — bf16 GEMM on v_mfma_f32_32x32x16_bf16 for the audio encoder's bf16 mode (BASELINE.json configs[2]):
// the three LDS-staged bf16 tile kernels and launch_tgemm's dispatch.
//
//     Y[m][n] = epi( sum_k A[m][k] * W[n][k] )        A, W bf16 with k contiguous ("NT"), fp32 accumulation
//
// In bf16 mode the Wav2Vec2 encoder (wav2vec2.py:13-82 + the HF internals it inherits) keeps its activations TOKEN-major
// [t][c]: both MFMA operands then want 8 consecutive k per lane, i.e. one 16-byte load each, and a strided Conv1d over
// token-major data IS a GEMM whose A rows overlap — row m starts at element m * stride * C and spans taps * C
// contiguous elements — so the six 512-channel feature-extractor convolutions, the feature projection and the 48
// encoder-layer projections all run through this one kernel.  (The fp32 mode keeps the channel-major kernels.)
//
// Tile: 128 tokens x 128 outputs x 64 k per workgroup of 4 waves (2 x 2, each 64 x 64 = 2 x 2 MFMA tiles, 64 accumulator
// registers).  Operand tiles are staged through LDS with register double-buffering (global -> registers for tile k+1
// while tile k multiplies, one barrier per tile); LDS rows are padded to 72 halfs so that the 16-byte fragment reads of
// 8 consecutive lanes fall on distinct banks.  72 KB of LDS per workgroup: two workgroups share a CU.
#include <algorithm>
#include <type_traits>

#include "gemm_common.h"
#include "tgemm.h"
#include "tgemm_dev.h"
#include "split_f16.h"

namespace said {

constexpr int TBM = 128, TBK = 64, TLP = 72;   // rows of the small tile, k per tile, LDS row pitch in halfs

// ---- what the three tile kernels share: the accumulator clear, the MFMAs of one k-tile and the epilogue tail
template <int NJ>
__device__ __forceinline__ void tile_clear(f32x16 (&acc0)[NJ], f32x16 (&acc1)[NJ]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[j][r] = 0.f; acc1[j][r] = 0.f; }
}
// One k-tile of a wave: per k16 step two A fragments (tile rows ar, ar + 32), NJ W fragments (tile rows wr + 32 j) and 2 NJ v_mfma_f32_32x32x16_bf16.
// frag_a / frag_w (row, ks) read the lane's 16 bytes of step ks from the operand tile in LDS: the row pitch TLP in the staged tiles, the XOR swizzle in the direct one.
template <int NJ, class FA, class FW>
__device__ __forceinline__ void tile_mfma(f32x16 (&acc0)[NJ], f32x16 (&acc1)[NJ], int ar, int wr, FA frag_a, FW frag_w) {
#pragma unroll
    for (int ks = 0; ks < TBK / 16; ++ks) {
        bf16x8 fa[2], fb[NJ];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = frag_a(ar + i * 32, ks);
#pragma unroll
        for (int j = 0; j < NJ; ++j) fb[j] = frag_w(wr + j * 32, ks);
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            acc0[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0], fb[j], acc0[j], 0, 0, 0);
            acc1[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1], fb[j], acc1[j], 0, 0, 0);
        }
    }
}
// the K loop ended with a barrier: the operand buffers are free and serve as per-wave transposition scratch.  mw / nw: first row / column of wave w's 64 x 32 NJ part
template <int NJ>
__device__ __forceinline__ void tile_epilogue(const TGemmArgs& a, f32x16 (&acc0)[NJ], f32x16 (&acc1)[NJ], unsigned short* lds, int w, int l, int b, int mw, int nw,
                                              int nlim = 0) {
    float* sc = reinterpret_cast<float*>(lds) + w * (32 * (32 * NJ + 4));
    tg_epilogue<NJ>(a, acc0, b, mw, nw, l, sc, nullptr, 0, nlim);
    tg_epilogue<NJ>(a, acc1, b, mw + 32, nw, l, sc, nullptr, 0, nlim);
}

// BM = 128 (4 waves as 2 x 2): BN = 128: each wave 64 tokens x 64 outputs; BN = 64 (N = 192, 576): each wave 64 tokens x 32 outputs
// SB (single LDS buffer): one operand buffer and one register set instead of two of each — 36.9 KB of LDS and ~84 VGPRs, so FOUR
// workgroups share a CU (two with the double buffer); a k-tile then costs two barriers, which the other three workgroups fill.
// ------------------------------------------------------------------------------------------------------------------
// BM = 256, the 256-row tile (large M): 8 waves as 4 (rows) x 2 (columns), each 64 rows x BN / 2 columns, BN = 256 (N % 256 == 0: the audio
// encoder's 512 / 768 / 2304 / 3072-wide outputs, GEGLU) or 192 (the UNet's 192 / 576-wide outputs).  The 128-row kernel
// was bound by operand bytes per FLOP, not by MFMA: 15.6-24 B per kFLOP from L2 with two tiles in flight per workgroup
// left the MFMA pipes 11-22 % busy and the waves 45 % parked on s_waitcnt (profiles/r02c_pmc_sq_b32_bf16.txt).  This shape moves
// 7.8 (256 x 256) / 9.1 (256 x 192) B per kFLOP and gives each wave 32 / 24 MFMAs per k-tile to hide the next tile's loads.
// With seg_rows > 0 the row axis is the whole batch (per-sample pitch seg_rows), so M = 600 does not cost tile padding.
// ------------------------------------------------------------------------------------------------------------------
// The two heights differ in: the thread count and wave grid; the operand offsets (64-bit for 128 rows, 32-bit element offsets within one sample's operand / the
// weight matrix for 256 rows: < 2^31, host-checked); grouped launches (128 rows only); batch-as-rows addressing (256 rows only).
template <int BM, int BN, bool SB = false>
__global__ __launch_bounds__(2 * BM) void tgemm_kernel(const TGemmArgs a) {
    static_assert(BM == 128 || (BM == 256 && !SB), "the single-buffer variant exists for the 128-row tile only");
    extern __shared__ __attribute__((aligned(16))) unsigned short lds[];   // [2 buffers][A BM x 72 | W BN x 72]
    constexpr bool BIG = BM == 256;
    constexpr int NTH = 2 * BM;
    constexpr int NJ = BN / 64;                 // MFMA column tiles per wave
    constexpr int WCH = BN * 8 / NTH;           // 16-byte W chunks per thread and tile
    constexpr int BUF = (BM + BN) * TLP;
    typedef typename std::conditional<BIG, int, long long>::type ofs_t;
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    const int wm = w >> 1, wn = w & 1;
    const int rows_tot = (BIG && a.seg_rows > 0) ? a.batch * a.seg_rows : a.M;   // rows of the A operand per grid batch entry
    const int nbatch = (BIG && a.seg_rows > 0) ? 1 : a.batch;
    // The 1-D grid enumerates (sample, M tile) pairs of the whole batch, so all eight XCDs stay busy whatever M is.
    const int MT = (rows_tot + BM - 1) / BM;
    int nt, mg;
    xcd_tile(a.N / BN, nt, mg);
    const int b = mg / MT, mt_ = mg - b * MT;
    if (b >= nbatch) return;   // padding of the tile count to a multiple of 8 (the whole workgroup exits together)
    const int m0 = mt_ * BM, n0 = nt * BN;
    // grouped launch (a.grp > 1: the positional convolution's 16 groups): the grid's batch axis is (sample, group); a group has its own
    // A columns / weights and writes columns [g col_gs, g col_gs + n_store) of the sample's output rows
    int bs = b, g = 0;
    if constexpr (!BIG) {
        if (a.grp > 1) { bs = b / a.grp; g = b - bs * a.grp; }
    }
    const unsigned short* A = reinterpret_cast<const unsigned short*>(a.a) + (long long)bs * a.a_bs + (long long)g * a.a_gs;
    const unsigned short* A2 = reinterpret_cast<const unsigned short*>(a.a2) + (long long)bs * a.a2_bs;
    const unsigned short* W = reinterpret_cast<const unsigned short*>(a.w) + (long long)g * a.w_gs;
    const int nk = a.K / TBK;
    const int nk1 = (a.a2 ? a.K1 : a.K) / TBK;   // K tiles served by the first A segment

    // global -> register staging: chunk c of a tile: row c >> 3, k piece c & 7 (16 bytes).  TWO register sets: the tile two
    // steps ahead is requested while the current one multiplies, so every load has a whole k-step (plus the other
    // workgroup of the CU) to arrive — one set gave each load only the ~500 clocks of one step's MFMAs.
    struct RegTile { u32x4 a[4]; u32x4 w[WCH]; };
    RegTile S0, S1;
    ofs_t aoff[4], a2off[4], woff[WCH];
    int loff[4], lwoff[WCH];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tid + NTH * i, row = c >> 3, kp = c & 7;
        const int m = min(m0 + row, rows_tot - 1);   // rows past M repeat the last row (never stored)
        aoff[i] = (ofs_t)m * a.lda + kp * 8;
        a2off[i] = (ofs_t)m * a.lda2 + kp * 8;
        loff[i] = row * TLP + kp * 8;
    }
#pragma unroll
    for (int i = 0; i < WCH; ++i) {
        const int c = tid + NTH * i, row = c >> 3, kp = c & 7;
        woff[i] = (ofs_t)(n0 + row) * a.K + kp * 8;
        lwoff[i] = row * TLP + kp * 8;
    }
    auto gload_tile = [&](RegTile& R, int kt) {
        const bool first = kt < nk1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned short* p = first ? A + (aoff[i] + (ofs_t)kt * TBK) : A2 + (a2off[i] + (ofs_t)(kt - nk1) * TBK);
            R.a[i] = *reinterpret_cast<const u32x4*>(p);
        }
#pragma unroll
        for (int i = 0; i < WCH; ++i) R.w[i] = *reinterpret_cast<const u32x4*>(W + (woff[i] + (ofs_t)kt * TBK));
    };
    auto lds_store = [&](const RegTile& R, int buf) {
        unsigned short* pa = lds + buf * BUF;
        unsigned short* pw = pa + BM * TLP;
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<u32x4*>(pa + loff[i]) = R.a[i];
#pragma unroll
        for (int i = 0; i < WCH; ++i) *reinterpret_cast<u32x4*>(pw + lwoff[i]) = R.w[i];
    };

    f32x16 acc0[NJ], acc1[NJ];   // two row tiles per wave (separate arrays: one [2][NJ] array of this size is not promoted to registers)
    tile_clear<NJ>(acc0, acc1);

    const int frow = l & 31, fk = 8 * (l >> 5);
    auto compute = [&](int buf) {
        const unsigned short* pa = lds + buf * BUF;
        const unsigned short* pw = pa + BM * TLP;
        tile_mfma<NJ>(acc0, acc1, wm * 64 + frow, wn * (32 * NJ) + frow,
                      [&](int row, int ks) { return *reinterpret_cast<const bf16x8*>(pa + row * TLP + ks * 16 + fk); },
                      [&](int row, int ks) { return *reinterpret_cast<const bf16x8*>(pw + row * TLP + ks * 16 + fk); });
    };

    // Every load and LDS store of the loop is UNCONDITIONAL (steps past the end re-request the last tile and park it in the
    // buffer nobody reads any more): with memory operations inside run-time branches the compiler's wait-count analysis
    // gives up at the joins and drains every outstanding load (s_waitcnt vmcnt(0)) before it issues the next tile's — which
    // is exactly the overlap the second register set exists for.
    if constexpr (SB) {
        gload_tile(S0, 0);
        lds_store(S0, 0);
        gload_tile(S0, min(1, nk - 1));
        __syncthreads();
        for (int kt = 0; kt < nk; ++kt) {   // LDS holds tile kt, S0 tile kt + 1 (in flight)
            __builtin_amdgcn_sched_barrier(0);
            compute(0);
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();                 // every wave has read tile kt
            lds_store(S0, 0);
            gload_tile(S0, min(kt + 2, nk - 1));
            __syncthreads();
        }
    } else {
    gload_tile(S0, 0);
    gload_tile(S1, min(1, nk - 1));
    lds_store(S0, 0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt += 2) {
        // even step: tile kt multiplies from buffer 0, tile kt + 1 sits in S1, tile kt + 2 is requested into S0
        gload_tile(S0, min(kt + 2, nk - 1));
        __builtin_amdgcn_sched_barrier(0);   // keep the order request -> multiply -> park: the scheduler otherwise hoists the
        compute(0);                          // LDS stores (and the wait for their loads) above the MFMAs
        __builtin_amdgcn_sched_barrier(0);
        lds_store(S1, 1);
        __syncthreads();
        // odd step: tile kt + 1 from buffer 1, tile kt + 2 sits in S0, tile kt + 3 is requested into S1
        gload_tile(S1, min(kt + 3, nk - 1));
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < nk) compute(1);
        __builtin_amdgcn_sched_barrier(0);
        lds_store(S0, 0);
        __syncthreads();
    }
    }

    const int nlim = (!BIG && a.grp > 1) ? g * a.col_gs + a.n_store : 0;
    tile_epilogue<NJ>(a, acc0, acc1, lds, w, l, bs, m0 + wm * 64, n0 + g * a.col_gs + wn * (32 * NJ), nlim);
}

// ------------------------------------------------------------------------------------------------------------------
// tgemm256d_kernel (round 6): the 256 x 256 x 64 tile with its operand tiles fetched global -> LDS DIRECTLY (buffer_load_dwordx4 ... lds): no staging registers, no
// LDS stores, one barrier per k-tile.  Direct loads write a wave's 64 x 16 bytes contiguously (8 rows x 128 bytes: no row padding), so the 16-byte chunks are
// XOR-swizzled instead — LDS chunk p of row r holds the row's k-chunk p ^ swz(r), and a fragment read of chunk c takes p = c ^ swz(r) (TG256D_SWZ below).  Bring-up and knock-outs: scripts/ubench/bgemm.hip (profiles/r06k_bgemm_bringup.txt): the audio encoder's four projection shapes at
// 32 clips take 77 / 28 / 85 / 83 us with a plain store epilogue where tgemm_kernel<128, 128, SB> averages 124 and tgemm_kernel<256, 256> 135; with every load, barrier and
// LDS read of the k16 steps knocked out the loop still takes 63-65 us: prologue, epilogue and three rounds of 256 workgroups are what is left above the MFMAs.
// Same operands, same k order per accumulator as the other bf16 tiles: bit-identical results.  Per-sample operands only (seg_rows == 0), one K segment, N % 256 == 0.
// ------------------------------------------------------------------------------------------------------------------
// The swizzle term of row r.  A 128-byte row is half of the 64 banks (its parity picks the half), and a ds_read_b128 is serviced in FOUR groups of 16 lanes that are NOT
// contiguous — {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 (MI355X_MICROARCH.md, LDS table): a group holds eight rows of each parity, so the eight
// chunk positions must be told apart by (r >> 1) & 7.  The first version used r & 7 — right for sixteen CONSECUTIVE rows — and every fragment read was a 2-way conflict
// (SQ_LDS_BANK_CONFLICT 46 % of the LDS-active cycles: profiles/r06m_sq_lds_l2_counters.txt).
#define TG256D_SWZ(r) (((r) >> 1) & 7)
constexpr int TG256D_TILE = (256 + 256) * 128;                                   // bytes of one buffer: A 256 rows + W 256 rows x 64 bf16
constexpr int TG256D_LDS = 2 * TG256D_TILE > 8 * 32 * (32 * 4 + 4) * 4 ? 2 * TG256D_TILE : 8 * 32 * (32 * 4 + 4) * 4;   // two buffers / the epilogue's per-wave scratch
__global__ __launch_bounds__(512) void tgemm256d_kernel(const TGemmArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned short lds[];
    typedef __attribute__((address_space(3))) void* lds_ptr;
    constexpr int BM2 = 256, BN = 256, NJ = 4;
    char* const ldsb = reinterpret_cast<char*>(lds);
    const int tid = threadIdx.x, l = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = w >> 1, wn = w & 1;
    const int MT = (a.M + BM2 - 1) / BM2;
    int nt, mg;
    xcd_tile(a.N / BN, nt, mg);
    const int b = mg / MT, mt_ = mg - b * MT;
    if (b >= a.batch) return;
    const int m0 = mt_ * BM2, n0 = nt * BN;
    const int nk = a.K / TBK;
    const rsrc_t ra = make_rsrc(reinterpret_cast<const unsigned short*>(a.a) + (long long)b * a.a_bs, (unsigned)(((long long)(a.M - 1) * a.lda + a.K) * 2));
    const rsrc_t rw = make_rsrc(a.w, (unsigned)((long long)a.N * a.K * 2));
    // wave-load j of an operand tile = rows 8 j .. 8 j + 7 (1 KB, contiguous in LDS); lane -> (row 8 j + (l >> 3), LDS chunk l & 7) = the row's k-chunk (l & 7) ^ (l >> 3)
    const int lrow = l >> 3;
    int aoff[4], woff[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = w * 4 + i;
        const int lchunk = (l & 7) ^ TG256D_SWZ(8 * j + lrow);
        aoff[i] = (min(m0 + 8 * j + lrow, a.M - 1) * a.lda + lchunk * 8) * 2;   // rows past M repeat the last row (never stored)
        woff[i] = ((n0 + 8 * j + lrow) * a.K + lchunk * 8) * 2;
    }
    auto issue = [&](int kt, int buf) {
        char* base = ldsb + buf * TG256D_TILE;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = w * 4 + i;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, (lds_ptr)(base + j * 1024), 16, aoff[i], kt * (TBK * 2), 0, 0);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_ptr)(base + BM2 * 128 + j * 1024), 16, woff[i], kt * (TBK * 2), 0, 0);
        }
    };
    f32x16 acc0[NJ], acc1[NJ];
    tile_clear<NJ>(acc0, acc1);
    const int frow = l & 31, fh = l >> 5;
    auto compute = [&](int buf) {
        const char* pa = ldsb + buf * TG256D_TILE;
        const char* pw = pa + BM2 * 128;
        tile_mfma<NJ>(acc0, acc1, wm * 64 + frow, wn * (32 * NJ) + frow,
                      [&](int row, int ks) { return *reinterpret_cast<const bf16x8*>(pa + row * 128 + (((ks * 2 + fh) ^ TG256D_SWZ(row)) << 4)); },
                      [&](int row, int ks) { return *reinterpret_cast<const bf16x8*>(pw + row * 128 + (((ks * 2 + fh) ^ TG256D_SWZ(row)) << 4)); });
    };
    issue(0, 0);
    __builtin_amdgcn_s_waitcnt(0);   // (vmcnt(0): the tile is in LDS)
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        // tile kt + 1 goes into the buffer tile kt - 1 was read from: every wave passed the barrier that ended that step
        if (kt + 1 < nk) issue(kt + 1, (kt + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
        compute(kt & 1);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(0);
        __syncthreads();
    }
    tile_epilogue<NJ>(a, acc0, acc1, lds, w, l, b, m0 + wm * 64, n0 + wn * (32 * NJ));
}

bool tgemm_supports(const TGemmArgs& a) {
    if (a.f32) {   // fp32 kernel: 4-float chunks, 32-float k-tiles; 96- or 128-wide column tiles; batch-as-rows addressing only
        if (!(a.M >= 1 && (a.N % 96 == 0 || a.N % 128 == 0) && a.K >= FBK && a.K % FBK == 0 && a.lda % 4 == 0 && a.seg_rows > 0)) return false;
        if (a.geglu && a.N % 128) return false;
        if (a.a2 && (a.K1 % FBK || a.K1 <= 0 || a.K1 >= a.K || a.lda2 % 4)) return false;
        if (a.geglu && (a.N % 256 || !a.yf)) return false;
        if (a.yb) return false;
    } else
    if (!(a.M >= 1 && a.N >= 64 && a.N % 64 == 0 && a.K >= TBK && a.K % TBK == 0 && a.lda % 8 == 0 && a.a_bs % 8 == 0)) return false;
    if (a.qk && (a.qk_n % 32 || a.head_dim % 32)) return false;
    if (a.a2 && (a.K1 % TBK || a.K1 <= 0 || a.K1 >= a.K || a.lda2 % 8 || a.a2_bs % 8)) return false;
    if (!a.f32 && a.geglu && (a.N % 256 || !a.yb)) return false;   // the GEGLU row interleaving is the 256-wide tile's (tgemm_geglu_src_row)
    if (a.y_cm && (a.cm_pitch % 4 || a.cm_pitch < ((a.M + 3) & ~3))) return false;
    if (a.seg_rows && (a.seg_rows % 32 || a.seg_rows < a.M)) return false;
    if (a.yb && (a.ldy % 8 || a.y_bs % 8)) return false;   // 16-byte bf16 stores
    if ((long long)a.N * a.K > 0x7fffffffLL) return false;   // 32-bit element offsets in the 256-row kernel
    return true;
}
// GEGLU weight-row interleaving for the 256-wide tile: tile-local column tile pairs (2p, 2p + 1) of each wave are (value, gate)
// of the same 32 channels.  Returns the source row (value rows [0, N/2), gate rows [N/2, N)) of permuted row n.
int tgemm_geglu_src_row(int n, int N) {
    const int tile = n / 256, wn = (n % 256) / 128, j = (n % 128) / 32, i = n % 32;
    const int c = tile * 128 + wn * 64 + (j >> 1) * 32 + i;
    return (j & 1) ? N / 2 + c : c;
}
void configure_tgemm_kernel() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tgemm256d_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, TG256D_LDS);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tgemm_kernel<128, 128, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (TBM + 128) * TLP * 2);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tgemm_kernel<128, 128>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (TBM + 128) * TLP * 2);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tgemm_kernel<128, 64>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (TBM + 64) * TLP * 2);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tgemm_kernel<256, 256>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (256 + 256) * TLP * 2);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&tgemm_kernel<256, 192>), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * (256 + 192) * TLP * 2);
    configure_fgemm_kernels();
}
// Which kernel a launch takes (TGemmVariant, tgemm.h): launch_tgemm switches on this and on nothing else.
int tgemm_variant(const TGemmArgs& a, int batch) {
    if (!tgemm_supports(a)) return TG_NONE;
    const long long rows_tot = a.seg_rows > 0 ? (long long)batch * a.seg_rows : a.M;
    const int nb = a.seg_rows > 0 ? 1 : batch;
    if (a.f32) return TG_FGEMM;
    // bf16, batch-as-rows (UNet): the 64-row K-split tile of the fp32 path on bf16 operands.  The kernels' time is their fp32
    // epilogue traffic, and the 256-row tiles give a 192-wide output 152 workgroups on 256 CUs (42.0 -> 35.8 us on the small tile).
    // For q/k/v and GEGLU (456 / 912 big workgroups) the isolated replays of said_profile_unet favour the big tile (29.8 vs 32.7,
    // 69.7 vs 75.0 us) but the real step does not: 122.1 vs 120.3 ms per 32 clips x 50 steps, three alternating runs on one box
    // (scripts/gpu_r2_ak.sh) — one 147 KB-LDS workgroup per CU starts and drains badly between neighbours of other shapes.  So
    // the small tile is the rule.
    if (a.seg_rows > 0 && a.K % 64 == 0 && (!a.a2 || a.K1 % 64 == 0) && (a.N % 96 == 0 || a.N % 128 == 0)) return TG_FGEMM;
    if (a.grp > 1 && (a.seg_rows > 0 || a.a2 || a.n_store < 1 || a.col_gs < a.n_store)) return TG_NONE;   // grouped launches: tgemm_kernel only
    const bool big = a.grp <= 1 && (a.N % 256 == 0 || a.N % 192 == 0) && rows_tot * nb >= 4096 &&
                     (rows_tot + 2) * (long long)std::max(a.lda, a.lda2) < 0x7fffffffLL;
    if (a.geglu && !big) return TG_NONE;   // the GEGLU epilogue needs the 256-wide tile
    // Per-sample operands (audio encoder): a 256-row tile holds one workgroup per CU, so its grid runs in rounds of 256 — the
    // encoder's 768-wide GEMMs at 32 clips x 600 frames are 288 workgroups = two rounds, the second 12 % full.  Where the
    // 128 x 128 tile (two per CU, rounds of 512) fills its rounds clearly better (by a margin of 0.15), it is used instead.
    bool use_big = big;
    if (big && a.seg_rows == 0 && !a.geglu && a.N % 128 == 0) {
        const long long mt_big = (rows_tot + 255) / 256, mt_128 = (a.M + TBM - 1) / TBM;
        const long long g_big = (long long)nb * mt_big * (a.N / (a.N % 256 == 0 ? 256 : 192));
        const long long g_128 = (long long)batch * mt_128 * (a.N / 128);
        // efficiency = how full the rounds are x how full the row tiles are (rows past M repeat the last row: wasted work)
        const double e_big = (double)g_big / (double)(((g_big + 255) / 256) * 256) * (double)rows_tot / (double)(mt_big * 256);
        const double e_128 = (double)g_128 / (double)(((g_128 + 511) / 512) * 512) * (double)a.M / (double)(mt_128 * TBM);
        if (e_128 > e_big + 0.15) use_big = false;
    }
    // round 6: per-sample operands with 256-wide outputs (the audio encoder's projections): the direct-to-LDS 256 x 256 tile (a.direct; said_debug_option "tgemm_direct")
    if (a.direct && a.grp <= 1 && a.seg_rows == 0 && !a.geglu && !a.a2 && a.N % 256 == 0 && a.K % TBK == 0 && (long long)a.M * batch >= 4096 &&
        ((long long)(a.M - 1) * a.lda + a.K) * 2 < 0x7fffffffLL && (long long)a.N * a.K * 2 < 0x7fffffffLL)
        return TG_256D;
    if (a.sb && a.seg_rows == 0 && !a.geglu && a.N % 128 == 0) use_big = false;   // the single-buffer 128 x 128 variant was asked for
    if (use_big) return a.N % 256 == 0 ? TG_256 : TG_256X192;
    if (a.seg_rows > 0) return TG_NONE;   // batch-as-rows addressing needs the 256-row tile
    if (a.N % 128 == 0) return a.sb ? TG_128SB : TG_128;
    return TG_128X64;
}
bool launch_tgemm(const TGemmArgs& a, int batch, hipStream_t s, int* variant) {
    const int v = tgemm_variant(a, batch);
    if (variant) *variant = v;
    if (v == TG_NONE) return false;
    TGemmArgs a2 = a;
    a2.batch = batch;
    if (v == TG_FGEMM) return launch_fgemm(a2, s);
    const long long rows_tot = a.seg_rows > 0 ? (long long)batch * a.seg_rows : a.M;
    const int nb = a.seg_rows > 0 ? 1 : batch;
    const long long mt8_256d = ((long long)batch * ((a.M + 255) / 256) + 7) / 8 * 8;
    const long long mt8_big = ((long long)nb * ((rows_tot + 255) / 256) + 7) / 8 * 8;
    const long long mtiles8 = ((long long)batch * ((a.M + TBM - 1) / TBM) + 7) / 8 * 8;   // (sample, M tile) pairs padded to the 8 XCDs
    switch (v) {
    case TG_256D:
        hipLaunchKernelGGL(tgemm256d_kernel, dim3((unsigned)(mt8_256d * (a.N / 256))), dim3(512), TG256D_LDS, s, a2);
        break;
    case TG_256:
        hipLaunchKernelGGL((tgemm_kernel<256, 256>), dim3((unsigned)(mt8_big * (a.N / 256))), dim3(512), 2 * (256 + 256) * TLP * 2, s, a2);
        break;
    case TG_256X192:
        hipLaunchKernelGGL((tgemm_kernel<256, 192>), dim3((unsigned)(mt8_big * (a.N / 192))), dim3(512), 2 * (256 + 192) * TLP * 2, s, a2);
        break;
    case TG_128SB:
        hipLaunchKernelGGL((tgemm_kernel<128, 128, true>), dim3((unsigned)(mtiles8 * (a.N / 128))), dim3(256), (TBM + 128) * TLP * 2, s, a2);
        break;
    case TG_128:
        hipLaunchKernelGGL((tgemm_kernel<128, 128>), dim3((unsigned)(mtiles8 * (a.N / 128))), dim3(256), 2 * (TBM + 128) * TLP * 2, s, a2);
        break;
    case TG_128X64:
        hipLaunchKernelGGL((tgemm_kernel<128, 64>), dim3((unsigned)(mtiles8 * (a.N / 64))), dim3(256), 2 * (TBM + 64) * TLP * 2, s, a2);
        break;
    default:
        return false;
    }
    return true;
}

}  // namespace said
