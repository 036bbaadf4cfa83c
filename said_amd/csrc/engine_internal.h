// engine_internal.h — what the host modules of libsaid_hip.so share: model constants, weight and activation types, HostCtx (what every
// context owns), the parts said_ctx is the sum of (one per owner and lifetime: ModelWeights, Switches, Cells, Workspace, LazyBuffers,
// StepGraphs, DebugState), the error / allocation / lifecycle helpers and the few functions one module calls in another.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/said_hip.h"
#include "said_hip_debug.h"
#include "kernels.h"
#include "audio_plan.h"
#include "stchain.h"
#include "tgemm.h"

namespace said {
namespace host __attribute__((visibility("hidden"))) {

constexpr int MC = 192;       // model_channels (unet_1d_condition.py:40)
constexpr int TE = 768;       // time_embed_dim = 4 * model_channels
constexpr int HEADS = 6;      // 192 / num_head_channels(32)
constexpr int HD = 32;
constexpr int FFI = 768;      // GEGLU inner dim (4 * 192)
constexpr int NRES = 5, NST = 4;
constexpr int W2V_H = 768, W2V_HEADS = 12, W2V_HD = 64, W2V_FFN = 3072, W2V_CONV = 512;

extern std::string g_create_err;   // the error of a failed said_*_create (engine.cpp)

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
    int64_t numel() const { int64_t n = 1; for (auto d : shape) n *= d; return n; }
};

struct PW {  // packed GEMM weight (up to 2 K-segments) + bias
    float* w[2] = {nullptr, nullptr};
    float* w4[2] = {nullptr, nullptr};   // dwordx4 packing for the LDS-staged kernel
    float* w2[2] = {nullptr, nullptr};   // bf16 packing for the LDS-staged kernel's bf16 MFMA mode (same tails as w4)
    float* ws[2] = {nullptr, nullptr};   // split-fp16 packing (kernels.h Seg::ws; same tails as w4) — UNet weights only (weights.cpp pack_pw_split)
    bool ws_flat = false;                // ws in the flat step layout (GEGLU's one-tile-per-wave shape)
    float* bias = nullptr;
    int N = 0, C[2] = {0, 0}, taps = 1, nseg = 1;
    bool gn_tail = false;                // w4[s] is followed by the GroupNorm gamma[C] and beta[C] of its source segment
    bool ln_tail = false;                // ... and then by the LayerNorm gamma[C] and beta[C]
};
struct ResW { float *g1, *b1, *g2, *b2; PW conv1, conv2, skip; int cin; bool has_skip; float* bias2;
              void *t_conv1 = nullptr, *t_conv2 = nullptr; /* bf16 [192][taps * cin] (conv2: [576 | 384 skip]) for tgemm.hip */
              void *tf_conv1 = nullptr, *tf_conv2 = nullptr; /* the same matrices in fp32 (fgemm_kernel) */
              void *tp_conv1 = nullptr, *tp_conv2 = nullptr; /* ... and as packed split-fp16 pairs (h | l << 16 per element: fgemm_kernel's packed mode, round 6) */ };
struct STW { float *gn_g, *gn_b, *l1g, *l1b, *l2g, *l2b, *l3g, *l3b; PW qkv, out1, q2, out2, ff1, ff2, proj, ffproj;
             void *t_qkv = nullptr, *t_ff1 = nullptr, *t_ffproj = nullptr; float* t_ff1_bias = nullptr; /* bf16 weights for tgemm.hip */
             void *tf_qkv = nullptr, *tf_ff1 = nullptr, *tf_ffproj = nullptr; /* fp32 copies (fgemm_kernel) */
             void* tp_qkv = nullptr; /* q/k/v rows as packed split-fp16 pairs (fgemm_kernel's packed mode) */
             void *t_out1 = nullptr, *t_q2 = nullptr, *t_out2 = nullptr, *tf_out1 = nullptr, *tf_q2 = nullptr, *tf_out2 = nullptr; /* [192][192] (xgemm_kernel) */
             float *chain_w = nullptr, *chain_vec = nullptr; /* round 5: weight stream + vectors of the fused tail (stchain.hip) */
             float* chain_w3 = nullptr; /* round 6: the three-slice stream (small launches: three workgroups per token tile) */
             float* chain_w2 = nullptr; /* ... and the two-slice stream (launches of 86 .. 128 tiles) */
             void* chain_wb = nullptr; /* ... and the bf16 stream (1 KB units) of its bf16-mode variant */ };
struct W2VLayer { PW qkv, out, ff1, ff2; float *ln1g, *ln1b, *ln2g, *ln2b; };

struct ActBuf {  // channel-major activation + its GroupNorm partial statistics
    float* p = nullptr;
    float* st = nullptr;
    void* t = nullptr;   // token-major twin [sample][seg rows][192] in the precision mode's element type (round 3, large batches)
};

// What every engine context owns, the UNet's (said_ctx) and the others' (as their member `c`): device, error strings, host weights,
// allocations.  Not copyable: the lists own device memory.
struct HostCtx {
    int device = 0;
    std::string err;
    std::string launch_err;          // set by a schedule function whose kernel refused its shape; reported by the C-ABI entry point
    std::map<std::string, HostTensor> host_w;
    std::vector<void*> allocs;       // weights, tables and lazily grown buffers: live as long as the context
    std::vector<void*> ws_allocs;    // the (max_batch_eff, max_frames)-sized workspace: replaced as a whole by said_reserve
    std::map<void*, size_t> alloc_bytes;   // size of every live allocation made through dalloc (said_debug_ws_*)
    std::vector<void*>* alloc_list = &allocs;
    HostCtx() = default;
    HostCtx(const HostCtx&) = delete;
    HostCtx& operator=(const HostCtx&) = delete;
};

// ---- the parts of said_ctx: one per owner and lifetime ----

// The model: written by said_create (the dims, the freqs table's allocation) and by weights.cpp up to said_finalize_weights, by nothing afterwards.
// said_clone copies it: a clone's pointers point into the parent's allocations (read-only on the device).
struct ModelWeights {
    int cin = 32, ctx_dim = 768;
    bool finalized = false, has_audio = false, has_audio_proj = false;
    int w2v_layers = 0;
    int w2v_kernel[7] = {0}, w2v_stride[7] = {5, 2, 2, 2, 2, 2, 2};
    int n_set_weight = 0;   // said_set_weight calls so far (tests: capacity growth must not re-upload the weights, and a clone reports its parent's count)

    // ---- UNet weights ----
    PW conv_in, conv_out, te1, te2, emb_all, kv_all;
    float *out_g = nullptr, *out_b = nullptr;
    ResW res[NRES];
    STW st[NST];
    float* null_cond = nullptr;
    float* c2[NST] = {nullptr, nullptr, nullptr, nullptr};   // attn2 output of the unconditional half: to_out(to_v(null_cond_emb)) + bias, per block
    float* freqs = nullptr;
    bool freqs_set = false;
    bool split_unsafe = false;   // a weight tensor lies outside the split-fp16 representation's range (scan_split_range): SAID_PREC_FP32 then runs as SAID_PREC_FP32_STRICT
    std::string split_note;      // ... which tensor and why (said_precision_note)

    // ---- audio encoder weights ----
    float *c0_w = nullptr, *c0_g = nullptr, *c0_b = nullptr;
    PW aconv[7];
    float *fp_lng = nullptr, *fp_lnb = nullptr, *enc_lng = nullptr, *enc_lnb = nullptr;
    float* mask_embed = nullptr;   // audio_encoder.masked_spec_embed [768], or null: optional, read by said_audio_encode_train's time mask only
    PW fproj, posconv, aproj;
    std::vector<W2VLayer> layers;

    // ---- bf16 audio encoder (tgemm.hip): bf16 weights [N][K] (convs: K = tap-major) ----
    void* bw_conv[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    void *bw_fproj = nullptr, *bw_aproj = nullptr;
    void* bw_out = nullptr;   // out.2 weights bf16 [in_channels][3 taps][192] for out_sched_tm_kernel (round 4)
    void* bw_pos = nullptr;       // positional conv as 16 GEMMs: bf16 [16][64 (48 + 16 zero rows)][taps * 48], tap-major
    float* pos_bias_pad = nullptr; // its bias, 16 zeros appended (the last group's 64-wide tile reads past 768)
    struct BLayer { void *qkv, *out, *ff1, *ff2; };
    std::vector<BLayer> blayers;
};

// The precision mode and the schedule switches: written by said_set_precision and said_debug_option only, read by the schedules.  said_clone copies it.
struct Switches {
    bool bf16_mode = false;  // said_set_precision(SAID_PREC_BF16): multiply in bf16 wherever the LDS-staged kernel is used
    int prec_mode = 0;       // the SAID_PREC_* mode asked for (said_set_precision)
    int st_chain_bf16 = -1;      // bf16 mode, large batches: the same fused tail on bf16 operands instead of rgemm's five launches; 0: off; -1 / 1: stchain_kernel<true> (one token tile per
                                 // workgroup, two workgroups per CU; said_debug_option "st_chain_bf16").  (Round 5's two-tiles-per-workgroup variant measured slower — 96 vs 83 us,
                                 // profiles/r05p_stchain2_two_tiles_ab.txt — and was removed in round 6.)
    int attn_2q = -1;            // fp32 mode, pre-split K / V, four key slices: three query tiles per wave (attn2q_kernel) — -1: launches of >= 512 (sample, head, tile) triples, 0: never, 1: always (said_debug_option "attn_2q")
    int st_chain_slices = -1;    // fp32 mode: -1 / 3: launches of at most CHAIN3_MAX_TILES (sample, token tile) pairs run THREE workgroups per tile, of at most CHAIN2_MAX_TILES two
                                 // (stchain.hip CU<>); 2: two wherever slicing is possible; 1: never
                                 // (said_debug_option "st_chain_slices")
    int st_chain = -1;           // fp32 mode, small batches: everything behind self-attention as ONE launch per block (stchain.hip); 0: the five launches
                                 // (said_debug_option "st_chain")
    int out_tm = -1;          // the token-major out + scheduler kernel behind the bf16 large-batch schedule (said_debug_option "out_tm": 0 off)
    int tm_acts = -1;         // bf16 mode, large batches: token-major bf16 activations BETWEEN the UNet kernels, operand transforms inside the GEMMs (-1 / 1: on; 0: the
                              // channel-major schedule with preparation kernels — said_debug_option "tm_acts").  The fp32 twin of this schedule (round 3: 4.78 vs 4.41 ms per
                              // step at 32 clips) was removed in round 6 together with xgemm_kernel's fp32 instantiations.
    int tgemm_direct = -1;    // audio encoder (bf16): the projections on tgemm256d_kernel (256 x 256 tile, operand tiles loaded straight into LDS; -1 / 1: on, 0: tgemm_kernel<128, 128> — said_debug_option "tgemm_direct")
    int attn_split = -1;      // fp32 mode: both attention products on split-fp16 operands (attn.hip: PM == 2; x = h + 2^-11 l: 22-bit significands, fp32 accumulation,
                              // as close to a float64 evaluation as the fp32 MFMAs: tests/test_gpu_round4.py).  Default (-1) and 1: ON since round 5; 0: v_mfma_f32_32x32x2_f32
                              // on the fp32 operands (said_debug_option "attn_split").  Round 4 shipped it opt-in because runs beside other streams were not bit-stable;
                              // round 5 found the mechanism in OTHER kernels' packed-fp32 instructions (split_f16.h, build.py NO_SLP) and removed it.
    int gemm_presplit = -1;   // fp32 mode, large batches: the ResBlock convolutions' and q / k / v's operands reach fgemm_kernel already split (prep_kernel packs the activations,
                              // the weights have a packed copy): -1 / 1 on; 0: fp32 operands split in the k loop (said_debug_option "gemm_presplit"; bit-identical)
    int gemm_split = -1;      // fp32 mode: the large-batch token-major GEMMs (fgemm_kernel) on split-fp16 operands (fgemm.hip: SP).  Default (-1) and 1: ON since round 5
                              // (as above); 0: fp32 MFMAs (said_debug_option "gemm_split").
    int attn_presplit = -1;   // fp32 small batch: the q/k/v GEMM stores k and v as packed split-fp16 pairs and attn_kernel<PM = 3> unpacks them instead of splitting all of K and V
                              // again in each of a sample's query-tile workgroups (-1 / 1: on; 0: off — said_debug_option "attn_presplit")
    int out_split = -1;       // out_sched_kernel's convolution on split-fp16 operands (-1 / 1: on; 0: fp32 matrix instructions — said_debug_option "out_split")
    int kconv = -1;           // fp32 mode, small batch: the K-long ResBlock convolutions of the up path as straight-line two- / three-block waves (gemm_lds.hip kconv_body; -1 / 1: on,
                              // 0: ugemm_body's block loop — said_debug_option "kconv"; bit-identical)
    int chain_coef = -1;      // fp32 small batch: stchain_kernel takes the block input's GroupNorm coefficients from the q/k/v GEMM (-1 / 1: on; 0: finalises them itself — said_debug_option "chain_coef")
    int ugemm_split = -1;     // fp32 mode: the small-batch channel-major GEMMs (ugemm_kernel) on split-fp16 operands too (gemm_lds.hip: SP; weights pre-split on the host:
                              // Seg::ws).  Default (-1) and 1: ON; 0: fp32 MFMAs (said_debug_option "ugemm_split")
    // tokens per launch from which the token-major GEMM path is taken (measured crossovers, scripts/gpu_r2_w.sh: bf16 between 4800
    // and 6000 tokens, fp32 between 9600 and 10800; said_debug_option "unet_tgemm_min_tokens" overrides both)
    // (bf16: 3000 since round 4 — with the persistent kernels the crossover sits between 2400 rows (2 clips x 600 frames under guidance: 21.9 vs 22.6 ms per
    //  50 steps) and 3600 (3 clips: 30.3 vs 22.7 ms); rounds 2-3: 5800)
    long long unet_tgemm_min_tokens = 3000, unet_fgemm_min_tokens = 10000;
    long long unet_fgemm_min_concurrent = 6000;   // fp32 threshold while other contexts' loops run beside this one (said_loop_params::concurrent)
    int spg_limit = 50;      // denoise steps captured per graph in loops of >= 400 steps, at most 10 below (steps_per_graph; round 6: 10 -> 50: at 0.245 ms per step the 100 graph boundaries of a 1000-step loop were 0.4-0.5 % of it — headline
                             // 2424-2429 -> 2435-2438 frames/s; 100 / 250 / 500 add nothing: profiles/r06l_steps_per_graph.txt)
    int audio_chunk = 32;    // clips per audio-encoder pass
    int audio_train_sites = -1;  // said_audio_encode_train: which kinds of dropout site draw a mask — bits 1 feature projection, 2 encoder front, 4 probabilities, 8 attention output,
                                 // 16 activation, 32 FFN output; -1: all (said_debug_option "audio_train_sites": tests isolate the three sites that share p_hidden)
    int audio_stop_after = -1;   // audio encoder (bf16 branch and fp32 branch outside train mode): issue only the first n stages of each pass (said_debug_option "audio_stop_after"; < 0: all) — host side only
};

// The fixed-size device cells: allocated once by alloc_cells (said_create and said_clone), written by the entry points and kernels of their own context only.
struct Cells {
    float* coef1_dev = nullptr;  // one row for said_ddim_step
    int* step_dev = nullptr;
    int* status_dev = nullptr;   // [2] sticky numeric status of the last loop / forward call (said_numeric_status)
    int* chain_ticket = nullptr; // the sliced fused tail's arrival counters [CHAIN2_MAX_TILES][6]: zero between launches (not part of the workspace: said_debug_ws_fill must not touch them)
    unsigned* seed_dev = nullptr;  // [2] Philox key of the loop's eta noise (said_loop_params::noise_seed)
    long long* clk_dev = nullptr;  // [64 launches][8 waves][8 slots]
};

// The (max_batch_eff, max_frames)-sized workspace: every pointer is assigned by alloc_workspace (said_create, said_clone, said_reserve) and by nothing else; the band
// and key-major-copy descriptions say what set_band and run_kv last put into it.
struct Workspace {
    int maxBe = 0, maxT = 0;
    int maxTp = 0, maxNp = 0;
    float *x_cm = nullptr, *eps_cm = nullptr;
    ActBuf H0, H1, P, Q, M;
    float *X1 = nullptr, *X2 = nullptr, *X3 = nullptr, *O = nullptr, *QK = nullptr, *VT = nullptr, *F = nullptr;
    float *KV = nullptr, *CTX = nullptr;
    float* KVT = nullptr;        // key-major copy of KV [sample][S][NST * 2 * MC] for the fused SpatialTransformer tail (stchain.hip), made by run_kv
    int kvt_S = -1;              // key count of the key-major copy KVT as run_kv last made it (-1: not made — the fused tail then does not run: ADVICE r5)
    int kvt_bf16 = 0;            // ... and its element type
    float* chain_part = nullptr; // the sliced fused tail's partial sums [CHAIN3_MAX_TILES][3][6][16][64]
    float *E0 = nullptr, *E1 = nullptr, *E2 = nullptr, *EO = nullptr;
    long long* ts_dev = nullptr;
    float* coef_dev = nullptr;
    float* axpby_coef = nullptr;
    int *band_lo = nullptr, *band_hi = nullptr;
    int band_T = -1, band_S = -1, band_wmax = 0;
    bool band_chain_ok = false;  // the alignment band fits stchain's window tile (set_band)
    float *init_cm = nullptr, *enoise_cm = nullptr, *mask_cm = nullptr, *rescale_part = nullptr;
    float* x0h_cm = nullptr;     // DPM-Solver++: the previous step's x0, x_cm's layout (each element read and written by the thread that owns it)
    // bf16-mode UNet at large batch: token-major bf16 GEMM operands (tgemm.hip) prepared from the channel-major fp32 activations
    float* gn_coef = nullptr;   // [maxBe][192][2] GroupNorm coefficients of a block input (PrepArgs::coef_out / GemmCommon::gn_coef_out / gn_coef_kernel; room for two)
    void *uPA = nullptr, *uPB = nullptr, *uPL = nullptr, *uPH = nullptr, *uPX = nullptr;   // conv operand [Be][T+2][384], raw cat input
                                                                                            // [Be][T][384], LN'd [Be][T][192], GEGLU out [Be][T][768], raw x2 [Be][T][192]
    void *tX1 = nullptr, *tX2 = nullptr, *tO = nullptr, *tF = nullptr;   // token-major x1, x2, attention output [.][192], GEGLU product [.][768]
};

// The lazily grown buffers: each grows (drealloc) in the call that first needs more, on its own context's stream; empty in a new context and in a new clone.
struct LazyBuffers {
    // ---- fp32 audio workspace ----
    float *abufA = nullptr, *abufB = nullptr; size_t abuf_elems[2] = {0, 0};
    float *aH = nullptr, *aT = nullptr, *aO = nullptr, *aQK = nullptr, *aVT = nullptr, *aF = nullptr, *aPOS = nullptr, *aX = nullptr;
    size_t a_tok_elems = 0;
    // ---- bf16 audio encoder (tgemm.hip): token-major workspace ----
    void *bA0 = nullptr, *bA1 = nullptr, *bX = nullptr, *bHb = nullptr, *bF = nullptr, *bO = nullptr;
    float *bH = nullptr, *bT = nullptr, *bPosT = nullptr;
    size_t b_conv_elems[2] = {0, 0}, b_tok = 0;
    void* bXg = nullptr;          // per-group operand [clips][16][R][48] bf16
    size_t bXg_elems = 0;
    // ---- the loop's step noise, channel-major (said_loop_params::step_noise_dev) ----
    float* noise_cm = nullptr; size_t noise_cm_elems = 0;
};

// The captured step graphs: built by build_step_graphs, dropped by drop_graphs; gkey is cleared by whatever makes the cached graph stale.
struct StepGraphs {
    hipStream_t cap_stream = nullptr;  // private stream used only to capture the per-step graph
    hipGraph_t graph = nullptr, graph_rem = nullptr;       // `gspg` consecutive steps / the N % gspg remaining steps
    hipGraphExec_t gexec = nullptr, gexec_rem = nullptr;
    std::vector<long long> gkey;
    int gspg = 1;            // denoise steps captured per graph
    int gnodes = 0;
};

// Debug and counter state: the said_debug_* / said_profile_unet entry points write the switches, the schedules count their launches; a new context and a new clone start at zero.
struct DebugState {
    int dbg_stop = -1, dbg_count = 0, dbg_only = -1;
    bool log_on = false;
    struct StageInfo { int kind, epi, NB, KS; double bytes, flops; };
    std::vector<StageInfo> stage_log;
    bool clk_on = false;
    bool xclk_on = false;
    long long n_rgemm = 0;
    long long n_stchain = 0;  // launches issued through stchain_kernel (said_debug_get)
    long long n_out_sched = 0, n_out_sched_tm = 0, n_sched_step = 0;   // ... through the step's last kernel: out_sched_kernel, out_sched_tm_kernel, sched_step_kernel
    long long n_xgemm = 0;    // launches issued through round 3's xgemm_kernel (said_debug_get; n_rgemm: through rgemm_kernel)
    long long n_tgemm[TG_NVARIANTS] = {0};   // the bf16 encoder's launch_tgemm calls per kernel (tgemm.h TGemmVariant; said_debug_get "n_tgemm_*")
    long long n_audio_attn[2] = {0, 0};      // ... and its attention launches: [0] eight key slices + cm_to_tm_bf16, [1] no key split, token-major bf16 store
    long long n_audio_attn_f32[3] = {0, 0, 0};   // the fp32 encoder's attention launches (attn_kernel<2, KS, PM 2 / PM 0>) with [0] eight, [1] four key slices, [2] no key split
    long long n_audio_clips = 0;   // clips encoded by said_audio_encode so far (tests: identical rows of a batch are encoded once)
};

}  // namespace host
}  // namespace said

using namespace said;
using namespace said::host;

// The UNet context of the C ABI (said_hip.h): the sum of the parts above and the few fields of the context itself.
struct said_ctx : HostCtx, ModelWeights, Switches, Cells, Workspace, LazyBuffers, StepGraphs, DebugState {
    bool is_clone = false;           // said_clone: the packed weights and tables belong to the parent context
    hipStream_t own_stream = nullptr;  // a clone's stream (said_stream): from the process-wide pool (engine.cpp), never destroyed
    int n_clones = 0;                  // clones made of this context so far (picks the pool slot)
    bool cur_concurrent = false;       // the running loop's said_loop_params::concurrent
    unsigned seed_host[2] = {0, 0};    // staging of seed_dev
};

namespace said {
namespace host __attribute__((visibility("hidden"))) {

int fail(HostCtx* c, const char* fmt, ...);
// Every said_*_create: `device` exists and is a gfx950, and is made current (the caller holds a DeviceRestore); failures are create errors
// ("<entry>: ...", said_*_last_error(NULL)).
int open_device(const char* entry, int device);
// Every said_*_destroy: frees the context's device allocations with its device made current (the caller holds a DeviceRestore).
void free_allocs(HostCtx* c);

// fp32 mode multiplies on split-fp16 operands (split_f16.h) unless the caller asked for strict fp32 (said_set_precision) or the weights do not fit the
// representation (scan_split_range): `opt` is one of the per-kernel-family development switches (said_debug_option), all on by default.
inline bool strict_f32(const said_ctx* c) { return !c->bf16_mode && (c->prec_mode == SAID_PREC_FP32_STRICT || c->split_unsafe); }
inline bool sp_on(const said_ctx* c, int opt) { return opt != 0 && !strict_f32(c); }

// -DSAID_TRACE (SAID_EXTRA_DEFS): every UNet launch is reported on stderr and synchronised
#ifdef SAID_TRACE
constexpr bool trace_on() { return true; }
#else
constexpr bool trace_on() { return false; }
#endif

#define TRACE(msg) do { if (trace_on()) { fprintf(stderr, "[said] %s:%d %s\n", __FILE__, __LINE__, msg); fflush(stderr); } } while (0)

#define HIPCHK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) return fail(ctx, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// a schedule function's kernel refused its shape (nothing was launched for it): report instead of continuing
#define LAUNCHCHK()                                                                                   \
    do {                                                                                              \
        if (const char* f_ = launch_fault_peek()) { const std::string m_ = f_; launch_fault_clear(); ctx->launch_err.clear(); return fail(ctx, "%s", m_.c_str()); } \
        if (!ctx->launch_err.empty()) { const std::string m_ = ctx->launch_err; ctx->launch_err.clear(); return fail(ctx, "%s", m_.c_str()); } \
    } while (0)

inline int rup(int v, int m) { return (v + m - 1) / m * m; }

// said_create / said_destroy must not change the calling thread's current device as a side effect
struct DeviceRestore {
    int prev = -1;
    DeviceRestore() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    ~DeviceRestore() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// The lifecycle of the contexts that hold their HostCtx as the member `c` (said_vae, said_metrics, said_optimize, said_train, said_unet_train, said_render,
// said_jpeg, said_beat).  new_ctx is the head of said_*_create — the caller holds a DeviceRestore, which has to outlive the allocations that follow: the new
// context on `device`, or nullptr with the create error set.
template <typename C>
C* new_ctx(const char* entry, C** out, int device) {
    if (!out) { fail(nullptr, "%s: out is null", entry); return nullptr; }
    *out = nullptr;
    if (open_device(entry, device)) return nullptr;
    C* x = new C();
    x->c.device = device;
    return x;
}
// ... said_*_destroy, for what the allocation lists own: a context with streams, graphs or events of its own releases those first
template <typename C>
int delete_ctx(C* x) {
    if (!x) return 0;
    DeviceRestore restore_device;
    free_allocs(&x->c);
    delete x;
    return 0;
}
// ... and said_*_last_error
template <typename C>
const char* ctx_error(const C* x) { return x ? x->c.err.c_str() : g_create_err.c_str(); }

template <typename T>
int dalloc(HostCtx* ctx, T** out, size_t n, bool zero = true) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
    if (zero) HIPCHK(hipMemset(p, 0, std::max<size_t>(n, 1) * sizeof(T)));
    ctx->alloc_list->push_back(p);
    ctx->alloc_bytes[p] = std::max<size_t>(n, 1) * sizeof(T);
    *out = static_cast<T*>(p);
    return 0;
}
// grow-on-demand buffers: the buffer being replaced is released (the caller has synchronised the stream that used it)
template <typename T>
int drealloc(HostCtx* ctx, T** out, size_t n, bool zero = true) {
    if (*out) {
        auto it = std::find(ctx->allocs.begin(), ctx->allocs.end(), static_cast<void*>(*out));
        if (it != ctx->allocs.end()) ctx->allocs.erase(it);
        HIPCHK(hipFree(*out));
        *out = nullptr;
    }
    return dalloc(ctx, out, n, zero);
}

// ---- weights (weights.cpp) ----
int upload(HostCtx* ctx, float** out, const float* h, size_t n);   // n host floats -> a new device array owned by the context
// the host tensor `name` of exactly `shape`; nullptr (and the context's error set) if it is missing or has another shape
const HostTensor* getw(HostCtx* ctx, const std::string& name, std::initializer_list<int64_t> shape);
// Linear/conv weight `wname` (N, Ctot[, taps]) packed for the GEMM kernels, without the UNet's split-fp16 packing
int make_pw(HostCtx* ctx, PW* pw, const std::string& wname, const std::string& bname, int N, int Ctot, int taps, int nseg = 1,
            const std::string& gn_gamma = "", const std::string& gn_beta = "", const std::string& ln_gamma = "",
            const std::string& ln_beta = "");

// ---- context (engine.cpp) ----
int check_ready(said_ctx* ctx);   // 0 once said_finalize_weights has run, else -1 with the error set

// ---- UNet launch schedules (unet_sched.cpp) ----
// (LaunchCfg and pick_cfg: audio_plan.h)
Seg mkseg(const float* x, long long bstride, int pitch, int C, int taps, int pad, int stride, int Tin, int xform, const float* w);
GemmArgs mkargs(int T, int N);
// geometry of one UNet evaluation
struct UGeo {
    int Be, B_lat /* latents batch (b_mod) */, T, Tp, np /* GN partials per channel */, S, Sp;
    long long hs;      // batch stride of a 192-channel activation
    long long sts;     // batch stride of its stats
    const int* step_ptr;
    int emb_b_stride;
    int* step_inc;     // if set: the first kernel of the schedule increments this counter
    const OutSchedArgs* out_sched;   // if set: the `out` conv is fused with the scheduler update (loop only)
    int Bc;            // > 0: classifier-free guidance over Bc clips — samples [0, Bc) are the unconditional half (context =
                       // null_cond_emb repeated), [Bc, 2 Bc) the conditional half, both on the SAME latents and timestep
                       // (diffusion.py:397-400, 421-423).  Then (a) everything before the first cross-attention is computed
                       // once per clip, (b) the unconditional half's cross-attention output is the constant c2[blk].
};
UGeo make_geo(said_ctx* c, int Be, int B_lat, int T, int S);
void run_unet(said_ctx* c, const UGeo& g, hipStream_t s);
void run_time_embed(said_ctx* c, int n, hipStream_t s);
void run_kv(said_ctx* c, int b0, int nb, int S, int Sp, hipStream_t s);
int set_band(said_ctx* ctx, int T, int S, hipStream_t s);

}  // namespace host
}  // namespace said
