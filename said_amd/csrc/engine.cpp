// engine.cpp — the UNet context's lifecycle (create, reserve, clone and the stream pool), SAID.forward, the hipGraph-replayed
// denoising loop, the scheduler / noise / precision entry points and the debug and profiling entry points of the C ABI.
#include <cstdarg>
#include <mutex>

#include "audio_train.h"
#include "engine_internal.h"

namespace said {
namespace host {

std::string g_create_err;

int fail(HostCtx* c, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_err = buf;
    return -1;
}

int open_device(const char* entry, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(nullptr, "%s: no HIP device visible (this library has no CPU path)", entry);
    if (device < 0 || device >= ndev) return fail(nullptr, "%s: device %d out of range (%d visible)", entry, device, ndev);
    hipDeviceProp_t prop;
    if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(nullptr, "%s: cannot query device %d", entry, device);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return fail(nullptr, "%s: device is %s; this library is built for gfx950 only", entry, prop.gcnArchName);
    return 0;
}

void free_allocs(HostCtx* c) {
    (void)hipSetDevice(c->device);
    for (void* p : c->allocs) (void)hipFree(p);
    for (void* p : c->ws_allocs) (void)hipFree(p);
    c->allocs.clear();
    c->ws_allocs.clear();
}

int check_ready(said_ctx* ctx) {
    if (!ctx) return -1;
    if (!ctx->finalized) return fail(ctx, "weights not finalized: call said_finalize_weights first");
    return 0;
}

}  // namespace host
}  // namespace said

namespace {

// The capture streams exist only while a graph is being built: a live stream holds one of the device's few hardware queues
// (four by default), and streams beyond that count share queues, which serialises launches the caller meant to run side by
// side (the clip groups' loops).
static int ensure_cap_streams(said_ctx* ctx) {
    if (!ctx->cap_stream) HIPCHK(hipStreamCreateWithFlags(&ctx->cap_stream, hipStreamNonBlocking));
    return 0;
}
static void release_cap_streams(said_ctx* ctx) {
    if (ctx->cap_stream) (void)hipStreamDestroy(ctx->cap_stream);
    ctx->cap_stream = nullptr;
}

// The fixed-size device cells of a context (Cells), for said_create and said_clone.
int alloc_cells(said_ctx* ctx) {
    int rc = 0;
    rc |= dalloc(ctx, &ctx->coef1_dev, 8);
    rc |= dalloc(ctx, &ctx->step_dev, 4);
    rc |= dalloc(ctx, &ctx->status_dev, 4);
    rc |= dalloc(ctx, &ctx->chain_ticket, CHAIN2_MAX_TILES * 6);
    rc |= dalloc(ctx, &ctx->seed_dev, 4);
    rc |= dalloc(ctx, &ctx->clk_dev, 64 * 128);
    return rc;
}

// The workspace of a context: every buffer whose size depends on (max_batch_eff, max_frames).  Allocated by said_create and
// replaced as a whole by said_reserve; weights, packed tables and the lazily grown audio / noise buffers are not touched.
int alloc_workspace(said_ctx* ctx, int max_batch_eff, int max_frames) {
    ctx->maxBe = max_batch_eff; ctx->maxT = max_frames;
    ctx->maxTp = rup(max_frames, 32);
    ctx->maxNp = rup(std::max(1024, max_batch_eff), 32);
    ctx->alloc_list = &ctx->ws_allocs;
    const size_t Be = max_batch_eff, Tp = ctx->maxTp, np = Tp / 32;
    const int ctx_dim = ctx->ctx_dim;
    int rc = 0;
    const size_t act = Be * MC * Tp, stt = Be * MC * np * 2;
    rc |= dalloc(ctx, &ctx->x_cm, Be * 32 * Tp);
    rc |= dalloc(ctx, &ctx->eps_cm, Be * 32 * Tp);
    for (ActBuf* a : {&ctx->H0, &ctx->H1, &ctx->P, &ctx->Q, &ctx->M}) { rc |= dalloc(ctx, &a->p, act); rc |= dalloc(ctx, &a->st, stt); }
    rc |= dalloc(ctx, &ctx->X1, act); rc |= dalloc(ctx, &ctx->X2, act); rc |= dalloc(ctx, &ctx->X3, act);
    rc |= dalloc(ctx, &ctx->O, 2 * act);  // same batch stride as QK so attention can share one stride
    rc |= dalloc(ctx, &ctx->QK, 2 * act);
    rc |= dalloc(ctx, &ctx->VT, Be * HEADS * Tp * HD);
    rc |= dalloc(ctx, &ctx->F, Be * FFI * Tp);
    rc |= dalloc(ctx, &ctx->KV, Be * NST * 2 * MC * Tp);
    rc |= dalloc(ctx, &ctx->KVT, Be * NST * 2 * MC * Tp);
    rc |= dalloc(ctx, &ctx->chain_part, (size_t)256 * 6 * 16 * 64);   // (85 x 3 or 128 x 2 workgroups)
    rc |= dalloc(ctx, &ctx->CTX, Be * (size_t)ctx_dim * Tp);
    const size_t Np = ctx->maxNp;
    rc |= dalloc(ctx, &ctx->E0, MC * Np); rc |= dalloc(ctx, &ctx->E1, TE * Np); rc |= dalloc(ctx, &ctx->E2, TE * Np);
    rc |= dalloc(ctx, &ctx->EO, NRES * MC * Np);
    rc |= dalloc(ctx, &ctx->ts_dev, Np); rc |= dalloc(ctx, &ctx->coef_dev, Np * 8);
    rc |= dalloc(ctx, &ctx->axpby_coef, 2 * Np);
    rc |= dalloc(ctx, &ctx->band_lo, Tp); rc |= dalloc(ctx, &ctx->band_hi, Tp);
    rc |= dalloc(ctx, &ctx->init_cm, Be * 32 * Tp); rc |= dalloc(ctx, &ctx->enoise_cm, Be * 32 * Tp); rc |= dalloc(ctx, &ctx->mask_cm, Be * 32 * Tp);
    rc |= dalloc(ctx, &ctx->rescale_part, Be * 2 * 64 * 3);
    {   // operand buffers of the large-batch token-major path (sized for fp32 elements; zero-initialised, so padding rows start at 0)
        const size_t Tm = (size_t)rup(max_frames + 2, 32);   // tg_rows(): per-sample row pitch
        rc |= dalloc(ctx, reinterpret_cast<uint16_t**>(&ctx->uPA), 2 * (Be * Tm * 2 * MC + 4096));
        rc |= dalloc(ctx, reinterpret_cast<uint16_t**>(&ctx->uPB), 2 * (Be * Tm * 2 * MC + 4096));
        rc |= dalloc(ctx, reinterpret_cast<uint16_t**>(&ctx->uPL), 2 * (Be * Tm * MC + 4096));
        rc |= dalloc(ctx, reinterpret_cast<uint16_t**>(&ctx->uPH), 2 * (Be * Tm * FFI + 4096));
        rc |= dalloc(ctx, reinterpret_cast<uint16_t**>(&ctx->uPX), 2 * (Be * Tm * MC + 4096));
        rc |= dalloc(ctx, &ctx->gn_coef, 2 * Be * 2 * MC);
    }
    {   // token-major activations of the round-3 large-batch path: sample pitch = frames rounded up to 64 tokens, fp32-sized
        const size_t seg = (size_t)rup(max_frames, 64), tm = Be * seg * MC + 4096;
        for (ActBuf* a : {&ctx->H0, &ctx->H1, &ctx->P, &ctx->Q, &ctx->M}) rc |= dalloc(ctx, reinterpret_cast<float**>(&a->t), tm);
        rc |= dalloc(ctx, reinterpret_cast<float**>(&ctx->tX1), tm);
        rc |= dalloc(ctx, reinterpret_cast<float**>(&ctx->tX2), tm);
        rc |= dalloc(ctx, reinterpret_cast<float**>(&ctx->tO), tm);
        rc |= dalloc(ctx, reinterpret_cast<float**>(&ctx->tF), Be * seg * FFI + 4096);
    }
    rc |= dalloc(ctx, &ctx->x0h_cm, Be * 32 * Tp);   // (last: the workspace-inspection indices of the buffers above stay)
    ctx->alloc_list = &ctx->allocs;
    ctx->band_T = ctx->band_S = -1;   // the band tables are part of the workspace
    ctx->kvt_S = -1;                  // ... and so is the key-major K / V copy
    return rc;
}

void drop_graphs(said_ctx* ctx) {
    if (ctx->gexec) { (void)hipGraphExecDestroy(ctx->gexec); ctx->gexec = nullptr; }
    if (ctx->graph) { (void)hipGraphDestroy(ctx->graph); ctx->graph = nullptr; }
    if (ctx->gexec_rem) { (void)hipGraphExecDestroy(ctx->gexec_rem); ctx->gexec_rem = nullptr; }
    if (ctx->graph_rem) { (void)hipGraphDestroy(ctx->graph_rem); ctx->graph_rem = nullptr; }
    ctx->gkey.clear();
    ctx->gnodes = 0;
}

}  // namespace

// ============================================================================================
// C ABI
// ============================================================================================
extern "C" {

int said_abi_version(void) { return 9; }   // 9: said_set_precision modes (SAID_PREC_FP32_STRICT), said_effective_precision, said_precision_note, said_numeric_status; 8: said_loop_progress_reset; 7: said_debug_ws_*; 6: said_loop_progress; 5: said_clone, said_loop_params::noise_batch_offset; 4: said_reserve, noise_seed, said_philox_normal, said_debug_option

const char* said_last_error(const said_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int said_create(said_ctx** out, int device, int max_batch_eff, int max_frames, int in_channels, int ctx_dim) {
    if (!out) return fail(nullptr, "said_create: out is null");
    *out = nullptr;
    DeviceRestore restore_device;
    if (open_device("said_create", device)) return -1;
    if (max_batch_eff < 1 || max_frames < 1) return fail(nullptr, "said_create: bad sizes");
    if (in_channels != 32) return fail(nullptr, "said_create: in_channels must be 32 (got %d)", in_channels);
    if (ctx_dim < 16 || ctx_dim % 16) return fail(nullptr, "said_create: ctx_dim must be a positive multiple of 16 (got %d)", ctx_dim);
    said_ctx* ctx = new said_ctx();
    ctx->device = device; ctx->cin = in_channels; ctx->ctx_dim = ctx_dim;
    configure_gemm_kernels();
    configure_ugemm_kernels();
    configure_stchain_kernel();
    configure_attn_kernels();
    configure_audio_train_kernels();
    configure_out_sched_kernel();
    configure_tgemm_kernel();
    configure_xgemm_kernels();
    configure_rgemm_kernels();

    int rc = alloc_cells(ctx);
    rc |= dalloc(ctx, &ctx->freqs, MC / 2);
    rc |= alloc_workspace(ctx, max_batch_eff, max_frames);
    if (rc) { g_create_err = ctx->err; said_destroy(ctx); return -1; }
    *out = ctx;
    return 0;
}

int said_destroy(said_ctx* ctx) {
    if (!ctx) return 0;
    DeviceRestore restore_device;
    (void)hipSetDevice(ctx->device);
    drop_graphs(ctx);
    release_cap_streams(ctx);   // (own_stream belongs to the pool)
    free_allocs(ctx);
    delete ctx;
    return 0;
}

int said_reserve(said_ctx* ctx, int max_batch_eff, int max_frames) {
    if (!ctx) return -1;
    if (max_batch_eff < 1 || max_frames < 1) return fail(ctx, "said_reserve: bad sizes");
    if (max_batch_eff <= ctx->maxBe && max_frames <= ctx->maxT) return 0;
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    // earlier calls may still be running on any stream: the buffers they use are about to be freed
    HIPCHK(hipDeviceSynchronize());
    drop_graphs(ctx);   // the captured step graphs hold the old buffers' addresses
    for (void* p : ctx->ws_allocs) (void)hipFree(p);
    ctx->ws_allocs.clear();
    const int want_be = std::max(max_batch_eff, ctx->maxBe), want_t = std::max(max_frames, ctx->maxT);
    if (alloc_workspace(ctx, want_be, want_t)) {
        // Out of memory part-way through: the old workspace is gone and some members still hold its (freed) addresses.  Release what was
        // obtained and advertise NO capacity — every entry point then refuses its sizes instead of running on freed memory — until a
        // later said_reserve (e.g. with a smaller batch) succeeds and re-assigns every workspace pointer.
        const std::string why = ctx->err;
        for (void* p : ctx->ws_allocs) (void)hipFree(p);
        ctx->ws_allocs.clear();
        (void)hipGetLastError();
        ctx->maxBe = 0; ctx->maxT = 0; ctx->maxTp = 0;
        ctx->band_T = ctx->band_S = -1;
        return fail(ctx, "said_reserve(%d, %d): workspace allocation failed (%s); the context has no workspace until a smaller said_reserve succeeds",
                    want_be, want_t, why.c_str());
    }
    return 0;
}

// The clones' streams come from ONE pool per device for the whole process (three streams, chosen on first use, never destroyed): a live
// stream is mapped onto one of the device's few hardware queues (four by default), streams on the same queue serialise, and the mapping
// follows creation order — with two other streams alive in the application the pool's second stream landed on the CALLER's queue and a
// three-group loop ran 37 % slower (2.43 vs 1.77 ms per step), while with four others it was fine again.  There is no API to ask which
// queue a stream sits on, so the pool is chosen by measurement: candidates are created one by one and probed with a 0.3 ms spinning wave —
// two streams that finish two such waves in the time of one are on different queues — until three are found that run beside the default
// stream and beside each other; the other candidates are destroyed.  Two models with a stream per clone were enough to exhaust the queues
// (the second model's groups ran 16 % SLOWER than its unsplit batch): clones of different parents share the pool.
constexpr int POOL_STREAMS = 3, POOL_DEVICES = 64, POOL_CANDIDATES = 12;
static std::mutex g_pool_mu;
static hipStream_t g_pool[POOL_DEVICES][POOL_STREAMS];
static bool g_pool_ready[POOL_DEVICES];
static int g_pool_probed[POOL_DEVICES];   // candidates looked at (said_debug_get "pool_probed")

// true when a wave on `b` runs beside one on `a` (a == nullptr: the default stream)
static bool streams_overlap(hipStream_t a, hipStream_t b, hipEvent_t e0, hipEvent_t e1) {
    const long long ticks = 30000;   // 0.3 ms of the 100 MHz wall clock
    if (hipEventRecord(e0, a) != hipSuccess) return false;
    launch_spin(ticks, a);
    launch_spin(ticks, b);
    if (hipEventRecord(e1, b) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipStreamSynchronize(a) != hipSuccess) return false;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return false;
    return ms < 0.48f;               // serialised: >= 0.6 ms
}
static void pool_init(int dev) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int found = 0;
    if (hipDeviceSynchronize() == hipSuccess && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
        launch_spin(1, nullptr);     // first launch of the probe kernel (module load) outside the measurements
        (void)hipDeviceSynchronize();
        hipStream_t rejected[POOL_CANDIDATES];
        int nrej = 0;
        for (int c = 0; c < POOL_CANDIDATES && found < POOL_STREAMS; ++c) {
            hipStream_t s = nullptr;
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) break;
            ++g_pool_probed[dev];
            bool ok = streams_overlap(nullptr, s, e0, e1);
            for (int k = 0; ok && k < found; ++k) ok = streams_overlap(g_pool[dev][k], s, e0, e1);
            if (ok) g_pool[dev][found++] = s;
            else rejected[nrej++] = s;   // kept alive until the end: a destroyed candidate's queue is the next candidate's again
        }
        for (int i = 0; i < nrej; ++i) (void)hipStreamDestroy(rejected[i]);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipGetLastError();
    for (; found < POOL_STREAMS; ++found)   // fewer independent queues than groups (or the probe failed): any stream will do
        if (hipStreamCreateWithFlags(&g_pool[dev][found], hipStreamNonBlocking) != hipSuccess) g_pool[dev][found] = nullptr;
    g_pool_ready[dev] = true;
}
static hipStream_t pool_stream(int dev, int idx) {
    if (dev < 0 || dev >= POOL_DEVICES) return nullptr;
    std::lock_guard<std::mutex> lk(g_pool_mu);
    if (!g_pool_ready[dev]) pool_init(dev);
    return g_pool[dev][idx];
}

int said_clone(said_ctx* parent, said_ctx** out, int max_batch_eff, int max_frames) {
    if (!out) return fail(parent, "said_clone: out is null");
    *out = nullptr;
    if (check_ready(parent)) return -1;
    if (max_batch_eff < 1 || max_frames < 1) return fail(parent, "said_clone: bad sizes");
    DeviceRestore restore_device;
    {
        said_ctx* ctx = parent;
        HIPCHK(hipSetDevice(parent->device));
    }
    // a new context with the parent's model and switches: every packed weight / table pointer is SHARED (read-only on the device); everything a run writes is its own
    said_ctx* c = new said_ctx();
    static_cast<ModelWeights&>(*c) = *parent;
    static_cast<Switches&>(*c) = *parent;
    c->device = parent->device;
    c->is_clone = true;
    auto bail = [&](const char* what) { parent->err = std::string("said_clone: ") + what + (c->err.empty() ? "" : ": " + c->err); said_destroy(c); return -1; };
    c->own_stream = pool_stream(parent->device, parent->n_clones++ % POOL_STREAMS);
    if (!c->own_stream) return bail("hipStreamCreateWithFlags failed");
    int rc = alloc_cells(c);
    rc |= alloc_workspace(c, max_batch_eff, max_frames);
    if (rc) return bail("workspace allocation failed");
    *out = c;
    return 0;
}

void* said_stream(const said_ctx* ctx) { return ctx ? (void*)ctx->own_stream : nullptr; }

int said_capacity(const said_ctx* ctx, int* max_batch_eff, int* max_frames) {
    if (!ctx) return -1;
    if (max_batch_eff) *max_batch_eff = ctx->maxBe;
    if (max_frames) *max_frames = ctx->maxT;
    return 0;
}

// --------------------------------------------------------------------------------------------
// SAID.forward
// --------------------------------------------------------------------------------------------
int said_unet_forward(said_ctx* ctx, const float* sample_dev, const int64_t* timesteps_host, const float* context_dev,
                      int Be, int T, int S, float* out_dev, void* stream) {
    if (check_ready(ctx)) return -1;
    ctx->cur_concurrent = false;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    if (Be < 1 || Be > ctx->maxBe) return fail(ctx, "batch %d exceeds the context's max_batch_eff %d", Be, ctx->maxBe);
    if (T < 1 || T > ctx->maxT || S < 1 || S > ctx->maxT) return fail(ctx, "frames %d / context length %d exceed max_frames %d", T, S, ctx->maxT);
    if (set_band(ctx, T, S, s)) return -1;
    UGeo g = make_geo(ctx, Be, 0, T, S);
    g.emb_b_stride = 1;
    std::vector<long long> ts(timesteps_host, timesteps_host + Be);
    HIPCHK(hipMemcpyAsync(ctx->ts_dev, ts.data(), Be * sizeof(long long), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));  // ts is a stack-local staging buffer
    ctx->dbg_count = 0;
    HIPCHK(hipMemsetAsync(ctx->status_dev, 0, 2 * sizeof(int), s));
    run_time_embed(ctx, Be, s);
    launch_tm_to_cm(context_dev, ctx->CTX, Be, S, ctx->ctx_dim, g.Sp, (long long)ctx->ctx_dim * g.Sp, s);
    run_kv(ctx, 0, Be, S, g.Sp, s);
    launch_tm_to_cm(sample_dev, ctx->x_cm, Be, T, ctx->cin, g.Tp, (long long)ctx->cin * g.Tp, s);
    run_unet(ctx, g, s);
    if (ctx->dbg_stop < 0) launch_nonfinite_check(ctx->eps_cm, (long long)ctx->cin * g.Tp, g.Tp, Be, T, ctx->cin, ctx->status_dev, s);
    launch_cm_to_tm(ctx->eps_cm, out_dev, Be, T, ctx->cin, g.Tp, (long long)ctx->cin * g.Tp, s);
    LAUNCHCHK();
    HIPCHK(hipGetLastError());
    return 0;
}

// --------------------------------------------------------------------------------------------
// SAID.inference loop
// --------------------------------------------------------------------------------------------
// What the captured step graph depends on (everything else it reads from device memory at replay time).
// Denoise steps captured per graph.  A graph launch costs its host-side enqueue (~1 us per node) before the GPU sees its first kernel: behind a running graph that is hidden,
// for the FIRST graph of a loop it is not — 1200-1400 nodes (50 steps) in front of a 50- or 100-step loop cost configs[2] / configs[4] 2-6 % where the long loops gain 0.4-0.5 %
// from five times fewer graph boundaries (profiles/r06l_steps_per_graph.txt).  So: spg_limit (50) from 400 steps on, at most 10 below.
static int steps_per_graph(const said_ctx* ctx, int N) {
    const int lim = N >= 400 ? ctx->spg_limit : std::min(ctx->spg_limit, 10);
    return std::max(1, std::min(lim, N));
}
// Solver family of a coefficient table (column SAID_COEF_SOLVER): 0 = DDIM rows only, 1 = DDPM / DPM-Solver++ rows only, -1 = malformed
// (the message in *why).  The family picks the kernels the step graph holds; the row's own code picks the update inside them.
static int table_solver(const said_loop_params* p, std::string* why) {
    char buf[160];
    int fam = -1;
    for (int k = 0; k < p->num_steps; ++k) {
        const float v = p->coef_host[(size_t)k * 8 + 7];
        const int code = (v >= 0.f && v <= 3.f) ? (int)v : -1;
        if (code < 0 || v != (float)code) { snprintf(buf, sizeof buf, "coefficient row %d: unknown solver code %g in column 7", k, (double)v); *why = buf; return -1; }
        const int f = code != 0;
        if (fam >= 0 && f != fam) { snprintf(buf, sizeof buf, "coefficient row %d: DDIM and DDPM / DPM-Solver++ rows mixed in one table", k); *why = buf; return -1; }
        fam = f;
        if (code == 3 && k == 0) { *why = "coefficient row 0: a loop's first step cannot be second order (no previous x0)"; return -1; }
        if (code >= 2 && p->use_step_noise) { snprintf(buf, sizeof buf, "coefficient row %d: DPM-Solver++ rows draw no step noise (use_step_noise must be 0)", k); *why = buf; return -1; }
    }
    return fam < 0 ? 0 : fam;
}
static std::vector<long long> loop_graph_key(const said_ctx* ctx, const said_loop_params* p, const float* noise_cm, int solver) {
    const bool cfg = p->guidance_scale > 1.0f;
    float gs = p->guidance_scale, gr = (cfg && p->guidance_rescale > 0.f) ? p->guidance_rescale : 0.f, ls = p->latent_scale;
    int gsi, gri, lsi;
    memcpy(&gsi, &gs, 4); memcpy(&gri, &gr, 4); memcpy(&lsi, &ls, 4);
    const int spg = p->num_steps > 0 ? steps_per_graph(ctx, p->num_steps) : 0;
    const int rem = spg > 0 ? p->num_steps % spg : 0;
    return {spg, rem, p->batch, p->frames, cfg, gsi, gri, lsi, p->prediction_type, p->use_mask, p->use_step_noise, ctx->bf16_mode ? 1 : (strict_f32(ctx) ? 2 : 0), p->noise_batch_offset, p->concurrent != 0,
            (long long)(uintptr_t)(p->save_intermediate ? p->intermediates_dev : nullptr), (long long)(uintptr_t)(p->use_step_noise == 1 ? noise_cm : nullptr), solver};
}

// ---- the loop's phases, in the order loop_impl runs them ----
// Argument checks; *solver <- the coefficient table's solver family.
static int loop_check(said_ctx* ctx, const said_loop_params* p, int* solver) {
    const int B = p->batch, T = p->frames, N = p->num_steps;
    const int Be = p->guidance_scale > 1.0f ? 2 * B : B;
    if (B < 1 || Be > ctx->maxBe) return fail(ctx, "effective batch %d exceeds the context's max_batch_eff %d", Be, ctx->maxBe);
    if (T < 1 || T > ctx->maxT) return fail(ctx, "frames %d exceed max_frames %d", T, ctx->maxT);
    if (N < 0 || N > ctx->maxNp) return fail(ctx, "num_steps %d exceeds %d", N, ctx->maxNp);
    if (p->prediction_type < 0 || p->prediction_type > 2) return fail(ctx, "bad prediction_type %d", p->prediction_type);
    if (!p->latents_dev || !p->context_dev) return fail(ctx, "latents_dev/context_dev must not be null");
    if (p->use_mask && !(p->init_latents_dev && p->edit_noise_dev && p->mask_dev)) return fail(ctx, "use_mask needs init_latents_dev, edit_noise_dev and mask_dev");
    if (p->use_step_noise == 1 && !p->step_noise_dev) return fail(ctx, "use_step_noise = 1 needs step_noise_dev");
    if (p->use_step_noise < 0 || p->use_step_noise > 2) return fail(ctx, "bad use_step_noise %d", p->use_step_noise);
    if (p->save_intermediate && !p->intermediates_dev) return fail(ctx, "save_intermediate needs intermediates_dev");
    if (N > 0 && !p->coef_host) return fail(ctx, "coef_host must not be null");
    std::string why;
    *solver = table_solver(p, &why);
    if (*solver < 0) return fail(ctx, "said_denoise_loop: %s", why.c_str());
    return 0;
}
// The per-clip, step-invariant work: everything the step graph reads from device memory at replay time.
static int loop_stage(said_ctx* ctx, const said_loop_params* p, const UGeo& g, hipStream_t s) {
    const int B = p->batch, T = p->frames, N = p->num_steps, C = ctx->cin;
    const bool cfg = p->guidance_scale > 1.0f;
    const long long xs = (long long)C * g.Tp;
    if (N > 0) {
        HIPCHK(hipMemcpyAsync(ctx->ts_dev, p->timesteps_host, N * sizeof(long long), hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(ctx->coef_dev, p->coef_host, (size_t)N * 8 * sizeof(float), hipMemcpyHostToDevice, s));
        run_time_embed(ctx, N, s);
    }
    const long long cs = (long long)ctx->ctx_dim * g.Sp;
    const bool uncond_const = g.Bc > 0;   // the unconditional half's cross-attention is the constant c2[blk]: its context and K/V are never read
    if (cfg) {  // uncond FIRST (diffusion.py:397-400): null_cond_emb repeated over (B, S)
        if (!uncond_const) launch_fill_cm_vec(ctx->null_cond, ctx->CTX, B, T, ctx->ctx_dim, g.Sp, cs, s);
        launch_tm_to_cm(p->context_dev, ctx->CTX + (long long)B * cs, B, T, ctx->ctx_dim, g.Sp, cs, s);
    } else {
        launch_tm_to_cm(p->context_dev, ctx->CTX, B, T, ctx->ctx_dim, g.Sp, cs, s);
    }
    TRACE("loop: ctx done");
    if (uncond_const) run_kv(ctx, B, B, T, g.Sp, s); else run_kv(ctx, 0, g.Be, T, g.Sp, s);
    TRACE("loop: kv launched");
    launch_tm_to_cm(p->latents_dev, ctx->x_cm, B, T, C, g.Tp, xs, s);
    if (p->use_mask) {
        launch_tm_to_cm(p->init_latents_dev, ctx->init_cm, B, T, C, g.Tp, xs, s);
        launch_tm_to_cm(p->edit_noise_dev, ctx->enoise_cm, B, T, C, g.Tp, xs, s);
        launch_tm_to_cm(p->mask_dev, ctx->mask_cm, B, T, C, g.Tp, xs, s);
    }
    if (p->use_step_noise == 2) {   // Philox key of this call's eta noise (the graph reads it from device memory)
        ctx->seed_host[0] = (unsigned)(p->noise_seed & 0xffffffffu); ctx->seed_host[1] = (unsigned)(p->noise_seed >> 32);
        HIPCHK(hipMemcpyAsync(ctx->seed_dev, ctx->seed_host, 2 * sizeof(unsigned), hipMemcpyHostToDevice, s));
    }
    if (p->use_step_noise == 1 && N > 0) {
        const size_t need = (size_t)N * B * xs;
        if (need > ctx->noise_cm_elems) {
            HIPCHK(hipStreamSynchronize(s));
            if (drealloc(ctx, &ctx->noise_cm, need)) return -1;
            ctx->noise_cm_elems = need;
        }
        launch_tm_to_cm(p->step_noise_dev, ctx->noise_cm, N * B, T, C, g.Tp, xs, s);
    }
    HIPCHK(hipMemsetAsync(ctx->step_dev, 0xFF, sizeof(int), s));  // step = -1
    HIPCHK(hipMemsetAsync(ctx->status_dev, 0, 2 * sizeof(int), s));   // numeric status of THIS loop (the eager warm-up step sees step 0's own data)
    return 0;
}
// The argument blocks of the step's last kernel: the update's operands once, then what each route adds.  `fused`: the out conv runs inside that kernel.
struct LoopArgs {
    SchedArgs sa{};
    OutSchedArgs osa{};
    bool fused = false;
};
static void loop_args(const said_ctx* ctx, const said_loop_params* p, const UGeo& g, int solver, LoopArgs* la) {
    const bool cfg = p->guidance_scale > 1.0f;
    StepUpdateArgs u{};
    u.coef = ctx->coef_dev; u.step_ptr = ctx->step_dev;
    u.x = ctx->x_cm; u.x_bstride = (long long)ctx->cin * g.Tp; u.pitch = g.Tp;
    u.B = p->batch; u.T = p->frames; u.C = ctx->cin; u.cfg = cfg ? 1 : 0; u.prediction_type = p->prediction_type;
    u.guidance_scale = p->guidance_scale; u.guidance_rescale = (cfg && p->guidance_rescale > 0.f) ? p->guidance_rescale : 0.f; u.latent_scale = p->latent_scale;
    u.step_noise = p->use_step_noise == 1 ? ctx->noise_cm : nullptr;
    u.noise_seed = p->use_step_noise == 2 ? ctx->seed_dev : nullptr;
    u.noise_elem0 = (unsigned)((long long)p->noise_batch_offset * p->frames * ctx->cin);
    u.init = p->use_mask ? ctx->init_cm : nullptr; u.edit_noise = p->use_mask ? ctx->enoise_cm : nullptr; u.mask = p->use_mask ? ctx->mask_cm : nullptr;
    u.inter = p->save_intermediate ? p->intermediates_dev : nullptr;
    u.status = ctx->status_dev;
    u.x0h = solver ? ctx->x0h_cm : nullptr; u.solver = solver;

    static_cast<StepUpdateArgs&>(la->sa) = u;
    la->sa.eps = ctx->eps_cm; la->sa.eps_bstride = u.x_bstride; la->sa.rescale_part = ctx->rescale_part; la->sa.rescale_nblk = 16;

    static_cast<StepUpdateArgs&>(la->osa) = u;
    OutSchedArgs& o = la->osa;
    o.h = ctx->P.p; o.h_bstride = g.hs; o.gn_part = ctx->P.st; o.gn_part_bstride = g.sts; o.gn_nparts = g.np; o.gn_gamma = ctx->out_g; o.gn_beta = ctx->out_b;
    o.w4 = ctx->conv_out.w4[0]; o.ws = sp_on(ctx, ctx->out_split) ? ctx->conv_out.ws[0] : nullptr; o.bias = ctx->conv_out.bias; o.Cin = MC;
    la->fused = ctx->conv_out.w4[0] && out_sched_supports(o);
}
// Until keep is set, leaving the scope drops the step graphs: a half-built or faulted graph is never cached.  The capture stream is released either way
// (a live stream pins a hardware queue: DESIGN.md 5.1).
struct GraphBuildGuard {
    said_ctx* ctx;
    bool keep = false;
    ~GraphBuildGuard() {
        if (!keep) drop_graphs(ctx);
        release_cap_streams(ctx);
    }
};
// One denoise step: the UNet (its last kernel holds the update when fused), else the unfused scheduler launches behind it.
static void run_step(said_ctx* ctx, const UGeo& g, const LoopArgs& la, hipStream_t s) {
    run_unet(ctx, g, s);
    if (!la.fused) {
        if (la.sa.guidance_rescale > 0.f) launch_rescale_partials(la.sa, ctx->rescale_part, s);
        launch_sched_step(la.sa, s);
        ++ctx->n_sched_step;
    }
}
// Warm-up, then capture of the spg-step graph and of the graph of the rem remaining steps.
static int build_step_graphs(said_ctx* ctx, const said_loop_params* p, const UGeo& g, const LoopArgs& la, hipStream_t s, int spg, int rem, const std::vector<long long>& key) {
    drop_graphs(ctx);
    GraphBuildGuard guard{ctx};
    // Eager warm-up of the exact step sequence first: the first launch of a kernel inside a
    // stream capture hangs on ROCm 7.2 (lazy per-kernel initialisation is not capturable).
    // The step is run on step index 0 and its effect on the latents is undone afterwards.
    TRACE("loop: warmup begin");
    run_step(ctx, g, la, s);
    TRACE("loop: warmup unet launched");
    launch_tm_to_cm(p->latents_dev, ctx->x_cm, p->batch, p->frames, ctx->cin, g.Tp, (long long)ctx->cin * g.Tp, s);
    HIPCHK(hipMemsetAsync(ctx->step_dev, 0xFF, sizeof(int), s));
    HIPCHK(hipStreamSynchronize(s));
    TRACE("loop: warmup synced");
    // A launch helper that refused a shape launched NOTHING (launch_fault / launch_err): a graph captured from the same schedule would be
    // missing that kernel and — cached under this key — replay silently wrong on every later call.  So the faults of the warm-up and of
    // each capture are consumed HERE, on the thread that drove them, in the prepare-only path too, and nothing is cached.
    auto loop_fault = [&]() -> bool { return launch_fault_peek() != nullptr || !ctx->launch_err.empty(); };
    if (loop_fault()) LAUNCHCHK();
    // capture on a private stream: the caller's stream may be the legacy default stream,
    // which cannot be captured; the instantiated graph is then replayed on the caller's stream
    if (ensure_cap_streams(ctx)) return -1;
    hipStream_t cs = ctx->cap_stream;
    auto capture_steps = [&](int nsteps, hipGraph_t* gr, hipGraphExec_t* ge) -> int {
        HIPCHK(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
        for (int rep = 0; rep < nsteps; ++rep) run_step(ctx, g, la, cs);
        TRACE("loop: capture recorded");
        hipError_t e = hipStreamEndCapture(cs, gr);
        if (e != hipSuccess) return fail(ctx, "hipStreamEndCapture: %s", hipGetErrorString(e));
        HIPCHK(hipGraphInstantiate(ge, *gr, nullptr, nullptr, 0));
        return 0;
    };
    if (capture_steps(spg, &ctx->graph, &ctx->gexec)) return -1;
    if (loop_fault()) LAUNCHCHK();
    if (rem > 0 && capture_steps(rem, &ctx->graph_rem, &ctx->gexec_rem)) return -1;
    if (loop_fault()) LAUNCHCHK();
    size_t nn = 0;
    (void)hipGraphGetNodes(ctx->graph, nullptr, &nn);
    ctx->gnodes = (int)nn / spg;
    ctx->gspg = spg;
    ctx->gkey = key;
    guard.keep = true;
    TRACE("loop: graph instantiated");
    return 0;
}

static int loop_impl(said_ctx* ctx, const said_loop_params* p, void* stream, bool prepare_only) {
    if (check_ready(ctx)) return -1;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    ctx->cur_concurrent = p->concurrent != 0;
    ctx->dbg_count = 0;   // (said_debug_stop_after counts launches from the start of the call: the eager warm-up step then runs the first n launches, the captured steps none)
    int solver = 0;
    if (loop_check(ctx, p, &solver)) return -1;
    const int B = p->batch, T = p->frames, N = p->num_steps, C = ctx->cin;
    const bool cfg = p->guidance_scale > 1.0f;
    if (prepare_only) {   // nothing to do when the step graph of this configuration exists
        if (N == 0) return 0;
        const bool grow = p->use_step_noise == 1 && (size_t)N * B * C * (size_t)rup(T, 32) > ctx->noise_cm_elems;
        if (!grow && ctx->gexec && loop_graph_key(ctx, p, ctx->noise_cm, solver) == ctx->gkey) return 0;
    }
    if (set_band(ctx, T, T, s)) return -1;
    UGeo g = make_geo(ctx, cfg ? 2 * B : B, cfg ? B : 0, T, T);
    g.step_ptr = ctx->step_dev;
    g.step_inc = ctx->step_dev;   // the first kernel of the step (conv_in) advances the step counter itself
    if (cfg) g.Bc = B;

    TRACE("loop: begin");
    if (loop_stage(ctx, p, g, s)) return -1;
    LoopArgs la;
    loop_args(ctx, p, g, solver, &la);
    if (la.fused) g.out_sched = &la.osa;

    if (N > 0) {
        // steps per graph: consecutive denoise steps captured back to back in ONE graph (the device-side step counter
        // makes the copies distinct): N / spg launches of the spg-step graph cover the loop, and a second graph holding
        // the N % spg remaining steps finishes it (prime N, e.g. 997 = 99 x 10 + 7)
        const int spg = steps_per_graph(ctx, N);   // measured: ~6 us per graph launch boundary; 10 steps per graph recovered 1.2 % at B=1 (round 1), 50 another 0.4-0.5 % of a long loop (round 6)
        const int rem = N % spg;
        const std::vector<long long> key = loop_graph_key(ctx, p, la.sa.step_noise, solver);
        if ((!ctx->gexec || key != ctx->gkey) && build_step_graphs(ctx, p, g, la, s, spg, rem, key)) return -1;
        if (prepare_only) return 0;
        for (int k = 0; k < N / ctx->gspg; ++k) HIPCHK(hipGraphLaunch(ctx->gexec, s));
        if (rem > 0) HIPCHK(hipGraphLaunch(ctx->gexec_rem, s));
    }
    TRACE("loop: graphs launched");
    launch_finish(ctx->x_cm, (long long)C * g.Tp, g.Tp, B, T, C, p->latent_scale, p->latents_dev, p->result_dev, s, ctx->dbg_stop < 0 ? ctx->status_dev : nullptr);
    LAUNCHCHK();
    HIPCHK(hipGetLastError());
    return 0;
}

int said_denoise_loop(said_ctx* ctx, const said_loop_params* p, void* stream) { return loop_impl(ctx, p, stream, false); }

int said_loop_prepare(said_ctx* ctx, const said_loop_params* p, void* stream) { return loop_impl(ctx, p, stream, true); }

// said_ddim_step / said_solver_step after their own argument checks: the coefficient row's upload and the launch
static int step_flat(said_ctx* ctx, int solver, const float* model_out_dev, const float* uncond_dev, float guidance_scale, const float* sample_dev, const float* coef_host,
                     int prediction_type, float* x0_hist_dev, const float* step_noise_dev, const float* init_latents_dev, const float* edit_noise_dev, const float* mask_dev,
                     float* prev_sample_dev, int64_t n, hipStream_t s) {
    HIPCHK(hipMemcpyAsync(ctx->coef1_dev, coef_host, 8 * sizeof(float), hipMemcpyHostToDevice, s));
    if (n > 0)
        launch_step_flat(solver, model_out_dev, uncond_dev, guidance_scale, sample_dev, ctx->coef1_dev, prediction_type, x0_hist_dev, step_noise_dev, init_latents_dev,
                         edit_noise_dev, mask_dev, prev_sample_dev, n, s);
    HIPCHK(hipGetLastError());
    return 0;
}

int said_ddim_step(said_ctx* ctx, const float* eps_dev, const float* eps_uncond_dev, float guidance_scale,
                   const float* sample_dev, const float* coef_host, int prediction_type, const float* step_noise_dev,
                   const float* init_latents_dev, const float* edit_noise_dev, const float* mask_dev, float* prev_sample_dev,
                   int64_t n, void* stream) {
    if (!ctx) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    if (prediction_type < 0 || prediction_type > 2) return fail(ctx, "bad prediction_type %d", prediction_type);
    if (mask_dev && !(init_latents_dev && edit_noise_dev)) return fail(ctx, "mask needs init_latents_dev and edit_noise_dev");
    return step_flat(ctx, 0, eps_dev, eps_uncond_dev, guidance_scale, sample_dev, coef_host, prediction_type, nullptr, step_noise_dev, init_latents_dev, edit_noise_dev, mask_dev,
                     prev_sample_dev, n, (hipStream_t)stream);
}

int said_solver_step(said_ctx* ctx, const float* model_out_dev, const float* uncond_dev, float guidance_scale, const float* sample_dev,
                     const float* coef_host, int prediction_type, float* x0_hist_dev, const float* step_noise_dev, const float* init_latents_dev,
                     const float* edit_noise_dev, const float* mask_dev, float* prev_sample_dev, int64_t n, void* stream) {
    if (!ctx) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    if (prediction_type < 0 || prediction_type > 2) return fail(ctx, "bad prediction_type %d", prediction_type);
    if (!coef_host) return fail(ctx, "said_solver_step: coef_host must not be null");
    if (mask_dev && !(init_latents_dev && edit_noise_dev)) return fail(ctx, "mask needs init_latents_dev and edit_noise_dev");
    const float v = coef_host[7];
    const int code = (v >= 1.f && v <= 3.f) ? (int)v : -1;
    if (code < 0 || v != (float)code)
        return fail(ctx, "said_solver_step: solver code %g in column 7 is not DDPM (1) or DPM-Solver++ (2, 3); DDIM rows go to said_ddim_step", (double)v);
    if (code >= 2 && step_noise_dev) return fail(ctx, "said_solver_step: DPM-Solver++ rows draw no step noise");
    if (code >= 2 && !x0_hist_dev) return fail(ctx, "said_solver_step: DPM-Solver++ rows need x0_hist_dev");
    return step_flat(ctx, 1, model_out_dev, uncond_dev, guidance_scale, sample_dev, coef_host, prediction_type, x0_hist_dev, step_noise_dev, init_latents_dev, edit_noise_dev,
                     mask_dev, prev_sample_dev, n, (hipStream_t)stream);
}

int said_axpby(said_ctx* ctx, const float* a_host, const float* x_dev, const float* c_host, const float* y_dev, float* out_dev,
               int batch, int64_t n_per_batch, void* stream) {
    if (!ctx) return -1;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    if (batch < 1 || batch > ctx->maxNp) return fail(ctx, "said_axpby: batch %d out of range", batch);
    // coefficient staging shares the (otherwise idle here) E0 table: 2 * batch floats
    std::vector<float> ac(2 * (size_t)batch, 0.f);
    for (int b = 0; b < batch; ++b) { ac[b] = a_host[b]; ac[batch + b] = (y_dev && c_host) ? c_host[b] : 0.f; }
    HIPCHK(hipMemcpyAsync(ctx->axpby_coef, ac.data(), ac.size() * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    if (n_per_batch > 0) launch_axpby(ctx->axpby_coef, x_dev, ctx->axpby_coef + batch, y_dev, out_dev, batch, n_per_batch, s);
    HIPCHK(hipGetLastError());
    return 0;
}

int said_debug_clocks(said_ctx* ctx, int enable, long long* out_host /* [64][8][8] or null */) {
    if (!ctx) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    ctx->clk_on = enable != 0;
    if (out_host) {
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(out_host, ctx->clk_dev, 64 * 128 * sizeof(long long), hipMemcpyDeviceToHost));
    }
    return 0;
}

// The said_debug_option names whose value is a tri-state: < 0 the default (-1), 0 off, anything else on (1).
struct TriState { const char* name; int Switches::*field; };
static const TriState kTriStates[] = {
    {"tm_acts", &Switches::tm_acts},           {"gemm_presplit", &Switches::gemm_presplit}, {"gemm_split", &Switches::gemm_split},
    {"attn_split", &Switches::attn_split},     {"attn_presplit", &Switches::attn_presplit}, {"out_split", &Switches::out_split},
    {"ugemm_split", &Switches::ugemm_split},   {"chain_coef", &Switches::chain_coef},       {"tgemm_direct", &Switches::tgemm_direct},
    {"st_chain", &Switches::st_chain},         {"attn_2q", &Switches::attn_2q},             {"st_chain_bf16", &Switches::st_chain_bf16},
};

int said_debug_option(said_ctx* ctx, const char* name, long long value) {
    if (!ctx || !name) return -1;
    const std::string k = name;
    if (k == "unet_tgemm_min_tokens") {
        ctx->unet_tgemm_min_tokens = value < 0 ? 3000 : value;
        ctx->unet_fgemm_min_tokens = value < 0 ? 10000 : value;
    } else if (k == "audio_chunk") {
        if (value < 1) return fail(ctx, "audio_chunk must be >= 1");
        ctx->audio_chunk = (int)value;
    } else if (k == "audio_train_sites") {
        ctx->audio_train_sites = value < 0 ? -1 : (int)(value & 63);
    } else if (k == "audio_stop_after") {
        ctx->audio_stop_after = value < 0 ? -1 : (int)std::min<long long>(value, 1 << 20);
    } else if (k == "steps_per_graph") {
        if (value < 1) return fail(ctx, "steps_per_graph must be >= 1");
        ctx->spg_limit = (int)value;
    } else if (k == "out_tm") {
        ctx->out_tm = (int)value;
    } else if (k == "xgemm_clk") {   // shader-clock stamps of the token-major-activation GEMMs (-DSAID_CLK_STAMPS builds); read with said_debug_clocks
        ctx->xclk_on = value != 0;
    } else if (k == "kconv") {
        ctx->kconv = value < 0 ? -1 : (value == 2 ? 2 : (value != 0));
    } else if (k == "st_chain_slices") {
        ctx->st_chain_slices = value < 0 ? -1 : ((value == 3 || value == 2) ? (int)value : 1);   // 2: two slices wherever a sliced launch is possible (<= 128 tiles)
    } else {
        int Switches::*tri = nullptr;
        for (const TriState& t : kTriStates) if (k == t.name) tri = t.field;
        if (!tri) return fail(ctx, "said_debug_option: unknown option %s", name);
        ctx->*tri = value < 0 ? -1 : (value != 0);
    }
    ctx->gkey.clear();   // the captured step graph may hold the other schedule
    return 0;
}

long long said_debug_get(const said_ctx* ctx, const char* name) {
    if (!ctx || !name) return -1;
    const std::string k = name;
    if (k == "n_set_weight") return ctx->n_set_weight;
    if (k == "n_audio_clips") return (int)ctx->n_audio_clips;
    if (k == "unet_tgemm_min_tokens") return ctx->bf16_mode ? ctx->unet_tgemm_min_tokens : ctx->unet_fgemm_min_tokens;
    if (k == "audio_chunk") return ctx->audio_chunk;
    if (k == "audio_stop_after") return ctx->audio_stop_after;
    if (k == "audio_train_sites") return ctx->audio_train_sites;
    if (k == "n_tgemm_128") return ctx->n_tgemm[TG_128];
    if (k == "n_tgemm_128sb") return ctx->n_tgemm[TG_128SB];
    if (k == "n_tgemm_128x64") return ctx->n_tgemm[TG_128X64];
    if (k == "n_tgemm_256") return ctx->n_tgemm[TG_256];
    if (k == "n_tgemm_256x192") return ctx->n_tgemm[TG_256X192];
    if (k == "n_tgemm_256d") return ctx->n_tgemm[TG_256D];
    if (k == "n_audio_attn_ks8") return ctx->n_audio_attn[0];
    if (k == "n_audio_attn_tm") return ctx->n_audio_attn[1];
    if (k == "n_audio_attn_f32_ks8") return ctx->n_audio_attn_f32[0];
    if (k == "n_audio_attn_f32_ks4") return ctx->n_audio_attn_f32[1];
    if (k == "n_audio_attn_f32_ks1") return ctx->n_audio_attn_f32[2];
    if (k == "steps_per_graph") return ctx->spg_limit;
    if (k == "tm_acts") return ctx->tm_acts;
    if (k == "gemm_split") return (!ctx->bf16_mode && sp_on(ctx, ctx->gemm_split)) ? 1 : 0;
    if (k == "ugemm_split") return (!ctx->bf16_mode && sp_on(ctx, ctx->ugemm_split)) ? 1 : 0;
    if (k == "st_chain") return (!ctx->bf16_mode && sp_on(ctx, ctx->st_chain)) ? 1 : 0;
    if (k == "n_stchain") return ctx->n_stchain;
    if (k == "n_out_sched") return ctx->n_out_sched;
    if (k == "n_out_sched_tm") return ctx->n_out_sched_tm;
    if (k == "n_sched_step") return ctx->n_sched_step;
    if (k == "st_chain_bf16") return (ctx->bf16_mode && ctx->st_chain_bf16 != 0) ? 1 : 0;
    if (k == "attn_split") return (!ctx->bf16_mode && sp_on(ctx, ctx->attn_split)) ? 1 : 0;   // 1: fp32-mode attention products run on split-fp16 operands
    if (k == "n_rgemm") return ctx->n_rgemm;
    if (k == "n_xgemm") return ctx->n_xgemm;
    if (k == "pool_probed") return (ctx->device >= 0 && ctx->device < POOL_DEVICES) ? g_pool_probed[ctx->device] : -1;
    return -1;
}

int said_philox_normal(said_ctx* ctx, uint64_t seed, int step0, int nsteps, int64_t n_per_step, float* out_dev, void* stream) {
    if (!ctx) return -1;
    if (nsteps < 0 || n_per_step < 0 || n_per_step > 0xffffffffLL || !out_dev) return fail(ctx, "said_philox_normal: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    ctx->seed_host[0] = (unsigned)(seed & 0xffffffffu); ctx->seed_host[1] = (unsigned)(seed >> 32);
    HIPCHK(hipMemcpyAsync(ctx->seed_dev, ctx->seed_host, 2 * sizeof(unsigned), hipMemcpyHostToDevice, s));
    launch_philox_normal(ctx->seed_dev, step0, nsteps, n_per_step, out_dev, s);
    HIPCHK(hipGetLastError());
    return 0;
}

int said_debug_stop_after(said_ctx* ctx, int n) {
    if (!ctx) return -1;
    ctx->dbg_stop = n;
    ctx->dbg_count = 0;
    ctx->gkey.clear();   // a cached step graph holds the other launch count
    return 0;
}

int said_debug_read(said_ctx* ctx, const char* name, float* out_host, int64_t n) {
    if (!ctx) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    const std::map<std::string, const float*> m = {
        {"H0", ctx->H0.p}, {"H1", ctx->H1.p}, {"P", ctx->P.p}, {"Q", ctx->Q.p}, {"M", ctx->M.p},
        {"stH0", ctx->H0.st}, {"stH1", ctx->H1.st}, {"stP", ctx->P.st}, {"stQ", ctx->Q.st}, {"stM", ctx->M.st},
        {"X1", ctx->X1}, {"X2", ctx->X2}, {"X3", ctx->X3}, {"O", ctx->O}, {"QK", ctx->QK}, {"VT", ctx->VT}, {"F", ctx->F},
        {"KV", ctx->KV}, {"CTX", ctx->CTX}, {"EO", ctx->EO}, {"E0", ctx->E0}, {"E1", ctx->E1}, {"E2", ctx->E2},
        {"x", ctx->x_cm}, {"eps", ctx->eps_cm}, {"aH", ctx->aH}, {"aT", ctx->aT}, {"aX", ctx->aX}, {"aPOS", ctx->aPOS},
        {"aQK", ctx->aQK}, {"aO", ctx->aO}, {"aF", ctx->aF}, {"abufA", ctx->abufA}, {"abufB", ctx->abufB}};
    auto it = m.find(name);
    if (it == m.end() || !it->second) return fail(ctx, "said_debug_read: unknown or unallocated buffer %s", name);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out_host, it->second, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

// ---- workspace inspection (tests / race hunting): every (max_batch_eff, max_frames)-sized buffer by index --------------------------------
static const char* ws_name(const said_ctx* c, const void* p) {
    const std::pair<const void*, const char*> t[] = {
        {c->x_cm, "x"}, {c->eps_cm, "eps"}, {c->H0.p, "H0"}, {c->H1.p, "H1"}, {c->P.p, "P"}, {c->Q.p, "Q"}, {c->M.p, "M"},
        {c->H0.st, "stH0"}, {c->H1.st, "stH1"}, {c->P.st, "stP"}, {c->Q.st, "stQ"}, {c->M.st, "stM"},
        {c->X1, "X1"}, {c->X2, "X2"}, {c->X3, "X3"}, {c->O, "O"}, {c->QK, "QK"}, {c->VT, "VT"}, {c->F, "F"}, {c->KV, "KV"}, {c->KVT, "KVT"}, {c->chain_part, "chain_part"}, {c->CTX, "CTX"},
        {c->E0, "E0"}, {c->E1, "E1"}, {c->E2, "E2"}, {c->EO, "EO"}, {c->ts_dev, "ts"}, {c->coef_dev, "coef"}, {c->axpby_coef, "axpby_coef"},
        {c->band_lo, "band_lo"}, {c->band_hi, "band_hi"}, {c->init_cm, "init_cm"}, {c->enoise_cm, "enoise_cm"}, {c->mask_cm, "mask_cm"},
        {c->rescale_part, "rescale_part"}, {c->uPA, "uPA"}, {c->uPB, "uPB"}, {c->uPL, "uPL"}, {c->uPH, "uPH"}, {c->uPX, "uPX"}, {c->gn_coef, "gn_coef"},
        {c->H0.t, "tH0"}, {c->H1.t, "tH1"}, {c->P.t, "tP"}, {c->Q.t, "tQ"}, {c->M.t, "tM"}, {c->tX1, "tX1"}, {c->tX2, "tX2"}, {c->tO, "tO"}, {c->tF, "tF"}, {c->x0h_cm, "x0h"}};
    for (const auto& e : t) if (e.first == p) return e.second;
    return "?";
}
int said_debug_ws_count(const said_ctx* ctx) { return ctx ? (int)ctx->ws_allocs.size() : -1; }
int said_debug_ws_info(said_ctx* ctx, int idx, void** ptr_out, long long* bytes_out, const char** name_out) {
    if (!ctx || idx < 0 || idx >= (int)ctx->ws_allocs.size()) return -1;
    void* p = ctx->ws_allocs[idx];
    if (ptr_out) *ptr_out = p;
    if (bytes_out) { auto it = ctx->alloc_bytes.find(p); *bytes_out = it == ctx->alloc_bytes.end() ? 0 : (long long)it->second; }
    if (name_out) *name_out = ws_name(ctx, p);
    return 0;
}
int said_debug_ws_fill(said_ctx* ctx, int byte_value) {
    if (!ctx) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());
    for (void* p : ctx->ws_allocs) {
        auto it = ctx->alloc_bytes.find(p);
        if (it != ctx->alloc_bytes.end()) HIPCHK(hipMemset(p, byte_value, it->second));
    }
    HIPCHK(hipDeviceSynchronize());
    ctx->band_T = ctx->band_S = -1;   // the band tables were part of it
    drop_graphs(ctx);
    return 0;
}
int said_debug_ws_copy(said_ctx* ctx, int idx, void* dst_dev, long long bytes, void* stream) {
    if (!ctx || idx < 0 || idx >= (int)ctx->ws_allocs.size() || !dst_dev) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(dst_dev, ctx->ws_allocs[idx], (size_t)bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}
// the audio encoder's lazily sized buffers by name (they are not part of the workspace list): bf16 mode's token-major set, fp32 mode's channel-major set and the
// attention operands both share
struct AudioBuf { const char* name; void* p; };
static std::vector<AudioBuf> audio_bufs(const said_ctx* ctx) {
    return {{"bA0", ctx->bA0}, {"bA1", ctx->bA1}, {"bX", ctx->bX}, {"bXg", ctx->bXg}, {"bH", ctx->bH}, {"bHb", ctx->bHb}, {"bT", ctx->bT}, {"bF", ctx->bF},
            {"bO", ctx->bO}, {"bPosT", ctx->bPosT}, {"aQK", ctx->aQK}, {"aVT", ctx->aVT}, {"aO", ctx->aO},
            {"abufA", ctx->abufA}, {"abufB", ctx->abufB}, {"aX", ctx->aX}, {"aH", ctx->aH}, {"aT", ctx->aT}, {"aF", ctx->aF}, {"aPOS", ctx->aPOS}};
}
int said_debug_audio_copy(said_ctx* ctx, const char* name, void* dst_dev, long long bytes, void* stream) {
    if (!ctx) return -1;
    if (!name || !dst_dev || bytes < 0) return fail(ctx, "said_debug_audio_copy: bad arguments");
    const void* p = nullptr;
    bool known = false;
    for (const AudioBuf& e : audio_bufs(ctx)) if (!strcmp(e.name, name)) { known = true; p = e.p; }
    if (!known) return fail(ctx, "said_debug_audio_copy: unknown buffer %s", name);
    auto it = p ? ctx->alloc_bytes.find(const_cast<void*>(p)) : ctx->alloc_bytes.end();
    if (it == ctx->alloc_bytes.end()) return fail(ctx, "said_debug_audio_copy: buffer %s is not allocated", name);
    if ((size_t)bytes > it->second) return fail(ctx, "said_debug_audio_copy: %lld bytes asked of %s, %zu allocated", bytes, name, it->second);
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(dst_dev, p, (size_t)bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}
int said_debug_audio_fill(said_ctx* ctx, int byte_value) {
    if (!ctx) return -1;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());
    for (const AudioBuf& e : audio_bufs(ctx)) {
        auto it = e.p ? ctx->alloc_bytes.find(e.p) : ctx->alloc_bytes.end();
        if (it != ctx->alloc_bytes.end()) HIPCHK(hipMemset(e.p, byte_value, it->second));
    }
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

int said_profile_unet(said_ctx* ctx, int Be, int T, int cfg_clips, int reps, int max_stages, float* us_out, double* bytes_out, double* flops_out,
                      int* kind_out, int* epi_out, int* nb_out, int* ks_out, int* n_stages_out, void* stream) {
    if (check_ready(ctx)) return -1;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    if (Be < 1 || Be > ctx->maxBe || T < 1 || T > ctx->maxT) return fail(ctx, "said_profile_unet: shape out of range");
    if (set_band(ctx, T, T, s)) return -1;
    if (cfg_clips < 0 || (cfg_clips > 0 && Be != 2 * cfg_clips)) return fail(ctx, "said_profile_unet: cfg_clips must be 0 or batch_eff / 2");
    UGeo g = make_geo(ctx, Be, cfg_clips, T, T);
    g.emb_b_stride = 0;
    if (cfg_clips > 0) g.Bc = cfg_clips;   // the schedule the guided loop runs
    run_unet(ctx, g, s);  // eager warm-up: kernels must not see their first launch inside a capture
    HIPCHK(hipStreamSynchronize(s));
    if (ensure_cap_streams(ctx)) return -1;
    // pass 0: log the schedule without launching anything
    ctx->stage_log.clear();
    ctx->log_on = true; ctx->dbg_only = -1; ctx->dbg_stop = 0; ctx->dbg_count = 0;
    run_unet(ctx, g, ctx->cap_stream);
    ctx->log_on = false; ctx->dbg_stop = -1;
    const int n = (int)ctx->stage_log.size();
    if (n_stages_out) *n_stages_out = n;
    if (n > max_stages) return fail(ctx, "said_profile_unet: %d stages > max_stages %d", n, max_stages);
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    for (int k = 0; k < n; ++k) {
        // `reps` back-to-back launches of stage k captured in one graph, timed with HIP events on `s`
        hipGraph_t gr = nullptr;
        hipGraphExec_t ge = nullptr;
        ctx->dbg_only = k;
        HIPCHK(hipStreamBeginCapture(ctx->cap_stream, hipStreamCaptureModeThreadLocal));
        for (int r = 0; r < reps; ++r) { ctx->dbg_count = 0; run_unet(ctx, g, ctx->cap_stream); }
        hipError_t e = hipStreamEndCapture(ctx->cap_stream, &gr);
        ctx->dbg_only = -1;
        if (e != hipSuccess) return fail(ctx, "profile capture: %s", hipGetErrorString(e));
        HIPCHK(hipGraphInstantiate(&ge, gr, nullptr, nullptr, 0));
        HIPCHK(hipGraphLaunch(ge, s));  // warm-up
        HIPCHK(hipEventRecord(e0, s));
        HIPCHK(hipGraphLaunch(ge, s));
        HIPCHK(hipEventRecord(e1, s));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        const auto& si = ctx->stage_log[k];
        us_out[k] = ms * 1000.f / reps;
        bytes_out[k] = si.bytes; flops_out[k] = si.flops; kind_out[k] = si.kind; epi_out[k] = si.epi; nb_out[k] = si.NB; ks_out[k] = si.KS;
        (void)hipGraphExecDestroy(ge);
        (void)hipGraphDestroy(gr);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    release_cap_streams(ctx);   // a live stream pins a hardware queue (the clip groups need them): DESIGN.md 5.1
    return 0;
}

int said_graph_num_nodes(const said_ctx* ctx) { return ctx ? ctx->gnodes : 0; }

int said_loop_progress(said_ctx* ctx, int* steps_done) {
    if (!ctx || !steps_done) return -1;
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t ps = nullptr;   // (created per call: a live stream holds one of the device's few hardware queues — DESIGN.md 5.1)
    HIPCHK(hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
    int v = -1;
    hipError_t e = hipMemcpyAsync(&v, ctx->step_dev, sizeof(int), hipMemcpyDeviceToHost, ps);
    if (e == hipSuccess) e = hipStreamSynchronize(ps);
    (void)hipStreamDestroy(ps);
    if (e != hipSuccess) return -2;   // (no fail(): this is called from a polling thread while the loop's thread may be writing ctx->err — ADVICE r4)
    *steps_done = v + 1;        // the counter is -1 before the first step and k - 1 once step k - 1 has STARTED; its kernels complete in order
    return 0;
}

int said_loop_progress_reset(said_ctx* ctx) {
    if (!ctx) return -1;
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    const int m1 = -1;
    HIPCHK(hipMemcpy(ctx->step_dev, &m1, sizeof(int), hipMemcpyHostToDevice));   // synchronous: a poller started after this call never sees the previous loop's count
    return 0;
}

int said_set_precision(said_ctx* ctx, int mode) {
    if (!ctx) return -1;
    if (mode != SAID_PREC_FP32 && mode != SAID_PREC_BF16 && mode != SAID_PREC_FP32_STRICT) return fail(ctx, "said_set_precision: unknown mode %d", mode);
    if (mode != ctx->prec_mode) {
        ctx->prec_mode = mode;
        ctx->bf16_mode = mode == SAID_PREC_BF16;
        ctx->gkey.clear();   // the captured step graph holds the other kernels
    }
    return 0;
}
int said_get_precision(const said_ctx* ctx) { return ctx ? ctx->prec_mode : 0; }
int said_effective_precision(const said_ctx* ctx) { return !ctx ? 0 : (ctx->bf16_mode ? SAID_PREC_BF16 : (strict_f32(ctx) ? SAID_PREC_FP32_STRICT : SAID_PREC_FP32)); }
const char* said_precision_note(const said_ctx* ctx) { return ctx ? ctx->split_note.c_str() : ""; }

int said_numeric_status(said_ctx* ctx, void* stream, int* first_bad_step, int* result_nonfinite) {
    if (!ctx) return -1;
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    int v[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(v, ctx->status_dev, sizeof v, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    if (first_bad_step) *first_bad_step = v[0] - 1;
    if (result_nonfinite) *result_nonfinite = v[1];
    return 0;
}

double said_unet_algorithmic_bytes(int Be, int T, int bytes_per_elem) {
    // W + Be*T*A, A = 63,232 B/token at fp32
    return 6992672.0 * bytes_per_elem + (double)Be * T * (63232.0 * bytes_per_elem / 4.0);
}
double said_unet_algorithmic_flops(int Be, int T) {
    // banded cross-attention, cross K/V precomputed
    const double lin = 5492736.0 - 1179648.0;
    return 2.0 * Be * (lin * T + 1536.0 * T * (double)T + 4608.0 * T) + 2.0 * Be * 1474560.0;
}

}  // extern "C"
