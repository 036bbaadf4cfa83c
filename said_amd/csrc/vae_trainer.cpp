// vae_trainer.cpp — the BCVAE trainer context (include/said_train.h): the state-dict table, the device copies of the model state and of
// the optimizer, the window sets, and the step: gather, forward, loss, backward, clip, AdamW, EMA, enqueued in that order (vae_train.hip)
// and captured once per batch size into a hipGraph.  The per-step inputs (scalars, std, items, noise) travel in one record copied to the
// device ahead of each step from a ring of pinned host slots, so a step makes no host round trip.
#include "../../include/said_train.h"

#include "engine_internal.h"
#include "train_store.h"
#include "vae_train.h"

using namespace said::vt;

static_assert(OPT_SLOTS_MATCH(SAID_TRAIN_S_), "said_train.h and train_opt.h disagree on the optimizer's slots of the step record");
static_assert(NACC == TS_NACC && A_BAD == TS_A_BAD && SAID_TRAIN_NOT_FINITE == 1, "train_store.h reads the accumulators of vae_train.h");

namespace {

enum Kind { K_PARAM = 0, K_RMEAN, K_RVAR, K_COUNT };
struct TDesc {
    const char* name;
    int kind;
    long long numel;
};

// BCVAE().state_dict() of said/model/vae.py, in its order
const TDesc kTensors[70] = {
#define CONV(p, co, ci, k) {p ".weight", K_PARAM, (long long)(co) * (ci) * (k)}, {p ".bias", K_PARAM, co}
#define LIN(p, o, i) {p ".weight", K_PARAM, (long long)(o) * (i)}, {p ".bias", K_PARAM, o}
#define BN(p, c) {p ".weight", K_PARAM, c}, {p ".bias", K_PARAM, c}, {p ".running_mean", K_RMEAN, c}, {p ".running_var", K_RVAR, c}, \
                 {p ".num_batches_tracked", K_COUNT, 1}
    CONV("encoder.conv_layers.0", 32, 32, 3), BN("encoder.conv_layers.1", 32), CONV("encoder.conv_layers.3", 64, 32, 3),
    BN("encoder.conv_layers.4", 64), CONV("encoder.conv_layers.6", 64, 64, 4), BN("encoder.conv_layers.7", 64),
    CONV("encoder.conv_layers.9", 32, 64, 3), LIN("encoder.fc_layers.0", 256, 1760), BN("encoder.fc_layers.1", 256),
    LIN("encoder.fc_layers.3", 128, 256), BN("encoder.fc_layers.4", 128), LIN("encoder.fc_layers.6", 64, 128), LIN("encoder.fc_mu", 64, 64),
    LIN("encoder.fc_logvar", 64, 64), LIN("decoder.fc_layers.0", 240, 64), BN("decoder.fc_layers.1", 240), LIN("decoder.fc_layers.3", 480, 240),
    CONV("decoder.conv_layers.0", 32, 4, 3), BN("decoder.conv_layers.1", 32), CONV("decoder.conv_layers.3", 32, 32, 3),
    BN("decoder.conv_layers.4", 32), CONV("decoder.conv_layers.6", 32, 32, 3), CONV("decoder.conv_layers.7", 32, 32, 3),
#undef CONV
#undef LIN
#undef BN
};
// the eight BatchNorm1d layers in state-dict order: prefix, channels, positions per channel and sample, LeakyReLU slope after it
struct BNDesc { const char* prefix; int C, L; float slope; };
const BNDesc kBN[8] = {{"encoder.conv_layers.1", 32, 118, 0.2f}, {"encoder.conv_layers.4", 64, 116, 0.2f}, {"encoder.conv_layers.7", 64, 57, 0.2f},
                       {"encoder.fc_layers.1", 256, 1, 0.01f},   {"encoder.fc_layers.4", 128, 1, 0.01f},  {"decoder.fc_layers.1", 240, 1, 0.01f},
                       {"decoder.conv_layers.1", 32, 122, 0.2f}, {"decoder.conv_layers.4", 32, 124, 0.2f}};
constexpr int NBN = 8;
constexpr int RING = 64;    // pinned step-record slots

struct DataSet {
    float* frames = nullptr;
    long long* off = nullptr;
    int* len = nullptr;
    int* mirror = nullptr;
    int nseq = 0;
};

// a BatchNorm seam's buffers: the layer output a, normalised xhat, activated h (h is the next layer's input)
struct BNBuf { float *a = nullptr, *xhat = nullptr, *h = nullptr; };

}  // namespace

struct said_train {
    HostCtx c;
    int maxB = 0;
    hipStream_t s = nullptr;
    TrainStore st;            // the parameters and the optimizer's state
    long long nbuf = 0;
    std::vector<long long> off;   // offset of each tensor in st.P (parameters) or RS (running stats); counters: index into nbt
    float* RS = nullptr;
    long long nbt[NBN] = {};
    float* stats = nullptr;    // [NBN][2][256]
    // step record on the device and its pinned host ring
    float* rec = nullptr;
    size_t rec_n = 0;
    float* ring = nullptr;
    hipEvent_t ring_ev[RING] = {};
    bool ring_used[RING] = {};
    int ring_pos = 0;
    DataSet data[2];
    // activations
    float* X = nullptr;
    BNBuf e0, e1, e2, e4, e5, d0, d2, d3;
    float *F = nullptr, *A6 = nullptr, *MU = nullptr, *LV = nullptr, *Zb = nullptr, *D1 = nullptr, *D4 = nullptr, *U = nullptr;
    float *g0 = nullptr, *g1 = nullptr, *dMU = nullptr, *dLV = nullptr;
    std::map<int, hipGraphExec_t> graphs;
};

namespace {

int tindex(const char* name) {
    if (!name) return -1;
    for (int i = 0; i < 70; ++i)
        if (!strcmp(kTensors[i].name, name)) return i;
    return -1;
}
float* par(said_train* t, const float* base, const std::string& name) { return const_cast<float*>(base) + t->off[tindex(name.c_str())]; }
float* rs(said_train* t, const std::string& name) { return t->RS + t->off[tindex(name.c_str())]; }

TAct cf(const float* p, int Cn, int L) { return TAct{p, Cn * L, L, 1}; }        // channel-first (B, C, L)
TActW cfw(float* p, int Cn, int L) { return TActW{p, Cn * L, L, 1}; }
TAct tm(const float* p) { return TAct{p, T * C, 1, C}; }                        // time-major (B, 120, 32)
TActW tmw(float* p) { return TActW{p, T * C, 1, C}; }
TAct fl(const float* p, int F) { return TAct{p, F, 1, 1}; }                     // (B, F): channel c of sample b at b F + c, L = 1
TActW flw(float* p, int F) { return TActW{p, F, 1, 1}; }

int* rec_items(said_train*, float* rec) { return reinterpret_cast<int*>(rec + NSCAL + C); }
float* rec_eps(said_train* t, float* rec) { return rec + NSCAL + C + (size_t)t->maxB * ITEM; }

// the forward chain; base = P or E (parameters), train: batch statistics and running-stat updates
void enqueue_forward(said_train* t, int B, const float* base, int train, int set) {
    hipStream_t s = t->s;
    float* rec = t->rec;
    const DataSet& d = t->data[set];
    gather(s, B, d.frames, d.off, d.len, rec_items(t, rec), d.mirror, t->X);
    auto bn = [&](int i, TAct a, const BNBuf& b) {
        const std::string p = kBN[i].prefix;
        bn_fwd(s, train, B, kBN[i].C, kBN[i].L, a, par(t, base, p + ".weight"), par(t, base, p + ".bias"), rs(t, p + ".running_mean"),
               rs(t, p + ".running_var"), t->stats + i * 512, kBN[i].slope, b.xhat, b.h);
    };
    const std::string E = "encoder.", D = "decoder.";
    conv_fwd(s, 0, B, 32, 32, 3, 1, 120, 118, tm(t->X), par(t, base, E + "conv_layers.0.weight"), par(t, base, E + "conv_layers.0.bias"), cfw(t->e0.a, 32, 118));
    bn(0, cf(t->e0.a, 32, 118), t->e0);
    conv_fwd(s, 0, B, 32, 64, 3, 1, 118, 116, cf(t->e0.h, 32, 118), par(t, base, E + "conv_layers.3.weight"), par(t, base, E + "conv_layers.3.bias"), cfw(t->e1.a, 64, 116));
    bn(1, cf(t->e1.a, 64, 116), t->e1);
    conv_fwd(s, 0, B, 64, 64, 4, 2, 116, 57, cf(t->e1.h, 64, 116), par(t, base, E + "conv_layers.6.weight"), par(t, base, E + "conv_layers.6.bias"), cfw(t->e2.a, 64, 57));
    bn(2, cf(t->e2.a, 64, 57), t->e2);
    conv_fwd(s, 0, B, 64, 32, 3, 1, 57, 55, cf(t->e2.h, 64, 57), par(t, base, E + "conv_layers.9.weight"), par(t, base, E + "conv_layers.9.bias"), cfw(t->F, 32, 55));
    linear_fwd(s, B, 1760, 256, t->F, par(t, base, E + "fc_layers.0.weight"), par(t, base, E + "fc_layers.0.bias"), t->e4.a);
    bn(3, fl(t->e4.a, 256), t->e4);
    linear_fwd(s, B, 256, 128, t->e4.h, par(t, base, E + "fc_layers.3.weight"), par(t, base, E + "fc_layers.3.bias"), t->e5.a);
    bn(4, fl(t->e5.a, 128), t->e5);
    linear_fwd(s, B, 128, 64, t->e5.h, par(t, base, E + "fc_layers.6.weight"), par(t, base, E + "fc_layers.6.bias"), t->A6);
    linear_fwd(s, B, 64, 64, t->A6, par(t, base, E + "fc_mu.weight"), par(t, base, E + "fc_mu.bias"), t->MU);
    linear_fwd(s, B, 64, 64, t->A6, par(t, base, E + "fc_logvar.weight"), par(t, base, E + "fc_logvar.bias"), t->LV);
    reparam(s, B, t->MU, t->LV, rec_eps(t, rec), t->Zb);
    linear_fwd(s, B, 64, 240, t->Zb, par(t, base, D + "fc_layers.0.weight"), par(t, base, D + "fc_layers.0.bias"), t->d0.a);
    bn(5, fl(t->d0.a, 240), t->d0);
    linear_fwd(s, B, 240, 480, t->d0.h, par(t, base, D + "fc_layers.3.weight"), par(t, base, D + "fc_layers.3.bias"), t->D1);
    conv_fwd(s, 1, B, 4, 32, 3, 1, 120, 122, cf(t->D1, 4, 120), par(t, base, D + "conv_layers.0.weight"), par(t, base, D + "conv_layers.0.bias"), cfw(t->d2.a, 32, 122));
    bn(6, cf(t->d2.a, 32, 122), t->d2);
    conv_fwd(s, 1, B, 32, 32, 3, 1, 122, 124, cf(t->d2.h, 32, 122), par(t, base, D + "conv_layers.3.weight"), par(t, base, D + "conv_layers.3.bias"), cfw(t->d3.a, 32, 124));
    bn(7, cf(t->d3.a, 32, 124), t->d3);
    conv_fwd(s, 0, B, 32, 32, 3, 1, 124, 122, cf(t->d3.h, 32, 124), par(t, base, D + "conv_layers.6.weight"), par(t, base, D + "conv_layers.6.bias"), cfw(t->D4, 32, 122));
    conv_fwd(s, 0, B, 32, 32, 3, 1, 122, 120, cf(t->D4, 32, 122), par(t, base, D + "conv_layers.7.weight"), par(t, base, D + "conv_layers.7.bias"), tmw(t->U));
}

// backward of the whole chain into G (every parameter's gradient is written, none accumulated)
void enqueue_backward(said_train* t, int B) {
    hipStream_t s = t->s;
    const float* P = t->st.P;
    float* G = t->st.G;
    float *g0 = t->g0, *g1 = t->g1;
    const std::string E = "encoder.", D = "decoder.";
    auto w = [&](const std::string& n) { return par(t, P, n); };
    auto gw = [&](const std::string& n) { return par(t, G, n); };
    auto bnb = [&](int i, TAct dh, const BNBuf& b, TAct hl, TAct xl, TActW da) {
        const std::string p = kBN[i].prefix;
        bn_bwd(s, B, kBN[i].C, kBN[i].L, dh, hl, xl, w(p + ".weight"), t->stats + i * 512, kBN[i].slope, gw(p + ".weight"), gw(p + ".bias"), da);
        (void)b;
    };
    // loss -> du (g0, time-major)
    loss(s, B, t->X, t->U, t->MU, t->LV, t->rec, g0, t->st.last, t->st.acc);
    // decoder conv_layers.7: D4 -> U
    conv_bwd_weight(s, 0, B, 32, 32, 3, 1, 122, 120, cf(t->D4, 32, 122), tm(g0), gw(D + "conv_layers.7.weight"), gw(D + "conv_layers.7.bias"));
    conv_bwd_data(s, 0, B, 32, 32, 3, 1, 122, 120, tm(g0), w(D + "conv_layers.7.weight"), cfw(g1, 32, 122));
    // conv_layers.6: d3.h -> D4
    conv_bwd_weight(s, 0, B, 32, 32, 3, 1, 124, 122, cf(t->d3.h, 32, 124), cf(g1, 32, 122), gw(D + "conv_layers.6.weight"), gw(D + "conv_layers.6.bias"));
    conv_bwd_data(s, 0, B, 32, 32, 3, 1, 124, 122, cf(g1, 32, 122), w(D + "conv_layers.6.weight"), cfw(g0, 32, 124));
    bnb(7, cf(g0, 32, 124), t->d3, cf(t->d3.h, 32, 124), cf(t->d3.xhat, 32, 124), cfw(g1, 32, 124));
    // conv_layers.3 (transposed): d2.h -> d3.a
    conv_bwd_weight(s, 1, B, 32, 32, 3, 1, 122, 124, cf(t->d2.h, 32, 122), cf(g1, 32, 124), gw(D + "conv_layers.3.weight"), gw(D + "conv_layers.3.bias"));
    conv_bwd_data(s, 1, B, 32, 32, 3, 1, 122, 124, cf(g1, 32, 124), w(D + "conv_layers.3.weight"), cfw(g0, 32, 122));
    bnb(6, cf(g0, 32, 122), t->d2, cf(t->d2.h, 32, 122), cf(t->d2.xhat, 32, 122), cfw(g1, 32, 122));
    // conv_layers.0 (transposed): D1 (4, 120) -> d2.a
    conv_bwd_weight(s, 1, B, 4, 32, 3, 1, 120, 122, cf(t->D1, 4, 120), cf(g1, 32, 122), gw(D + "conv_layers.0.weight"), gw(D + "conv_layers.0.bias"));
    conv_bwd_data(s, 1, B, 4, 32, 3, 1, 120, 122, cf(g1, 32, 122), w(D + "conv_layers.0.weight"), cfw(g0, 4, 120));
    // fc_layers.3: d0.h -> D1
    linear_bwd_weight(s, B, 240, 480, t->d0.h, g0, gw(D + "fc_layers.3.weight"), gw(D + "fc_layers.3.bias"));
    linear_bwd_data(s, B, 240, 480, g0, w(D + "fc_layers.3.weight"), nullptr, nullptr, g1);
    bnb(5, fl(g1, 240), t->d0, fl(t->d0.h, 240), fl(t->d0.xhat, 240), flw(g0, 240));
    // fc_layers.0: Z -> d0.a
    linear_bwd_weight(s, B, 64, 240, t->Zb, g0, gw(D + "fc_layers.0.weight"), gw(D + "fc_layers.0.bias"));
    linear_bwd_data(s, B, 64, 240, g0, w(D + "fc_layers.0.weight"), nullptr, nullptr, g1);
    // reparametrisation and KL -> dmu, dlv
    kl_reparam_bwd(s, B, t->MU, t->LV, rec_eps(t, t->rec), g1, t->rec, t->dMU, t->dLV);
    linear_bwd_weight(s, B, 64, 64, t->A6, t->dMU, gw(E + "fc_mu.weight"), gw(E + "fc_mu.bias"));
    linear_bwd_weight(s, B, 64, 64, t->A6, t->dLV, gw(E + "fc_logvar.weight"), gw(E + "fc_logvar.bias"));
    linear_bwd_data(s, B, 64, 64, t->dMU, w(E + "fc_mu.weight"), t->dLV, w(E + "fc_logvar.weight"), g0);
    // encoder fc_layers.6: e5.h -> A6
    linear_bwd_weight(s, B, 128, 64, t->e5.h, g0, gw(E + "fc_layers.6.weight"), gw(E + "fc_layers.6.bias"));
    linear_bwd_data(s, B, 128, 64, g0, w(E + "fc_layers.6.weight"), nullptr, nullptr, g1);
    bnb(4, fl(g1, 128), t->e5, fl(t->e5.h, 128), fl(t->e5.xhat, 128), flw(g0, 128));
    linear_bwd_weight(s, B, 256, 128, t->e4.h, g0, gw(E + "fc_layers.3.weight"), gw(E + "fc_layers.3.bias"));
    linear_bwd_data(s, B, 256, 128, g0, w(E + "fc_layers.3.weight"), nullptr, nullptr, g1);
    bnb(3, fl(g1, 256), t->e4, fl(t->e4.h, 256), fl(t->e4.xhat, 256), flw(g0, 256));
    linear_bwd_weight(s, B, 1760, 256, t->F, g0, gw(E + "fc_layers.0.weight"), gw(E + "fc_layers.0.bias"));
    linear_bwd_data(s, B, 1760, 256, g0, w(E + "fc_layers.0.weight"), nullptr, nullptr, g1);
    // conv_layers.9: e2.h (64, 57) -> F (32, 55)
    conv_bwd_weight(s, 0, B, 64, 32, 3, 1, 57, 55, cf(t->e2.h, 64, 57), cf(g1, 32, 55), gw(E + "conv_layers.9.weight"), gw(E + "conv_layers.9.bias"));
    conv_bwd_data(s, 0, B, 64, 32, 3, 1, 57, 55, cf(g1, 32, 55), w(E + "conv_layers.9.weight"), cfw(g0, 64, 57));
    bnb(2, cf(g0, 64, 57), t->e2, cf(t->e2.h, 64, 57), cf(t->e2.xhat, 64, 57), cfw(g1, 64, 57));
    conv_bwd_weight(s, 0, B, 64, 64, 4, 2, 116, 57, cf(t->e1.h, 64, 116), cf(g1, 64, 57), gw(E + "conv_layers.6.weight"), gw(E + "conv_layers.6.bias"));
    conv_bwd_data(s, 0, B, 64, 64, 4, 2, 116, 57, cf(g1, 64, 57), w(E + "conv_layers.6.weight"), cfw(g0, 64, 116));
    bnb(1, cf(g0, 64, 116), t->e1, cf(t->e1.h, 64, 116), cf(t->e1.xhat, 64, 116), cfw(g1, 64, 116));
    conv_bwd_weight(s, 0, B, 32, 64, 3, 1, 118, 116, cf(t->e0.h, 32, 118), cf(g1, 64, 116), gw(E + "conv_layers.3.weight"), gw(E + "conv_layers.3.bias"));
    conv_bwd_data(s, 0, B, 32, 64, 3, 1, 118, 116, cf(g1, 64, 116), w(E + "conv_layers.3.weight"), cfw(g0, 32, 118));
    bnb(0, cf(g0, 32, 118), t->e0, cf(t->e0.h, 32, 118), cf(t->e0.xhat, 32, 118), cfw(g1, 32, 118));
    conv_bwd_weight(s, 0, B, 32, 32, 3, 1, 120, 118, tm(t->X), cf(g1, 32, 118), gw(E + "conv_layers.0.weight"), gw(E + "conv_layers.0.bias"));
}

void enqueue_step(said_train* t, int B) {
    enqueue_forward(t, B, t->st.P, 1, SAID_TRAIN_SET_TRAIN);
    enqueue_backward(t, B);
    store_enqueue_update(&t->st, t->s, t->rec);
}

// copy the step record (scalars, std, items, eps) through the next pinned ring slot to the device
int put_record(said_train* t, int B, const int* items, const float* eps, const float* scalars, const float* std_) {
    HostCtx* ctx = &t->c;
    const int k = t->ring_pos;
    t->ring_pos = (k + 1) % RING;
    if (t->ring_used[k]) HIPCHK(hipEventSynchronize(t->ring_ev[k]));   // only waits when the device is RING steps behind
    float* h = t->ring + (size_t)k * t->rec_n;
    memset(h, 0, t->rec_n * sizeof(float));
    if (scalars) memcpy(h, scalars, sizeof(float) * (SAID_TRAIN_NSCAL));
    h[S_USE_STD] = std_ ? 1.f : 0.f;
    if (std_) memcpy(h + NSCAL, std_, sizeof(float) * C);
    if (items) memcpy(rec_items(t, h), items, sizeof(int) * B * ITEM);
    if (eps) memcpy(rec_eps(t, h), eps, sizeof(float) * B * Z);
    HIPCHK(hipMemcpyAsync(t->rec, h, t->rec_n * sizeof(float), hipMemcpyHostToDevice, t->s));
    HIPCHK(hipEventRecord(t->ring_ev[k], t->s));
    t->ring_used[k] = true;
    return 0;
}

int check_items(said_train* t, int set, int B, const int* items, const char* what) {
    HostCtx* ctx = &t->c;
    if (set != 0 && set != 1) return fail(ctx, "%s: set %d is neither SAID_TRAIN_SET_TRAIN nor SAID_TRAIN_SET_VAL", what, set);
    if (B < 1 || B > t->maxB) return fail(ctx, "%s: batch %d outside [1, %d] (the context's max_batch)", what, B, t->maxB);
    if (!t->data[set].frames) return fail(ctx, "%s: no window set uploaded as set %d (said_train_set_data)", what, set);
    if (!items) return fail(ctx, "%s: items are null", what);
    for (int b = 0; b < B; ++b) {
        const int* it = items + b * ITEM;
        if (it[0] < 0 || it[0] >= t->data[set].nseq) return fail(ctx, "%s: item %d names sequence %d of %d", what, b, it[0], t->data[set].nseq);
    }
    return 0;
}

int check_std(said_train* t, const float* std_, const char* what) {
    if (!std_) return 0;
    for (int c = 0; c < C; ++c)
        if (!(std::isfinite(std_[c]) && std_[c] != 0.f)) return fail(&t->c, "%s: std[%d] = %g is not a finite non-zero value", what, c, (double)std_[c]);
    return 0;
}

float* copy_of(said_train* t, int which, int i) {
    const TDesc& d = kTensors[i];
    if (d.kind == K_RMEAN || d.kind == K_RVAR) return which == SAID_TRAIN_STATE ? t->RS + t->off[i] : nullptr;
    return d.kind == K_PARAM ? store_copy_of(&t->st, which, t->off[i]) : nullptr;
}

}  // namespace

extern "C" {

const char* said_train_tensor_name(int i) { return (i >= 0 && i < 70) ? kTensors[i].name : nullptr; }
long long said_train_tensor_numel(int i) { return (i >= 0 && i < 70) ? kTensors[i].numel : -1; }
int said_train_tensor_is_counter(int i) { return (i >= 0 && i < 70) ? (kTensors[i].kind == K_COUNT) : -1; }

int said_train_create(said_train** out, int device, int max_batch) {
    DeviceRestore restore_device;
    said_train* t = new_ctx("said_train_create", out, device);
    if (!t) return -1;
    if (max_batch < 1 || max_batch > 4096) { delete t; return fail(nullptr, "said_train_create: max_batch %d outside [1, 4096]", max_batch); }
    HostCtx* ctx = &t->c;
    t->maxB = max_batch;
    std::vector<long long> sizes(70);
    for (int i = 0; i < 70; ++i) sizes[i] = kTensors[i].kind == K_PARAM ? kTensors[i].numel : 0;
    t->rec_n = NSCAL + C + (size_t)max_batch * ITEM + (size_t)max_batch * Z;
    const size_t Bm = (size_t)max_batch;
    auto bnbuf = [&](BNBuf& b, size_t n) { return dalloc(ctx, &b.a, Bm * n) || dalloc(ctx, &b.xhat, Bm * n) || dalloc(ctx, &b.h, Bm * n); };
    int rc = store_build(&t->st, ctx, sizes, false, &t->off);
    for (int i = 0, nb = 0; i < 70; ++i) {
        const TDesc& d = kTensors[i];
        if (d.kind == K_COUNT) {
            t->off[i] = nb++;
        } else if (d.kind != K_PARAM) {
            t->off[i] = t->nbuf;
            t->nbuf += d.numel;
        }
    }
    rc = rc || hipStreamCreateWithFlags(&t->s, hipStreamNonBlocking) != hipSuccess;
    rc = rc || dalloc(ctx, &t->RS, t->nbuf) || dalloc(ctx, &t->stats, (size_t)NBN * 512) || dalloc(ctx, &t->rec, t->rec_n);
    rc = rc || dalloc(ctx, &t->X, Bm * T * C) || bnbuf(t->e0, 32 * 118) || bnbuf(t->e1, 64 * 116) || bnbuf(t->e2, 64 * 57) || bnbuf(t->e4, 256) ||
         bnbuf(t->e5, 128) || bnbuf(t->d0, 240) || bnbuf(t->d2, 32 * 122) || bnbuf(t->d3, 32 * 124) || dalloc(ctx, &t->F, Bm * 1760) ||
         dalloc(ctx, &t->A6, Bm * Z) || dalloc(ctx, &t->MU, Bm * Z) || dalloc(ctx, &t->LV, Bm * Z) || dalloc(ctx, &t->Zb, Bm * Z) ||
         dalloc(ctx, &t->D1, Bm * 480) || dalloc(ctx, &t->D4, Bm * 32 * 122) || dalloc(ctx, &t->U, Bm * T * C) ||
         dalloc(ctx, &t->g0, Bm * 64 * 116) || dalloc(ctx, &t->g1, Bm * 64 * 116) || dalloc(ctx, &t->dMU, Bm * Z) || dalloc(ctx, &t->dLV, Bm * Z);
    rc = rc || hipHostMalloc((void**)&t->ring, (size_t)RING * t->rec_n * sizeof(float), hipHostMallocDefault) != hipSuccess;
    for (int k = 0; k < RING && !rc; ++k) rc = hipEventCreateWithFlags(&t->ring_ev[k], hipEventDisableTiming) != hipSuccess;
    if (!rc) {
        std::vector<float> one(t->nbuf, 1.f);   // running_var starts at one, running_mean at zero (nn.BatchNorm1d)
        for (int i = 0; i < 70 && !rc; ++i)
            if (kTensors[i].kind == K_RVAR) rc = hipMemcpy(t->RS + t->off[i], one.data(), kTensors[i].numel * sizeof(float), hipMemcpyHostToDevice) != hipSuccess;
    }
    if (rc) {
        g_create_err = ctx->err.empty() ? std::string("said_train_create: allocation failed") : ctx->err;
        said_train_destroy(t);
        return -1;
    }
    *out = t;
    return 0;
}

int said_train_destroy(said_train* t) {
    if (!t) return 0;
    DeviceRestore restore_device;
    (void)hipSetDevice(t->c.device);
    if (t->s) (void)hipStreamSynchronize(t->s);
    for (auto& kv : t->graphs) (void)hipGraphExecDestroy(kv.second);
    for (int k = 0; k < RING; ++k)
        if (t->ring_ev[k]) (void)hipEventDestroy(t->ring_ev[k]);
    if (t->ring) (void)hipHostFree(t->ring);
    if (t->s) (void)hipStreamDestroy(t->s);   // (synchronised above)
    return delete_ctx(t);
}

const char* said_train_last_error(const said_train* t) { return ctx_error(t); }

int said_train_set_tensor(said_train* t, int which, const char* name, const void* host, long long n) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    const int i = tindex(name);
    if (i < 0) return fail(ctx, "said_train_set_tensor: unknown tensor %s", name ? name : "(null)");
    if (!host || n != kTensors[i].numel) return fail(ctx, "said_train_set_tensor: %s has %lld elements, got %lld", name, kTensors[i].numel, n);
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (kTensors[i].kind == K_COUNT) {
        if (which != SAID_TRAIN_STATE) return fail(ctx, "said_train_set_tensor: %s is a buffer, it has no copy %d", name, which);
        t->nbt[t->off[i]] = *static_cast<const long long*>(host);
        return 0;
    }
    float* dst = copy_of(t, which, i);
    if (!dst) return fail(ctx, "said_train_set_tensor: %s has no copy %d (buffers have only SAID_TRAIN_STATE)", name, which);
    return store_copy(&t->st, t->s, dst, static_cast<const float*>(host), n, hipMemcpyHostToDevice, true);
}

int said_train_get_tensor(said_train* t, int which, const char* name, void* host, long long n) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    const int i = tindex(name);
    if (i < 0) return fail(ctx, "said_train_get_tensor: unknown tensor %s", name ? name : "(null)");
    if (!host || n != kTensors[i].numel) return fail(ctx, "said_train_get_tensor: %s has %lld elements, got %lld", name, kTensors[i].numel, n);
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (kTensors[i].kind == K_COUNT) {
        if (which != SAID_TRAIN_STATE) return fail(ctx, "said_train_get_tensor: %s is a buffer, it has no copy %d", name, which);
        *static_cast<long long*>(host) = t->nbt[t->off[i]];
        return 0;
    }
    float* src = copy_of(t, which, i);
    if (!src) return fail(ctx, "said_train_get_tensor: %s has no copy %d (buffers have only SAID_TRAIN_STATE)", name, which);
    return store_copy(&t->st, t->s, static_cast<float*>(host), src, n, hipMemcpyDeviceToHost, true);
}

int said_train_reset_optimizer(said_train* t) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    return store_reset_optimizer(&t->st, t->s);
}

int said_train_set_data(said_train* t, int set, const float* frames, long long nframes, const long long* off, const int* len, int nseq, const int* mirror) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (set != 0 && set != 1) return fail(ctx, "said_train_set_data: set %d is neither SAID_TRAIN_SET_TRAIN nor SAID_TRAIN_SET_VAL", set);
    if (!frames || !off || !len || !mirror || nseq < 1 || nframes < 1) return fail(ctx, "said_train_set_data: empty or null window set");
    for (int s = 0; s < nseq; ++s)
        if (len[s] < 1 || off[s] < 0 || off[s] + len[s] > nframes) return fail(ctx, "said_train_set_data: sequence %d (offset %lld, %d frames) outside the %lld frames", s, off[s], len[s], nframes);
    for (int c = 0; c < C; ++c)
        if (mirror[c] < 0 || mirror[c] >= C) return fail(ctx, "said_train_set_data: mirror[%d] = %d is not a channel", c, mirror[c]);
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(t->s));
    DataSet& d = t->data[set];
    if (drealloc(ctx, &d.frames, (size_t)nframes * C, false) || drealloc(ctx, &d.off, (size_t)nseq, false) || drealloc(ctx, &d.len, (size_t)nseq, false) ||
        drealloc(ctx, &d.mirror, (size_t)C, false))
        return -1;
    HIPCHK(hipMemcpy(d.frames, frames, (size_t)nframes * C * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.off, off, (size_t)nseq * sizeof(long long), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.len, len, (size_t)nseq * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d.mirror, mirror, (size_t)C * sizeof(int), hipMemcpyHostToDevice));
    d.nseq = nseq;
    if (set == SAID_TRAIN_SET_TRAIN) {   // the step graphs hold the old set's pointers
        for (auto& kv : t->graphs) (void)hipGraphExecDestroy(kv.second);
        t->graphs.clear();
    }
    return 0;
}

int said_train_gather(said_train* t, int set, int B, const int* items, float* x_host) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (check_items(t, set, B, items, "said_train_gather")) return -1;
    if (!x_host) return fail(ctx, "said_train_gather: null output");
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (put_record(t, B, items, nullptr, nullptr, nullptr)) return -1;
    const DataSet& d = t->data[set];
    gather(t->s, B, d.frames, d.off, d.len, rec_items(t, t->rec), d.mirror, t->X);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(x_host, t->X, (size_t)B * T * C * sizeof(float), hipMemcpyDeviceToHost, t->s));
    HIPCHK(hipStreamSynchronize(t->s));
    return 0;
}

int said_train_step(said_train* t, int B, const int* items, const float* eps, const float* scalars, const float* std_, int use_graph) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (B == 1)
        return fail(ctx, "said_train_step: a batch of 1 cannot train (BatchNorm1d expects more than 1 value per channel when training; "
                         "the linear layers' statistics run over the batch)");
    if (check_items(t, SAID_TRAIN_SET_TRAIN, B, items, "said_train_step") || check_std(t, std_, "said_train_step")) return -1;
    if (!eps || !scalars) return fail(ctx, "said_train_step: null eps or scalars");
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (put_record(t, B, items, eps, scalars, std_)) return -1;
    if (use_graph) {
        auto it = t->graphs.find(B);
        if (it == t->graphs.end()) {
            hipGraph_t g = nullptr;
            hipGraphExec_t ge = nullptr;
            HIPCHK(hipStreamBeginCapture(t->s, hipStreamCaptureModeThreadLocal));
            enqueue_step(t, B);
            const hipError_t le = hipGetLastError();
            HIPCHK(hipStreamEndCapture(t->s, &g));
            if (le != hipSuccess) {
                (void)hipGraphDestroy(g);
                return fail(ctx, "said_train_step: launch failed during capture: %s", hipGetErrorString(le));
            }
            const hipError_t ie = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ie != hipSuccess) return fail(ctx, "said_train_step: hipGraphInstantiate failed: %s", hipGetErrorString(ie));
            it = t->graphs.emplace(B, ge).first;
        }
        HIPCHK(hipGraphLaunch(it->second, t->s));
    } else {
        enqueue_step(t, B);
        HIPCHK(hipGetLastError());
    }
    for (int i = 0; i < NBN; ++i) ++t->nbt[i];
    return 0;
}

int said_train_apply_update(said_train* t, const float* scalars) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (!scalars) return fail(ctx, "said_train_apply_update: null scalars");
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (put_record(t, 0, nullptr, nullptr, scalars, nullptr)) return -1;
    store_enqueue_update(&t->st, t->s, t->rec);
    HIPCHK(hipGetLastError());
    return 0;
}

int said_train_eval_loss(said_train* t, int set, int B, const int* items, const float* eps, const float* scalars, const float* std_, int ema) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (check_items(t, set, B, items, "said_train_eval_loss") || check_std(t, std_, "said_train_eval_loss")) return -1;
    if (!eps || !scalars) return fail(ctx, "said_train_eval_loss: null eps or scalars");
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (put_record(t, B, items, eps, scalars, std_)) return -1;
    enqueue_forward(t, B, ema ? t->st.E : t->st.P, 0, set);
    loss(t->s, B, t->X, t->U, t->MU, t->LV, t->rec, nullptr, t->st.last, t->st.acc + NACC);
    HIPCHK(hipGetLastError());
    return 0;
}

int said_train_read_losses(said_train* t, int val, double* acc_host, int* status, int reset) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (!acc_host) return fail(ctx, "said_train_read_losses: null output");
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    return store_read_losses(&t->st, t->s, val, acc_host, status, reset);
}

int said_train_last_losses(said_train* t, float* out) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (!out) return fail(ctx, "said_train_last_losses: null output");
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(out, t->st.last, 4 * sizeof(float), hipMemcpyDeviceToHost, t->s));
    HIPCHK(hipStreamSynchronize(t->s));
    return 0;
}

int said_train_bn_stats(said_train* t, int bn, float* out) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (bn < 0 || bn >= NBN || !out) return fail(ctx, "said_train_bn_stats: layer %d outside [0, %d) or null output", bn, NBN);
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    const int Cn = kBN[bn].C;
    HIPCHK(hipMemcpyAsync(out, t->stats + bn * 512, Cn * sizeof(float), hipMemcpyDeviceToHost, t->s));
    HIPCHK(hipMemcpyAsync(out + Cn, t->stats + bn * 512 + Cn, Cn * sizeof(float), hipMemcpyDeviceToHost, t->s));
    HIPCHK(hipStreamSynchronize(t->s));
    return 0;
}

int said_train_graph_count(const said_train* t) { return t ? (int)t->graphs.size() : 0; }

}  // extern "C"
