// unet_trainer.cpp — the UNet denoiser trainer context (include/said_unet_train.h): the table of trainable tensors, the device copies of the
// parameters and of the optimizer, the activation arena, and the step: add_noise, forward, objective, backward, clip, AdamW, EMA, launched in that
// order on the context's stream (unet_train.hip).  T is a run-time value, so nothing is captured into a graph.  A context made with
// feature_dim = F > 0 also holds and trains audio_proj_layer (768 -> F) and runs the context at width F; F <= 0 leaves every launch as it is.
// A context made with finetune_layers = L > 0 (said_unet_finetune.h) also holds and trains the Wav2Vec2 transformer in the same store: its
// forward runs in front of the UNet's and its backward behind it (kernels: audio_ft.hip); L <= 0 leaves every launch as it is.  Such a context
// can run the encoder's dense products on split-fp16 operands (said_unet_train_products.h; kernel: enc_gemm.hip); the default leaves every
// launch as it is.
#include "said_unet_train_products.h"

#include "audio_ft.h"
#include "enc_gemm.h"
#include "engine_internal.h"
#include "train_store.h"
#include "unet_train.h"
#include "ut_gemm_plan.h"

#include <map>
#include <mutex>

using namespace said::ut;

static_assert(OPT_SLOTS_MATCH(SAID_UT_S_), "said_unet_train.h and train_opt.h disagree on the optimizer's slots of the step record");
static_assert(NACC == TS_NACC && A_BAD == TS_A_BAD && SAID_UT_NOT_FINITE == 1, "train_store.h reads the accumulators of unet_train.h");

namespace {

struct TDesc { std::string name; long long numel; };
constexpr int CH = 192, TEd = 768, FF = 768, NH = 6;
constexpr int AUD = SAID_UT_CTX_DIM;   // width of the frozen encoder's output, and of the context without an audio_proj_layer

// null_cond_emb, (F > 0: audio_proj_layer,) then UNet1DConditionModel.state_dict() under "denoiser.", in the reference's registration order.
// F <= 0: the context is the encoder's output itself (SAID_UNet1D(feature_dim = -1))
// audio_encoder.* of an L-layer wav2vec2-base encoder without its feature extractor, in state-dict order (transformers 4.30.2 key layout)
constexpr int EH = 768, ECONV = 512, EFFN = 3072, ENH = 12, EHD = 64, EPK = 128, EPG = 16, EPC = EH / EPG, MAXL = 32;
static_assert(TEd == UT_TED && EH == UT_EH && EPG == UT_EPG && EPC == UT_EPC && EPK == UT_EPK, "ut_gemm_plan.h sizes gpart for these widths");
const char* const kEnc = "audio_encoder.";
std::string enc_layer(int l) { return std::string(kEnc) + "encoder.layers." + std::to_string(l); }
void add_encoder(std::vector<TDesc>& v, int L) {
    auto add = [&](const std::string& n, long long k) { v.push_back({kEnc + n, k}); };
    auto wb = [&](const std::string& n, long long no, long long ni) { add(n + ".weight", no * ni); add(n + ".bias", no); };
    add("masked_spec_embed", EH);
    wb("feature_projection.layer_norm", ECONV, 1);
    wb("feature_projection.projection", EH, ECONV);
    add("encoder.pos_conv_embed.conv.bias", EH);
    add("encoder.pos_conv_embed.conv.weight_g", EPK);
    add("encoder.pos_conv_embed.conv.weight_v", (long long)EH * EPC * EPK);
    wb("encoder.layer_norm", EH, 1);
    for (int l = 0; l < L; ++l) {
        const std::string p = "encoder.layers." + std::to_string(l);
        for (const char* n : {"k_proj", "v_proj", "q_proj", "out_proj"}) wb(p + ".attention." + n, EH, EH);
        wb(p + ".layer_norm", EH, 1);
        wb(p + ".feed_forward.intermediate_dense", EFFN, EH);
        wb(p + ".feed_forward.output_dense", EH, EFFN);
        wb(p + ".final_layer_norm", EH, 1);
    }
}

std::vector<TDesc> make_table(int F, int L) {
    std::vector<TDesc> v;
    auto add = [&](const std::string& n, long long k) { v.push_back({n, k}); };
    const int CTX = F > 0 ? F : AUD;
    add("null_cond_emb", CTX);
    if (F > 0) { add("audio_proj_layer.weight", (long long)F * AUD); add("audio_proj_layer.bias", F); }
    const std::string m = "denoiser.model.";
    add(m + "time_embed.0.weight", TEd * CH); add(m + "time_embed.0.bias", TEd);
    add(m + "time_embed.2.weight", TEd * TEd); add(m + "time_embed.2.bias", TEd);
    add(m + "input_blocks.0.0.weight", CH * XC * 3); add(m + "input_blocks.0.0.bias", CH);
    auto res = [&](const std::string& p, int cin) {
        add(p + ".in_layers.0.weight", cin); add(p + ".in_layers.0.bias", cin);
        add(p + ".in_layers.2.weight", (long long)CH * cin * 3); add(p + ".in_layers.2.bias", CH);
        add(p + ".emb_layers.1.weight", CH * TEd); add(p + ".emb_layers.1.bias", CH);
        add(p + ".out_layers.0.weight", CH); add(p + ".out_layers.0.bias", CH);
        add(p + ".out_layers.3.weight", CH * CH * 3); add(p + ".out_layers.3.bias", CH);
        if (cin != CH) { add(p + ".skip_connection.weight", (long long)CH * cin); add(p + ".skip_connection.bias", CH); }
    };
    auto st = [&](const std::string& p) {
        add(p + ".norm.weight", CH); add(p + ".norm.bias", CH);
        const std::string b = p + ".transformer_blocks.0";
        auto attn = [&](int a) {
            const std::string q = b + ".attn" + std::to_string(a);
            const int kd = a == 1 ? CH : CTX;
            add(q + ".to_q.weight", CH * CH); add(q + ".to_k.weight", CH * kd); add(q + ".to_v.weight", CH * kd);
            add(q + ".to_out.0.weight", CH * CH); add(q + ".to_out.0.bias", CH);
        };
        // BasicTransformerBlock registers attn1, ff, attn2, norm1..3 (ldm/attention.py:144-157)
        attn(1);
        add(b + ".ff.net.0.proj.weight", 2 * FF * CH); add(b + ".ff.net.0.proj.bias", 2 * FF);
        add(b + ".ff.net.2.weight", CH * FF); add(b + ".ff.net.2.bias", CH);
        attn(2);
        for (int n = 1; n <= 3; ++n) { add(b + ".norm" + std::to_string(n) + ".weight", CH); add(b + ".norm" + std::to_string(n) + ".bias", CH); }
        add(p + ".proj_out.weight", CH * CH); add(p + ".proj_out.bias", CH);
    };
    res(m + "input_blocks.1.0", CH); st(m + "input_blocks.1.1");
    res(m + "middle_block.0", CH); st(m + "middle_block.1"); res(m + "middle_block.2", CH);
    res(m + "output_blocks.0.0", 2 * CH); st(m + "output_blocks.0.1");
    res(m + "output_blocks.1.0", 2 * CH); st(m + "output_blocks.1.1");
    add(m + "out.0.weight", CH); add(m + "out.0.bias", CH);
    add(m + "out.2.weight", XC * CH * 3); add(m + "out.2.bias", XC);
    if (L > 0) add_encoder(v, L);
    return v;
}
// the table of feature_dim F (<= 0: the default one) and L fine-tuned encoder layers (<= 0: a frozen encoder), built once; a std::map's
// nodes stay where they are
const std::vector<TDesc>& table(int F = 0, int L = 0) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, std::vector<TDesc>> tabs;
    const std::pair<int, int> key(F > 0 ? F : 0, L > 0 ? L : 0);
    std::lock_guard<std::mutex> lock(mu);
    auto it = tabs.find(key);
    if (it == tabs.end()) it = tabs.emplace(key, make_table(key.first, key.second)).first;
    return it->second;
}
const char* kRes[5] = {"denoiser.model.input_blocks.1.0", "denoiser.model.middle_block.0", "denoiser.model.middle_block.2",
                       "denoiser.model.output_blocks.0.0", "denoiser.model.output_blocks.1.0"};
const int kResCin[5] = {CH, CH, CH, 2 * CH, 2 * CH};
const char* kST[4] = {"denoiser.model.input_blocks.1.1", "denoiser.model.middle_block.1", "denoiser.model.output_blocks.0.1",
                      "denoiser.model.output_blocks.1.1"};
constexpr int VBLK = 256;

// what a ResBlock / SpatialTransformer keeps from the forward
struct ResAct { const float* x; int ldx; float *xh1, *rs1, *a1, *ee, *c1, *xh2, *rs2, *a2, *out; };
struct STAct {
    const float* x;
    float *xhg, *rsg, *hn, *xh1, *rs1, *y1, *q, *k, *v, *P1, *o1, *x1, *xh2, *rs2, *y2, *q2, *k2, *v2, *P2, *o2, *x2, *xh3, *rs3, *y3, *u, *gg, *x3, *out;
};
struct Acts {
    float *ctx, *noisy, *answer, *temb, *e1, *e1s, *emb, *embs, *h0, *cat0, *cat1, *xho, *rso, *ho, *pred;
    ResAct r[5];
    STAct s[4];
    // backward scratch
    float *d, *dcat, *dH0, *dH1, *g1, *g2, *g3, *g4, *g5, *big1, *big2, *PB, *dctx, *dee, *dembs, *demb, *de1s, *de1, *R, *dpred, *GV;
    // feature_dim > 0: the projected audio (B T, F) and the conditional samples' rows of dctx
    float *proj, *dcond;
};
// what the fine-tuned encoder keeps from its forward: per layer the input, q, k, v, the undropped probabilities, the attention output, both
// LayerNorms' xhat / rstd, the FFN's pre-activation and its dropped GELU, the layer's output
struct EncLayer { const float* x; float *q, *k, *v, *P, *o, *xh1, *rs1, *x1, *u, *gd, *xh2, *rs2, *out; };
struct EncActs {
    float *xh0, *rs0, *y0, *hp, *h0, *wnorm, *w, *pospre, *pos, *xhf, *rsf, *x0;
    EncLayer l[MAXL];
    const float* out;   // the last hidden state (B T, 768)
    // scratch of the forward and the backward
    float *t768, *Pd, *PB, *d, *g1, *g2, *g3, *big, *dw, *wnpart, *wndot, *dy0;
};

}  // namespace

struct said_unet_train {
    HostCtx c;
    int maxB = 0, maxT = 0;
    int F = 0, CTX = AUD;     // feature_dim (0: no audio_proj_layer) and the context width, F or 768
    int L = 0;                // fine-tuned encoder layers (0: the encoder is frozen and its output an input)
    float* feat = nullptr;    // L > 0: the batch's conv features (B T, 512)
    unsigned char* mask = nullptr;   // L > 0: the step's time mask (B T)
    long long enc_off = 0, enc_n = 0;   // L > 0: the encoder's tensors in the store
    size_t gpart_n = 0;
    int products = SAID_UT_PRODUCTS_FP32;   // L > 0: the arithmetic of the encoder's dense products (said_unet_train_products.h)
    unsigned* amax = nullptr;               // split products: the partial maxima of a gradient operand, allocated when the mode is first asked for
    EncActs e;
    const std::vector<TDesc>* tb = nullptr;
    hipStream_t s = nullptr;
    TrainStore st;            // the parameters (with the stash of EMAModel.store) and the optimizer's state
    std::map<std::string, long long> off;
    float* rec = nullptr;     // NSCAL + 32
    float *coeffs = nullptr, *noise = nullptr, *tsf = nullptr, *sasb = nullptr, *audio = nullptr;
    int *cond = nullptr, *band = nullptr;
    float* arena = nullptr;
    size_t arena_n = 0;
    float* gpart = nullptr;   // K-split partial tiles
    double* vpart = nullptr;  // vertex partial sums
    float *D = nullptr, *Ev = nullptr;   // vertex loss: deltas (B, 32, 3V) and E (B T, 3V), grown on demand
    size_t D_n = 0, Ev_n = 0;
    std::vector<float> alphas;
    Acts a;
};

namespace {

size_t layout(Acts& a, float* base, int B, int T, int F, int L = 0, EncActs* e = nullptr) {
    size_t pos = 0;
    const size_t M = (size_t)B * T, CTX = F > 0 ? F : AUD;
    auto take = [&](size_t n) { float* p = base ? base + pos : nullptr; pos += (n + 63) / 64 * 64; return p; };
    a.ctx = take(M * CTX); a.noisy = take(M * XC); a.answer = take(M * XC); a.temb = take((size_t)B * CH); a.e1 = take((size_t)B * TEd);
    a.e1s = take((size_t)B * TEd); a.emb = take((size_t)B * TEd); a.embs = take((size_t)B * TEd); a.h0 = take(M * CH);
    a.cat0 = take(M * 2 * CH); a.cat1 = take(M * 2 * CH); a.xho = take(M * CH); a.rso = take((size_t)B * 32); a.ho = take(M * CH); a.pred = take(M * XC);
    for (int i = 0; i < 5; ++i) {
        ResAct& r = a.r[i];
        const size_t ci = kResCin[i];
        r.xh1 = take(M * ci); r.rs1 = take((size_t)B * 32); r.a1 = take(M * ci); r.ee = take((size_t)B * CH); r.c1 = take(M * CH);
        r.xh2 = take(M * CH); r.rs2 = take((size_t)B * 32); r.a2 = take(M * CH); r.out = take(M * CH);
    }
    for (int i = 0; i < 4; ++i) {
        STAct& s = a.s[i];
        float** f[] = {&s.xhg, &s.hn, &s.xh1, &s.y1, &s.q, &s.k, &s.v, &s.o1, &s.x1, &s.xh2, &s.y2, &s.q2, &s.k2, &s.v2, &s.o2, &s.x2, &s.xh3, &s.y3, &s.x3, &s.out};
        for (float** p : f) *p = take(M * CH);
        s.rsg = take((size_t)B * 32); s.rs1 = take(M); s.rs2 = take(M); s.rs3 = take(M);
        s.P1 = take((size_t)B * NH * T * T); s.P2 = take((size_t)B * NH * T * T);
        s.u = take(M * 2 * FF); s.gg = take(M * FF);
    }
    a.d = take(M * CH); a.dcat = take(M * 2 * CH); a.dH0 = take(M * CH); a.dH1 = take(M * CH);
    a.g1 = take(M * 2 * CH); a.g2 = take(M * 2 * CH); a.g3 = take(M * 2 * CH); a.g4 = take(M * CH); a.g5 = take(M * CH);
    a.big1 = take(M * FF); a.big2 = take(M * 2 * FF); a.PB = take((size_t)B * NH * T * T); a.dctx = take(M * CTX);
    a.dee = take((size_t)B * CH); a.dembs = take((size_t)B * TEd); a.demb = take((size_t)B * TEd); a.de1s = take((size_t)B * TEd); a.de1 = take((size_t)B * TEd);
    a.R = take(M * XC); a.dpred = take(M * XC); a.GV = take(M * XC);
    a.proj = a.dcond = nullptr;
    if (F > 0) { a.proj = take(M * F); a.dcond = take(M * F); }
    if (L > 0) {
        if (F <= 0) a.dcond = take(M * CTX);
        const size_t PP = (size_t)B * ENH * T * T, WN = (size_t)EH * EPC * EPK;
        e->xh0 = take(M * ECONV); e->rs0 = take(M); e->y0 = take(M * ECONV); e->hp = take(M * EH); e->h0 = take(M * EH); e->wnorm = take(EPK);
        e->w = take(WN); e->pospre = take(M * EH); e->pos = take(M * EH); e->xhf = take(M * EH); e->rsf = take(M); e->x0 = take(M * EH);
        for (int l = 0; l < L; ++l) {
            EncLayer& z = e->l[l];
            float** f[] = {&z.q, &z.k, &z.v, &z.o, &z.xh1, &z.x1, &z.xh2, &z.out};
            for (float** p : f) *p = take(M * EH);
            z.rs1 = take(M); z.rs2 = take(M); z.P = take(PP); z.u = take(M * EFFN); z.gd = take(M * EFFN);
        }
        e->t768 = take(M * EH); e->Pd = take(PP); e->PB = take(PP); e->d = take(M * EH); e->g1 = take(M * EH); e->g2 = take(M * EH);
        e->g3 = take(M * EH); e->big = take(M * EFFN); e->dw = take(WN); e->wnpart = take((size_t)aft::WN_SEG * EPK); e->wndot = take(EPK);
        e->dy0 = take(M * ECONV);
    }
    return pos;
}

UOp plain(const float* p, int sr, int sc, long long zb = 0, long long zh = 0) { return UOp{p, zb, zh, 0, 1, 0, sr, sc, 0, 1, 1, 0, 0, 0}; }

struct Gm {
    said_unet_train* t;
    int products = SAID_UT_PRODUCTS_FP32;   // of lin / lin_dgrad / lin_wgrad: the encoder's dense products are made with the context's mode
    bool split() const { return products == SAID_UT_PRODUCTS_SPLIT_F16; }
    eg::EncGemm split_base(int layout, const float* a, int lda, const float* b, int ldb, float* c, int ldc, int M, int N, int K) const {
        eg::EncGemm g{};
        g.layout = layout; g.a = a; g.lda = lda; g.b = b; g.ldb = ldb; g.c = c; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.KS = 1; g.kchunk = M;
        g.part = t->gpart; g.amax = t->amax;
        return g;
    }
    UGemm base(UOp A, UOp B, float* C, int ldc, int M, int N, int K) const {
        UGemm g{};
        g.A = A; g.B = B; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.Z = 1; g.ZH = 1; g.alpha = 1.f; g.rbT = 1; g.KS = 1; g.kchunk = ut_unsplit(K).kchunk;
        g.part = t->gpart;
        return g;
    }
    void ksplit(UGemm& g) const {   // the weight gradients: few tiles, long K
        const UtSplit p = ut_ksplit(g.K, g.M, g.N, g.Z, t->gpart_n);
        g.KS = p.KS; g.kchunk = p.kchunk;
    }
    // y (M, N) = x (M, K; ldx) W^T (W: N x K) + bias (+ rowb) (+ res)
    void lin(const float* x, int ldx, const float* W, const float* bias, float* y, int ldy, int M, int N, int K, const float* res = nullptr, int ldr = 0,
             int accumulate = 0) const {
        if (split()) {
            eg::EncGemm e = split_base(eg::EG_FWD, x, ldx, W, K, y, ldy, M, N, K);
            e.bias = bias; e.res = res; e.ldr = ldr; e.accumulate = accumulate;
            return eg::enc_gemm(t->s, e);
        }
        UGemm g = base(plain(x, ldx, 1), plain(W, K, 1), y, ldy, M, N, K);
        g.bias = bias; g.res = res; g.ldr = ldr; g.accumulate = accumulate;
        gemm(t->s, g);
    }
    // dx (M, K; lddx) (+)= dy (M, N) W
    void lin_dgrad(const float* dy, const float* W, float* dx, int lddx, int M, int N, int K, int accumulate) const {
        if (split()) {
            eg::EncGemm e = split_base(eg::EG_DGRAD, dy, N, W, K, dx, lddx, M, N, K);
            e.accumulate = accumulate;
            return eg::enc_gemm(t->s, e);
        }
        UGemm g = base(plain(dy, N, 1), plain(W, 1, K), dx, lddx, M, K, N);
        g.accumulate = accumulate;
        gemm(t->s, g);
    }
    // dW (N, K) = dy^T (rows x N) x (rows x K; ldx); dbias = column sums of dy
    void lin_wgrad(const float* dy, const float* x, int ldx, float* dW, float* dbias, int rows, int N, int K) const {
        if (split()) {
            eg::EncGemm e = split_base(eg::EG_WGRAD, dy, N, x, ldx, dW, K, rows, N, K);
            const UtSplit p = ut_ksplit(rows, N, K, 1, t->gpart_n);
            e.KS = p.KS; e.kchunk = p.kchunk;
            eg::enc_gemm(t->s, e);
        } else {
            UGemm g = base(plain(dy, 1, N), plain(x, 1, ldx), dW, K, N, K, rows);
            ksplit(g);
            gemm(t->s, g);
        }
        if (dbias) colsum(t->s, dy, N, nullptr, 0, rows, 1, N, dbias, 0);
    }
    // Conv1d(k = 3, padding 1) over (B, T): y (M, Co) = sum_j x[t + j - 1] W[:, :, j]^T
    void conv(const float* x, int ldx, int Ci, const float* W, const float* bias, float* y, int Co, int B, int T, const float* rowb = nullptr,
              const float* res = nullptr, int ldr = 0, int accumulate = 0) const {
        UOp A{x, 0, 0, 0, T, ldx, 0, 1, 0, Ci, 3, 0, -1, 1};
        UOp Bw{W, 0, 0, 0, 1, 0, Ci * 3, 3, 1, Ci, 3, 0, 0, 0};
        UGemm g = base(A, Bw, y, Co, B * T, Co, 3 * Ci);
        g.bias = bias; g.rowb = rowb; g.rbT = T; g.res = res; g.ldr = ldr; g.accumulate = accumulate;
        gemm(t->s, g);
    }
    void conv_dgrad(const float* dy, int Co, const float* W, float* dx, int Ci, int B, int T) const {
        UOp A{dy, 0, 0, 0, T, Co, 0, 1, 0, Co, 3, 0, 1, -1};
        UOp Bw{W, 0, 0, 0, 1, 0, 3, Ci * 3, 1, Co, 3, 0, 0, 0};
        gemm(t->s, base(A, Bw, dx, Ci, B * T, Ci, 3 * Co));
    }
    void conv_wgrad(const float* dy, int Co, const float* x, int ldx, int Ci, float* dW, float* dbias, int B, int T) const {
        UOp Bx{x, 0, 0, 1, T, ldx, 0, 1, 0, Ci, 3, 1, -1, 1};
        UGemm g = base(plain(dy, 1, Co), Bx, dW, Ci * 3, Co, Ci * 3, B * T);
        ksplit(g);
        gemm(t->s, g);
        colsum(t->s, dy, Co, nullptr, 0, B * T, 1, Co, dbias, 0);
    }
    // per (sample, head): C (Mz x Nz) = A B^T with the operands' (row, k) strides; activations (B T, 192) hold head h in columns 32 h ..
    void heads(UOp A, UOp B, float* C, long long czb, long long czh, int ldc, int Bn, int M, int N, int K) const {
        UGemm g = base(A, B, C, ldc, M, N, K);
        g.Z = Bn * NH; g.ZH = NH; g.czb = czb; g.czh = czh;
        gemm(t->s, g);
    }
};

UOp act_rows(const float* p, int T) { return plain(p, CH, 1, (long long)T * CH, 32); }     // (t, d) of head h
UOp act_cols(const float* p, int T) { return plain(p, 1, CH, (long long)T * CH, 32); }     // (d, t)
UOp prob_rows(const float* p, int T) { return plain(p, T, 1, (long long)NH * T * T, (long long)T * T); }   // (i, j)
UOp prob_cols(const float* p, int T) { return plain(p, 1, T, (long long)NH * T * T, (long long)T * T); }   // (j, i)

float* par(said_unet_train* t, const float* base, const std::string& name) { return const_cast<float*>(base) + t->off.at(name); }

// the forward; base = P or E; p: dropout probability (0: none); `noisy` already holds the model input
void enqueue_forward(said_unet_train* t, int B, int T, const float* base, float p, unsigned long long seed) {
    hipStream_t s = t->s;
    Acts& a = t->a;
    const Gm gm{t};
    const int M = B * T;
    auto w = [&](const std::string& n) { return par(t, base, n); };
    const std::string m = "denoiser.model.";
    const int CTX = t->CTX;
    const float* audio = t->L > 0 ? t->e.out : t->audio;   // the fine-tuned encoder's output of this call (enqueue_enc_forward), or the input
    if (t->F > 0) {
        // get_audio_embedding projects, then the trainer selects (script/train.py:86-94)
        gm.lin(audio, AUD, w("audio_proj_layer.weight"), w("audio_proj_layer.bias"), a.proj, CTX, M, CTX, AUD);
        select_ctx(s, B, T, CTX, a.proj, w("null_cond_emb"), t->cond, a.ctx);
    } else {
        select_ctx(s, B, T, CTX, audio, w("null_cond_emb"), t->cond, a.ctx);
    }
    timestep_embedding(s, B, CH, t->tsf, a.temb);
    gm.lin(a.temb, CH, w(m + "time_embed.0.weight"), w(m + "time_embed.0.bias"), a.e1, TEd, B, TEd, CH);
    silu_fwd(s, (long long)B * TEd, a.e1, a.e1s);
    gm.lin(a.e1s, TEd, w(m + "time_embed.2.weight"), w(m + "time_embed.2.bias"), a.emb, TEd, B, TEd, TEd);
    silu_fwd(s, (long long)B * TEd, a.emb, a.embs);
    gm.conv(a.noisy, XC, XC, w(m + "input_blocks.0.0.weight"), w(m + "input_blocks.0.0.bias"), a.h0, CH, B, T);

    auto res = [&](int i, const float* x, int ldx, float* out_override, int ldo) {
        ResAct& r = a.r[i];
        const std::string q = kRes[i];
        const int ci = kResCin[i];
        r.x = x; r.ldx = ldx;
        float* out = out_override ? out_override : r.out;
        const int lo = out_override ? ldo : CH;
        gn_fwd(s, B, T, ci, x, ldx, w(q + ".in_layers.0.weight"), w(q + ".in_layers.0.bias"), 1e-5f, 1, 0.f, 0, 0, r.xh1, r.rs1, r.a1);
        gm.lin(a.embs, TEd, w(q + ".emb_layers.1.weight"), w(q + ".emb_layers.1.bias"), r.ee, CH, B, CH, TEd);
        gm.conv(r.a1, ci, ci, w(q + ".in_layers.2.weight"), w(q + ".in_layers.2.bias"), r.c1, CH, B, T, r.ee);
        gn_fwd(s, B, T, CH, r.c1, CH, w(q + ".out_layers.0.weight"), w(q + ".out_layers.0.bias"), 1e-5f, 1, p, seed, i, r.xh2, r.rs2, r.a2);
        if (ci != CH) {
            gm.lin(x, ldx, w(q + ".skip_connection.weight"), w(q + ".skip_connection.bias"), r.out, CH, M, CH, ci);
            gm.conv(r.a2, CH, CH, w(q + ".out_layers.3.weight"), w(q + ".out_layers.3.bias"), r.out, CH, B, T, nullptr, nullptr, 0, 1);
        } else {
            // the convolution's GEMM epilogue writes element (m, n) at m ldc + n: a strided destination is a copy afterwards
            gm.conv(r.a2, CH, CH, w(q + ".out_layers.3.weight"), w(q + ".out_layers.3.bias"), r.out, CH, B, T, nullptr, x, ldx, 0);
        }
        if (out_override) copy2d(s, M, CH, r.out, CH, out, lo, 0);
        return r.out;
    };
    auto st = [&](int i, const float* x, float* out_override, int ldo) {
        STAct& z = a.s[i];
        const std::string q = kST[i], b = q + ".transformer_blocks.0";
        z.x = x;
        const float scale = 0.17677669529663687f;   // 32^-0.5
        gn_fwd(s, B, T, CH, x, CH, w(q + ".norm.weight"), w(q + ".norm.bias"), 1e-6f, 0, 0.f, 0, 0, z.xhg, z.rsg, z.hn);
        ln_fwd(s, M, z.hn, w(b + ".norm1.weight"), w(b + ".norm1.bias"), z.xh1, z.rs1, z.y1);
        gm.lin(z.y1, CH, w(b + ".attn1.to_q.weight"), nullptr, z.q, CH, M, CH, CH);
        gm.lin(z.y1, CH, w(b + ".attn1.to_k.weight"), nullptr, z.k, CH, M, CH, CH);
        gm.lin(z.y1, CH, w(b + ".attn1.to_v.weight"), nullptr, z.v, CH, M, CH, CH);
        gm.heads(act_rows(z.q, T), act_rows(z.k, T), z.P1, (long long)NH * T * T, (long long)T * T, T, B, T, T, 32);
        softmax_fwd(s, (long long)B * NH * T, T, T, scale, nullptr, nullptr, z.P1);
        gm.heads(prob_rows(z.P1, T), act_cols(z.v, T), z.o1, (long long)T * CH, 32, CH, B, T, 32, T);
        gm.lin(z.o1, CH, w(b + ".attn1.to_out.0.weight"), w(b + ".attn1.to_out.0.bias"), z.x1, CH, M, CH, CH, z.hn, CH);
        ln_fwd(s, M, z.x1, w(b + ".norm2.weight"), w(b + ".norm2.bias"), z.xh2, z.rs2, z.y2);
        gm.lin(z.y2, CH, w(b + ".attn2.to_q.weight"), nullptr, z.q2, CH, M, CH, CH);
        gm.lin(a.ctx, CTX, w(b + ".attn2.to_k.weight"), nullptr, z.k2, CH, M, CH, CTX);
        gm.lin(a.ctx, CTX, w(b + ".attn2.to_v.weight"), nullptr, z.v2, CH, M, CH, CTX);
        gm.heads(act_rows(z.q2, T), act_rows(z.k2, T), z.P2, (long long)NH * T * T, (long long)T * T, T, B, T, T, 32);
        softmax_fwd(s, (long long)B * NH * T, T, T, scale, t->band, t->band + t->maxT, z.P2);
        gm.heads(prob_rows(z.P2, T), act_cols(z.v2, T), z.o2, (long long)T * CH, 32, CH, B, T, 32, T);
        gm.lin(z.o2, CH, w(b + ".attn2.to_out.0.weight"), w(b + ".attn2.to_out.0.bias"), z.x2, CH, M, CH, CH, z.x1, CH);
        ln_fwd(s, M, z.x2, w(b + ".norm3.weight"), w(b + ".norm3.bias"), z.xh3, z.rs3, z.y3);
        gm.lin(z.y3, CH, w(b + ".ff.net.0.proj.weight"), w(b + ".ff.net.0.proj.bias"), z.u, 2 * FF, M, 2 * FF, CH);
        geglu_fwd(s, M, FF, z.u, z.gg);
        gm.lin(z.gg, FF, w(b + ".ff.net.2.weight"), w(b + ".ff.net.2.bias"), z.x3, CH, M, CH, FF, z.x2, CH);
        gm.lin(z.x3, CH, w(q + ".proj_out.weight"), w(q + ".proj_out.bias"), z.out, CH, M, CH, CH, x, CH);
        if (out_override) copy2d(s, M, CH, z.out, CH, out_override, ldo, 0);
        return z.out;
    };
    // torch.cat([h, skip], dim = channels): cat0 = [r3 | s1], cat1 = [s3 | h0]
    const float* r1 = res(0, a.h0, CH, nullptr, 0);
    const float* s1 = st(0, r1, a.cat0 + CH, 2 * CH);
    const float* r2 = res(1, s1, CH, nullptr, 0);
    const float* s2 = st(1, r2, nullptr, 0);
    res(2, s2, CH, a.cat0, 2 * CH);
    copy2d(s, M, CH, a.h0, CH, a.cat1 + CH, 2 * CH, 0);
    const float* r4 = res(3, a.cat0, 2 * CH, nullptr, 0);
    st(2, r4, a.cat1, 2 * CH);
    const float* r5 = res(4, a.cat1, 2 * CH, nullptr, 0);
    const float* s4 = st(3, r5, nullptr, 0);
    gn_fwd(s, B, T, CH, s4, CH, w(m + "out.0.weight"), w(m + "out.0.bias"), 1e-5f, 1, 0.f, 0, 0, a.xho, a.rso, a.ho);
    gm.conv(a.ho, CH, CH, w(m + "out.2.weight"), w(m + "out.2.bias"), a.pred, XC, B, T);
}

// losses of a.pred against a.answer; with_grad: a.dpred = d total / d pred.  V > 0: the vertex term on t->D
void enqueue_loss(said_unet_train* t, int B, int T, int V, bool with_grad, double* acc) {
    hipStream_t s = t->s;
    Acts& a = t->a;
    const Gm gm{t};
    const int M = B * T, n = M * XC, V3 = 3 * V;
    loss_residual(s, n, a.pred, a.answer, t->rec, a.R);
    if (V > 0) {
        // E[b] (T, 3V) = R[b] (T, 32) D[b] (32, 3V); GV[b] = sign(E[b]) D[b]^T
        UGemm g = gm.base(plain(a.R, XC, 1, (long long)T * XC, 0), plain(t->D, 1, V3, (long long)XC * V3, 0), t->Ev, V3, T, V3, XC);
        g.Z = B; g.czb = (long long)T * V3;
        gemm(s, g);
        vertex_abs(s, (long long)M * V3, t->Ev, t->vpart, VBLK);
        if (with_grad) {
            UGemm h = gm.base(plain(t->Ev, V3, 1, (long long)T * V3, 0), plain(t->D, V3, 1, (long long)XC * V3, 0), a.GV, XC, T, XC, V3);
            h.Z = B; h.czb = (long long)T * XC;
            gemm(s, h);
        }
    }
    loss_final(s, B, T, a.R, V > 0 ? (with_grad ? a.GV : a.R) : nullptr, t->vpart, VBLK, (long long)M * V3, t->rec, with_grad ? a.dpred : nullptr, t->st.last, acc);
}

// the caller has zeroed a.dembs and a.dctx (accumulated into below)
void enqueue_backward(said_unet_train* t, int B, int T, float p, unsigned long long seed) {
    hipStream_t s = t->s;
    Acts& a = t->a;
    const Gm gm{t};
    const int M = B * T;
    const float* P = t->st.P;
    auto w = [&](const std::string& n) { return par(t, P, n); };
    auto gw = [&](const std::string& n) { return par(t, t->st.G, n); };
    const std::string m = "denoiser.model.";
    const float scale = 0.17677669529663687f;
    const int CTX = t->CTX;
    // norm gradients: dgamma = sum du xhat, dbeta = sum du over the rows
    auto norm_grads = [&](const float* du, const float* xh, int C, const std::string& name) {
        colsum(s, du, C, xh, C, M, 1, C, gw(name + ".weight"), 0);
        colsum(s, du, C, nullptr, 0, M, 1, C, gw(name + ".bias"), 0);
    };
    // ResBlock: dout (M, 192) -> dx (M, cin).  cin = 192: in place in `d`; cin = 384: into a.dcat
    auto res_bwd = [&](int i, float* d) {
        ResAct& r = a.r[i];
        const std::string q = kRes[i];
        const int ci = kResCin[i];
        gm.conv_wgrad(d, CH, r.a2, CH, CH, gw(q + ".out_layers.3.weight"), gw(q + ".out_layers.3.bias"), B, T);
        gm.conv_dgrad(d, CH, w(q + ".out_layers.3.weight"), a.g1, CH, B, T);
        gn_bwd(s, B, T, CH, a.g1, r.xh2, r.rs2, w(q + ".out_layers.0.weight"), w(q + ".out_layers.0.bias"), 1, p, seed, i, a.g2, a.g3, CH, 0);
        norm_grads(a.g2, r.xh2, CH, q + ".out_layers.0");
        // g3 = d c1: the embedding row's gradient is its sum over the sample's frames
        colsum(s, a.g3, CH, nullptr, 0, T, B, CH, a.dee, 0);
        gm.lin_wgrad(a.dee, a.embs, TEd, gw(q + ".emb_layers.1.weight"), gw(q + ".emb_layers.1.bias"), B, CH, TEd);
        gm.lin_dgrad(a.dee, w(q + ".emb_layers.1.weight"), a.dembs, TEd, B, CH, TEd, 1);
        gm.conv_wgrad(a.g3, CH, r.a1, ci, ci, gw(q + ".in_layers.2.weight"), gw(q + ".in_layers.2.bias"), B, T);
        gm.conv_dgrad(a.g3, CH, w(q + ".in_layers.2.weight"), a.g1, ci, B, T);
        float* dx = d;
        if (ci != CH) {
            dx = a.dcat;
            gm.lin_wgrad(d, r.x, r.ldx, gw(q + ".skip_connection.weight"), gw(q + ".skip_connection.bias"), M, CH, ci);
            gm.lin_dgrad(d, w(q + ".skip_connection.weight"), dx, ci, M, CH, ci, 0);
        }
        gn_bwd(s, B, T, ci, a.g1, r.xh1, r.rs1, w(q + ".in_layers.0.weight"), w(q + ".in_layers.0.bias"), 1, 0.f, 0, 0, a.g2, dx, ci, 1);
        norm_grads(a.g2, r.xh1, ci, q + ".in_layers.0");
    };
    // SpatialTransformer, in place in d (M, 192)
    auto st_bwd = [&](int i, float* d) {
        STAct& z = a.s[i];
        const std::string q = kST[i], b = q + ".transformer_blocks.0";
        gm.lin_wgrad(d, z.x3, CH, gw(q + ".proj_out.weight"), gw(q + ".proj_out.bias"), M, CH, CH);
        gm.lin_dgrad(d, w(q + ".proj_out.weight"), a.g1, CH, M, CH, CH, 0);                       // g1 = d x3
        gm.lin_wgrad(a.g1, z.gg, FF, gw(b + ".ff.net.2.weight"), gw(b + ".ff.net.2.bias"), M, CH, FF);
        gm.lin_dgrad(a.g1, w(b + ".ff.net.2.weight"), a.big1, FF, M, CH, FF, 0);
        geglu_bwd(s, M, FF, z.u, a.big1, a.big2);
        gm.lin_wgrad(a.big2, z.y3, CH, gw(b + ".ff.net.0.proj.weight"), gw(b + ".ff.net.0.proj.bias"), M, 2 * FF, CH);
        gm.lin_dgrad(a.big2, w(b + ".ff.net.0.proj.weight"), a.g2, CH, M, 2 * FF, CH, 0);         // g2 = d y3
        norm_grads(a.g2, z.xh3, CH, b + ".norm3");
        ln_bwd(s, M, a.g2, z.xh3, z.rs3, w(b + ".norm3.weight"), a.g1, 1);                        // g1 = d x2
        // attn2
        gm.lin_wgrad(a.g1, z.o2, CH, gw(b + ".attn2.to_out.0.weight"), gw(b + ".attn2.to_out.0.bias"), M, CH, CH);
        gm.lin_dgrad(a.g1, w(b + ".attn2.to_out.0.weight"), a.g2, CH, M, CH, CH, 0);              // g2 = d o2
        gm.heads(act_rows(a.g2, T), act_rows(z.v2, T), a.PB, (long long)NH * T * T, (long long)T * T, T, B, T, T, 32);   // dP = do v^T
        gm.heads(prob_cols(z.P2, T), act_cols(a.g2, T), a.g3, (long long)T * CH, 32, CH, B, T, 32, T);                   // dv = P^T do
        softmax_bwd(s, (long long)B * NH * T, T, scale, z.P2, a.PB);
        gm.heads(prob_rows(a.PB, T), act_cols(z.k2, T), a.g4, (long long)T * CH, 32, CH, B, T, 32, T);                   // dq = dS k
        gm.heads(prob_cols(a.PB, T), act_cols(z.q2, T), a.g5, (long long)T * CH, 32, CH, B, T, 32, T);                   // dk = dS^T q
        gm.lin_wgrad(a.g4, z.y2, CH, gw(b + ".attn2.to_q.weight"), nullptr, M, CH, CH);
        gm.lin_wgrad(a.g5, a.ctx, CTX, gw(b + ".attn2.to_k.weight"), nullptr, M, CH, CTX);
        gm.lin_wgrad(a.g3, a.ctx, CTX, gw(b + ".attn2.to_v.weight"), nullptr, M, CH, CTX);
        gm.lin_dgrad(a.g5, w(b + ".attn2.to_k.weight"), a.dctx, CTX, M, CH, CTX, 1);
        gm.lin_dgrad(a.g3, w(b + ".attn2.to_v.weight"), a.dctx, CTX, M, CH, CTX, 1);
        gm.lin_dgrad(a.g4, w(b + ".attn2.to_q.weight"), a.g2, CH, M, CH, CH, 0);                  // g2 = d y2
        norm_grads(a.g2, z.xh2, CH, b + ".norm2");
        ln_bwd(s, M, a.g2, z.xh2, z.rs2, w(b + ".norm2.weight"), a.g1, 1);                        // g1 = d x1
        // attn1
        gm.lin_wgrad(a.g1, z.o1, CH, gw(b + ".attn1.to_out.0.weight"), gw(b + ".attn1.to_out.0.bias"), M, CH, CH);
        gm.lin_dgrad(a.g1, w(b + ".attn1.to_out.0.weight"), a.g2, CH, M, CH, CH, 0);
        gm.heads(act_rows(a.g2, T), act_rows(z.v, T), a.PB, (long long)NH * T * T, (long long)T * T, T, B, T, T, 32);
        gm.heads(prob_cols(z.P1, T), act_cols(a.g2, T), a.g3, (long long)T * CH, 32, CH, B, T, 32, T);
        softmax_bwd(s, (long long)B * NH * T, T, scale, z.P1, a.PB);
        gm.heads(prob_rows(a.PB, T), act_cols(z.k, T), a.g4, (long long)T * CH, 32, CH, B, T, 32, T);
        gm.heads(prob_cols(a.PB, T), act_cols(z.q, T), a.g5, (long long)T * CH, 32, CH, B, T, 32, T);
        gm.lin_wgrad(a.g4, z.y1, CH, gw(b + ".attn1.to_q.weight"), nullptr, M, CH, CH);
        gm.lin_wgrad(a.g5, z.y1, CH, gw(b + ".attn1.to_k.weight"), nullptr, M, CH, CH);
        gm.lin_wgrad(a.g3, z.y1, CH, gw(b + ".attn1.to_v.weight"), nullptr, M, CH, CH);
        gm.lin_dgrad(a.g4, w(b + ".attn1.to_q.weight"), a.g2, CH, M, CH, CH, 0);
        gm.lin_dgrad(a.g5, w(b + ".attn1.to_k.weight"), a.g2, CH, M, CH, CH, 1);
        gm.lin_dgrad(a.g3, w(b + ".attn1.to_v.weight"), a.g2, CH, M, CH, CH, 1);                  // g2 = d y1
        norm_grads(a.g2, z.xh1, CH, b + ".norm1");
        ln_bwd(s, M, a.g2, z.xh1, z.rs1, w(b + ".norm1.weight"), a.g1, 1);                        // g1 = d hn
        gn_bwd(s, B, T, CH, a.g1, z.xhg, z.rsg, w(q + ".norm.weight"), w(q + ".norm.bias"), 0, 0.f, 0, 0, a.g2, d, CH, 1);
        norm_grads(a.g2, z.xhg, CH, q + ".norm");
    };

    gm.conv_wgrad(a.dpred, XC, a.ho, CH, CH, gw(m + "out.2.weight"), gw(m + "out.2.bias"), B, T);
    gm.conv_dgrad(a.dpred, XC, w(m + "out.2.weight"), a.g1, CH, B, T);
    gn_bwd(s, B, T, CH, a.g1, a.xho, a.rso, w(m + "out.0.weight"), w(m + "out.0.bias"), 1, 0.f, 0, 0, a.g2, a.d, CH, 0);
    norm_grads(a.g2, a.xho, CH, m + "out.0");
    st_bwd(3, a.d);
    res_bwd(4, a.d);                                           // dcat = d [s3 | h0]
    copy2d(s, M, CH, a.dcat, 2 * CH, a.d, CH, 0);
    copy2d(s, M, CH, a.dcat + CH, 2 * CH, a.dH0, CH, 0);
    st_bwd(2, a.d);
    res_bwd(3, a.d);                                           // dcat = d [r3 | s1]
    copy2d(s, M, CH, a.dcat, 2 * CH, a.d, CH, 0);
    copy2d(s, M, CH, a.dcat + CH, 2 * CH, a.dH1, CH, 0);
    res_bwd(2, a.d);
    st_bwd(1, a.d);
    res_bwd(1, a.d);
    copy2d(s, M, CH, a.dH1, CH, a.d, CH, 1);
    st_bwd(0, a.d);
    res_bwd(0, a.d);
    copy2d(s, M, CH, a.dH0, CH, a.d, CH, 1);
    gm.conv_wgrad(a.d, CH, a.noisy, XC, XC, gw(m + "input_blocks.0.0.weight"), gw(m + "input_blocks.0.0.bias"), B, T);
    // the time embedding MLP
    silu_bwd(s, (long long)B * TEd, a.emb, a.dembs, a.demb);
    gm.lin_wgrad(a.demb, a.e1s, TEd, gw(m + "time_embed.2.weight"), gw(m + "time_embed.2.bias"), B, TEd, TEd);
    gm.lin_dgrad(a.demb, w(m + "time_embed.2.weight"), a.de1s, TEd, B, TEd, TEd, 0);
    silu_bwd(s, (long long)B * TEd, a.e1, a.de1s, a.de1);
    gm.lin_wgrad(a.de1, a.temb, CH, gw(m + "time_embed.0.weight"), gw(m + "time_embed.0.bias"), B, TEd, CH);
    // null_cond_emb: the context gradient summed over the unconditional samples' positions
    if (t->F > 0) {
        // the conditional samples' rows go to the projection (nothing flows into the frozen encoder's output)
        split_cond_rows(s, B, T, CTX, t->cond, a.dctx, a.dcond);
        colsum(s, a.dctx, CTX, nullptr, 0, M, 1, CTX, gw("null_cond_emb"), 0);
        gm.lin_wgrad(a.dcond, t->L > 0 ? t->e.out : t->audio, AUD, gw("audio_proj_layer.weight"), gw("audio_proj_layer.bias"), M, CTX, AUD);
    } else if (t->L > 0) {
        // the conditional samples' rows are the gradient at the fine-tuned encoder's output (enqueue_enc_backward)
        split_cond_rows(s, B, T, CTX, t->cond, a.dctx, a.dcond);
        colsum(s, a.dctx, CTX, nullptr, 0, M, 1, CTX, gw("null_cond_emb"), 0);
    } else {
        mask_cond_rows(s, B, T, CTX, t->cond, a.dctx);
        colsum(s, a.dctx, CTX, nullptr, 0, M, 1, CTX, gw("null_cond_emb"), 0);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the fine-tuned encoder
// The Wav2Vec2 transformer behind the frozen feature extractor (include/said_unet_train.h), fp32 token-major.  tp == nullptr: eval mode.
struct EncGm {
    said_unet_train* t;
    int B, T;
    UOp rows(const float* p) const { return plain(p, EH, 1, (long long)T * EH, EHD); }     // (t, d) of head h
    UOp cols(const float* p) const { return plain(p, 1, EH, (long long)T * EH, EHD); }     // (d, t)
    UOp prow(const float* p) const { return plain(p, T, 1, (long long)ENH * T * T, (long long)T * T); }
    UOp pcol(const float* p) const { return plain(p, 1, T, (long long)ENH * T * T, (long long)T * T); }
    void heads(UOp A, UOp Bo, float* C, long long czb, long long czh, int ldc, int M, int N, int K) const {
        UGemm g = Gm{t}.base(A, Bo, C, ldc, M, N, K);
        g.Z = B * ENH; g.ZH = ENH; g.czb = czb; g.czh = czh;
        gemm(t->s, g);
    }
    void scores(const float* q, const float* k, float* S) const { heads(rows(q), rows(k), S, (long long)ENH * T * T, (long long)T * T, T, T, T, EHD); }
    void apply(UOp Pm, const float* v, float* o) const { heads(Pm, cols(v), o, (long long)T * EH, EHD, EH, T, EHD, T); }
    // the grouped positional convolution (k = 128, padding 64, the last output dropped) as shifted-operand GEMMs, the group as batch index;
    // a short batch splits K = 128 x 48 so that more than 16 workgroups run
    void split_small(UGemm& g) const {
        const UtSplit p = ut_split_small(g.K, g.M, g.N, g.Z, t->gpart_n);
        g.KS = p.KS; g.kchunk = p.kchunk;
    }
    void pos_fwd(const float* h, const float* w, float* y) const {   // without the bias: the epilogue's bias[n] counts columns inside a group
        UOp A{h, 0, EPC, 0, T, EH, 0, 1, 0, EPC, EPK, 0, -EPK / 2, 1};
        UOp W{w, 0, (long long)EPC * EPC * EPK, 0, 1, 0, EPC * EPK, EPK, 1, EPC, EPK, 0, 0, 0};
        UGemm g = Gm{t}.base(A, W, y, EH, B * T, EPC, EPK * EPC);
        g.Z = EPG; g.ZH = EPG; g.czh = EPC;
        split_small(g);
        gemm(t->s, g);
    }
    void pos_dgrad(const float* dy, const float* w, float* dh) const {   // dh += ...
        UOp A{dy, 0, EPC, 0, T, EH, 0, 1, 0, EPC, EPK, 0, EPK / 2, -1};
        UOp W{w, 0, (long long)EPC * EPC * EPK, 0, 1, 0, EPK, EPC * EPK, 1, EPC, EPK, 0, 0, 0};
        UGemm g = Gm{t}.base(A, W, dh, EH, B * T, EPC, EPK * EPC);
        g.Z = EPG; g.ZH = EPG; g.czh = EPC; g.accumulate = 1;
        split_small(g);
        gemm(t->s, g);
    }
    void pos_wgrad(const float* dy, const float* h, float* dw) const {   // dw (768, 48, 128)
        UOp A = plain(dy, 1, EH, 0, EPC);
        UOp X{h, 0, EPC, 1, T, EH, 0, 1, 0, EPC, EPK, 1, -EPK / 2, 1};
        UGemm g = Gm{t}.base(A, X, dw, EPC * EPK, EPC, EPC * EPK, B * T);
        g.Z = EPG; g.ZH = EPG; g.czh = (long long)EPC * EPC * EPK;
        Gm{t}.ksplit(g);
        gemm(t->s, g);
    }
};

void enqueue_enc_forward(said_unet_train* t, int B, int T, const float* base, const said_audio_train_params* tp) {
    hipStream_t s = t->s;
    EncActs& e = t->e;
    const Gm gm{t, t->products};
    const EncGm eg{t, B, T};
    const int M = B * T;
    auto w = [&](const std::string& n) { return par(t, base, kEnc + n); };
    auto site = [&](int id, float p) { return aft::drop(tp ? tp->seed : 0, id, tp ? p : 0.f); };
    const aft::Drop none = aft::drop(0, 0, 0.f);
    const unsigned char* mask = (tp && tp->time_mask_dev) ? t->mask : nullptr;
    aft::ln_fwd(s, M, ECONV, t->feat, nullptr, w("feature_projection.layer_norm.weight"), w("feature_projection.layer_norm.bias"), none, none, e.xh0,
                e.rs0, e.y0);
    gm.lin(e.y0, ECONV, w("feature_projection.projection.weight"), w("feature_projection.projection.bias"), e.hp, EH, M, EH, ECONV);
    aft::mask_drop_fwd(s, M, EH, e.hp, mask, w("masked_spec_embed"), site(0, tp ? tp->p_feat_proj : 0.f), e.h0);
    aft::weight_norm_fwd(s, EH * EPC, EPK, w("encoder.pos_conv_embed.conv.weight_g"), w("encoder.pos_conv_embed.conv.weight_v"), e.wnpart, e.wnorm, e.w);
    eg.pos_fwd(e.h0, e.w, e.pospre);
    aft::add_bias(s, M, EH, w("encoder.pos_conv_embed.conv.bias"), e.pospre);
    aft::gelu_drop_fwd(s, (long long)M * EH, e.pospre, none, e.pos);
    aft::ln_fwd(s, M, EH, e.pos, e.h0, w("encoder.layer_norm.weight"), w("encoder.layer_norm.bias"), none, site(1, tp ? tp->p_hidden : 0.f), e.xhf, e.rsf,
                e.x0);
    const float* x = e.x0;
    for (int l = 0; l < t->L; ++l) {
        if (tp && (tp->skip_layers >> l & 1u)) continue;   // LayerDrop: the layer is the identity for the whole batch
        EncLayer& z = e.l[l];
        const std::string p = "encoder.layers." + std::to_string(l);
        z.x = x;
        gm.lin(x, EH, w(p + ".attention.q_proj.weight"), w(p + ".attention.q_proj.bias"), z.q, EH, M, EH, EH);
        gm.lin(x, EH, w(p + ".attention.k_proj.weight"), w(p + ".attention.k_proj.bias"), z.k, EH, M, EH, EH);
        gm.lin(x, EH, w(p + ".attention.v_proj.weight"), w(p + ".attention.v_proj.bias"), z.v, EH, M, EH, EH);
        eg.scores(z.q, z.k, z.P);
        softmax_fwd(s, (long long)B * ENH * T, T, T, 0.125f, nullptr, nullptr, z.P);
        const aft::Drop pd = site(16 + 4 * l, tp ? tp->p_attention : 0.f);
        const float* Pd = z.P;   // the denominator summed the undropped terms; the mask goes on the normalised probabilities
        if (pd.p > 0.f) { aft::prob_drop(s, (long long)B * ENH * T, T, z.P, pd, e.Pd); Pd = e.Pd; }
        eg.apply(eg.prow(Pd), z.v, z.o);
        gm.lin(z.o, EH, w(p + ".attention.out_proj.weight"), w(p + ".attention.out_proj.bias"), e.t768, EH, M, EH, EH);
        aft::ln_fwd(s, M, EH, e.t768, x, w(p + ".layer_norm.weight"), w(p + ".layer_norm.bias"), site(16 + 4 * l + 1, tp ? tp->p_hidden : 0.f), none, z.xh1,
                    z.rs1, z.x1);
        gm.lin(z.x1, EH, w(p + ".feed_forward.intermediate_dense.weight"), w(p + ".feed_forward.intermediate_dense.bias"), z.u, EFFN, M, EFFN, EH);
        aft::gelu_drop_fwd(s, (long long)M * EFFN, z.u, site(16 + 4 * l + 2, tp ? tp->p_activation : 0.f), z.gd);
        gm.lin(z.gd, EFFN, w(p + ".feed_forward.output_dense.weight"), w(p + ".feed_forward.output_dense.bias"), e.t768, EH, M, EH, EFFN);
        aft::ln_fwd(s, M, EH, e.t768, z.x1, w(p + ".final_layer_norm.weight"), w(p + ".final_layer_norm.bias"), site(16 + 4 * l + 3, tp ? tp->p_hidden : 0.f),
                    none, z.xh2, z.rs2, z.out);
        x = z.out;
    }
    e.out = x;
}

// dE (B T, 768): the gradient at the encoder's output, exact zeros in the unconditional samples' rows; it is overwritten.  The caller has
// zeroed the encoder's gradients: a skipped layer's, and masked_spec_embed's without a mask, stay exact zeros.
void enqueue_enc_backward(said_unet_train* t, int B, int T, const said_audio_train_params* tp, float* dE) {
    hipStream_t s = t->s;
    EncActs& e = t->e;
    const Gm gm{t, t->products};
    const EncGm eg{t, B, T};
    const int M = B * T;
    const float* P = t->st.P;
    auto w = [&](const std::string& n) { return par(t, P, kEnc + n); };
    auto gw = [&](const std::string& n) { return par(t, t->st.G, kEnc + n); };
    auto site = [&](int id, float p) { return aft::drop(tp ? tp->seed : 0, id, tp ? p : 0.f); };
    const aft::Drop none = aft::drop(0, 0, 0.f);
    const unsigned char* mask = (tp && tp->time_mask_dev) ? t->mask : nullptr;
    auto norm_grads = [&](const float* du, const float* xh, int C, const std::string& name) {
        colsum(s, du, C, xh, C, M, 1, C, gw(name + ".weight"), 0);
        colsum(s, du, C, nullptr, 0, M, 1, C, gw(name + ".bias"), 0);
    };
    float* d = dE;
    for (int l = t->L - 1; l >= 0; --l) {
        if (tp && (tp->skip_layers >> l & 1u)) continue;
        EncLayer& z = e.l[l];
        const std::string p = "encoder.layers." + std::to_string(l);
        // final_layer_norm over x1 + dropout(f): g1 = d x1 (so far), g2 = d f
        norm_grads(d, z.xh2, EH, p + ".final_layer_norm");
        aft::ln_bwd(s, M, EH, d, z.xh2, z.rs2, w(p + ".final_layer_norm.weight"), site(16 + 4 * l + 3, tp ? tp->p_hidden : 0.f), none, nullptr, e.g1, 0, e.g2);
        gm.lin_wgrad(e.g2, z.gd, EFFN, gw(p + ".feed_forward.output_dense.weight"), gw(p + ".feed_forward.output_dense.bias"), M, EH, EFFN);
        gm.lin_dgrad(e.g2, w(p + ".feed_forward.output_dense.weight"), e.big, EFFN, M, EH, EFFN, 0);
        aft::gelu_drop_bwd(s, (long long)M * EFFN, z.u, e.big, site(16 + 4 * l + 2, tp ? tp->p_activation : 0.f), e.big);
        gm.lin_wgrad(e.big, z.x1, EH, gw(p + ".feed_forward.intermediate_dense.weight"), gw(p + ".feed_forward.intermediate_dense.bias"), M, EFFN, EH);
        gm.lin_dgrad(e.big, w(p + ".feed_forward.intermediate_dense.weight"), e.g1, EH, M, EFFN, EH, 1);
        // layer_norm over x + dropout(a): d = d x (so far), g2 = d a
        norm_grads(e.g1, z.xh1, EH, p + ".layer_norm");
        aft::ln_bwd(s, M, EH, e.g1, z.xh1, z.rs1, w(p + ".layer_norm.weight"), site(16 + 4 * l + 1, tp ? tp->p_hidden : 0.f), none, nullptr, d, 0, e.g2);
        gm.lin_wgrad(e.g2, z.o, EH, gw(p + ".attention.out_proj.weight"), gw(p + ".attention.out_proj.bias"), M, EH, EH);
        gm.lin_dgrad(e.g2, w(p + ".attention.out_proj.weight"), e.g3, EH, M, EH, EH, 0);                    // g3 = d o
        const aft::Drop pd = site(16 + 4 * l, tp ? tp->p_attention : 0.f);
        const float* Pd = z.P;
        if (pd.p > 0.f) { aft::prob_drop(s, (long long)B * ENH * T, T, z.P, pd, e.Pd); Pd = e.Pd; }
        eg.scores(e.g3, z.v, e.PB);                                                                           // d Pd = do v^T
        eg.apply(eg.pcol(Pd), e.g3, e.g2);                                                                    // g2 = d v = Pd^T do
        if (pd.p > 0.f) aft::prob_drop(s, (long long)B * ENH * T, T, e.PB, pd, e.PB);                         // d P: masked and scaled
        softmax_bwd(s, (long long)B * ENH * T, T, 0.125f, z.P, e.PB);
        eg.apply(eg.prow(e.PB), z.k, e.g1);                                                                   // g1 = d q = dS k
        eg.apply(eg.pcol(e.PB), z.q, e.g3);                                                                   // g3 = d k = dS^T q
        gm.lin_wgrad(e.g1, z.x, EH, gw(p + ".attention.q_proj.weight"), gw(p + ".attention.q_proj.bias"), M, EH, EH);
        gm.lin_wgrad(e.g3, z.x, EH, gw(p + ".attention.k_proj.weight"), gw(p + ".attention.k_proj.bias"), M, EH, EH);
        gm.lin_wgrad(e.g2, z.x, EH, gw(p + ".attention.v_proj.weight"), gw(p + ".attention.v_proj.bias"), M, EH, EH);
        gm.lin_dgrad(e.g1, w(p + ".attention.q_proj.weight"), d, EH, M, EH, EH, 1);
        gm.lin_dgrad(e.g3, w(p + ".attention.k_proj.weight"), d, EH, M, EH, EH, 1);
        gm.lin_dgrad(e.g2, w(p + ".attention.v_proj.weight"), d, EH, M, EH, EH, 1);
    }
    // the front: x0 = dropout(LN(h0 + gelu(pos_conv(h0)))): g2 = the gradient behind the dropout, g1 = d (h0 + pos)
    aft::ln_bwd(s, M, EH, d, e.xhf, e.rsf, w("encoder.layer_norm.weight"), none, site(1, tp ? tp->p_hidden : 0.f), e.g2, e.g1, 0, nullptr);
    norm_grads(e.g2, e.xhf, EH, "encoder.layer_norm");
    aft::gelu_drop_bwd(s, (long long)M * EH, e.pospre, e.g1, none, e.g3);                                     // g3 = d pos_conv output
    colsum(s, e.g3, EH, nullptr, 0, M, 1, EH, gw("encoder.pos_conv_embed.conv.bias"), 0);
    eg.pos_wgrad(e.g3, e.h0, e.dw);
    aft::weight_norm_bwd(s, EH * EPC, EPK, w("encoder.pos_conv_embed.conv.weight_g"), w("encoder.pos_conv_embed.conv.weight_v"), e.wnorm, e.dw, e.wnpart,
                         e.wndot, gw("encoder.pos_conv_embed.conv.weight_g"), gw("encoder.pos_conv_embed.conv.weight_v"));
    eg.pos_dgrad(e.g3, e.w, e.g1);                                                                            // g1 = d h0
    // masked rows give their gradient to masked_spec_embed and none to the projection
    aft::mask_drop_bwd(s, M, EH, e.g1, mask, site(0, tp ? tp->p_feat_proj : 0.f), e.g2, mask ? e.g3 : nullptr);
    if (mask) colsum(s, e.g3, EH, nullptr, 0, M, 1, EH, gw("masked_spec_embed"), 0);
    gm.lin_wgrad(e.g2, e.y0, ECONV, gw("feature_projection.projection.weight"), gw("feature_projection.projection.bias"), M, EH, ECONV);
    gm.lin_dgrad(e.g2, w("feature_projection.projection.weight"), e.dy0, ECONV, M, EH, ECONV, 0);
    norm_grads(e.dy0, e.xh0, ECONV, "feature_projection.layer_norm");   // nothing flows into the features
}

int put_record(said_unet_train* t, const float* scalars, const float* std_) {
    HostCtx* ctx = &t->c;
    float h[NSCAL + XC] = {};
    if (scalars) memcpy(h, scalars, sizeof(float) * SAID_UT_NSCAL);
    h[S_USE_STD] = std_ ? 1.f : 0.f;
    if (std_) memcpy(h + NSCAL, std_, sizeof(float) * XC);
    HIPCHK(hipMemcpyAsync(t->rec, h, sizeof h, hipMemcpyHostToDevice, t->s));
    HIPCHK(hipStreamSynchronize(t->s));   // h is on the stack
    return 0;
}

// shape checks and the upload of a batch's inputs; x0 / noise may be null (forward_only passes the sample as x0)
int put_inputs(said_unet_train* t, const char* what, int B, int T, const float* x0, const float* noise, const long long* ts, const int* cond,
               const void* audio, int audio_on_device, bool need_alphas, bool ft = false) {
    HostCtx* ctx = &t->c;
    if (ft && t->L <= 0) return fail(ctx, "%s: the context has no fine-tuned encoder (said_unet_train_create_ft with finetune_layers >= 1)", what);
    if (!ft && t->L > 0) return fail(ctx, "%s: the context fine-tunes its encoder and takes conv features: call the _ft entry point", what);
    if (ft && (unsigned long long)B * T * EFFN >= (1ull << 32)) return fail(ctx, "%s: %d windows of %d frames need a dropout index of 2^32 or more", what, B, T);
    if (B < 1 || B > t->maxB) return fail(ctx, "%s: batch %d outside [1, %d] (the context's max_batch)", what, B, t->maxB);
    if (T < 2 || T > t->maxT) return fail(ctx, "%s: %d frames outside [2, %d] (the context's max_frames)", what, T, t->maxT);
    if (!x0 || !ts || !cond || !audio) return fail(ctx, "%s: null input", what);
    const size_t n = (size_t)B * T * XC;
    std::vector<float> tf(B), ab(2 * (size_t)B, 0.f);
    for (int b = 0; b < B; ++b) {
        tf[b] = (float)ts[b];
        if (need_alphas) {
            if (t->alphas.empty()) return fail(ctx, "%s: no alphas_cumprod set (said_unet_train_set_alphas)", what);
            if (ts[b] < 0 || ts[b] >= (long long)t->alphas.size()) return fail(ctx, "%s: timestep %lld outside [0, %zu)", what, ts[b], t->alphas.size());
            const float ac = t->alphas[ts[b]];
            ab[2 * b] = sqrtf(ac);          // diffusers add_noise / get_velocity: alphas_cumprod ** 0.5, (1 - alphas_cumprod) ** 0.5 in float32
            ab[2 * b + 1] = sqrtf(1.f - ac);
        }
    }
    // ldm/attention.py:170-189 with Python's banker's round; the context has one position per frame
    std::vector<int> band(2 * (size_t)t->maxT, 0);
    const double ratio = 1.0, kh = ratio / 2 + 1;   // context length / frames: the audio embedding has one position per frame
    for (int i = 0; i < T; ++i) {
        const double mid = (i + 0.5) * ratio;
        band[i] = std::max((int)std::nearbyint(mid - kh), 0);
        band[t->maxT + i] = std::min((int)std::nearbyint(mid + kh), T);
    }
    HIPCHK(hipMemcpyAsync(t->coeffs, x0, n * sizeof(float), hipMemcpyHostToDevice, t->s));
    if (noise) HIPCHK(hipMemcpyAsync(t->noise, noise, n * sizeof(float), hipMemcpyHostToDevice, t->s));
    HIPCHK(hipMemcpyAsync(t->tsf, tf.data(), B * sizeof(float), hipMemcpyHostToDevice, t->s));
    HIPCHK(hipMemcpyAsync(t->sasb, ab.data(), 2 * B * sizeof(float), hipMemcpyHostToDevice, t->s));
    HIPCHK(hipMemcpyAsync(t->cond, cond, B * sizeof(int), hipMemcpyHostToDevice, t->s));
    HIPCHK(hipMemcpyAsync(t->band, band.data(), band.size() * sizeof(int), hipMemcpyHostToDevice, t->s));
    HIPCHK(hipMemcpyAsync(ft ? t->feat : t->audio, audio, (size_t)B * T * (ft ? ECONV : AUD) * sizeof(float),
                          audio_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, t->s));
    HIPCHK(hipStreamSynchronize(t->s));   // the host vectors above end with this call
    return 0;
}

int put_deltas(said_unet_train* t, const char* what, int B, int T, const float* deltas, int V) {
    HostCtx* ctx = &t->c;
    if (!deltas) return 0;
    if (V < 1 || V > 65536) return fail(ctx, "%s: %d vertices outside [1, 65536]", what, V);
    const size_t dn = (size_t)B * XC * 3 * V, en = (size_t)B * T * 3 * V;
    if (dn > t->D_n) { if (drealloc(ctx, &t->D, dn, false)) return -1; t->D_n = dn; }
    if (en > t->Ev_n) { if (drealloc(ctx, &t->Ev, en, false)) return -1; t->Ev_n = en; }
    HIPCHK(hipMemcpyAsync(t->D, deltas, dn * sizeof(float), hipMemcpyHostToDevice, t->s));
    HIPCHK(hipStreamSynchronize(t->s));
    return 0;
}

int check_std(said_unet_train* t, const float* std_, const char* what) {
    if (!std_) return 0;
    for (int c = 0; c < XC; ++c)
        if (!(std::isfinite(std_[c]) && std_[c] != 0.f)) return fail(&t->c, "%s: std[%d] = %g is not a finite non-zero value", what, c, (double)std_[c]);
    return 0;
}

int tindex(const said_unet_train* t, const char* name) {
    if (!name) return -1;
    const auto& tb = *t->tb;
    for (size_t i = 0; i < tb.size(); ++i)
        if (tb[i].name == name) return (int)i;
    return -1;
}

}  // namespace

extern "C" {

const char* said_unet_train_tensor_name(int i) { return said_unet_train_table_name(0, i); }
long long said_unet_train_tensor_numel(int i) { return said_unet_train_table_numel(0, i); }

int said_unet_train_table_size(int feature_dim) { return said_unet_train_table_size_ft(feature_dim, 0); }
const char* said_unet_train_table_name(int feature_dim, int i) { return said_unet_train_table_name_ft(feature_dim, 0, i); }
long long said_unet_train_table_numel(int feature_dim, int i) { return said_unet_train_table_numel_ft(feature_dim, 0, i); }
int said_unet_train_table_size_ft(int feature_dim, int finetune_layers) {
    return (feature_dim > SAID_UT_MAX_FEATURE_DIM || finetune_layers > SAID_UT_MAX_FINETUNE_LAYERS) ? -1 : (int)table(feature_dim, finetune_layers).size();
}
const char* said_unet_train_table_name_ft(int feature_dim, int finetune_layers, int i) {
    if (feature_dim > SAID_UT_MAX_FEATURE_DIM || finetune_layers > SAID_UT_MAX_FINETUNE_LAYERS) return nullptr;
    const auto& tb = table(feature_dim, finetune_layers);
    return (i >= 0 && i < (int)tb.size()) ? tb[i].name.c_str() : nullptr;
}
long long said_unet_train_table_numel_ft(int feature_dim, int finetune_layers, int i) {
    if (feature_dim > SAID_UT_MAX_FEATURE_DIM || finetune_layers > SAID_UT_MAX_FINETUNE_LAYERS) return -1;
    const auto& tb = table(feature_dim, finetune_layers);
    return (i >= 0 && i < (int)tb.size()) ? tb[i].numel : -1;
}
int said_unet_train_finetune_layers(const said_unet_train* t) { return t ? t->L : -1; }
int said_unet_train_num_tensors(const said_unet_train* t) { return t ? (int)t->tb->size() : -1; }
int said_unet_train_feature_dim(const said_unet_train* t) { return (t && t->F > 0) ? t->F : -1; }
const char* said_unet_train_context_tensor_name(const said_unet_train* t, int i) {
    return (t && i >= 0 && i < (int)t->tb->size()) ? (*t->tb)[i].name.c_str() : nullptr;
}
long long said_unet_train_context_tensor_numel(const said_unet_train* t, int i) {
    return (t && i >= 0 && i < (int)t->tb->size()) ? (*t->tb)[i].numel : -1;
}

int said_unet_train_create(said_unet_train** out, int device, int max_batch, int max_frames) {
    return said_unet_train_create_dim(out, device, max_batch, max_frames, -1);
}

int said_unet_train_create_dim(said_unet_train** out, int device, int max_batch, int max_frames, int feature_dim) {
    return said_unet_train_create_ft(out, device, max_batch, max_frames, feature_dim, 0);
}

int said_unet_train_create_ft(said_unet_train** out, int device, int max_batch, int max_frames, int feature_dim, int finetune_layers) {
    DeviceRestore restore_device;
    static_assert(SAID_UT_MAX_FINETUNE_LAYERS == MAXL, "said_unet_train.h and the encoder's activation table disagree");
    if (finetune_layers > SAID_UT_MAX_FINETUNE_LAYERS)
        return fail(nullptr, "said_unet_train_create_ft: finetune_layers %d above %d (SAID_UT_MAX_FINETUNE_LAYERS)", finetune_layers, SAID_UT_MAX_FINETUNE_LAYERS);
    if (feature_dim > SAID_UT_MAX_FEATURE_DIM)
        return fail(nullptr, "said_unet_train_create_dim: feature_dim %d above %d (SAID_UT_MAX_FEATURE_DIM)", feature_dim, SAID_UT_MAX_FEATURE_DIM);
    said_unet_train* t = new_ctx("said_unet_train_create", out, device);
    if (!t) return -1;
    if (max_batch < 1 || max_batch > 256) { delete t; return fail(nullptr, "said_unet_train_create: max_batch %d outside [1, 256]", max_batch); }
    if (max_frames < 2 || max_frames > 2048) { delete t; return fail(nullptr, "said_unet_train_create: max_frames %d outside [2, 2048]", max_frames); }
    HostCtx* ctx = &t->c;
    t->maxB = max_batch;
    t->maxT = max_frames;
    t->F = feature_dim > 0 ? feature_dim : 0;
    t->CTX = t->F > 0 ? t->F : AUD;
    t->L = finetune_layers > 0 ? finetune_layers : 0;
    t->tb = &table(t->F, t->L);
    const auto& tb = *t->tb;
    std::vector<long long> sizes, off;
    for (const TDesc& d : tb) sizes.push_back(d.numel);
    Acts tmp;
    EncActs etmp;
    t->arena_n = layout(tmp, nullptr, max_batch, max_frames, t->F, t->L, &etmp);
    // K-split partial tiles: the UNet's weight gradients; with a fine-tuned encoder its FFN's and the positional convolution's (768 x 48 x 128)
    t->gpart_n = ut_gpart_n(t->F, t->L);
    const size_t Mx = (size_t)max_batch * max_frames;
    int rc = 0;
    rc = rc || hipStreamCreateWithFlags(&t->s, hipStreamNonBlocking) != hipSuccess;
    rc = rc || dalloc(ctx, &t->rec, NSCAL + XC) || dalloc(ctx, &t->coeffs, Mx * XC) ||
         dalloc(ctx, &t->noise, Mx * XC) || dalloc(ctx, &t->tsf, max_batch) || dalloc(ctx, &t->sasb, (size_t)2 * max_batch) ||
         dalloc(ctx, &t->audio, Mx * AUD) || dalloc(ctx, &t->cond, max_batch) || dalloc(ctx, &t->band, (size_t)2 * max_frames) ||
         dalloc(ctx, &t->arena, t->arena_n) || dalloc(ctx, &t->gpart, t->gpart_n) || dalloc(ctx, &t->vpart, VBLK);
    if (t->L > 0) rc = rc || dalloc(ctx, &t->feat, Mx * ECONV) || dalloc(ctx, &t->mask, Mx);
    rc = rc || store_build(&t->st, ctx, sizes, true, &off);   // last: it ends with a synchronous copy, after every allocation's memset
    for (size_t i = 0; i < tb.size() && !rc; ++i) {
        t->off[tb[i].name] = off[i];
        if (tb[i].name.compare(0, strlen(kEnc), kEnc) == 0) {
            if (t->enc_n == 0) t->enc_off = off[i];
            t->enc_n += tb[i].numel;
        }
    }
    if (rc) {
        g_create_err = ctx->err.empty() ? std::string("said_unet_train_create: allocation failed") : ctx->err;
        said_unet_train_destroy(t);
        return -1;
    }
    *out = t;
    return 0;
}

int said_unet_train_destroy(said_unet_train* t) {
    if (!t) return 0;
    DeviceRestore restore_device;
    (void)hipSetDevice(t->c.device);
    if (t->s) { (void)hipStreamSynchronize(t->s); (void)hipStreamDestroy(t->s); }
    return delete_ctx(t);
}

const char* said_unet_train_last_error(const said_unet_train* t) { return ctx_error(t); }

static float* copy_of(said_unet_train* t, int which, int i) { return store_copy_of(&t->st, which, t->off.at((*t->tb)[i].name)); }

int said_unet_train_set_tensor(said_unet_train* t, int which, const char* name, const float* host, long long n) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    const int i = tindex(t, name);
    if (i < 0) return fail(ctx, "said_unet_train_set_tensor: unknown tensor %s", name ? name : "(null)");
    if (!host || n != (*t->tb)[i].numel) return fail(ctx, "said_unet_train_set_tensor: %s has %lld elements, got %lld", name, (*t->tb)[i].numel, n);
    float* dst = copy_of(t, which, i);
    if (!dst) return fail(ctx, "said_unet_train_set_tensor: no copy %d", which);
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    return store_copy(&t->st, t->s, dst, host, n, hipMemcpyHostToDevice, true);
}

int said_unet_train_get_tensor(said_unet_train* t, int which, const char* name, float* host, long long n) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    const int i = tindex(t, name);
    if (i < 0) return fail(ctx, "said_unet_train_get_tensor: unknown tensor %s", name ? name : "(null)");
    if (!host || n != (*t->tb)[i].numel) return fail(ctx, "said_unet_train_get_tensor: %s has %lld elements, got %lld", name, (*t->tb)[i].numel, n);
    float* src = copy_of(t, which, i);
    if (!src) return fail(ctx, "said_unet_train_get_tensor: no copy %d", which);
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    return store_copy(&t->st, t->s, host, src, n, hipMemcpyDeviceToHost, true);
}

int said_unet_train_reset_optimizer(said_unet_train* t) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    return store_reset_optimizer(&t->st, t->s);
}

int said_unet_train_copy(said_unet_train* t, int dst, int src) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    float *d = store_copy_of(&t->st, dst, 0), *s = store_copy_of(&t->st, src, 0);
    if (!d || !s || dst == src) return fail(ctx, "said_unet_train_copy: copies %d <- %d", dst, src);
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    return store_copy(&t->st, t->s, d, s, t->st.nparam, hipMemcpyDeviceToDevice, false);
}

int said_unet_train_set_alphas(said_unet_train* t, const float* ac, int n) {
    if (!t) return -1;
    if (!ac || n < 1) return fail(&t->c, "said_unet_train_set_alphas: empty table");
    t->alphas.assign(ac, ac + n);
    return 0;
}

int said_unet_train_step(said_unet_train* t, int B, int T, const float* coeffs, const float* noise, const long long* ts, const int* cond,
                         const void* audio, int audio_on_device, unsigned long long seed, const float* scalars, const float* std_,
                         const float* deltas, int V) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    const char* what = "said_unet_train_step";
    if (!noise || !scalars) return fail(ctx, "%s: null noise or scalars", what);
    const float p = scalars[SAID_UT_S_DROPOUT];
    if (!(p >= 0.f && p < 1.f)) return fail(ctx, "%s: dropout probability %g outside [0, 1)", what, (double)p);
    if (check_std(t, std_, what)) return -1;
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (put_inputs(t, what, B, T, coeffs, noise, ts, cond, audio, audio_on_device, true) || put_deltas(t, what, B, T, deltas, V) ||
        put_record(t, scalars, std_))
        return -1;
    layout(t->a, t->arena, B, T, t->F);
    add_noise(t->s, B, T, t->coeffs, t->noise, t->sasb, t->rec, t->a.noisy, t->a.answer);
    enqueue_forward(t, B, T, t->st.P, p, seed);
    enqueue_loss(t, B, T, deltas ? V : 0, true, t->st.acc);
    HIPCHK(hipMemsetAsync(t->a.dembs, 0, (size_t)B * TEd * sizeof(float), t->s));
    HIPCHK(hipMemsetAsync(t->a.dctx, 0, (size_t)B * T * t->CTX * sizeof(float), t->s));
    enqueue_backward(t, B, T, p, seed);
    store_enqueue_update(&t->st, t->s, t->rec);
    HIPCHK(hipGetLastError());
    return 0;
}

int said_unet_train_eval_loss(said_unet_train* t, int B, int T, const float* coeffs, const float* noise, const long long* ts, const int* cond,
                              const void* audio, int audio_on_device, const float* scalars, const float* std_, const float* deltas, int V, int ema) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    const char* what = "said_unet_train_eval_loss";
    if (!noise || !scalars) return fail(ctx, "%s: null noise or scalars", what);
    if (check_std(t, std_, what)) return -1;
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (put_inputs(t, what, B, T, coeffs, noise, ts, cond, audio, audio_on_device, true) || put_deltas(t, what, B, T, deltas, V) ||
        put_record(t, scalars, std_))
        return -1;
    layout(t->a, t->arena, B, T, t->F);
    add_noise(t->s, B, T, t->coeffs, t->noise, t->sasb, t->rec, t->a.noisy, t->a.answer);
    enqueue_forward(t, B, T, ema ? t->st.E : t->st.P, 0.f, 0);
    enqueue_loss(t, B, T, deltas ? V : 0, false, t->st.acc + NACC);
    HIPCHK(hipGetLastError());
    return 0;
}

int said_unet_train_forward_only(said_unet_train* t, int B, int T, const float* sample, const long long* ts, const int* cond, const void* audio,
                                 int audio_on_device, int ema, float* out) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    const char* what = "said_unet_train_forward_only";
    if (!out) return fail(ctx, "%s: null output", what);
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (put_inputs(t, what, B, T, sample, nullptr, ts, cond, audio, audio_on_device, false)) return -1;
    layout(t->a, t->arena, B, T, t->F);
    HIPCHK(hipMemcpyAsync(t->a.noisy, t->coeffs, (size_t)B * T * XC * sizeof(float), hipMemcpyDeviceToDevice, t->s));
    enqueue_forward(t, B, T, ema ? t->st.E : t->st.P, 0.f, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, t->a.pred, (size_t)B * T * XC * sizeof(float), hipMemcpyDeviceToHost, t->s));
    HIPCHK(hipStreamSynchronize(t->s));
    return 0;
}

// the _ft entry points' own checks and the upload of the step's time mask; tp may be null (eval mode)
static int put_audio_params(said_unet_train* t, const char* what, int B, int T, const said_audio_train_params* tp) {
    HostCtx* ctx = &t->c;
    if (!tp) return 0;
    for (const float p : {tp->p_feat_proj, tp->p_hidden, tp->p_attention, tp->p_activation})
        if (!(p >= 0.f && p < 1.f)) return fail(ctx, "%s: dropout probability %g is outside [0, 1)", what, (double)p);
    if (tp->time_mask_dev) {
        HIPCHK(hipMemcpyAsync(t->mask, tp->time_mask_dev, (size_t)B * T, hipMemcpyDeviceToDevice, t->s));
        HIPCHK(hipStreamSynchronize(t->s));   // the caller's mask may go away after the call
    }
    return 0;
}

int said_unet_train_step_ft(said_unet_train* t, int B, int T, const float* coeffs, const float* noise, const long long* ts, const int* cond,
                            const void* features, int features_on_device, const said_audio_train_params* tp, unsigned long long seed,
                            const float* scalars, const float* std_, const float* deltas, int V) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    const char* what = "said_unet_train_step_ft";
    if (!noise || !scalars) return fail(ctx, "%s: null noise or scalars", what);
    const float p = scalars[SAID_UT_S_DROPOUT];
    if (!(p >= 0.f && p < 1.f)) return fail(ctx, "%s: dropout probability %g outside [0, 1)", what, (double)p);
    if (check_std(t, std_, what)) return -1;
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (put_inputs(t, what, B, T, coeffs, noise, ts, cond, features, features_on_device, true, true) || put_audio_params(t, what, B, T, tp) ||
        put_deltas(t, what, B, T, deltas, V) || put_record(t, scalars, std_))
        return -1;
    layout(t->a, t->arena, B, T, t->F, t->L, &t->e);
    const size_t M = (size_t)B * T;
    add_noise(t->s, B, T, t->coeffs, t->noise, t->sasb, t->rec, t->a.noisy, t->a.answer);
    enqueue_enc_forward(t, B, T, t->st.P, tp);
    enqueue_forward(t, B, T, t->st.P, p, seed);
    enqueue_loss(t, B, T, deltas ? V : 0, true, t->st.acc);
    HIPCHK(hipMemsetAsync(t->a.dembs, 0, (size_t)B * TEd * sizeof(float), t->s));
    HIPCHK(hipMemsetAsync(t->a.dctx, 0, M * t->CTX * sizeof(float), t->s));
    HIPCHK(hipMemsetAsync(t->st.G + t->enc_off, 0, (size_t)t->enc_n * sizeof(float), t->s));
    enqueue_backward(t, B, T, p, seed);
    // a.dcond: the conditional samples' rows of the context gradient; through W_proj when there is a projection
    float* dE = t->a.dcond;
    if (t->F > 0) {
        Gm{t}.lin_dgrad(t->a.dcond, par(t, t->st.P, "audio_proj_layer.weight"), t->e.d, AUD, (int)M, t->CTX, AUD, 0);
        dE = t->e.d;
    }
    enqueue_enc_backward(t, B, T, tp, dE);
    store_enqueue_update(&t->st, t->s, t->rec);
    HIPCHK(hipGetLastError());
    return 0;
}

int said_unet_train_eval_loss_ft(said_unet_train* t, int B, int T, const float* coeffs, const float* noise, const long long* ts, const int* cond,
                                 const void* features, int features_on_device, const said_audio_train_params* tp, const float* scalars,
                                 const float* std_, const float* deltas, int V, int ema) {
    if (!t) return -1;
    (void)tp;   // validation runs the encoder in eval mode
    HostCtx* ctx = &t->c;
    const char* what = "said_unet_train_eval_loss_ft";
    if (!noise || !scalars) return fail(ctx, "%s: null noise or scalars", what);
    if (check_std(t, std_, what)) return -1;
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (put_inputs(t, what, B, T, coeffs, noise, ts, cond, features, features_on_device, true, true) || put_deltas(t, what, B, T, deltas, V) ||
        put_record(t, scalars, std_))
        return -1;
    layout(t->a, t->arena, B, T, t->F, t->L, &t->e);
    add_noise(t->s, B, T, t->coeffs, t->noise, t->sasb, t->rec, t->a.noisy, t->a.answer);
    enqueue_enc_forward(t, B, T, ema ? t->st.E : t->st.P, nullptr);
    enqueue_forward(t, B, T, ema ? t->st.E : t->st.P, 0.f, 0);
    enqueue_loss(t, B, T, deltas ? V : 0, false, t->st.acc + NACC);
    HIPCHK(hipGetLastError());
    return 0;
}

int said_unet_train_forward_only_ft(said_unet_train* t, int B, int T, const float* sample, const long long* ts, const int* cond, const void* features,
                                    int features_on_device, const said_audio_train_params* tp, int ema, float* out) {
    if (!t) return -1;
    (void)tp;   // the forward runs the encoder in eval mode
    HostCtx* ctx = &t->c;
    const char* what = "said_unet_train_forward_only_ft";
    if (!out) return fail(ctx, "%s: null output", what);
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (put_inputs(t, what, B, T, sample, nullptr, ts, cond, features, features_on_device, false, true)) return -1;
    layout(t->a, t->arena, B, T, t->F, t->L, &t->e);
    HIPCHK(hipMemcpyAsync(t->a.noisy, t->coeffs, (size_t)B * T * XC * sizeof(float), hipMemcpyDeviceToDevice, t->s));
    enqueue_enc_forward(t, B, T, ema ? t->st.E : t->st.P, nullptr);
    enqueue_forward(t, B, T, ema ? t->st.E : t->st.P, 0.f, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, t->a.pred, (size_t)B * T * XC * sizeof(float), hipMemcpyDeviceToHost, t->s));
    HIPCHK(hipStreamSynchronize(t->s));
    return 0;
}

int said_unet_train_last_conditioning(said_unet_train* t, int B, int T, float* out) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (t->L <= 0 || !out || B < 1 || B > t->maxB || T < 2 || T > t->maxT)
        return fail(ctx, "said_unet_train_last_conditioning: needs a fine-tuning context, an output and the last call's shape");
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    layout(t->a, t->arena, B, T, t->F, t->L, &t->e);
    HIPCHK(hipMemcpyAsync(out, t->a.ctx, (size_t)B * T * t->CTX * sizeof(float), hipMemcpyDeviceToHost, t->s));
    HIPCHK(hipStreamSynchronize(t->s));
    return 0;
}

// the split products' scratch exists only in a context that was asked for them
static int need_split_scratch(said_unet_train* t) {
    if (t->amax) return 0;
    return dalloc(&t->c, &t->amax, eg::EG_AMAX_BLOCKS);
}

int said_unet_train_set_encoder_products(said_unet_train* t, int mode) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    const char* what = "said_unet_train_set_encoder_products";
    if (t->L <= 0) return fail(ctx, "%s: the context has no fine-tuned encoder (said_unet_train_create_ft with finetune_layers >= 1)", what);
    if (mode != SAID_UT_PRODUCTS_FP32 && mode != SAID_UT_PRODUCTS_SPLIT_F16)
        return fail(ctx, "%s: unknown mode %d (SAID_UT_PRODUCTS_FP32 = 0, SAID_UT_PRODUCTS_SPLIT_F16 = 1)", what, mode);
    static_assert(eg::enc_gemm_takes(EH, EH) && eg::enc_gemm_takes(EH, ECONV) && eg::enc_gemm_takes(EFFN, EH), "enc_gemm.hip's tile and the encoder's widths");
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (mode == SAID_UT_PRODUCTS_SPLIT_F16 && need_split_scratch(t)) return -1;
    t->products = mode;
    return 0;
}

int said_unet_train_encoder_products(const said_unet_train* t) { return t ? t->products : -1; }

int said_unet_train_dense_product(said_unet_train* t, int layout, int rows, int n, int k, const float* a_host, const float* b_host,
                                  const float* bias_host, const float* res_host, int accumulate, int mode, float* out_host) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    const char* what = "said_unet_train_dense_product";
    const bool fwd = layout == SAID_UT_PRODUCT_FORWARD, dg = layout == SAID_UT_PRODUCT_DGRAD, wg = layout == SAID_UT_PRODUCT_WGRAD;
    if (!fwd && !dg && !wg) return fail(ctx, "%s: unknown layout %d", what, layout);
    if (mode != SAID_UT_PRODUCTS_FP32 && mode != SAID_UT_PRODUCTS_SPLIT_F16) return fail(ctx, "%s: unknown mode %d", what, mode);
    if (rows < 1 || n < 1 || k < 1 || (long long)rows * std::max(n, k) >= (1ll << 31) || (long long)n * k >= (1ll << 31))
        return fail(ctx, "%s: %d rows, widths (%d, %d)", what, rows, n, k);
    if (!a_host || !b_host || !out_host) return fail(ctx, "%s: null operand or output", what);
    if (!fwd && (bias_host || res_host)) return fail(ctx, "%s: only the forward layout has a bias and a residual", what);
    if (wg && accumulate) return fail(ctx, "%s: the weight gradient does not accumulate", what);
    if (mode == SAID_UT_PRODUCTS_SPLIT_F16) {
        if (t->L <= 0) return fail(ctx, "%s: split products need a context with a fine-tuned encoder", what);
        if (!eg::enc_gemm_takes(n, k)) return fail(ctx, "%s: split products take widths that are multiples of %d, got (%d, %d)", what, eg::EG_TILE, n, k);
    }
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (mode == SAID_UT_PRODUCTS_SPLIT_F16 && need_split_scratch(t)) return -1;
    const size_t na = (size_t)rows * (fwd ? k : n), nb = wg ? (size_t)rows * k : (size_t)n * k;
    const size_t no = fwd ? (size_t)rows * n : dg ? (size_t)rows * k : (size_t)n * k;
    // one allocation for the call: a, b, out, bias, res, each from a 256-byte boundary
    auto up = [](size_t v) { return (v + 63) / 64 * 64; };
    const size_t oa = 0, ob = oa + up(na), oo = ob + up(nb), obias = oo + up(no), ores = obias + up((size_t)n), total = ores + up(no);
    float* buf = nullptr;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&buf), total * sizeof(float)));
    int rc = 0;
    auto put = [&](size_t off, const float* h, size_t cnt) {
        if (!rc && h && hipMemcpyAsync(buf + off, h, cnt * sizeof(float), hipMemcpyHostToDevice, t->s) != hipSuccess) rc = -1;
    };
    put(oa, a_host, na); put(ob, b_host, nb); put(obias, bias_host, (size_t)n); put(ores, res_host, no);
    if (accumulate) put(oo, out_host, no);
    else if (!rc && hipMemsetAsync(buf + oo, 0xff, no * sizeof(float), t->s) != hipSuccess) rc = -1;   // NaNs: the product must write every element
    if (!rc) {
        const Gm gm{t, mode};
        if (fwd) gm.lin(buf + oa, k, buf + ob, bias_host ? buf + obias : nullptr, buf + oo, n, rows, n, k, res_host ? buf + ores : nullptr, n, accumulate);
        else if (dg) gm.lin_dgrad(buf + oa, buf + ob, buf + oo, k, rows, n, k, accumulate);
        else gm.lin_wgrad(buf + oa, buf + ob, k, buf + oo, nullptr, rows, n, k);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(out_host, buf + oo, no * sizeof(float), hipMemcpyDeviceToHost, t->s) != hipSuccess) rc = -1;
    }
    const hipError_t se = hipStreamSynchronize(t->s);
    (void)hipFree(buf);
    if (rc || se != hipSuccess) return fail(ctx, "%s: a copy or a launch failed: %s", what, hipGetErrorString(se));
    return 0;
}

int said_unet_train_apply_update(said_unet_train* t, const float* scalars) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (!scalars) return fail(ctx, "said_unet_train_apply_update: null scalars");
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    if (put_record(t, scalars, nullptr)) return -1;
    store_enqueue_update(&t->st, t->s, t->rec);
    HIPCHK(hipGetLastError());
    return 0;
}

int said_unet_train_read_losses(said_unet_train* t, int val, double* acc_host, int* status, int reset) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (!acc_host) return fail(ctx, "said_unet_train_read_losses: null output");
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    return store_read_losses(&t->st, t->s, val, acc_host, status, reset);
}

int said_unet_train_last_losses(said_unet_train* t, float* out) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (!out) return fail(ctx, "said_unet_train_last_losses: null output");
    DeviceRestore restore_device;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(out, t->st.last, 4 * sizeof(float), hipMemcpyDeviceToHost, t->s));
    HIPCHK(hipMemcpyAsync(out + 4, t->st.clip, 2 * sizeof(float), hipMemcpyDeviceToHost, t->s));
    HIPCHK(hipStreamSynchronize(t->s));
    return 0;
}

}  // extern "C"
