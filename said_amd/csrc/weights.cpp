// weights.cpp — said_set_weight / said_finalize_weights: validation of the state dict, the host-side folds, and the upload of every weight in the
// layouts of weight_pack.h (MFMA fragment order in fp32, bf16 and split-fp16, the fused transformer tail's weight streams).
#include "engine_internal.h"
#include "weight_pack.h"

namespace said {
namespace host {

using namespace pack;

namespace {

// the one allocate-and-copy primitive: `bytes` host bytes -> a new device array owned by the context
int upload_bytes(HostCtx* ctx, void** out, const void* h, size_t bytes) {
    char* d = nullptr;
    if (dalloc(ctx, &d, bytes, false)) return -1;
    HIPCHK(hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    *out = d;
    return 0;
}
template <typename D, typename T>
int upload_vec(HostCtx* ctx, D** out, const std::vector<T>& v) {
    void* d = nullptr;
    if (upload_bytes(ctx, &d, v.data(), v.size() * sizeof(T))) return -1;
    *out = static_cast<D*>(d);
    return 0;
}

}  // namespace

int upload(HostCtx* ctx, float** out, const float* h, size_t n) {
    void* d = nullptr;
    if (upload_bytes(ctx, &d, h, n * sizeof(float))) return -1;
    *out = static_cast<float*>(d);
    return 0;
}

const HostTensor* getw(HostCtx* ctx, const std::string& name, std::initializer_list<int64_t> shape) {
    auto it = ctx->host_w.find(name);
    if (it == ctx->host_w.end()) { fail(ctx, "missing key in state dict: %s", name.c_str()); return nullptr; }
    if (it->second.shape != std::vector<int64_t>(shape)) {
        std::string got;
        for (auto d : it->second.shape) got += std::to_string(d) + ",";
        fail(ctx, "size mismatch for %s: got (%s)", name.c_str(), got.c_str());
        return nullptr;
    }
    return &it->second;
}

namespace {

// a Linear weight (N, C), or a Conv1d weight (N, C, taps) where the state dict holds a 3-d tensor under that name
const HostTensor* getw_mat(HostCtx* ctx, const std::string& name, int N, int C, int taps) {
    auto it = ctx->host_w.find(name);
    return taps > 0 && it != ctx->host_w.end() && it->second.shape.size() == 3 ? getw(ctx, name, {N, C, taps}) : getw(ctx, name, {N, C});
}
// the tensors of one part of the model (names share `prefix`): each fetched and validated once; `ok` turns false at the first that is missing or misshapen
struct Fetch {
    HostCtx* ctx;
    std::string prefix;
    bool ok = true;
    const HostTensor* keep(const HostTensor* t) { ok = ok && t; return t; }
    const HostTensor* operator()(const std::string& name, std::initializer_list<int64_t> shape) { return keep(getw(ctx, prefix + name, shape)); }
    const HostTensor* mat(const std::string& name, int N, int C, int taps) { return keep(getw_mat(ctx, prefix + name, N, C, taps)); }
};

int upvec(HostCtx* ctx, float** out, const std::string& name, int64_t n) {
    const HostTensor* t = getw(ctx, name, {n});
    return t ? upload_vec(ctx, out, t->data) : -1;
}

// Range check of a tensor whose elements are split into fp16 planes (w = h + 2^-11 l, both fp16): h is finite for |w| < 65504 — a 2x margin is kept — and the
// pair resolves 2^-36 absolute, i.e. 2^-22 of the tensor's largest element (fp32's own resolution in a dot product) only while that element is >= 2^-14.
// Outside this range fp32 mode keeps the fp32 matrix instructions for EVERYTHING (one arithmetic per run), and said_precision_note says why.
void scan_split_range(said_ctx* ctx, const std::string& name, const std::vector<float>& w) {
    if (ctx->split_unsafe) return;
    float mx = 0.f;
    bool finite = true;
    for (const float v : w) { const float a = std::fabs(v); if (!(a <= 3.4028234663852886e38f)) finite = false; else if (a > mx) mx = a; }
    if (!finite || mx >= 32768.f || (mx > 0.f && mx < 6.103515625e-05f)) {
        char b[320];
        snprintf(b, sizeof b, "%s: max |w| = %.3g is outside [2^-14, 2^15): fp32 mode runs on v_mfma_f32_32x32x2_f32 (SAID_PREC_FP32_STRICT) instead of split-fp16 products",
                 name.c_str(), finite ? (double)mx : INFINITY);
        ctx->split_unsafe = true;
        ctx->split_note = b;
    }
}

// fp32 host matrix [N][C][taps] -> bf16 (RNE) device array with the K axis tap-major (the token-major im2col order of tgemm.hip)
int upload_bf16(HostCtx* ctx, void** out, const float* W, size_t N, size_t C, size_t taps) { return upload_vec(ctx, out, to_bf16(tap_major(W, N, C, taps))); }
// the same matrix in bf16 AND fp32 (UNet operands of the token-major GEMMs: the precision mode is chosen per call)
// out_packed (optional): a third copy whose elements are split-fp16 pairs, one dword h | l << 16 each —
// fgemm_kernel's packed mode unpacks them with v_perm instead of splitting fp32 weights in its k loop
int upload_tm_pair(HostCtx* ctx, void** out_bf, void** out_f32, const float* W, size_t N, size_t C, size_t taps, void** out_packed = nullptr) {
    const std::vector<float> tm = tap_major(W, N, C, taps);
    if (upload_vec(ctx, out_bf, to_bf16(tm)) || upload_vec(ctx, out_f32, tm)) return -1;
    return out_packed ? upload_vec(ctx, out_packed, to_split_words(tm)) : 0;
}

// the split-fp16 packing (PW::ws) a UNet weight gets besides w / w4 / w2: per 24-channel block, or flat (GEGLU: one output tile per wave over the whole K)
enum class Split { none, block, flat };
struct Affine { const HostTensor *g = nullptr, *b = nullptr; };   // gamma and beta (Ctot each) of a norm applied to a GEMM's source

// Segment s of pw (its N and taps are set): the K range [c_begin, c_begin + C) of W (N, Ctot[, taps]).  gn / ln: this range of the GroupNorm / LayerNorm affines is appended to the w4, w2
// and ws blocks so that the LDS-staged kernel can locate them from its preloaded header alone (gemm_lds.hip, FastHdr).
int pack_seg(HostCtx* ctx, PW* pw, int s, const HostTensor& W, int c_begin, int C, Affine gn, Affine ln, Split split) {
    const Rows rows = rows_dense(W.data.data(), (int)W.shape[1], pw->taps, pw->N);
    pw->C[s] = C;
    if (upload_vec(ctx, &pw->w[s], pack_rows(rows, c_begin, C))) return -1;
    if (C % 8 || (pw->taps != 1 && pw->taps != 3)) return 0;
    std::vector<float> tail;
    for (const Affine& a : {gn, ln})
        for (const HostTensor* t : {a.g, a.b})
            if (t) tail.insert(tail.end(), t->data.begin() + c_begin, t->data.begin() + c_begin + C);
    pw->gn_tail = pw->gn_tail || gn.g;
    pw->ln_tail = pw->ln_tail || ln.g;
    auto with_tail = [&](std::vector<float> p) { p.insert(p.end(), tail.begin(), tail.end()); return p; };
    if (upload_vec(ctx, &pw->w4[s], with_tail(pack_rows4(rows, c_begin, C))) || upload_vec(ctx, &pw->w2[s], with_tail(pack_rows_bf16(rows, c_begin, C)))) return -1;
    if (split != Split::none && C % 192 == 0) {   // (KS = 8 waves x whole 24-channel blocks)
        pw->ws_flat = split == Split::flat;
        if (upload_vec(ctx, &pw->ws[s], with_tail(pack_rows_split(rows, c_begin, C, pw->ws_flat)))) return -1;
    }
    return 0;
}
// Linear / conv weight W (N, Ctot[, taps]) -> PW with the K range split into `nseg` equal segments, and its bias (optional)
int pack_pw(HostCtx* ctx, PW* pw, const HostTensor& W, const HostTensor* bias, int nseg = 1, Affine gn = {}, Affine ln = {}, Split split = Split::none) {
    const int Ctot = (int)W.shape[1];
    pw->N = (int)W.shape[0]; pw->taps = W.shape.size() == 3 ? (int)W.shape[2] : 1; pw->nseg = nseg;
    for (int s = 0; s < nseg; ++s)
        if (pack_seg(ctx, pw, s, W, s * (Ctot / nseg), Ctot / nseg, gn, ln, split)) return -1;
    return bias ? upload_vec(ctx, &pw->bias, bias->data) : 0;
}
// a UNet weight that also gets the split-fp16 packing: its range is scanned first, under `name`
int pack_pw_split(said_ctx* ctx, PW* pw, const std::string& name, const HostTensor& W, const HostTensor* bias, int nseg = 1, Affine gn = {}, Affine ln = {},
                  Split split = Split::block) {
    scan_split_range(ctx, name, W.data);
    return pack_pw(ctx, pw, W, bias, nseg, gn, ln, split);
}

}  // namespace

int make_pw(HostCtx* ctx, PW* pw, const std::string& wname, const std::string& bname, int N, int Ctot, int taps, int nseg,
            const std::string& gn_gamma, const std::string& gn_beta, const std::string& ln_gamma, const std::string& ln_beta) {
    Fetch get{ctx, ""};
    const HostTensor* W = get.mat(wname, N, Ctot, taps);
    if (!W) return -1;
    Affine gn, ln;
    if (!gn_gamma.empty()) gn = {get(gn_gamma, {Ctot}), get(gn_beta, {Ctot})};
    if (!ln_gamma.empty()) ln = {get(ln_gamma, {Ctot}), get(ln_beta, {Ctot})};
    const HostTensor* bias = bname.empty() ? nullptr : get(bname, {N});
    return get.ok ? pack_pw(ctx, pw, *W, bias, nseg, gn, ln) : -1;
}

namespace {

// ---- the parts of said_finalize_weights ----
const std::string D = "denoiser.model.";

// the time embedding and the in and out convolutions
int finalize_embed_in_out(said_ctx* ctx) {
    if (make_pw(ctx, &ctx->te1, D + "time_embed.0.weight", D + "time_embed.0.bias", TE, MC, 0)) return -1;
    if (make_pw(ctx, &ctx->te2, D + "time_embed.2.weight", D + "time_embed.2.bias", TE, TE, 0)) return -1;
    if (make_pw(ctx, &ctx->conv_in, D + "input_blocks.0.0.weight", D + "input_blocks.0.0.bias", MC, ctx->cin, 3)) return -1;
    Fetch get{ctx, D + "out."};
    const HostTensor *g = get("0.weight", {MC}), *b = get("0.bias", {MC}), *w = get("2.weight", {ctx->cin, MC, 3}), *wb = get("2.bias", {ctx->cin});
    if (!get.ok) return -1;
    // (out_sched_kernel's split-fp16 products)
    if (pack_pw_split(ctx, &ctx->conv_out, D + "out.2.weight", *w, wb, 1, {g, b})) return -1;
    if (upload_bf16(ctx, &ctx->bw_out, w->data.data(), (size_t)ctx->cin, MC, 3)) return -1;
    return upload_vec(ctx, &ctx->out_g, g->data) || upload_vec(ctx, &ctx->out_b, b->data) ? -1 : 0;
}

// ResBlock `r` (`p` = its key prefix); its emb_layers rows go into the one GEMM of all five (emb_w, emb_b)
int finalize_resblock(said_ctx* ctx, int r, const std::string& p, HostTensor& emb_w, HostTensor& emb_b) {
    ResW& rw = ctx->res[r];
    rw.cin = r >= 3 ? 2 * MC : MC;
    rw.has_skip = r >= 3;
    rw.bias2 = nullptr;
    Fetch get{ctx, p};
    const HostTensor *g1 = get(".in_layers.0.weight", {rw.cin}), *b1 = get(".in_layers.0.bias", {rw.cin});
    const HostTensor *w1 = get(".in_layers.2.weight", {MC, rw.cin, 3}), *wb1 = get(".in_layers.2.bias", {MC});
    const HostTensor *g2 = get(".out_layers.0.weight", {MC}), *b2 = get(".out_layers.0.bias", {MC});
    const HostTensor *w2 = get(".out_layers.3.weight", {MC, MC, 3}), *wb2 = get(".out_layers.3.bias", {MC});
    const HostTensor *ew = get(".emb_layers.1.weight", {MC, TE}), *eb = get(".emb_layers.1.bias", {MC});
    const HostTensor *sk = rw.has_skip ? get(".skip_connection.weight", {MC, 2 * MC, 1}) : nullptr, *skb = rw.has_skip ? get(".skip_connection.bias", {MC}) : nullptr;
    if (!get.ok) return -1;
    // the ResBlock weights also in the split-fp16 packing (small-batch fp32 products: gemm_lds.hip SP)
    if (upload_vec(ctx, &rw.g1, g1->data) || upload_vec(ctx, &rw.b1, b1->data)) return -1;
    if (pack_pw_split(ctx, &rw.conv1, p + ".in_layers.2.weight", *w1, wb1, rw.has_skip ? 2 : 1, {g1, b1})) return -1;
    if (upload_vec(ctx, &rw.g2, g2->data) || upload_vec(ctx, &rw.b2, b2->data)) return -1;
    if (pack_pw_split(ctx, &rw.conv2, p + ".out_layers.3.weight", *w2, wb2, 1, {g2, b2})) return -1;
    {   // tgemm.hip operands: conv1 [192][3 * cin] tap-major; conv2 [192][576 (+ 384 skip columns)]
        if (upload_tm_pair(ctx, &rw.t_conv1, &rw.tf_conv1, w1->data.data(), MC, (size_t)rw.cin, 3, &rw.tp_conv1)) return -1;
        const size_t Kc = 3 * MC + (sk ? 2 * MC : 0);
        std::vector<float> cat((size_t)MC * Kc);
        for (int n = 0; n < MC; ++n) {
            for (int t = 0; t < 3; ++t)
                for (int cc = 0; cc < MC; ++cc) cat[n * Kc + t * MC + cc] = w2->data[((size_t)n * MC + cc) * 3 + t];
            if (sk) for (int cc = 0; cc < 2 * MC; ++cc) cat[n * Kc + 3 * MC + cc] = sk->data[(size_t)n * 2 * MC + cc];
        }
        if (upload_tm_pair(ctx, &rw.t_conv2, &rw.tf_conv2, cat.data(), MC, Kc, 1, &rw.tp_conv2)) return -1;
    }
    std::copy(ew->data.begin(), ew->data.end(), emb_w.data.begin() + (size_t)r * MC * TE);
    std::copy(eb->data.begin(), eb->data.end(), emb_b.data.begin() + (size_t)r * MC);
    if (sk) {
        if (pack_pw_split(ctx, &rw.skip, p + ".skip_connection.weight", *sk, skb, 2)) return -1;
        std::vector<float> sum(MC);
        for (int i = 0; i < MC; ++i) sum[i] = wb2->data[i] + skb->data[i];
        if (upload_vec(ctx, &rw.bias2, sum)) return -1;
    }
    return 0;
}

// attn2 output for the unconditional context (null_cond_emb repeated: every key / value identical, softmax
// uniform => output = to_v(null)), pushed through to_out: c2 = W_out (W_v null) + b_out, in double
std::vector<float> fold_null_attn2(const HostTensor& wv, const HostTensor& nc, const HostTensor& wo, const HostTensor& bo, int CD) {
    std::vector<double> vn(MC, 0.0);
    for (int r = 0; r < MC; ++r) {
        double a = 0.0;
        for (int k = 0; k < CD; ++k) a += (double)wv.data[(size_t)r * CD + k] * nc.data[k];
        vn[r] = (double)(float)a;   // the reference's value rows are fp32
    }
    std::vector<float> c2v(MC);
    for (int n = 0; n < MC; ++n) {
        double a = bo.data[n];
        for (int r = 0; r < MC; ++r) a += (double)wo.data[(size_t)n * MC + r] * vn[r];
        c2v[n] = (float)a;
    }
    return c2v;
}

// proj_out o ff.net.2 folded into ONE GEMM over [h (768) ; x2 (192)]  (attention.py:193 `ff(norm3(x)) + x`, :232-234):
//   proj(F2 h + b2 + x2) + bp = (P F2) h + P x2 + (P b2 + bp).  The products are formed in double on the host: pf = P F2 [192][768], pb = P b2 + bp.
void fold_ffproj(const HostTensor& F2, const HostTensor& b2, const HostTensor& Pw, const HostTensor& bp, HostTensor& pf, HostTensor& pb) {
    pf = HostTensor{std::vector<float>((size_t)MC * FFI), {MC, FFI}};
    pb = HostTensor{std::vector<float>(MC), {MC}};
    std::vector<double> row(FFI);
    for (int n = 0; n < MC; ++n) {
        std::fill(row.begin(), row.end(), 0.0);
        double bb = bp.data[n];
        for (int k = 0; k < MC; ++k) {
            const double pk = Pw.data[(size_t)n * MC + k];
            bb += pk * b2.data[k];
            const float* f2 = &F2.data[(size_t)k * FFI];
            for (int c = 0; c < FFI; ++c) row[c] += pk * f2[c];
        }
        for (int c = 0; c < FFI; ++c) pf.data[(size_t)n * FFI + c] = (float)row[c];
        pb.data[n] = (float)bb;
    }
}

// Operands of the fused SpatialTransformer tail (stchain.hip) for block `b` (= "...transformer_blocks.0"): the weight streams of weight_pack.h (chain_plan) for
// one, three and two slices and in bf16, and the vectors b1, bq = Wq beta2, bo2, c2, bffp, bff'.  LayerNorm2 / LayerNorm3 affines are folded in:
// W' = W diag(gamma), bias' = bias + W beta.
struct ChainSrc { const HostTensor *W1, *B1, *Wq, *G2, *Be2, *W3, *B3, *Wf, *Bf, *G3, *Be3, *ffproj /* [P F2 | P] */, *ffproj_b; };
int pack_chain(said_ctx* ctx, STW& sw, const std::string& b, const ChainSrc& t, const std::vector<float>& c2v) {
    static_assert(MC == CHAIN_MC && FFI == CHAIN_FFI, "the tail's layout is fixed to the model's sizes");
    // the matrices the stream holds that pack_pw_split has not seen: the LayerNorm-folded to_q and GEGLU projections
    const std::vector<float> wq = fold_gamma(t.Wq->data.data(), MC, MC, t.G2->data.data()), wf = fold_gamma(t.Wf->data.data(), 2 * FFI, MC, t.G3->data.data());
    scan_split_range(ctx, b + ".attn2.to_q.weight * norm2.weight", wq);
    scan_split_range(ctx, b + ".ff.net.0.proj.weight * norm3.weight", wf);
    const ChainMats m{{t.W1->data.data(), wq.data(), t.W3->data.data(), wf.data(), t.ffproj->data.data()}};
    const std::vector<ChainUnit> plan1 = chain_plan(1), plan3 = chain_plan(3), plan2 = chain_plan(2);
    const std::vector<uint16_t> s1 = chain_stream_f16(plan1, m);
    if (s1.size() * 2 != CHAIN_STREAM_BYTES) return fail(ctx, "pack_chain: stream size mismatch");
    const std::vector<uint16_t> sb = chain_stream_bf16(plan1, m);
    if (sb.size() != CHAIN_STREAM_UNITS * 512) return fail(ctx, "pack_chain: bf16 stream size mismatch");
    if (upload_vec(ctx, &sw.chain_wb, sb) || upload_vec(ctx, &sw.chain_w, s1)) return -1;
    const std::vector<uint16_t> s3 = chain_stream_f16(plan3, m);   // (stchain.h CHAIN3_*)
    if (s3.size() * 2 != CHAIN3_STREAM_BYTES) return fail(ctx, "pack_chain: three-slice stream size mismatch");
    if (upload_vec(ctx, &sw.chain_w3, s3)) return -1;
    const std::vector<uint16_t> s2 = chain_stream_f16(plan2, m);   // (stchain.h CHAIN2_*)
    if (s2.size() * 2 != CHAIN2_STREAM_BYTES) return fail(ctx, "pack_chain: two-slice stream size mismatch");
    if (upload_vec(ctx, &sw.chain_w2, s2)) return -1;
    if ((int)c2v.size() != MC) return -1;
    const std::vector<float> bq = fold_beta(t.Wq->data.data(), MC, MC, t.Be2->data.data(), nullptr);
    const std::vector<float> bff = fold_beta(t.Wf->data.data(), 2 * FFI, MC, t.Be3->data.data(), t.Bf->data.data());
    return upload_vec(ctx, &sw.chain_vec, chain_vec(t.B1->data.data(), bq.data(), t.B3->data.data(), c2v.data(), t.ffproj_b->data.data(), bff.data()));
}

// SpatialTransformer `i` (`p` = its key prefix); its cross-attention k / v rows go into the one GEMM of all four (kv_w)
int finalize_transformer(said_ctx* ctx, int i, const std::string& p, HostTensor& kv_w) {
    const int CD = ctx->ctx_dim;
    const std::string b = p + ".transformer_blocks.0";
    STW& sw = ctx->st[i];
    Fetch get{ctx, p};
    const HostTensor *gn_g = get(".norm.weight", {MC}), *gn_b = get(".norm.bias", {MC});
    const HostTensor *proj = get.mat(".proj_out.weight", MC, MC, 1), *proj_b = get(".proj_out.bias", {MC});
    get.prefix = b;
    const HostTensor *l1g = get(".norm1.weight", {MC}), *l1b = get(".norm1.bias", {MC}), *l2g = get(".norm2.weight", {MC}), *l2b = get(".norm2.bias", {MC});
    const HostTensor *l3g = get(".norm3.weight", {MC}), *l3b = get(".norm3.bias", {MC});
    const HostTensor *wq = get(".attn1.to_q.weight", {MC, MC}), *wk = get(".attn1.to_k.weight", {MC, MC}), *wv = get(".attn1.to_v.weight", {MC, MC});
    const HostTensor *out1 = get(".attn1.to_out.0.weight", {MC, MC}), *out1_b = get(".attn1.to_out.0.bias", {MC});
    const HostTensor *q2 = get(".attn2.to_q.weight", {MC, MC}), *k2 = get(".attn2.to_k.weight", {MC, CD}), *v2 = get(".attn2.to_v.weight", {MC, CD});
    const HostTensor *out2 = get(".attn2.to_out.0.weight", {MC, MC}), *out2_b = get(".attn2.to_out.0.bias", {MC});
    const HostTensor *ff1 = get(".ff.net.0.proj.weight", {2 * FFI, MC}), *ff1_b = get(".ff.net.0.proj.bias", {2 * FFI});
    const HostTensor *ff2 = get(".ff.net.2.weight", {MC, FFI}), *ff2_b = get(".ff.net.2.bias", {MC});
    get.prefix = "";
    const HostTensor* nc = get("null_cond_emb", {1, 1, CD});
    if (!get.ok) return -1;

    for (auto [dst, t] : {std::pair{&sw.gn_g, gn_g}, {&sw.gn_b, gn_b}, {&sw.l1g, l1g}, {&sw.l1b, l1b}, {&sw.l2g, l2g}, {&sw.l2b, l2b}, {&sw.l3g, l3g}, {&sw.l3b, l3b}})
        if (upload_vec(ctx, dst, t->data)) return -1;
    // the weights also in the split-fp16 packing (small-batch fp32 products: gemm_lds.hip SP)
    HostTensor qkv{wq->data, {3 * MC, MC}};
    qkv.data.insert(qkv.data.end(), wk->data.begin(), wk->data.end());
    qkv.data.insert(qkv.data.end(), wv->data.begin(), wv->data.end());
    if (pack_pw_split(ctx, &sw.qkv, "__qkv", qkv, nullptr, 1, {gn_g, gn_b}, {l1g, l1b})) return -1;
    if (pack_pw_split(ctx, &sw.out1, b + ".attn1.to_out.0.weight", *out1, out1_b)) return -1;
    if (pack_pw_split(ctx, &sw.q2, b + ".attn2.to_q.weight", *q2, nullptr, 1, {}, {l2g, l2b})) return -1;
    std::copy(k2->data.begin(), k2->data.end(), kv_w.data.begin() + (size_t)(i * 2) * MC * CD);
    std::copy(v2->data.begin(), v2->data.end(), kv_w.data.begin() + (size_t)(i * 2 + 1) * MC * CD);
    if (pack_pw_split(ctx, &sw.out2, b + ".attn2.to_out.0.weight", *out2, out2_b)) return -1;
    // the three 192 x 192 projections around the banded cross-attention as token-major GEMM operands (xgemm_kernel)
    if (upload_tm_pair(ctx, &sw.t_out1, &sw.tf_out1, out1->data.data(), MC, MC, 1) || upload_tm_pair(ctx, &sw.t_q2, &sw.tf_q2, q2->data.data(), MC, MC, 1) ||
        upload_tm_pair(ctx, &sw.t_out2, &sw.tf_out2, out2->data.data(), MC, MC, 1))
        return -1;
    const std::vector<float> c2v = fold_null_attn2(*v2, *nc, *out2, *out2_b, CD);
    if (upload_vec(ctx, &ctx->c2[i], c2v)) return -1;
    // GEGLU runs as one output tile per wave over the whole K (NB = 4): flat step layout
    if (pack_pw_split(ctx, &sw.ff1, b + ".ff.net.0.proj.weight", *ff1, ff1_b, 1, {}, {l3g, l3b}, Split::flat)) return -1;
    // (no launch multiplies by ff.net.2 or proj_out alone — only by their fold below — but their packing keeps both in fp32 mode's split-range scan)
    if (pack_pw_split(ctx, &sw.ff2, b + ".ff.net.2.weight", *ff2, ff2_b)) return -1;
    if (pack_pw_split(ctx, &sw.proj, p + ".proj_out.weight", *proj, proj_b)) return -1;
    HostTensor pf, pb, ffproj{std::vector<float>((size_t)MC * (FFI + MC)), {MC, FFI + MC}};   // ffproj = [P F2 | P]
    fold_ffproj(*ff2, *ff2_b, *proj, *proj_b, pf, pb);
    for (int n = 0; n < MC; ++n) {
        std::copy(pf.data.begin() + (size_t)n * FFI, pf.data.begin() + (size_t)(n + 1) * FFI, ffproj.data.begin() + (size_t)n * (FFI + MC));
        std::copy(proj->data.begin() + (size_t)n * MC, proj->data.begin() + (size_t)(n + 1) * MC, ffproj.data.begin() + (size_t)n * (FFI + MC) + FFI);
    }
    {   // its two K segments have different widths, and its halves are range-scanned as the matrices they are
        scan_split_range(ctx, "__ffproj.w0", pf.data);
        scan_split_range(ctx, "__ffproj.w1", proj->data);
        PW& fp = sw.ffproj;
        fp.N = MC; fp.taps = 1; fp.nseg = 2;
        if (pack_seg(ctx, &fp, 0, ffproj, 0, FFI, {}, {}, Split::block) || upload_vec(ctx, &fp.bias, pb.data) || pack_seg(ctx, &fp, 1, ffproj, FFI, MC, {}, {}, Split::block)) return -1;
    }
    {   // tgemm.hip operands of this block: q/k/v rows, GEGLU rows tile-interleaved (value, gate), [P F2 | P]
        if (upload_tm_pair(ctx, &sw.t_qkv, &sw.tf_qkv, qkv.data.data(), 3 * MC, MC, 1, &sw.tp_qkv)) return -1;
        std::vector<float> pw((size_t)2 * FFI * MC), pbias((size_t)2 * FFI);
        for (int np = 0; np < 2 * FFI; ++np) {   // tile-interleaved (value, gate) rows for tgemm.hip's 256-wide tile
            const int src = tgemm_geglu_src_row(np, 2 * FFI);
            std::copy(ff1->data.begin() + (size_t)src * MC, ff1->data.begin() + (size_t)(src + 1) * MC, pw.begin() + (size_t)np * MC);
            pbias[np] = ff1_b->data[src];
        }
        if (upload_tm_pair(ctx, &sw.t_ff1, &sw.tf_ff1, pw.data(), 2 * FFI, MC, 1) || upload_vec(ctx, &sw.t_ff1_bias, pbias)) return -1;
        if (upload_tm_pair(ctx, &sw.t_ffproj, &sw.tf_ffproj, ffproj.data.data(), MC, FFI + MC, 1)) return -1;
    }
    return pack_chain(ctx, sw, b, ChainSrc{out1, out1_b, q2, l2g, l2b, out2, out2_b, ff1, ff1_b, l3g, l3b, &ffproj, &pb}, c2v);
}

size_t count_prefix(const said_ctx* ctx, const std::string& p) {
    size_t n = 0;
    for (auto& kv : ctx->host_w) if (kv.first.rfind(p, 0) == 0) ++n;
    return n;
}

const std::string A = "audio_encoder.";

// the audio encoder (optional as a group: absent => said_audio_encode is unavailable) and the audio projection
int finalize_audio(said_ctx* ctx) {
    const size_t n_audio = count_prefix(ctx, A);
    if (n_audio > 0) {
        int cin = 1;
        for (int i = 0; i < 7; ++i) {
            const std::string wn = A + "feature_extractor.conv_layers." + std::to_string(i) + ".conv.weight";
            auto it = ctx->host_w.find(wn);
            if (it == ctx->host_w.end() || it->second.shape.size() != 3) return fail(ctx, "missing key in state dict: %s", wn.c_str());
            const int k = (int)it->second.shape[2];
            ctx->w2v_kernel[i] = k;
            const HostTensor* w = getw(ctx, wn, {W2V_CONV, cin, k});
            if (!w) return -1;
            if (i == 0) {
                if (upload_vec(ctx, &ctx->c0_w, w->data)) return -1;
                if (upvec(ctx, &ctx->c0_g, A + "feature_extractor.conv_layers.0.layer_norm.weight", W2V_CONV)) return -1;
                if (upvec(ctx, &ctx->c0_b, A + "feature_extractor.conv_layers.0.layer_norm.bias", W2V_CONV)) return -1;
            } else {
                if (pack_pw(ctx, &ctx->aconv[i], *w, nullptr)) return -1;
                if (upload_bf16(ctx, &ctx->bw_conv[i], w->data.data(), W2V_CONV, W2V_CONV, (size_t)k)) return -1;
            }
            cin = W2V_CONV;
        }
        if (upvec(ctx, &ctx->fp_lng, A + "feature_projection.layer_norm.weight", W2V_CONV)) return -1;
        if (upvec(ctx, &ctx->fp_lnb, A + "feature_projection.layer_norm.bias", W2V_CONV)) return -1;
        if (make_pw(ctx, &ctx->fproj, A + "feature_projection.projection.weight", A + "feature_projection.projection.bias", W2V_H, W2V_CONV, 0)) return -1;
        if (upload_bf16(ctx, &ctx->bw_fproj, ctx->host_w[A + "feature_projection.projection.weight"].data.data(), W2V_H, W2V_CONV, 1)) return -1;
        const bool has_mse = ctx->host_w.count(A + "masked_spec_embed") != 0;   // optional: only a train-mode time mask reads it
        if (has_mse && upvec(ctx, &ctx->mask_embed, A + "masked_spec_embed", W2V_H)) return -1;
        {   // positional conv: weight_norm(dim=2) folded on the host, then grouped packing (16 groups of 48)
            auto ig = ctx->host_w.find(A + "encoder.pos_conv_embed.conv.weight_g");
            if (ig == ctx->host_w.end() || ig->second.shape.size() != 3) return fail(ctx, "missing key in state dict: %sencoder.pos_conv_embed.conv.weight_g", A.c_str());
            const int K = (int)ig->second.shape[2];
            const int G = 16, CG = W2V_H / G;
            const HostTensor* wg = getw(ctx, A + "encoder.pos_conv_embed.conv.weight_g", {1, 1, K});
            const HostTensor* wv = getw(ctx, A + "encoder.pos_conv_embed.conv.weight_v", {W2V_H, CG, K});
            if (!wg || !wv) return -1;
            std::vector<double> nrm(K, 0.0);
            for (size_t i = 0; i < wv->data.size(); ++i) nrm[i % K] += (double)wv->data[i] * wv->data[i];
            std::vector<float> wfull(wv->data.size());
            for (size_t i = 0; i < wv->data.size(); ++i) {
                const float nk = (float)std::sqrt(nrm[i % K]);
                wfull[i] = wv->data[i] * (wg->data[i % K] / nk);
            }
            PW& pw = ctx->posconv;
            pw.N = CG; pw.taps = K; pw.nseg = 1; pw.C[0] = CG;
            std::vector<float> packed;
            for (int g = 0; g < G; ++g) {
                const auto part = pack_rows(rows_dense(wfull.data(), CG, K, CG, g * CG), 0, CG);
                packed.insert(packed.end(), part.begin(), part.end());
            }
            if (upload_vec(ctx, &pw.w[0], packed)) return -1;
            const HostTensor* pb = getw(ctx, A + "encoder.pos_conv_embed.conv.bias", {W2V_H});
            if (!pb || upload_vec(ctx, &pw.bias, pb->data)) return -1;
            if (CG % 8 == 0 && CG <= 64 && (K * CG) % 64 == 0) {   // bf16 mode: group g as a GEMM, rows padded to one 64-wide tile
                std::vector<float> wg64((size_t)G * 64 * K * CG, 0.f);
                for (int g = 0; g < G; ++g)
                    for (int n = 0; n < CG; ++n)
                        for (int c = 0; c < CG; ++c)
                            for (int k = 0; k < K; ++k)
                                wg64[(((size_t)g * 64 + n) * K + k) * CG + c] = wfull[((size_t)(g * CG + n) * CG + c) * K + k];
                if (upload_bf16(ctx, &ctx->bw_pos, wg64.data(), (size_t)G * 64, (size_t)K * CG, 1)) return -1;
                std::vector<float> bp(W2V_H + 64, 0.f);
                std::copy(pb->data.begin(), pb->data.end(), bp.begin());
                if (upload_vec(ctx, &ctx->pos_bias_pad, bp)) return -1;
            }
        }
        if (upvec(ctx, &ctx->enc_lng, A + "encoder.layer_norm.weight", W2V_H) || upvec(ctx, &ctx->enc_lnb, A + "encoder.layer_norm.bias", W2V_H)) return -1;
        int L = 0;
        while (ctx->host_w.count(A + "encoder.layers." + std::to_string(L) + ".layer_norm.weight")) ++L;
        ctx->w2v_layers = L;
        ctx->layers.resize(L);
        ctx->blayers.resize(L);
        for (int l = 0; l < L; ++l) {
            const std::string p = A + "encoder.layers." + std::to_string(l);
            W2VLayer& ly = ctx->layers[l];
            Fetch get{ctx, p};
            HostTensor qkv{{}, {3 * W2V_H, W2V_H}}, qb{{}, {3 * W2V_H}};
            for (const char* n : {"q_proj", "k_proj", "v_proj"}) {
                const HostTensor* w = get(std::string(".attention.") + n + ".weight", {W2V_H, W2V_H});
                const HostTensor* b = get(std::string(".attention.") + n + ".bias", {W2V_H});
                if (!get.ok) return -1;
                qkv.data.insert(qkv.data.end(), w->data.begin(), w->data.end());
                qb.data.insert(qb.data.end(), b->data.begin(), b->data.end());
            }
            const HostTensor *ow = get(".attention.out_proj.weight", {W2V_H, W2V_H}), *ob = get(".attention.out_proj.bias", {W2V_H});
            const HostTensor *f1 = get(".feed_forward.intermediate_dense.weight", {W2V_FFN, W2V_H}), *f1b = get(".feed_forward.intermediate_dense.bias", {W2V_FFN});
            const HostTensor *f2 = get(".feed_forward.output_dense.weight", {W2V_H, W2V_FFN}), *f2b = get(".feed_forward.output_dense.bias", {W2V_H});
            if (!get.ok) return -1;
            if (pack_pw(ctx, &ly.qkv, qkv, &qb) || pack_pw(ctx, &ly.out, *ow, ob) || pack_pw(ctx, &ly.ff1, *f1, f1b) || pack_pw(ctx, &ly.ff2, *f2, f2b)) return -1;
            // bf16 copies for the bf16-mode encoder
            said_ctx::BLayer& bl = ctx->blayers[l];
            if (upload_bf16(ctx, &bl.qkv, qkv.data.data(), 3 * W2V_H, W2V_H, 1) || upload_bf16(ctx, &bl.out, ow->data.data(), W2V_H, W2V_H, 1) ||
                upload_bf16(ctx, &bl.ff1, f1->data.data(), W2V_FFN, W2V_H, 1) || upload_bf16(ctx, &bl.ff2, f2->data.data(), W2V_H, W2V_FFN, 1))
                return -1;
            if (upvec(ctx, &ly.ln1g, p + ".layer_norm.weight", W2V_H) || upvec(ctx, &ly.ln1b, p + ".layer_norm.bias", W2V_H)) return -1;
            if (upvec(ctx, &ly.ln2g, p + ".final_layer_norm.weight", W2V_H) || upvec(ctx, &ly.ln2b, p + ".final_layer_norm.bias", W2V_H)) return -1;
        }
        const size_t expect = (has_mse ? 1 : 0) + 7 + 2 + 4 + 3 + 2 + (size_t)L * 16;
        if (n_audio != expect) return fail(ctx, "unexpected key(s) in state dict: %zu audio_encoder.* tensors, expected %zu", n_audio, expect);
        ctx->has_audio = true;
    }
    if (ctx->host_w.count("audio_proj_layer.weight")) {
        if (make_pw(ctx, &ctx->aproj, "audio_proj_layer.weight", "audio_proj_layer.bias", ctx->ctx_dim, W2V_H, 0)) return -1;
        if (upload_bf16(ctx, &ctx->bw_aproj, ctx->host_w["audio_proj_layer.weight"].data.data(), (size_t)ctx->ctx_dim, W2V_H, 1)) return -1;
        ctx->has_audio_proj = true;
    }
    return 0;
}

// the key census: no tensor outside the groups packed above
int census(said_ctx* ctx) {
    for (auto& kv : ctx->host_w) {
        const std::string& k = kv.first;
        if (k.rfind("denoiser.", 0) == 0 || k.rfind(A, 0) == 0 || k == "null_cond_emb" || k == "audio_proj_layer.weight" || k == "audio_proj_layer.bias") continue;
        return fail(ctx, "unexpected key(s) in state dict: %s", k.c_str());
    }
    return 0;
}

}  // namespace

}  // namespace host
}  // namespace said

extern "C" {

int said_set_weight(said_ctx* ctx, const char* name, const float* data_host, const int64_t* shape, int ndim) {
    if (!ctx) return -1;
    if (ctx->finalized) return fail(ctx, "said_set_weight after finalize");
    if (!name || !data_host || !shape || ndim < 1 || ndim > 8) return fail(ctx, "said_set_weight: bad arguments");
    for (int i = 0; i < ndim; ++i) if (shape[i] < 0) return fail(ctx, "said_set_weight(%s): negative dimension", name);
    ++ctx->n_set_weight;
    HostTensor t;
    t.shape.assign(shape, shape + ndim);
    t.data.assign(data_host, data_host + t.numel());
    ctx->host_w[name] = std::move(t);
    return 0;
}

int said_set_timestep_freqs(said_ctx* ctx, const float* f, int n) {
    if (!ctx) return -1;
    if (n != MC / 2) return fail(ctx, "said_set_timestep_freqs: expected %d entries, got %d", MC / 2, n);
    HIPCHK(hipMemcpy(ctx->freqs, f, n * sizeof(float), hipMemcpyHostToDevice));
    ctx->freqs_set = true;
    return 0;
}

int said_finalize_weights(said_ctx* ctx, void* stream) {
    (void)stream;
    if (!ctx) return -1;
    if (ctx->finalized) return fail(ctx, "weights already finalized");
    HIPCHK(hipSetDevice(ctx->device));
    const int CD = ctx->ctx_dim;

    // ---- UNet ----
    if (finalize_embed_in_out(ctx)) return -1;
    const char* res_names[NRES] = {"input_blocks.1.0", "middle_block.0", "middle_block.2", "output_blocks.0.0", "output_blocks.1.0"};
    const char* st_names[NST] = {"input_blocks.1.1", "middle_block.1", "output_blocks.0.1", "output_blocks.1.1"};
    HostTensor emb_w{std::vector<float>((size_t)NRES * MC * TE), {NRES * MC, TE}}, emb_b{std::vector<float>((size_t)NRES * MC), {NRES * MC}};
    for (int r = 0; r < NRES; ++r)
        if (finalize_resblock(ctx, r, D + res_names[r], emb_w, emb_b)) return -1;
    if (pack_pw(ctx, &ctx->emb_all, emb_w, &emb_b)) return -1;   // all five emb_layers as one GEMM (960 x 768)
    HostTensor kv_w{std::vector<float>((size_t)NST * 2 * MC * CD), {NST * 2 * MC, CD}};
    for (int i = 0; i < NST; ++i)
        if (finalize_transformer(ctx, i, D + st_names[i], kv_w)) return -1;
    if (pack_pw(ctx, &ctx->kv_all, kv_w, nullptr)) return -1;     // all four blocks' cross-attention k and v as one GEMM
    const HostTensor* nc = getw(ctx, "null_cond_emb", {1, 1, CD});
    if (!nc || upload_vec(ctx, &ctx->null_cond, nc->data)) return -1;
    if (count_prefix(ctx, "denoiser.") != 160) return fail(ctx, "unexpected key(s) in state dict: %zu denoiser.* tensors, expected 160", count_prefix(ctx, "denoiser."));

    if (finalize_audio(ctx) || census(ctx)) return -1;
    if (!ctx->freqs_set) {
        std::vector<float> f(MC / 2);
        for (int k = 0; k < MC / 2; ++k) f[k] = (float)std::exp(-std::log(10000.0) * k / (MC / 2));
        HIPCHK(hipMemcpy(ctx->freqs, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    ctx->host_w.clear();
    ctx->finalized = true;
    return 0;
}

}  // extern "C"
