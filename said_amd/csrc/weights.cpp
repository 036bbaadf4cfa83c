// weights.cpp — said_set_weight / said_finalize_weights: validation of the state dict and packing of every weight
// into MFMA fragment order (fp32, bf16 and split-fp16 layouts), the fused transformer tail's weight stream included.
#include "engine_internal.h"

namespace said {
namespace host {

int upload(HostCtx* ctx, float** out, const float* h, size_t n) {
    if (dalloc(ctx, out, n, false)) return -1;
    HIPCHK(hipMemcpy(*out, h, n * sizeof(float), hipMemcpyHostToDevice));
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

int upvec(HostCtx* ctx, float** out, const std::string& name, int64_t n) {
    const HostTensor* t = getw(ctx, name, {n});
    if (!t) return -1;
    return upload(ctx, out, t->data.data(), (size_t)n);
}

// Range check of a tensor whose elements are split into fp16 planes (w = h + 2^-11 l, both fp16): h is finite for |w| < 65504 — a 2x margin is kept — and the
// pair resolves 2^-36 absolute, i.e. 2^-22 of the tensor's largest element (fp32's own resolution in a dot product) only while that element is >= 2^-14.
// Outside this range fp32 mode keeps the fp32 matrix instructions for EVERYTHING (one arithmetic per run), and said_precision_note says why.
void scan_split_range(said_ctx* ctx, const std::string& name, const float* w, size_t n) {
    if (ctx->split_unsafe) return;
    float mx = 0.f;
    bool finite = true;
    for (size_t i = 0; i < n; ++i) { const float a = std::fabs(w[i]); if (!(a <= 3.4028234663852886e38f)) finite = false; else if (a > mx) mx = a; }
    if (!finite || mx >= 32768.f || (mx > 0.f && mx < 6.103515625e-05f)) {
        char b[320];
        snprintf(b, sizeof b, "%s: max |w| = %.3g is outside [2^-14, 2^15): fp32 mode runs on v_mfma_f32_32x32x2_f32 (SAID_PREC_FP32_STRICT) instead of split-fp16 products",
                 name.c_str(), finite ? (double)mx : INFINITY);
        ctx->split_unsafe = true;
        ctx->split_note = b;
    }
}

// Pack W[Ntot][Ctot][taps] into MFMA A-fragment order: Wp[group][tile][tap][cpair][lane],
// lane l <-> (n = tile*32 + (l & 31), c = c_begin + 2*cpair + (l >> 5)); rows beyond N are zero.
std::vector<float> pack_rows(const float* W, int Ctot, int taps, const std::vector<int>& row_of /* per (group,tile,r): row or -1 */,
                             int ntiles_total, int c_begin, int C) {
    std::vector<float> out((size_t)ntiles_total * taps * (C / 2) * 64);
    size_t o = 0;
    for (int tile = 0; tile < ntiles_total; ++tile)
        for (int tap = 0; tap < taps; ++tap)
            for (int cp = 0; cp < C / 2; ++cp)
                for (int l = 0; l < 64; ++l) {
                    const int row = row_of[tile * 32 + (l & 31)];
                    const int c = c_begin + 2 * cp + (l >> 5);
                    out[o++] = row < 0 ? 0.f : W[((size_t)row * Ctot + c) * taps + tap];
                }
    return out;
}
// dwordx4 packing: Wq[tile][tap][c/8][lane][4]; value j of lane l = W[tile*32 + (l & 31)][c_begin + 8*cq + 2*j + (l >> 5)][tap]
std::vector<float> pack_rows4(const float* W, int Ctot, int taps, const std::vector<int>& row_of, int ntiles_total, int c_begin, int C) {
    std::vector<float> out((size_t)ntiles_total * taps * (C / 8) * 256);
    size_t o = 0;
    for (int tile = 0; tile < ntiles_total; ++tile)
        for (int tap = 0; tap < taps; ++tap)
            for (int cq = 0; cq < C / 8; ++cq)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 4; ++j) {
                        const int row = row_of[tile * 32 + (l & 31)];
                        const int c = c_begin + 8 * cq + 2 * j + (l >> 5);
                        out[o++] = row < 0 ? 0.f : W[((size_t)row * Ctot + c) * taps + tap];
                    }
    return out;
}
// round-to-nearest-even fp32 -> bf16 (finite inputs)
inline uint16_t bf16_rne(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    x += 0x7fffu + ((x >> 16) & 1u);
    return (uint16_t)(x >> 16);
}
// bf16 packing for v_mfma_f32_32x32x8_bf16_1k: Wb[tile][tap][c/8][lane][4]; value j of lane l =
// W[tile*32 + (l & 31)][c_begin + 8*cq + 4*(l >> 5) + j][tap].  Returned as float storage (2 bf16 per float).
std::vector<float> pack_rows_bf16(const float* W, int Ctot, int taps, const std::vector<int>& row_of, int ntiles_total, int c_begin, int C) {
    std::vector<uint16_t> h((size_t)ntiles_total * taps * (C / 8) * 256);
    size_t o = 0;
    for (int tile = 0; tile < ntiles_total; ++tile)
        for (int tap = 0; tap < taps; ++tap)
            for (int cq = 0; cq < C / 8; ++cq)
                for (int l = 0; l < 64; ++l)
                    for (int j = 0; j < 4; ++j) {
                        const int row = row_of[tile * 32 + (l & 31)];
                        const int c = c_begin + 8 * cq + 4 * (l >> 5) + j;
                        h[o++] = row < 0 ? (uint16_t)0 : bf16_rne(W[((size_t)row * Ctot + c) * taps + tap]);
                    }
    std::vector<float> out(h.size() / 2);
    memcpy(out.data(), h.data(), h.size() * 2);
    return out;
}
// split-fp16 packing for v_mfma_f32_32x32x16_f16 (gemm_lds.hip SP; kernels.h Seg::ws): w = h + 2^-11 l with h = RN16(w), l = RN16((w - h) * 2^11) (split_f16.h).
// Per 24-channel block: NS = 5 (3 taps) / 2 (1 tap) k16 steps x 2 planes (h, l) x 64 lanes x 8 halfs; the 8 halfs of lane l in step s are K-group
// g = 2 s + (l >> 5) of the block's tap-major K slice (tap = g / 3, channels 8 (g % 3) .. + 7), zeros past the slice's 9 / 3 groups.  flat: C / 16 steps over
// the whole K (taps == 1), no padding.  Returned as float storage (2 halfs per float).
std::vector<float> pack_rows_split(const float* W, int Ctot, int taps, const std::vector<int>& row_of, int ntiles_total, int c_begin, int C, bool flat) {
    const int nblk = flat ? 1 : C / 24, ns = flat ? C / 16 : (taps == 3 ? 5 : 2), ng = flat ? C / 8 : 3 * taps;
    std::vector<_Float16> h((size_t)ntiles_total * nblk * ns * 2 * 512);
    size_t o = 0;
    for (int tile = 0; tile < ntiles_total; ++tile)
        for (int blk = 0; blk < nblk; ++blk)
            for (int st = 0; st < ns; ++st)
                for (int pl = 0; pl < 2; ++pl)
                    for (int l = 0; l < 64; ++l)
                        for (int j = 0; j < 8; ++j) {
                            const int row = row_of[tile * 32 + (l & 31)];
                            const int g = 2 * st + (l >> 5);
                            float v = 0.f;
                            if (row >= 0 && g < ng) {
                                const int tap = flat ? 0 : g / 3;
                                const int c = c_begin + (flat ? 8 * g : 24 * blk + 8 * (g % 3)) + j;
                                v = W[((size_t)row * Ctot + c) * taps + tap];
                            }
                            const _Float16 hv = (_Float16)v;
                            h[o++] = pl == 0 ? hv : (_Float16)((v - (float)hv) * 2048.f);
                        }
    std::vector<float> out(h.size() / 2);
    memcpy(out.data(), h.data(), h.size() * 2);
    return out;
}
// fp32 host matrix -> bf16 (RNE) device array; `perm` (optional) reorders the K axis of a Conv1d weight [N][C][taps] to
// tap-major [N][taps][C] (the token-major im2col order of tgemm.hip)
int upload_bf16(said_ctx* ctx, void** out, const float* W, size_t N, size_t C, size_t taps) {
    std::vector<uint16_t> h(N * C * taps);
    for (size_t n = 0; n < N; ++n)
        for (size_t t = 0; t < taps; ++t)
            for (size_t c = 0; c < C; ++c) h[(n * taps + t) * C + c] = bf16_rne(W[(n * C + c) * taps + t]);
    uint16_t* d = nullptr;
    if (dalloc(ctx, &d, h.size(), false)) return -1;
    HIPCHK(hipMemcpy(d, h.data(), h.size() * 2, hipMemcpyHostToDevice));
    *out = d;
    return 0;
}
// the same matrix in bf16 AND fp32 (UNet operands of the token-major GEMMs: the precision mode is chosen per call)
// out_packed (optional): a third copy whose elements are split-fp16 pairs, one dword h | l << 16 each (split_f16.h pack_split_f16: the same two conversions) —
// fgemm_kernel's packed mode unpacks them with v_perm instead of splitting fp32 weights in its k loop
int upload_tm_pair(said_ctx* ctx, void** out_bf, void** out_f32, const float* W, size_t N, size_t C, size_t taps, void** out_packed = nullptr) {
    if (upload_bf16(ctx, out_bf, W, N, C, taps)) return -1;
    std::vector<float> h(N * C * taps);
    for (size_t n = 0; n < N; ++n)
        for (size_t t = 0; t < taps; ++t)
            for (size_t c = 0; c < C; ++c) h[(n * taps + t) * C + c] = W[(n * C + c) * taps + t];
    float* d = nullptr;
    if (upload(ctx, &d, h.data(), h.size())) return -1;
    *out_f32 = d;
    if (out_packed) {
        std::vector<float> pk(h.size());
        for (size_t i = 0; i < h.size(); ++i) {
            const float v = h[i];
            const _Float16 hv = (_Float16)v;
            const _Float16 lv = (_Float16)((v - (float)hv) * 2048.f);
            uint16_t hb, lb;
            memcpy(&hb, &hv, 2); memcpy(&lb, &lv, 2);
            const uint32_t u = (uint32_t)hb | ((uint32_t)lb << 16);
            memcpy(&pk[i], &u, 4);
        }
        float* dp = nullptr;
        if (upload(ctx, &dp, pk.data(), pk.size())) return -1;
        *out_packed = dp;
    }
    return 0;
}
std::vector<int> rows_dense(int N, int row0 = 0) {
    const int nt = (N + 31) / 32;
    std::vector<int> r(nt * 32, -1);
    for (int i = 0; i < N; ++i) r[i] = row0 + i;
    return r;
}

// Linear/conv weight `wname` (N, Ctot[, taps]) -> PW with the K range split into `nseg` equal segments.
// gn_gamma/gn_beta (optional): affine of the GroupNorm applied to this GEMM's source; appended to each segment's w4
// block so that the LDS-staged kernel can locate them from its preloaded header alone (gemm_lds.hip, FastHdr).
// unet (UNet weights only): also the split-fp16 packing its pw_split asks for.
int pack_pw(HostCtx* ctx, said_ctx* unet, PW* pw, const std::string& wname, const std::string& bname, int N, int Ctot, int taps, int nseg,
            const std::string& gn_gamma, const std::string& gn_beta, const std::string& ln_gamma, const std::string& ln_beta) {
    const int split = unet ? unet->pw_split : 0;
    const HostTensor* t = taps > 0 && ctx->host_w.count(wname) && ctx->host_w[wname].shape.size() == 3
                              ? getw(ctx, wname, {N, Ctot, taps})
                              : getw(ctx, wname, {N, Ctot});
    if (!t) return -1;
    const int tp = t->shape.size() == 3 ? taps : 1;
    pw->N = N; pw->taps = tp; pw->nseg = nseg;
    const auto rows = rows_dense(N);
    for (int s = 0; s < nseg; ++s) {
        const int C = Ctot / nseg;
        pw->C[s] = C;
        auto packed = pack_rows(t->data.data(), Ctot, tp, rows, (N + 31) / 32, s * C, C);
        if (upload(ctx, &pw->w[s], packed.data(), packed.size())) return -1;
        if (C % 8 == 0 && (tp == 1 || tp == 3)) {
            auto p4 = pack_rows4(t->data.data(), Ctot, tp, rows, (N + 31) / 32, s * C, C);
            auto p2 = pack_rows_bf16(t->data.data(), Ctot, tp, rows, (N + 31) / 32, s * C, C);
            const size_t w4_floats = p4.size();
            if (!gn_gamma.empty()) {
                const HostTensor* gg = getw(ctx, gn_gamma, {Ctot});
                const HostTensor* gb = getw(ctx, gn_beta, {Ctot});
                if (!gg || !gb) return -1;
                p4.insert(p4.end(), gg->data.begin() + s * C, gg->data.begin() + (s + 1) * C);
                p4.insert(p4.end(), gb->data.begin() + s * C, gb->data.begin() + (s + 1) * C);
                pw->gn_tail = true;
            }
            if (!ln_gamma.empty()) {
                const HostTensor* lg = getw(ctx, ln_gamma, {Ctot});
                const HostTensor* lb = getw(ctx, ln_beta, {Ctot});
                if (!lg || !lb) return -1;
                p4.insert(p4.end(), lg->data.begin() + s * C, lg->data.begin() + (s + 1) * C);
                p4.insert(p4.end(), lb->data.begin() + s * C, lb->data.begin() + (s + 1) * C);
                pw->ln_tail = true;
            }
            p2.insert(p2.end(), p4.begin() + w4_floats, p4.end());   // the GroupNorm / LayerNorm tails, unchanged
            if (upload(ctx, &pw->w4[s], p4.data(), p4.size())) return -1;
            if (upload(ctx, &pw->w2[s], p2.data(), p2.size())) return -1;
            if (split && C % 192 == 0) {   // (KS = 8 waves x whole 24-channel blocks)
                const bool flat = split == 2;
                if (s == 0) scan_split_range(unet, wname, t->data.data(), t->data.size());
                auto ps = pack_rows_split(t->data.data(), Ctot, tp, rows, (N + 31) / 32, s * C, C, flat);
                ps.insert(ps.end(), p4.begin() + w4_floats, p4.end());
                if (upload(ctx, &pw->ws[s], ps.data(), ps.size())) return -1;
                pw->ws_flat = flat;
            }
        }
    }
    if (!bname.empty()) { if (upvec(ctx, &pw->bias, bname, N)) return -1; }
    return 0;
}

// the UNet's and the audio encoder's weights: said_ctx::pw_split selects the split-fp16 packing
int make_pw(said_ctx* ctx, PW* pw, const std::string& wname, const std::string& bname, int N, int Ctot, int taps, int nseg = 1,
            const std::string& gn_gamma = "", const std::string& gn_beta = "", const std::string& ln_gamma = "",
            const std::string& ln_beta = "") {
    return pack_pw(ctx, ctx, pw, wname, bname, N, Ctot, taps, nseg, gn_gamma, gn_beta, ln_gamma, ln_beta);
}

}  // namespace

int make_pw(HostCtx* ctx, PW* pw, const std::string& wname, const std::string& bname, int N, int Ctot, int taps, int nseg,
            const std::string& gn_gamma, const std::string& gn_beta, const std::string& ln_gamma, const std::string& ln_beta) {
    return pack_pw(ctx, nullptr, pw, wname, bname, N, Ctot, taps, nseg, gn_gamma, gn_beta, ln_gamma, ln_beta);
}

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

// Operands of the fused SpatialTransformer tail (stchain.hip) for block `b` (= "...transformer_blocks.0"):
//  * one weight stream: for each of the kernel's eight waves, 2 KB units (a k16 step's h and l fragments of v_mfma_f32_32x32x16_f16 A operands: lane l holds
//    row 32 tile + (l & 31), k = 16 step + 8 (l >> 5) .. + 7) in the order the wave consumes them — waves 0-5 (column owner j = output columns [32 j, 32 j + 32)):
//    to_out1 12 steps, to_q 12, to_out2 12, GEGLU pairs j, j + 8, j + 16 (12 steps each, value then gate unit per step), folded proj_out over [h ; x2]: 60 steps for
//    j < 4, steps 0 .. 29 for j = 4, 5; waves 6, 7: GEGLU pairs w, w + 8, w + 16, then steps 30 .. 59 of the folded proj_out's column tiles 4, 5.  LayerNorm2 / LayerNorm3 affines are folded in: W' = W diag(gamma) (formed in double), bias' = bias + W beta.
//  * the vectors b1, bq = Wq beta2, bo2, c2, bffp, bff' (CHAIN_VEC_FLOATS).
static int pack_chain(said_ctx* ctx, STW& sw, const std::string& b, const std::vector<float>& c2v) {
    const HostTensor* W1 = getw(ctx, b + ".attn1.to_out.0.weight", {MC, MC});
    const HostTensor* B1 = getw(ctx, b + ".attn1.to_out.0.bias", {MC});
    const HostTensor* Wq = getw(ctx, b + ".attn2.to_q.weight", {MC, MC});
    const HostTensor* G2 = getw(ctx, b + ".norm2.weight", {MC});
    const HostTensor* Be2 = getw(ctx, b + ".norm2.bias", {MC});
    const HostTensor* W3 = getw(ctx, b + ".attn2.to_out.0.weight", {MC, MC});
    const HostTensor* B3 = getw(ctx, b + ".attn2.to_out.0.bias", {MC});
    const HostTensor* Wf = getw(ctx, b + ".ff.net.0.proj.weight", {2 * FFI, MC});
    const HostTensor* Bf = getw(ctx, b + ".ff.net.0.proj.bias", {2 * FFI});
    const HostTensor* G3 = getw(ctx, b + ".norm3.weight", {MC});
    const HostTensor* Be3 = getw(ctx, b + ".norm3.bias", {MC});
    const HostTensor* PF = getw(ctx, "__ffproj.w0", {MC, FFI});
    const HostTensor* PX = getw(ctx, "__ffproj.w1", {MC, MC});
    const HostTensor* PB = getw(ctx, "__ffproj.b", {MC});
    if (!W1 || !B1 || !Wq || !G2 || !Be2 || !W3 || !B3 || !Wf || !Bf || !G3 || !Be3 || !PF || !PX || !PB || (int)c2v.size() != MC) return -1;
    // element (row n, k) of the matrix a unit multiplies, in double (the folds) -> split into fp16 planes
    auto elem = [&](int kind, int n, int k) -> double {
        switch (kind) {
            case 0: return W1->data[(size_t)n * MC + k];
            case 1: return (double)Wq->data[(size_t)n * MC + k] * (double)G2->data[k];
            case 2: return W3->data[(size_t)n * MC + k];
            case 3: return (double)Wf->data[(size_t)n * MC + k] * (double)G3->data[k];
            default: return k < FFI ? PF->data[(size_t)n * FFI + k] : PX->data[(size_t)n * MC + (k - FFI)];
        }
    };
    {   // the matrices the stream holds that make_pw has not seen: the LayerNorm-folded to_q and GEGLU projections
        std::vector<float> f((size_t)2 * FFI * MC);
        for (int n = 0; n < MC; ++n) for (int k = 0; k < MC; ++k) f[(size_t)n * MC + k] = (float)elem(1, n, k);
        scan_split_range(ctx, b + ".attn2.to_q.weight * norm2.weight", f.data(), (size_t)MC * MC);
        for (int n = 0; n < 2 * FFI; ++n) for (int k = 0; k < MC; ++k) f[(size_t)n * MC + k] = (float)elem(3, n, k);
        scan_split_range(ctx, b + ".ff.net.0.proj.weight * norm3.weight", f.data(), f.size());
    }
    std::vector<_Float16> st(CHAIN_STREAM_BYTES / 2);
    size_t o = 0;
    auto put_unit = [&](int kind, int row0, int step) {
        for (int pl = 0; pl < 2; ++pl)
            for (int l = 0; l < 64; ++l)
                for (int i = 0; i < 8; ++i) {
                    const float v = (float)elem(kind, row0 + (l & 31), 16 * step + 8 * (l >> 5) + i);
                    const _Float16 hv = (_Float16)v;
                    st[o++] = pl == 0 ? hv : (_Float16)((v - (float)hv) * 2048.f);
                }
    };
    auto put_geglu = [&](int w) {
        for (int pi = 0; pi < 3; ++pi)
            for (int s = 0; s < 12; ++s) {
                put_unit(3, 32 * (w + 8 * pi), s);
                put_unit(3, FFI + 32 * (w + 8 * pi), s);
            }
    };
    for (int w = 0; w < 6; ++w) {
        for (int kind = 0; kind < 3; ++kind)
            for (int s = 0; s < 12; ++s) put_unit(kind, 32 * w, s);
        put_geglu(w);
        for (int s = 0; s < (w < 4 ? 60 : 30); ++s) put_unit(4, 32 * w, s);   // (column tiles 4, 5: steps 30 .. 59 belong to waves 6, 7)
    }
    for (int w = 6; w < 8; ++w) {
        put_geglu(w);
        for (int s = 30; s < 60; ++s) put_unit(4, 32 * (w - 2), s);
    }
    if (o != st.size()) return fail(ctx, "pack_chain: stream size mismatch");
    {   // the bf16 stream: the same units in the same order, ONE plane of bf16 (RNE) — 1 KB per unit
        std::vector<uint16_t> sb(CHAIN_STREAM_UNITS * 512);
        size_t ob = 0;
        auto put_unit_b = [&](int kind, int row0, int step) {
            for (int l = 0; l < 64; ++l)
                for (int i = 0; i < 8; ++i) sb[ob++] = bf16_rne((float)elem(kind, row0 + (l & 31), 16 * step + 8 * (l >> 5) + i));
        };
        auto put_geglu_b = [&](int w) {
            for (int pi = 0; pi < 3; ++pi)
                for (int s = 0; s < 12; ++s) {
                    put_unit_b(3, 32 * (w + 8 * pi), s);
                    put_unit_b(3, FFI + 32 * (w + 8 * pi), s);
                }
        };
        for (int w = 0; w < 6; ++w) {
            for (int kind = 0; kind < 3; ++kind)
                for (int s = 0; s < 12; ++s) put_unit_b(kind, 32 * w, s);
            put_geglu_b(w);
            for (int s = 0; s < (w < 4 ? 60 : 30); ++s) put_unit_b(4, 32 * w, s);
        }
        for (int w = 6; w < 8; ++w) {
            put_geglu_b(w);
            for (int s = 30; s < 60; ++s) put_unit_b(4, 32 * (w - 2), s);
        }
        if (ob != sb.size()) return fail(ctx, "pack_chain: bf16 stream size mismatch");
        uint16_t* d = nullptr;
        if (dalloc(ctx, &d, sb.size(), false)) return -1;
        HIPCHK(hipMemcpy(d, sb.data(), sb.size() * 2, hipMemcpyHostToDevice));
        sw.chain_wb = d;
    }
    std::vector<float> stf(st.size() / 2);
    memcpy(stf.data(), st.data(), st.size() * 2);
    if (upload(ctx, &sw.chain_w, stf.data(), stf.size())) return -1;
    {   // the three-slice stream (stchain.h CHAIN3_*): slice c = GEGLU pairs 8 c .. 8 c + 7 (one per wave) + k16 steps 16 c .. 16 c + 15 of the folded proj_out's GEGLU
        // segment + steps 4 c .. 4 c + 3 of its x2 segment (steps 48 .. 59 of the 60); the three 192 x 192 projections in front are in every slice
        st.assign(CHAIN3_STREAM_BYTES / 2, (_Float16)0.f);
        o = 0;
        for (int c = 0; c < 3; ++c) {
            int ff[20];
            for (int i = 0; i < 16; ++i) ff[i] = 16 * c + i;
            for (int i = 0; i < 4; ++i) ff[16 + i] = 48 + 4 * c + i;
            auto put_pair = [&](int p) {
                for (int s2 = 0; s2 < 12; ++s2) { put_unit(3, 32 * p, s2); put_unit(3, FFI + 32 * p, s2); }
            };
            for (int w = 0; w < 6; ++w) {
                for (int kind = 0; kind < 3; ++kind)
                    for (int s2 = 0; s2 < 12; ++s2) put_unit(kind, 32 * w, s2);
                put_pair(8 * c + w);
                for (int i = 0; i < (w < 4 ? 20 : 10); ++i) put_unit(4, 32 * w, ff[i]);
            }
            for (int w = 6; w < 8; ++w) {
                put_pair(8 * c + w);
                for (int i = 10; i < 20; ++i) put_unit(4, 32 * (w - 2), ff[i]);
            }
        }
        if (o != st.size()) return fail(ctx, "pack_chain: three-slice stream size mismatch");
        stf.resize(st.size() / 2);
        memcpy(stf.data(), st.data(), st.size() * 2);
        if (upload(ctx, &sw.chain_w3, stf.data(), stf.size())) return -1;
    }
    {   // the two-slice stream (stchain.h CHAIN2_*): slice c = GEGLU pairs 12 c .. 12 c + 11 — waves 0-3 two each (local pairs w, w + 4), waves 4-7 one (w + 4) —
        // + k16 steps 24 c .. 24 c + 23 of the folded proj_out's GEGLU segment + steps 6 c .. 6 c + 5 of its x2 segment
        st.assign(CHAIN2_STREAM_BYTES / 2, (_Float16)0.f);
        o = 0;
        for (int c = 0; c < 2; ++c) {
            int ff[30];
            for (int i = 0; i < 24; ++i) ff[i] = 24 * c + i;
            for (int i = 0; i < 6; ++i) ff[24 + i] = 48 + 6 * c + i;
            auto put_pair = [&](int p) {
                for (int s2 = 0; s2 < 12; ++s2) { put_unit(3, 32 * p, s2); put_unit(3, FFI + 32 * p, s2); }
            };
            for (int w = 0; w < 6; ++w) {
                for (int kind = 0; kind < 3; ++kind)
                    for (int s2 = 0; s2 < 12; ++s2) put_unit(kind, 32 * w, s2);
                if (w < 4) { put_pair(12 * c + w); put_pair(12 * c + w + 4); } else put_pair(12 * c + w + 4);
                for (int i = 0; i < (w < 4 ? 30 : 15); ++i) put_unit(4, 32 * w, ff[i]);
            }
            for (int w = 6; w < 8; ++w) {
                put_pair(12 * c + w + 4);
                for (int i = 15; i < 30; ++i) put_unit(4, 32 * (w - 2), ff[i]);
            }
        }
        if (o != st.size()) return fail(ctx, "pack_chain: two-slice stream size mismatch");
        stf.resize(st.size() / 2);
        memcpy(stf.data(), st.data(), st.size() * 2);
        if (upload(ctx, &sw.chain_w2, stf.data(), stf.size())) return -1;
    }
    std::vector<float> vec(CHAIN_VEC_FLOATS);
    for (int n = 0; n < MC; ++n) {
        double bq = 0.0;
        for (int k = 0; k < MC; ++k) bq += (double)Wq->data[(size_t)n * MC + k] * (double)Be2->data[k];
        vec[n] = B1->data[n];
        vec[MC + n] = (float)bq;
        vec[2 * MC + n] = B3->data[n];
        vec[3 * MC + n] = c2v[n];
        vec[4 * MC + n] = PB->data[n];
    }
    for (int n = 0; n < 2 * FFI; ++n) {
        double bf = Bf->data[n];
        for (int k = 0; k < MC; ++k) bf += (double)Wf->data[(size_t)n * MC + k] * (double)Be3->data[k];
        vec[5 * MC + n] = (float)bf;
    }
    return upload(ctx, &sw.chain_vec, vec.data(), vec.size());
}

int said_finalize_weights(said_ctx* ctx, void* stream) {
    (void)stream;
    if (!ctx) return -1;
    if (ctx->finalized) return fail(ctx, "weights already finalized");
    HIPCHK(hipSetDevice(ctx->device));
    const std::string D = "denoiser.model.";
    const int CD = ctx->ctx_dim;
    size_t used = 0;
    auto count_prefix = [&](const std::string& p) { size_t n = 0; for (auto& kv : ctx->host_w) if (kv.first.rfind(p, 0) == 0) ++n; return n; };

    // ---- UNet ----
    if (make_pw(ctx, &ctx->te1, D + "time_embed.0.weight", D + "time_embed.0.bias", TE, MC, 0)) return -1;
    if (make_pw(ctx, &ctx->te2, D + "time_embed.2.weight", D + "time_embed.2.bias", TE, TE, 0)) return -1;
    if (make_pw(ctx, &ctx->conv_in, D + "input_blocks.0.0.weight", D + "input_blocks.0.0.bias", MC, ctx->cin, 3)) return -1;
    ctx->pw_split = 1;   // (out_sched_kernel's split-fp16 products)
    if (make_pw(ctx, &ctx->conv_out, D + "out.2.weight", D + "out.2.bias", ctx->cin, MC, 3, 1, D + "out.0.weight", D + "out.0.bias")) return -1;
    ctx->pw_split = 0;
    if (upload_bf16(ctx, &ctx->bw_out, ctx->host_w[D + "out.2.weight"].data.data(), (size_t)ctx->cin, MC, 3)) return -1;
    if (upvec(ctx, &ctx->out_g, D + "out.0.weight", MC) || upvec(ctx, &ctx->out_b, D + "out.0.bias", MC)) return -1;
    used += 8;
    const char* res_names[NRES] = {"input_blocks.1.0", "middle_block.0", "middle_block.2", "output_blocks.0.0", "output_blocks.1.0"};
    const char* st_names[NST] = {"input_blocks.1.1", "middle_block.1", "output_blocks.0.1", "output_blocks.1.1"};
    std::vector<float> emb_w((size_t)NRES * MC * TE), emb_b((size_t)NRES * MC);
    ctx->pw_split = 1;   // the ResBlock / SpatialTransformer weights also in the split-fp16 packing (small-batch fp32 products: gemm_lds.hip SP)
    for (int r = 0; r < NRES; ++r) {
        const std::string p = D + res_names[r];
        ResW& rw = ctx->res[r];
        rw.cin = r >= 3 ? 2 * MC : MC;
        rw.has_skip = r >= 3;
        if (upvec(ctx, &rw.g1, p + ".in_layers.0.weight", rw.cin) || upvec(ctx, &rw.b1, p + ".in_layers.0.bias", rw.cin)) return -1;
        if (make_pw(ctx, &rw.conv1, p + ".in_layers.2.weight", p + ".in_layers.2.bias", MC, rw.cin, 3, rw.has_skip ? 2 : 1, p + ".in_layers.0.weight", p + ".in_layers.0.bias")) return -1;
        if (upvec(ctx, &rw.g2, p + ".out_layers.0.weight", MC) || upvec(ctx, &rw.b2, p + ".out_layers.0.bias", MC)) return -1;
        if (make_pw(ctx, &rw.conv2, p + ".out_layers.3.weight", p + ".out_layers.3.bias", MC, MC, 3, 1, p + ".out_layers.0.weight", p + ".out_layers.0.bias")) return -1;
        {   // tgemm.hip operands: conv1 [192][3 * cin] tap-major; conv2 [192][576 (+ 384 skip columns)]
            if (upload_tm_pair(ctx, &rw.t_conv1, &rw.tf_conv1, ctx->host_w[p + ".in_layers.2.weight"].data.data(), MC, (size_t)rw.cin, 3, &rw.tp_conv1)) return -1;
            const HostTensor& c2w = ctx->host_w[p + ".out_layers.3.weight"];
            std::vector<float> cat((size_t)MC * (3 * MC + (rw.has_skip ? 2 * MC : 0)));
            const size_t Kc = 3 * MC + (rw.has_skip ? 2 * MC : 0);
            const HostTensor* sk = rw.has_skip ? getw(ctx, p + ".skip_connection.weight", {MC, 2 * MC, 1}) : nullptr;
            if (rw.has_skip && !sk) return -1;
            for (int n = 0; n < MC; ++n) {
                for (int t = 0; t < 3; ++t)
                    for (int cc = 0; cc < MC; ++cc) cat[n * Kc + t * MC + cc] = c2w.data[((size_t)n * MC + cc) * 3 + t];
                if (sk) for (int cc = 0; cc < 2 * MC; ++cc) cat[n * Kc + 3 * MC + cc] = sk->data[(size_t)n * 2 * MC + cc];
            }
            if (upload_tm_pair(ctx, &rw.t_conv2, &rw.tf_conv2, cat.data(), MC, Kc, 1, &rw.tp_conv2)) return -1;
        }
        const HostTensor* ew = getw(ctx, p + ".emb_layers.1.weight", {MC, TE});
        const HostTensor* eb = getw(ctx, p + ".emb_layers.1.bias", {MC});
        if (!ew || !eb) return -1;
        std::copy(ew->data.begin(), ew->data.end(), emb_w.begin() + (size_t)r * MC * TE);
        std::copy(eb->data.begin(), eb->data.end(), emb_b.begin() + (size_t)r * MC);
        used += 10;
        rw.bias2 = nullptr;
        if (rw.has_skip) {
            if (make_pw(ctx, &rw.skip, p + ".skip_connection.weight", p + ".skip_connection.bias", MC, 2 * MC, 1, 2)) return -1;
            const HostTensor* b2 = getw(ctx, p + ".out_layers.3.bias", {MC});
            const HostTensor* bs = getw(ctx, p + ".skip_connection.bias", {MC});
            std::vector<float> sum(MC);
            for (int i = 0; i < MC; ++i) sum[i] = b2->data[i] + bs->data[i];
            if (upload(ctx, &rw.bias2, sum.data(), MC)) return -1;
            used += 2;
        }
    }
    ctx->pw_split = 0;
    {   // all five emb_layers as one GEMM (960 x 768)
        ctx->host_w["__emb_all.w"] = HostTensor{emb_w, {NRES * MC, TE}};
        ctx->host_w["__emb_all.b"] = HostTensor{emb_b, {NRES * MC}};
        if (make_pw(ctx, &ctx->emb_all, "__emb_all.w", "__emb_all.b", NRES * MC, TE, 0)) return -1;
    }
    std::vector<float> kv_w((size_t)NST * 2 * MC * CD);
    for (int i = 0; i < NST; ++i) {
        const std::string p = D + st_names[i], b = p + ".transformer_blocks.0";
        STW& sw = ctx->st[i];
        ctx->pw_split = 1;
        if (upvec(ctx, &sw.gn_g, p + ".norm.weight", MC) || upvec(ctx, &sw.gn_b, p + ".norm.bias", MC)) return -1;
        if (upvec(ctx, &sw.l1g, b + ".norm1.weight", MC) || upvec(ctx, &sw.l1b, b + ".norm1.bias", MC)) return -1;
        if (upvec(ctx, &sw.l2g, b + ".norm2.weight", MC) || upvec(ctx, &sw.l2b, b + ".norm2.bias", MC)) return -1;
        if (upvec(ctx, &sw.l3g, b + ".norm3.weight", MC) || upvec(ctx, &sw.l3b, b + ".norm3.bias", MC)) return -1;
        const HostTensor* wq = getw(ctx, b + ".attn1.to_q.weight", {MC, MC});
        const HostTensor* wk = getw(ctx, b + ".attn1.to_k.weight", {MC, MC});
        const HostTensor* wv = getw(ctx, b + ".attn1.to_v.weight", {MC, MC});
        if (!wq || !wk || !wv) return -1;
        std::vector<float> qkv;
        qkv.insert(qkv.end(), wq->data.begin(), wq->data.end());
        qkv.insert(qkv.end(), wk->data.begin(), wk->data.end());
        qkv.insert(qkv.end(), wv->data.begin(), wv->data.end());
        ctx->host_w["__qkv"] = HostTensor{qkv, {3 * MC, MC}};
        if (make_pw(ctx, &sw.qkv, "__qkv", "", 3 * MC, MC, 0, 1, p + ".norm.weight", p + ".norm.bias", b + ".norm1.weight", b + ".norm1.bias")) return -1;
        if (make_pw(ctx, &sw.out1, b + ".attn1.to_out.0.weight", b + ".attn1.to_out.0.bias", MC, MC, 0)) return -1;
        if (make_pw(ctx, &sw.q2, b + ".attn2.to_q.weight", "", MC, MC, 0, 1, "", "", b + ".norm2.weight", b + ".norm2.bias")) return -1;
        const HostTensor* k2 = getw(ctx, b + ".attn2.to_k.weight", {MC, CD});
        const HostTensor* v2 = getw(ctx, b + ".attn2.to_v.weight", {MC, CD});
        if (!k2 || !v2) return -1;
        std::copy(k2->data.begin(), k2->data.end(), kv_w.begin() + (size_t)(i * 2) * MC * CD);
        std::copy(v2->data.begin(), v2->data.end(), kv_w.begin() + (size_t)(i * 2 + 1) * MC * CD);
        if (make_pw(ctx, &sw.out2, b + ".attn2.to_out.0.weight", b + ".attn2.to_out.0.bias", MC, MC, 0)) return -1;
        {   // the three 192 x 192 projections around the banded cross-attention as token-major GEMM operands (xgemm_kernel)
            const HostTensor* w1 = getw(ctx, b + ".attn1.to_out.0.weight", {MC, MC});
            const HostTensor* wq2 = getw(ctx, b + ".attn2.to_q.weight", {MC, MC});
            const HostTensor* w2 = getw(ctx, b + ".attn2.to_out.0.weight", {MC, MC});
            if (!w1 || !wq2 || !w2) return -1;
            if (upload_tm_pair(ctx, &sw.t_out1, &sw.tf_out1, w1->data.data(), MC, MC, 1) || upload_tm_pair(ctx, &sw.t_q2, &sw.tf_q2, wq2->data.data(), MC, MC, 1) ||
                upload_tm_pair(ctx, &sw.t_out2, &sw.tf_out2, w2->data.data(), MC, MC, 1))
                return -1;
        }
        std::vector<float> c2_host;
        {   // attn2 output for the unconditional context (null_cond_emb repeated: every key / value identical, softmax
            // uniform => output = to_v(null)), pushed through to_out: c2 = W_out (W_v null) + b_out, in double
            const HostTensor* nc = getw(ctx, "null_cond_emb", {1, 1, CD});
            const HostTensor* wo = getw(ctx, b + ".attn2.to_out.0.weight", {MC, MC});
            const HostTensor* bo = getw(ctx, b + ".attn2.to_out.0.bias", {MC});
            if (!nc || !wo || !bo) return -1;
            std::vector<double> vn(MC, 0.0);
            for (int r = 0; r < MC; ++r) {
                double a = 0.0;
                for (int k = 0; k < CD; ++k) a += (double)v2->data[(size_t)r * CD + k] * nc->data[k];
                vn[r] = (double)(float)a;   // the reference's value rows are fp32
            }
            std::vector<float> c2v(MC);
            for (int n = 0; n < MC; ++n) {
                double a = bo->data[n];
                for (int r = 0; r < MC; ++r) a += (double)wo->data[(size_t)n * MC + r] * vn[r];
                c2v[n] = (float)a;
            }
            if (upload(ctx, &ctx->c2[i], c2v.data(), MC)) return -1;
            c2_host = c2v;
        }
        ctx->pw_split = 2;   // GEGLU runs as one output tile per wave over the whole K (NB = 4): flat step layout
        if (make_pw(ctx, &sw.ff1, b + ".ff.net.0.proj.weight", b + ".ff.net.0.proj.bias", 2 * FFI, MC, 0, 1, "", "", b + ".norm3.weight", b + ".norm3.bias")) return -1;
        ctx->pw_split = 1;
        // (no launch multiplies by ff.net.2 or proj_out alone — only by their fold below — but their packing keeps both in fp32 mode's split-range scan)
        if (make_pw(ctx, &sw.ff2, b + ".ff.net.2.weight", b + ".ff.net.2.bias", MC, FFI, 0)) return -1;
        if (make_pw(ctx, &sw.proj, p + ".proj_out.weight", p + ".proj_out.bias", MC, MC, 1)) return -1;
        {   // proj_out o ff.net.2 folded into ONE GEMM over [h (768) ; x2 (192)]  (attention.py:193 `ff(norm3(x)) + x`, :232-234):
            //   proj(F2 h + b2 + x2) + bp = (P F2) h + P x2 + (P b2 + bp).  The product is formed in double on the host.
            const HostTensor* F2 = getw(ctx, b + ".ff.net.2.weight", {MC, FFI});
            const HostTensor* b2 = getw(ctx, b + ".ff.net.2.bias", {MC});
            const HostTensor* Pw = ctx->host_w.count(p + ".proj_out.weight") && ctx->host_w[p + ".proj_out.weight"].shape.size() == 3
                                       ? getw(ctx, p + ".proj_out.weight", {MC, MC, 1}) : getw(ctx, p + ".proj_out.weight", {MC, MC});
            const HostTensor* bp = getw(ctx, p + ".proj_out.bias", {MC});
            if (!F2 || !b2 || !Pw || !bp) return -1;
            HostTensor PF, PX, PB;
            PF.shape = {MC, FFI}; PF.data.resize((size_t)MC * FFI);
            PX.shape = {MC, MC}; PX.data = Pw->data;
            PB.shape = {MC}; PB.data.resize(MC);
            std::vector<double> row(FFI);
            for (int n = 0; n < MC; ++n) {
                std::fill(row.begin(), row.end(), 0.0);
                double bb = bp->data[n];
                for (int k = 0; k < MC; ++k) {
                    const double pk = Pw->data[(size_t)n * MC + k];
                    bb += pk * b2->data[k];
                    const float* f2 = &F2->data[(size_t)k * FFI];
                    for (int c = 0; c < FFI; ++c) row[c] += pk * f2[c];
                }
                for (int c = 0; c < FFI; ++c) PF.data[(size_t)n * FFI + c] = (float)row[c];
                PB.data[n] = (float)bb;
            }
            ctx->host_w["__ffproj.w0"] = std::move(PF);
            ctx->host_w["__ffproj.w1"] = std::move(PX);
            ctx->host_w["__ffproj.b"] = std::move(PB);
            PW t0, t1;
            if (make_pw(ctx, &t0, "__ffproj.w0", "__ffproj.b", MC, FFI, 0) || make_pw(ctx, &t1, "__ffproj.w1", "", MC, MC, 0)) return -1;
            {   // tgemm.hip operands of this block: q/k/v rows, GEGLU rows tile-interleaved (value, gate), [P F2 | P]
                if (upload_tm_pair(ctx, &sw.t_qkv, &sw.tf_qkv, qkv.data(), 3 * MC, MC, 1, &sw.tp_qkv)) return -1;
                const HostTensor* f1 = getw(ctx, b + ".ff.net.0.proj.weight", {2 * FFI, MC});
                const HostTensor* f1b = getw(ctx, b + ".ff.net.0.proj.bias", {2 * FFI});
                if (!f1 || !f1b) return -1;
                std::vector<float> pw((size_t)2 * FFI * MC), pb((size_t)2 * FFI);
                for (int np = 0; np < 2 * FFI; ++np) {   // tile-interleaved (value, gate) rows for tgemm.hip's 256-wide tile
                    const int src = tgemm_geglu_src_row(np, 2 * FFI);
                    std::copy(f1->data.begin() + (size_t)src * MC, f1->data.begin() + (size_t)(src + 1) * MC, pw.begin() + (size_t)np * MC);
                    pb[np] = f1b->data[src];
                }
                if (upload_tm_pair(ctx, &sw.t_ff1, &sw.tf_ff1, pw.data(), 2 * FFI, MC, 1) || upload(ctx, &sw.t_ff1_bias, pb.data(), pb.size())) return -1;
                const HostTensor& w0 = ctx->host_w["__ffproj.w0"];
                const HostTensor& w1 = ctx->host_w["__ffproj.w1"];
                std::vector<float> cat((size_t)MC * (FFI + MC));
                for (int n = 0; n < MC; ++n) {
                    std::copy(w0.data.begin() + (size_t)n * FFI, w0.data.begin() + (size_t)(n + 1) * FFI, cat.begin() + (size_t)n * (FFI + MC));
                    std::copy(w1.data.begin() + (size_t)n * MC, w1.data.begin() + (size_t)(n + 1) * MC, cat.begin() + (size_t)n * (FFI + MC) + FFI);
                }
                if (upload_tm_pair(ctx, &sw.t_ffproj, &sw.tf_ffproj, cat.data(), MC, FFI + MC, 1)) return -1;
            }
            PW& fp = sw.ffproj;
            fp.N = MC; fp.taps = 1; fp.nseg = 2; fp.bias = t0.bias;
            fp.w[0] = t0.w[0]; fp.w4[0] = t0.w4[0]; fp.w2[0] = t0.w2[0]; fp.ws[0] = t0.ws[0]; fp.C[0] = FFI;
            fp.w[1] = t1.w[0]; fp.w4[1] = t1.w4[0]; fp.w2[1] = t1.w2[0]; fp.ws[1] = t1.ws[0]; fp.C[1] = MC;
        }
        if (pack_chain(ctx, sw, b, c2_host)) return -1;
        used += 24;
        ctx->pw_split = 0;
    }
    ctx->host_w["__kv_all"] = HostTensor{kv_w, {NST * 2 * MC, CD}};
    if (make_pw(ctx, &ctx->kv_all, "__kv_all", "", NST * 2 * MC, CD, 0)) return -1;
    {
        const HostTensor* nc = getw(ctx, "null_cond_emb", {1, 1, CD});
        if (!nc) return -1;
        if (upload(ctx, &ctx->null_cond, nc->data.data(), CD)) return -1;
        used += 1;
    }
    if (count_prefix("denoiser.") != 160) return fail(ctx, "unexpected key(s) in state dict: %zu denoiser.* tensors, expected 160", count_prefix("denoiser."));

    // ---- audio encoder (optional as a group: absent => said_audio_encode is unavailable) ----
    const std::string A = "audio_encoder.";
    const size_t n_audio = count_prefix(A);
    if (n_audio > 0) {
        int cin = 1;
        for (int i = 0; i < 7; ++i) {
            const std::string wn = A + "feature_extractor.conv_layers." + std::to_string(i) + ".conv.weight";
            auto it = ctx->host_w.find(wn);
            if (it == ctx->host_w.end() || it->second.shape.size() != 3) return fail(ctx, "missing key in state dict: %s", wn.c_str());
            const int k = (int)it->second.shape[2];
            ctx->w2v_kernel[i] = k;
            if (!getw(ctx, wn, {W2V_CONV, cin, k})) return -1;
            if (i == 0) {
                if (upload(ctx, &ctx->c0_w, it->second.data.data(), (size_t)W2V_CONV * k)) return -1;
                if (upvec(ctx, &ctx->c0_g, A + "feature_extractor.conv_layers.0.layer_norm.weight", W2V_CONV)) return -1;
                if (upvec(ctx, &ctx->c0_b, A + "feature_extractor.conv_layers.0.layer_norm.bias", W2V_CONV)) return -1;
            } else {
                if (make_pw(ctx, &ctx->aconv[i], wn, "", W2V_CONV, W2V_CONV, k)) return -1;
                if (upload_bf16(ctx, &ctx->bw_conv[i], it->second.data.data(), W2V_CONV, W2V_CONV, (size_t)k)) return -1;
            }
            cin = W2V_CONV;
        }
        if (upvec(ctx, &ctx->fp_lng, A + "feature_projection.layer_norm.weight", W2V_CONV)) return -1;
        if (upvec(ctx, &ctx->fp_lnb, A + "feature_projection.layer_norm.bias", W2V_CONV)) return -1;
        if (make_pw(ctx, &ctx->fproj, A + "feature_projection.projection.weight", A + "feature_projection.projection.bias", W2V_H, W2V_CONV, 0)) return -1;
        if (upload_bf16(ctx, &ctx->bw_fproj, ctx->host_w[A + "feature_projection.projection.weight"].data.data(), W2V_H, W2V_CONV, 1)) return -1;
        if (!getw(ctx, A + "masked_spec_embed", {W2V_H})) return -1;
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
                auto rows = rows_dense(CG, g * CG);
                auto part = pack_rows(wfull.data(), CG, K, rows, (CG + 31) / 32, 0, CG);
                packed.insert(packed.end(), part.begin(), part.end());
            }
            if (upload(ctx, &pw.w[0], packed.data(), packed.size())) return -1;
            if (upvec(ctx, &pw.bias, A + "encoder.pos_conv_embed.conv.bias", W2V_H)) return -1;
            if (CG % 8 == 0 && CG <= 64 && (K * CG) % 64 == 0) {   // bf16 mode: group g as a GEMM, rows padded to one 64-wide tile
                std::vector<float> wg64((size_t)G * 64 * K * CG, 0.f);
                for (int g = 0; g < G; ++g)
                    for (int n = 0; n < CG; ++n)
                        for (int c = 0; c < CG; ++c)
                            for (int k = 0; k < K; ++k)
                                wg64[(((size_t)g * 64 + n) * K + k) * CG + c] = wfull[((size_t)(g * CG + n) * CG + c) * K + k];
                if (upload_bf16(ctx, &ctx->bw_pos, wg64.data(), (size_t)G * 64, (size_t)K * CG, 1)) return -1;
                std::vector<float> bp(W2V_H + 64, 0.f);
                const HostTensor* pb = getw(ctx, A + "encoder.pos_conv_embed.conv.bias", {W2V_H});
                if (!pb) return -1;
                std::copy(pb->data.begin(), pb->data.end(), bp.begin());
                if (upload(ctx, &ctx->pos_bias_pad, bp.data(), bp.size())) return -1;
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
            std::vector<float> qkv, qb;
            for (const char* n : {"q_proj", "k_proj", "v_proj"}) {
                const HostTensor* w = getw(ctx, p + ".attention." + n + ".weight", {W2V_H, W2V_H});
                const HostTensor* b = getw(ctx, p + ".attention." + n + ".bias", {W2V_H});
                if (!w || !b) return -1;
                qkv.insert(qkv.end(), w->data.begin(), w->data.end());
                qb.insert(qb.end(), b->data.begin(), b->data.end());
            }
            ctx->host_w["__aqkv.w"] = HostTensor{qkv, {3 * W2V_H, W2V_H}};
            ctx->host_w["__aqkv.b"] = HostTensor{qb, {3 * W2V_H}};
            if (make_pw(ctx, &ly.qkv, "__aqkv.w", "__aqkv.b", 3 * W2V_H, W2V_H, 0)) return -1;
            if (make_pw(ctx, &ly.out, p + ".attention.out_proj.weight", p + ".attention.out_proj.bias", W2V_H, W2V_H, 0)) return -1;
            if (make_pw(ctx, &ly.ff1, p + ".feed_forward.intermediate_dense.weight", p + ".feed_forward.intermediate_dense.bias", W2V_FFN, W2V_H, 0)) return -1;
            if (make_pw(ctx, &ly.ff2, p + ".feed_forward.output_dense.weight", p + ".feed_forward.output_dense.bias", W2V_H, W2V_FFN, 0)) return -1;
            {   // bf16 copies for the bf16-mode encoder (the shapes were validated by make_pw above)
                said_ctx::BLayer& bl = ctx->blayers[l];
                if (upload_bf16(ctx, &bl.qkv, qkv.data(), 3 * W2V_H, W2V_H, 1)) return -1;
                if (upload_bf16(ctx, &bl.out, ctx->host_w[p + ".attention.out_proj.weight"].data.data(), W2V_H, W2V_H, 1)) return -1;
                if (upload_bf16(ctx, &bl.ff1, ctx->host_w[p + ".feed_forward.intermediate_dense.weight"].data.data(), W2V_FFN, W2V_H, 1)) return -1;
                if (upload_bf16(ctx, &bl.ff2, ctx->host_w[p + ".feed_forward.output_dense.weight"].data.data(), W2V_H, W2V_FFN, 1)) return -1;
            }
            if (upvec(ctx, &ly.ln1g, p + ".layer_norm.weight", W2V_H) || upvec(ctx, &ly.ln1b, p + ".layer_norm.bias", W2V_H)) return -1;
            if (upvec(ctx, &ly.ln2g, p + ".final_layer_norm.weight", W2V_H) || upvec(ctx, &ly.ln2b, p + ".final_layer_norm.bias", W2V_H)) return -1;
        }
        const size_t expect = 1 + 7 + 2 + 4 + 3 + 2 + (size_t)L * 16;
        if (n_audio != expect) return fail(ctx, "unexpected key(s) in state dict: %zu audio_encoder.* tensors, expected %zu", n_audio, expect);
        ctx->has_audio = true;
    }
    if (ctx->host_w.count("audio_proj_layer.weight")) {
        if (make_pw(ctx, &ctx->aproj, "audio_proj_layer.weight", "audio_proj_layer.bias", CD, W2V_H, 0)) return -1;
        if (upload_bf16(ctx, &ctx->bw_aproj, ctx->host_w["audio_proj_layer.weight"].data.data(), (size_t)CD, W2V_H, 1)) return -1;
        ctx->has_audio_proj = true;
    }
    for (auto& kv : ctx->host_w) {
        const std::string& k = kv.first;
        if (k.rfind("denoiser.", 0) == 0 || k.rfind(A, 0) == 0 || k.rfind("__", 0) == 0 || k == "null_cond_emb" ||
            k == "audio_proj_layer.weight" || k == "audio_proj_layer.bias")
            continue;
        return fail(ctx, "unexpected key(s) in state dict: %s", k.c_str());
    }
    if (!ctx->freqs_set) {
        std::vector<float> f(MC / 2);
        for (int k = 0; k < MC / 2; ++k) f[k] = (float)std::exp(-std::log(10000.0) * k / (MC / 2));
        HIPCHK(hipMemcpy(ctx->freqs, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    ctx->host_w.clear();
    ctx->finalized = true;
    (void)used;
    return 0;
}

}  // extern "C"
