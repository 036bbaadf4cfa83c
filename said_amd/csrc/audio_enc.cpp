// audio_enc.cpp — said_audio_encode: the Wav2Vec2 audio encoder (feature extractor, positional conv, transformer layers,
// optional projection) on the gfx950 kernels; said_audio_encode_train: its fp32 channel-major route in Wav2Vec2's train mode
// (include/said_audio_train.h; kernels: audio_train.hip).
#include "../../include/said_audio_train.h"
#include "audio_train.h"
#include "said_audio_features.h"
#include "engine_internal.h"

namespace {

// Both entry points.  tp == nullptr: said_audio_encode, launch for launch what it always issued.  tp != nullptr (validated by
// said_audio_encode_train; fp32 route only): SpecAugment span replacement, the four dropouts and LayerDrop of the train-mode forward.
// features_only: stop behind the interpolation and store the conv features token-major, (B, frames, 512) (said_audio_extract_features).
int audio_encode(said_ctx* ctx, const float* wav_dev, int B, int Ta, int num_frames, int apply_proj, const said_audio_train_params* tp,
                 float* out_dev, int* out_frames, void* stream, bool features_only = false) {
    if (check_ready(ctx)) return -1;
    if (!ctx->has_audio) return fail(ctx, "audio_encoder.* weights were not loaded");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    ctx->n_audio_clips += B;
    int L[7];
    {
        int len = Ta;
        for (int i = 0; i < 7; ++i) {
            len = (len - ctx->w2v_kernel[i]) / ctx->w2v_stride[i] + 1;
            if (len < 1) return fail(ctx, "waveform of %d samples is too short for the feature extractor", Ta);
            L[i] = len;
        }
    }
    const int Fr = num_frames > 0 ? num_frames : L[6];
    if (out_frames) *out_frames = Fr;
    const int Fp = rup(Fr, 32);
    // the dropout masks count logical elements in 32 bits; the largest site is the FFN activation (B, frames, 3072)
    if (tp && (unsigned long long)B * Fr * W2V_FFN >= (1ull << 32))
        return fail(ctx, "said_audio_encode_train: %d clips of %d frames need a dropout index of 2^32 or more", B, Fr);
    if (apply_proj && !ctx->has_audio_proj) return fail(ctx, "apply_proj requested but audio_proj_layer.* was not loaded");
    const int out_dim = apply_proj ? ctx->ctx_dim : W2V_H;
    // workspace: ping-pong conv buffers + token-domain buffers, for `chunk` clips at a time
    // clips per pass: the 65 MB/clip conv0 activation is what bounds it (32 clips = 2.1 GB of 288 GB); larger launches
    // amortise the 377 MB of encoder weights over more tokens
    const int chunk = std::min(B, ctx->audio_chunk);
    const size_t eA = (size_t)chunk * W2V_CONV * rup(L[0], 32), eB = (size_t)chunk * W2V_CONV * rup(L[1], 32);
    const size_t tok = (size_t)chunk * Fp;
    const size_t tw = std::max<size_t>(W2V_H, (size_t)ctx->ctx_dim);   // aT also receives the audio_proj_layer output (ctx_dim wide)
    if (eA > ctx->abuf_elems[0] || eB > ctx->abuf_elems[1] || tok > ctx->a_tok_elems) {
        HIPCHK(hipStreamSynchronize(s));   // the buffers being replaced may still be in use by an earlier call
        if (eA > ctx->abuf_elems[0]) { if (drealloc(ctx, &ctx->abufA, eA)) return -1; ctx->abuf_elems[0] = eA; }
        if (eB > ctx->abuf_elems[1]) { if (drealloc(ctx, &ctx->abufB, eB)) return -1; ctx->abuf_elems[1] = eB; }
        if (tok > ctx->a_tok_elems) {
            if (drealloc(ctx, &ctx->aX, tok * W2V_CONV) || drealloc(ctx, &ctx->aH, tok * W2V_H) || drealloc(ctx, &ctx->aT, tok * tw) ||
                drealloc(ctx, &ctx->aO, tok * 2 * W2V_H) || drealloc(ctx, &ctx->aQK, tok * 2 * W2V_H) || drealloc(ctx, &ctx->aVT, tok * W2V_H) ||
                drealloc(ctx, &ctx->aF, tok * W2V_FFN) || drealloc(ctx, &ctx->aPOS, tok * W2V_H))
                return -1;
            ctx->a_tok_elems = tok;
        }
    }
    // bf16 mode (said_set_precision): token-major bf16 encoder on v_mfma_f32_32x32x16_bf16 (tgemm.hip).  conv0 + its
    // per-channel GroupNorm, the grouped positional convolution and the attention kernel are shared with the fp32 path.
    const bool bfa = !tp && ctx->bf16_mode && (!apply_proj || ctx->ctx_dim % 128 == 0) && (int)ctx->blayers.size() == ctx->w2v_layers;
    if (bfa) {
        const size_t e0 = (size_t)chunk * L[0] * W2V_CONV, e1 = (size_t)chunk * L[1] * W2V_CONV, tk = (size_t)chunk * Fr;
        const size_t xg = (size_t)chunk * 16 * (size_t)rup(Fr + ctx->posconv.taps, 8) * (W2V_H / 16) + 4096;   // per-group positional-conv operand
        if (e0 > ctx->b_conv_elems[0] || e1 > ctx->b_conv_elems[1] || tk > ctx->b_tok || xg > ctx->bXg_elems) {
            HIPCHK(hipStreamSynchronize(s));
            uint16_t** u;
            if (e0 > ctx->b_conv_elems[0]) { u = reinterpret_cast<uint16_t**>(&ctx->bA0); if (drealloc(ctx, u, e0 + 64)) return -1; ctx->b_conv_elems[0] = e0; }
            if (e1 > ctx->b_conv_elems[1]) { u = reinterpret_cast<uint16_t**>(&ctx->bA1); if (drealloc(ctx, u, e1 + 64)) return -1; ctx->b_conv_elems[1] = e1; }
            if (tk > ctx->b_tok) {
                if (drealloc(ctx, reinterpret_cast<uint16_t**>(&ctx->bX), tk * W2V_CONV) || drealloc(ctx, reinterpret_cast<uint16_t**>(&ctx->bHb), tk * W2V_H) ||
                    drealloc(ctx, reinterpret_cast<uint16_t**>(&ctx->bF), tk * W2V_FFN) || drealloc(ctx, reinterpret_cast<uint16_t**>(&ctx->bO), tk * W2V_H) ||
                    drealloc(ctx, &ctx->bH, tk * W2V_H) || drealloc(ctx, &ctx->bT, tk * std::max<size_t>(W2V_H, (size_t)ctx->ctx_dim)) ||
                    drealloc(ctx, &ctx->bPosT, tk * W2V_H))
                    return -1;
                ctx->b_tok = tk;
            }
            if (xg > ctx->bXg_elems) {
                if (drealloc(ctx, reinterpret_cast<uint16_t**>(&ctx->bXg), xg)) return -1;
                ctx->bXg_elems = xg;
            }
        }
        for (int b0 = 0; b0 < B; b0 += chunk) {
            const int nb = std::min(chunk, B - b0);
            // said_debug_option "audio_stop_after": a stage is one launch call site below, numbered per pass in the order documented in said_hip_debug.h;
            // on() is asked once per site, whether or not the site launches
            int stage = 0;
            auto on = [&]() { return ctx->audio_stop_after < 0 || stage++ < ctx->audio_stop_after; };
            auto tgemm = [&](const TGemmArgs& a, int batch) {
                int v = TG_NONE;
                if (!launch_tgemm(a, batch, s, &v)) ctx->launch_err = "audio encoder: token-major GEMM shape not served";
                else ++ctx->n_tgemm[v];
            };
            const int pitch0 = rup(L[0], 32);
            const long long bs0 = (long long)W2V_CONV * pitch0;
            // conv0 + GroupNorm + GELU straight to token-major bf16 (abufA, sized for the fp32 activation, serves as its scratch)
            if (on() && !launch_conv0_gn_gelu_tm_bf16(wav_dev + (long long)b0 * Ta, ctx->c0_w, ctx->c0_g, ctx->c0_b, ctx->abufA, ctx->bA0, nb, Ta, W2V_CONV,
                                              ctx->w2v_kernel[0], ctx->w2v_stride[0], L[0], 1e-5f, s)) {
                launch_conv0(wav_dev + (long long)b0 * Ta, ctx->c0_w, ctx->abufA, nb, Ta, W2V_CONV, ctx->w2v_kernel[0], ctx->w2v_stride[0], L[0], pitch0, bs0, s);
                launch_rownorm_gelu(ctx->abufA, ctx->c0_g, ctx->c0_b, W2V_CONV, nb, L[0], pitch0, bs0, 1e-5f, s);
                launch_cm_to_tm_bf16(ctx->abufA, bs0, pitch0, ctx->bA0, (long long)L[0] * W2V_CONV, nb, L[0], W2V_CONV, s);
            }
            void* src = ctx->bA0;
            void* dst = ctx->bA1;
            for (int i = 1; i < 7; ++i) {   // Conv1d(512, 512, k, stride 2, no bias) + GELU as a GEMM with overlapping rows
                TGemmArgs a;
                memset(&a, 0, sizeof a);
                a.a = src; a.a_bs = (long long)L[i - 1] * W2V_CONV; a.lda = ctx->w2v_stride[i] * W2V_CONV;
                a.w = ctx->bw_conv[i]; a.act = 1;
                a.yb = dst; a.y_bs = (long long)L[i] * W2V_CONV; a.ldy = W2V_CONV;
                a.M = L[i]; a.N = W2V_CONV; a.K = ctx->w2v_kernel[i] * W2V_CONV;
                if (on()) tgemm(a, nb);
                std::swap(src, dst);
            }
            // interpolation to the frame count (wav2vec2.py:41-44) + feature_projection.layer_norm
            if (on()) launch_interp_ln_tm(src, (long long)L[6] * W2V_CONV, L[6], ctx->bX, (long long)Fr * W2V_CONV, Fr, nb, W2V_CONV, ctx->fp_lng, ctx->fp_lnb, 1e-5f, s);
            const long long hsT = (long long)Fr * W2V_H;            // token-major batch stride
            const long long hs = (long long)W2V_H * Fp;             // channel-major batch stride (positional conv, attention operands)
            const long long tt = (long long)nb * ((Fr + 31) / 32);
            {   // feature_projection.projection
                TGemmArgs a;
                memset(&a, 0, sizeof a);
                a.a = ctx->bX; a.a_bs = (long long)Fr * W2V_CONV; a.lda = W2V_CONV; a.w = ctx->bw_fproj; a.bias = ctx->fproj.bias;
                a.yf = ctx->bH; a.y_bs = hsT; a.ldy = W2V_H; a.M = Fr; a.N = W2V_H; a.K = W2V_CONV;
                if (on()) tgemm(a, nb);
            }
            const int PK = ctx->posconv.taps, PG = 16, PCG = W2V_H / PG;
            if (ctx->bw_pos && PK % 2 == 0) {
                // positional conv embedding (wav2vec2: Conv1d(768, 768, k=128, padding=64, groups=16), last output dropped, GELU) as 16
                // GEMMs on the bf16 token-major kernel: group g's input channels laid out [R][48] with 64 zero rows in front, so
                // that output token t is row t's 128 x 48 contiguous elements times W_g (tap-major) — 150 GFLOP per 32 clips that
                // the grouped fp32 kernel ran at 40 TFLOP/s (7.5 of the encoder's 21 ms).  Epilogue: + bias, GELU, + hidden state.
                const int R = rup(Fr + PK, 8);
                if (on()) launch_tm_to_group_bf16(ctx->bH, hsT, ctx->bXg, nb, Fr, PG, PCG, R, PK / 2, s);
                {   // ONE grouped launch (batch axis = (clip, group)): 16 launches of 160 workgroups left 40 % of the CUs idle (16 x 60 us)
                    TGemmArgs a;
                    memset(&a, 0, sizeof a);
                    a.a = ctx->bXg; a.a_bs = (long long)PG * R * PCG; a.a_gs = (long long)R * PCG; a.lda = PCG;
                    a.w = ctx->bw_pos; a.w_gs = (long long)64 * PK * PCG; a.bias = ctx->pos_bias_pad; a.act = 1;
                    a.res = ctx->bH; a.res_bs = hsT; a.ldr = W2V_H;
                    a.yf = ctx->bT; a.y_bs = hsT; a.ldy = W2V_H; a.n_store = PCG;
                    a.grp = PG; a.col_gs = PCG;
                    a.M = Fr; a.N = 64; a.K = PK * PCG;
                    if (on()) tgemm(a, nb * PG);
                }
                if (on()) launch_ln_tm(ctx->bT, nullptr, ctx->bH, ctx->bHb, ctx->enc_lng, ctx->enc_lnb, (long long)nb * Fr, W2V_H, 1e-5f, s);
            } else {
            {   // positional conv embedding (grouped, fp32 channel-major kernel) on the projected features
                if (on()) launch_tm_to_cm(ctx->bH, ctx->aH, nb, Fr, W2V_H, Fp, hs, s);
                GemmArgs a = mkargs(Fr, W2V_H / 16);
                a.groups = 16; a.ntiles_per_group = 2;
                a.nseg = 1;
                a.seg[0] = mkseg(ctx->aH, hs, Fp, W2V_H / 16, ctx->posconv.taps, ctx->posconv.taps / 2, 1, Fr, XF_NONE, ctx->posconv.w[0]);
                a.seg[0].c_group_stride = W2V_H / 16;
                a.bias = ctx->posconv.bias; a.act = ACT_GELU;
                a.y = ctx->aPOS; a.y_bstride = hs; a.y_pitch = Fp;
                if (on()) {
                    const LaunchCfg lc = audio_plan::posconv(tt);
                    launch_gemm(a, EPI_STORE, nb, lc.NB, lc.KS, s);
                    launch_cm_to_tm(ctx->aPOS, ctx->bPosT, nb, Fr, W2V_H, Fp, hs, s);
                }
            }
            if (on()) launch_ln_tm(ctx->bH, ctx->bPosT, ctx->bH, ctx->bHb, ctx->enc_lng, ctx->enc_lnb, (long long)nb * Fr, W2V_H, 1e-5f, s);
            }
            for (int l = 0; l < ctx->w2v_layers; ++l) {
                const W2VLayer& ly = ctx->layers[l];
                const said_ctx::BLayer& bl = ctx->blayers[l];
                {   // q, k, v projections -> attn.hip's operand layout
                    TGemmArgs a;
                    memset(&a, 0, sizeof a);
                    a.a = ctx->bHb; a.a_bs = hsT; a.lda = W2V_H; a.w = bl.qkv; a.bias = ly.qkv.bias;
                    a.qk = ctx->aQK; a.vt = ctx->aVT; a.v_bs = hs; a.qk_n = 2 * W2V_H; a.head_dim = W2V_HD; a.rows = Fp; a.heads2 = 2 * W2V_HEADS;
                    a.v_pitch = Fp; a.M = Fr; a.N = 3 * W2V_H; a.K = W2V_H;
                    a.sb = 1; a.direct = ctx->tgemm_direct != 0;
                    if (on()) tgemm(a, nb);
                }
                {
                    AttnArgs a;
                    a.qk = ctx->aQK; a.v = ctx->aVT; a.o = ctx->aO;
                    a.v_bstride = hs; a.o_bstride = 2 * hs; a.b0 = 0;
                    a.pitch = Fp; a.T = Fr; a.heads = W2V_HEADS; a.rows = Fp; a.scale = 0.125f;
                    const int aks = tt * W2V_HEADS <= 2048 ? 8 : -4;
                    if (aks == -4) {   // the key-split-free variant writes the out_proj operand itself: token-major bf16 [clip][frame][768]
                        a.o = reinterpret_cast<float*>(ctx->bO); a.o_bstride = Fr; a.o_mode = 2;
                    }
                    if (on()) {
                        launch_attn(a, nb, W2V_HD, aks, s, 1);
                        ++ctx->n_audio_attn[aks == -4];
                    }
                    if (on() && aks != -4) launch_cm_to_tm_bf16(ctx->aO, 2 * hs, Fp, ctx->bO, hsT, nb, Fr, W2V_H, s);
                }
                {   // out_proj + residual, then layer_norm
                    TGemmArgs a;
                    memset(&a, 0, sizeof a);
                    // (row-wise GEMMs see the pass's clips as ONE [nb * frames][768] matrix: no per-clip tile padding, 600 = 4.7 tiles of 128)
                    a.a = ctx->bO; a.a_bs = hsT; a.lda = W2V_H; a.w = bl.out; a.bias = ly.out.bias;
                    a.res = ctx->bH; a.res_bs = hsT; a.ldr = W2V_H;
                    a.yf = ctx->bT; a.y_bs = hsT; a.ldy = W2V_H; a.M = nb * Fr; a.N = W2V_H; a.K = W2V_H;
                    a.sb = 1; a.direct = ctx->tgemm_direct != 0;
                    if (on()) tgemm(a, 1);
                }
                if (on()) launch_ln_tm(ctx->bT, nullptr, ctx->bH, ctx->bHb, ly.ln1g, ly.ln1b, (long long)nb * Fr, W2V_H, 1e-5f, s);
                {   // feed_forward.intermediate_dense + GELU
                    TGemmArgs a;
                    memset(&a, 0, sizeof a);
                    a.a = ctx->bHb; a.a_bs = hsT; a.lda = W2V_H; a.w = bl.ff1; a.bias = ly.ff1.bias; a.act = 1;
                    a.yb = ctx->bF; a.y_bs = (long long)Fr * W2V_FFN; a.ldy = W2V_FFN; a.M = nb * Fr; a.N = W2V_FFN; a.K = W2V_H;
                    a.sb = 1; a.direct = ctx->tgemm_direct != 0;
                    if (on()) tgemm(a, 1);
                }
                {   // feed_forward.output_dense + residual, then final_layer_norm
                    TGemmArgs a;
                    memset(&a, 0, sizeof a);
                    a.a = ctx->bF; a.a_bs = (long long)Fr * W2V_FFN; a.lda = W2V_FFN; a.w = bl.ff2; a.bias = ly.ff2.bias;
                    a.res = ctx->bH; a.res_bs = hsT; a.ldr = W2V_H;
                    a.yf = ctx->bT; a.y_bs = hsT; a.ldy = W2V_H; a.M = nb * Fr; a.N = W2V_H; a.K = W2V_FFN;
                    a.sb = 1; a.direct = ctx->tgemm_direct != 0;
                    if (on()) tgemm(a, 1);
                }
                const bool last = l + 1 == ctx->w2v_layers && !apply_proj;   // the last LayerNorm writes the (B, frames, 768) result itself
                if (on()) launch_ln_tm(ctx->bT, nullptr, last ? out_dev + (long long)b0 * Fr * W2V_H : ctx->bH, ctx->bHb, ly.ln2g, ly.ln2b, (long long)nb * Fr, W2V_H, 1e-5f, s);
            }
            if (apply_proj) {   // diffusion.py:228-229
                TGemmArgs a;
                memset(&a, 0, sizeof a);
                a.a = ctx->bHb; a.a_bs = hsT; a.lda = W2V_H; a.w = ctx->bw_aproj; a.bias = ctx->aproj.bias;
                a.yf = out_dev + (long long)b0 * Fr * out_dim; a.y_bs = (long long)Fr * out_dim; a.ldy = out_dim; a.M = Fr; a.N = out_dim; a.K = W2V_H;
                if (on()) tgemm(a, nb);
            } else if (ctx->w2v_layers == 0 && on()) {
                HIPCHK(hipMemcpyAsync(out_dev + (long long)b0 * Fr * W2V_H, ctx->bH, (size_t)nb * Fr * W2V_H * sizeof(float), hipMemcpyDeviceToDevice, s));
            }
        }
        LAUNCHCHK();
        HIPCHK(hipGetLastError());
        return 0;
    }
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        // said_debug_option "audio_stop_after" (said_audio_encode and said_audio_extract_features; train mode ignores it): a stage is one launch call site
        // below, numbered per pass in the order documented in said_hip_debug.h; on() is asked once per site, whether or not the site launches
        int stage = 0;
        auto on = [&]() { return tp || ctx->audio_stop_after < 0 || stage++ < ctx->audio_stop_after; };
        // ---- feature extractor ----
        int pitch = rup(L[0], 32);
        long long bs = (long long)W2V_CONV * pitch;
        if (on()) launch_conv0(wav_dev + (long long)b0 * Ta, ctx->c0_w, ctx->abufA, nb, Ta, W2V_CONV, ctx->w2v_kernel[0], ctx->w2v_stride[0], L[0], pitch, bs, s);
        if (on()) launch_rownorm_gelu(ctx->abufA, ctx->c0_g, ctx->c0_b, W2V_CONV, nb, L[0], pitch, bs, 1e-5f, s);
        float* src = ctx->abufA;
        float* dst = ctx->abufB;
        for (int i = 1; i < 7; ++i) {
            const int po = rup(L[i], 32);
            const long long bo = (long long)W2V_CONV * po;
            GemmArgs a = mkargs(L[i], W2V_CONV);
            a.nseg = 1;
            a.seg[0] = mkseg(src, bs, pitch, W2V_CONV, ctx->w2v_kernel[i], 0, ctx->w2v_stride[i], L[i - 1], XF_NONE, ctx->aconv[i].w[0]);
            a.act = ACT_GELU;
            a.y = dst; a.y_bstride = bo; a.y_pitch = po;
            const LaunchCfg lc = audio_plan::conv(audio_plan::token_tiles(nb, L[i]));
            if (on()) launch_gemm(a, EPI_STORE, nb, lc.NB, lc.KS, s);
            std::swap(src, dst);
            pitch = po; bs = bo;
        }
        // ---- interpolation to the frame count (wav2vec2.py:41-44) ----
        const long long xs = (long long)W2V_CONV * Fp, hs = (long long)W2V_H * Fp;
        const float* feat = src; long long feat_bs = bs; int feat_pitch = pitch;
        const bool interp_on = on();
        if (num_frames > 0) {
            if (interp_on) launch_interp_linear(src, ctx->aX, nb, W2V_CONV, L[6], Fr, pitch, Fp, bs, xs, s);
            feat = ctx->aX; feat_bs = xs; feat_pitch = Fp;
        }
        if (features_only) {
            if (on()) launch_cm_to_tm(feat, out_dev + (long long)b0 * Fr * W2V_CONV, nb, Fr, W2V_CONV, feat_pitch, feat_bs, s);
            continue;
        }
        const long long tt = audio_plan::token_tiles(nb, Fr);
        {   // feature_projection: LayerNorm(512) -> Linear(512, 768)
            GemmArgs a = mkargs(Fr, W2V_H);
            a.nseg = 1;
            a.seg[0] = mkseg(feat, feat_bs, feat_pitch, W2V_CONV, 1, 0, 1, Fr, XF_LN, ctx->fproj.w[0]);
            a.seg[0].ln_gamma = ctx->fp_lng; a.seg[0].ln_beta = ctx->fp_lnb; a.seg[0].ln_eps = 1e-5f;
            a.bias = ctx->fproj.bias;
            a.y = ctx->aH; a.y_bstride = hs; a.y_pitch = Fp;
            const LaunchCfg lc = audio_plan::hidden(tt);
            if (on()) launch_gemm(a, EPI_STORE, nb, lc.NB, lc.KS, s);
        }
        // train mode: every mask is indexed from the call's first clip (b0 + the launch's clip), so the result does not depend on `chunk`
        const unsigned long long seed = tp ? tp->seed : 0;
        // kind: the site's bit in said_debug_option "audio_train_sites" (all set unless a test isolates a site)
        auto site = [&](int id, float p, int kind) { return drop_site(seed, id, (ctx->audio_train_sites & kind) ? p : 0.f); };
        const DropSite none = drop_site(0, 0, 0.f);
        if (tp)   // dropout on the projection, then the SpecAugment spans
            launch_drop_cm(ctx->aH, nb, W2V_H, Fr, Fp, hs, b0, site(AT_SITE_FEAT_PROJ, tp->p_feat_proj, 1),
                           tp->time_mask_dev ? tp->time_mask_dev + (long long)b0 * Fr : nullptr, ctx->mask_embed, s);
        {   // positional conv embedding: grouped Conv1d(k=128, pad=64, groups=16) + GELU; last frame dropped
            GemmArgs a = mkargs(Fr, W2V_H / 16);
            a.groups = 16; a.ntiles_per_group = 2;
            a.nseg = 1;
            a.seg[0] = mkseg(ctx->aH, hs, Fp, W2V_H / 16, ctx->posconv.taps, ctx->posconv.taps / 2, 1, Fr, XF_NONE, ctx->posconv.w[0]);
            a.seg[0].c_group_stride = W2V_H / 16;
            a.bias = ctx->posconv.bias; a.act = ACT_GELU;
            a.y = ctx->aPOS; a.y_bstride = hs; a.y_pitch = Fp;
            const LaunchCfg lc = audio_plan::posconv(tt);
            if (on()) launch_gemm(a, EPI_STORE, nb, lc.NB, lc.KS, s);
        }
        if (tp) launch_ln_drop_cm(ctx->aH, ctx->aPOS, ctx->aH, ctx->enc_lng, ctx->enc_lnb, nb, W2V_H, Fr, Fp, hs, 1e-5f, b0, none, site(AT_SITE_FRONT, tp->p_hidden, 2), s);
        else if (on()) launch_layernorm_cm(ctx->aH, ctx->aPOS, ctx->aH, ctx->enc_lng, ctx->enc_lnb, nb, W2V_H, Fr, Fp, hs, 1e-5f, s);
        const int vt_rows = Fp;
        for (int l = 0; l < ctx->w2v_layers; ++l) {
            if (tp && (tp->skip_layers >> l & 1u)) continue;   // LayerDrop: the layer is the identity for the whole batch
            const W2VLayer& ly = ctx->layers[l];
            {
                GemmArgs a = mkargs(Fr, 3 * W2V_H);
                a.nseg = 1;
                a.seg[0] = mkseg(ctx->aH, hs, Fp, W2V_H, 1, 0, 1, Fr, XF_NONE, ly.qkv.w[0]);
                a.bias = ly.qkv.bias;
                a.tm_tiles = 2 * W2V_H / 32;
                a.vt = ctx->aQK; a.vt_heads = 2 * W2V_HEADS; a.vt_dim = W2V_HD; a.vt_rows = vt_rows;
                a.y = ctx->aVT - (long long)a.tm_tiles * 32 * Fp; a.y_bstride = hs; a.y_pitch = Fp;
                const LaunchCfg lc = audio_plan::qkv(tt);
                if (on()) launch_gemm(a, EPI_QKV, nb, lc.NB, lc.KS, s);
            }
            {
                AttnArgs a;
                a.qk = ctx->aQK; a.v = ctx->aVT; a.o = ctx->aO;
                a.v_bstride = hs; a.o_bstride = 2 * hs; a.b0 = 0;
                a.pitch = Fp; a.T = Fr; a.heads = W2V_HEADS; a.rows = vt_rows; a.scale = 0.125f;
                const int mode = sp_on(ctx, ctx->attn_split) ? 2 : 0;
                const DropSite pd = site(at_site_layer(l, 0), tp ? tp->p_attention : 0.f, 4);
                if (pd.p > 0.f) {   // (training batches are small: the key split stays on, eight waves or four)
                    launch_attn_drop(a, nb, audio_plan::attn_slices(tt, true), s, mode, b0, pd);
                } else if (on()) {
                    const int ks = audio_plan::attn_slices(tt);
                    launch_attn(a, nb, W2V_HD, ks, s, mode);
                    ++ctx->n_audio_attn_f32[ks == 8 ? 0 : (ks == 4 ? 1 : 2)];
                }
            }
            {
                GemmArgs a = mkargs(Fr, W2V_H);
                a.nseg = 1;
                a.seg[0] = mkseg(ctx->aO, 2 * hs, Fp, W2V_H, 1, 0, 1, Fr, XF_NONE, ly.out.w[0]);
                a.bias = ly.out.bias;
                if (!tp) { a.res_kind = RES_PLAIN; a.res = ctx->aH; a.res_bstride = hs; a.res_pitch = Fp; }   // train mode: the LayerNorm kernel adds the residual, behind the dropout
                a.y = ctx->aT; a.y_bstride = hs; a.y_pitch = Fp;
                const LaunchCfg lc = audio_plan::hidden(tt);
                if (on()) launch_gemm(a, EPI_STORE, nb, lc.NB, lc.KS, s);
            }
            if (tp) launch_ln_drop_cm(ctx->aT, ctx->aH, ctx->aH, ly.ln1g, ly.ln1b, nb, W2V_H, Fr, Fp, hs, 1e-5f, b0, site(at_site_layer(l, 1), tp->p_hidden, 8), none, s);
            else if (on()) launch_layernorm_cm(ctx->aT, nullptr, ctx->aH, ly.ln1g, ly.ln1b, nb, W2V_H, Fr, Fp, hs, 1e-5f, s);
            {
                GemmArgs a = mkargs(Fr, W2V_FFN);
                a.nseg = 1;
                a.seg[0] = mkseg(ctx->aH, hs, Fp, W2V_H, 1, 0, 1, Fr, XF_NONE, ly.ff1.w[0]);
                a.bias = ly.ff1.bias; a.act = ACT_GELU;
                a.y = ctx->aF; a.y_bstride = (long long)W2V_FFN * Fp; a.y_pitch = Fp;
                const LaunchCfg lc = audio_plan::ffn(tt);
                if (on()) launch_gemm(a, EPI_STORE, nb, lc.NB, lc.KS, s);
            }
            if (tp) launch_drop_cm(ctx->aF, nb, W2V_FFN, Fr, Fp, (long long)W2V_FFN * Fp, b0, site(at_site_layer(l, 2), tp->p_activation, 16), nullptr, nullptr, s);
            {
                GemmArgs a = mkargs(Fr, W2V_H);
                a.nseg = 1;
                a.seg[0] = mkseg(ctx->aF, (long long)W2V_FFN * Fp, Fp, W2V_FFN, 1, 0, 1, Fr, XF_NONE, ly.ff2.w[0]);
                a.bias = ly.ff2.bias;
                if (!tp) { a.res_kind = RES_PLAIN; a.res = ctx->aH; a.res_bstride = hs; a.res_pitch = Fp; }   // train mode: the LayerNorm kernel adds the residual, behind the dropout
                a.y = ctx->aT; a.y_bstride = hs; a.y_pitch = Fp;
                const LaunchCfg lc = audio_plan::hidden(tt);
                if (on()) launch_gemm(a, EPI_STORE, nb, lc.NB, lc.KS, s);
            }
            if (tp) launch_ln_drop_cm(ctx->aT, ctx->aH, ctx->aH, ly.ln2g, ly.ln2b, nb, W2V_H, Fr, Fp, hs, 1e-5f, b0, site(at_site_layer(l, 3), tp->p_hidden, 32), none, s);
            else if (on()) launch_layernorm_cm(ctx->aT, nullptr, ctx->aH, ly.ln2g, ly.ln2b, nb, W2V_H, Fr, Fp, hs, 1e-5f, s);
        }
        const float* fin = ctx->aH; long long fin_bs = hs;
        if (apply_proj) {  // diffusion.py:228-229
            GemmArgs a = mkargs(Fr, out_dim);
            a.nseg = 1;
            a.seg[0] = mkseg(ctx->aH, hs, Fp, W2V_H, 1, 0, 1, Fr, XF_NONE, ctx->aproj.w[0]);
            a.bias = ctx->aproj.bias;
            a.y = ctx->aT; a.y_bstride = (long long)out_dim * Fp; a.y_pitch = Fp;
            const LaunchCfg lc = audio_plan::proj(tt);
            if (on()) launch_gemm(a, EPI_STORE, nb, lc.NB, lc.KS, s);
            fin = ctx->aT; fin_bs = (long long)out_dim * Fp;
        }
        if (on()) launch_cm_to_tm(fin, out_dev + (long long)b0 * Fr * out_dim, nb, Fr, out_dim, Fp, fin_bs, s);
    }
    LAUNCHCHK();
    HIPCHK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int said_audio_encode(said_ctx* ctx, const float* wav_dev, int B, int Ta, int num_frames, int apply_proj, float* out_dev,
                      int* out_frames, void* stream) {
    return audio_encode(ctx, wav_dev, B, Ta, num_frames, apply_proj, nullptr, out_dev, out_frames, stream);
}

int said_audio_encode_train(said_ctx* ctx, const float* wav_dev, int B, int Ta, int num_frames, int apply_proj,
                            const said_audio_train_params* tp, float* out_dev, int* out_frames, void* stream) {
    if (check_ready(ctx)) return -1;
    if (!tp) return fail(ctx, "said_audio_encode_train: params is null");
    if (ctx->bf16_mode)
        return fail(ctx, "said_audio_encode_train: the context is in bf16 mode; the train-mode encoder runs on the fp32 route only (said_set_precision)");
    for (const float p : {tp->p_feat_proj, tp->p_hidden, tp->p_attention, tp->p_activation})
        if (!(p >= 0.f && p < 1.f)) return fail(ctx, "said_audio_encode_train: dropout probability %g is outside [0, 1)", (double)p);
    if (tp->time_mask_dev && !ctx->mask_embed)
        return fail(ctx, "said_audio_encode_train: a time mask needs audio_encoder.masked_spec_embed, which was not loaded");
    if (ctx->w2v_layers > 32) return fail(ctx, "said_audio_encode_train: skip_layers holds 32 layers, the encoder has %d", ctx->w2v_layers);
    return audio_encode(ctx, wav_dev, B, Ta, num_frames, apply_proj, tp, out_dev, out_frames, stream);
}

int said_audio_extract_features(said_ctx* ctx, const float* wav_dev, int B, int Ta, int num_frames, float* out_dev, int* out_frames, void* stream) {
    if (check_ready(ctx)) return -1;
    if (ctx->bf16_mode)
        return fail(ctx, "said_audio_extract_features: the context is in bf16 mode; the features come from the fp32 route only (said_set_precision)");
    return audio_encode(ctx, wav_dev, B, Ta, num_frames, 0, nullptr, out_dev, out_frames, stream, true);
}

}  // extern "C"
