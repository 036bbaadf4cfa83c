// sched_math.h — the per-element update that ends a denoise step.  step_update<SF> (at the end of this file) is the ONE statement of the sequence
// non-finite note -> optional dump of the pre-step latent -> DDIM / DDPM / DPM-Solver++ update -> eta noise -> editing-mask blend; every kernel that updates latents calls it: the stand-alone
// scheduler kernels (misc.hip: sched_step_kernel, step_flat_kernel) and the fused output-conv + scheduler kernels (out_sched.hip: OutEpilogue).
// The callers keep their loads, stores and addressing; the primitives (ddim_prev, solver_prev, mask_blend, philox_normal) are called from nowhere else.
#pragma once
#include <hip/hip_runtime.h>

namespace said {

// ------------------------------------------------------------------------------------------
// Scheduler arithmetic.  Every operation is an explicitly rounded fp32 op in diffusers'
// DDIMScheduler.step order (no FMA contraction), so given the same eps the result is
// bit-identical to the CPU restatement (oracle/scheduler.py).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float cfg_combine(float e_c, float e_u, float s) {
    // diffusion.py:430-434: noise_pred_audio + guidance_scale * (noise_pred_audio - noise_pred_uncond)
    return __fadd_rn(e_c, __fmul_rn(s, __fsub_rn(e_c, e_u)));
}
__device__ __forceinline__ float ddim_prev(float model_out, float x, const float* cf, int pred) {
    const float sa = cf[0], sb = cf[1], sap = cf[2], dir = cf[3];
    float x0, e;
    if (pred == 0) {
        x0 = __fdiv_rn(__fsub_rn(x, __fmul_rn(sb, model_out)), sa);
        e = model_out;
    } else if (pred == 1) {
        x0 = model_out;
        e = __fdiv_rn(__fsub_rn(x, __fmul_rn(sa, x0)), sb);
    } else {
        x0 = __fsub_rn(__fmul_rn(sa, x), __fmul_rn(sb, model_out));
        e = __fadd_rn(__fmul_rn(sa, model_out), __fmul_rn(sb, x));
    }
    x0 = (x0 != x0) ? x0 : fminf(fmaxf(x0, -1.0f), 1.0f);  // clip_sample=True, range 1.0 (torch.clamp keeps a NaN; fminf / fmaxf alone would turn it into -1)
    return __fadd_rn(__fmul_rn(sap, x0), __fmul_rn(dir, e));
}
// ------------------------------------------------------------------------------------------
// DDPM and DPM-Solver++(2M) (diffusers 0.19 DDPMScheduler.step, DPMSolverMultistepScheduler.step).  The solver is per row:
// coef column 7 (SAID_COEF_SOLVER) holds 1 = DDPM, 2 = DPM-Solver++ first order, 3 = second order (0 = DDIM: ddim_prev).
// Columns 0 / 1 are the x0 conversion pair (sqrt(alpha_prod_t), sqrt(1 - alpha_prod_t)); then
//   DDPM:  2 = pred_original_sample_coeff, 3 = current_sample_coeff, 4 = std (the caller adds std * noise, as for DDIM's sigma)
//   DPM:   2 = sigma_t / sigma_s0, 3 = alpha_t * (exp(-h) - 1), 4 = 1 / r0 (order 2)
// The previous step's x0 (order 2's m1) lives in `x0_prev`; every DPM row returns its own x0 in `x0_out` for the next step.
// ------------------------------------------------------------------------------------------
constexpr int SOLVER_DDIM = 0, SOLVER_DDPM = 1, SOLVER_DPM1 = 2, SOLVER_DPM2 = 3;
__device__ __forceinline__ int solver_code(const float* cf) { return (int)cf[7]; }
__device__ __forceinline__ float solver_prev(float model_out, float x, const float* cf, int pred, float x0_prev, float& x0_out) {
    const float sa = cf[0], sb = cf[1];
    const int code = solver_code(cf);
    float x0;
    if (pred == 0) x0 = __fdiv_rn(__fsub_rn(x, __fmul_rn(sb, model_out)), sa);
    else if (pred == 1) x0 = model_out;
    else x0 = __fsub_rn(__fmul_rn(sa, x), __fmul_rn(sb, model_out));
    if (code == SOLVER_DDPM) {
        x0 = (x0 != x0) ? x0 : fminf(fmaxf(x0, -1.0f), 1.0f);   // clip_sample=True, range 1.0 (NaN kept, as torch.clamp)
        return __fadd_rn(__fmul_rn(cf[2], x0), __fmul_rn(cf[3], x));
    }
    x0_out = x0;
    float prev = __fsub_rn(__fmul_rn(cf[2], x), __fmul_rn(cf[3], x0));
    if (code == SOLVER_DPM2) {   // - 0.5 * (alpha_t * (exp(-h) - 1)) * ((1 / r0) * (m0 - m1)); the halving is exact
        const float d1 = __fmul_rn(cf[4], __fsub_rn(x0, x0_prev));
        prev = __fsub_rn(prev, __fmul_rn(0.5f * cf[3], d1));
    }
    return prev;
}

// The model output of a step is not finite: remember the first such step (said_numeric_status).  fp32 mode multiplies on split-fp16 operands
// (split_f16.h: |x| < 65504); an operand beyond that becomes inf / NaN in its product and reaches this point through every later layer.
__device__ __forceinline__ void note_nonfinite(float model_out, int* status, int step) {
    if (status && !(fabsf(model_out) <= 3.4028234663852886e38f)) atomicCAS(status, 0, step + 1);
}
__device__ __forceinline__ float mask_blend(float prev, float init, float enoise, float mask, const float* cf) {
    // diffusion.py:446-456: add_noise(init, noise, t_next) * mask + latents * (1 - mask)
    const float noisy = __fadd_rn(__fmul_rn(cf[5], init), __fmul_rn(cf[6], enoise));
    return __fadd_rn(__fmul_rn(noisy, mask), __fmul_rn(prev, __fsub_rn(1.0f, mask)));
}


// ------------------------------------------------------------------------------------------
// eta > 0 variance noise generated on the device (said_loop_params::use_step_noise == 2): the reference draws
// `randn(model_output.shape)` inside DDIMScheduler.step once per step (diffusion.py:441-443) — a stream no other
// implementation reproduces bit for bit — so the product path draws its own standard normals, counter-based:
// Philox4x32-10 (Salmon et al., SC'11) with key = the call's 64-bit seed and counter = (element index in (B, T, C)
// order, step, 0, 0); the first two output words make one Box-Muller normal.  Layout- and launch-shape-independent,
// nothing is stored: no (N, B, T, C) buffer exists.  said_philox_normal fills a tensor with exactly these values.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ float philox_normal(unsigned seed_lo, unsigned seed_hi, unsigned step, unsigned elem) {
    unsigned r[4];
    philox4x32_10(elem, step, 0u, 0u, seed_lo, seed_hi, r);
    const float u1 = ((float)(r[0] >> 8) + 1.0f) * 5.9604644775390625e-8f;    // (0, 1], 24 bits
    const float u2 = (float)(r[1] >> 8) * 5.9604644775390625e-8f;             // [0, 1)
    return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

// ------------------------------------------------------------------------------------------
// One element's update.  The caller has loaded the operands; it stores `prev` over x and, for DPM-Solver++ rows (solver_code >= SOLVER_DPM1), `x0`
// into the history that the next step's `x0_prev` is read from (only second-order rows read it).
// ------------------------------------------------------------------------------------------
struct StepNoise {         // the eta noise of one element: cf[4] * ...
    bool from_tensor;      // ... `value`, loaded from the step-noise tensor
    float value;
    const unsigned* seed;  // ... else, if not null, philox_normal(seed, step, elem0 + elem) drawn here
    unsigned elem0, elem;  // element index in (B, T, C) order: of the call's first clip within the whole batch, of this element within the call
};
struct StepResult { float prev, x0; };
// SF (solver family of the table): 0 = DDIM rows (ddim_prev), 1 = DDPM / DPM-Solver++ rows (solver_prev).  e: the model output after guidance.
// dump_to (addressed by the caller, or null): the pre-step latent / latent_scale is stored there.
template <int SF>
__device__ __forceinline__ StepResult step_update(float e, float x, const float* cf, int pred, float x0_prev, int step, const StepNoise& nz, bool masked, float init,
                                                  float enoise, float mask, int* status, bool dump = false, float* dump_to = nullptr, float latent_scale = 1.f) {
    note_nonfinite(e, status, step);
    if (dump) *dump_to = x / latent_scale;
    StepResult r = {0.f, 0.f};
    if constexpr (SF == 0) r.prev = ddim_prev(e, x, cf, pred);
    else r.prev = solver_prev(e, x, cf, pred, x0_prev, r.x0);
    if (nz.from_tensor) r.prev = __fadd_rn(r.prev, __fmul_rn(cf[4], nz.value));
    else if (nz.seed) r.prev = __fadd_rn(r.prev, __fmul_rn(cf[4], philox_normal(nz.seed[0], nz.seed[1], (unsigned)step, nz.elem0 + nz.elem)));
    if (masked) r.prev = mask_blend(r.prev, init, enoise, mask, cf);
    return r;
}

}  // namespace said
