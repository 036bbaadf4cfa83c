// blendshape_qp.hip — the pseudo-GT blendshape-coefficient fit (said/optimize/blendshape_coeffs.py, script/optimize_blendshape_coeffs.py):
// the right-hand sides q_t = B_delta' (n - v_t) of every frame, and a batched primal-dual interior-point solver of
//
//     minimise  sum_t 1/2 w_t' P w_t + q_t' w_t   s.t.  0 <= w_t <= 1,  -delta <= w_t - w_{t+1} <= delta        (P = B_delta' B_delta, K x K)
//
// float64 throughout.  DESIGN.md section 13 has the derivation; in brief:
//
// * Every inequality is a row of G x <= h with slack s and dual z.  The Newton system of one Mehrotra iteration reduces to
//   M dx = b with M = I (x) P + G' diag(z / s) G: block-tridiagonal, diagonal blocks P + diag(a_t), off-diagonal blocks -diag(d_t), where d_t
//   collects the two difference rows of frames (t, t + 1) and a_t the box rows plus d_{t-1} + d_t.
// * The block elimination S_t = A_t - D_{t-1} S_{t-1}^-1 D_{t-1} cancels catastrophically once d grows large (an active difference
//   constraint): it is formed as S_t = C_t + D_t, C_t = P + diag(box_t) + E_{t-1}, E_{t-1} = (C_{t-1}^-1 + D_{t-1}^-1)^-1, which equals
//   D - D (C + D)^-1 D without the cancellation.  Three symmetric sweeps (Gauss-Jordan inversions without pivoting, stable on the
//   positive-definite blocks) per frame; S_t^-1 is kept in the workspace for the forward and backward block substitutions.
// * One step of iterative refinement on the dual residual P dx + G' dz + r_d per solve: without it the dual residual stalls near 1e-11
//   as z / s spans 1e20 (the direction's error along active constraints is amplified by z / s into dz).
// * P and q are scaled by a power of two (exact) chosen from P's largest diagonal entry, so the iteration sees the same numbers
//   whatever units the meshes are in; the duals are scaled back on output.
//
// Layout: one 64-lane workgroup (one wave) per sequence runs the whole iteration loop; K x K blocks live in LDS, padded to KP = 32 or 64.
// Lane (c = lane % KP, h = lane / KP) owns column c of rows h, h + H, h + 2H, ... (H = 64 / KP): with a symmetric matrix this lane's
// partial of (M v)_c runs over its rows in order, and the KP = 32 halves are added once.  Per-frame vectors are handled by lanes h == 0,
// c < K; elementwise passes over a sequence's T x K values by all 64 lanes.  Every sum runs in a fixed order; the workgroup of a sequence
// reads only that sequence's data, so its result does not depend on the batch it rides in.  No atomics.
//
// Why VALU and not v_mfma_f64_16x16x4_f64: the chain of one sequence is a sequence of rank-1 sweep updates of a 32 x 32 block (a matrix
// product nowhere), each step a handful of FMAs per lane between two barriers; what bounds it is the latency of that chain, not a
// floating-point rate.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/said_optimize.h"
#include "engine_internal.h"

namespace {

// per-frame vectors of the workspace (each FK = frames * K doubles)
enum Vec {
    X, SLO, SHI, SDP, SDM, ZLO, ZHI, ZDP, ZDM,   // iterate: primal, slacks and duals of the four inequality families
    RD, RLO, RHI, RDP, RDM,                       // residuals: dual, primal per family
    DX, DS0, DZ0 = DS0 + 4,                       // search direction
    CX = DZ0 + 4, CS0, CZ0 = CS0 + 4,             // refinement correction
    WB = CZ0 + 4, DD, BV, GG, RC0, E1 = RC0 + 4,  // box weights, difference weights, rhs, forward solution, complementarity rhs, refinement rhs
    NV
};

constexpr int RHS_F = 32;    // frames per workgroup of the rhs kernel
constexpr int RHS_CH = 64;   // coordinates per LDS chunk

// q (nframes, K) = B_delta' (n - v): thread (kq = tid & 31, fg = tid >> 5) accumulates k = kq, kq + 32 for frames fg + 8 j, j < 4, over
// every coordinate in order; the chunk of B_delta and of (n - v) of the workgroup's frames is staged in LDS.
__global__ __launch_bounds__(256) void rhs_kernel(const double* __restrict__ bdelta, const double* __restrict__ neutral, const double* __restrict__ verts,
                                                  long long nframes, long long n3v, int K, double* __restrict__ q) {
    __shared__ double Bs[RHS_CH][64];
    __shared__ double Es[RHS_F][RHS_CH + 1];
    const int tid = threadIdx.x, kq = tid & 31, fg = tid >> 5;
    const long long fb = (long long)blockIdx.x * RHS_F;
    double a0[4] = {0.0, 0.0, 0.0, 0.0}, a1[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long i0 = 0; i0 < n3v; i0 += RHS_CH) {
        for (int idx = tid; idx < RHS_CH * 64; idx += 256) {
            const int i = idx >> 6, k = idx & 63;
            Bs[i][k] = (k < K && i0 + i < n3v) ? bdelta[(i0 + i) * K + k] : 0.0;
        }
        for (int idx = tid; idx < RHS_F * RHS_CH; idx += 256) {
            const int f = idx / RHS_CH, i = idx % RHS_CH;
            const long long fr = fb + f;
            Es[f][i] = (fr < nframes && i0 + i < n3v) ? neutral[i0 + i] - verts[fr * n3v + i0 + i] : 0.0;
        }
        __syncthreads();
        for (int i = 0; i < RHS_CH; ++i) {
            const double b0 = Bs[i][kq], b1 = Bs[i][kq + 32];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double e = Es[fg + 8 * j][i];
                a0[j] = fma(b0, e, a0[j]);
                a1[j] = fma(b1, e, a1[j]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long fr = fb + fg + 8 * j;
        if (fr < nframes) {
            if (kq < K) q[fr * K + kq] = a0[j];
            if (kq + 32 < K) q[fr * K + kq + 32] = a1[j];
        }
    }
}

struct QPArgs {
    const double* P;        // (nbasis, KP, KP): P / scale, zero beyond K
    const double* scale;    // (nbasis) powers of two
    const long long* offs;  // (nseq + 1) frame offsets
    const int* basis;       // (nseq)
    const double* q;        // (F, K)
    double* ws;             // NV vectors of FK doubles, then (F, KP * KP) block inverses
    double* w;              // (F, K)
    double* z;              // (F, 4, K) or null
    int* status;
    int* iters;
    double* resid;          // (nseq, 3)
    long long FK;
    int K, coupled, max_iter;
    double delta, tol;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);   // a + b == b + a: every lane ends with the same bits
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
    return v;
}

template <int KP>
struct Solver {
    static constexpr int H = 64 / KP, R = KP * KP / 64;
    const QPArgs a;
    double* base;   // this sequence's element 0 of workspace vector 0
    long long f0;
    double* sinv;
    const double* q;
    double *Pm, *Cm, *Wm, *Em, *v0, *v1, *cb;
    int T, K, nd, lane, c, h;
    long long n;
    double delta, isc;

    __device__ Solver(const QPArgs& args, double* lds) : a(args) {
        const int s = blockIdx.x;
        f0 = a.offs[s];
        T = (int)(a.offs[s + 1] - f0);
        K = a.K;
        nd = a.coupled ? T - 1 : 0;
        n = (long long)T * K;
        base = a.ws + f0 * K;
        sinv = a.ws + (long long)NV * a.FK + f0 * KP * KP;
        q = a.q + f0 * K;
        lane = threadIdx.x;
        c = lane % KP;
        h = lane / KP;
        delta = a.delta;
        isc = 1.0 / a.scale[a.basis[s]];
        Pm = lds;
        Cm = lds + KP * KP;
        Wm = lds + 2 * KP * KP;
        Em = lds + 3 * KP * KP;
        v0 = lds + 4 * KP * KP;
        v1 = v0 + KP;
        cb = v1 + KP;
        const double* Pg = a.P + (long long)a.basis[s] * KP * KP;
        for (int i = lane; i < KP * KP; i += 64) Pm[i] = Pg[i];
        __syncthreads();
    }

    __device__ double* Vp(int i) const { return base + (long long)i * a.FK; }
    __device__ bool vlane() const { return h == 0 && c < K; }
    __device__ bool act(long long e) const { return e / K < nd; }   // a difference row exists for (t, t + 1)
    __device__ double qs(long long e) const { return q[e] * isc; }

    // (M v)_c for a symmetric KP x KP matrix M (LDS or global) and v in LDS; valid in the lanes with h == 0
    __device__ double matvec(const double* M, const double* v) const {
        double p = 0.0;
#pragma unroll 4
        for (int r = 0; r < R; ++r) {
            const int i = h + H * r;
            p = fma(M[i * KP + c], v[i], p);
        }
        if (KP == 32) p = p + __shfl_xor(p, 32);
        return p;
    }

    // A <- A^-1 in place (symmetric sweep over the first K pivots; rows and columns beyond K are zero and stay so).  Column k is copied to
    // cb before the update, so every lane reads the pivot row and column as they were.
    __device__ void inv_sweep(double* A) const {
        for (int k = 0; k < K; ++k) {
            const double pinv = 1.0 / A[k * KP + k];
            const double ckp = A[k * KP + c] * pinv;
            if (c == k) {
#pragma unroll 4
                for (int r = 0; r < R; ++r) cb[h + H * r] = A[(h + H * r) * KP + k];
            }
            __syncthreads();
#pragma unroll 4
            for (int r = 0; r < R; ++r) {
                const int i = h + H * r, idx = i * KP + c;
                const double ci = cb[i];
                double v;
                if (i == k) v = (c == k) ? -pinv : ckp;
                else if (c == k) v = ci * pinv;
                else v = fma(-ci, ckp, A[idx]);
                A[idx] = v;
            }
            __syncthreads();
        }
#pragma unroll 4
        for (int r = 0; r < R; ++r) {
            const int idx = (h + H * r) * KP + c;
            A[idx] = -A[idx];
        }
        __syncthreads();
    }

    // (G' u)_e for the four families u[0..3] at flat index e
    __device__ double gt(const double* u0, const double* u1, const double* u2, const double* u3, long long e) const {
        double g = u1[e] - u0[e];
        if (act(e)) g += u2[e] - u3[e];
        if (e >= K && act(e - K)) g -= u2[e - K] - u3[e - K];
        return g;
    }
    // (G x)_e of family f (0: -x, 1: x, 2: x_t - x_{t+1}, 3: x_{t+1} - x_t; 0 without a difference row)
    __device__ double gx(const double* x, int f, long long e) const {
        if (f == 0) return -x[e];
        if (f == 1) return x[e];
        if (!act(e)) return 0.0;
        const double dlt = x[e] - x[e + K];
        return f == 2 ? dlt : -dlt;
    }

    // residual: out = P x_t + q_t + (G' z)_t for every frame, in order, returning this lane's part of 1/2 x' P x + q' x;
    // otherwise out = -r_d - P x_t - (G' dz)_t (the refinement's right-hand side)
    __device__ double frames_px(const double* x, double* out, bool residual) const {
        double obj = 0.0;
        for (int t = 0; t < T; ++t) {
            double* v = (t & 1) ? v1 : v0;
            if (c < KP && h == 0) v[c] = c < K ? x[(long long)t * K + c] : 0.0;
            __syncthreads();
            const double y = matvec(Pm, v);
            if (vlane()) {
                const long long e = (long long)t * K + c;
                if (residual) {
                    out[e] = y + qs(e) + gt(Vp(ZLO), Vp(ZHI), Vp(ZDP), Vp(ZDM), e);
                    obj = obj + (0.5 * x[e] * y + qs(e) * x[e]);
                } else {
                    out[e] = -Vp(RD)[e] - y - gt(Vp(DZ0), Vp(DZ0 + 1), Vp(DZ0 + 2), Vp(DZ0 + 3), e);
                }
            }
        }
        __syncthreads();
        return obj;
    }

    // block factorisation of M into the S_t^-1 of the workspace
    __device__ void factor() {
        for (int r = 0; r < R; ++r) Em[(h + H * r) * KP + c] = 0.0;
        __syncthreads();
        for (int t = 0; t < T; ++t) {
            const double* wb = Vp(WB) + (long long)t * K;
            const double* dd = Vp(DD) + (long long)t * K;
            const bool link = t < nd;
#pragma unroll 4
            for (int r = 0; r < R; ++r) {
                const int i = h + H * r, idx = i * KP + c;
                double v = 0.0;
                if (i < K && c < K) {
                    v = Pm[idx] + Em[idx];
                    if (i == c) v = v + wb[i];
                }
                Cm[idx] = v;
                Wm[idx] = (link && i == c && i < K) ? v + dd[i] : v;
            }
            __syncthreads();
            inv_sweep(Wm);   // S_t^-1
            double* st = sinv + (long long)t * KP * KP;
#pragma unroll 4
            for (int r = 0; r < R; ++r) {
                const int idx = (h + H * r) * KP + c;
                st[idx] = Wm[idx];
            }
            if (link) {
                inv_sweep(Cm);   // C_t^-1, then E_t = (C_t^-1 + D_t^-1)^-1
#pragma unroll 4
                for (int r = 0; r < R; ++r) {
                    const int i = h + H * r;
                    if (i == c && i < K) Cm[i * KP + c] = Cm[i * KP + c] + 1.0 / dd[i];
                }
                __syncthreads();
                inv_sweep(Cm);
#pragma unroll 4
                for (int r = 0; r < R; ++r) {
                    const int idx = (h + H * r) * KP + c;
                    Em[idx] = Cm[idx];
                }
                __syncthreads();
            }
        }
    }

    // M dx = b by forward and backward block substitution (b in BV); dx to Vp(dx)
    __device__ void substitute(double* dx) {
        double* gg = Vp(GG);
        const double* b = Vp(BV);
        const double* dd = Vp(DD);
        if (h == 0) v0[c] = c < K ? b[c] : 0.0;
        __syncthreads();
        for (int t = 0; t < T; ++t) {
            double* v = (t & 1) ? v1 : v0;
            double* vn = (t & 1) ? v0 : v1;
            const double g = matvec(sinv + (long long)t * KP * KP, v);
            if (vlane()) {
                const long long e = (long long)t * K + c;
                gg[e] = g;
                if (t + 1 < T) vn[c] = b[e + K] + dd[e] * g;
            } else if (h == 0) {
                vn[c] = 0.0;
            }
            __syncthreads();
        }
        double xn = 0.0;
        if (vlane()) {
            xn = gg[(long long)(T - 1) * K + c];
            dx[(long long)(T - 1) * K + c] = xn;
        }
        for (int t = T - 2; t >= 0; --t) {
            double* v = (t & 1) ? v1 : v0;
            if (h == 0) v[c] = c < K ? dd[(long long)t * K + c] * xn : 0.0;
            __syncthreads();
            const double y = matvec(sinv + (long long)t * KP * KP, v);
            if (vlane()) {
                const long long e = (long long)t * K + c;
                xn = gg[e] + y;
                dx[e] = xn;
            }
        }
        __syncthreads();
    }

    // one Newton solve: full (r_d, r_p, rc in RC0..) into DX / DS0 / DZ0, or the refinement correction (rhs E1, r_p = rc = 0) into CX / CS0 / CZ0
    __device__ void solve1(bool correction) {
        const int ox = correction ? CX : DX, os = correction ? CS0 : DS0, oz = correction ? CZ0 : DZ0;
        double* b = Vp(BV);
        for (long long e = lane; e < n; e += 64) {
            if (correction) {
                b[e] = Vp(E1)[e];
            } else {
                // u_f = (rc_f - z_f r_f) / s_f at e and at e - K (the previous frame's difference rows)
                double u[4], up[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int f = 0; f < 4; ++f) {
                    const bool on = f < 2 || act(e);
                    u[f] = on ? (Vp(RC0 + f)[e] - Vp(ZLO + f)[e] * Vp(RLO + f)[e]) / Vp(SLO + f)[e] : 0.0;
                    if (f >= 2 && e >= K && act(e - K)) up[f] = (Vp(RC0 + f)[e - K] - Vp(ZLO + f)[e - K] * Vp(RLO + f)[e - K]) / Vp(SLO + f)[e - K];
                }
                b[e] = -Vp(RD)[e] + ((u[1] - u[0]) + (u[2] - u[3]) - (up[2] - up[3]));
            }
        }
        __syncthreads();
        substitute(Vp(ox));
        for (long long e = lane; e < n; e += 64) {
            for (int f = 0; f < 4; ++f) {
                const bool on = f < 2 || act(e);
                double ds = 0.0, dz = 0.0;
                if (on) {
                    if (correction) {
                        ds = -gx(Vp(ox), f, e);
                        dz = -(Vp(ZLO + f)[e] * ds) / Vp(SLO + f)[e];
                    } else {
                        ds = -Vp(RLO + f)[e] - gx(Vp(ox), f, e);
                        dz = (-Vp(RC0 + f)[e] - Vp(ZLO + f)[e] * ds) / Vp(SLO + f)[e];
                    }
                }
                Vp(os + f)[e] = ds;
                Vp(oz + f)[e] = dz;
            }
        }
        __syncthreads();
    }

    // the search direction for complementarity rhs RC0..: one solve and one refinement step on the dual residual
    __device__ void solve() {
        solve1(false);
        frames_px(Vp(DX), Vp(E1), false);   // E1 = -r_d - P dx - G' dz
        solve1(true);
        for (long long e = lane; e < n; e += 64) {
            Vp(DX)[e] += Vp(CX)[e];
            for (int f = 0; f < 8; ++f) Vp(DS0 + f)[e] += Vp(CS0 + f)[e];
        }
        __syncthreads();
    }

    // largest step in (0, 1] that keeps every slack and dual non-negative along (DS0.., DZ0..)
    __device__ double max_step() const {
        double al = 1.0;
        for (long long e = lane; e < n; e += 64)
            for (int f = 0; f < 8; ++f) {
                if (f % 4 >= 2 && !act(e)) continue;
                const double d = Vp(DS0 + f)[e];
                if (d < 0.0) al = fmin(al, -Vp(SLO + f)[e] / d);
            }
        return wave_min(al);
    }

    __device__ void run() {
        const int s = blockIdx.x;
        // start: the box's centre, unit duals; the difference rows of the last frame (and all when uncoupled) are held at s = 1, z = 0
        for (long long e = lane; e < n; e += 64) {
            const bool on = act(e);
            Vp(X)[e] = 0.5;
            Vp(SLO)[e] = Vp(SHI)[e] = 0.5;
            Vp(ZLO)[e] = Vp(ZHI)[e] = 1.0;
            Vp(SDP)[e] = Vp(SDM)[e] = on ? delta : 1.0;
            Vp(ZDP)[e] = Vp(ZDM)[e] = on ? 1.0 : 0.0;
            Vp(RDP)[e] = Vp(RDM)[e] = 0.0;
        }
        double qn = 0.0, pn = 0.0;
        for (long long e = lane; e < n; e += 64) qn = fmax(qn, fabs(qs(e)));
        for (int i = lane; i < KP * KP; i += 64) pn = fmax(pn, fabs(Pm[i]));
        qn = wave_max(qn);
        pn = wave_max(pn);
        const double m = 2.0 * (double)n + 2.0 * (double)nd * K;
        const double dscale = 1.0 + fmax(qn, pn), pscale = 1.0 + fmax(1.0, delta);
        __syncthreads();
        int it = 0, st = SAID_OPTIMIZE_MAX_ITER;
        double pres = 0.0, dres = 0.0, gres = 0.0;
        for (;; ++it) {
            const double obj = wave_sum(frames_px(Vp(X), Vp(RD), true));
            double rp = 0.0, rdm = 0.0, gap = 0.0;
            for (long long e = lane; e < n; e += 64) {
                rdm = fmax(rdm, fabs(Vp(RD)[e]));
                const double x = Vp(X)[e];
                const double r0 = -x + Vp(SLO)[e], r1 = x + Vp(SHI)[e] - 1.0;
                Vp(RLO)[e] = r0;
                Vp(RHI)[e] = r1;
                rp = fmax(rp, fmax(fabs(r0), fabs(r1)));
                gap = gap + (Vp(SLO)[e] * Vp(ZLO)[e] + Vp(SHI)[e] * Vp(ZHI)[e]);
                if (act(e)) {
                    const double dlt = x - Vp(X)[e + K];
                    const double r2 = dlt + Vp(SDP)[e] - delta, r3 = -dlt + Vp(SDM)[e] - delta;
                    Vp(RDP)[e] = r2;
                    Vp(RDM)[e] = r3;
                    rp = fmax(rp, fmax(fabs(r2), fabs(r3)));
                    gap = gap + (Vp(SDP)[e] * Vp(ZDP)[e] + Vp(SDM)[e] * Vp(ZDM)[e]);
                }
            }
            rp = wave_max(rp);
            rdm = wave_max(rdm);
            gap = wave_sum(gap);
            pres = rp / pscale;
            dres = rdm / dscale;
            gres = gap / (1.0 + fabs(obj));
            if (!isfinite(pres) || !isfinite(dres) || !isfinite(gres)) { st = SAID_OPTIMIZE_NOT_FINITE; break; }
            if (pres <= a.tol && dres <= a.tol && gres <= a.tol) { st = SAID_OPTIMIZE_CONVERGED; break; }
            if (it >= a.max_iter) { st = SAID_OPTIMIZE_MAX_ITER; break; }
            const double mu = gap / m;
            for (long long e = lane; e < n; e += 64) {
                Vp(WB)[e] = Vp(ZLO)[e] / Vp(SLO)[e] + Vp(ZHI)[e] / Vp(SHI)[e];
                Vp(DD)[e] = act(e) ? Vp(ZDP)[e] / Vp(SDP)[e] + Vp(ZDM)[e] / Vp(SDM)[e] : 0.0;
                for (int f = 0; f < 4; ++f) Vp(RC0 + f)[e] = (f < 2 || act(e)) ? Vp(SLO + f)[e] * Vp(ZLO + f)[e] : 0.0;
            }
            __syncthreads();
            factor();
            solve();   // predictor (affine scaling)
            const double aa = max_step();
            double ga = 0.0;
            for (long long e = lane; e < n; e += 64)
                for (int f = 0; f < 4; ++f)
                    if (f < 2 || act(e)) ga = ga + (Vp(SLO + f)[e] + aa * Vp(DS0 + f)[e]) * (Vp(ZLO + f)[e] + aa * Vp(DZ0 + f)[e]);
            ga = wave_sum(ga);
            const double ratio = (ga / m) / mu, sigma = ratio * ratio * ratio;
            for (long long e = lane; e < n; e += 64)
                for (int f = 0; f < 4; ++f)
                    Vp(RC0 + f)[e] = (f < 2 || act(e)) ? Vp(SLO + f)[e] * Vp(ZLO + f)[e] + Vp(DS0 + f)[e] * Vp(DZ0 + f)[e] - sigma * mu : 0.0;
            __syncthreads();
            solve();   // corrector
            const double al = fmin(1.0, 0.99 * max_step());
            for (long long e = lane; e < n; e += 64) {
                Vp(X)[e] += al * Vp(DX)[e];
                for (int f = 0; f < 8; ++f) Vp(SLO + f)[e] += al * Vp(DS0 + f)[e];
            }
            __syncthreads();
        }
        const double sc = 1.0 / isc;
        for (long long e = lane; e < n; e += 64) {
            a.w[f0 * K + e] = Vp(X)[e];
            if (a.z) {
                const long long fr = f0 + e / K, k = e % K;
                for (int f = 0; f < 4; ++f) a.z[(fr * 4 + f) * K + k] = Vp(ZLO + f)[e] * sc;
            }
        }
        if (lane == 0) {
            if (a.status) a.status[s] = st;
            if (a.iters) a.iters[s] = it;
            if (a.resid) {
                a.resid[3 * s] = pres;
                a.resid[3 * s + 1] = dres;
                a.resid[3 * s + 2] = gres;
            }
        }
    }
};

template <int KP>
__global__ __launch_bounds__(64) void qp_ip_kernel(QPArgs a) {
    __shared__ double lds[4 * KP * KP + 3 * KP];
    Solver<KP> s(a, lds);
    s.run();
}

}  // namespace

struct said_optimize {
    HostCtx c;
    int nbasis = 0, K = 0, KP = 0;
    long long n3v = 0;
    double *neutral = nullptr, *bdelta = nullptr, *P = nullptr, *scale = nullptr;
    double* ws = nullptr;
    size_t ws_n = 0;
    long long* offs = nullptr;
    int* basis = nullptr;
    int *status = nullptr, *iters = nullptr;
    double* resid = nullptr;
    int seq_cap = 0;
    std::vector<double> scale_host;
};

extern "C" {

int said_optimize_create(said_optimize** out, int device) {
    DeviceRestore restore_device;
    said_optimize* o = new_ctx("said_optimize_create", out, device);
    if (!o) return -1;
    *out = o;
    return 0;
}

int said_optimize_destroy(said_optimize* o) { return delete_ctx(o); }

const char* said_optimize_last_error(const said_optimize* o) { return ctx_error(o); }

int said_optimize_set_bases(said_optimize* o, int nbasis, int k, long long n3v, const double* neutral_host, const double* bdelta_host,
                            const double* p_host, void* stream) {
    if (!o) return -1;
    HostCtx* ctx = &o->c;
    if (nbasis < 1 || k < 1 || k > SAID_OPTIMIZE_MAX_K || n3v < 1) return fail(ctx, "said_optimize_set_bases: nbasis %d, k %d (1..%d), n3v %lld", nbasis, k, SAID_OPTIMIZE_MAX_K, n3v);
    if (!neutral_host || !bdelta_host || !p_host) return fail(ctx, "said_optimize_set_bases: null argument");
    const int KP = k <= 32 ? 32 : 64;
    std::vector<double> pp((size_t)nbasis * KP * KP, 0.0), sc(nbasis);
    for (int b = 0; b < nbasis; ++b) {
        const double* p = p_host + (size_t)b * k * k;
        double dmax = 0.0;
        for (int i = 0; i < k; ++i) dmax = std::max(dmax, p[i * k + i]);
        if (!(dmax > 0.0) || !std::isfinite(dmax)) return fail(ctx, "said_optimize_set_bases: basis %d has no positive finite diagonal in P", b);
        int ex = 0;
        std::frexp(dmax, &ex);
        sc[b] = std::ldexp(1.0, ex - 1);   // the power of two at or below P's largest diagonal entry: P / scale is exact
        for (int i = 0; i < k; ++i)
            for (int j = 0; j < k; ++j) {
                const double v = p[i * k + j];
                if (!std::isfinite(v)) return fail(ctx, "said_optimize_set_bases: non-finite P");
                pp[((size_t)b * KP + i) * KP + j] = v / sc[b];
            }
    }
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(s));
    if (drealloc(ctx, &o->neutral, (size_t)nbasis * n3v, false) || drealloc(ctx, &o->bdelta, (size_t)nbasis * n3v * k, false) ||
        drealloc(ctx, &o->P, pp.size(), false) || drealloc(ctx, &o->scale, (size_t)nbasis, false))
        return -1;
    HIPCHK(hipMemcpyAsync(o->neutral, neutral_host, sizeof(double) * nbasis * n3v, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(o->bdelta, bdelta_host, sizeof(double) * nbasis * n3v * k, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(o->P, pp.data(), sizeof(double) * pp.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(o->scale, sc.data(), sizeof(double) * nbasis, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    o->nbasis = nbasis;
    o->K = k;
    o->KP = KP;
    o->n3v = n3v;
    o->scale_host = sc;
    return 0;
}

int said_optimize_rhs(said_optimize* o, int basis, const double* verts_dev, long long nframes, double* q_dev, void* stream) {
    if (!o) return -1;
    HostCtx* ctx = &o->c;
    if (o->nbasis == 0) return fail(ctx, "said_optimize_rhs: no basis set (said_optimize_set_bases)");
    if (basis < 0 || basis >= o->nbasis) return fail(ctx, "said_optimize_rhs: basis %d outside [0, %d)", basis, o->nbasis);
    if (!verts_dev || !q_dev || nframes < 1) return fail(ctx, "said_optimize_rhs: need device buffers of nframes >= 1");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    const long long nb = (nframes + RHS_F - 1) / RHS_F;
    rhs_kernel<<<(unsigned)nb, 256, 0, s>>>(o->bdelta + (size_t)basis * o->n3v * o->K, o->neutral + (size_t)basis * o->n3v, verts_dev, nframes, o->n3v,
                                           o->K, q_dev);
    HIPCHK(hipGetLastError());
    return 0;
}

int said_optimize_solve(said_optimize* o, int nseq, const long long* offsets_host, const int* basis_host, const double* q_dev, double delta,
                        int coupled, int max_iter, double tol, double* w_dev, double* z_dev, int* status_host, int* iters_host, double* resid_host,
                        void* stream) {
    if (!o) return -1;
    HostCtx* ctx = &o->c;
    if (o->nbasis == 0) return fail(ctx, "said_optimize_solve: no basis set (said_optimize_set_bases)");
    if (nseq < 1 || !offsets_host || !basis_host || !q_dev || !w_dev) return fail(ctx, "said_optimize_solve: null argument or nseq < 1");
    if (offsets_host[0] != 0) return fail(ctx, "said_optimize_solve: offsets must start at 0");
    for (int i = 0; i < nseq; ++i) {
        if (offsets_host[i + 1] <= offsets_host[i]) return fail(ctx, "said_optimize_solve: sequence %d has no frames", i);
        if (offsets_host[i + 1] - offsets_host[i] > (1LL << 24)) return fail(ctx, "said_optimize_solve: sequence %d is too long", i);
        if (basis_host[i] < 0 || basis_host[i] >= o->nbasis) return fail(ctx, "said_optimize_solve: sequence %d names basis %d of %d", i, basis_host[i], o->nbasis);
    }
    if (coupled && !(delta > 0.0 && std::isfinite(delta))) return fail(ctx, "said_optimize_solve: delta must be positive and finite");
    if (max_iter < 0 || !(tol > 0.0)) return fail(ctx, "said_optimize_solve: max_iter >= 0 and tol > 0 required");
    const long long F = offsets_host[nseq], FK = F * o->K;
    const size_t need = (size_t)NV * FK + (size_t)F * o->KP * o->KP;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(s));
    if (need > o->ws_n) {
        if (drealloc(ctx, &o->ws, need, false)) return -1;
        o->ws_n = need;
    }
    if (nseq > o->seq_cap) {
        if (drealloc(ctx, &o->offs, (size_t)nseq + 1, false) || drealloc(ctx, &o->basis, (size_t)nseq, false) ||
            drealloc(ctx, &o->status, (size_t)nseq, false) || drealloc(ctx, &o->iters, (size_t)nseq, false) ||
            drealloc(ctx, &o->resid, (size_t)nseq * 3, false))
            return -1;
        o->seq_cap = nseq;
    }
    HIPCHK(hipMemcpyAsync(o->offs, offsets_host, sizeof(long long) * (nseq + 1), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(o->basis, basis_host, sizeof(int) * nseq, hipMemcpyHostToDevice, s));
    QPArgs a{o->P, o->scale, o->offs, o->basis, q_dev, o->ws, w_dev, z_dev, o->status, o->iters, o->resid, FK, o->K, coupled ? 1 : 0, max_iter, delta, tol};
    if (o->KP == 32) qp_ip_kernel<32><<<nseq, 64, 0, s>>>(a);
    else qp_ip_kernel<64><<<nseq, 64, 0, s>>>(a);
    HIPCHK(hipGetLastError());
    std::vector<int> st(nseq), itv(nseq);
    std::vector<double> rs((size_t)nseq * 3);
    HIPCHK(hipMemcpyAsync(st.data(), o->status, sizeof(int) * nseq, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(itv.data(), o->iters, sizeof(int) * nseq, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(rs.data(), o->resid, sizeof(double) * nseq * 3, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (status_host) std::copy(st.begin(), st.end(), status_host);
    if (iters_host) std::copy(itv.begin(), itv.end(), iters_host);
    if (resid_host) std::copy(rs.begin(), rs.end(), resid_host);
    return 0;
}

}  // extern "C"
