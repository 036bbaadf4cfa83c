// render.hip — the renderer's kernels (C ABI: include/said_render.h; host side: renderer.cpp; specification: DESIGN.md section 15).
//
// Five launches per chunk of frames, every one with the frame in blockIdx.y, so a frame's values never depend on the chunk it is in:
//   blend_vertices_kernel   v_t = n + B_delta w_t, and the colour-mapped |B_delta (w'_t - w_t)| per vertex          one thread per vertex
//   face_normals_kernel     unit normal and corner angles of every face, from edges formed relative to the neutral      one thread per triangle
//   vertex_normals_kernel   angle-weighted smooth normals, gathered through the incidence list in ascending face order  one thread per vertex
//   tri_setup_kernel        rotation about t_center, pinhole projection, winding made positive, pixel box            one thread per triangle
//   raster_shade_kernel     one workgroup per 32 x 32 tile: box cull + ballot compaction into LDS, depth test in registers, shading in place
//   raster_shade_ms_kernel  in its place at 4 samples per pixel (section 15.2): coverage and depth per sample, one shade per face, box resolve
// fp32 throughout, no atomics; every product-sum that section 15 writes as a chain is an explicit fmaf chain (the library is built with
// -ffp-contract=off, so nothing else is fused).
#include "render_kernels.h"

namespace said {
namespace render {

namespace {

constexpr int TILE = SAID_RENDER_TILE;
constexpr float PI_F = 3.14159265358979323846f;

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 ld3(const float* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ void st3(float* p, V3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 scale(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ V3 fma3(float s, V3 a, V3 acc) { return {fmaf(s, a.x, acc.x), fmaf(s, a.y, acc.y), fmaf(s, a.z, acc.z)}; }
// x / max(|x|, 1e-20)
__device__ __forceinline__ V3 unit(V3 a) { return scale(a, 1.0f / fmaxf(sqrtf(dot(a, a)), 1e-20f)); }
__device__ __forceinline__ V3 matvec(const float* R, V3 d) {
    return {fmaf(R[2], d.z, fmaf(R[1], d.y, R[0] * d.x)), fmaf(R[5], d.z, fmaf(R[4], d.y, R[3] * d.x)), fmaf(R[8], d.z, fmaf(R[7], d.y, R[6] * d.x))};
}
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

__global__ __launch_bounds__(256) void blend_vertices_kernel(Mesh m, Frames f, const float* __restrict__ coeffs, const float* __restrict__ target,
                                                             float max_diff, const float* __restrict__ lut) {
    __shared__ float w[SAID_RENDER_MAX_K], dw[SAID_RENDER_MAX_K];
    const int fr = blockIdx.y, tid = threadIdx.x;
    if (tid < m.k) {
        const float c = coeffs[(size_t)fr * m.k + tid];
        w[tid] = c;
        dw[tid] = target ? target[(size_t)fr * m.k + tid] - c : 0.0f;
    }
    __syncthreads();
    const int v = blockIdx.x * 256 + tid;
    if (v >= m.nv) return;
    V3 s = {0.f, 0.f, 0.f}, g = {0.f, 0.f, 0.f};
    for (int k = 0; k < m.k; ++k) {
        const V3 b = ld3(m.bdelta + ((size_t)k * m.nv + v) * 3);
        s = fma3(w[k], b, s);
        g = fma3(dw[k], b, g);
    }
    const size_t o = ((size_t)fr * m.nv + v) * 3;
    st3(f.verts + o, add(ld3(m.neutral + (size_t)v * 3), s));
    V3 col = {0.f, 0.f, 0.f};
    if (target) {
        const float x = fminf(fmaxf(sqrtf(dot(g, g)), 0.0f), max_diff) / max_diff;
        int idx = x >= 1.0f ? SAID_RENDER_LUT - 1 : (x > 0.0f ? (int)(x * (float)SAID_RENDER_LUT) : 0);   // matplotlib: int(x N), x == 1 -> N - 1
        idx = min(max(idx, 0), SAID_RENDER_LUT - 1);
        col = ld3(lut + idx * 3);
    }
    st3(f.colors + o, col);
}

// Unit normal and corner angles of every face.  Where the mesh folds onto a sliver (2e-7 m^2 on 1.4 mm edges in the test sequence, the
// vertex's summed normal 0.08 of its summed angles) an edge error of 1e-10 m turns the vertex normal by 1e-5: neither the fp32 vertices
// (rounded at 4e-9) nor a plain fp32 sum of the basis edges (3e-10 over 32 roundings at 1e-3) is enough.  So each edge is carried as an
// unevaluated fp32 pair hi + lo: set_mesh forms the edges of the neutral and of every B_delta[k] in float64 and splits them, the sum over k
// is compensated (every product's and every addition's rounding error is recovered by fmaf / TwoSum and accumulated), and the cross
// product takes its leading term as a difference of products with the products' errors recovered, plus the hi x lo terms.
struct P3 { V3 h, l; };
__device__ __forceinline__ void two_sum(float a, float b, float& s, float& e) {   // s + e = a + b exactly
    s = a + b;
    const float bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
__device__ __forceinline__ void acc1(float w, float bh, float bl, float& s, float& c) {   // (s, c) += w (bh + bl)
    const float p = w * bh, pe = fmaf(w, bh, -p);
    float e;
    two_sum(s, p, s, e);
    c += (e + pe) + w * bl;
}
__device__ __forceinline__ void fold1(float nh, float nl, float s, float c, float& h, float& l) {   // hi + lo = (nh + nl) + (s + c)
    float e;
    two_sum(nh, s, h, e);
    const float t = (e + nl) + c, hh = h + t;
    l = t - (hh - h);
    h = hh;
}
// a b - c d with both products' rounding errors recovered (Kahan)
__device__ __forceinline__ float diff_of_products(float a, float b, float c, float d) {
    const float w = c * d, e = fmaf(-c, d, w), g = fmaf(a, b, -w);
    return g + e;
}
__device__ __forceinline__ V3 cross_pairs(const P3& a, const P3& b) {
    const V3 lead = {diff_of_products(a.h.y, b.h.z, a.h.z, b.h.y), diff_of_products(a.h.z, b.h.x, a.h.x, b.h.z), diff_of_products(a.h.x, b.h.y, a.h.y, b.h.x)};
    return add(lead, add(cross(a.h, b.l), cross(a.l, b.h)));
}

__global__ __launch_bounds__(256) void face_normals_kernel(Mesh m, Frames f, const float* __restrict__ coeffs) {
    __shared__ float w[SAID_RENDER_MAX_K];
    const int fr = blockIdx.y, tid = threadIdx.x;
    if (tid < m.k) w[tid] = coeffs[(size_t)fr * m.k + tid];
    __syncthreads();
    const int t = blockIdx.x * 256 + tid;
    if (t >= m.nf) return;
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, c[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < m.k; ++k) {
        const float* eb = m.ebasis + ((size_t)k * m.nf + t) * 12;   // 6 hi, 6 lo
#pragma unroll
        for (int i = 0; i < 6; ++i) acc1(w[k], eb[i], eb[6 + i], s[i], c[i]);
    }
    const float* ne = m.nedge + (size_t)t * 12;
    float h[6], l[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) fold1(ne[i], ne[6 + i], s[i], c[i], h[i], l[i]);
    const P3 e1 = {{h[0], h[1], h[2]}, {l[0], l[1], l[2]}}, e2 = {{h[3], h[4], h[5]}, {l[3], l[4], l[5]}};
    const V3 nf = cross_pairs(e1, e2);
    const float l2 = dot(nf, nf);
    V3 n = {0.f, 0.f, 0.f}, ang = {0.f, 0.f, 0.f};
    if (l2 > 0.0f) {   // a face without area has no normal and no weight
        const float len = sqrtf(l2);   // |a x b| is twice the area at every corner
        n = scale(nf, 1.0f / len);
        const V3 e3 = sub(e2.h, e1.h), z = {0.f, 0.f, 0.f}, m1 = sub(z, e1.h), m2 = sub(z, e2.h), m3 = sub(z, e3);
        // corner 0: e1, e2; corner 1: p2 - p1, p0 - p1; corner 2: p0 - p2, p1 - p2
        ang = {atan2f(len, dot(e1.h, e2.h)), atan2f(len, dot(e3, m1)), atan2f(len, dot(m2, m3))};
    }
    float* o = f.face_na + ((size_t)fr * m.nf + t) * 6;
    st3(o, n);
    st3(o + 3, ang);
}

__global__ __launch_bounds__(256) void vertex_normals_kernel(Mesh m, Frames f) {
    const int fr = blockIdx.y;
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= m.nv) return;
    const float* na = f.face_na + (size_t)fr * m.nf * 6;
    V3 acc = {0.f, 0.f, 0.f};
    for (int e = m.inc_off[v]; e < m.inc_off[v + 1]; ++e) {   // ascending face index: a gather in a fixed order
        const int code = m.inc[e];
        const float* o = na + (size_t)(code >> 2) * 6;
        acc = fma3(o[3 + (code & 3)], ld3(o), acc);
    }
    const float l = sqrtf(dot(acc, acc));
    const V3 n = l > 0.0f ? scale(acc, 1.0f / l) : V3{0.f, 0.f, 0.f};
    st3(f.normals + ((size_t)fr * m.nv + v) * 3, n);
}

struct Cam {
    float fx, fy, cxc, cyc, znear, zfar, hw, hh;   // cxc = cx - width / 2, cyc = cy - height / 2; hw, hh: half the size
    float cam[3];
    int W, H;
};

__global__ __launch_bounds__(256) void tri_setup_kernel(Mesh m, Frames f, Cam cam, Xform xf, int vertex_colors) {
    const int fr = blockIdx.y;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= m.nf) return;
    V3 P[3], N[3], C[3];
    float sx[3], sy[3], invd[3];
    bool ok = true;
    const V3 c = {xf.c[0], xf.c[1], xf.c[2]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const size_t o = ((size_t)fr * m.nv + m.faces[t * 3 + j]) * 3;
        P[j] = add(matvec(xf.R, sub(ld3(f.verts + o), c)), c);
        N[j] = matvec(xf.R, ld3(f.normals + o));
        C[j] = vertex_colors ? ld3(f.colors + o) : V3{0.f, 0.f, 0.f};
        const float qx = P[j].x - cam.cam[0], qy = P[j].y - cam.cam[1], d = cam.cam[2] - P[j].z;
        ok = ok && d >= cam.znear;   // a triangle that reaches in front of the near plane is dropped whole (section 15)
        sx[j] = (cam.fx * qx) / d + cam.cxc;
        sy[j] = cam.cyc - (cam.fy * qy) / d;
        invd[j] = 1.0f / d;
        ok = ok && isfinite(sx[j]) && isfinite(sy[j]) && isfinite(invd[j]);
    }
    const float area2 = (sx[1] - sx[0]) * (sy[2] - sy[0]) - (sy[1] - sy[0]) * (sx[2] - sx[0]);
    ok = ok && area2 != 0.0f && isfinite(area2);
    const bool sw = area2 < 0.0f;   // vertices 1 and 2 change places when the winding is negative: interior is E > 0 from here on
    const size_t rec = ((size_t)fr * m.nf + t);
    float* r = f.tri_rec + rec * TRI_REC;
    r[0] = sx[0]; r[1] = sy[0]; r[2] = sw ? sx[2] : sx[1]; r[3] = sw ? sy[2] : sy[1]; r[4] = sw ? sx[1] : sx[2]; r[5] = sw ? sy[1] : sy[2];
    r[6] = invd[0]; r[7] = sw ? invd[2] : invd[1]; r[8] = sw ? invd[1] : invd[2]; r[9] = __int_as_float(t); r[10] = 0.f; r[11] = 0.f;
    float* at = f.tri_attr + rec * TRI_ATTR;
    float* a1 = at + (sw ? 6 : 3);
    float* a2 = at + (sw ? 3 : 6);
    st3(at + 0, P[0]); st3(a1, P[1]); st3(a2, P[2]);
    st3(at + 9, N[0]); st3(a1 + 9, N[1]); st3(a2 + 9, N[2]);
    st3(at + 18, C[0]); st3(a1 + 18, C[1]); st3(a2 + 18, C[2]);
    int bx = 1, by = 1;   // empty: min 1 > max 0
    if (ok) {
        // every pixel whose centre can lie inside, one pixel of slack each way; clamped as floats before the conversion
        const float lim_x = (float)cam.W + 1.0f, lim_y = (float)cam.H + 1.0f;
        const float x0 = fminf(fmaxf(fminf(sx[0], fminf(sx[1], sx[2])) + cam.hw, -2.0f), lim_x), x1 = fminf(fmaxf(fmaxf(sx[0], fmaxf(sx[1], sx[2])) + cam.hw, -2.0f), lim_x);
        const float y0 = fminf(fmaxf(fminf(sy[0], fminf(sy[1], sy[2])) + cam.hh, -2.0f), lim_y), y1 = fminf(fmaxf(fmaxf(sy[0], fmaxf(sy[1], sy[2])) + cam.hh, -2.0f), lim_y);
        const int xmin = max((int)floorf(x0) - 1, 0), xmax = min((int)floorf(x1) + 1, cam.W - 1);
        const int ymin = max((int)floorf(y0) - 1, 0), ymax = min((int)floorf(y1) + 1, cam.H - 1);
        if (xmin <= xmax && ymin <= ymax) { bx = xmin | (xmax << 16); by = ymin | (ymax << 16); }
    }
    f.tri_box[rec * 2 + 0] = bx;
    f.tri_box[rec * 2 + 1] = by;
}

struct Shading {
    int n_lights;
    float light[SAID_RENDER_MAX_LIGHTS][3], intensity[SAID_RENDER_MAX_LIGHTS];
    float ambient, base[3], metallic, roughness;
};

// The three edge functions of a record at a pixel centre (centred coordinates), E_i > 0 inside; tl_i: edge i is a top or a left edge.
struct Edges {
    float x0, y0, x1, y1, x2, y2, A0, B0, A1, B1, A2, B2;
    bool tl0, tl1, tl2;
    __device__ __forceinline__ Edges(float4 a, float4 b) : x0(a.x), y0(a.y), x1(a.z), y1(a.w), x2(b.x), y2(b.y) {
        A0 = y1 - y2; B0 = x2 - x1; A1 = y2 - y0; B1 = x0 - x2; A2 = y0 - y1; B2 = x1 - x0;
        tl0 = A0 > 0.f || (A0 == 0.f && B0 > 0.f); tl1 = A1 > 0.f || (A1 == 0.f && B1 > 0.f); tl2 = A2 > 0.f || (A2 == 0.f && B2 > 0.f);
    }
    __device__ __forceinline__ bool eval(float px, float py, float& E0, float& E1, float& E2) const {
        E0 = fmaf(A0, px - x1, B0 * (py - y1));
        E1 = fmaf(A1, px - x2, B1 * (py - y2));
        E2 = fmaf(A2, px - x0, B2 * (py - y0));
        return (E0 > 0.f || (E0 == 0.f && tl0)) && (E1 > 0.f || (E1 == 0.f && tl1)) && (E2 > 0.f || (E2 == 0.f && tl2));
    }
};

__device__ V3 shade_fragment(const float* __restrict__ rec, const float* __restrict__ at, float px, float py, const Cam& cam, const Shading& sh, int vertex_colors) {
    const float4 ra = *reinterpret_cast<const float4*>(rec), rb = *reinterpret_cast<const float4*>(rec + 4);
    const float i2 = rec[8];
    const Edges ed(ra, rb);
    float E0, E1, E2;
    ed.eval(px, py, E0, E1, E2);
    const float w0 = E0 * rb.z, w1 = E1 * rb.w, w2 = E2 * i2, ws = (w0 + w1) + w2;
    const float b0 = w0 / ws, b1 = w1 / ws, b2 = w2 / ws;
    const V3 P = fma3(b2, ld3(at + 6), fma3(b1, ld3(at + 3), scale(ld3(at + 0), b0)));
    const V3 N = unit(fma3(b2, ld3(at + 15), fma3(b1, ld3(at + 12), scale(ld3(at + 9), b0))));
    V3 base = {sh.base[0], sh.base[1], sh.base[2]};
    if (vertex_colors) base = fma3(b2, ld3(at + 24), fma3(b1, ld3(at + 21), scale(ld3(at + 18), b0)));
    const float met = sh.metallic, alpha = sh.roughness * sh.roughness, a2 = alpha * alpha, k = alpha * 0.5f;
    const float dielectric = 0.04f * (1.0f - met), kd = (1.0f - 0.04f) * (1.0f - met);
    const V3 F0 = {fmaf(base.x, met, dielectric), fmaf(base.y, met, dielectric), fmaf(base.z, met, dielectric)};
    const V3 cdiff = scale(base, kd);
    const V3 V = unit(sub(V3{cam.cam[0], cam.cam[1], cam.cam[2]}, P));
    const float NdV = clamp01(dot(N, V));
    V3 col = scale(base, sh.ambient);
    for (int l = 0; l < sh.n_lights; ++l) {
        const V3 Lv = sub(V3{sh.light[l][0], sh.light[l][1], sh.light[l][2]}, P);
        const float d2 = dot(Lv, Lv);
        const V3 L = unit(Lv), H = unit(add(L, V));
        const float NdL = clamp01(dot(N, L)), NdH = clamp01(dot(N, H)), VdH = clamp01(dot(V, H));
        const float den = fmaf(NdH * NdH, a2 - 1.0f, 1.0f);
        const float D = a2 / (PI_F * den * den);
        const float vis = 1.0f / (4.0f * fmaf(NdL, 1.0f - k, k) * fmaf(NdV, 1.0f - k, k));
        const float x = 1.0f - VdH, x2 = x * x, x5 = x2 * x2 * x;
        const float e = (sh.intensity[l] / fmaxf(d2, 1e-20f)) * NdL, dv = D * vis;
        const V3 F = {fmaf(1.0f - F0.x, x5, F0.x), fmaf(1.0f - F0.y, x5, F0.y), fmaf(1.0f - F0.z, x5, F0.z)};
        col.x = fmaf(e, fmaf(F.x, dv, (1.0f - F.x) * cdiff.x / PI_F), col.x);
        col.y = fmaf(e, fmaf(F.y, dv, (1.0f - F.y) * cdiff.y / PI_F), col.y);
        col.z = fmaf(e, fmaf(F.z, dv, (1.0f - F.z) * cdiff.z / PI_F), col.z);
    }
    return col;
}

__device__ __forceinline__ unsigned to_u8(float c) { return (unsigned)floorf(fmaf(clamp01(c), 255.0f, 0.5f)); }

__global__ __launch_bounds__(256) void raster_shade_kernel(Mesh m, Frames f, Cam cam, Shading sh, int vertex_colors, int tiles_x,
                                                           unsigned char* __restrict__ out, int* __restrict__ face_ids) {
    __shared__ float4 lrec[256 * 3];
    __shared__ int wave_cnt[4];
    const int fr = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tx0 = (blockIdx.x % tiles_x) * TILE, ty0 = (blockIdx.x / tiles_x) * TILE;
    const int row = ty0 + (tid >> 3), col0 = tx0 + (tid & 7) * 4;   // four pixels of one row
    const float py = ((float)row + 0.5f) - cam.hh;
    float px[4], best_d[4];
    int best[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        px[j] = ((float)(col0 + j) + 0.5f) - cam.hw;
        best_d[j] = INFINITY;
        best[j] = -1;
    }
    const float* rec_fr = f.tri_rec + (size_t)fr * m.nf * TRI_REC;
    const int* box_fr = f.tri_box + (size_t)fr * m.nf * 2;
    for (int base = 0; base < m.nf; base += 256) {
        const int t = base + tid;
        bool hit = false;
        if (t < m.nf) {
            const int bx = box_fr[t * 2], by = box_fr[t * 2 + 1];
            const int xmin = bx & 0xffff, xmax = bx >> 16, ymin = by & 0xffff, ymax = by >> 16;
            hit = xmin <= xmax && xmin <= tx0 + TILE - 1 && xmax >= tx0 && ymin <= ty0 + TILE - 1 && ymax >= ty0;
        }
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) wave_cnt[wv] = __popcll(mask);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = wave_cnt[i];
            off += i < wv ? c : 0;
            total += c;
        }
        if (hit) {   // ascending triangle index: waves in order, lanes in order within a wave
            const int pos = off + __popcll(mask & ((1ull << lane) - 1ull));
            const float4* src = reinterpret_cast<const float4*>(rec_fr + (size_t)t * TRI_REC);
            lrec[pos * 3 + 0] = src[0];
            lrec[pos * 3 + 1] = src[1];
            lrec[pos * 3 + 2] = src[2];
        }
        __syncthreads();
        for (int j = 0; j < total; ++j) {
            const float4 ra = lrec[j * 3], rb = lrec[j * 3 + 1], rc = lrec[j * 3 + 2];
            const Edges ed(ra, rb);
            const int id = __float_as_int(rc.y);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                float E0, E1, E2;
                if (ed.eval(px[p], py, E0, E1, E2)) {
                    const float d = ((E0 + E1) + E2) / fmaf(E2, rc.x, fmaf(E1, rb.w, E0 * rb.z));
                    if (d >= cam.znear && d <= cam.zfar && d < best_d[p]) {   // strict: a tie stays with the lower face index
                        best_d[p] = d;
                        best[p] = id;
                    }
                }
            }
        }
        __syncthreads();   // the list and the counts are rewritten by the next chunk
    }
    if (row >= cam.H) return;
    unsigned bytes[12];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        V3 c = {0.f, 0.f, 0.f};
        if (best[p] >= 0) {
            const size_t r = (size_t)fr * m.nf + best[p];
            c = shade_fragment(f.tri_rec + r * TRI_REC, f.tri_attr + r * TRI_ATTR, px[p], py, cam, sh, vertex_colors);
        }
        const bool bg = best[p] < 0;
        bytes[p * 3 + 0] = bg ? 0u : to_u8(c.z);   // B, G, R
        bytes[p * 3 + 1] = bg ? 0u : to_u8(c.y);
        bytes[p * 3 + 2] = bg ? 0u : to_u8(c.x);
    }
    const size_t pix = ((size_t)fr * cam.H + row) * cam.W + col0;
    if ((cam.W & 3) == 0 && col0 + 3 < cam.W) {   // 12 bytes at a multiple of 12 from a row start that is a multiple of 4
        unsigned* o = reinterpret_cast<unsigned*>(out + pix * 3);
#pragma unroll
        for (int q = 0; q < 3; ++q) o[q] = bytes[q * 4] | (bytes[q * 4 + 1] << 8) | (bytes[q * 4 + 2] << 16) | (bytes[q * 4 + 3] << 24);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (col0 + p < cam.W)
                for (int q = 0; q < 3; ++q) out[(pix + p) * 3 + q] = (unsigned char)bytes[p * 3 + q];
    }
    if (face_ids) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (col0 + p < cam.W) face_ids[pix + p] = best[p];
    }
}

// The 4-sample variant: coverage and depth per sample at the rotated-grid offsets below, the winners of a thread's
// 4 pixels x 4 samples in registers (every index a compile-time constant: all loops over them are unrolled), then one shade per distinct
// face of a pixel at the pixel centre, to_u8 per sample and the box resolve (c0 + c1 + c2 + c3 + 2) >> 2.  The tile scan is that of
// raster_shade_kernel; the compacting thread also leaves the triangle's pixel box in the two spare words of its LDS record, so a thread
// whose four pixels lie outside the box skips the sixteen sample tests (the box holds every sample of every pixel the triangle can touch).
__device__ __forceinline__ constexpr float ms_ox(int s) { return s == 0 ? -0.125f : s == 1 ? 0.375f : s == 2 ? -0.375f : 0.125f; }
__device__ __forceinline__ constexpr float ms_oy(int s) { return s == 0 ? -0.375f : s == 1 ? -0.125f : s == 2 ? 0.125f : 0.375f; }

__global__ __launch_bounds__(256) void raster_shade_ms_kernel(Mesh m, Frames f, Cam cam, Shading sh, int vertex_colors, int tiles_x,
                                                              unsigned char* __restrict__ out, int* __restrict__ sample_ids) {
    __shared__ float4 lrec[256 * 3];
    __shared__ int wave_cnt[4];
    const int fr = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tx0 = (blockIdx.x % tiles_x) * TILE, ty0 = (blockIdx.x / tiles_x) * TILE;
    const int row = ty0 + (tid >> 3), col0 = tx0 + (tid & 7) * 4;   // four pixels of one row
    const float py = ((float)row + 0.5f) - cam.hh;
    float px[4], best_d[4][4];
    int best[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        px[p] = ((float)(col0 + p) + 0.5f) - cam.hw;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            best_d[p][s] = INFINITY;
            best[p][s] = -1;
        }
    }
    const float* rec_fr = f.tri_rec + (size_t)fr * m.nf * TRI_REC;
    const int* box_fr = f.tri_box + (size_t)fr * m.nf * 2;
    for (int base = 0; base < m.nf; base += 256) {
        const int t = base + tid;
        bool hit = false;
        int bx = 1, by = 1;
        if (t < m.nf) {
            bx = box_fr[t * 2];
            by = box_fr[t * 2 + 1];
            const int xmin = bx & 0xffff, xmax = bx >> 16, ymin = by & 0xffff, ymax = by >> 16;
            hit = xmin <= xmax && xmin <= tx0 + TILE - 1 && xmax >= tx0 && ymin <= ty0 + TILE - 1 && ymax >= ty0;
        }
        const unsigned long long mask = __ballot(hit);
        if (lane == 0) wave_cnt[wv] = __popcll(mask);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = wave_cnt[i];
            off += i < wv ? c : 0;
            total += c;
        }
        if (hit) {   // ascending triangle index: waves in order, lanes in order within a wave
            const int pos = off + __popcll(mask & ((1ull << lane) - 1ull));
            const float4* src = reinterpret_cast<const float4*>(rec_fr + (size_t)t * TRI_REC);
            float4 c = src[2];
            c.z = __int_as_float(bx);
            c.w = __int_as_float(by);
            lrec[pos * 3 + 0] = src[0];
            lrec[pos * 3 + 1] = src[1];
            lrec[pos * 3 + 2] = c;
        }
        __syncthreads();
        for (int j = 0; j < total; ++j) {
            const float4 rc = lrec[j * 3 + 2];
            const int bxj = __float_as_int(rc.z), byj = __float_as_int(rc.w);
            if (row < (byj & 0xffff) || row > (byj >> 16) || col0 + 3 < (bxj & 0xffff) || col0 > (bxj >> 16)) continue;
            const float4 ra = lrec[j * 3], rb = lrec[j * 3 + 1];
            const Edges ed(ra, rb);
            const int id = __float_as_int(rc.y);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    float E0, E1, E2;
                    if (ed.eval(px[p] + ms_ox(s), py + ms_oy(s), E0, E1, E2)) {
                        const float d = ((E0 + E1) + E2) / fmaf(E2, rc.x, fmaf(E1, rb.w, E0 * rb.z));
                        if (d >= cam.znear && d <= cam.zfar && d < best_d[p][s]) {   // strict: a tie stays with the lower face index
                            best_d[p][s] = d;
                            best[p][s] = id;
                        }
                    }
                }
            }
        }
        __syncthreads();   // the list and the counts are rewritten by the next chunk
    }
    if (row >= cam.H) return;
    // One shade per distinct face of a pixel.  The loop is not unrolled, so shade_fragment has one call site; `it` picks its sample through
    // selects and hands the colour to every sample of the same pixel that shows the same face.
    unsigned packed[4][4];   // B | G << 8 | R << 16 of each sample, 0 where nothing covers it
    unsigned done = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int s = 0; s < 4; ++s) packed[p][s] = 0u;
#pragma unroll 1
    for (int it = 0; it < 16; ++it) {
        int id = -1;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int s = 0; s < 4; ++s) id = it == p * 4 + s ? best[p][s] : id;
        const int pi = it >> 2;
        if (id < 0 || ((done >> it) & 1u) || col0 + pi >= cam.W) continue;   // a pixel beyond the image's last column is never stored
        const float pxc = ((float)(col0 + pi) + 0.5f) - cam.hw;
        const size_t r = (size_t)fr * m.nf + id;
        const V3 c = shade_fragment(f.tri_rec + r * TRI_REC, f.tri_attr + r * TRI_ATTR, pxc, py, cam, sh, vertex_colors);
        const unsigned v = to_u8(c.z) | (to_u8(c.y) << 8) | (to_u8(c.x) << 16);
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int s = 0; s < 4; ++s)
                if (p == pi && best[p][s] == id) {
                    packed[p][s] = v;
                    done |= 1u << (p * 4 + s);
                }
    }
    unsigned bytes[12];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            unsigned sum = 2u;
#pragma unroll
            for (int s = 0; s < 4; ++s) sum += (packed[p][s] >> (8 * q)) & 0xffu;
            bytes[p * 3 + q] = sum >> 2;
        }
    const size_t pix = ((size_t)fr * cam.H + row) * cam.W + col0;
    if ((cam.W & 3) == 0 && col0 + 3 < cam.W) {   // 12 bytes at a multiple of 12 from a row start that is a multiple of 4
        unsigned* o = reinterpret_cast<unsigned*>(out + pix * 3);
#pragma unroll
        for (int q = 0; q < 3; ++q) o[q] = bytes[q * 4] | (bytes[q * 4 + 1] << 8) | (bytes[q * 4 + 2] << 16) | (bytes[q * 4 + 3] << 24);
    } else {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (col0 + p < cam.W)
                for (int q = 0; q < 3; ++q) out[(pix + p) * 3 + q] = (unsigned char)bytes[p * 3 + q];
    }
    if (sample_ids) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (col0 + p < cam.W) reinterpret_cast<int4*>(sample_ids)[pix + p] = make_int4(best[p][0], best[p][1], best[p][2], best[p][3]);
    }
}

Cam make_cam(const said_render_scene& sc) {
    Cam c;
    c.fx = sc.fx; c.fy = sc.fy;
    c.hw = 0.5f * (float)sc.width; c.hh = 0.5f * (float)sc.height;
    c.cxc = sc.cx - c.hw; c.cyc = sc.cy - c.hh;
    c.znear = sc.znear; c.zfar = sc.zfar;
    for (int i = 0; i < 3; ++i) c.cam[i] = sc.cam_pos[i];
    c.W = sc.width; c.H = sc.height;
    return c;
}

Shading make_shading(const said_render_scene& sc, bool vertex_colors) {
    Shading sh;
    sh.n_lights = sc.n_lights;
    for (int l = 0; l < SAID_RENDER_MAX_LIGHTS; ++l) {
        for (int i = 0; i < 3; ++i) sh.light[l][i] = sc.light_pos[l][i];
        sh.intensity[l] = sc.light_intensity[l];
    }
    sh.ambient = sc.ambient;
    for (int i = 0; i < 3; ++i) sh.base[i] = sc.base_color[i];
    sh.metallic = vertex_colors ? sc.vc_metallic : sc.metallic;
    sh.roughness = vertex_colors ? sc.vc_roughness : sc.roughness;
    return sh;
}

}  // namespace

void launch_blend_vertices(const Mesh& m, const Frames& f, const float* coeffs, const float* target, float max_diff, const float* lut, hipStream_t s) {
    blend_vertices_kernel<<<dim3((m.nv + 255) / 256, f.n), 256, 0, s>>>(m, f, coeffs, target, max_diff, lut);
}

void launch_face_normals(const Mesh& m, const Frames& f, const float* coeffs, hipStream_t s) {
    face_normals_kernel<<<dim3((m.nf + 255) / 256, f.n), 256, 0, s>>>(m, f, coeffs);
}

void launch_vertex_normals(const Mesh& m, const Frames& f, hipStream_t s) {
    vertex_normals_kernel<<<dim3((m.nv + 255) / 256, f.n), 256, 0, s>>>(m, f);
}

void launch_tri_setup(const Mesh& m, const Frames& f, const said_render_scene& sc, const Xform& x, bool vertex_colors, hipStream_t s) {
    tri_setup_kernel<<<dim3((m.nf + 255) / 256, f.n), 256, 0, s>>>(m, f, make_cam(sc), x, vertex_colors ? 1 : 0);
}

void launch_raster_shade(const Mesh& m, const Frames& f, const said_render_scene& sc, bool vertex_colors, unsigned char* out, int* face_ids,
                         hipStream_t s) {
    const int tiles_x = (sc.width + TILE - 1) / TILE, tiles_y = (sc.height + TILE - 1) / TILE;
    raster_shade_kernel<<<dim3(tiles_x * tiles_y, f.n), 256, 0, s>>>(m, f, make_cam(sc), make_shading(sc, vertex_colors), vertex_colors ? 1 : 0, tiles_x, out, face_ids);
}

void launch_raster_shade_ms(const Mesh& m, const Frames& f, const said_render_scene& sc, bool vertex_colors, unsigned char* out, int* sample_ids,
                            hipStream_t s) {
    const int tiles_x = (sc.width + TILE - 1) / TILE, tiles_y = (sc.height + TILE - 1) / TILE;
    raster_shade_ms_kernel<<<dim3(tiles_x * tiles_y, f.n), 256, 0, s>>>(m, f, make_cam(sc), make_shading(sc, vertex_colors), vertex_colors ? 1 : 0, tiles_x, out, sample_ids);
}

}  // namespace render
}  // namespace said
