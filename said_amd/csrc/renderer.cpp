// renderer.cpp — host side of the renderer (C ABI: include/said_render.h; kernels: render.hip): the context, the mesh
// upload with its incidence list, the scene, and the five launches of a chunk, the last of them at one sample per pixel or, through
// include/said_render_ms.h, at four (section 15.2).  (Not render.cpp: a .cpp and a .hip of one stem would share the names of their
// -save-temps files, which the build's ISA scan reads — section 14.)
#include "engine_internal.h"
#include "render_kernels.h"
#include "../../include/said_render_ms.h"

using namespace said::render;

struct said_render {
    HostCtx c;
    int nv = 0, nf = 0, k = 0;
    float *neutral = nullptr, *bdelta = nullptr, *nedge = nullptr, *ebasis = nullptr, *lut = nullptr;
    int *faces = nullptr, *inc_off = nullptr, *inc = nullptr;
    bool has_scene = false, has_lut = false;
    said_render_scene scene{};
    // workspace of a chunk, grown on demand
    int cap = 0, last_n = 0;
    float *verts = nullptr, *face_na = nullptr, *normals = nullptr, *colors = nullptr, *tri_rec = nullptr, *tri_attr = nullptr;
    int* tri_box = nullptr;
};

namespace {

constexpr int MAX_CHUNK = 4096;   // frames per call (blockIdx.y)

Mesh mesh_of(const said_render* r) { return Mesh{r->nv, r->nf, r->k, r->neutral, r->bdelta, r->faces, r->nedge, r->ebasis, r->inc_off, r->inc}; }
Frames frames_of(const said_render* r, int n) { return Frames{n, r->verts, r->face_na, r->normals, r->colors, r->tri_rec, r->tri_box, r->tri_attr}; }

// Rodrigues' formula in float64, rounded to fp32 once: R = I + sin(t) K + (1 - cos(t)) K^2, K the cross-product matrix of the unit axis.
void rodrigues(const double* rot, float* R) {
    const double t = rot ? std::sqrt(rot[0] * rot[0] + rot[1] * rot[1] + rot[2] * rot[2]) : 0.0;
    double M[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (t > 0.0) {
        const double x = rot[0] / t, y = rot[1] / t, z = rot[2] / t, s = std::sin(t), c1 = 1.0 - std::cos(t);
        const double K[9] = {0, -z, y, z, 0, -x, -y, x, 0};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double k2 = 0.0;
                for (int l = 0; l < 3; ++l) k2 += K[i * 3 + l] * K[l * 3 + j];
                M[i * 3 + j] += s * K[i * 3 + j] + c1 * k2;
            }
    }
    for (int i = 0; i < 9; ++i) R[i] = (float)M[i];
}

int read_stage(said_render* r, const char* entry, const float* src, int n_frames, float* out_host, void* stream) {
    if (!r) return -1;
    HostCtx* ctx = &r->c;
    if (!out_host || n_frames < 1 || n_frames > r->last_n) return fail(ctx, "%s: n_frames %d outside 1 .. %d (the last render's chunk)", entry, n_frames, r->last_n);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(out_host, src, sizeof(float) * 3 * r->nv * n_frames, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

// Both render entries: `samples` is 1 (said_render_render's path, whatever entry asked for it) or 4 (section 15.2).
int render_chunk(said_render* r, const char* entry, int samples, const float* coeffs_dev, const float* target_dev, long long t0, int n_frames, float max_diff,
                 const double* rot_host, const double* t_center_host, unsigned char* out_u8_dev, int* face_ids_dev, int* sample_ids_dev, void* stream) {
    HostCtx* ctx = &r->c;
    if (r->nf == 0) return fail(ctx, "%s: no mesh set (said_render_set_mesh)", entry);
    if (!r->has_scene) return fail(ctx, "%s: no scene set (said_render_set_scene)", entry);
    if (!coeffs_dev || !out_u8_dev) return fail(ctx, "%s: null coefficients or output", entry);
    if (t0 < 0 || n_frames < 1 || n_frames > MAX_CHUNK) return fail(ctx, "%s: t0 %lld, n_frames %d (t0 >= 0, 1 .. %d frames per call)", entry, t0, n_frames, MAX_CHUNK);
    if (target_dev && !r->has_lut) return fail(ctx, "%s: a target sequence needs a colour map (said_render_set_colormap)", entry);
    if (target_dev && !(max_diff > 0.f && std::isfinite(max_diff))) return fail(ctx, "%s: max_diff must be positive and finite", entry);
    Xform xf;
    rodrigues(rot_host, xf.R);
    for (int i = 0; i < 3; ++i) {
        const double c = t_center_host ? t_center_host[i] : 0.0;
        if (!std::isfinite(c) || !std::isfinite((double)xf.R[i * 3])) return fail(ctx, "%s: non-finite rotation or centre", entry);
        xf.c[i] = (float)c;
    }
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    if (n_frames > r->cap) {
        HIPCHK(hipStreamSynchronize(s));
        r->cap = r->last_n = 0;
        const size_t n = (size_t)n_frames, nv3 = n * r->nv * 3, nf = n * r->nf;
        if (drealloc(ctx, &r->verts, nv3, false) || drealloc(ctx, &r->face_na, nf * 6, false) || drealloc(ctx, &r->normals, nv3, false) || drealloc(ctx, &r->colors, nv3, false) ||
            drealloc(ctx, &r->tri_rec, nf * TRI_REC, false) || drealloc(ctx, &r->tri_box, nf * 2, false) || drealloc(ctx, &r->tri_attr, nf * TRI_ATTR, false))
            return -1;
        r->cap = n_frames;
    }
    const Mesh m = mesh_of(r);
    const Frames f = frames_of(r, n_frames);
    const bool vc = target_dev != nullptr;
    launch_blend_vertices(m, f, coeffs_dev + t0 * r->k, vc ? target_dev + t0 * r->k : nullptr, max_diff, r->lut, s);
    HIPCHK(hipGetLastError());
    launch_face_normals(m, f, coeffs_dev + t0 * r->k, s);
    HIPCHK(hipGetLastError());
    launch_vertex_normals(m, f, s);
    HIPCHK(hipGetLastError());
    launch_tri_setup(m, f, r->scene, xf, vc, s);
    HIPCHK(hipGetLastError());
    if (samples == 4)
        launch_raster_shade_ms(m, f, r->scene, vc, out_u8_dev, sample_ids_dev, s);
    else
        launch_raster_shade(m, f, r->scene, vc, out_u8_dev, face_ids_dev, s);
    HIPCHK(hipGetLastError());
    r->last_n = n_frames;
    return 0;
}

}  // namespace

extern "C" {

int said_render_create(said_render** out, int device) {
    DeviceRestore restore_device;
    said_render* r = new_ctx("said_render_create", out, device);
    if (!r) return -1;
    *out = r;
    return 0;
}

int said_render_destroy(said_render* r) { return delete_ctx(r); }

const char* said_render_last_error(const said_render* r) { return ctx_error(r); }

int said_render_set_mesh(said_render* r, int nv, int nf, int k, const double* neutral_host, const int* faces_host, const double* blendshapes_host,
                         void* stream) {
    if (!r) return -1;
    HostCtx* ctx = &r->c;
    if (nv < 1 || nv > (1 << 24)) return fail(ctx, "said_render_set_mesh: %d vertices (1 .. 2^24)", nv);
    if (nf < 1 || nf > (1 << 24)) return fail(ctx, "said_render_set_mesh: %d faces (1 .. 2^24): a mesh without faces cannot be drawn", nf);
    if (k < 1 || k > SAID_RENDER_MAX_K) return fail(ctx, "said_render_set_mesh: %d blendshapes (1 .. %d)", k, SAID_RENDER_MAX_K);
    if (!neutral_host || !faces_host || !blendshapes_host) return fail(ctx, "said_render_set_mesh: null argument");
    for (long long i = 0; i < 3LL * nf; ++i)
        if (faces_host[i] < 0 || faces_host[i] >= nv)
            return fail(ctx, "said_render_set_mesh: face %lld names vertex %d, outside [0, %d)", i / 3, faces_host[i], nv);
    const size_t n3 = (size_t)nv * 3;
    std::vector<float> nh(n3), bd((size_t)k * n3);
    for (size_t i = 0; i < n3; ++i) {
        if (!std::isfinite(neutral_host[i])) return fail(ctx, "said_render_set_mesh: non-finite neutral vertex");
        nh[i] = (float)neutral_host[i];
        for (int j = 0; j < k; ++j) {
            const double d = blendshapes_host[i * k + j] - neutral_host[i];
            if (!std::isfinite(d)) return fail(ctx, "said_render_set_mesh: non-finite blendshape %d", j);
            bd[(size_t)j * n3 + i] = (float)d;
        }
    }
    // the two edges v1 - v0, v2 - v0 of every face, of the neutral and of every B_delta[k], in float64, each split into an fp32 pair hi + lo
    // (face_normals_kernel)
    std::vector<float> ne((size_t)nf * 12), eb((size_t)k * nf * 12);
    auto split = [](double x, float* hi, float* lo) { *hi = (float)x; *lo = (float)(x - (double)*hi); };
    for (int f = 0; f < nf; ++f)
        for (int j = 0; j < 2; ++j)
            for (int a = 0; a < 3; ++a) {
                const size_t i1 = (size_t)faces_host[f * 3 + j + 1] * 3 + a, i0 = (size_t)faces_host[f * 3] * 3 + a, c = (size_t)j * 3 + a;
                const double en = neutral_host[i1] - neutral_host[i0];
                split(en, &ne[(size_t)f * 12 + c], &ne[(size_t)f * 12 + 6 + c]);
                for (int b = 0; b < k; ++b) {
                    float* e = &eb[((size_t)b * nf + f) * 12];
                    split((blendshapes_host[i1 * k + b] - blendshapes_host[i0 * k + b]) - en, e + c, e + 6 + c);
                }
            }
    // incidence list: for every vertex its (face, corner) pairs in ascending face index
    std::vector<int> off(nv + 1, 0), inc((size_t)nf * 3);
    for (long long i = 0; i < 3LL * nf; ++i) ++off[faces_host[i] + 1];
    for (int v = 0; v < nv; ++v) off[v + 1] += off[v];
    {
        std::vector<int> cur(off.begin(), off.end() - 1);
        for (int f = 0; f < nf; ++f)
            for (int c = 0; c < 3; ++c) inc[cur[faces_host[f * 3 + c]]++] = f * 4 + c;
    }
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(s));
    r->nv = r->nf = r->k = 0;   // nothing to draw until every upload below has succeeded
    r->cap = r->last_n = 0;     // the workspace is sized by the mesh
    if (drealloc(ctx, &r->neutral, n3, false) || drealloc(ctx, &r->bdelta, bd.size(), false) || drealloc(ctx, &r->faces, (size_t)nf * 3, false) || drealloc(ctx, &r->nedge, ne.size(), false) || drealloc(ctx, &r->ebasis, eb.size(), false) ||
        drealloc(ctx, &r->inc_off, off.size(), false) || drealloc(ctx, &r->inc, inc.size(), false))
        return -1;
    HIPCHK(hipMemcpyAsync(r->neutral, nh.data(), sizeof(float) * n3, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(r->bdelta, bd.data(), sizeof(float) * bd.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(r->nedge, ne.data(), sizeof(float) * ne.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(r->ebasis, eb.data(), sizeof(float) * eb.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(r->faces, faces_host, sizeof(int) * nf * 3, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(r->inc_off, off.data(), sizeof(int) * off.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(r->inc, inc.data(), sizeof(int) * inc.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    r->nv = nv;
    r->nf = nf;
    r->k = k;
    return 0;
}

int said_render_set_scene(said_render* r, const said_render_scene* sc) {
    if (!r) return -1;
    HostCtx* ctx = &r->c;
    if (!sc) return fail(ctx, "said_render_set_scene: scene is null");
    if (sc->width < 1 || sc->height < 1 || sc->width > 16384 || sc->height > 16384) return fail(ctx, "said_render_set_scene: image of %d x %d (1 .. 16384)", sc->width, sc->height);
    if (!(sc->fx > 0.f) || !(sc->fy > 0.f) || !(sc->znear > 0.f) || !(sc->zfar > sc->znear) || !std::isfinite(sc->fx) || !std::isfinite(sc->fy) || !std::isfinite(sc->zfar) ||
        !std::isfinite(sc->cx) || !std::isfinite(sc->cy))
        return fail(ctx, "said_render_set_scene: need finite fx, fy > 0 and 0 < znear < zfar");
    if (sc->n_lights < 0 || sc->n_lights > SAID_RENDER_MAX_LIGHTS) return fail(ctx, "said_render_set_scene: %d lights (0 .. %d)", sc->n_lights, SAID_RENDER_MAX_LIGHTS);
    r->scene = *sc;
    r->has_scene = true;
    return 0;
}

int said_render_set_colormap(said_render* r, const float* lut_host, void* stream) {
    if (!r) return -1;
    HostCtx* ctx = &r->c;
    if (!lut_host) return fail(ctx, "said_render_set_colormap: lut is null");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(s));
    if (!r->lut && dalloc(ctx, &r->lut, (size_t)SAID_RENDER_LUT * 3, false)) return -1;
    HIPCHK(hipMemcpyAsync(r->lut, lut_host, sizeof(float) * SAID_RENDER_LUT * 3, hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    r->has_lut = true;
    return 0;
}

int said_render_render(said_render* r, const float* coeffs_dev, const float* target_dev, long long t0, int n_frames, float max_diff,
                       const double* rot_host, const double* t_center_host, unsigned char* out_u8_dev, int* face_ids_dev, void* stream) {
    if (!r) return -1;
    return render_chunk(r, "said_render_render", 1, coeffs_dev, target_dev, t0, n_frames, max_diff, rot_host, t_center_host, out_u8_dev, face_ids_dev, nullptr, stream);
}

int said_render_render_ms(said_render* r, int samples, const float* coeffs_dev, const float* target_dev, long long t0, int n_frames, float max_diff,
                          const double* rot_host, const double* t_center_host, unsigned char* out_u8_dev, int* face_ids_dev, int* sample_ids_dev,
                          void* stream) {
    if (!r) return -1;
    HostCtx* ctx = &r->c;
    const char* entry = "said_render_render_ms";
    if (samples != 1 && samples != 4) return fail(ctx, "%s: %d samples per pixel (1 or 4)", entry, samples);
    if (samples == 1 && sample_ids_dev) return fail(ctx, "%s: sample_ids_dev must be NULL at 1 sample (face_ids_dev receives the faces)", entry);
    if (samples == 4 && face_ids_dev) return fail(ctx, "%s: face_ids_dev must be NULL at 4 samples (sample_ids_dev receives the faces)", entry);
    if (((uintptr_t)sample_ids_dev & 15) != 0) return fail(ctx, "%s: sample_ids_dev must be 16-byte aligned", entry);
    return render_chunk(r, entry, samples, coeffs_dev, target_dev, t0, n_frames, max_diff, rot_host, t_center_host, out_u8_dev, face_ids_dev, sample_ids_dev, stream);
}

int said_render_read_vertices(said_render* r, int n_frames, float* out_host, void* stream) {
    return read_stage(r, "said_render_read_vertices", r ? r->verts : nullptr, n_frames, out_host, stream);
}
int said_render_read_normals(said_render* r, int n_frames, float* out_host, void* stream) {
    return read_stage(r, "said_render_read_normals", r ? r->normals : nullptr, n_frames, out_host, stream);
}
int said_render_read_colors(said_render* r, int n_frames, float* out_host, void* stream) {
    return read_stage(r, "said_render_read_colors", r ? r->colors : nullptr, n_frames, out_host, stream);
}

}  // extern "C"
