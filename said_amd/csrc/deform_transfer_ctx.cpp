// deform_transfer_ctx.cpp — host side of deformation transfer (C ABI: include/said_transfer.h; kernels: deform_transfer.hip; DESIGN.md section
// 18): the context, the checks of every index array before a kernel indexes with it, the uploads, the conjugate-gradient driver (rounds of
// iterations, the columns' flags read once per block of iterations) and the three stages.
#include "engine_internal.h"
#include "deform_transfer_kernels.h"
#include "../../include/said_transfer.h"

#include <cmath>

using namespace said::dt;

namespace {

struct DevMesh {
    int nv = 0, nf = 0;
    double *verts = nullptr, *w = nullptr, *gc = nullptr, *fn = nullptr, *cen = nullptr, *vn = nullptr;
    int *faces = nullptr, *vf_ptr = nullptr, *vf_idx = nullptr;
};

struct DevSystem {
    int m = 0, n = 0, nnz = 0;
    int *rowptr = nullptr, *col = nullptr, *c0 = nullptr, *c1 = nullptr, *rowclass = nullptr, *rowaux = nullptr, *rhsclass = nullptr, *at_rowptr = nullptr, *at_col = nullptr,
        *at_src = nullptr;
    double *val = nullptr, *at_val = nullptr;
};

}  // namespace

struct said_transfer {
    HostCtx c;
    DevMesh src, tgt, tmp;
    int k = 0;
    double* shapes = nullptr;          // (k, V_s, 3)
    double* reg = nullptr;             // (V_s, 3): the registered source
    bool has_reg = false;
    double tgt_diag = 0.0;
    DevSystem sys;
    // solver work
    double *b = nullptr, *x = nullptr, *r = nullptr, *z = nullptr, *p = nullptr, *sv = nullptr, *q = nullptr, *minv = nullptr, *part_a = nullptr, *part_b = nullptr,
           *part_c = nullptr;
    SolveState st{};
    // stage work
    double *weights = nullptr, *xfix = nullptr, *grad = nullptr, *nrm_work = nullptr, *fn_work = nullptr, *cen_work = nullptr, *d2 = nullptr, *out = nullptr;
    int* closest = nullptr;
    unsigned char* colfixed = nullptr;
};

namespace {

template <typename T>
int grow(HostCtx* ctx, T** p, size_t n) { return drealloc(ctx, p, n, false); }

template <typename T>
int up(HostCtx* ctx, T** dev, const T* host, size_t n) {
    if (grow(ctx, dev, n)) return -1;
    HIPCHK(hipMemcpy(*dev, host, sizeof(T) * n, hipMemcpyHostToDevice));
    return 0;
}

int check_csr(HostCtx* ctx, const char* what, const int* rowptr, const int* col, int nrows, int ncols, int nnz) {
    if (!rowptr || !col) return fail(ctx, "%s: null row pointers or columns", what);
    if (rowptr[0] != 0 || rowptr[nrows] != nnz) return fail(ctx, "%s: row pointers run from %d to %d, not from 0 to %d", what, rowptr[0], rowptr[nrows], nnz);
    for (int i = 0; i < nrows; ++i)
        if (rowptr[i + 1] < rowptr[i]) return fail(ctx, "%s: row pointers decrease at row %d", what, i);
    for (int j = 0; j < nnz; ++j)
        if (col[j] < 0 || col[j] >= ncols) return fail(ctx, "%s: entry %d names column %d of %d", what, j, col[j], ncols);
    return 0;
}

int check_faces(HostCtx* ctx, const char* what, int nv, int nf, const double* verts, const int* faces) {
    if (!verts || !faces || nv < 3 || nf < 1 || nv > (1 << 26) || nf > (1 << 26)) return fail(ctx, "%s: null vertices or faces, or %d vertices, %d faces", what, nv, nf);
    for (int i = 0; i < 3 * nf; ++i)
        if (faces[i] < 0 || faces[i] >= nv) return fail(ctx, "%s: face %d names vertex %d of %d", what, i / 3, faces[i], nv);
    return 0;
}

// uploads a mesh and runs its passes: frame inverses, face normals and centroids, vertex normals (the faces of a vertex in ascending order)
int load_mesh(HostCtx* ctx, DevMesh* ms, int nv, int nf, const double* verts, const int* faces, hipStream_t s) {
    ms->nv = ms->nf = 0;
    std::vector<int> ptr((size_t)nv + 1, 0), idx((size_t)nf * 3);
    for (int i = 0; i < 3 * nf; ++i) ++ptr[(size_t)faces[i] + 1];
    for (int v = 0; v < nv; ++v) ptr[(size_t)v + 1] += ptr[(size_t)v];
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (int f = 0; f < nf; ++f)
        for (int k = 0; k < 3; ++k) idx[(size_t)fill[(size_t)faces[3 * f + k]]++] = f;
    HIPCHK(hipStreamSynchronize(s));
    if (up(ctx, &ms->verts, verts, (size_t)nv * 3) || up(ctx, &ms->faces, faces, (size_t)nf * 3) || up(ctx, &ms->vf_ptr, ptr.data(), ptr.size()) ||
        up(ctx, &ms->vf_idx, idx.data(), idx.size()))
        return -1;
    if (grow(ctx, &ms->w, (size_t)nf * 9) || grow(ctx, &ms->gc, (size_t)nf * 12) || grow(ctx, &ms->fn, (size_t)nf * 3) || grow(ctx, &ms->cen, (size_t)nf * 3) ||
        grow(ctx, &ms->vn, (size_t)nv * 3))
        return -1;
    launch_frames(ms->verts, ms->faces, nf, ms->w, ms->gc, s);
    launch_face_normals(ms->verts, ms->faces, nf, ms->fn, ms->cen, s);
    launch_vertex_normals(ms->fn, ms->vf_ptr, ms->vf_idx, nv, ms->vn, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));
    ms->nv = nv;
    ms->nf = nf;
    return 0;
}

int solver_work(said_transfer* t, int m, int n, int R) {
    HostCtx* ctx = &t->c;
    const size_t nr = (size_t)n * R, nb = (size_t)n_blocks(n) * R;
    if (grow(ctx, &t->r, nr) || grow(ctx, &t->z, nr) || grow(ctx, &t->p, nr) || grow(ctx, &t->sv, nr) || grow(ctx, &t->q, (size_t)m * R) || grow(ctx, &t->minv, (size_t)n) ||
        grow(ctx, &t->part_a, nb) || grow(ctx, &t->part_b, nb) || grow(ctx, &t->part_c, nb) || grow(ctx, &t->st.rz, (size_t)2 * R) || grow(ctx, &t->st.active, (size_t)2 * R) ||
        grow(ctx, &t->st.bnorm2, (size_t)R) || grow(ctx, &t->st.rr, (size_t)R) || grow(ctx, &t->st.iters, (size_t)R) || grow(ctx, &t->st.status, (size_t)R))
        return -1;
    return 0;
}

bool any_active(const std::vector<int>& a) {
    for (int v : a)
        if (v) return true;
    return false;
}

// min |A x - b| per column from x (n, R) on the device; b (m, R).  The work buffers are sized by solver_work.
int pcg(said_transfer* t, Csr A, Csr AT, int R, const double* b, double* x, double tol, int max_iter, int check_every, int* status_host, int* iters_host, double* resid_host,
        hipStream_t s) {
    HostCtx* ctx = &t->c;
    const int n = AT.nrows, nb = n_blocks(n);
    const double tol2 = tol * tol;
    SolveState st = t->st;
    std::vector<int> flags((size_t)R);
    HIPCHK(hipMemsetAsync(st.iters, 0, sizeof(int) * (size_t)R, s));
    HIPCHK(hipMemsetAsync(st.status, 0xFF, sizeof(int) * (size_t)R, s));   // -1: running
    launch_column_norms(AT, t->minv, s);
    launch_spmv(2, AT, b, nullptr, t->r, t->part_a, R, nullptr, s);
    launch_reduce_columns(t->part_a, nb, R, st.bnorm2, s);
    HIPCHK(hipGetLastError());
    for (int round = 0; round <= SAID_TRANSFER_MAX_ROUNDS; ++round) {
        // the true residual A'(b - A x) of every column
        launch_spmv(1, A, x, b, t->q, nullptr, R, nullptr, s);
        launch_spmv(2, AT, t->q, nullptr, t->r, t->part_a, R, nullptr, s);
        launch_reduce_columns(t->part_a, nb, R, st.rr, s);
        launch_round(st, R, tol2, round == SAID_TRANSFER_MAX_ROUNDS, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(flags.data(), st.active, sizeof(int) * (size_t)R, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (!any_active(flags)) break;
        launch_precondition(n, R, t->r, t->minv, t->z, t->p, t->part_b, st.active, s);
        launch_reduce_columns(t->part_b, nb, R, st.rz, s);
        int cur = 0;
        for (long long launched = 0; launched <= (long long)max_iter + check_every; launched += check_every) {
            for (int i = 0; i < check_every; ++i) {
                const int* act = st.active + (size_t)cur * R;
                launch_spmv(0, A, t->p, nullptr, t->q, nullptr, R, act, s);
                launch_spmv(2, AT, t->q, t->p, t->sv, t->part_a, R, act, s);
                launch_update(n, R, x, t->r, t->p, t->sv, t->z, t->minv, t->part_a, st.rz + (size_t)cur * R, act, t->part_b, t->part_c, s);
                launch_direction(n, R, t->p, t->z, t->part_b, t->part_c, st, cur, tol2, max_iter, s);
                cur ^= 1;
            }
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(flags.data(), st.active + (size_t)cur * R, sizeof(int) * (size_t)R, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
            if (!any_active(flags)) break;
        }
    }
    std::vector<double> rr((size_t)R), bn((size_t)R);
    std::vector<int> status((size_t)R);
    HIPCHK(hipMemcpyAsync(rr.data(), st.rr, sizeof(double) * (size_t)R, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(bn.data(), st.bnorm2, sizeof(double) * (size_t)R, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(status.data(), st.status, sizeof(int) * (size_t)R, hipMemcpyDeviceToHost, s));
    if (iters_host) HIPCHK(hipMemcpyAsync(iters_host, st.iters, sizeof(int) * (size_t)R, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int c = 0; c < R; ++c) {
        if (status_host) status_host[c] = status[(size_t)c] < 0 ? SAID_TRANSFER_MAX_ITER : status[(size_t)c];
        if (resid_host) resid_host[c] = bn[(size_t)c] > 0.0 ? std::sqrt(rr[(size_t)c] / bn[(size_t)c]) : std::sqrt(rr[(size_t)c]);
    }
    return 0;
}

int check_solver_args(HostCtx* ctx, const char* what, int R, double tol, int max_iter, int check_every) {
    if (R < 1 || R > SAID_TRANSFER_MAX_COLUMNS) return fail(ctx, "%s: %d right-hand-side columns (1 .. %d)", what, R, (int)SAID_TRANSFER_MAX_COLUMNS);
    if (!(tol > 0.0) || max_iter < 1 || check_every < 1) return fail(ctx, "%s: tol %g, max_iter %d, check_every %d (all positive)", what, tol, max_iter, check_every);
    return 0;
}

// checks and uploads a system's structure against the mesh whose G table its values come from
int load_system(said_transfer* t, const char* what, const said_transfer_system* sy, const DevMesh& mesh, bool transfer, int aux_limit_closest, int nf_src) {
    HostCtx* ctx = &t->c;
    t->sys.m = 0;
    if (!sy) return fail(ctx, "%s: null system", what);
    const int m = sy->m, n = sy->n, nnz = sy->nnz;
    if (m < 1 || nnz < 1 || n != mesh.nv + mesh.nf) return fail(ctx, "%s: a system of %d rows, %d entries and %d unknowns for a mesh with %d", what, m, nnz, n, mesh.nv + mesh.nf);
    if ((long long)m * 3 > (1LL << 30)) return fail(ctx, "%s: %d rows", what, m);
    if (check_csr(ctx, what, sy->rowptr, sy->col, m, n, nnz) || check_csr(ctx, what, sy->at_rowptr, sy->at_col, n, m, nnz)) return -1;
    if (!sy->c0 || !sy->c1 || !sy->rowclass || !sy->rowaux || !sy->at_src || (transfer && !sy->rhsclass)) return fail(ctx, "%s: a null array in the system", what);
    const int ncoef = 12 * mesh.nf;
    for (int j = 0; j < nnz; ++j) {
        if (sy->c0[j] < -2 || sy->c0[j] >= ncoef || sy->c1[j] < -1 || sy->c1[j] >= ncoef) return fail(ctx, "%s: entry %d names coefficients %d and %d of %d", what, j, sy->c0[j], sy->c1[j], ncoef);
        if (sy->at_src[j] < 0 || sy->at_src[j] >= nnz) return fail(ctx, "%s: transposed entry %d takes its value from entry %d of %d", what, j, sy->at_src[j], nnz);
    }
    for (int i = 0; i < m; ++i) {
        const int cls = sy->rowclass[i], aux = sy->rowaux[i];
        if (cls < 0 || cls > SAID_TRANSFER_ROW_UNIT) return fail(ctx, "%s: row %d has class %d", what, i, cls);
        if (!transfer) {
            if (cls == SAID_TRANSFER_ROW_CLOSEST && (aux < 0 || aux >= aux_limit_closest)) return fail(ctx, "%s: closest-point row %d names vertex %d of %d", what, i, aux, aux_limit_closest);
            if (cls == SAID_TRANSFER_ROW_IDENTITY && (aux < 0 || aux > 2)) return fail(ctx, "%s: identity row %d names row %d of the identity", what, i, aux);
        } else {
            const int rc = sy->rhsclass[i];
            const int limit = rc == SAID_TRANSFER_RHS_PAIR ? 3 * nf_src : rc == SAID_TRANSFER_RHS_IDENTITY ? 3 : rc == SAID_TRANSFER_RHS_ANCHOR ? mesh.nv : 0;
            if (cls == SAID_TRANSFER_ROW_CLOSEST || aux < 0 || aux >= limit) return fail(ctx, "%s: row %d has right-hand-side class %d and names %d of %d", what, i, rc, aux, limit);
        }
    }
    DevSystem& d = t->sys;
    const size_t z = (size_t)nnz;
    if (up(ctx, &d.rowptr, sy->rowptr, (size_t)m + 1) || up(ctx, &d.col, sy->col, z) || up(ctx, &d.c0, sy->c0, z) || up(ctx, &d.c1, sy->c1, z) ||
        up(ctx, &d.rowclass, sy->rowclass, (size_t)m) || up(ctx, &d.rowaux, sy->rowaux, (size_t)m) || up(ctx, &d.at_rowptr, sy->at_rowptr, (size_t)n + 1) ||
        up(ctx, &d.at_col, sy->at_col, z) || up(ctx, &d.at_src, sy->at_src, z) || grow(ctx, &d.val, z) || grow(ctx, &d.at_val, z))
        return -1;
    if (transfer && up(ctx, &d.rhsclass, sy->rhsclass, (size_t)m)) return -1;
    d.m = m;
    d.n = n;
    d.nnz = nnz;
    return 0;
}

}  // namespace

extern "C" {

int said_transfer_create(said_transfer** out, int device) {
    DeviceRestore restore_device;
    said_transfer* t = new_ctx("said_transfer_create", out, device);
    if (!t) return -1;
    *out = t;
    return 0;
}

int said_transfer_destroy(said_transfer* t) { return delete_ctx(t); }

const char* said_transfer_last_error(const said_transfer* t) { return ctx_error(t); }

int said_transfer_set_source(said_transfer* t, int nv, int nf, int k, const double* neutral_host, const int* faces_host, const double* shapes_host, void* stream) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    t->src.nv = 0;
    t->has_reg = false;
    if (check_faces(ctx, "said_transfer_set_source", nv, nf, neutral_host, faces_host)) return -1;
    if (k < 0 || 3 * k > SAID_TRANSFER_MAX_COLUMNS || (k > 0 && !shapes_host)) return fail(ctx, "said_transfer_set_source: %d shapes (0 .. %d), or null shapes", k, (int)SAID_TRANSFER_MAX_COLUMNS / 3);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    if (load_mesh(ctx, &t->src, nv, nf, neutral_host, faces_host, s)) return -1;
    if (k > 0 && up(ctx, &t->shapes, shapes_host, (size_t)k * nv * 3)) return -1;
    t->k = k;
    return 0;
}

int said_transfer_set_target(said_transfer* t, int nv, int nf, const double* neutral_host, const int* faces_host, void* stream) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    t->tgt.nv = 0;
    if (check_faces(ctx, "said_transfer_set_target", nv, nf, neutral_host, faces_host)) return -1;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    if (load_mesh(ctx, &t->tgt, nv, nf, neutral_host, faces_host, s)) return -1;
    double lo[3], hi[3], d2 = 0.0;
    for (int c = 0; c < 3; ++c) lo[c] = hi[c] = neutral_host[c];
    for (int v = 0; v < nv; ++v)
        for (int c = 0; c < 3; ++c) {
            lo[c] = std::min(lo[c], neutral_host[3 * (size_t)v + c]);
            hi[c] = std::max(hi[c], neutral_host[3 * (size_t)v + c]);
        }
    for (int c = 0; c < 3; ++c) d2 += (hi[c] - lo[c]) * (hi[c] - lo[c]);
    t->tgt_diag = std::sqrt(d2);
    return 0;
}

int said_transfer_solve(said_transfer* t, int m, int n, int nnz, int R, const int* a_rowptr_host, const int* a_col_host, const double* a_val_host, const int* at_rowptr_host,
                        const int* at_col_host, const double* at_val_host, const double* b_host, const double* x0_host, double tol, int max_iter, int check_every,
                        double* x_host, int* status_host, int* iters_host, double* resid_host, void* stream) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (m < 1 || n < 1 || nnz < 1 || (long long)m * 3 > (1LL << 30) || (long long)n * 3 > (1LL << 30)) return fail(ctx, "said_transfer_solve: a system of %d rows, %d unknowns and %d entries", m, n, nnz);
    if (check_solver_args(ctx, "said_transfer_solve", R, tol, max_iter, check_every)) return -1;
    if (!a_val_host || !at_val_host || !b_host || !x_host) return fail(ctx, "said_transfer_solve: null values, right-hand side or solution");
    if (check_csr(ctx, "said_transfer_solve (A)", a_rowptr_host, a_col_host, m, n, nnz) || check_csr(ctx, "said_transfer_solve (A')", at_rowptr_host, at_col_host, n, m, nnz)) return -1;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(s));
    DevSystem& d = t->sys;
    d.m = 0;
    const size_t z = (size_t)nnz;
    if (up(ctx, &d.rowptr, a_rowptr_host, (size_t)m + 1) || up(ctx, &d.col, a_col_host, z) || up(ctx, &d.val, a_val_host, z) || up(ctx, &d.at_rowptr, at_rowptr_host, (size_t)n + 1) ||
        up(ctx, &d.at_col, at_col_host, z) || up(ctx, &d.at_val, at_val_host, z) || up(ctx, &t->b, b_host, (size_t)m * R) || grow(ctx, &t->x, (size_t)n * R) || solver_work(t, m, n, R))
        return -1;
    if (x0_host) HIPCHK(hipMemcpy(t->x, x0_host, sizeof(double) * (size_t)n * R, hipMemcpyHostToDevice));
    else HIPCHK(hipMemset(t->x, 0, sizeof(double) * (size_t)n * R));
    const Csr A{d.rowptr, d.col, d.val, m}, AT{d.at_rowptr, d.at_col, d.at_val, n};
    if (pcg(t, A, AT, R, t->b, t->x, tol, max_iter, check_every, status_host, iters_host, resid_host, s)) return -1;
    HIPCHK(hipMemcpy(x_host, t->x, sizeof(double) * (size_t)n * R, hipMemcpyDeviceToHost));
    return 0;
}

int said_transfer_register(said_transfer* t, const said_transfer_system* sys, int n_markers, const int* marker_src_host, const double* marker_pos_host, double w_s, double w_i,
                           int n_solves, const double* wc_host, double tol, int max_iter, double* x_host, int* closest_host, int* status_host, int* iters_host,
                           double* resid_host, void* stream) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    const char* what = "said_transfer_register";
    t->has_reg = false;
    if (!t->src.nv || !t->tgt.nv) return fail(ctx, "%s: needs the source and the target first (said_transfer_set_source, said_transfer_set_target)", what);
    if (check_solver_args(ctx, what, 3, tol, max_iter, 1)) return -1;
    if (n_markers < 0 || (n_markers > 0 && (!marker_src_host || !marker_pos_host)) || n_solves < 1 || !wc_host || !x_host || !(w_s >= 0.0) || !(w_i >= 0.0))
        return fail(ctx, "%s: null markers, weights or solution, or %d markers, %d solves, w_s %g, w_i %g", what, n_markers, n_solves, w_s, w_i);
    if (wc_host[0] != 0.0) return fail(ctx, "%s: the first solve has no earlier solution to take closest points from: its weight must be 0, not %g", what, wc_host[0]);
    const int nv = t->src.nv, n = t->src.nv + t->src.nf;
    std::vector<unsigned char> fixed((size_t)n, 0);
    std::vector<double> xfix((size_t)n * 3, 0.0);
    for (int i = 0; i < n_markers; ++i) {
        const int v = marker_src_host[i];
        if (v < 0 || v >= nv) return fail(ctx, "%s: marker %d names source vertex %d of %d", what, i, v, nv);
        if (fixed[(size_t)v]) return fail(ctx, "%s: source vertex %d is a marker twice", what, v);
        fixed[(size_t)v] = 1;
        for (int c = 0; c < 3; ++c) xfix[3 * (size_t)v + c] = marker_pos_host[3 * i + c];
    }
    for (int j = 0; j < n_solves; ++j)
        if (!(wc_host[j] >= 0.0)) return fail(ctx, "%s: closest-point weight %g of solve %d", what, wc_host[j], j);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(s));
    if (load_system(t, what, sys, t->src, false, nv, 0)) return -1;
    const DevSystem& d = t->sys;
    const int m = d.m;
    if (up(ctx, &t->colfixed, fixed.data(), fixed.size()) || up(ctx, &t->xfix, xfix.data(), xfix.size()) || grow(ctx, &t->b, (size_t)m * 3) || grow(ctx, &t->x, (size_t)n * 3) ||
        grow(ctx, &t->weights, (size_t)4) || grow(ctx, &t->closest, (size_t)nv) || grow(ctx, &t->fn_work, (size_t)t->src.nf * 3) || grow(ctx, &t->nrm_work, (size_t)nv * 3) ||
        grow(ctx, &t->reg, (size_t)nv * 3) || solver_work(t, m, n, 3))
        return -1;
    // the start: the fixed vertices at their positions, everything else at 0; later solves start from the one before
    HIPCHK(hipMemcpy(t->x, xfix.data(), sizeof(double) * xfix.size(), hipMemcpyHostToDevice));
    const Csr A{d.rowptr, d.col, d.val, m}, AT{d.at_rowptr, d.at_col, d.at_val, n};
    for (int j = 0; j < n_solves; ++j) {
        const double wts[4] = {std::sqrt(w_s), std::sqrt(w_i), std::sqrt(wc_host[j]), 1.0};
        HIPCHK(hipMemcpy(t->weights, wts, sizeof(wts), hipMemcpyHostToDevice));
        if (wc_host[j] > 0.0) {   // the first nv rows of x are the deformed source's vertices
            launch_face_normals(t->x, t->src.faces, t->src.nf, t->fn_work, nullptr, s);
            launch_vertex_normals(t->fn_work, t->src.vf_ptr, t->src.vf_idx, nv, t->nrm_work, s);
            launch_closest(t->x, t->nrm_work, nv, t->tgt.verts, t->tgt.vn, t->tgt.nv, t->closest, nullptr, s);
        } else {
            HIPCHK(hipMemsetAsync(t->closest, 0xFF, sizeof(int) * (size_t)nv, s));
        }
        // the right-hand side with the fixed columns of the full matrix carried over, then the matrix without them
        launch_fill_values(d.rowptr, d.col, d.c0, d.c1, d.rowclass, d.rowaux, m, t->src.gc, t->weights, t->closest, nullptr, d.val, s);
        launch_register_rhs(d.rowclass, d.rowaux, m, t->weights, t->closest, t->tgt.verts, t->b, s);
        launch_spmv(1, A, t->xfix, t->b, t->b, nullptr, 3, nullptr, s);
        launch_fill_values(d.rowptr, d.col, d.c0, d.c1, d.rowclass, d.rowaux, m, t->src.gc, t->weights, t->closest, t->colfixed, d.val, s);
        launch_gather(d.at_src, d.val, d.nnz, d.at_val, s);
        HIPCHK(hipGetLastError());
        if (pcg(t, A, AT, 3, t->b, t->x, tol, max_iter, 50, status_host ? status_host + 3 * j : nullptr, iters_host ? iters_host + 3 * j : nullptr,
                resid_host ? resid_host + 3 * j : nullptr, s))
            return -1;
        HIPCHK(hipMemcpy(x_host + (size_t)j * n * 3, t->x, sizeof(double) * (size_t)n * 3, hipMemcpyDeviceToHost));
        if (closest_host) HIPCHK(hipMemcpy(closest_host + (size_t)j * nv, t->closest, sizeof(int) * (size_t)nv, hipMemcpyDeviceToHost));
    }
    HIPCHK(hipMemcpy(t->reg, t->x, sizeof(double) * (size_t)nv * 3, hipMemcpyDeviceToDevice));
    t->has_reg = true;
    return 0;
}

int said_transfer_correspond(said_transfer* t, const double* reg_host, double threshold, int* t2s_host, int* s2t_host, double* t2s_d2_host, double* s2t_d2_host, void* stream) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    const char* what = "said_transfer_correspond";
    if (!t->src.nv || !t->tgt.nv) return fail(ctx, "%s: needs the source and the target first", what);
    if (!reg_host && !t->has_reg) return fail(ctx, "%s: no registered source (said_transfer_register, or pass one)", what);
    if (!t2s_host || !s2t_host || !(threshold >= 0.0)) return fail(ctx, "%s: null outputs, or threshold %g", what, threshold);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(s));
    const int nv = t->src.nv, fs = t->src.nf, ft = t->tgt.nf, most = std::max(fs, ft);
    if (reg_host) {
        if (up(ctx, &t->reg, reg_host, (size_t)nv * 3)) return -1;
        t->has_reg = true;
    }
    if (grow(ctx, &t->fn_work, (size_t)fs * 3) || grow(ctx, &t->cen_work, (size_t)fs * 3) || grow(ctx, &t->closest, (size_t)most) || grow(ctx, &t->d2, (size_t)most)) return -1;
    launch_face_normals(t->reg, t->src.faces, fs, t->fn_work, t->cen_work, s);
    const double limit = threshold * t->tgt_diag;
    std::vector<double> d2((size_t)most);
    for (int dir = 0; dir < 2; ++dir) {
        const int nq = dir == 0 ? ft : fs;
        int* idx_host = dir == 0 ? t2s_host : s2t_host;
        double* d2_host = dir == 0 ? t2s_d2_host : s2t_d2_host;
        if (dir == 0) launch_closest(t->tgt.cen, t->tgt.fn, ft, t->cen_work, t->fn_work, fs, t->closest, t->d2, s);
        else launch_closest(t->cen_work, t->fn_work, fs, t->tgt.cen, t->tgt.fn, ft, t->closest, t->d2, s);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(idx_host, t->closest, sizeof(int) * (size_t)nq, hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(d2.data(), t->d2, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int i = 0; i < nq; ++i) {
            if (idx_host[i] >= 0 && !(std::sqrt(d2[(size_t)i]) <= limit)) idx_host[i] = -1;
            if (d2_host) d2_host[i] = d2[(size_t)i];
        }
    }
    return 0;
}

int said_transfer_transfer(said_transfer* t, const said_transfer_system* sys, double tol, int max_iter, double* residuals_host, int* status_host, int* iters_host,
                           double* resid_host, void* stream) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    const char* what = "said_transfer_transfer";
    if (!t->src.nv || !t->tgt.nv || t->k < 1) return fail(ctx, "%s: needs a source with shapes and the target first", what);
    const int K = t->k, R = 3 * K;
    if (check_solver_args(ctx, what, R, tol, max_iter, 1)) return -1;
    if (!residuals_host) return fail(ctx, "%s: null residuals", what);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(s));
    if (load_system(t, what, sys, t->tgt, true, 0, t->src.nf)) return -1;
    const DevSystem& d = t->sys;
    const int m = d.m, n = d.n, nv = t->tgt.nv;
    if ((long long)m * R > (1LL << 31) - 1 || (long long)n * R > (1LL << 31) - 1) return fail(ctx, "%s: %d rows x %d columns", what, m, R);
    if (grow(ctx, &t->b, (size_t)m * R) || grow(ctx, &t->x, (size_t)n * R) || grow(ctx, &t->weights, (size_t)4) || grow(ctx, &t->grad, (size_t)K * t->src.nf * 9) ||
        grow(ctx, &t->closest, (size_t)1) || grow(ctx, &t->out, (size_t)K * nv * 3) || solver_work(t, m, n, R))
        return -1;
    const double wts[4] = {0.0, 0.0, 0.0, 1.0};
    HIPCHK(hipMemcpy(t->weights, wts, sizeof(wts), hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(t->x, 0, sizeof(double) * (size_t)n * R, s));
    launch_gradients(t->src.w, t->shapes, K, t->src.nv, t->src.faces, t->src.nf, t->grad, s);
    launch_fill_values(d.rowptr, d.col, d.c0, d.c1, d.rowclass, d.rowaux, m, t->tgt.gc, t->weights, t->closest, nullptr, d.val, s);
    launch_gather(d.at_src, d.val, d.nnz, d.at_val, s);
    launch_transfer_rhs(d.rhsclass, d.rowaux, m, K, t->grad, t->src.nf, t->tgt.verts, t->b, s);
    HIPCHK(hipGetLastError());
    const Csr A{d.rowptr, d.col, d.val, m}, AT{d.at_rowptr, d.at_col, d.at_val, n};
    if (pcg(t, A, AT, R, t->b, t->x, tol, max_iter, 50, status_host, iters_host, resid_host, s)) return -1;
    launch_residuals(t->x, t->tgt.verts, nv, K, t->out, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(residuals_host, t->out, sizeof(double) * (size_t)K * nv * 3, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int said_transfer_mesh(said_transfer* t, int nv, int nf, const double* verts_host, const int* faces_host, double* w_host, double* gc_host, double* fn_host,
                       double* centroid_host, double* vn_host, void* stream) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (check_faces(ctx, "said_transfer_mesh", nv, nf, verts_host, faces_host)) return -1;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    if (load_mesh(ctx, &t->tmp, nv, nf, verts_host, faces_host, s)) return -1;
    if (w_host) HIPCHK(hipMemcpy(w_host, t->tmp.w, sizeof(double) * (size_t)nf * 9, hipMemcpyDeviceToHost));
    if (gc_host) HIPCHK(hipMemcpy(gc_host, t->tmp.gc, sizeof(double) * (size_t)nf * 12, hipMemcpyDeviceToHost));
    if (fn_host) HIPCHK(hipMemcpy(fn_host, t->tmp.fn, sizeof(double) * (size_t)nf * 3, hipMemcpyDeviceToHost));
    if (centroid_host) HIPCHK(hipMemcpy(centroid_host, t->tmp.cen, sizeof(double) * (size_t)nf * 3, hipMemcpyDeviceToHost));
    if (vn_host) HIPCHK(hipMemcpy(vn_host, t->tmp.vn, sizeof(double) * (size_t)nv * 3, hipMemcpyDeviceToHost));
    return 0;
}

int said_transfer_gradients(said_transfer* t, int nv, int nf, const double* ref_host, const int* faces_host, int k, const double* deformed_host, double* q_host,
                            void* stream) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (check_faces(ctx, "said_transfer_gradients", nv, nf, ref_host, faces_host)) return -1;
    if (k < 1 || k > 256 || !deformed_host || !q_host) return fail(ctx, "said_transfer_gradients: %d shapes (1 .. 256), or a null array", k);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    if (load_mesh(ctx, &t->tmp, nv, nf, ref_host, faces_host, s)) return -1;
    if (up(ctx, &t->out, deformed_host, (size_t)k * nv * 3) || grow(ctx, &t->grad, (size_t)k * nf * 9)) return -1;
    launch_gradients(t->tmp.w, t->out, k, nv, t->tmp.faces, nf, t->grad, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(q_host, t->grad, sizeof(double) * (size_t)k * nf * 9, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

int said_transfer_closest(said_transfer* t, int nq, const double* qpos_host, const double* qnrm_host, int nt, const double* tpos_host, const double* tnrm_host,
                          int* idx_host, double* d2_host, void* stream) {
    if (!t) return -1;
    HostCtx* ctx = &t->c;
    if (nq < 1 || nt < 1 || nq > (1 << 26) || nt > (1 << 26) || !qpos_host || !tpos_host || !idx_host || (qnrm_host == nullptr) != (tnrm_host == nullptr))
        return fail(ctx, "said_transfer_closest: %d queries, %d targets, a null array, or normals on one side only", nq, nt);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(s));
    // the four inputs share one buffer: query positions, query normals, target positions, target normals
    const size_t q3 = (size_t)nq * 3, t3 = (size_t)nt * 3;
    if (grow(ctx, &t->out, 2 * q3 + 2 * t3) || grow(ctx, &t->closest, (size_t)nq) || grow(ctx, &t->d2, (size_t)nq)) return -1;
    double *qp = t->out, *qn = qp + q3, *tp = qn + q3, *tn = tp + t3;
    HIPCHK(hipMemcpy(qp, qpos_host, sizeof(double) * q3, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(tp, tpos_host, sizeof(double) * t3, hipMemcpyHostToDevice));
    if (qnrm_host) {
        HIPCHK(hipMemcpy(qn, qnrm_host, sizeof(double) * q3, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(tn, tnrm_host, sizeof(double) * t3, hipMemcpyHostToDevice));
    }
    launch_closest(qp, qnrm_host ? qn : nullptr, nq, tp, qnrm_host ? tn : nullptr, nt, t->closest, t->d2, s);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(idx_host, t->closest, sizeof(int) * (size_t)nq, hipMemcpyDeviceToHost, s));
    if (d2_host) HIPCHK(hipMemcpyAsync(d2_host, t->d2, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

}  // extern "C"
