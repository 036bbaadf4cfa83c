// deform_transfer.hip — kernels of deformation transfer (host side: deform_transfer_ctx.cpp; C ABI: include/said_transfer.h).
//
// Everything is float64.  Mesh passes: frame inverses W = V^-T and the four coefficients per row of G_t, deformation gradients, face and
// vertex normals, the brute-force closest compatible point.  System passes: the values of a host-built CSR structure and the right-hand
// sides.  Solver: Jacobi-preconditioned conjugate gradients on A'A x = A'b with A and A' both in CSR and R right-hand-side columns in a
// row-major (n, R) block.
//
// Thread layout of every kernel over an (n, R) block: a workgroup owns ROWS_PER_BLOCK = 64 rows and a tile of CW = min(64, next power of two
// >= R) columns; thread t works on column t % CW (lanes across R) and on rows t / CW, t / CW + 256 / CW, ...  Sums: a matrix row is summed
// in the order of its CSR entries; a dot product is summed first over the 64 rows of a workgroup in ascending order by one thread per
// column (from LDS), then over the workgroups in ascending order (sum_partials, which every consumer repeats for itself).  Neither order
// depends on R or CW, there are no atomics, and a column never reads another column's data: equal inputs give bit-identical outputs, and a
// column's result does not depend on the columns solved beside it.
#include "deform_transfer_kernels.h"

namespace said {
namespace dt {

namespace {

constexpr int THREADS = 256;

struct Tile {
    int cw_log2, cw, c_local, rl, rlanes, c;
};

__device__ inline Tile tile_of(int cw_log2) {
    Tile t;
    t.cw_log2 = cw_log2;
    t.cw = 1 << cw_log2;
    t.c_local = (int)threadIdx.x & (t.cw - 1);
    t.rl = (int)threadIdx.x >> cw_log2;
    t.rlanes = THREADS >> cw_log2;
    t.c = (int)blockIdx.y * t.cw + t.c_local;
    return t;
}

inline int cw_log2_of(int R) {
    int l = 0;
    while ((1 << l) < R && (1 << l) < MAX_TILE) ++l;
    return l;
}

inline dim3 grid_of(int rows, int R) {
    const int cw = 1 << cw_log2_of(R);
    return dim3((unsigned)n_blocks(rows), (unsigned)((R + cw - 1) / cw));
}

// second reduction stage: the workgroups' partials of column c in ascending order
__device__ inline double sum_partials(const double* partial, int nb, int R, int c) {
    double s = 0.0;
    int b = 0;
    for (; b + 8 <= nb; b += 8) {   // eight loads in flight, added in the same ascending order
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = partial[(size_t)(b + k) * R + c];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += v[k];
    }
    for (; b < nb; ++b) s += partial[(size_t)b * R + c];
    return s;
}

// first reduction stage: red holds (64, cw) products; one thread per column sums its 64 rows in ascending order
__device__ inline void reduce_rows(const double* red, const Tile& t, int R, double* partial) {
    __syncthreads();
    if (t.rl == 0 && t.c < R) {
        double s = 0.0;
        for (int lr = 0; lr < ROWS_PER_BLOCK; ++lr) s += red[lr * t.cw + t.c_local];
        partial[(size_t)blockIdx.x * R + t.c] = s;
    }
    __syncthreads();
}

__device__ inline void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// the frame of triangle f: e[0] = v2 - v1, e[1] = v3 - v1, e[2] = n / sqrt(|n|)
__device__ inline void frame_of(const double* verts, const int* faces, int f, double e[3][3]) {
    const int i1 = faces[3 * f], i2 = faces[3 * f + 1], i3 = faces[3 * f + 2];
    for (int k = 0; k < 3; ++k) {
        e[0][k] = verts[3 * (size_t)i2 + k] - verts[3 * (size_t)i1 + k];
        e[1][k] = verts[3 * (size_t)i3 + k] - verts[3 * (size_t)i1 + k];
    }
    cross3(e[0], e[1], e[2]);
    const double len = sqrt((e[2][0] * e[2][0] + e[2][1] * e[2][1]) + e[2][2] * e[2][2]);
    const double sc = sqrt(len);
    for (int k = 0; k < 3; ++k) e[2][k] /= sc;
}

__global__ __launch_bounds__(THREADS) void frames_kernel(const double* verts, const int* faces, int nf, double* w, double* gc) {
    const int f = (int)(blockIdx.x * THREADS + threadIdx.x);
    if (f >= nf) return;
    double e[3][3], bc[3], ca[3], ab[3];
    frame_of(verts, faces, f, e);
    cross3(e[1], e[2], bc);
    cross3(e[2], e[0], ca);
    cross3(e[0], e[1], ab);
    const double det = (e[0][0] * bc[0] + e[0][1] * bc[1]) + e[0][2] * bc[2];
    for (int r = 0; r < 3; ++r) {
        const double w0 = bc[r] / det, w1 = ca[r] / det, w2 = ab[r] / det;   // row r of W = V^-T
        if (w) {
            w[9 * (size_t)f + 3 * r] = w0;
            w[9 * (size_t)f + 3 * r + 1] = w1;
            w[9 * (size_t)f + 3 * r + 2] = w2;
        }
        if (gc) {   // row r of G_t: the coefficients of x1, x2, x3, x4
            gc[12 * (size_t)f + 4 * r] = -((w0 + w1) + w2);
            gc[12 * (size_t)f + 4 * r + 1] = w0;
            gc[12 * (size_t)f + 4 * r + 2] = w1;
            gc[12 * (size_t)f + 4 * r + 3] = w2;
        }
    }
}

// Q = V~ V^-1: Q[i][j] = sum_k V~[i][k] W[j][k]; blockIdx.y is the shape
__global__ __launch_bounds__(THREADS) void gradients_kernel(const double* w_ref, const double* deformed, int nv, const int* faces, int nf, double* q) {
    const int f = (int)(blockIdx.x * THREADS + threadIdx.x);
    if (f >= nf) return;
    const size_t shape = blockIdx.y;
    double e[3][3];
    frame_of(deformed + shape * 3 * (size_t)nv, faces, f, e);
    const double* w = w_ref + 9 * (size_t)f;
    double* out = q + (shape * (size_t)nf + f) * 9;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[3 * i + j] = (e[0][i] * w[3 * j] + e[1][i] * w[3 * j + 1]) + e[2][i] * w[3 * j + 2];
}

__global__ __launch_bounds__(THREADS) void face_normals_kernel(const double* verts, const int* faces, int nf, double* fn, double* centroid) {
    const int f = (int)(blockIdx.x * THREADS + threadIdx.x);
    if (f >= nf) return;
    const int i1 = faces[3 * f], i2 = faces[3 * f + 1], i3 = faces[3 * f + 2];
    double a[3], b[3], n[3];
    for (int k = 0; k < 3; ++k) {
        a[k] = verts[3 * (size_t)i2 + k] - verts[3 * (size_t)i1 + k];
        b[k] = verts[3 * (size_t)i3 + k] - verts[3 * (size_t)i1 + k];
    }
    cross3(a, b, n);
    for (int k = 0; k < 3; ++k) {
        fn[3 * (size_t)f + k] = n[k];
        if (centroid) centroid[3 * (size_t)f + k] = ((verts[3 * (size_t)i1 + k] + verts[3 * (size_t)i2 + k]) + verts[3 * (size_t)i3 + k]) / 3.0;
    }
}

// the faces of a vertex in ascending order (vf_ptr, vf_idx: built on the host), so no atomics
__global__ __launch_bounds__(THREADS) void vertex_normals_kernel(const double* fn, const int* vf_ptr, const int* vf_idx, int nv, double* vn) {
    const int v = (int)(blockIdx.x * THREADS + threadIdx.x);
    if (v >= nv) return;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int j = vf_ptr[v]; j < vf_ptr[v + 1]; ++j) {
        const size_t f = (size_t)vf_idx[j];
        s0 += fn[3 * f];
        s1 += fn[3 * f + 1];
        s2 += fn[3 * f + 2];
    }
    const double len = sqrt((s0 * s0 + s1 * s1) + s2 * s2);
    vn[3 * (size_t)v] = s0 / len;
    vn[3 * (size_t)v + 1] = s1 / len;
    vn[3 * (size_t)v + 2] = s2 / len;
}

// one thread per query, the targets staged through LDS in tiles of 256; a strict < in ascending order gives ties to the lower index
__global__ __launch_bounds__(THREADS) void closest_kernel(const double* qpos, const double* qnrm, int nq, const double* tpos, const double* tnrm, int nt, int* idx,
                                                          double* d2out) {
    __shared__ double tp[THREADS * 3], tn[THREADS * 3];
    const int q = (int)(blockIdx.x * THREADS + threadIdx.x);
    const bool live = q < nq;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0;
    if (live) {
        p0 = qpos[3 * (size_t)q];
        p1 = qpos[3 * (size_t)q + 1];
        p2 = qpos[3 * (size_t)q + 2];
        if (qnrm) {
            n0 = qnrm[3 * (size_t)q];
            n1 = qnrm[3 * (size_t)q + 1];
            n2 = qnrm[3 * (size_t)q + 2];
        }
    }
    int best = -1;
    double bestd = HUGE_VAL;
    for (int t0 = 0; t0 < nt; t0 += THREADS) {
        const int cnt = min(THREADS, nt - t0);
        __syncthreads();
        for (int i = (int)threadIdx.x; i < cnt * 3; i += THREADS) {
            tp[i] = tpos[3 * (size_t)t0 + i];
            tn[i] = qnrm ? tnrm[3 * (size_t)t0 + i] : 0.0;
        }
        __syncthreads();
        if (!live) continue;
        for (int i = 0; i < cnt; ++i) {
            if (qnrm && !((n0 * tn[3 * i] + n1 * tn[3 * i + 1]) + n2 * tn[3 * i + 2] > 0.0)) continue;
            const double dx = p0 - tp[3 * i], dy = p1 - tp[3 * i + 1], dz = p2 - tp[3 * i + 2];
            const double d = (dx * dx + dy * dy) + dz * dz;
            if (d < bestd) {
                bestd = d;
                best = t0 + i;
            }
        }
    }
    if (live) {
        idx[q] = best;
        if (d2out) d2out[q] = bestd;
    }
}

// values of a system: entry j of row i is weight(row) * (term(c0[j]) - term(c1[j])), a term being a coefficient of gc (>= 0), nothing (-1) or, for c0, 1
// (-2); a closest-point row of a vertex without a compatible point weighs 0; a fixed column is emptied
__global__ __launch_bounds__(THREADS) void fill_values_kernel(const int* rowptr, const int* col, const int* c0, const int* c1, const int* rowclass, const int* rowaux, int m,
                                                              const double* gc, const double* weights, const int* closest, const unsigned char* colfixed, double* val) {
    const int i = (int)(blockIdx.x * THREADS + threadIdx.x);
    if (i >= m) return;
    const int cls = rowclass[i];
    double w = weights[cls];
    if (cls == ROW_CLOSEST && closest[rowaux[i]] < 0) w = 0.0;
    for (int j = rowptr[i]; j < rowptr[i + 1]; ++j) {
        const double t0 = c0[j] >= 0 ? gc[c0[j]] : c0[j] == -2 ? 1.0 : 0.0, t1 = c1[j] >= 0 ? gc[c1[j]] : 0.0;
        double v = w * (t0 - t1);
        if (colfixed && colfixed[col[j]]) v = 0.0;
        val[j] = v;
    }
}

__global__ __launch_bounds__(THREADS) void gather_kernel(const int* src, const double* in, long long n, double* out) {
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (i < n) out[i] = in[src[i]];
}

__global__ __launch_bounds__(THREADS) void register_rhs_kernel(const int* rowclass, const int* rowaux, int m, const double* weights, const int* closest, const double* tpos,
                                                               double* b) {
    const int i = (int)(blockIdx.x * THREADS + threadIdx.x);
    if (i >= m) return;
    const int cls = rowclass[i], aux = rowaux[i];
    const double w = weights[cls];
    for (int c = 0; c < 3; ++c) {
        double v = 0.0;
        if (cls == ROW_IDENTITY) v = aux == c ? w : 0.0;
        if (cls == ROW_CLOSEST) {
            const int t = closest[aux];
            v = t >= 0 ? w * tpos[3 * (size_t)t + c] : 0.0;
        }
        b[3 * (size_t)i + c] = v;
    }
}

// column 3k + c of row i: S_{s,k}[c][r] for a pair row (aux = 3s + r), the identity's [r][c] for an unpaired triangle's row (aux = r), the
// neutral position of an anchor (aux = its vertex)
__global__ __launch_bounds__(THREADS) void transfer_rhs_kernel(const int* rowclass, const int* rowaux, int m, int n_shapes, const double* q, int nf_src, const double* tpos,
                                                               double* b) {
    const int R = 3 * n_shapes;
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= (long long)m * R) return;
    const int i = (int)(e / R), j = (int)(e % R), k = j / 3, c = j % 3;
    const int cls = rowclass[i], aux = rowaux[i];
    double v;
    if (cls == RHS_PAIR) {
        const int s = aux / 3, r = aux % 3;
        v = q[((size_t)k * nf_src + s) * 9 + 3 * c + r];
    } else if (cls == RHS_IDENTITY) {
        v = aux == c ? 1.0 : 0.0;
    } else {
        v = tpos[3 * (size_t)aux + c];
    }
    b[e] = v;
}

__global__ __launch_bounds__(THREADS) void residuals_kernel(const double* x, const double* neutral, int nv, int n_shapes, double* out) {
    const long long e = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (e >= (long long)n_shapes * nv * 3) return;
    const int c = (int)(e % 3), v = (int)((e / 3) % nv), k = (int)(e / (3LL * nv));
    out[e] = x[(size_t)v * (3 * n_shapes) + 3 * k + c] - neutral[3 * (size_t)v + c];
}

// ---- solver

// 1 / (squared norm of A's column j) from row j of A'; an empty column (a fixed unknown) gets 0: its x never moves
__global__ __launch_bounds__(THREADS) void column_norms_kernel(Csr at, double* minv) {
    const int j = (int)(blockIdx.x * THREADS + threadIdx.x);
    if (j >= at.nrows) return;
    double s = 0.0;
    for (int e = at.rowptr[j]; e < at.rowptr[j + 1]; ++e) s += at.val[e] * at.val[e];
    minv[j] = s > 0.0 ? 1.0 / s : 0.0;
}

template <int MODE>
__global__ __launch_bounds__(THREADS) void spmv_kernel(Csr mat, const double* v, const double* b_or_dot, double* y, double* partial, int R, int cw_log2, const int* active) {
    __shared__ double red[MODE == 2 ? ROWS_PER_BLOCK * MAX_TILE : 1];
    const Tile t = tile_of(cw_log2);
    const bool on = t.c < R && (!active || active[t.c]);
    const int row0 = (int)blockIdx.x * ROWS_PER_BLOCK;
    for (int lr = t.rl; lr < ROWS_PER_BLOCK; lr += t.rlanes) {
        const int i = row0 + lr;
        double prod = 0.0;
        if (on && i < mat.nrows) {
            double acc = 0.0;
            for (int e = mat.rowptr[i]; e < mat.rowptr[i + 1]; ++e) acc += mat.val[e] * v[(size_t)mat.col[e] * R + t.c];
            const size_t o = (size_t)i * R + t.c;
            if (MODE == 1) acc = b_or_dot[o] - acc;
            y[o] = acc;
            if (MODE == 2) prod = (b_or_dot ? b_or_dot[o] : acc) * acc;
        }
        if (MODE == 2) red[lr * t.cw + t.c_local] = prod;
    }
    if (MODE == 2) reduce_rows(red, t, R, partial);
}

__global__ __launch_bounds__(MAX_TILE) void reduce_columns_kernel(const double* partial, int nb, int R, double* out) {
    const int c = (int)(blockIdx.x * MAX_TILE + threadIdx.x);
    if (c < R) out[c] = sum_partials(partial, nb, R, c);
}

// the start of a round, from the true residual's |r|^2 in st.rr: a running column whose residual passes is finished, the others go on
// (active[0]); after the last round a column still running has not converged
__global__ __launch_bounds__(MAX_TILE) void round_kernel(SolveState st, int R, double tol2, int final_round) {
    const int c = (int)(blockIdx.x * MAX_TILE + threadIdx.x);
    if (c >= R) return;
    int go = 0;
    if (st.status[c] < 0) {
        const double rr = st.rr[c];
        if (!(rr == rr) || rr > 1.0e300) st.status[c] = 2;
        else if (rr <= tol2 * st.bnorm2[c]) st.status[c] = 0;
        else if (final_round) st.status[c] = 1;
        else go = 1;
    }
    st.active[c] = go;
    st.active[R + c] = 0;
}

// z = M^-1 r, p = z, first-stage partials of r'z
__global__ __launch_bounds__(THREADS) void precondition_kernel(int n, int R, int cw_log2, const double* r, const double* minv, double* z, double* p, double* partial_rz,
                                                               const int* active) {
    __shared__ double red[ROWS_PER_BLOCK * MAX_TILE];
    const Tile t = tile_of(cw_log2);
    const bool on = t.c < R && active[t.c];
    const int row0 = (int)blockIdx.x * ROWS_PER_BLOCK;
    for (int lr = t.rl; lr < ROWS_PER_BLOCK; lr += t.rlanes) {
        const int i = row0 + lr;
        double prod = 0.0;
        if (on && i < n) {
            const size_t o = (size_t)i * R + t.c;
            const double rv = r[o], zv = minv[i] * rv;
            z[o] = zv;
            p[o] = zv;
            prod = rv * zv;
        }
        red[lr * t.cw + t.c_local] = prod;
    }
    reduce_rows(red, t, R, partial_rz);
}

// alpha = r'z / p'A'Ap; x += alpha p; r -= alpha s; z = M^-1 r; first-stage partials of r'z and r'r
__global__ __launch_bounds__(THREADS) void update_kernel(int n, int R, int cw_log2, int nb, double* x, double* r, const double* p, const double* sv, double* z, const double* minv,
                                                         const double* partial_ps, const double* rz_cur, const int* active_cur, double* partial_rz, double* partial_rr) {
    __shared__ double red[ROWS_PER_BLOCK * MAX_TILE];
    __shared__ double alpha_s[MAX_TILE];
    const Tile t = tile_of(cw_log2);
    const bool on = t.c < R && active_cur[t.c];
    if (t.rl == 0) alpha_s[t.c_local] = on ? rz_cur[t.c] / sum_partials(partial_ps, nb, R, t.c) : 0.0;
    __syncthreads();
    const double alpha = alpha_s[t.c_local];
    const int row0 = (int)blockIdx.x * ROWS_PER_BLOCK;
    for (int lr = t.rl; lr < ROWS_PER_BLOCK; lr += t.rlanes) {
        const int i = row0 + lr;
        double prod = 0.0;
        if (on && i < n) {
            const size_t o = (size_t)i * R + t.c;
            x[o] = x[o] + alpha * p[o];
            const double rv = r[o] - alpha * sv[o], zv = minv[i] * rv;
            r[o] = rv;
            z[o] = zv;
            prod = rv * zv;
        }
        red[lr * t.cw + t.c_local] = prod;
    }
    reduce_rows(red, t, R, partial_rz);
    for (int lr = t.rl; lr < ROWS_PER_BLOCK; lr += t.rlanes) {
        const int i = row0 + lr;
        double prod = 0.0;
        if (on && i < n) {
            const double rv = r[(size_t)i * R + t.c];   // this thread's own store above
            prod = rv * rv;
        }
        red[lr * t.cw + t.c_local] = prod;
    }
    reduce_rows(red, t, R, partial_rr);
}

// beta = r'z (new) / r'z (old); p = z + beta p; workgroup row 0 writes the next iteration's state: a column whose recurrence residual passes,
// or that reached max_iter or left the finite numbers, is not active in the next iteration
__global__ __launch_bounds__(THREADS) void direction_kernel(int n, int R, int cw_log2, int nb, double* p, const double* z, const double* partial_rz, const double* partial_rr,
                                                            SolveState st, int cur, double tol2, int max_iter) {
    __shared__ double beta_s[MAX_TILE];
    __shared__ int go_s[MAX_TILE];
    const Tile t = tile_of(cw_log2);
    if (t.rl == 0) {
        int go = 0;
        double beta = 0.0;
        if (t.c < R) {
            const int nxt = cur ^ 1;
            if (st.active[cur * R + t.c]) {
                const double rzn = sum_partials(partial_rz, nb, R, t.c), rr = sum_partials(partial_rr, nb, R, t.c);
                beta = rzn / st.rz[cur * R + t.c];
                const bool bad = !(rr == rr) || !(rzn == rzn) || rr > 1.0e300;
                const bool conv = !bad && rr <= tol2 * st.bnorm2[t.c];
                go = !(bad || conv);
                if (blockIdx.x == 0) {
                    const int it = st.iters[t.c] + 1;
                    st.iters[t.c] = it;
                    st.rz[nxt * R + t.c] = rzn;
                    if (bad) st.status[t.c] = 2;
                    else if (!conv && it >= max_iter) st.status[t.c] = 1;
                    st.active[nxt * R + t.c] = go && it < max_iter;
                }
            } else if (blockIdx.x == 0) {
                st.active[nxt * R + t.c] = 0;
            }
        }
        beta_s[t.c_local] = beta;
        go_s[t.c_local] = go;
    }
    __syncthreads();
    if (!go_s[t.c_local]) return;
    const double beta = beta_s[t.c_local];
    const int row0 = (int)blockIdx.x * ROWS_PER_BLOCK;
    for (int lr = t.rl; lr < ROWS_PER_BLOCK; lr += t.rlanes) {
        const int i = row0 + lr;
        if (i < n) {
            const size_t o = (size_t)i * R + t.c;
            p[o] = z[o] + beta * p[o];
        }
    }
}

inline unsigned blocks_for(long long n) { return (unsigned)((n + THREADS - 1) / THREADS); }

}  // namespace

void launch_frames(const double* verts, const int* faces, int nf, double* w, double* gc, hipStream_t s) {
    hipLaunchKernelGGL(frames_kernel, dim3(blocks_for(nf)), dim3(THREADS), 0, s, verts, faces, nf, w, gc);
}

void launch_gradients(const double* w_ref, const double* deformed, int n_shapes, int nv, const int* faces, int nf, double* q, hipStream_t s) {
    hipLaunchKernelGGL(gradients_kernel, dim3(blocks_for(nf), (unsigned)n_shapes), dim3(THREADS), 0, s, w_ref, deformed, nv, faces, nf, q);
}

void launch_face_normals(const double* verts, const int* faces, int nf, double* fn, double* centroid, hipStream_t s) {
    hipLaunchKernelGGL(face_normals_kernel, dim3(blocks_for(nf)), dim3(THREADS), 0, s, verts, faces, nf, fn, centroid);
}

void launch_vertex_normals(const double* fn, const int* vf_ptr, const int* vf_idx, int nv, double* vn, hipStream_t s) {
    hipLaunchKernelGGL(vertex_normals_kernel, dim3(blocks_for(nv)), dim3(THREADS), 0, s, fn, vf_ptr, vf_idx, nv, vn);
}

void launch_closest(const double* qpos, const double* qnrm, int nq, const double* tpos, const double* tnrm, int nt, int* idx, double* d2, hipStream_t s) {
    hipLaunchKernelGGL(closest_kernel, dim3(blocks_for(nq)), dim3(THREADS), 0, s, qpos, qnrm, nq, tpos, tnrm, nt, idx, d2);
}

void launch_fill_values(const int* rowptr, const int* col, const int* c0, const int* c1, const int* rowclass, const int* rowaux, int m, const double* gc,
                        const double* weights, const int* closest, const unsigned char* colfixed, double* val, hipStream_t s) {
    hipLaunchKernelGGL(fill_values_kernel, dim3(blocks_for(m)), dim3(THREADS), 0, s, rowptr, col, c0, c1, rowclass, rowaux, m, gc, weights, closest, colfixed, val);
}

void launch_gather(const int* src, const double* in, long long n, double* out, hipStream_t s) {
    hipLaunchKernelGGL(gather_kernel, dim3(blocks_for(n)), dim3(THREADS), 0, s, src, in, n, out);
}

void launch_register_rhs(const int* rowclass, const int* rowaux, int m, const double* weights, const int* closest, const double* tpos, double* b, hipStream_t s) {
    hipLaunchKernelGGL(register_rhs_kernel, dim3(blocks_for(m)), dim3(THREADS), 0, s, rowclass, rowaux, m, weights, closest, tpos, b);
}

void launch_transfer_rhs(const int* rowclass, const int* rowaux, int m, int n_shapes, const double* q, int nf_src, const double* tpos, double* b, hipStream_t s) {
    hipLaunchKernelGGL(transfer_rhs_kernel, dim3(blocks_for((long long)m * 3 * n_shapes)), dim3(THREADS), 0, s, rowclass, rowaux, m, n_shapes, q, nf_src, tpos, b);
}

void launch_residuals(const double* x, const double* neutral, int nv, int n_shapes, double* out, hipStream_t s) {
    hipLaunchKernelGGL(residuals_kernel, dim3(blocks_for((long long)n_shapes * nv * 3)), dim3(THREADS), 0, s, x, neutral, nv, n_shapes, out);
}

void launch_column_norms(Csr at, double* minv, hipStream_t s) {
    hipLaunchKernelGGL(column_norms_kernel, dim3(blocks_for(at.nrows)), dim3(THREADS), 0, s, at, minv);
}

void launch_spmv(int mode, Csr mat, const double* v, const double* b_or_dot, double* y, double* partial, int R, const int* active, hipStream_t s) {
    const dim3 grid = grid_of(mat.nrows, R);
    const int l = cw_log2_of(R);
    if (mode == 0) hipLaunchKernelGGL(spmv_kernel<0>, grid, dim3(THREADS), 0, s, mat, v, b_or_dot, y, partial, R, l, active);
    else if (mode == 1) hipLaunchKernelGGL(spmv_kernel<1>, grid, dim3(THREADS), 0, s, mat, v, b_or_dot, y, partial, R, l, active);
    else hipLaunchKernelGGL(spmv_kernel<2>, grid, dim3(THREADS), 0, s, mat, v, b_or_dot, y, partial, R, l, active);
}

void launch_reduce_columns(const double* partial, int nb, int R, double* out, hipStream_t s) {
    hipLaunchKernelGGL(reduce_columns_kernel, dim3((unsigned)((R + MAX_TILE - 1) / MAX_TILE)), dim3(MAX_TILE), 0, s, partial, nb, R, out);
}

void launch_round(SolveState st, int R, double tol2, int final_round, hipStream_t s) {
    hipLaunchKernelGGL(round_kernel, dim3((unsigned)((R + MAX_TILE - 1) / MAX_TILE)), dim3(MAX_TILE), 0, s, st, R, tol2, final_round);
}

void launch_precondition(int n, int R, const double* r, const double* minv, double* z, double* p, double* partial_rz, const int* active, hipStream_t s) {
    hipLaunchKernelGGL(precondition_kernel, grid_of(n, R), dim3(THREADS), 0, s, n, R, cw_log2_of(R), r, minv, z, p, partial_rz, active);
}

void launch_update(int n, int R, double* x, double* r, const double* p, const double* sv, double* z, const double* minv, const double* partial_ps, const double* rz_cur,
                   const int* active_cur, double* partial_rz, double* partial_rr, hipStream_t s) {
    hipLaunchKernelGGL(update_kernel, grid_of(n, R), dim3(THREADS), 0, s, n, R, cw_log2_of(R), n_blocks(n), x, r, p, sv, z, minv, partial_ps, rz_cur, active_cur, partial_rz,
                       partial_rr);
}

void launch_direction(int n, int R, double* p, const double* z, const double* partial_rz, const double* partial_rr, SolveState st, int cur, double tol2, int max_iter,
                      hipStream_t s) {
    hipLaunchKernelGGL(direction_kernel, grid_of(n, R), dim3(THREADS), 0, s, n, R, cw_log2_of(R), n_blocks(n), p, z, partial_rz, partial_rr, st, cur, tol2, max_iter);
}

}  // namespace dt
}  // namespace said
