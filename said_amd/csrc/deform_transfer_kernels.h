// deform_transfer_kernels.h — launchers of deform_transfer.hip for deform_transfer_ctx.cpp.
#pragma once
#include <hip/hip_runtime.h>

namespace said {
namespace dt __attribute__((visibility("hidden"))) {

constexpr int ROWS_PER_BLOCK = 64;   // rows of a vector one workgroup owns: the unit of the first reduction stage, whatever R is
constexpr int MAX_TILE = 64;         // right-hand-side columns of one workgroup (lanes across R)

// row classes of a system (said_transfer_system::rowclass)
enum { ROW_SMOOTH = 0, ROW_IDENTITY = 1, ROW_CLOSEST = 2, ROW_UNIT = 3 };
// row classes of the transfer system's right-hand side
enum { RHS_PAIR = 0, RHS_IDENTITY = 1, RHS_ANCHOR = 2 };

struct Csr {          // device arrays
    const int* rowptr;
    const int* col;
    const double* val;
    int nrows;
};

struct SolveState {   // device arrays, R entries each unless noted
    double* rz;        // (2, R): r'z of the current and the next iteration
    int* active;       // (2, R)
    double* bnorm2;    // |A'b|^2
    double* rr;        // |r|^2 of the last look
    int* iters;
    int* status;       // -1 while running
};

inline int n_blocks(int rows) { return (rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK; }

// mesh passes
void launch_frames(const double* verts, const int* faces, int nf, double* w, double* gc, hipStream_t s);
void launch_gradients(const double* w_ref, const double* deformed, int n_shapes, int nv, const int* faces, int nf, double* q, hipStream_t s);
void launch_face_normals(const double* verts, const int* faces, int nf, double* fn, double* centroid, hipStream_t s);
void launch_vertex_normals(const double* fn, const int* vf_ptr, const int* vf_idx, int nv, double* vn, hipStream_t s);
void launch_closest(const double* qpos, const double* qnrm, int nq, const double* tpos, const double* tnrm, int nt, int* idx, double* d2, hipStream_t s);

// system values and right-hand sides
void launch_fill_values(const int* rowptr, const int* col, const int* c0, const int* c1, const int* rowclass, const int* rowaux, int m, const double* gc,
                        const double* weights, const int* closest, const unsigned char* colfixed, double* val, hipStream_t s);
void launch_gather(const int* src, const double* in, long long n, double* out, hipStream_t s);
void launch_register_rhs(const int* rowclass, const int* rowaux, int m, const double* weights, const int* closest, const double* tpos, double* b, hipStream_t s);
void launch_transfer_rhs(const int* rowclass, const int* rowaux, int m, int n_shapes, const double* q, int nf_src, const double* tpos, double* b, hipStream_t s);
void launch_residuals(const double* x, const double* neutral, int nv, int n_shapes, double* out, hipStream_t s);

// solver
void launch_column_norms(Csr at, double* minv, hipStream_t s);
// y = M v (mode 0), y = b - M v (mode 1), y = M v with the first-stage partials of dot . y (dot null: y . y) per 64 rows (mode 2)
void launch_spmv(int mode, Csr mat, const double* v, const double* b_or_dot, double* y, double* partial, int R, const int* active, hipStream_t s);
void launch_reduce_columns(const double* partial, int nb, int R, double* out, hipStream_t s);
void launch_round(SolveState st, int R, double tol2, int final_round, hipStream_t s);
void launch_precondition(int n, int R, const double* r, const double* minv, double* z, double* p, double* partial_rz, const int* active, hipStream_t s);
void launch_update(int n, int R, double* x, double* r, const double* p, const double* sv, double* z, const double* minv, const double* partial_ps, const double* rz_cur,
                   const int* active_cur, double* partial_rz, double* partial_rr, hipStream_t s);
void launch_direction(int n, int R, double* p, const double* z, const double* partial_rz, const double* partial_rr, SolveState st, int cur, double tol2, int max_iter,
                      hipStream_t s);

}  // namespace dt
}  // namespace said
