/*
 * said_transfer.h — C ABI of deformation transfer (said_amd/csrc/deform_transfer.hip, deform_transfer_ctx.cpp), in libsaid_hip.so beside
 * said_optimize.h.
 *
 * DESIGN.md section 17 is the specification: blendshapes of a source head are carried onto a target head of another topology after Sumner &
 * Popovic (2004) in three stages (registration of the source neutral onto the target neutral, triangle correspondence, transfer), which
 * share one solver: conjugate gradients on the normal equations A'A x = A'b with a Jacobi preconditioner (the squared column norms of A),
 * A and A' both in CSR, the product never formed, and R right-hand-side columns solved side by side with step lengths and convergence of
 * their own.
 *
 * A system's index structure is built by the caller (said_amd/optimize/deformation_transfer.py); its values are filled on the device from
 * the frame inverses of the mesh the unknowns belong to.  The unknowns of a mesh are its V vertices followed by one fourth vertex per
 * triangle, n = V + F rows.
 *
 * Conventions are those of said_optimize.h: 0 on success, said_transfer_last_error(ctx) (NULL for create failures) gives the message;
 * `*_host` are host memory; `stream` is a hipStream_t.  All values are float64, all indices int32.  Every call but create / destroy /
 * last_error synchronises `stream` before it returns.  Every sum runs in a fixed order and nothing uses atomics: equal inputs give
 * bit-identical outputs, and a right-hand-side column's result does not depend on the columns solved with it.  Every index array is checked
 * on the host before a kernel indexes with it.
 */
#ifndef SAID_TRANSFER_H
#define SAID_TRANSFER_H

#ifdef __cplusplus
extern "C" {
#endif

/* per-column status of a solve.  MAX_ITER also stands for a column whose true residual did not pass within SAID_TRANSFER_MAX_ROUNDS restarts. */
enum { SAID_TRANSFER_CONVERGED = 0, SAID_TRANSFER_MAX_ITER = 1, SAID_TRANSFER_NOT_FINITE = 2 };
enum { SAID_TRANSFER_MAX_ROUNDS = 8, SAID_TRANSFER_MAX_COLUMNS = 3 * 256 };
/* said_transfer_system::rowclass: which weight a row carries (smoothness, identity, closest point, 1) */
enum { SAID_TRANSFER_ROW_SMOOTH = 0, SAID_TRANSFER_ROW_IDENTITY = 1, SAID_TRANSFER_ROW_CLOSEST = 2, SAID_TRANSFER_ROW_UNIT = 3 };
/* said_transfer_system::rhsclass of the transfer system */
enum { SAID_TRANSFER_RHS_PAIR = 0, SAID_TRANSFER_RHS_IDENTITY = 1, SAID_TRANSFER_RHS_ANCHOR = 2 };

/* The index structure of a system A (m, n) with nnz entries, all arrays on the host.
 * rowptr (m + 1), col (nnz): CSR of A, no column twice in a row.  Entry j has the value weight(row) * (term(c0[j]) - term(c1[j])): a term is
 * coefficient c of the mesh's G table (F, 3, 4: triangle, row of G_t, vertex slot 1..4) when c >= 0, nothing for -1, and 1 for c0 = -2.
 * rowclass (m): SAID_TRANSFER_ROW_*.  rowaux (m): the source vertex of a closest-point row; for the transfer's right-hand side 3 s + r of a
 * pair row, r of an identity row, the target vertex of an anchor row.  rhsclass (m): SAID_TRANSFER_RHS_*, transfer only (else NULL).
 * at_rowptr (n + 1), at_col (nnz), at_src (nnz): CSR of A', entry j taking its value from entry at_src[j] of A. */
typedef struct said_transfer_system {
    int m, n, nnz;
    const int *rowptr, *col, *c0, *c1, *rowclass, *rowaux, *rhsclass, *at_rowptr, *at_col, *at_src;
} said_transfer_system;

typedef struct said_transfer said_transfer;
int said_transfer_create(said_transfer** out, int device);
int said_transfer_destroy(said_transfer* t);
const char* said_transfer_last_error(const said_transfer* t);

/* The source: neutral (nv, 3), faces (nf, 3), shapes (k, nv, 3) absolute positions (k may be 0, shapes NULL).  The target: neutral and faces.
 * Both compute the mesh's frame inverses and normals.  Fails on a face index outside the vertices or a degenerate triangle count of 0. */
int said_transfer_set_source(said_transfer* t, int nv, int nf, int k, const double* neutral_host, const int* faces_host, const double* shapes_host, void* stream);
int said_transfer_set_target(said_transfer* t, int nv, int nf, const double* neutral_host, const int* faces_host, void* stream);

/* The solver alone: min |A x - b| for R columns.  A (m, n) and A' in CSR with values, b (m, R) and x0 (n, R; NULL: zeros) row-major.
 * A column stops when |A'(b - A x)| <= tol |A'b|, judged on the recurrence residual and confirmed on the recomputed one (a column that
 * fails the confirmation restarts from it).  The host looks at the columns' flags once per check_every iterations.  x_host (n, R);
 * status_host, iters_host, resid_host (R: the final recomputed |A'(b - A x)| / |A'b|), each nullable. */
int said_transfer_solve(said_transfer* t, int m, int n, int nnz, int R, const int* a_rowptr_host, const int* a_col_host, const double* a_val_host,
                        const int* at_rowptr_host, const int* at_col_host, const double* at_val_host, const double* b_host, const double* x0_host, double tol,
                        int max_iter, int check_every, double* x_host, int* status_host, int* iters_host, double* resid_host, void* stream);

/* Stage 1.  sys: the registration system over the source's V_s + F_s unknowns (smoothness, identity and closest-point rows).  The source
 * vertices marker_src_host[i] are fixed at marker_pos_host[i] (n_markers, 3).  Solve j uses the closest-point weight wc_host[j]; when it is
 * positive, the closest compatible target vertices come from solve j - 1 (so wc_host[0] must be 0).  x_host (n_solves, V_s + F_s, 3);
 * closest_host (n_solves, V_s): the target vertex used per source vertex, -1 for none; status / iters / resid (n_solves, 3).  The last
 * solution's vertices stay on the device as the registered source. */
int said_transfer_register(said_transfer* t, const said_transfer_system* sys, int n_markers, const int* marker_src_host, const double* marker_pos_host, double w_s,
                           double w_i, int n_solves, const double* wc_host, double tol, int max_iter, double* x_host, int* closest_host, int* status_host,
                           int* iters_host, double* resid_host, void* stream);

/* Stage 2.  reg_host (V_s, 3): the registered source vertices (NULL: those of the last said_transfer_register).  t2s_host (F_t): per target
 * triangle the registered-source triangle with the nearest centroid among those whose normal has a positive dot product with its own, -1
 * for none or when the centroids lie further apart than threshold x the target's bounding-box diagonal; s2t_host (F_s) likewise.  The
 * nullable t2s_d2_host / s2t_d2_host receive the squared centroid distances of the searches. */
int said_transfer_correspond(said_transfer* t, const double* reg_host, double threshold, int* t2s_host, int* s2t_host, double* t2s_d2_host, double* s2t_d2_host,
                             void* stream);

/* Stage 3.  sys: the transfer system over the target's V_t + F_t unknowns; the right-hand side's 3 k columns are formed on the device from the
 * source's deformation gradients.  residuals_host (k, V_t, 3) = x - neutral; status / iters / resid (3 k). */
int said_transfer_transfer(said_transfer* t, const said_transfer_system* sys, double tol, int max_iter, double* residuals_host, int* status_host, int* iters_host,
                           double* resid_host, void* stream);

/* The mesh passes alone, for tests.  mesh: w_host (nf, 3, 3) = V^-T, gc_host (nf, 3, 4) the G table, fn_host (nf, 3) un-normalised face
 * normals, centroid_host (nf, 3), vn_host (nv, 3) vertex normals; each nullable.  gradients: q_host (k, nf, 3, 3) = V~ V^-1 of deformed
 * (k, nv, 3) against ref.  closest: per query the nearest target with a positive normal dot product (qnrm_host and tnrm_host NULL: the
 * nearest), ties to the lower index, -1 for none. */
int said_transfer_mesh(said_transfer* t, int nv, int nf, const double* verts_host, const int* faces_host, double* w_host, double* gc_host, double* fn_host,
                       double* centroid_host, double* vn_host, void* stream);
int said_transfer_gradients(said_transfer* t, int nv, int nf, const double* ref_host, const int* faces_host, int k, const double* deformed_host, double* q_host,
                            void* stream);
int said_transfer_closest(said_transfer* t, int nq, const double* qpos_host, const double* qnrm_host, int nt, const double* tpos_host, const double* tnrm_host,
                          int* idx_host, double* d2_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAID_TRANSFER_H */
