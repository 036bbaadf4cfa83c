/*
 * said_optimize.h — C ABI of the pseudo-GT blendshape-coefficient fit (said_amd/csrc/blendshape_qp.hip), in libsaid_hip.so beside said_hip.h.
 *
 * The reference (said/optimize/blendshape_coeffs.py, driven by script/optimize_blendshape_coeffs.py) fits K blendshape coefficients per frame
 * to a mesh sequence by the quadratic program
 *
 *     minimise  sum_t 1/2 w_t' P w_t + q_t' w_t   subject to  0 <= w_t <= 1,  -delta <= w_t - w_{t+1} <= delta   (elementwise)
 *
 * with B_delta = B - n, P = B_delta' B_delta and q_t = B_delta' (n - v_t).  Here the right-hand sides q_t are computed on the device from the
 * frames' vertices, and every sequence of a batch is solved by a primal-dual interior-point method (Mehrotra predictor-corrector) that runs
 * entirely on the device, one workgroup per sequence.  Uncoupled solves drop the difference constraints (OptimizationProblemSingle).
 *
 * Conventions are those of said_metrics.h: 0 on success, said_optimize_last_error(ctx) (NULL for create failures) gives the message; `*_dev` are
 * device pointers, `*_host` host memory; `stream` is a hipStream_t.  All values are float64.  said_optimize_set_bases and said_optimize_solve
 * synchronise `stream`; said_optimize_rhs does not.  Every sum runs in a fixed order and each sequence is solved by a workgroup of its own, so a
 * sequence's result does not depend on the batch it is solved in, and equal inputs give bit-identical outputs.
 */
#ifndef SAID_OPTIMIZE_H
#define SAID_OPTIMIZE_H

#ifdef __cplusplus
extern "C" {
#endif

enum { SAID_OPTIMIZE_MAX_K = 64 };
/* per-sequence status of said_optimize_solve */
enum { SAID_OPTIMIZE_CONVERGED = 0, SAID_OPTIMIZE_MAX_ITER = 1, SAID_OPTIMIZE_NOT_FINITE = 2 };

typedef struct said_optimize said_optimize;
int said_optimize_create(said_optimize** out, int device);
int said_optimize_destroy(said_optimize* o);
const char* said_optimize_last_error(const said_optimize* o);

/* nbasis bases of k (<= 64) blendshapes over n3v = 3V vertex coordinates (one per person of a multi-person batch), replacing earlier ones.
 * neutral_host (nbasis, n3v); bdelta_host (nbasis, n3v, k) row-major, B - n as the caller formed it; p_host (nbasis, k, k) = B_delta' B_delta.
 * Synchronises. */
int said_optimize_set_bases(said_optimize* o, int nbasis, int k, long long n3v, const double* neutral_host, const double* bdelta_host,
                            const double* p_host, void* stream);

/* q_dev (nframes, k) = B_delta' (n - v) for the frames verts_dev (nframes, n3v) of basis `basis`: the difference first, then each 3V-long dot
 * product in one fixed order. */
int said_optimize_rhs(said_optimize* o, int basis, const double* verts_dev, long long nframes, double* q_dev, void* stream);

/* Solve nseq sequences in one launch.  Sequence s owns frames [offsets_host[s], offsets_host[s + 1]) of q_dev (frames, k) and basis
 * basis_host[s]; coupled != 0 adds the difference constraints with bound delta (> 0).  Convergence: the primal residual, the dual residual and
 * the duality gap, each relative to the data, at most tol, within max_iter iterations.
 * w_dev (frames, k): the primal solution, unclipped.  z_dev (frames, 4, k), nullable: the duals of -w <= 0, w <= 1, w_t - w_{t+1} <= delta and
 * w_{t+1} - w_t <= delta (the last two zero at each sequence's last frame and when uncoupled).  status_host, iters_host (nseq) and
 * resid_host (nseq, 3: primal, dual, gap), each nullable.  Synchronises. */
int said_optimize_solve(said_optimize* o, int nseq, const long long* offsets_host, const int* basis_host, const double* q_dev, double delta,
                        int coupled, int max_iter, double tol, double* w_dev, double* z_dev, int* status_host, int* iters_host, double* resid_host,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAID_OPTIMIZE_H */
