/*
 * said_metrics.h — C ABI of the evaluation metrics' device passes (said_amd/csrc/metrics.hip), in libsaid_hip.so beside said_hip.h.
 *
 * The reference evaluates generated animation in script/test_evaluate.py with said/metric/{frechet_distance,multimodality,wind}.py: the mean and
 * covariance of VAE latents (np.mean / np.cov), and GaussianMixture(n_components=K).fit (scikit-learn, covariance_type="full", initialised from
 * KMeans(n_clusters=K, n_init=1) with k-means++ seeding).  Every pass whose cost grows with the number of latents N runs here, in float64; the
 * K x 64 x 64 algebra and the convergence tests stay with the caller (said_amd/metric/_gmm.py).  Paths are relative to the reference repository;
 * scikit-learn's functions are named by module.
 *
 * Conventions are those of said_hip.h: 0 on success, said_metrics_last_error(ctx) (NULL for create failures) gives the message; `*_dev` are device
 * pointers, `*_host` host memory; `stream` is a hipStream_t.  Latents are fp32 (n, 64) row-major device buffers.  Entry points that return host values
 * synchronise `stream`.  Every sum runs in a fixed order: equal inputs give bit-identical outputs.
 */
#ifndef SAID_METRICS_H
#define SAID_METRICS_H

#ifdef __cplusplus
extern "C" {
#endif

enum { SAID_METRICS_DIM = 64, SAID_METRICS_MAX_K = 8 };
/* weights of the moment passes: unit (k = 1), one-hot of the last k-means labels, exp(log_resp) of the last E-step */
enum { SAID_METRICS_W_UNIT = 0, SAID_METRICS_W_LABELS = 1, SAID_METRICS_W_RESP = 2 };

typedef struct said_metrics said_metrics;
/* Workspace for up to `max_points` latents (about 200 bytes each) on `device`. */
int said_metrics_create(said_metrics** out, int device, long long max_points);
int said_metrics_destroy(said_metrics* m);
const char* said_metrics_last_error(const said_metrics* m);
long long said_metrics_max_points(const said_metrics* m);

/* Pass 1 of the weighted moments: nk_host (k) = sum r, sum_host (k, 64) = sum r x.  np.mean (frechet_distance.py:30), the first half of
 * sklearn.mixture._gaussian_mixture._estimate_gaussian_parameters, and the centre update of sklearn.cluster._k_means_lloyd.lloyd_iter_chunked_dense. */
int said_metrics_weighted_sums(said_metrics* m, const float* x_dev, long long n, int k, int wsrc, double* nk_host, double* sum_host, void* stream);
/* Pass 2: scatter_host (k, 64, 64) = sum r (x - mu_k)(x - mu_k)^T for the caller's means_host (k, 64).  np.cov (frechet_distance.py:31) before its
 * 1 / (n - 1), and sklearn.mixture._gaussian_mixture._estimate_gaussian_covariances_full before its 1 / n_k and reg_covar. */
int said_metrics_weighted_scatter(said_metrics* m, const float* x_dev, long long n, int k, int wsrc, const double* means_host, double* scatter_host,
                                  void* stream);

/* sklearn.mixture.GaussianMixture._e_step (covariance_type="full"): y = x U_k - mu_k U_k, log N = -0.5 (64 log 2 pi + |y|^2) + log_det_k, + log_w_k,
 * logsumexp over k.  prec_chol_host (k, 64, 64) upper-triangular precision Cholesky factors, mean_prec_host (k, 64) = mu_k U_k, log_det_host (k),
 * log_weights_host (k).  *lower_bound_host = mean log_prob_norm.  The responsibilities stay in the context for SAID_METRICS_W_RESP; log_resp_dev
 * (n, k) and log_prob_norm_dev (n) float64, nullable, receive copies. */
int said_metrics_gmm_estep(said_metrics* m, const float* x_dev, long long n, int k, const double* prec_chol_host, const double* mean_prec_host,
                           const double* log_det_host, const double* log_weights_host, double* lower_bound_host, double* log_resp_dev,
                           double* log_prob_norm_dev, void* stream);

/* The assignment step of sklearn.cluster._kmeans._kmeans_single_lloyd: each point's nearest of centres_host (k, 64) by |c|^2 - 2 x.c, ties to the lower
 * index; the labels stay in the context for SAID_METRICS_W_LABELS.  compare != 0: *n_changed_host counts labels that differ from the previous call's
 * (np.array_equal(labels, labels_old)).  *inertia_host (nullable) = sum of the exact squared distances to the chosen centres. */
int said_metrics_kmeans_assign(said_metrics* m, const float* x_dev, long long n, int k, const double* centres_host, int compare,
                               long long* n_changed_host, double* inertia_host, void* stream);
/* The last assignment's labels (n int32) and squared distances (n float64) to the host, both nullable (empty-cluster relocation,
 * sklearn.cluster._k_means_common._relocate_empty_clusters_dense, and tests). */
int said_metrics_kmeans_read(said_metrics* m, long long n, int* labels_host, double* dist_host, void* stream);

/* Labels (n int32 in [0, k)) given by the caller in place of an assignment: GaussianMixture(init_params="kmeans") from labels computed elsewhere. */
int said_metrics_kmeans_set_labels(said_metrics* m, long long n, int k, const int* labels_host, void* stream);
/* sklearn.cluster._kmeans._kmeans_plusplus: the first centre (x[centre_id]); *pot_host = sum of squared distances to it. */
int said_metrics_kmeanspp_first(said_metrics* m, const float* x_dev, long long n, long long centre_id, double* pot_host, void* stream);
/* One further centre: the candidates are searchsorted(cumsum(closest_dist_sq), rand_host[t]) for `trials` (<= 4) values the caller drew as
 * uniform * current potential; the one of least potential (first on ties) becomes *centre_id_host, its potential *pot_host. */
int said_metrics_kmeanspp_step(said_metrics* m, const float* x_dev, long long n, const double* rand_host, int trials, long long* centre_id_host,
                               double* pot_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAID_METRICS_H */
