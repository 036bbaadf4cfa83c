/*
 * said_train.h — C ABI of the BCVAE trainer (said_amd/csrc/vae_train.hip, vae_trainer.cpp), in libsaid_hip.so beside said_hip.h.
 *
 * One context trains BCVAE(channels=32, seq_len=120, z_dim=64) (said/model/vae.py) with the step of script/train_vae.py: training-mode forward
 * (BatchNorm on batch statistics), elbo_loss with the reweighting done out of place, backward, clip_grad_norm_(1.0), torch.optim.AdamW and the
 * EMA shadow of diffusers' EMAModel.  fp32 throughout; every sum runs in a fixed order, so equal inputs give bit-identical results.  Paths are
 * relative to the reference repository.
 *
 * Conventions are those of said_hip.h: 0 on success, said_train_last_error(ctx) (NULL for create failures) gives the message; `*_host` is host
 * memory.  The context owns its stream: entry points that return host values synchronise it, the others only enqueue.  Tensors are named by
 * their keys in the reference's BCVAE().state_dict(); the `*.num_batches_tracked` counters are int64, every other tensor fp32.
 */
#ifndef SAID_TRAIN_H
#define SAID_TRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

enum { SAID_TRAIN_NUM_TENSORS = 70, SAID_TRAIN_CHANNELS = 32, SAID_TRAIN_WINDOW = 120, SAID_TRAIN_ZDIM = 64, SAID_TRAIN_ITEM = 4 };
/* the per-step scalars (float32, SAID_TRAIN_NSCAL of them; unused slots 0).  The host computes them as torch does, in double:
 * LR = lr_k, WD_FACTOR = 1 - lr_k wd, STEP_SIZE = lr_k / (1 - beta1^k), BC2_SQRT = sqrt(1 - beta2^k), EMA_OMD = 1 - EMA decay,
 * BETA = KL weight, WVEL = velocity weight, OMB1 = 1 - beta1, B2 = beta2, OMB2 = 1 - beta2, EPS = Adam eps, USE_EMA = 0 / 1. */
enum {
    SAID_TRAIN_S_LR = 0, SAID_TRAIN_S_WD_FACTOR, SAID_TRAIN_S_STEP_SIZE, SAID_TRAIN_S_BC2_SQRT, SAID_TRAIN_S_EMA_OMD, SAID_TRAIN_S_BETA,
    SAID_TRAIN_S_WVEL, SAID_TRAIN_S_OMB1, SAID_TRAIN_S_B2, SAID_TRAIN_S_OMB2, SAID_TRAIN_S_EPS, SAID_TRAIN_S_USE_EMA, SAID_TRAIN_NSCAL = 16
};
/* the copies of a tensor: the model state (parameters and buffers), and for parameters only the EMA shadow, the last step's gradient (before the
 * clip) and Adam's two moments */
enum { SAID_TRAIN_STATE = 0, SAID_TRAIN_EMA = 1, SAID_TRAIN_GRAD = 2, SAID_TRAIN_EXP_AVG = 3, SAID_TRAIN_EXP_AVG_SQ = 4 };
/* loss accumulators: sums of loss * batch size over the steps since the last reset, the sample count, and the number of steps whose total loss
 * was not finite */
enum { SAID_TRAIN_ACC_RECONST = 0, SAID_TRAIN_ACC_REGULARIZE, SAID_TRAIN_ACC_VELOCITY, SAID_TRAIN_ACC_TOTAL, SAID_TRAIN_ACC_COUNT,
       SAID_TRAIN_ACC_NOT_FINITE, SAID_TRAIN_NACC = 8 };
enum { SAID_TRAIN_OK = 0, SAID_TRAIN_NOT_FINITE = 1 };
enum { SAID_TRAIN_SET_TRAIN = 0, SAID_TRAIN_SET_VAL = 1 };

typedef struct said_train said_train;
/* Workspace for batches of up to `max_batch` windows on `device`.  All state starts at zero (running_var at one): set every tensor. */
int said_train_create(said_train** out, int device, int max_batch);
int said_train_destroy(said_train* t);
const char* said_train_last_error(const said_train* t);
/* the i-th state-dict key (reference order), its element count and whether it is an int64 counter; NULL / -1 outside [0, 70) */
const char* said_train_tensor_name(int i);
long long said_train_tensor_numel(int i);
int said_train_tensor_is_counter(int i);

/* copy `n` elements (the tensor's numel) of copy `which` of tensor `name` from / to the host (int64 for the counters, float32 otherwise) */
int said_train_set_tensor(said_train* t, int which, const char* name, const void* host, long long n);
int said_train_get_tensor(said_train* t, int which, const char* name, void* host, long long n);
/* zero the gradients and both moments and copy the parameters into the EMA shadow (EMAModel(params) at the start of training) */
int said_train_reset_optimizer(said_train* t);

/* A window set on the device: `nseq` sequences of len_host[s] frames x 32 coefficients, concatenated in frames_host (nframes x 32) at frame
 * offsets off_host[s]; mirror_host (32) is the channel permutation of the horizontal flip. */
int said_train_set_data(said_train* t, int set, const float* frames_host, long long nframes, const long long* off_host, const int* len_host, int nseq,
                        const int* mirror_host);
/* items_host (B x 4): (sequence, bdx, flip, zero) per window, as BlendVOCAVAEDataset.__getitem__ draws them; x_host (B, 120, 32) */
int said_train_gather(said_train* t, int set, int B, const int* items_host, float* x_host);

/* One optimizer step on the B windows of the training set named by items_host: forward, loss, backward, clip, AdamW, EMA.  eps_host (B, 64) is
 * the reparametrisation noise, scalars_host the SAID_TRAIN_S_* values, std_host (32, nullable) the coefficient std of the reweighting.  B >= 2
 * (BatchNorm1d needs more than one value per channel in training mode).  use_graph: replay the step's hipGraph (captured on first use per B). */
int said_train_step(said_train* t, int B, const int* items_host, const float* eps_host, const float* scalars_host, const float* std_host,
                    int use_graph);
/* clip, AdamW and EMA on the gradients as they stand (set them with SAID_TRAIN_GRAD) */
int said_train_apply_update(said_train* t, const float* scalars_host);
/* eval-mode forward (running statistics) and losses of B windows of `set`, accumulated into the validation accumulators; ema != 0 uses the EMA
 * parameters in place of the live ones */
int said_train_eval_loss(said_train* t, int set, int B, const int* items_host, const float* eps_host, const float* scalars_host, const float* std_host,
                         int ema);
/* the accumulators (SAID_TRAIN_NACC doubles) of the training steps (val = 0) or of eval_loss (val = 1); *status SAID_TRAIN_NOT_FINITE if a step's
 * loss was not finite.  reset != 0 zeroes them afterwards. */
int said_train_read_losses(said_train* t, int val, double* acc_host, int* status, int reset);
/* reconst, regularize, velocity, total of the last step or eval_loss call */
int said_train_last_losses(said_train* t, float* out_host);
/* batch mean and 1 / sqrt(var + eps) of the last training step at BatchNorm layer `bn` (0..7, state-dict order): 2 x C floats */
int said_train_bn_stats(said_train* t, int bn, float* out_host);
/* captured step graphs so far (one per batch size) */
int said_train_graph_count(const said_train* t);

#ifdef __cplusplus
}
#endif
#endif /* SAID_TRAIN_H */
