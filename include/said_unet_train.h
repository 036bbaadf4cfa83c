/*
 * said_unet_train.h — C ABI of the UNet denoiser trainer (said_amd/csrc/unet_train.hip, unet_trainer.cpp), in libsaid_hip.so beside said_train.h.
 *
 * One context trains UNet1DConditionModel(32, 32, 768) and null_cond_emb of SAID_UNet1D (said/model/diffusion.py) with the step of script/train.py:
 * add_noise, training-mode forward (dropout 0.1 in the five ResBlocks), random_noise_loss, backward, clip_grad_norm_(1.0), torch.optim.AdamW and
 * diffusers' EMAModel.  fp32 throughout; every sum runs in a fixed order, so equal inputs give bit-identical results.  The audio encoder is frozen:
 * its output for the batch is an input.  Paths are relative to the reference repository.
 *
 * Conventions are those of said_train.h: 0 on success, said_unet_train_last_error(ctx) (NULL for create failures) gives the message; `*_host` is
 * host memory.  The context owns its stream: entry points that return host values synchronise it, the others only enqueue.  Tensors are named by
 * their keys in SAID_UNet1D().state_dict(): "null_cond_emb" and "denoiser.model.*".
 *
 * feature_dim.  A context made by said_unet_train_create_dim with feature_dim = F > 0 trains SAID_UNet1D(feature_dim = F) instead: the trainable
 * audio_proj_layer = nn.Linear(768, F) behind the frozen encoder, null_cond_emb (1, 1, F), and UNet1DConditionModel(32, 32, F), whose four
 * attn2.to_k / to_v weights are (192, F).  Its table has 163 tensors: "null_cond_emb", "audio_proj_layer.weight", "audio_proj_layer.bias", then
 * "denoiser.model.*".  The forward projects the audio embedding (proj = audio W^T + b, fp32) and then selects against null_cond_emb; the backward
 * gives audio_proj_layer the context gradient of the conditional samples and null_cond_emb that of the unconditional ones.  The projection is
 * clipped, decayed, updated and EMA-averaged with the rest; eval_loss and forward_only with ema != 0 use its EMA copy.  feature_dim <= 0 is the
 * context of said_unet_train_create: the same 161 tensors, the same launches, the same bits.
 */
#ifndef SAID_UNET_TRAIN_H
#define SAID_UNET_TRAIN_H

#ifdef __cplusplus
extern "C" {
#endif

/* NUM_TENSORS: the default table's size; CTX_DIM: the width of the audio encoder's output (and of the context when feature_dim <= 0);
 * MAX_FEATURE_DIM: the largest feature_dim a context is made for (the K-split workspace and the arena are sized from it at create) */
enum { SAID_UT_NUM_TENSORS = 161, SAID_UT_CHANNELS = 32, SAID_UT_CTX_DIM = 768, SAID_UT_MAX_FEATURE_DIM = 1024 };
/* the per-step scalars (float32, SAID_UT_NSCAL of them; unused slots 0), computed by the host in double as torch does: LR = lr_k,
 * WD_FACTOR = 1 - lr_k wd, STEP_SIZE = lr_k / (1 - beta1^k), BC2_SQRT = sqrt(1 - beta2^k), EMA_OMD = 1 - EMA decay, WVEL / WVERTEX = loss weights,
 * OMB1 = 1 - beta1, B2 = beta2, OMB2 = 1 - beta2, EPS = Adam eps, USE_EMA = 0 / 1, PRED_TYPE = 0 epsilon / 1 sample / 2 v_prediction,
 * DROPOUT = the ResBlocks' dropout probability (0: no mask is drawn) */
enum {
    SAID_UT_S_LR = 0, SAID_UT_S_WD_FACTOR, SAID_UT_S_STEP_SIZE, SAID_UT_S_BC2_SQRT, SAID_UT_S_EMA_OMD, SAID_UT_S_WVEL, SAID_UT_S_WVERTEX,
    SAID_UT_S_OMB1, SAID_UT_S_B2, SAID_UT_S_OMB2, SAID_UT_S_EPS, SAID_UT_S_USE_EMA, SAID_UT_S_PRED_TYPE, SAID_UT_S_DROPOUT, SAID_UT_NSCAL = 16
};
/* the copies of a tensor: parameters, EMA shadow, the last step's gradient (before the clip), Adam's two moments, and the stash that
 * EMAModel.store keeps the live parameters in */
enum { SAID_UT_STATE = 0, SAID_UT_EMA = 1, SAID_UT_GRAD = 2, SAID_UT_EXP_AVG = 3, SAID_UT_EXP_AVG_SQ = 4, SAID_UT_STASH = 5 };
/* loss accumulators: sums of loss * batch size since the last reset, the sample count, the number of steps whose total loss was not finite */
enum { SAID_UT_ACC_PREDICT = 0, SAID_UT_ACC_VELOCITY, SAID_UT_ACC_VERTEX, SAID_UT_ACC_TOTAL, SAID_UT_ACC_COUNT, SAID_UT_ACC_NOT_FINITE,
       SAID_UT_NACC = 8 };
enum { SAID_UT_OK = 0, SAID_UT_NOT_FINITE = 1 };

typedef struct said_unet_train said_unet_train;
/* Workspace for batches of up to `max_batch` windows of up to `max_frames` frames on `device`.  All state starts at zero: set every tensor. */
int said_unet_train_create(said_unet_train** out, int device, int max_batch, int max_frames);
/* The same with SAID_UNet1D's feature_dim: <= 0 is said_unet_train_create; F > 0 adds audio_proj_layer (768 -> F) and makes the context F wide.
 * feature_dim above SAID_UT_MAX_FEATURE_DIM fails with a message. */
int said_unet_train_create_dim(said_unet_train** out, int device, int max_batch, int max_frames, int feature_dim);
int said_unet_train_destroy(said_unet_train* t);
const char* said_unet_train_last_error(const said_unet_train* t);
/* the i-th trainable tensor of the default table (feature_dim <= 0) and its element count; NULL / -1 outside [0, SAID_UT_NUM_TENSORS) */
const char* said_unet_train_tensor_name(int i);
long long said_unet_train_tensor_numel(int i);
/* the table of a given feature_dim, without a context or a device: its size (-1 above SAID_UT_MAX_FEATURE_DIM), the i-th name and element count */
int said_unet_train_table_size(int feature_dim);
const char* said_unet_train_table_name(int feature_dim, int i);
long long said_unet_train_table_numel(int feature_dim, int i);
/* a context's own table (set_tensor, get_tensor, copy, reset_optimizer and the update work over it) and its feature_dim (-1: none) */
int said_unet_train_num_tensors(const said_unet_train* t);
const char* said_unet_train_context_tensor_name(const said_unet_train* t, int i);
long long said_unet_train_context_tensor_numel(const said_unet_train* t, int i);
int said_unet_train_feature_dim(const said_unet_train* t);
int said_unet_train_set_tensor(said_unet_train* t, int which, const char* name, const float* host, long long n);
int said_unet_train_get_tensor(said_unet_train* t, int which, const char* name, float* host, long long n);
/* zero the gradients and both moments and copy the parameters into the EMA shadow */
int said_unet_train_reset_optimizer(said_unet_train* t);
/* copy every tensor's copy `src` into copy `dst` on the device (EMAModel.store / copy_to / restore); enqueues only */
int said_unet_train_copy(said_unet_train* t, int dst, int src);
/* the noise scheduler's alphas_cumprod (n training timesteps, float32 as diffusers keeps them) */
int said_unet_train_set_alphas(said_unet_train* t, const float* alphas_cumprod_host, int n);

/* One optimizer step on B windows of T frames (2 <= T <= max_frames).  coeffs_host, noise_host (B, T, 32): the latents and the noise;
 * timesteps_host (B); cond_host (B): 0 replaces the sample's audio embedding by null_cond_emb; audio_embedding (B, T, 768) in host memory, or
 * in device memory when audio_on_device: always the frozen encoder's output, so with feature_dim > 0 the features BEFORE audio_proj_layer (here
 * and in eval_loss and forward_only); dropout_seed: the Philox key of the step's dropout masks (counter (ResBlock index, element
 * (b T + t) C + c, 0, 0); kept iff (word 0 >> 8) 2^-24 >= p); std_host (32, nullable): the coefficient std; deltas_host (B, 32, 3 V, nullable): each
 * sample's blendshape deltas divided by their mean absolute value, for the vertex loss. */
int said_unet_train_step(said_unet_train* t, int B, int T, const float* coeffs_host, const float* noise_host, const long long* timesteps_host,
                         const int* cond_host, const void* audio_embedding, int audio_on_device, unsigned long long dropout_seed,
                         const float* scalars_host, const float* std_host, const float* deltas_host, int V);
/* the losses of the same objective without dropout and without an update, on the EMA parameters when ema != 0, accumulated into the
 * validation accumulators */
int said_unet_train_eval_loss(said_unet_train* t, int B, int T, const float* coeffs_host, const float* noise_host, const long long* timesteps_host,
                              const int* cond_host, const void* audio_embedding, int audio_on_device, const float* scalars_host,
                              const float* std_host, const float* deltas_host, int V, int ema);
/* the model output (B, T, 32) for the noisy sample `sample_host`, dropout off */
int said_unet_train_forward_only(said_unet_train* t, int B, int T, const float* sample_host, const long long* timesteps_host, const int* cond_host,
                                 const void* audio_embedding, int audio_on_device, int ema, float* out_host);
/* clip, AdamW and EMA on the gradients as they stand */
int said_unet_train_apply_update(said_unet_train* t, const float* scalars_host);
/* the accumulators (SAID_UT_NACC doubles) of the training steps (val = 0) or of eval_loss (val = 1); reset != 0 zeroes them afterwards */
int said_unet_train_read_losses(said_unet_train* t, int val, double* acc_host, int* status, int reset);
/* predict, velocity, vertex, total of the last step or eval_loss call, then the clip factor and the gradient norm of the last update */
int said_unet_train_last_losses(said_unet_train* t, float* out6_host);

#ifdef __cplusplus
}
#endif
#endif /* SAID_UNET_TRAIN_H */
