/*
 * said_unet_train_products.h — the arithmetic of the fine-tuned audio encoder's dense products in a said_unet_train context
 * (said_unet_finetune.h, whose conventions hold here).  Kernel: said_amd/csrc/enc_gemm.hip; host: unet_trainer.cpp.
 *
 * The encoder's dense products are q / k / v / out_proj and the two feed-forward layers of every transformer layer and the feature
 * projection, each as forward, data gradient and weight gradient.  In SAID_UT_PRODUCTS_FP32, the default, they run in fp32 like every
 * other product of the step.  In SAID_UT_PRODUCTS_SPLIT_F16 they run on split-fp16 operands, x ~= h + 2^-11 l with h and l fp16 (22
 * significand bits), with fp32 accumulation on the fp16 matrix instruction.  Activations and weights are split as they are: their domain is
 * |x| < 65504, and an element past it makes its results non-finite.  A gradient operand (dy of a data or weight gradient) is first multiplied
 * by a power of two taken from its own largest magnitude, so that this lies in [2^14, 2^15), and the product by the inverse; both are
 * exact, an all-zero operand gives exact zeros, a non-finite one a non-finite result.  The exact-zero guarantees of said_unet_finetune.h hold
 * in both modes, and so does "equal inputs give equal bits".  Every other product of the step (the denoiser's, audio_proj_layer, the
 * attention head products, the positional convolution) and every column sum is the same in both modes.
 */
#ifndef SAID_UNET_TRAIN_PRODUCTS_H
#define SAID_UNET_TRAIN_PRODUCTS_H

#include "said_unet_finetune.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SAID_UT_PRODUCTS_FP32 = 0, SAID_UT_PRODUCTS_SPLIT_F16 = 1 };
/* the layouts of said_unet_train_dense_product */
enum { SAID_UT_PRODUCT_FORWARD = 0, SAID_UT_PRODUCT_DGRAD = 1, SAID_UT_PRODUCT_WGRAD = 2 };

/* The mode of step_ft, eval_loss_ft and forward_only_ft from the next call on.  Fails with a message on a context without a fine-tuned
 * encoder and on an unknown mode. */
int said_unet_train_set_encoder_products(said_unet_train* t, int mode);
/* the context's mode (-1: null context) */
int said_unet_train_encoder_products(const said_unet_train* t);

/* One dense product of a linear layer with weight W (n, k) on the context's stream, from host arrays, by the route the encoder's products
 * take in `mode`; returns when out_host is written.  For tests of the kernel at shapes the model does not have.
 *   SAID_UT_PRODUCT_FORWARD  out (rows, n) = a (rows, k) W^T + bias (+ res) (+ out);      a = x,  b = W; bias (n) and res (rows, n) nullable
 *   SAID_UT_PRODUCT_DGRAD    out (rows, k) (+)= a (rows, n) W;                            a = dy, b = W
 *   SAID_UT_PRODUCT_WGRAD    out (n, k) = a^T b, a = dy (rows, n), b = x (rows, k); bias_host, res_host and accumulate must be null / 0
 * accumulate != 0: out_host holds the destination's value before the call.  Split mode needs a fine-tuning context and n, k multiples of 64. */
int said_unet_train_dense_product(said_unet_train* t, int layout, int rows, int n, int k, const float* a_host, const float* b_host,
                                  const float* bias_host, const float* res_host, int accumulate, int mode, float* out_host);

#ifdef __cplusplus
}
#endif
#endif /* SAID_UNET_TRAIN_PRODUCTS_H */
