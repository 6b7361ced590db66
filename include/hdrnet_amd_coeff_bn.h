/* Training-loop helper of libhdrnet_amd.so beside include/hdrnet_amd_train.h, which includes this file: the coefficient
 * network's training step WITH batch norm.  Kept in a header of its own because it needs the network description of
 * include/hdrnet_amd.h, which the other helpers do not. */
#ifndef HDRNET_AMD_COEFF_BN_H_
#define HDRNET_AMD_COEFF_BN_H_

#include <stddef.h>

#include "hdrnet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The coefficient network (hdrnet_coeff_net of hdrnet_amd.h) trained WITH batch norm: the reference's --batch_norm
 * (hdrnet/bin/train.py:229; hdrnet/models.py:74-114; hdrnet/layers.py:30-54 with is_training=True), as torch's
 * F.batch_norm(x, running_mean, running_var, weight = 1, bias = beta, training = True, momentum, eps) defines it.  The
 * normalised layers are splat layers 1 .. n_ds - 1, both global convolutions, the first local convolution, fc1 and fc2;
 * such a layer has no bias (its pointer in `net` is not read: leave it NULL) and
 *   y = relu((z - mean) * rsqrt(var + eps) + beta),   mean / var (biased) per channel over batch and pixels,
 *   running_mean <- (1 - momentum) * running_mean + momentum * mean
 *   running_var  <- (1 - momentum) * running_var  + momentum * var * M / (M - 1)      (M = rows of the statistics)
 * The first splat layer, fc3, the second local convolution and the prediction layer are as in hdrnet_coefficients_f32.
 * `net` holds the LIVE parameters in torch's own layouts as hdrnet_coefficients_grad_f32 takes them (Conv2d weights in
 * channels_last memory order, fc_layout = 1); index 0 of the splat arrays below is unused.
 *
 * hdrnet_coefficients_bn_train_f32: lowres [B][N][N][3] -> coeffs [B][sb][sb][gd][n_out][n_in], moving the running
 * statistics in place; `workspace` (hdrnet_coefficients_bn_workspace_bytes) keeps what the backward reads.  The
 * convolution and fully connected launches are those of hdrnet_coefficients_f32; every normalised layer adds two launches
 * (per-chunk sums, then normalise; csrc/coeff_net_bn.hip), fc1 / fc2 one each: 3 * n_ds + 11 launches, 23 at n_ds = 4.
 * hdrnet_coefficients_bn_grad_f32: the gradient of every weight, of the three biases that exist (splat_b[0], fc_b[2],
 * pred_b) and of every beta, WRITTEN (not accumulated) in the parameters' layouts; the other bias pointers of `grads.net`
 * are not written.  `forward_workspace` is the forward call's buffer, untouched since.  The launches of
 * hdrnet_coefficients_grad_f32 plus two per normalised convolution and one per normalised fc layer: 3 * n_ds + 15, 27 at
 * n_ds = 4.
 * Both: no atomics (two calls give identical bits), no host synchronisation, no allocation, capturable in a hipGraph.
 * Like the other training-loop helpers they leave hdrnet_last_kernel() as it was (a sequence of kernels of three files has
 * no one name) and set / clear hdrnet_last_error().
 * Supported: what hdrnet_coefficients_grad_f32 supports with 2 <= B <= 8 (a batch of one has no variance: torch refuses
 * it too) and n_levels = 1; otherwise the workspace queries return 0 and the entry points return 1 with
 * hdrnet_last_error() starting with the entry point's name.  Buffers 16-byte aligned. */
typedef struct hdrnet_coeff_net_bn {
  hdrnet_coeff_net net;
  const float* splat_beta[8];
  float* splat_running_mean[8];
  float* splat_running_var[8];
  const float* global_conv_beta[2];
  float* global_conv_running_mean[2];
  float* global_conv_running_var[2];
  const float* fc_beta[2];
  float* fc_running_mean[2];
  float* fc_running_var[2];
  const float* local_beta; /* the first local convolution */
  float* local_running_mean;
  float* local_running_var;
  float eps;      /* 1e-3 in the reference */
  float momentum; /* 1 - decay: 1e-3 in the reference */
} hdrnet_coeff_net_bn;

typedef struct hdrnet_coeff_net_bn_grads {
  hdrnet_coeff_net_grads net;
  float* splat_beta[8];
  float* global_conv_beta[2];
  float* fc_beta[2];
  float* local_beta;
} hdrnet_coeff_net_bn_grads;

size_t hdrnet_coefficients_bn_workspace_bytes(const hdrnet_coeff_net_bn* net, int B);
int hdrnet_coefficients_bn_train_f32(const float* lowres, const hdrnet_coeff_net_bn* net, float* coeffs, int B,
                                     void* workspace, size_t workspace_bytes, void* stream);
size_t hdrnet_coefficients_bn_grad_workspace_bytes(const hdrnet_coeff_net_bn* net, int B);
int hdrnet_coefficients_bn_grad_f32(const float* lowres, const hdrnet_coeff_net_bn* net, const void* forward_workspace,
                                    const float* dcoeffs, const hdrnet_coeff_net_bn_grads* grads, int B, void* workspace,
                                    size_t workspace_bytes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* HDRNET_AMD_COEFF_BN_H_ */
