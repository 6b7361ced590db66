/* Training-loop helper of libhdrnet_amd.so beside include/hdrnet_amd_train.h, which includes this file: the coefficient
 * network's training step, with and without batch norm, for batches of up to 32 images -- the reference trains with
 * --batch_size 16 (hdrnet/bin/train.py:212) and its data pipeline defaults to 32 (hdrnet/data_pipeline.py:71). */
#ifndef HDRNET_AMD_COEFF_WIDE_H_
#define HDRNET_AMD_COEFF_WIDE_H_

#include <stddef.h>

#include "hdrnet_amd.h"
#include "hdrnet_amd_coeff_bn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Each function is the twin of the one without "wide" in its name (hdrnet_amd.h, hdrnet_amd_coeff_bn.h): the same
 * arguments, layouts, workspaces, return codes and guarantees (written not accumulated, no atomics -- two calls give
 * identical bits --, no host synchronisation, no allocation, capturable in a hipGraph).  The forward without batch norm is
 * hdrnet_coefficients_f32 itself, which takes any batch; its workspace is what hdrnet_coefficients_grad_wide_f32 reads.
 * Supported: what the twin supports with 1 <= B <= 32, with batch norm 2 <= B <= 32.  Up to B = 8 a wide entry point
 * issues exactly its twin's launches (one code path) and returns the same bits; from B = 9 on the fully connected layers'
 * backward and their batch norm run on the 16- and 32-image instances of the kernels of csrc/coeff_fc_train.hip, every
 * other launch is unchanged.  The first entry points keep their range, B <= 8, and their texts.
 * Refusals are the twins': the workspace queries return 0, the entry points return 1 with hdrnet_last_error() starting
 * with the entry point's own name, naming the limit and carrying B=<the batch>.  A workspace is sized by the query of the
 * same name (for B <= 8 the two queries agree). */
size_t hdrnet_coefficients_grad_wide_workspace_bytes(const hdrnet_coeff_net* net, int B);
int hdrnet_coefficients_grad_wide_f32(const float* lowres, const hdrnet_coeff_net* net, const void* forward_workspace,
                                      const float* dcoeffs, const hdrnet_coeff_net_grads* grads, int B, void* workspace,
                                      size_t workspace_bytes, void* stream);
size_t hdrnet_coefficients_bn_wide_workspace_bytes(const hdrnet_coeff_net_bn* net, int B);
int hdrnet_coefficients_bn_train_wide_f32(const float* lowres, const hdrnet_coeff_net_bn* net, float* coeffs, int B,
                                          void* workspace, size_t workspace_bytes, void* stream);
size_t hdrnet_coefficients_bn_grad_wide_workspace_bytes(const hdrnet_coeff_net_bn* net, int B);
int hdrnet_coefficients_bn_grad_wide_f32(const float* lowres, const hdrnet_coeff_net_bn* net, const void* forward_workspace,
                                         const float* dcoeffs, const hdrnet_coeff_net_bn_grads* grads, int B,
                                         void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* HDRNET_AMD_COEFF_WIDE_H_ */
