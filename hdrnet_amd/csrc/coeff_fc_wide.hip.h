// The fully connected layers of the coefficient network's training step for batches of 9 to 32 images
// (coeff_fc_wide.hip): the launchers the backward sequences (coeff_net_train.hip) and the batch-norm launchers
// (coeff_net_bn.hip) hand such batches to.  Batches up to kCoeffNarrowMaxB stay on coeff_fc_bwd / coeff_bn_fc /
// coeff_bn_fc_bwd.
#pragma once

#include <hip/hip_runtime.h>

namespace hdrnet_amd {

constexpr int kCoeffNarrowMaxB = 8;   // coeff_fc_bwd, coeff_bn_fc, coeff_bn_fc_bwd: one register per image
constexpr int kCoeffWideMaxB = 32;    // their wide twins: 16 or 32 registers per image

// dW [O][K], db [O] (written, not accumulated) and dx [B][K] (or null) of y = x W^T + b: x [B][K], dy [B][O], w [O][K];
// mask_x: dx passes where x > 0.  kCoeffNarrowMaxB < B <= kCoeffWideMaxB.
hipError_t launch_fc_bwd_wide(const float* x, const float* dy, const float* w, float* dw, float* db, float* dx, int B,
                              int K, int O, int mask_x, hipStream_t s);
// launch_bn_fc_forward / launch_bn_fc_backward (coeff_net_bn.hip.h) for kCoeffNarrowMaxB < B <= kCoeffWideMaxB.
hipError_t launch_bn_fc_forward_wide(const float* zpart, int S, int B, int O, const float* beta, float* running_mean,
                                     float* running_var, float* xhat, float* y, float* inv_std, float* zeros, float eps,
                                     float momentum, hipStream_t s);
hipError_t launch_bn_fc_backward_wide(const float* g, const float* xhat, const float* inv_std, float* dz, float* dbeta,
                                      int B, int O, hipStream_t s);

}  // namespace hdrnet_amd
