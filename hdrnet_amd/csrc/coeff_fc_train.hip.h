// The fully connected layers of the coefficient network's training step (coeff_fc_train.hip): the launchers the backward
// sequence (coeff_net_train.hip) and the batch-norm forward (coeff_net.hip) call.  Every kernel holds its images in
// registers, NB = 8, 16 or 32 of them: the launchers take the smallest instance that holds B.
#pragma once

#include <hip/hip_runtime.h>

namespace hdrnet_amd {

constexpr int kCoeffNarrowMaxB = 8;   // the batch limit of the C ABI's first training entry points
constexpr int kCoeffWideMaxB = 32;    // of their ..._wide twins, and with it the largest instance of the kernels

// dW [O][K], db [O] (written, not accumulated) and dx [B][K] (or null) of y = x W^T + b: x [B][K], dy [B][O], w [O][K];
// mask_x: dx passes where x > 0 (the input is a ReLU's output).  1 <= B <= kCoeffWideMaxB.
hipError_t launch_fc_bwd(const float* x, const float* dy, const float* w, float* dw, float* db, float* dx, int B, int K,
                         int O, int mask_x, hipStream_t s);
// Training-mode batch norm of a fully connected layer: z[b][o] = sum_s zpart[b][s][o]; xhat and y = relu(xhat + beta) are
// [B][O], inv_std [O]; `zeros` (optional): O floats set to 0 (the bias the consumers of y read).  2 <= B <= kCoeffWideMaxB.
hipError_t launch_bn_fc_forward(const float* zpart, int S, int B, int O, const float* beta, float* running_mean,
                                float* running_var, float* xhat, float* y, float* inv_std, float* zeros, float eps,
                                float momentum, hipStream_t s);
// g = the gradient of y already masked with [y > 0] (coeff_fc_bwd's mask_x); dz may be g.
hipError_t launch_bn_fc_backward(const float* g, const float* xhat, const float* inv_std, float* dz, float* dbeta, int B,
                                 int O, hipStream_t s);

}  // namespace hdrnet_amd
