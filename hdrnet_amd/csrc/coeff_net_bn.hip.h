// Training-mode batch norm of the coefficient network (coeff_net_bn.hip): launch plan, the workspace it adds to the
// forward's, and the launchers the forward (coeff_net.hip) and backward (coeff_net_train.hip) sequences call for the
// convolutions' outputs; the fully connected layers' are in coeff_fc_train.hip.h.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>

#include "../../include/hdrnet_amd_train.h"
#include "coeff_net.hip.h"

namespace hdrnet_amd {

// An activation [M][C] (C = 4 * a power of two) is cut into chunks of rows, one workgroup each per group of <= 256
// channels: thread = (float4 of channels, row of a pass).  At most kBnMaxChunks chunks, so that every workgroup of the
// second stage re-reduces a few partial sums.
constexpr int kBnMaxChunks = 64;
constexpr int kBnRowsPerThread = 8;

struct BnPlan {
  int cwshift;         // float4 columns per workgroup = 1 << cwshift (<= 64)
  int groups;          // column groups = (C / 4) >> cwshift
  int rows_per_chunk;  // rows of a chunk (the last chunk may be shorter)
  int nchunks;
};

inline BnPlan bn_plan(long long M, int C) {
  BnPlan p{};
  const int c4 = C / 4;
  while ((1 << p.cwshift) < c4 && p.cwshift < 6) ++p.cwshift;
  p.groups = c4 >> p.cwshift;
  const long long per_pass = 256 >> p.cwshift;
  long long n = (M + per_pass * kBnRowsPerThread - 1) / (per_pass * kBnRowsPerThread);
  n = n < 1 ? 1 : (n > kBnMaxChunks ? kBnMaxChunks : n);
  p.rows_per_chunk = (int)((M + n - 1) / n);
  p.nchunks = (int)((M + p.rows_per_chunk - 1) / p.rows_per_chunk);
  return p;
}

// the partial sums of one layer: [nchunks][C] pairs of doubles
inline size_t bn_part_doubles(int C) { return (size_t)2 * kBnMaxChunks * C; }

// y = relu((z - mean) * rsqrt(var + eps) + beta) over [M][C]; save[0 .. C) = mean, save[C .. 2C) = rsqrt(var + eps);
// running <- (1 - momentum) * running + momentum * (mean | var * M / (M - 1)).  M >= 2.
hipError_t launch_bn_forward(const float* z, float* y, int M, int C, const float* beta, float* running_mean,
                             float* running_var, float* save, double* part, float eps, float momentum, hipStream_t s);
// g = (dy [+ dy2]) * [y > 0];  dbeta = sum g;  dz = inv_std * (g - mean(g) - xhat * mean(g * xhat)).  dz may be dy.
hipError_t launch_bn_backward(const float* dy, const float* dy2, const float* y, const float* z, const float* save,
                              float* dz, float* dbeta, int M, int C, double* part, hipStream_t s);

namespace {

// What the batch-norm forward keeps beside the plain forward workspace (float offsets from the workspace's start; the
// plain part, net_workspace(d).total * B floats, comes first and holds the ACTIVATED outputs where the plain forward
// holds them, so the backward reads both the same way).
struct BnWorkspace {
  size_t zsplat[8], zlocal1, zg1, zg2;           // raw convolution outputs of the normalised layers, whole batch
  size_t ssplat[8], slocal1, sg1, sg2;           // their saved mean / inv_std, [2 C]
  size_t xh1, xh2, y1, y2, inv1, inv2, zeros;    // fc1 / fc2: xhat, activated output, inv_std; 4 * gl zeros
  size_t part;                                   // partial sums (doubles), reused layer after layer
  size_t total;
};

inline int bn_max_channels(const NetDims& d) { return d.feat > d.gl ? d.feat : d.gl; }

inline BnWorkspace bn_workspace(const NetDims& d, int B) {
  BnWorkspace w{};
  size_t off = net_workspace(d).total * (size_t)B;
  auto take = [&](size_t n) { const size_t o = off; off += (n + 3) & ~(size_t)3; return o; };
  int side = d.N / 2;
  for (int i = 1; i < d.n_ds; ++i) {
    side /= 2;
    const int c = (d.cm * d.gd) << i;
    w.zsplat[i] = take((size_t)B * side * side * c);
    w.ssplat[i] = take((size_t)2 * c);
  }
  const int g1side = (d.sb + 1) / 2;
  w.zlocal1 = take((size_t)B * d.sb * d.sb * d.gl);
  w.zg1 = take((size_t)B * g1side * g1side * d.gl);
  w.zg2 = take((size_t)B * d.gside * d.gside * d.gl);
  w.slocal1 = take((size_t)2 * d.gl);
  w.sg1 = take((size_t)2 * d.gl);
  w.sg2 = take((size_t)2 * d.gl);
  w.xh1 = take((size_t)B * 4 * d.gl);
  w.y1 = take((size_t)B * 4 * d.gl);
  w.inv1 = take((size_t)4 * d.gl);
  w.xh2 = take((size_t)B * 2 * d.gl);
  w.y2 = take((size_t)B * 2 * d.gl);
  w.inv2 = take((size_t)2 * d.gl);
  w.zeros = take((size_t)4 * d.gl);
  w.part = take(2 * bn_part_doubles(bn_max_channels(d)));
  w.total = off;
  return w;
}

}  // namespace
}  // namespace hdrnet_amd
