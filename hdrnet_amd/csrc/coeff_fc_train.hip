// The fully connected layers of the coefficient network's training step: the backward of a layer and, with batch norm
// (hdrnet/layers.py:30-54 with is_training=True), the normalisation of fc1 / fc2 over the batch and its backward.  A
// layer has B <= 32 rows (the reference trains with --batch_size 16, hdrnet/bin/train.py; its data pipeline defaults to
// 32), so every kernel keeps one register per image, and the image count is a template parameter, NB = 8, 16 or 32, so
// that every loop over the images unrolls into registers.  The launchers take the smallest NB that holds B.
//
//   coeff_fc_bwd<NB>     dW, db and dx of a layer in one launch.  Thread = (input k, part of the outputs), every
//                        (o, k) of dW owned by one thread; all loads of a 256-output chunk -- the thread's 16
//                        weights, the chunk's dy staged through the LDS -- in flight before the first is used.
//                        3 NB + 16 live values per thread (x, the dx partial sums, the bias gradient's addends,
//                        the weights).  The staged dy ([NB][256]) and the dx partial sums ([NB][16][17]) share one
//                        LDS array: dy is dead when the output loop ends (34 KB at NB = 32 instead of 67.6).
//   coeff_bn_fc<NB>      reduces a layer's partial sums, then mean and M2 per channel in double over the images in
//                        index order; thread (channel, r) finishes images r and r + 16.
//   coeff_bn_fc_bwd<NB>  a thread per channel, sum g and sum g * xhat in double.
//
// Sums over images run b = 0, 1, .. and sums over outputs in the same order in every instance: a batch gives the same
// bits whichever instance holds it.  Deterministic, no atomics.
#include <hip/hip_runtime.h>

#include "coeff_fc_train.hip.h"

namespace hdrnet_amd {
namespace {

struct FcBwdParams {
  const float* x;   // [B][K]: the layer's (activated) input
  const float* dy;  // [B][O]
  const float* w;   // [O][K]
  float* dw;        // [O][K]
  float* db;        // [O]
  float* dx;        // [B][K] or null
  int B, K, O, mask_x;  // mask_x: dx passes where x > 0 (the input is a ReLU's output)
};

// Block = 16 inputs k x 16 parts of the outputs; every (o, k) of dW belongs to exactly one thread.  The layers are tiny
// (<= 1 MB of weights) and the kernel is a chain of memory round trips, so every load of a 256-output chunk is issued before
// the first is used: the 16 weights of a thread as predicated loads of a fully unrolled loop (a run-time trip count leaves
// small layers in the compiler's serial remainder loop: one round trip per output), dy staged through the LDS once per
// workgroup instead of B broadcast loads per output, the bias gradient's loads at the top, spread over the workgroups.
// B <= NB.
template <int NB>
__global__ __launch_bounds__(256) void coeff_fc_bwd(const FcBwdParams p) {
  constexpr int kRedFloats = NB * 16 * 17, kDysFloats = NB * 256;
  __shared__ float lds[kRedFloats > kDysFloats ? kRedFloats : kDysFloats];
  float* dys = lds;  // [NB][256] during the output loop
  float* red = lds;  // [NB][16][17] after it
  const int tid = threadIdx.x, kl = tid & 15, op = tid >> 4;
  const int k = blockIdx.x * 16 + kl;
  const bool k_ok = k < p.K;
  float xk[NB], dxp[NB], dbv[NB];
  const int ob = blockIdx.x * 256 + tid;  // this thread's bias gradient (one per thread of the first O / 256 workgroups)
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    xk[b] = (b < p.B && k_ok) ? p.x[(size_t)b * p.K + k] : 0.0f;
    dbv[b] = (b < p.B && ob < p.O) ? p.dy[(size_t)b * p.O + ob] : 0.0f;
    dxp[b] = 0.0f;
  }
  for (int o0 = 0; o0 < p.O; o0 += 256) {
    if (o0 > 0) __syncthreads();
#pragma unroll
    for (int b = 0; b < NB; ++b)  // rows beyond B repeat the last image: their x is zero
      dys[b * 256 + tid] = (o0 + tid < p.O) ? p.dy[(size_t)min(b, p.B - 1) * p.O + o0 + tid] : 0.0f;
    float w[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int o = o0 + op + 16 * i;
      w[i] = (k_ok && o < p.O) ? p.w[(size_t)o * p.K + k] : 0.0f;
    }
    __syncthreads();
    // the thread's outputs of this chunk are i < ni.  (Asked as `o < p.O` again, the 16 lane masks of the loads above stay
    // in scalar registers across the barrier, which at NB = 32 has none to spare.)
    const int ni = k_ok ? (min(p.O - o0, 256) - op + 15) >> 4 : 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int o = o0 + op + 16 * i;
      float dwv = 0.0f;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const float g = dys[b * 256 + op + 16 * i];
        dwv = __builtin_fmaf(g, xk[b], dwv);
        dxp[b] = __builtin_fmaf(g, w[i], dxp[b]);
      }
      if (i < ni) p.dw[(size_t)o * p.K + k] = dwv;
      // the dx sums are due here: left alone, the compiler keeps all 16 outputs' NB gradients in registers (beyond 256
      // of them at NB = 32) and adds them up after the last store
#pragma unroll
      for (int b = 0; b < NB; ++b) asm volatile("" : "+v"(dxp[b]));
    }
  }
  __syncthreads();  // the last chunk's dy has been read: the array becomes the dx partial sums
#pragma unroll
  for (int b = 0; b < NB; ++b) red[(b * 16 + op) * 17 + kl] = dxp[b];
  __syncthreads();
  if (p.dx && k_ok) {  // thread (kl, op): images op, op + 16
    for (int img = op; img < p.B; img += 16) {
      float v = 0.0f;
#pragma unroll
      for (int o2 = 0; o2 < 16; ++o2) v += red[(img * 16 + o2) * 17 + kl];
      const float xv = p.x[(size_t)img * p.K + k];
      p.dx[(size_t)img * p.K + k] = (p.mask_x && !(xv > 0.0f)) ? 0.0f : v;
    }
  }
  if (ob < p.O) {
    float v = 0.0f;
#pragma unroll
    for (int b = 0; b < NB; ++b) v += dbv[b];  // images beyond B hold zeros: the order of the sum is b = 0, 1, ...
    p.db[ob] = v;
  }
  for (int o = ob + (int)gridDim.x * 256; o < p.O; o += (int)gridDim.x * 256) {  // (a grid below O / 256 workgroups)
    float v = 0.0f;
    for (int b = 0; b < p.B; ++b) v += p.dy[(size_t)b * p.O + o];
    p.db[o] = v;
  }
}

struct BnFcParams {
  const float* zpart;  // forward: [B][S][O] partial sums of the layer's output (coeff_fc)
  const float* g;      // backward: [B][O] masked gradient of y
  const float* beta;
  float* xhat;         // [B][O] (forward writes, backward reads)
  float* y;            // [B][O]
  float* inv_std;      // [O]
  float* zeros;        // [O] or null
  float* running_mean;
  float* running_var;
  float* dz;           // [B][O]
  float* dbeta;        // [O]
  int S, B, O;
  float eps, momentum;
};

// Workgroup = 16 channels x 16 reducers of the partial sums (as coeff_fc reduces its input); then thread (channel, r) =
// images r, r + 16.
template <int NB>
__global__ __launch_bounds__(256) void coeff_bn_fc(const BnFcParams p) {
  __shared__ float red[NB][16][17];
  __shared__ float zs[NB][16];
  const int tid = threadIdx.x, cl = tid & 15, r = tid >> 4;
  const int c = blockIdx.x * 16 + cl;
  const bool c_ok = c < p.O;
  float acc[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) acc[b] = 0.0f;
  if (c_ok) {
    for (int s = r; s < p.S; s += 16) {
#pragma unroll
      for (int b = 0; b < NB; ++b)
        if (b < p.B) acc[b] += p.zpart[((size_t)b * p.S + s) * p.O + c];
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) red[b][r][cl] = acc[b];
  __syncthreads();
  for (int img = r; img < p.B; img += 16) {
    float v = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) v += red[img][k][cl];
    zs[img][cl] = v;
  }
  __syncthreads();
  if (r >= p.B || !c_ok) return;
  double sum = 0.0;
  for (int b = 0; b < p.B; ++b) sum += (double)zs[b][cl];
  const double mean = sum / p.B;
  double m2 = 0.0;
  for (int b = 0; b < p.B; ++b) {
    const double d = (double)zs[b][cl] - mean;
    m2 = __builtin_fma(d, d, m2);
  }
  const double var = m2 / p.B;
  const float inv = (float)(1.0 / sqrt(var + (double)p.eps));
  const float beta = p.beta[c];
  for (int img = r; img < p.B; img += 16) {
    const float xh = (zs[img][cl] - (float)mean) * inv;
    p.xhat[(size_t)img * p.O + c] = xh;
    p.y[(size_t)img * p.O + c] = fmaxf(xh + beta, 0.0f);
  }
  if (r == 0) {
    p.inv_std[c] = inv;
    if (p.zeros) p.zeros[c] = 0.0f;
    const double m = p.momentum;
    p.running_mean[c] = (float)((1.0 - m) * p.running_mean[c] + m * mean);
    p.running_var[c] = (float)((1.0 - m) * p.running_var[c] + m * (m2 / (p.B - 1)));
  }
}

template <int NB>
__global__ __launch_bounds__(256) void coeff_bn_fc_bwd(const BnFcParams p) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= p.O) return;
  float g[NB], xh[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    g[b] = b < p.B ? p.g[(size_t)b * p.O + c] : 0.0f;
    xh[b] = b < p.B ? p.xhat[(size_t)b * p.O + c] : 0.0f;
  }
  const float inv = p.inv_std[c];
  double a = 0.0, q = 0.0;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    a += (double)g[b];
    q = __builtin_fma((double)g[b], (double)xh[b], q);
  }
  const float m1 = (float)(a / p.B), m2 = (float)(q / p.B);
#pragma unroll
  for (int b = 0; b < NB; ++b)
    if (b < p.B) p.dz[(size_t)b * p.O + c] = inv * (g[b] - m1 - xh[b] * m2);
  p.dbeta[c] = (float)a;
}

}  // namespace

// One workgroup per 16 inputs.
hipError_t launch_fc_bwd(const float* x, const float* dy, const float* w, float* dw, float* db, float* dx, int B, int K,
                         int O, int mask_x, hipStream_t s) {
  if (B < 1 || B > kCoeffWideMaxB || K < 1 || O < 1) return hipErrorInvalidValue;
  const FcBwdParams p{x, dy, w, dw, db, dx, B, K, O, mask_x};
  const dim3 grid((unsigned)((K + 15) / 16));
  if (B <= 8) coeff_fc_bwd<8><<<grid, 256, 0, s>>>(p);
  else if (B <= 16) coeff_fc_bwd<16><<<grid, 256, 0, s>>>(p);
  else coeff_fc_bwd<32><<<grid, 256, 0, s>>>(p);
  return hipGetLastError();
}

hipError_t launch_bn_fc_forward(const float* zpart, int S, int B, int O, const float* beta, float* running_mean,
                                float* running_var, float* xhat, float* y, float* inv_std, float* zeros, float eps,
                                float momentum, hipStream_t s) {
  if (B < 2 || B > kCoeffWideMaxB || S < 1 || O < 1) return hipErrorInvalidValue;
  BnFcParams p{};
  p.zpart = zpart; p.S = S; p.B = B; p.O = O; p.beta = beta; p.running_mean = running_mean; p.running_var = running_var;
  p.xhat = xhat; p.y = y; p.inv_std = inv_std; p.zeros = zeros; p.eps = eps; p.momentum = momentum;
  const dim3 grid((unsigned)((O + 15) / 16));
  if (B <= 8) coeff_bn_fc<8><<<grid, 256, 0, s>>>(p);
  else if (B <= 16) coeff_bn_fc<16><<<grid, 256, 0, s>>>(p);
  else coeff_bn_fc<32><<<grid, 256, 0, s>>>(p);
  return hipGetLastError();
}

hipError_t launch_bn_fc_backward(const float* g, const float* xhat, const float* inv_std, float* dz, float* dbeta, int B,
                                 int O, hipStream_t s) {
  if (B < 2 || B > kCoeffWideMaxB || O < 1) return hipErrorInvalidValue;
  BnFcParams p{};
  p.g = g; p.xhat = const_cast<float*>(xhat); p.inv_std = const_cast<float*>(inv_std); p.dz = dz; p.dbeta = dbeta;
  p.B = B; p.O = O;
  const dim3 grid((unsigned)((O + 255) / 256));
  if (B <= 8) coeff_bn_fc_bwd<8><<<grid, 256, 0, s>>>(p);
  else if (B <= 16) coeff_bn_fc_bwd<16><<<grid, 256, 0, s>>>(p);
  else coeff_bn_fc_bwd<32><<<grid, 256, 0, s>>>(p);
  return hipGetLastError();
}

}  // namespace hdrnet_amd
