// Training-mode batch norm of the coefficient network (hdrnet/layers.py:30-54 with is_training=True; here
// models._BN: F.batch_norm with gamma = 1, beta trained, the unbiased variance in the running update), on the
// channel-innermost activations [M][C] the convolution and fully connected kernels of coeff_net.hip write.
//
// The statistics of a layer need every row before any row can be normalised, forward and backward, so each way is
// two launches over the same cut of the rows into chunks (coeff_net_bn.hip.h: bn_plan):
//
//   coeff_bn_stats       per chunk and channel the sum and the sum of squares of z
//   coeff_bn_apply       every workgroup re-reduces the chunks' sums in the same fixed order, then writes
//                        y = relu((z - mean) * inv_std + beta) for its own chunk; the workgroups of chunk 0 also save
//                        mean / inv_std for the backward and move the running statistics
//   coeff_bn_bwd_stats   per chunk and channel sum g and sum g * xhat,  g = (dy [+ dy2]) * [y > 0]
//   coeff_bn_bwd_apply   re-reduces them and writes dz = inv_std * (g - mean(g) - xhat * mean(g * xhat)) for its chunk
//                        (in place over dy if asked to); chunk 0 writes dbeta
//
// z stays where the convolution wrote it: xhat is recomputed from it, for every element (the backward formula needs
// it also where y = 0).  The fully connected layers (M = B <= 32 rows) are one launch each way, with the images in
// registers: coeff_bn_fc / coeff_bn_fc_bwd, coeff_fc_train.hip.
//
// Sums run in float64 from the first addend on: E[z^2] - mean^2 then loses nothing that matters (the operands are
// exact to 2^-53, the cancellation costs mean^2 / var of that), and the order of the additions is fixed -- per thread
// its rows in order, a tree over the threads of a workgroup, the chunks in index order.  No atomics, nothing read by
// the host, no allocation.
#include <hip/hip_runtime.h>

#include "coeff_net_bn.hip.h"

namespace hdrnet_amd {
namespace {

struct BnParams {
  const float* z;     // [M][C] raw layer output
  const float* y;     // backward: the activated output (ReLU mask)
  const float* dy;    // backward: gradient of y
  const float* dy2;   // backward: optional second addend
  float* out;         // forward: y; backward: dz (may be dy)
  double* part;       // [nchunks][C][2]
  const float* beta;  // [C]
  float* save;        // [2 C]: mean, inv_std (forward writes, backward reads)
  float* running_mean;
  float* running_var;
  float* dbeta;       // [C]
  int M, C, cwshift, rows_per_chunk, nchunks;
  float eps, momentum;
};

// The thread's place: float4 column c4 of the layer, row `rl` of a pass of `rp` rows; rows [row0, row0 + rows) are the
// workgroup's chunk.
struct BnPlace {
  int c4l, rl, rp, c4, row0, rows;
};

__device__ __forceinline__ BnPlace bn_place(const BnParams& p) {
  BnPlace t;
  const int tid = threadIdx.x;
  t.c4l = tid & ((1 << p.cwshift) - 1);
  t.rl = tid >> p.cwshift;
  t.rp = 256 >> p.cwshift;
  t.c4 = ((int)blockIdx.y << p.cwshift) + t.c4l;
  t.row0 = (int)blockIdx.x * p.rows_per_chunk;
  t.rows = min(p.rows_per_chunk, p.M - t.row0);
  return t;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// The workgroup's sums of (a, b) per channel: a tree over the rows of a pass in LDS, then [chunk][channel] = {A, B}.
__device__ __forceinline__ void bn_chunk_sums(const BnParams& p, const BnPlace& t, const double (&a)[4],
                                              const double (&b)[4], double* red) {
  // red[(rl * cw + c4l) * 8 + 2 * e + {0, 1}]
  double* mine = red + (size_t)threadIdx.x * 8;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    mine[2 * e] = a[e];
    mine[2 * e + 1] = b[e];
  }
  __syncthreads();
  for (int stride = t.rp >> 1; stride >= 1; stride >>= 1) {
    if (t.rl < stride) {
      const double* other = mine + ((size_t)stride << p.cwshift) * 8;
#pragma unroll
      for (int k = 0; k < 8; ++k) mine[k] += other[k];
    }
    __syncthreads();
  }
  if (t.rl == 0) {
    double* dst = p.part + ((size_t)blockIdx.x * p.C + 4 * t.c4) * 2;
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k] = mine[k];
  }
}

// Every workgroup's copy of the layer-wide sums of its channels, chunks added in index order: thread `ch` < 4 << cwshift.
__device__ __forceinline__ void bn_total(const BnParams& p, int ch, double* A, double* B) {
  const int c = ((int)blockIdx.y << (p.cwshift + 2)) + ch;
  double a = 0.0, b = 0.0;
  const double* src = p.part + (size_t)c * 2;
  for (int k = 0; k < p.nchunks; ++k) {
    a += src[(size_t)k * p.C * 2];
    b += src[(size_t)k * p.C * 2 + 1];
  }
  *A = a;
  *B = b;
}

__global__ __launch_bounds__(256) void coeff_bn_stats(const BnParams p) {
  __shared__ double red[256 * 8];
  const BnPlace t = bn_place(p);
  double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
  const float* src = p.z + (size_t)t.row0 * p.C + 4 * t.c4;
  for (int r = t.rl; r < t.rows; r += t.rp) {
    const float4 v = ld4(src + (size_t)r * p.C);
    const double d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s[e] += d[e];
      q[e] = __builtin_fma(d[e], d[e], q[e]);
    }
  }
  bn_chunk_sums(p, t, s, q, red);
}

__global__ __launch_bounds__(256) void coeff_bn_apply(const BnParams p) {
  __shared__ __attribute__((aligned(16))) float sm[256], si[256], sb[256];
  const BnPlace t = bn_place(p);
  const int tid = threadIdx.x;
  if (tid < (4 << p.cwshift)) {
    const int c = ((int)blockIdx.y << (p.cwshift + 2)) + tid;
    double S, Q;
    bn_total(p, tid, &S, &Q);
    const double mean = S / p.M;
    double var = Q / p.M - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const double inv = 1.0 / sqrt(var + (double)p.eps);
    sm[tid] = (float)mean;
    si[tid] = (float)inv;
    sb[tid] = p.beta[c];
    if (blockIdx.x == 0) {
      p.save[c] = (float)mean;
      p.save[p.C + c] = (float)inv;
      const double m = p.momentum;
      p.running_mean[c] = (float)((1.0 - m) * p.running_mean[c] + m * mean);
      p.running_var[c] = (float)((1.0 - m) * p.running_var[c] + m * (var * p.M / (p.M - 1)));
    }
  }
  __syncthreads();
  const float4 mean = ld4(sm + 4 * t.c4l), inv = ld4(si + 4 * t.c4l), beta = ld4(sb + 4 * t.c4l);
  const size_t base = (size_t)t.row0 * p.C + 4 * t.c4;
  for (int r = t.rl; r < t.rows; r += t.rp) {
    const float4 v = ld4(p.z + base + (size_t)r * p.C);
    float4 o;
    o.x = fmaxf((v.x - mean.x) * inv.x + beta.x, 0.0f);
    o.y = fmaxf((v.y - mean.y) * inv.y + beta.y, 0.0f);
    o.z = fmaxf((v.z - mean.z) * inv.z + beta.z, 0.0f);
    o.w = fmaxf((v.w - mean.w) * inv.w + beta.w, 0.0f);
    *reinterpret_cast<float4*>(p.out + base + (size_t)r * p.C) = o;
  }
}

// One element's masked gradient and xhat, four channels.
struct BnBwdElem {
  float g[4], xh[4];
};

__device__ __forceinline__ BnBwdElem bn_bwd_elem(const BnParams& p, size_t off, const float4& mean, const float4& inv) {
  float4 g = ld4(p.dy + off);
  if (p.dy2) {
    const float4 g2 = ld4(p.dy2 + off);
    g = make_float4(g.x + g2.x, g.y + g2.y, g.z + g2.z, g.w + g2.w);
  }
  const float4 y = ld4(p.y + off), z = ld4(p.z + off);
  BnBwdElem e;
  e.g[0] = y.x > 0.0f ? g.x : 0.0f;
  e.g[1] = y.y > 0.0f ? g.y : 0.0f;
  e.g[2] = y.z > 0.0f ? g.z : 0.0f;
  e.g[3] = y.w > 0.0f ? g.w : 0.0f;
  e.xh[0] = (z.x - mean.x) * inv.x;
  e.xh[1] = (z.y - mean.y) * inv.y;
  e.xh[2] = (z.z - mean.z) * inv.z;
  e.xh[3] = (z.w - mean.w) * inv.w;
  return e;
}

__global__ __launch_bounds__(256) void coeff_bn_bwd_stats(const BnParams p) {
  __shared__ double red[256 * 8];
  const BnPlace t = bn_place(p);
  const float4 mean = ld4(p.save + 4 * t.c4), inv = ld4(p.save + p.C + 4 * t.c4);
  double a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};
  const size_t base = (size_t)t.row0 * p.C + 4 * t.c4;
  for (int r = t.rl; r < t.rows; r += t.rp) {
    const BnBwdElem el = bn_bwd_elem(p, base + (size_t)r * p.C, mean, inv);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      a[e] += (double)el.g[e];
      b[e] = __builtin_fma((double)el.g[e], (double)el.xh[e], b[e]);
    }
  }
  bn_chunk_sums(p, t, a, b, red);
}

__global__ __launch_bounds__(256) void coeff_bn_bwd_apply(const BnParams p) {
  __shared__ __attribute__((aligned(16))) float s1[256], s2[256];
  const BnPlace t = bn_place(p);
  const int tid = threadIdx.x;
  if (tid < (4 << p.cwshift)) {
    const int c = ((int)blockIdx.y << (p.cwshift + 2)) + tid;
    double A, B;
    bn_total(p, tid, &A, &B);
    s1[tid] = (float)(A / p.M);
    s2[tid] = (float)(B / p.M);
    if (blockIdx.x == 0) p.dbeta[c] = (float)A;
  }
  __syncthreads();
  const float4 mean = ld4(p.save + 4 * t.c4), inv = ld4(p.save + p.C + 4 * t.c4);
  const float4 m1 = ld4(s1 + 4 * t.c4l), m2 = ld4(s2 + 4 * t.c4l);
  const size_t base = (size_t)t.row0 * p.C + 4 * t.c4;
  for (int r = t.rl; r < t.rows; r += t.rp) {
    const size_t off = base + (size_t)r * p.C;
    const BnBwdElem el = bn_bwd_elem(p, off, mean, inv);
    float4 o;
    o.x = inv.x * (el.g[0] - m1.x - el.xh[0] * m2.x);
    o.y = inv.y * (el.g[1] - m1.y - el.xh[1] * m2.y);
    o.z = inv.z * (el.g[2] - m1.z - el.xh[2] * m2.z);
    o.w = inv.w * (el.g[3] - m1.w - el.xh[3] * m2.w);
    *reinterpret_cast<float4*>(p.out + off) = o;
  }
}

BnParams bn_params(int M, int C, const BnPlan& pl, double* part) {
  BnParams p{};
  p.M = M; p.C = C; p.cwshift = pl.cwshift; p.rows_per_chunk = pl.rows_per_chunk; p.nchunks = pl.nchunks;
  p.part = part;
  return p;
}

}  // namespace

hipError_t launch_bn_forward(const float* z, float* y, int M, int C, const float* beta, float* running_mean,
                             float* running_var, float* save, double* part, float eps, float momentum, hipStream_t s) {
  if (M < 2 || C < 4 || C % 4 != 0) return hipErrorInvalidValue;
  const BnPlan pl = bn_plan(M, C);
  BnParams p = bn_params(M, C, pl, part);
  p.z = z; p.out = y; p.beta = beta; p.save = save; p.running_mean = running_mean; p.running_var = running_var;
  p.eps = eps; p.momentum = momentum;
  const dim3 grid((unsigned)pl.nchunks, (unsigned)pl.groups);
  coeff_bn_stats<<<grid, 256, 0, s>>>(p);
  coeff_bn_apply<<<grid, 256, 0, s>>>(p);
  return hipGetLastError();
}

hipError_t launch_bn_backward(const float* dy, const float* dy2, const float* y, const float* z, const float* save,
                              float* dz, float* dbeta, int M, int C, double* part, hipStream_t s) {
  if (M < 2 || C < 4 || C % 4 != 0) return hipErrorInvalidValue;
  const BnPlan pl = bn_plan(M, C);
  BnParams p = bn_params(M, C, pl, part);
  p.dy = dy; p.dy2 = dy2; p.y = y; p.z = z; p.save = const_cast<float*>(save); p.out = dz; p.dbeta = dbeta;
  const dim3 grid((unsigned)pl.nchunks, (unsigned)pl.groups);
  coeff_bn_bwd_stats<<<grid, 256, 0, s>>>(p);
  coeff_bn_bwd_apply<<<grid, 256, 0, s>>>(p);
  return hipGetLastError();
}

}  // namespace hdrnet_amd
