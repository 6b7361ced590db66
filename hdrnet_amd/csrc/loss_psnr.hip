// The training loop's monitors in the pass that computes the loss: hdrnet/bin/train.py:95-96, 117-125 groups the minimiser
// with an exponential moving average (decay 0.99) of the l2 loss AND of the PSNR (hdrnet/metrics.py:27-33, the mean over
// the batch of -10 / ln 10 * log(mean per image of the squared difference)), and its evaluation loop (:160-174) averages
// the PSNR over a set.  As separate torch chains the PSNR reads prediction and target a second time in five passes;
// here ONE pass over both (the bytes of l2_loss_partial, csrc/metrics.hip) leaves the sum of squared differences PER
// IMAGE -- and, when wanted, the same unit gradient (2 / n)(prediction - target) -- and a second, one-workgroup launch
// finishes the loss, the per-image mean squared errors, the PSNR and the two optional state blocks on the device.
//
// The partition.  prediction / target are [B][m] fp32, m = n / B.  With B <= kBlocks, image b owns the `share` =
// floor(kBlocks / B) consecutive workgroups b * share .. (b + 1) * share - 1 (grid = B * share <= kBlocks), each striding over
// that image's float4 body; with B > kBlocks the grid is kBlocks workgroups of share 1 and workgroup g walks the whole
// images g, g + kBlocks, ...  Either way partial[b * share + r] belongs to image b alone, so the finish needs no atomics
// and every sum has a fixed order: results are bit-repeatable from launch to launch.
// m need not be a multiple of 4: image b starts at float b * m, 4-byte aligned only.  head = (-b * m) & 3 scalars reach the
// next 16-byte boundary, (m - head) & 3 scalars follow the float4 body; prediction, target and the gradient share the
// misalignment (the bases are 16-byte aligned), so one head serves all three.  The image's workgroup r = 0 takes both.
// Loads are nontemporal (each byte is read once); the gradient is a plain store, the slice-apply's gradient kernels
// read it next -- as in l2_loss_partial.
//
// The finish sums an image's partials in double: one wavefront per image, lane l takes partials l, l + 64, ... in order,
// then a fixed butterfly (share 1: the partial is the sum).  Partials that are zero behind the last non-zero one do not
// change that sum, so with m % 4 == 0 (no heads) an image whose float4 body fits one pass of its workgroups
// (m / 4 <= 256 * share) gets the same bits whatever the batch it arrives in; a larger image's partials depend on its
// share, and its figures on the batch in their last bits.  All per-image figures derive from the REPORTED fp32 mean squared error,
// image_mse[b] = float(S_b / m): psnr_b = -10 / ln 10 * log(image_mse[b]) in double (S_b == 0: +inf, as the reference's
// formula gives), psnr = float(mean_b psnr_b); loss = float(sum_b S_b / n) from the unrounded sums.
//
// EMA block (device fp32 {ema_loss, ema_psnr, updates}): s <- s - (1 - decay)(s - value), value the fp32 loss / psnr just
// stored, formed in double from the stored floats and rounded once on the store; updates += 1 (exact up to 2^24).  The
// shadow starts wherever the caller put it -- 0 in hdrnet_amd.metrics.Monitor -- and is NOT debiased: that is what
// tf.train.ExponentialMovingAverage(decay).apply([tensor]) does for a tensor in TF 1.x as far as the authors remember
// (no TensorFlow was at hand to confirm it; for a Variable the shadow starts at the variable's value instead).  The
// debiased reading, s / (1 - decay^updates), is Python's business.  `decay` travels as a float: 1 - decay is formed in
// double from that float.
// Totals block (device float64 {sum of per-image PSNR, sum of per-image MSE, images}): accumulated in place, image by
// image in index order by one thread, so a set fed in batches of any size adds the same numbers in the same order.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/hdrnet_amd_train.h"
#include "launch.hip.h"

namespace hdrnet_amd {
namespace {

constexpr int kBlocks = 2048;  // workgroups of the first pass at most (kLossBlocks of metrics.hip)
constexpr int kThreads = 256;
typedef float v4f __attribute__((ext_vector_type(4)));

inline int share_of(int B) { return B >= kBlocks ? 1 : kBlocks / B; }
inline int grid_of(int B) { return B >= kBlocks ? kBlocks : share_of(B) * B; }
// partial[B * share] floats, padded to 16 bytes, then per_image[B][2] doubles for the totals block's ordered walk
inline size_t partial_bytes(int B) { return (((size_t)B * share_of(B) * sizeof(float)) + 15u) & ~(size_t)15u; }

template <bool GRAD>
__global__ __launch_bounds__(kThreads) void loss_psnr_partial(const float* __restrict__ pred,
                                                              const float* __restrict__ target, long long m, int B,
                                                              int share, float k, float* __restrict__ partial,
                                                              float* __restrict__ dunit) {
  __shared__ float red[kThreads];
  const int r = (int)(blockIdx.x % (unsigned)share);
  const int images_per_sweep = (int)(gridDim.x / (unsigned)share);  // B when B <= kBlocks (one image per workgroup)
  for (long long b = blockIdx.x / (unsigned)share; b < B; b += images_per_sweep) {
    const long long base = b * m;
    long long head = (4 - (base & 3)) & 3;
    if (head > m) head = m;
    const long long body4 = (m - head) >> 2;
    const int tail = (int)((m - head) & 3);
    const v4f* p4 = reinterpret_cast<const v4f*>(pred + base + head);
    const v4f* t4 = reinterpret_cast<const v4f*>(target + base + head);
    float acc = 0.0f;
    for (long long i = (long long)r * kThreads + threadIdx.x; i < body4; i += (long long)share * kThreads) {
      const v4f a = __builtin_nontemporal_load(p4 + i), c = __builtin_nontemporal_load(t4 + i);
      const float dx = a.x - c.x, dy = a.y - c.y, dz = a.z - c.z, dw = a.w - c.w;
      acc += (dx * dx + dy * dy) + (dz * dz + dw * dw);
      if constexpr (GRAD) {
        v4f d;
        d.x = k * dx, d.y = k * dy, d.z = k * dz, d.w = k * dw;
        reinterpret_cast<v4f*>(dunit + base + head)[i] = d;  // plain store: the slice-apply's gradient kernels read it next
      }
    }
    if (r == 0) {  // the scalars in front of and behind the float4 body
      if ((long long)threadIdx.x < head) {
        const long long i = base + threadIdx.x;
        const float d = pred[i] - target[i];
        acc += d * d;
        if constexpr (GRAD) dunit[i] = k * d;
      }
      if ((int)threadIdx.x < tail) {
        const long long i = base + head + (body4 << 2) + threadIdx.x;
        const float d = pred[i] - target[i];
        acc += d * d;
        if constexpr (GRAD) dunit[i] = k * d;
      }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[b * share + r] = red[0];
  }
}

__global__ __launch_bounds__(kThreads) void loss_psnr_final(const float* __restrict__ partial, int B, int share,
                                                            long long m, float* __restrict__ loss,
                                                            float* __restrict__ psnr, float* __restrict__ image_mse,
                                                            float* __restrict__ ema, float decay,
                                                            double* __restrict__ totals,
                                                            double* __restrict__ per_image) {
  __shared__ double red_s[kThreads], red_p[kThreads];
  const double kDb = -10.0 / 2.302585092994045684;  // -10 / ln 10
  double acc_s = 0.0, acc_p = 0.0;
  auto image = [&](int b, double s) {
    const float mse = (float)(s / (double)m);
    const double p = kDb * log((double)mse);
    if (image_mse) image_mse[b] = mse;
    if (per_image) per_image[2 * (long long)b] = p, per_image[2 * (long long)b + 1] = (double)mse;
    acc_s += s;
    acc_p += p;
  };
  if (share == 1) {
    for (int b = threadIdx.x; b < B; b += kThreads) image(b, (double)partial[b]);
  } else {
    const int lane = threadIdx.x & 63;
    for (int b = threadIdx.x >> 6; b < B; b += kThreads / 64) {
      const float* mine = partial + (long long)b * share;
      double s = 0.0;
      for (int j = lane; j < share; j += 64) s += (double)mine[j];
      for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w, 64);
      if (lane == 0) image(b, s);
    }
  }
  red_s[threadIdx.x] = acc_s;
  red_p[threadIdx.x] = acc_p;
  __syncthreads();  // also: per_image is visible to thread 0
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red_s[threadIdx.x] += red_s[threadIdx.x + s];
      red_p[threadIdx.x] += red_p[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const float l = (float)(red_s[0] / ((double)m * (double)B));
  const float q = (float)(red_p[0] / (double)B);
  loss[0] = l;
  psnr[0] = q;
  if (ema) {
    const double keep = 1.0 - (double)decay, s0 = (double)ema[0], s1 = (double)ema[1];
    ema[0] = (float)(s0 - keep * (s0 - (double)l));
    ema[1] = (float)(s1 - keep * (s1 - (double)q));
    ema[2] += 1.0f;
  }
  if (totals) {
    double t0 = totals[0], t1 = totals[1];
    for (int b = 0; b < B; ++b) t0 += per_image[2 * (long long)b], t1 += per_image[2 * (long long)b + 1];
    totals[0] = t0;
    totals[1] = t1;
    totals[2] += (double)B;
  }
}

}  // namespace
}  // namespace hdrnet_amd

extern "C" size_t hdrnet_loss_psnr_workspace_bytes(long long n, int batch) {
  using namespace hdrnet_amd;
  if (n <= 0 || batch <= 0 || n % batch != 0) return 0;
  return partial_bytes(batch) + (size_t)batch * 2 * sizeof(double);
}

extern "C" int hdrnet_loss_psnr_f32(const float* prediction, const float* target, long long n, int batch, float* loss,
                                    float* psnr, float* image_mse, float* dprediction_unit, float* ema, float decay,
                                    double* totals, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_loss_psnr_f32";
  if (n <= 0 || batch <= 0 || n % batch != 0)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: needs n > 0, batch > 0 and n a multiple of batch (n=%lld, batch=%d)", what, n,
                batch);
  if (!prediction || !target || !loss || !psnr || !workspace)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer", what);
  if (workspace_bytes < hdrnet_loss_psnr_workspace_bytes(n, batch))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: needs a workspace of hdrnet_loss_psnr_workspace_bytes() = %zu bytes", what,
                hdrnet_loss_psnr_workspace_bytes(n, batch));
  if (((uintptr_t)prediction | (uintptr_t)target | (uintptr_t)dprediction_unit | (uintptr_t)workspace) & 15u)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: prediction, target, dprediction_unit and workspace must be 16-B aligned", what);
  if (((uintptr_t)loss | (uintptr_t)psnr | (uintptr_t)image_mse | (uintptr_t)ema) & 3u)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: loss, psnr, image_mse and ema must be 4-B aligned", what);
  if ((uintptr_t)totals & 7u) return fail(HDRNET_INVALID_ARGUMENT, "%s: totals must be 8-B aligned", what);
  if (ema && !(decay >= 0.0f && decay < 1.0f))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: decay must lie in [0, 1) (decay=%g)", what, (double)decay);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long m = n / batch;
  const int share = share_of(batch), grid = grid_of(batch);
  float* partial = static_cast<float*>(workspace);
  double* per_image = totals ? reinterpret_cast<double*>(static_cast<char*>(workspace) + partial_bytes(batch)) : nullptr;
  const float k = (float)(2.0 / (double)n);
  if (dprediction_unit)
    loss_psnr_partial<true><<<grid, kThreads, 0, s>>>(prediction, target, m, batch, share, k, partial, dprediction_unit);
  else
    loss_psnr_partial<false><<<grid, kThreads, 0, s>>>(prediction, target, m, batch, share, k, partial, nullptr);
  loss_psnr_final<<<1, kThreads, 0, s>>>(partial, batch, share, m, loss, psnr, image_mse, ema, decay, totals, per_image);
  return finish_launch(hipGetLastError(), what, nullptr);
}
