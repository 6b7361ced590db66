// The bilinear resize (align_corners = true) reading a YUV 4:2:0 SURFACE (hdrnet_resize_bilinear_yuv[_planar],
// include/hdrnet_amd_pyramid_yuv.h): level 1 of the pyramid model built from a decoder surface as it arrives --
//   out [B][Hout][Wout][3] float32 = resize_bilinear_ac(the frame hdrnet_yuv_to_rgb_f32 writes)
// without that frame: a 2:1 reduction of a 4K NV12 surface reads 12 MB where the float32 frame is 100 MB.
//
// Taps, scales and lerps are resize_bilinear_ac's (resize_bilinear.hip), expression for expression: mul_rn, floorf / ceilf,
// the min(., in - 1) clamps, top + (bot - top) * ly.  Each of the four taps is a pixel converted by yuv_load_px
// (yuv_convert.hip.h): luma (row, x), chroma (row >> 1, x >> 1), clamped to [0, 1] BEFORE the blend, as the frame's pixels
// are.  Semi-planar and planar surfaces, uint8 and uint16 samples, pitches and image strides under the surface rules.
//
// The kernel is a gather bound by load latency, as resize_bilinear_io_ac is: a thread owns kYuvRun consecutive output
// pixels, so its 4 * kYuvRun taps' sample loads are independent and in flight together, and its float store is 48
// contiguous bytes (three float4) -- or scalar stores where Wout % 4 != 0 or the output is not 16-byte aligned.  A run's
// pixels past the row repeat its last one and are not stored.  Every tap index is clamped into the surface.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "launch.hip.h"
#include "numerics.hip.h"
#include "yuv_convert.hip.h"

namespace hdrnet_amd {
namespace {

constexpr int kYuvRun = 4;

template <typename TI, class Surface>
__global__ __launch_bounds__(256) void resize_bilinear_yuv_ac(const Surface in, const float* __restrict__ to_rgb,
                                                              float* __restrict__ out, int Hin, int Win, int Hout, int Wout,
                                                              int nrun, float sh, float sw, long long nruns, int vec) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= nruns) return;
  const int x = (int)(p % nrun) * kYuvRun;
  const int y = (int)((p / nrun) % Hout);
  const int b = (int)(p / ((long long)nrun * Hout));
  const YuvMatrix m = yuv_load_matrix(to_rgb);
  const float sy = mul_rn((float)y, sh);
  const float fy = floorf(sy);
  const float ly = sy - fy;
  const int y0 = min((int)fy, Hin - 1), y1 = min((int)ceilf(sy), Hin - 1);
  float tl[kYuvRun][3], tr[kYuvRun][3], bl[kYuvRun][3], br[kYuvRun][3], lx[kYuvRun];
#pragma unroll
  for (int k = 0; k < kYuvRun; ++k) {
    const int xk = min(x + k, Wout - 1);  // a run's pixels past the row repeat its last one and are not stored
    const float sx = mul_rn((float)xk, sw);
    const float fx = floorf(sx);
    lx[k] = sx - fx;
    const int x0 = min((int)fx, Win - 1), x1 = min((int)ceilf(sx), Win - 1);
    yuv_load_px<TI>(in, m, b, y0, x0, tl[k]);
    yuv_load_px<TI>(in, m, b, y0, x1, tr[k]);
    yuv_load_px<TI>(in, m, b, y1, x0, bl[k]);
    yuv_load_px<TI>(in, m, b, y1, x1, br[k]);
  }
  float o[kYuvRun * 3];
#pragma unroll
  for (int k = 0; k < kYuvRun; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float top = tl[k][c] + (tr[k][c] - tl[k][c]) * lx[k];
      const float bot = bl[k][c] + (br[k][c] - bl[k][c]) * lx[k];
      o[k * 3 + c] = top + (bot - top) * ly;
    }
  }
  float* op = out + (((long long)b * Hout + y) * Wout + x) * 3;
  if (vec) {  // uniform: Wout % kYuvRun == 0 and a 16-byte aligned output
#pragma unroll
    for (int q = 0; q < 3; ++q) reinterpret_cast<float4*>(op)[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < kYuvRun; ++k) {
      if (x + k < Wout) {
#pragma unroll
        for (int c = 0; c < 3; ++c) op[k * 3 + c] = o[k * 3 + c];
      }
    }
  }
}

template <class Surface>
hipError_t launch(const Surface& in, int sample_dtype, const float* to_rgb, float* out, int B, int Hin, int Win, int Hout,
                  int Wout, hipStream_t s) {
  if (B <= 0 || Hout <= 0 || Wout <= 0) return hipSuccess;
  if (Hin <= 0 || Win <= 0 || (sample_dtype != 1 && sample_dtype != 2)) return hipErrorInvalidValue;
  const int nrun = (Wout + kYuvRun - 1) / kYuvRun;
  const long long nruns = (long long)B * Hout * nrun;
  const long long nblocks = (nruns + 255) / 256;
  if (nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const float sh = Hout > 1 ? (float)(Hin - 1) / (float)(Hout - 1) : (float)Hin / (float)Hout;
  const float sw = Wout > 1 ? (float)(Win - 1) / (float)(Wout - 1) : (float)Win / (float)Wout;
  const int vec = (Wout % kYuvRun == 0 && ((uintptr_t)out & 15u) == 0) ? 1 : 0;
  if (sample_dtype == 1)
    resize_bilinear_yuv_ac<uint8_t, Surface><<<(unsigned)nblocks, 256, 0, s>>>(in, to_rgb, out, Hin, Win, Hout, Wout, nrun, sh,
                                                                               sw, nruns, vec);
  else
    resize_bilinear_yuv_ac<uint16_t, Surface><<<(unsigned)nblocks, 256, 0, s>>>(in, to_rgb, out, Hin, Win, Hout, Wout, nrun, sh,
                                                                                sw, nruns, vec);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_resize_bilinear_yuv(const YuvSurface& in, int sample_dtype, const float* to_rgb, float* out, int B, int Hin,
                                      int Win, int Hout, int Wout, hipStream_t s, const char** name) {
  *name = sample_dtype == 1 ? "resize_bilinear_yuv/nv12" : "resize_bilinear_yuv/p016";
  return launch(in, sample_dtype, to_rgb, out, B, Hin, Win, Hout, Wout, s);
}

hipError_t launch_resize_bilinear_yuv_planar(const YuvPlanarSurface& in, int sample_dtype, const float* to_rgb, float* out,
                                             int B, int Hin, int Win, int Hout, int Wout, hipStream_t s, const char** name) {
  *name = sample_dtype == 1 ? "resize_bilinear_yuv/i420" : "resize_bilinear_yuv/i016";
  return launch(in, sample_dtype, to_rgb, out, B, Hin, Win, Hout, Wout, s);
}

}  // namespace hdrnet_amd
