// The wire-format forward (apply_fwd_io.hip.h) for PLANAR YUV surfaces of another chroma layout than 4:2:0
// (include/hdrnet_amd_yuv_chroma.h), written once on the layout CH: the kernel's instantiations for {uint8, uint16} planes in x
// {float32 RGB, uint8 RGB, a planar surface of the same sample width and layout} out x the five guide forms -- 30 per layout,
// as many as apply_fwd_io_yuv_planar.hip's -- and the plain planar surface -> float32 RGB conversion.  Each layout is a
// translation unit of its own (apply_fwd_io_yuv_planar_422.hip: yuv422p...; apply_fwd_io_yuv_planar_444.hip: yuv444p...), so
// that the build's longest compile stays what it was.
#pragma once

#include "apply_fwd_io.hip.h"

namespace hdrnet_amd {
namespace {

// A lane owns 4 pixels of one row: one dword of Y in (two for uint16) and its chroma samples from each of U and V (two for
// 4:2:2, four for 4:4:4), three float4 out.
template <typename TI, int CH>
__global__ __launch_bounds__(256) void yuv_planar_chroma_to_rgb_kernel(const YuvPlanarSurface in, const float* __restrict__ to_rgb,
                                                                       float* __restrict__ rgb, int H, int W) {
  const int x = 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int y = blockIdx.y, b = blockIdx.z;
  if (x >= W) return;
  float c[12];
  yuv_load_quad<TI, CH>(in, yuv_load_matrix(to_rgb), b, y, x, c);
  float4* out = reinterpret_cast<float4*>(rgb + (((size_t)b * (unsigned)H + (unsigned)y) * (unsigned)W + (unsigned)x) * 3);
#pragma unroll
  for (int q = 0; q < 3; ++q) out[q] = make_float4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
}

template <int GUIDE, int CH>
hipError_t planar_chroma_types(const ApplyIoArgs& a, hipStream_t s) {
  const bool u8 = a.input_dtype == 1;
  switch (a.yuvp->out_kind) {
    case 0:  // float32 RGB
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, float, kPxYuvPlanar, kOutFrame, CH>(a, s)
                : launch_io<3, 3, true, GUIDE, uint16_t, float, kPxYuvPlanar, kOutFrame, CH>(a, s);
    case 1:  // uint8 RGB
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, uint8_t, kPxYuvPlanar, kOutFrame, CH>(a, s)
                : launch_io<3, 3, true, GUIDE, uint16_t, uint8_t, kPxYuvPlanar, kOutFrame, CH>(a, s);
    case kYuvPlanarOutPlanar:
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, uint8_t, kPxYuvPlanar, kOutI420, CH>(a, s)
                : launch_io<3, 3, true, GUIDE, uint16_t, uint16_t, kPxYuvPlanar, kOutI016, CH>(a, s);
    default: return hipErrorInvalidValue;
  }
}

template <int CH>
hipError_t launch_planar_chroma(const ApplyIoArgs& a, hipStream_t s, const char** name) {
  if (!apply_fwd_io_yuv_planar_chroma_supported(a) || a.yuvp->chroma != CH) return hipErrorInvalidValue;
  *name = io_label(a);
  return with_guide_form(a, [&](auto guide) { return planar_chroma_types<decltype(guide)::value, CH>(a, s); });
}

template <int CH>
hipError_t launch_planar_chroma_to_rgb(const YuvPlanarSurface& in, int sample_dtype, const float* to_rgb, float* rgb, int B,
                                       int H, int W, hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0) return hipSuccess;
  if (H > 65535 || B > 65535) return hipErrorInvalidValue;  // grid dimensions y and z
  const int threads = 256;
  const dim3 grid((unsigned)((W / 4 + threads - 1) / threads), (unsigned)H, (unsigned)B);
  if (sample_dtype == 1) yuv_planar_chroma_to_rgb_kernel<uint8_t, CH><<<grid, threads, 0, s>>>(in, to_rgb, rgb, H, W);
  else if (sample_dtype == 2) yuv_planar_chroma_to_rgb_kernel<uint16_t, CH><<<grid, threads, 0, s>>>(in, to_rgb, rgb, H, W);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace
}  // namespace hdrnet_amd
