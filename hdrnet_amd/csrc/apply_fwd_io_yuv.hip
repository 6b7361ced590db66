// The wire-format forward (apply_fwd_io.hip.h) for semi-planar YUV 4:2:0 surfaces (include/hdrnet_amd_yuv.h): the kernel's
// instantiations for {NV12 uint8, P010 / P016 uint16} in x {float32 RGB, uint8 RGB, NV12} out x the five guide forms, and
// the plain surface -> float32 RGB conversion that is their yardstick (hdrnet_yuv_to_rgb_f32).  A translation unit of its
// own, as apply_fwd_io_px.hip is; the RGB and packed-format instantiations are unchanged.
#include "apply_fwd_io.hip.h"

#include "../../include/hdrnet_amd_yuv.h"

namespace hdrnet_amd {
namespace {

// A lane owns 4 pixels of one row: one dword of Y and one of UV in (two each for uint16), three float4 out.
template <typename TI>
__global__ __launch_bounds__(256) void yuv_to_rgb_kernel(const YuvSurface in, const float* __restrict__ to_rgb,
                                                         float* __restrict__ rgb, int H, int W) {
  const int x = 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int y = blockIdx.y, b = blockIdx.z;
  if (x >= W) return;
  float c[12];
  yuv_load_quad<TI>(in, yuv_load_matrix(to_rgb), b, y, x, c);
  float4* out = reinterpret_cast<float4*>(rgb + (((size_t)b * (unsigned)H + (unsigned)y) * (unsigned)W + (unsigned)x) * 3);
#pragma unroll
  for (int q = 0; q < 3; ++q) out[q] = make_float4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
}

template <int GUIDE>
hipError_t yuv_types(const ApplyIoArgs& a, hipStream_t s) {
  const bool u8 = a.input_dtype == 1;
  switch (a.yuv->out_kind) {
    case HDRNET_YUV_OUT_RGB_F32:
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, float, kPxYuv>(a, s) : launch_io<3, 3, true, GUIDE, uint16_t, float, kPxYuv>(a, s);
    case HDRNET_YUV_OUT_RGB_U8:
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, uint8_t, kPxYuv>(a, s)
                : launch_io<3, 3, true, GUIDE, uint16_t, uint8_t, kPxYuv>(a, s);
    case HDRNET_YUV_OUT_NV12:
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, uint8_t, kPxYuv, kOutNV12>(a, s)
                : launch_io<3, 3, true, GUIDE, uint16_t, uint8_t, kPxYuv, kOutNV12>(a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

bool apply_fwd_io_yuv_supported(const ApplyIoArgs& a) {
  if (!a.yuv || (a.input_dtype != 1 && a.input_dtype != 2)) return false;
  if (a.yuv->out_kind < 0 || a.yuv->out_kind > HDRNET_YUV_OUT_NV12) return false;  // P010 / P016 out: apply_fwd_io_u16.hip
  return io_surface_ok(a);
}

hipError_t launch_apply_fwd_io_yuv(const ApplyIoArgs& a, hipStream_t s, const char** name) {
  if (!apply_fwd_io_yuv_supported(a)) return hipErrorInvalidValue;
  *name = io_label(a);
  return with_guide_form(a, [&](auto guide) { return yuv_types<decltype(guide)::value>(a, s); });
}

hipError_t launch_yuv_to_rgb(const YuvSurface& in, int sample_dtype, const float* to_rgb, float* rgb, int B, int H, int W,
                             hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0) return hipSuccess;
  if (H > 65535 || B > 65535) return hipErrorInvalidValue;  // grid dimensions y and z
  const int threads = 256;
  const dim3 grid((unsigned)((W / 4 + threads - 1) / threads), (unsigned)H, (unsigned)B);
  if (sample_dtype == 1) yuv_to_rgb_kernel<uint8_t><<<grid, threads, 0, s>>>(in, to_rgb, rgb, H, W);
  else if (sample_dtype == 2) yuv_to_rgb_kernel<uint16_t><<<grid, threads, 0, s>>>(in, to_rgb, rgb, H, W);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace hdrnet_amd
