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
  if (!a.yuv || !(a.Cin == 3 && a.Cout == 3 && a.has_offset)) return false;
  if (a.input_dtype != 1 && a.input_dtype != 2) return false;
  if (a.yuv->out_kind < 0 || a.yuv->out_kind > HDRNET_YUV_OUT_NV12) return false;  // P010 / P016 out: apply_fwd_io_u16.hip
  if (a.H % 2 != 0 || a.W % 4 != 0) return false;
  return io_geom(a).ok;
}

hipError_t launch_apply_fwd_io_yuv(const ApplyIoArgs& a, hipStream_t s, const char** name) {
  if (!apply_fwd_io_yuv_supported(a)) return hipErrorInvalidValue;
  static const char* const out[3] = {"f32", "u8", "nv12"};
  static const char* const suffix[5] = {"", "+nnguide", "+curvesguide", "+curvesguide/scan", "+curvesguide/cells"};
  if (a.yuv->out_kind < 0 || a.yuv->out_kind > 2) return hipErrorInvalidValue;
  static thread_local char label[64];
  snprintf(label, sizeof label, "apply_fwd_io/%s->%s%s", a.input_dtype == 1 ? "nv12" : "p016", out[a.yuv->out_kind],
           suffix[io_guide_form(a)]);
  *name = label;
  switch (io_guide_form(a)) {
    case kGuideMap: return yuv_types<kGuideMap>(a, s);
    case kGuideNN: return yuv_types<kGuideNN>(a, s);
    case kGuideCurves: return yuv_types<kGuideCurves>(a, s);
    case kGuideCurvesCells: return yuv_types<kGuideCurvesCells>(a, s);
    default: return yuv_types<kGuideCurvesScan>(a, s);
  }
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
