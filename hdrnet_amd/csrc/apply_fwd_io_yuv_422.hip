// The wire-format forward (apply_fwd_io.hip.h) for semi-planar YUV 4:2:2 surfaces (include/hdrnet_amd_yuv_chroma.h): the
// kernel's instantiations with CH = kChroma422 for {NV16 uint8, P210 / P216 uint16} in x {float32 RGB, uint8 RGB, NV16} out and
// P210 / P216 -> P210 / P216, each x the five guide forms -- 35 -- and the plain surface -> float32 RGB conversion that is
// their yardstick.  A translation unit of its own, as apply_fwd_io_yuv.hip is; the 4:2:0 instantiations are unchanged.
// Semi-planar 4:4:4 (NV24, P410) is not instantiated and is refused by rule.
#include "apply_fwd_io.hip.h"

#include "../../include/hdrnet_amd_yuv_chroma.h"

namespace hdrnet_amd {
namespace {

static_assert(kChroma420 == HDRNET_CHROMA_420 && kChroma422 == HDRNET_CHROMA_422 && kChroma444 == HDRNET_CHROMA_444,
              "yuv_convert.hip.h and the header name the same layouts");
static_assert(kYuvOutP016 == HDRNET_CHROMA_OUT_SURFACE_U16, "launch.hip.h and the header name the same output kind");

// A lane owns 4 pixels of one row: one dword of Y and one of UV in (two each for uint16), three float4 out.
template <typename TI>
__global__ __launch_bounds__(256) void yuv_422_to_rgb_kernel(const YuvSurface in, const float* __restrict__ to_rgb,
                                                             float* __restrict__ rgb, int H, int W) {
  const int x = 4 * (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int y = blockIdx.y, b = blockIdx.z;
  if (x >= W) return;
  float c[12];
  yuv_load_quad<TI, kChroma422>(in, yuv_load_matrix(to_rgb), b, y, x, c);
  float4* out = reinterpret_cast<float4*>(rgb + (((size_t)b * (unsigned)H + (unsigned)y) * (unsigned)W + (unsigned)x) * 3);
#pragma unroll
  for (int q = 0; q < 3; ++q) out[q] = make_float4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
}

template <int GUIDE>
hipError_t yuv_422_types(const ApplyIoArgs& a, hipStream_t s) {
  const bool u8 = a.input_dtype == 1;
  constexpr int CH = kChroma422;
  switch (a.yuv->out_kind) {
    case HDRNET_CHROMA_OUT_RGB_F32:
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, float, kPxYuv, kOutFrame, CH>(a, s)
                : launch_io<3, 3, true, GUIDE, uint16_t, float, kPxYuv, kOutFrame, CH>(a, s);
    case HDRNET_CHROMA_OUT_RGB_U8:
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, uint8_t, kPxYuv, kOutFrame, CH>(a, s)
                : launch_io<3, 3, true, GUIDE, uint16_t, uint8_t, kPxYuv, kOutFrame, CH>(a, s);
    case HDRNET_CHROMA_OUT_SURFACE_U8:
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, uint8_t, kPxYuv, kOutNV12, CH>(a, s)
                : launch_io<3, 3, true, GUIDE, uint16_t, uint8_t, kPxYuv, kOutNV12, CH>(a, s);
    case HDRNET_CHROMA_OUT_SURFACE_U16:
      return u8 ? hipErrorInvalidValue : launch_io<3, 3, true, GUIDE, uint16_t, uint16_t, kPxYuv, kOutP016, CH>(a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

bool apply_fwd_io_yuv_422_supported(const ApplyIoArgs& a) {
  if (!a.yuv || a.yuvp || a.yuv->chroma != kChroma422 || (a.input_dtype != 1 && a.input_dtype != 2)) return false;
  const int kind = a.yuv->out_kind;
  if (kind < HDRNET_CHROMA_OUT_RGB_F32 || kind > HDRNET_CHROMA_OUT_SURFACE_U16) return false;
  if (kind == HDRNET_CHROMA_OUT_SURFACE_U16 &&
      (a.input_dtype != 2 || (a.yuv->out_bits != 10 && a.yuv->out_bits != 16)))
    return false;
  return io_surface_ok(a, kChroma422);
}

hipError_t launch_apply_fwd_io_yuv_422(const ApplyIoArgs& a, hipStream_t s, const char** name) {
  if (!apply_fwd_io_yuv_422_supported(a)) return hipErrorInvalidValue;
  *name = io_label(a);
  return with_guide_form(a, [&](auto guide) { return yuv_422_types<decltype(guide)::value>(a, s); });
}

hipError_t launch_yuv_422_to_rgb(const YuvSurface& in, int sample_dtype, const float* to_rgb, float* rgb, int B, int H, int W,
                                 hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0) return hipSuccess;
  if (H > 65535 || B > 65535) return hipErrorInvalidValue;  // grid dimensions y and z
  const int threads = 256;
  const dim3 grid((unsigned)((W / 4 + threads - 1) / threads), (unsigned)H, (unsigned)B);
  if (sample_dtype == 1) yuv_422_to_rgb_kernel<uint8_t><<<grid, threads, 0, s>>>(in, to_rgb, rgb, H, W);
  else if (sample_dtype == 2) yuv_422_to_rgb_kernel<uint16_t><<<grid, threads, 0, s>>>(in, to_rgb, rgb, H, W);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace hdrnet_amd
