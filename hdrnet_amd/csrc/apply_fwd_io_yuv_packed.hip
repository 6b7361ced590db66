// The wire-format forward (apply_fwd_io.hip.h) for packed YUV 4:2:2 surfaces (include/hdrnet_amd_yuv_packed.h): the kernel's
// instantiations with PX = kPxYuvPacked for {YUY2 / UYVY / YVYU uint8, Y210 / Y216 uint16} in x {float32 RGB, uint8 RGB, a
// packed surface of the input's width and order} out, each x the five guide forms -- 30 -- and the plain surface -> float32
// RGB conversion that is their yardstick.  The byte order is a run-time selector (yuv_convert.hip.h), not an instantiation.
// A translation unit of its own, as apply_fwd_io_yuv_422.hip is; every other instantiation is unchanged.
#include "apply_fwd_io.hip.h"

#include "../../include/hdrnet_amd_yuv_packed.h"

namespace hdrnet_amd {
namespace {

static_assert(kPackedYUYV == HDRNET_PACKED_YUYV && kPackedUYVY == HDRNET_PACKED_UYVY && kPackedYVYU == HDRNET_PACKED_YVYU,
              "yuv_convert.hip.h and the header name the same byte orders");

// A lane owns 4 pixels of one row: two dwords of the surface in (four for uint16), three float4 out.
template <typename TI>
__global__ __launch_bounds__(256) void yuv_packed_to_rgb_kernel(const YuvPackedSurface in, const float* __restrict__ to_rgb,
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
hipError_t yuv_packed_types(const ApplyIoArgs& a, hipStream_t s) {
  const bool u8 = a.input_dtype == 1;
  constexpr int CH = kChroma422, PX = kPxYuvPacked;
  switch (a.yuvk->out_kind) {
    case HDRNET_CHROMA_OUT_RGB_F32:
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, float, PX, kOutFrame, CH>(a, s)
                : launch_io<3, 3, true, GUIDE, uint16_t, float, PX, kOutFrame, CH>(a, s);
    case HDRNET_CHROMA_OUT_RGB_U8:
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, uint8_t, PX, kOutFrame, CH>(a, s)
                : launch_io<3, 3, true, GUIDE, uint16_t, uint8_t, PX, kOutFrame, CH>(a, s);
    case HDRNET_CHROMA_OUT_SURFACE_U8:
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, uint8_t, PX, kOutYuy2, CH>(a, s) : hipErrorInvalidValue;
    case HDRNET_CHROMA_OUT_SURFACE_U16:
      return u8 ? hipErrorInvalidValue : launch_io<3, 3, true, GUIDE, uint16_t, uint16_t, PX, kOutY216, CH>(a, s);
    default: return hipErrorInvalidValue;
  }
}

bool packed_order_ok(int sample_dtype, int order) {
  return sample_dtype == 2 ? order == kPackedYUYV : order >= kPackedYUYV && order <= kPackedYVYU;
}

}  // namespace

bool apply_fwd_io_yuv_packed_supported(const ApplyIoArgs& a) {
  if (!a.yuvk || a.yuv || a.yuvp || (a.input_dtype != 1 && a.input_dtype != 2)) return false;
  if (!packed_order_ok(a.input_dtype, a.yuvk->in.order)) return false;
  const int kind = a.yuvk->out_kind;
  if (kind < HDRNET_CHROMA_OUT_RGB_F32 || kind > HDRNET_CHROMA_OUT_SURFACE_U16) return false;
  if (kind == HDRNET_CHROMA_OUT_SURFACE_U8 && a.input_dtype != 1) return false;
  if (kind == HDRNET_CHROMA_OUT_SURFACE_U16 && (a.input_dtype != 2 || (a.yuvk->out_bits != 10 && a.yuvk->out_bits != 16)))
    return false;
  if (kind >= HDRNET_CHROMA_OUT_SURFACE_U8 && a.yuvk->out.order != a.yuvk->in.order) return false;
  return io_surface_ok(a, kChroma422);
}

hipError_t launch_apply_fwd_io_yuv_packed(const ApplyIoArgs& a, hipStream_t s, const char** name) {
  if (!apply_fwd_io_yuv_packed_supported(a)) return hipErrorInvalidValue;
  *name = io_label(a);
  return with_guide_form(a, [&](auto guide) { return yuv_packed_types<decltype(guide)::value>(a, s); });
}

hipError_t launch_yuv_packed_to_rgb(const YuvPackedSurface& in, int sample_dtype, const float* to_rgb, float* rgb, int B, int H,
                                    int W, hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0) return hipSuccess;
  if (H > 65535 || B > 65535 || !packed_order_ok(sample_dtype, in.order)) return hipErrorInvalidValue;  // grid dimensions y and z
  const int threads = 256;
  const dim3 grid((unsigned)((W / 4 + threads - 1) / threads), (unsigned)H, (unsigned)B);
  if (sample_dtype == 1) yuv_packed_to_rgb_kernel<uint8_t><<<grid, threads, 0, s>>>(in, to_rgb, rgb, H, W);
  else if (sample_dtype == 2) yuv_packed_to_rgb_kernel<uint16_t><<<grid, threads, 0, s>>>(in, to_rgb, rgb, H, W);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace hdrnet_amd
