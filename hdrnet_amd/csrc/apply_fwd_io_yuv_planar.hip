// The wire-format forward (apply_fwd_io.hip.h) for PLANAR YUV 4:2:0 surfaces (include/hdrnet_amd_yuv_planar.h): the
// kernel's instantiations for {I420 uint8, yuv420p10le / yuv420p16le uint16} in x {float32 RGB, uint8 RGB, a planar surface
// of the same sample width} out x the five guide forms -- 30, as many as apply_fwd_io_yuv.hip's -- and the plain planar
// surface -> float32 RGB conversion beside yuv_to_rgb_kernel.  A translation unit of its own, as apply_fwd_io_yuv.hip is;
// every other instantiation is unchanged.  Not instantiated, and refused by rule: uint16 planar in -> uint8 planar out,
// planar in -> semi-planar out and the reverse.
#include "apply_fwd_io.hip.h"

#include "../../include/hdrnet_amd_yuv_planar.h"

namespace hdrnet_amd {
namespace {

static_assert(kYuvPlanarOutPlanar == HDRNET_YUV_PLANAR_OUT_PLANAR, "launch.hip.h and the header name the same output kind");

// A lane owns 4 pixels of one row: one dword of Y and 16 bits from each of U and V in (two dwords and one from each for
// uint16), three float4 out.
template <typename TI>
__global__ __launch_bounds__(256) void yuv_planar_to_rgb_kernel(const YuvPlanarSurface in, const float* __restrict__ to_rgb,
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
hipError_t planar_types(const ApplyIoArgs& a, hipStream_t s) {
  const bool u8 = a.input_dtype == 1;
  switch (a.yuvp->out_kind) {
    case HDRNET_YUV_PLANAR_OUT_RGB_F32:
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, float, kPxYuvPlanar>(a, s)
                : launch_io<3, 3, true, GUIDE, uint16_t, float, kPxYuvPlanar>(a, s);
    case HDRNET_YUV_PLANAR_OUT_RGB_U8:
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, uint8_t, kPxYuvPlanar>(a, s)
                : launch_io<3, 3, true, GUIDE, uint16_t, uint8_t, kPxYuvPlanar>(a, s);
    case HDRNET_YUV_PLANAR_OUT_PLANAR:
      return u8 ? launch_io<3, 3, true, GUIDE, uint8_t, uint8_t, kPxYuvPlanar, kOutI420>(a, s)
                : launch_io<3, 3, true, GUIDE, uint16_t, uint16_t, kPxYuvPlanar, kOutI016>(a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

bool apply_fwd_io_yuv_planar_supported(const ApplyIoArgs& a) {
  if (!a.yuvp || a.yuv || (a.input_dtype != 1 && a.input_dtype != 2)) return false;
  const int kind = a.yuvp->out_kind;
  if (kind < HDRNET_YUV_PLANAR_OUT_RGB_F32 || kind > HDRNET_YUV_PLANAR_OUT_PLANAR) return false;
  if (kind == HDRNET_YUV_PLANAR_OUT_PLANAR) {  // the code's depth fits the sample width
    const int bits = a.yuvp->out_bits;
    if (a.input_dtype == 1 ? bits != 8 : (bits != 10 && bits != 16)) return false;
  }
  return io_surface_ok(a);
}

hipError_t launch_apply_fwd_io_yuv_planar(const ApplyIoArgs& a, hipStream_t s, const char** name) {
  if (!apply_fwd_io_yuv_planar_supported(a)) return hipErrorInvalidValue;
  *name = io_label(a);
  return with_guide_form(a, [&](auto guide) { return planar_types<decltype(guide)::value>(a, s); });
}

hipError_t launch_yuv_planar_to_rgb(const YuvPlanarSurface& in, int sample_dtype, const float* to_rgb, float* rgb, int B, int H,
                                    int W, hipStream_t s) {
  if (B <= 0 || H <= 0 || W <= 0) return hipSuccess;
  if (H > 65535 || B > 65535) return hipErrorInvalidValue;  // grid dimensions y and z
  const int threads = 256;
  const dim3 grid((unsigned)((W / 4 + threads - 1) / threads), (unsigned)H, (unsigned)B);
  if (sample_dtype == 1) yuv_planar_to_rgb_kernel<uint8_t><<<grid, threads, 0, s>>>(in, to_rgb, rgb, H, W);
  else if (sample_dtype == 2) yuv_planar_to_rgb_kernel<uint16_t><<<grid, threads, 0, s>>>(in, to_rgb, rgb, H, W);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace hdrnet_amd
