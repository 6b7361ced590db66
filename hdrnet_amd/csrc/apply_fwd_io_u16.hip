// The wire-format forward (apply_fwd_io.hip.h) with a 16-BIT OUTPUT (include/hdrnet_amd_u16_out.h): the kernel's
// instantiations that store a uint16 frame (TO = uint16_t) or a P010 / P016 surface (OUT = kOutP016).  A translation unit
// of its own, as apply_fwd_io_px.hip and apply_fwd_io_yuv.hip are; every other instantiation is unchanged.
//
// DELIBERATELY LIMITED, to keep the build small -- 27 instantiations:
//   frame out     uint16 and float32 RGB frames                       x the five guide forms             10
//   frame out     uint16 BGR / RGBA / BGRA frames                     x map, network, curves, cells      12
//   surface out   a uint16 surface (P010 / P016) -> P010 / P016       x the five guide forms              5
// Not instantiated, and refused by apply_fwd_io_u16_supported: uint8 -> 16 bit, float32 frames in packed orders, the
// knot-by-knot curves guide (more than 16 knots) on a packed frame, a uint16 RGB frame out of a YUV surface, an NV12
// surface -> P010 / P016, the pyramid's up-add.
#include "apply_fwd_io.hip.h"

namespace hdrnet_amd {
namespace {

template <int GUIDE, int PX>
hipError_t u16_frame(const ApplyIoArgs& a, hipStream_t s) {
  if (a.input_dtype == 2) return launch_io<3, 3, true, GUIDE, uint16_t, uint16_t, PX>(a, s);
  if constexpr (PX == kPxRGB) {  // float32 frames are RGB
    if (a.input_dtype == 0) return launch_io<3, 3, true, GUIDE, float, uint16_t>(a, s);
  }
  return hipErrorInvalidValue;
}

template <int GUIDE>
hipError_t u16_formats(const ApplyIoArgs& a, hipStream_t s) {
  if (a.yuv) return launch_io<3, 3, true, GUIDE, uint16_t, uint16_t, kPxYuv, kOutP016>(a, s);
  if (a.pixel_format == kPxRGB) return u16_frame<GUIDE, kPxRGB>(a, s);
  if constexpr (GUIDE != kGuideCurvesScan) {
    switch (a.pixel_format) {
      case kPxBGR: return u16_frame<GUIDE, kPxBGR>(a, s);
      case kPxRGBA: return u16_frame<GUIDE, kPxRGBA>(a, s);
      case kPxBGRA: return u16_frame<GUIDE, kPxBGRA>(a, s);
    }
  }
  return hipErrorInvalidValue;
}

}  // namespace

bool apply_fwd_io_u16_supported(const ApplyIoArgs& a) {
  if (a.output_dtype != 2) return false;
  if (a.yuv)  // a uint16 surface in, a uint16 surface out
    return a.input_dtype == 2 && a.yuv->out_kind == kYuvOutP016 && (a.yuv->out_bits == 10 || a.yuv->out_bits == 16) &&
           io_surface_ok(a);
  if (a.input_dtype != 0 && a.input_dtype != 2) return false;  // (so a packed order's integer frame is a uint16 one)
  if (a.pixel_format != kPxRGB && io_guide_form(a) == kGuideCurvesScan) return false;
  return io_frame_ok(a);
}

hipError_t launch_apply_fwd_io_u16(const ApplyIoArgs& a, hipStream_t s, const char** name) {
  if (!apply_fwd_io_u16_supported(a)) return hipErrorInvalidValue;
  *name = io_label(a);
  return with_guide_form(a, [&](auto guide) { return u16_formats<decltype(guide)::value>(a, s); });
}

}  // namespace hdrnet_amd
