// BilateralSliceApply forward with the product's wire formats fused in: the RGB instantiations of the kernel in
// apply_fwd_io.hip.h, the launch's front end (predicate, geometry, kernel label) and the curves guide's prepare kernel.
#include "apply_fwd_io.hip.h"

namespace hdrnet_amd {

bool apply_fwd_io_supported(const ApplyIoArgs& a) {
  if (!(a.Cin == 3 && a.Cout == 3 && a.has_offset)) return false;
  if (a.output_dtype != 0 && a.output_dtype != 1) return false;  // a 16-bit output: apply_fwd_io_u16.hip
  if (((uintptr_t)a.input | (uintptr_t)a.out) & 3u) return false;  // quantised pixels: whole dwords per lane
  if (a.pixel_format != kPxRGB) {
    if (a.pixel_format < 0 || a.pixel_format > kPxBGRA || a.input_dtype == 0) return false;  // integer frames only
    // pixels with alpha: one 16-byte access per lane, each way
    if (px_stored(a.pixel_format) == 4 && (((uintptr_t)a.input | (a.output_dtype == 1 ? (uintptr_t)a.out : 0)) & 15u)) return false;
  }
  return io_geom(a).ok;
}

rows::RowGeom apply_fwd_io_geom(const ApplyIoArgs& a) { return io_geom(a); }

size_t curves_guide_prepared_bytes(int Cin) { return Cin == 3 ? CurveCells<3>::kFloats * sizeof(float) : 0; }
size_t curves_guide_prepared_ok_offset(int Cin) { return Cin == 3 ? (size_t)CurveCells<3>::kOk : 0; }

hipError_t launch_curves_guide_prepare(const float* shifts, const float* slopes, int npts, int Cin, float* prepared,
                                       hipStream_t s) {
  if (Cin != 3 || npts > kCurveMaxKnots) return hipErrorInvalidValue;
  const GuideNet gn{nullptr, nullptr, shifts, slopes, nullptr, npts, false, false, nullptr};
  curves_prepare_kernel<3><<<1, 256, 0, s>>>(gn, prepared);
  return hipGetLastError();
}

hipError_t launch_apply_fwd_io(const ApplyIoArgs& a, hipStream_t s, const char** name) {
  if (!apply_fwd_io_supported(a)) return hipErrorInvalidValue;
  static const char* const io[3][2] = {{"f32->f32", "f32->u8"}, {"u8->f32", "u8->u8"}, {"u16->f32", "u16->u8"}};
  static const char* const suffix[5] = {"", "+nnguide", "+curvesguide", "+curvesguide/scan", "+curvesguide/cells"};
  static const char* const px[4] = {"", "/bgr", "/rgba", "/bgra"};
  static thread_local char label[64];
  snprintf(label, sizeof label, "apply_fwd_io/%s%s%s", io[a.input_dtype][a.output_dtype], suffix[io_guide_form(a)],
           px[a.pixel_format]);
  *name = label;
  return a.pixel_format == kPxRGB ? dispatch_guides<kPxRGB>(a, s) : launch_apply_fwd_io_px(a, s);
}

}  // namespace hdrnet_amd
