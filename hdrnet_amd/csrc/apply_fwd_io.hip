// BilateralSliceApply forward with the product's wire formats fused in: the RGB instantiations of the kernel in
// apply_fwd_io.hip.h, their launch (predicate, geometry), the choice of the kernel family among this unit and its
// siblings, and the curves guide's prepare kernel.  What the units' front ends share -- kernel label, guide-form dispatch,
// the predicates' common rules -- is in the header.
#include "apply_fwd_io.hip.h"

namespace hdrnet_amd {

bool apply_fwd_io_supported(const ApplyIoArgs& a) {
  if (a.output_dtype != 0 && a.output_dtype != 1) return false;  // a 16-bit output: apply_fwd_io_u16.hip
  return io_frame_ok(a);
}

// The kernel family of a call, chosen HERE and nowhere else: the 16-bit output's (a.output_dtype == 2), else the pixel
// source's (a.yuv, a.yuvp, or `coarse` for the pyramid's up-add).
namespace {
enum IoFamily { kFamilyFrame, kFamilyYuv, kFamilyU16, kFamilyUpAdd, kFamilyYuvPlanar, kFamilyYuv422, kFamilyYuvPlanarChroma,
                kFamilyUpAddYuv, kFamilyYuvPacked };
IoFamily io_family(const ApplyIoArgs& a, const float* coarse) {
  // (a 4:2:2 / 4:4:4 surface carries every output kind of its own, as a planar one does)
  if (a.yuvk) return kFamilyYuvPacked;  // (a packed 4:2:2 surface: every output kind of its own)
  if (a.yuvp && a.yuvp->chroma != kChroma420) return kFamilyYuvPlanarChroma;
  if (a.yuv && a.yuv->chroma != kChroma420) return kFamilyYuv422;
  if (coarse && (a.yuv || a.yuvp)) return kFamilyUpAddYuv;  // (the pyramid's finest level on a 4:2:0 surface, any output kind)
  if (a.yuvp) return kFamilyYuvPlanar;  // (a planar surface carries its own output kinds, the 16-bit one among them)
  return a.output_dtype == 2 && !coarse ? kFamilyU16 : a.yuv ? kFamilyYuv : coarse ? kFamilyUpAdd : kFamilyFrame;
}
}  // namespace

bool apply_fwd_io_family_supported(const ApplyIoArgs& a, const float* coarse) {
  switch (io_family(a, coarse)) {
    case kFamilyU16: return apply_fwd_io_u16_supported(a);
    case kFamilyYuv: return apply_fwd_io_yuv_supported(a);
    case kFamilyYuvPlanar: return !coarse && apply_fwd_io_yuv_planar_supported(a);
    case kFamilyYuv422: return !coarse && apply_fwd_io_yuv_422_supported(a);
    case kFamilyYuvPacked: return !coarse && apply_fwd_io_yuv_packed_supported(a);
    case kFamilyYuvPlanarChroma: return !coarse && apply_fwd_io_yuv_planar_chroma_supported(a);
    case kFamilyUpAdd: return apply_fwd_io_upadd_supported(a, coarse);
    case kFamilyUpAddYuv: return apply_fwd_io_upadd_yuv_supported(a, coarse);
    default: return apply_fwd_io_supported(a);
  }
}

hipError_t launch_apply_fwd_io_family(const ApplyIoArgs& a, const float* coarse, int Hc, int Wc, hipStream_t s,
                                      const char** name) {
  switch (io_family(a, coarse)) {
    case kFamilyU16: return launch_apply_fwd_io_u16(a, s, name);
    case kFamilyYuv: return launch_apply_fwd_io_yuv(a, s, name);
    case kFamilyYuvPlanar: return launch_apply_fwd_io_yuv_planar(a, s, name);
    case kFamilyYuv422: return launch_apply_fwd_io_yuv_422(a, s, name);
    case kFamilyYuvPacked: return launch_apply_fwd_io_yuv_packed(a, s, name);
    case kFamilyYuvPlanarChroma:
      return a.yuvp->chroma == kChroma422 ? launch_apply_fwd_io_yuv_planar_422(a, s, name)
                                          : launch_apply_fwd_io_yuv_planar_444(a, s, name);
    case kFamilyUpAdd: return launch_apply_fwd_io_upadd(a, coarse, Hc, Wc, s, name);
    case kFamilyUpAddYuv: return launch_apply_fwd_io_upadd_yuv(a, coarse, Hc, Wc, s, name);
    default: return launch_apply_fwd_io(a, s, name);
  }
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
  *name = io_label(a);
  return a.pixel_format == kPxRGB ? dispatch_guides<kPxRGB>(a, s) : launch_apply_fwd_io_px(a, s);
}

}  // namespace hdrnet_amd
