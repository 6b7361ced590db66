// The finest level of the pyramid model reading a YUV 4:2:0 SURFACE (include/hdrnet_amd_pyramid_yuv.h): the wire-format
// forward of apply_fwd_io.hip.h for PX = kPxYuv / kPxYuvPlanar with UPADD = true -- the bilinear (align_corners) up-add of
// the coarser level's output (upadd_quad, rows_common.hip.h; hdrnet/models.py:283-287) applied to a lane's 4 pixels after
// the pixel phase and before any store:
//   out = wire_out(slice_apply(grid, guide, to_rgb(surface)) + resize_bilinear(coarse -> H x W))
// with wire_out = identity (float32 RGB), (uint8)(255 * clip(., 0, 1)) (uint8 RGB) or the surface store of the input's
// container -- the clip, the luma code and the 2 x 2 chroma sums all AFTER the add.  A surface output keeps the row pair
// per workgroup; the up-add runs once per row with that row's y.  At 4K the level moves 1.5 + 1.5 B/px instead of 12 + 12.
//
// What apply_fwd_io_upadd.hip is to the RGB frames, as instantiations of the ONE kernel rather than a kernel of its own:
// load, LDS image, pixel phase and the stores are the single-level surface forwards', geometry and predicate rules are
// theirs (io_surface_ok -> io_geom, the RowGeom that apply_fwd_io_geom returns).  13 input -> output pairs x {guide map,
// guide network} = 26 instantiations; the curves guide belongs to the single-level models and is refused.
//   NV12 -> f32, u8, NV12        P010 / P016 -> f32, u8, NV12, P010 / P016
//   I420 -> f32, u8, I420        uint16 planar -> f32, u8, uint16 planar
// Out of scope: 4:2:2 / 4:4:4 surfaces, a uint16 RGB frame out.
#include "apply_fwd_io.hip.h"

#include "../../include/hdrnet_amd_yuv.h"
#include "../../include/hdrnet_amd_yuv_planar.h"

namespace hdrnet_amd {
namespace {

template <int GUIDE, typename TI, typename TO, int PX, int OUT = kOutFrame>
hipError_t launch_up(const ApplyIoArgs& a, const UpAdd& up, hipStream_t s) {
  return launch_io<3, 3, true, GUIDE, TI, TO, PX, OUT, kChroma420, true>(a, s, &up);
}

template <int GUIDE>
hipError_t semi_planar_types(const ApplyIoArgs& a, const UpAdd& up, hipStream_t s) {
  const bool u8 = a.input_dtype == 1;
  switch (a.yuv->out_kind) {
    case HDRNET_YUV_OUT_RGB_F32:
      return u8 ? launch_up<GUIDE, uint8_t, float, kPxYuv>(a, up, s) : launch_up<GUIDE, uint16_t, float, kPxYuv>(a, up, s);
    case HDRNET_YUV_OUT_RGB_U8:
      return u8 ? launch_up<GUIDE, uint8_t, uint8_t, kPxYuv>(a, up, s) : launch_up<GUIDE, uint16_t, uint8_t, kPxYuv>(a, up, s);
    case HDRNET_YUV_OUT_NV12:
      return u8 ? launch_up<GUIDE, uint8_t, uint8_t, kPxYuv, kOutNV12>(a, up, s)
                : launch_up<GUIDE, uint16_t, uint8_t, kPxYuv, kOutNV12>(a, up, s);
    case kYuvOutP016:
      return u8 ? hipErrorInvalidValue : launch_up<GUIDE, uint16_t, uint16_t, kPxYuv, kOutP016>(a, up, s);
    default: return hipErrorInvalidValue;
  }
}

template <int GUIDE>
hipError_t planar_types(const ApplyIoArgs& a, const UpAdd& up, hipStream_t s) {
  const bool u8 = a.input_dtype == 1;
  switch (a.yuvp->out_kind) {
    case HDRNET_YUV_PLANAR_OUT_RGB_F32:
      return u8 ? launch_up<GUIDE, uint8_t, float, kPxYuvPlanar>(a, up, s)
                : launch_up<GUIDE, uint16_t, float, kPxYuvPlanar>(a, up, s);
    case HDRNET_YUV_PLANAR_OUT_RGB_U8:
      return u8 ? launch_up<GUIDE, uint8_t, uint8_t, kPxYuvPlanar>(a, up, s)
                : launch_up<GUIDE, uint16_t, uint8_t, kPxYuvPlanar>(a, up, s);
    case HDRNET_YUV_PLANAR_OUT_PLANAR:
      return u8 ? launch_up<GUIDE, uint8_t, uint8_t, kPxYuvPlanar, kOutI420>(a, up, s)
                : launch_up<GUIDE, uint16_t, uint16_t, kPxYuvPlanar, kOutI016>(a, up, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

// The single-level surface forward's own predicate (one geometry: io_surface_ok -> io_geom) + a map or the network as the
// guide, nothing to write beside the output, and a coarse level readable dword by dword.
bool apply_fwd_io_upadd_yuv_supported(const ApplyIoArgs& a, const float* coarse) {
  if (!coarse || ((uintptr_t)coarse & 3u) || a.guide_shifts || a.guide_out) return false;
  if (a.yuvp) return !a.yuv && a.yuvp->chroma == kChroma420 && apply_fwd_io_yuv_planar_supported(a);
  if (!a.yuv || a.yuv->chroma != kChroma420) return false;
  return a.output_dtype == 2 ? apply_fwd_io_u16_supported(a) : apply_fwd_io_yuv_supported(a);
}

hipError_t launch_apply_fwd_io_upadd_yuv(const ApplyIoArgs& a, const float* coarse, int Hc, int Wc, hipStream_t s,
                                         const char** name) {
  if (!apply_fwd_io_upadd_yuv_supported(a, coarse) || Hc < 1 || Wc < 1) return hipErrorInvalidValue;
  static thread_local char label[80];
  snprintf(label, sizeof label, "%s+upadd", io_label(a));
  *name = label;
  const UpAdd up{coarse, Hc, Wc, resize_scale(Hc, a.H), resize_scale(Wc, a.W)};
  if (a.guide)
    return a.yuvp ? planar_types<kGuideMap>(a, up, s) : semi_planar_types<kGuideMap>(a, up, s);
  return a.yuvp ? planar_types<kGuideNN>(a, up, s) : semi_planar_types<kGuideNN>(a, up, s);
}

}  // namespace hdrnet_amd
