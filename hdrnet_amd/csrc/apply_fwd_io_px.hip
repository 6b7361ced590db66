// The wire-format forward (apply_fwd_io.hip.h) for frames in BGR, RGBA and BGRA order: the kernel's instantiations for the
// three formats x {uint8, uint16} in x {uint8, float32} out x the five guide forms.  A translation unit of its own so that
// the library's build time stays that of its slowest file; the RGB instantiations are apply_fwd_io.hip's, unchanged.
#include "apply_fwd_io.hip.h"

namespace hdrnet_amd {

hipError_t launch_apply_fwd_io_px(const ApplyIoArgs& a, hipStream_t s) {
  switch (a.pixel_format) {
    case kPxBGR: return dispatch_guides<kPxBGR>(a, s);
    case kPxRGBA: return dispatch_guides<kPxRGBA>(a, s);
    case kPxBGRA: return dispatch_guides<kPxBGRA>(a, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace hdrnet_amd
