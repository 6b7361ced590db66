// Planar YUV 4:4:4 surfaces (yuv444p, yuv444p10le / yuv444p16le; include/hdrnet_amd_yuv_chroma.h): the instantiations of
// apply_fwd_io_yuv_planar_chroma.hip.h with CH = kChroma444.
#include "apply_fwd_io_yuv_planar_chroma.hip.h"

namespace hdrnet_amd {

hipError_t launch_apply_fwd_io_yuv_planar_444(const ApplyIoArgs& a, hipStream_t s, const char** name) {
  return launch_planar_chroma<kChroma444>(a, s, name);
}

hipError_t launch_yuv_planar_444_to_rgb(const YuvPlanarSurface& in, int sample_dtype, const float* to_rgb, float* rgb, int B,
                                        int H, int W, hipStream_t s) {
  return launch_planar_chroma_to_rgb<kChroma444>(in, sample_dtype, to_rgb, rgb, B, H, W, s);
}

}  // namespace hdrnet_amd
