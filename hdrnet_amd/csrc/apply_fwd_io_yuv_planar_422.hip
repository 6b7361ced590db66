// Planar YUV 4:2:2 surfaces (yuv422p, yuv422p10le / yuv422p16le; include/hdrnet_amd_yuv_chroma.h): the instantiations of
// apply_fwd_io_yuv_planar_chroma.hip.h with CH = kChroma422, and the predicate both planar layouts share.
#include "apply_fwd_io_yuv_planar_chroma.hip.h"

namespace hdrnet_amd {

bool apply_fwd_io_yuv_planar_chroma_supported(const ApplyIoArgs& a) {
  if (!a.yuvp || a.yuv || (a.input_dtype != 1 && a.input_dtype != 2)) return false;
  const int chroma = a.yuvp->chroma, kind = a.yuvp->out_kind;
  if (chroma != kChroma422 && chroma != kChroma444) return false;
  if (kind < 0 || kind > kYuvPlanarOutPlanar) return false;
  if (kind == kYuvPlanarOutPlanar) {  // the code's depth fits the sample width
    const int bits = a.yuvp->out_bits;
    if (a.input_dtype == 1 ? bits != 8 : (bits != 10 && bits != 16)) return false;
  }
  return io_surface_ok(a, chroma);
}

hipError_t launch_apply_fwd_io_yuv_planar_422(const ApplyIoArgs& a, hipStream_t s, const char** name) {
  return launch_planar_chroma<kChroma422>(a, s, name);
}

hipError_t launch_yuv_planar_422_to_rgb(const YuvPlanarSurface& in, int sample_dtype, const float* to_rgb, float* rgb, int B,
                                        int H, int W, hipStream_t s) {
  return launch_planar_chroma_to_rgb<kChroma422>(in, sample_dtype, to_rgb, rgb, B, H, W, s);
}

}  // namespace hdrnet_amd
