/* Wire formats for the pyramid model (HDRNetGaussianPyrNN, hdrnet/models.py:213-289) of libhdrnet_amd.so, beside
 * include/hdrnet_amd.h: the two launches its inference was missing to take a uint8 / uint16 frame in and give a uint8
 * frame out without a float32 copy of the frame -- the resize that builds level 1 from the frame as it arrives, and the
 * finest level's slice-apply + up-add with both conversions in registers.  Dtype codes, white level, flags, return codes,
 * hdrnet_last_error() and hdrnet_last_kernel() are those of hdrnet_bilateral_slice_apply_io_ex (hdrnet_amd.h). */
#ifndef HDRNET_AMD_PYRAMID_IO_H_
#define HDRNET_AMD_PYRAMID_IO_H_

#include "hdrnet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out = resize_bilinear(input / white_level), align_corners = true (TensorFlow's legacy path: the arithmetic of
 * hdrnet_resize_bilinear_f32, tap for tap).
 *   input  [B][Hin][Win][3], input_dtype 0 float32 (never scaled) / 1 uint8 / 2 uint16; 4-byte aligned base
 *   out    [B][Hout][Wout][3] float32
 * value / white_level is the IEEE-rounded division of the wire-format forward.  Any Hin, Win >= 1; an empty output
 * (B, Hout or Wout == 0) is a no-op.  A uint8 row is 3 * Win bytes, so rows start at any byte: every load is an aligned
 * dword that holds at least one byte of the frame.  Refused (1, with a text): a null buffer, a non-positive input extent
 * or a negative output extent, an unknown dtype code, a white level that is not positive, C != 3, a base pointer that is
 * not 4-byte aligned.  Kernel names: resize_bilinear_io/u8, /u16, /f32. */
int hdrnet_resize_bilinear_io(const void* input, int input_dtype, float white_level, float* out, int B, int Hin, int Win,
                              int Hout, int Wout, int C, void* stream);

/* out = wire_out(bilateral_slice_apply(grid, guide, input / white_level) + resize_bilinear(coarse -> H x W)): one level of
 * the pyramid's output (hdrnet/models.py:277-289) with the wire formats of hdrnet_bilateral_slice_apply_io_ex.
 *   input   [B][H][W][3], input_dtype 0 / 1 / 2;   coarse [B][Hc][Wc][3] float32
 *   out     [B][H][W][3], output_dtype 0 float32 or 1 uint8 = (uint8)(255 * clip(v, 0, 1)), the clip AFTER the up-add
 *   guide   EITHER a [B][H][W] map OR the folded guide network (guide_conv1 [n][4], guide_conv2 [n + 1], n_feats);
 *           flags: HDRNET_GUIDE_SIGMOID_FAST, HDRNET_GUIDE_RELU_PRESCALED (guide network only)
 * Supported: Cin = Cout = 3 with offset, W % 4 == 0, 16-byte aligned grid / guide / float buffers, 4-byte aligned
 * integer buffers and coarse.  float32 in with float32 out is hdrnet_bilateral_slice_apply_upadd_f32_ex itself (its
 * kernel, its bits).  Refused (1, with a text) before anything is launched: extents, flags, channel counts, dtype codes
 * or white level, Hc or Wc < 1, both or neither guide, a guide network without conv2 / n_feats, a null buffer, and
 * anything outside "supported".  B * H * W == 0 is a no-op.  Kernel names: apply_fwd_io/<in>-><out>[+nnguide]+upadd. */
int hdrnet_bilateral_slice_apply_upadd_io_ex(const float* grid, const float* guide, const void* input,
                                             const float* coarse, int Hc, int Wc, void* out, int B, int H, int W, int GH,
                                             int GW, int GD, int Cin, int Cout, int has_offset, int input_dtype,
                                             float white_level, int output_dtype, const float* guide_conv1,
                                             const float* guide_conv2, int n_feats, unsigned flags, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* HDRNET_AMD_PYRAMID_IO_H_ */
