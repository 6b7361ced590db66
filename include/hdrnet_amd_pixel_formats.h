/* Pixel formats of the wire-format inference path of libhdrnet_amd.so, beside include/hdrnet_amd.h: frames as decoders,
 * OpenCV and display surfaces hand them over -- B first and / or with an alpha sample per pixel -- go through
 * hdrnet_lowres_input and the fused slice-apply forwards without a repack.  (The reference repacks on the host:
 * hdrnet/bin/run.py:145-150 drops alpha and flips BGR -> RGB, benchmark/src/utils.cc:18-20 and main.cc:146-147 convert
 * on the way in and out.)  Dtype codes, white level, flags, return codes, hdrnet_last_error() and hdrnet_last_kernel()
 * are those of the entry points these extend (hdrnet_amd.h).
 *
 * The rules, the same for every entry point below:
 *   - The op always sees R, G, B: Cin = Cout = 3, the grid and every guide parameter are indexed in that order.  The
 *     format says only where a pixel's samples lie in memory; the permutation happens in the load and in the store.
 *   - Integer frames (uint8, uint16) take all four formats; float32 frames take HDRNET_PX_RGB only.
 *   - A uint8 output has the INPUT's format (output_format == input_format); a float32 output is [B][H][W][3] in RGB
 *     order (output_format == HDRNET_PX_RGB).
 *   - Alpha is not an image sample: it is never divided by the white level and never quantised.  uint8 in -> uint8
 *     out copies the byte; uint16 in -> uint8 out stores alpha >> 8; a float32 output has no alpha.
 *   - W % 4 == 0.  3-channel integer buffers are 4-byte aligned, 4-channel buffers 16-byte aligned (one 16-byte access
 *     per lane); float buffers as in hdrnet_amd.h.
 *   - Anything else is refused with HDRNET_INVALID_ARGUMENT and a text that names the rule, before any HIP call.
 * With both formats HDRNET_PX_RGB every entry point IS the one it extends: the same kernel, the same label.
 * Out of scope: the pyramid model's entry points (hdrnet_amd_pyramid_io.h), hdrnet_prepare_batch, float32 frames in
 * other orders.  A uint16 output is include/hdrnet_amd_u16_out.h's: the entry points below keep refusing
 * output_dtype 2. */
#ifndef HDRNET_AMD_PIXEL_FORMATS_H_
#define HDRNET_AMD_PIXEL_FORMATS_H_

#include "hdrnet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HDRNET_PX_RGB 0  /* 3 samples per pixel, R first (the format of hdrnet_amd.h) */
#define HDRNET_PX_BGR 1  /* 3 samples per pixel, B first */
#define HDRNET_PX_RGBA 2 /* 4 samples per pixel, A last */
#define HDRNET_PX_BGRA 3 /* 4 samples per pixel, A last */

/* hdrnet_lowres_input for frames [B][H][W][3 or 4] in `pixel_format`: lowres [B][n][n][3] float32 is always RGB, the
 * same bits as hdrnet_lowres_input on the repacked frame.  Kernel name: sample_prep. */
int hdrnet_lowres_input_px(const void* frames, int dtype, float white_level, int B, int H, int W, float* lowres,
                           int net_input_size, int pixel_format, void* stream);

/* hdrnet_bilateral_slice_apply_io_ex for an input [B][H][W][3 or 4] in `input_format`; out is [B][H][W][3 or 4] uint8 in
 * `output_format` (== input_format) or [B][H][W][3] float32 (output_format == HDRNET_PX_RGB).  guide_out as there.
 * Kernel names: those of hdrnet_bilateral_slice_apply_io_ex with the format as a suffix, e.g.
 * apply_fwd_io/u8->u8+nnguide/bgra; HDRNET_PX_RGB keeps the label as it is. */
int hdrnet_bilateral_slice_apply_io_px(const float* grid, const float* guide, const void* input, void* out, int B, int H,
                                       int W, int GH, int GW, int GD, int Cin, int Cout, int has_offset, int input_dtype,
                                       float input_white_level, int output_dtype, const float* guide_conv1,
                                       const float* guide_conv2, int n_feats, float* guide_out, unsigned flags,
                                       int input_format, int output_format, void* stream);

/* hdrnet_bilateral_slice_apply_io_curves_prepared (`prepared` may be NULL: the sorted tables) with the same two formats. */
int hdrnet_bilateral_slice_apply_io_curves_px(const float* grid, const void* input, void* out, int B, int H, int W, int GH,
                                              int GW, int GD, int Cin, int Cout, int has_offset, int input_dtype,
                                              float input_white_level, int output_dtype, const float* guide_ccm,
                                              const float* guide_shifts, const float* guide_slopes,
                                              const float* guide_mix, int npts, const void* prepared, float* guide_out,
                                              int input_format, int output_format, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* HDRNET_AMD_PIXEL_FORMATS_H_ */
