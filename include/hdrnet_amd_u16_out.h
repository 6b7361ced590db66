/* 16-bit output of the wire-format inference path of libhdrnet_amd.so, beside include/hdrnet_amd.h,
 * include/hdrnet_amd_pixel_formats.h and include/hdrnet_amd_yuv.h: the fused slice-apply forwards store a uint16 frame or a
 * P010 / P016 surface, so that a 16-bit pipeline (HDR+ frames at white level 32767 or 65535, a 10-bit video chain) neither
 * leaves at 8 bits nor takes the float32 frame and quantises it in passes of its own.  Dtype codes, pixel format codes,
 * flags, return codes, hdrnet_last_error() and hdrnet_last_kernel() are those of hdrnet_amd.h and
 * hdrnet_amd_pixel_formats.h; a surface obeys the rules of hdrnet_amd_yuv.h.  The entry points of those headers are
 * unchanged and keep refusing output_dtype = 2 / output_kind = 3.
 *
 * The rules, the same for every entry point below:
 *   - A uint16 frame out: per sample, with c = fmed3(v, 0, 1) of the op's float32 result v,
 *         (uint16)(output_white_level * c)
 *     -- one float32 multiply, then truncation: the uint8 store's rule with 255 replaced by `output_white_level`, which must
 *     be finite with 0 < output_white_level <= 65535.  It is independent of input_white_level.
 *   - The frame in is uint16 (any pixel format) or float32 (HDRNET_PX_RGB only); the frame out has the input's pixel format
 *     (output_format == input_format), [B][H][W][3] or [B][H][W][4].  Alpha of a uint16 frame is copied bit for bit: it
 *     is never divided by a white level and never quantised.  Buffers: 4-byte aligned 3-channel, 16-byte aligned 4-channel
 *     integer frames, 16-byte aligned float32 frames; W % 4 == 0.
 *   - A P010 / P016 surface out: a uint16 surface of the same B, H, W as the uint16 surface in, with pitches and image
 *     strides of its own under the surface rules of hdrnet_amd_yuv.h (a row is W samples = 2 W bytes in either plane).
 *     `out_bits` is 10 (P010) or 16 (P016): the code values have out_bits bits and sit in the HIGH bits of the sample.
 *     `from_rgb` (12 floats: a row-major 3 x 3 matrix f, then 3 biases) is in code units of out_bits bits, with the + 0.5
 *     of the rounding folded into the biases (hdrnet_amd.yuv.yuv_encode_coefficients).  With c = clip(out, 0, 1) per pixel
 *     and channel and M = 2^out_bits - 1:
 *         Y  = ((uint32) fmed3(fmaf(f_02, c_B, fmaf(f_01, c_G, fmaf(f_00, c_R, bias_0))), 0, M)) << (16 - out_bits)
 *         l_i(pixel) = fmaf(f_i2, c_B, fmaf(f_i1, c_G, f_i0 * c_R))                                          i = U, V
 *         s_i = (l_i(2j, 2k) + l_i(2j, 2k + 1)) + (l_i(2j + 1, 2k) + l_i(2j + 1, 2k + 1))
 *         U, V = ((uint32) fmed3(fmaf(s_i, 0.25, bias_i), 0, M)) << (16 - out_bits)                per 2 x 2 block
 *     -- the NV12 rule of hdrnet_amd_yuv.h in the same operation order (horizontal pair first, even row then odd row,
 *     x 0.25, + bias) with another code maximum and the shift.  Padding beyond a row is never written.
 *   - The op is Cin = Cout = 3 with offset; the grid and every guide parameter are those of the entry point each one
 *     extends, and see R, G, B.  Frames in BGR / RGBA / BGRA order take a guide map, the guide network and the curves guide
 *     with at most 16 knots per channel.
 *   - Anything else is refused with HDRNET_INVALID_ARGUMENT and a text that names the rule, before any HIP call.
 *     B * H * W = 0 is a no-op (kernel name "noop").
 * P210 / P216 surfaces out (4:2:2) are include/hdrnet_amd_yuv_chroma.h's: the surface entry points below with a `chroma`
 * argument.
 * Out of scope (the kernels are instantiated for the cases above only): uint8 frames or NV12 surfaces to a 16-bit output,
 * float32 frames in other orders than RGB, a uint16 RGB frame out of a YUV surface, the pyramid model's uint16 RGB frame (its
 * P010 / P016 surface out is include/hdrnet_amd_pyramid_yuv.h's). */
#ifndef HDRNET_AMD_U16_OUT_H_
#define HDRNET_AMD_U16_OUT_H_

#include "hdrnet_amd.h"
#include "hdrnet_amd_pixel_formats.h"
#include "hdrnet_amd_yuv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hdrnet_bilateral_slice_apply_io_px (a guide map, or NULL and the guide network) with `output_dtype` replaced by
 * `output_white_level`: `out` is a uint16 frame in the input's pixel format.  Kernel names: apply_fwd_io/<u16|f32>->u16
 * with the guide and format suffixes of hdrnet_bilateral_slice_apply_io_px, e.g. apply_fwd_io/u16->u16+nnguide/bgra. */
int hdrnet_bilateral_slice_apply_io_px_u16(const float* grid, const float* guide, const void* input, void* out, int B,
                                           int H, int W, int GH, int GW, int GD, int Cin, int Cout, int has_offset,
                                           int input_dtype, float input_white_level, float output_white_level,
                                           const float* guide_conv1, const float* guide_conv2, int n_feats,
                                           float* guide_out, unsigned flags, int input_format, int output_format,
                                           void* stream);

/* hdrnet_bilateral_slice_apply_io_curves_px (`prepared` may be NULL: the sorted tables), changed the same way.  Kernel
 * names: e.g. apply_fwd_io/u16->u16+curvesguide/cells. */
int hdrnet_bilateral_slice_apply_io_curves_px_u16(const float* grid, const void* input, void* out, int B, int H, int W,
                                                  int GH, int GW, int GD, int Cin, int Cout, int has_offset,
                                                  int input_dtype, float input_white_level, float output_white_level,
                                                  const float* guide_ccm, const float* guide_shifts,
                                                  const float* guide_slopes, const float* guide_mix, int npts,
                                                  const void* prepared, float* guide_out, int input_format,
                                                  int output_format, void* stream);

/* hdrnet_bilateral_slice_apply_io_yuv with the `output_kind` ... `from_rgb` tail replaced by the output surface, its
 * constants and `out_bits`: `out_y` / `out_uv` are the planes of a uint16 surface of the same B, H, W.  The surface in
 * must be uint16 (sample_dtype 2).  Kernel names: apply_fwd_io/p016->p016 with the guide suffixes, e.g.
 * apply_fwd_io/p016->p016+nnguide. */
int hdrnet_bilateral_slice_apply_io_yuv_p016(const float* grid, const float* guide, const void* y, const void* uv,
                                             int sample_dtype, int pitch_y, int pitch_uv, long long image_stride_y,
                                             long long image_stride_uv, int B, int H, int W, const float* to_rgb, int GH,
                                             int GW, int GD, int Cin, int Cout, int has_offset, const float* guide_conv1,
                                             const float* guide_conv2, int n_feats, float* guide_out, unsigned flags,
                                             void* out_y, void* out_uv, int out_pitch_y, int out_pitch_uv,
                                             long long out_image_stride_y, long long out_image_stride_uv,
                                             const float* from_rgb, int out_bits, void* stream);

/* hdrnet_bilateral_slice_apply_io_curves_yuv, changed the same way.  Kernel names: e.g.
 * apply_fwd_io/p016->p016+curvesguide/cells. */
int hdrnet_bilateral_slice_apply_io_curves_yuv_p016(const float* grid, const void* y, const void* uv, int sample_dtype,
                                                    int pitch_y, int pitch_uv, long long image_stride_y,
                                                    long long image_stride_uv, int B, int H, int W, const float* to_rgb,
                                                    int GH, int GW, int GD, int Cin, int Cout, int has_offset,
                                                    const float* guide_ccm, const float* guide_shifts,
                                                    const float* guide_slopes, const float* guide_mix, int npts,
                                                    const void* prepared, float* guide_out, void* out_y, void* out_uv,
                                                    int out_pitch_y, int out_pitch_uv, long long out_image_stride_y,
                                                    long long out_image_stride_uv, const float* from_rgb, int out_bits,
                                                    void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* HDRNET_AMD_U16_OUT_H_ */
