/* Packed YUV 4:2:2 surfaces through the wire-format inference path of libhdrnet_amd.so, beside include/hdrnet_amd_yuv_chroma.h
 * (semi-planar and planar 4:2:2 / 4:4:4): what SDI and HDMI capture cards, webcams and most hardware overlays hand over --
 * YUY2 / UYVY / YVYU at 8 bits, Y210 / Y216 at 10 and 16 -- goes through the conversion, the low-res gather and the fused
 * slice-apply forwards as it is, without the strided de-interleave into an NV16 / P210 plane pair and without a float32 frame
 * in between, and a packed surface of the input's sample width and byte order can come out the same way.  A packed surface
 * is the NV16 / P210 surface with its two planes woven into one: every entry point below is its `..._yuv_chroma` counterpart
 * with HDRNET_CHROMA_422, reading and writing one plane in place of two, and gives that counterpart's bits.  Dtype codes,
 * flags, return codes, hdrnet_last_error() and hdrnet_last_kernel() are those of hdrnet_amd.h.
 *
 * The rules, the same for every entry point below:
 *   - The surface (a device pointer): ONE plane [B][H][2 W] samples, uint8 or uint16.  A row of W pixels is W / 2 groups of four
 *     samples; W % 4 == 0 (a lane owns four pixels: two groups), ANY H >= 1 (there is no row pair).
 *   - `order`, the samples of a group:
 *         HDRNET_PACKED_YUYV   Y0 U Y1 V     YUY2, ffmpeg yuyv422
 *         HDRNET_PACKED_UYVY   U Y0 V Y1     ffmpeg uyvy422
 *         HDRNET_PACKED_YVYU   Y0 V Y1 U     ffmpeg yvyu422
 *     uint8 samples take all three.  uint16 samples are Y210 / Y216 and take HDRNET_PACKED_YUYV only, the code in the HIGH
 *     bits of each 16-bit word, as in P210 / P216; another order at 16 bits is refused, with a text that says so.
 *   - `pitch` (bytes per row) is at least 2 W sizeof(sample); `image_stride` (bytes between the images of a batch) is
 *     non-negative and, for B > 1, at least pitch * H.  Base, pitch and image stride are multiples of 4: loads and stores are
 *     aligned dwords that lie wholly inside the row's samples.  Padding is never read and never written.  B * H * W == 0 is a
 *     no-op (kernel name "noop").
 *   - The arithmetic is hdrnet_amd_yuv_chroma.h's for HDRNET_CHROMA_422, expression for expression.  In: its one conversion
 *         c_i = fmed3(fmaf(m_i2, V, fmaf(m_i1, U, fmaf(m_i0, Y, bias_i))), 0, 1)        i = R, G, B
 *     on the samples as stored, chroma REPLICATED: the chroma samples of group x >> 1 serve pixels 2 (x >> 1) and
 *     2 (x >> 1) + 1.  Out: luma per pixel; with l_i the linear chroma term of a pixel,
 *         s = l(y,2k) + l(y,2k+1),   w = 0.5,   code = (T) fmed3(fmaf(s, w, bias_i), 0, code_max) << shift
 *     with code_max = 2^out_bits - 1 and shift = 16 - out_bits for uint16 samples, 255 and 0 for uint8.
 *   - The 12 floats `to_rgb` / `from_rgb` (hdrnet_amd.yuv.yuv_coefficients / yuv_encode_coefficients) are used as they are.
 *   - Outputs, `output_kind` (the codes of hdrnet_amd_yuv_chroma.h): HDRNET_CHROMA_OUT_RGB_F32 (float32 [B][H][W][3]),
 *     HDRNET_CHROMA_OUT_RGB_U8 (uint8 RGB = (uint8)(255 * clip(v, 0, 1))), or a packed surface of the INPUT's sample width and
 *     order with a pitch and image stride of its own: HDRNET_CHROMA_OUT_SURFACE_U8 from uint8 samples (out_bits ignored),
 *     HDRNET_CHROMA_OUT_SURFACE_U16 from uint16 samples with out_bits 10 (Y210) or 16 (Y216).
 *   - The op is Cin = Cout = 3 with offset; the grid and every guide parameter -- a guide map, the folded guide network (with
 *     HDRNET_GUIDE_SIGMOID_FAST / HDRNET_GUIDE_RELU_PRESCALED), the curves guide in its three forms -- and `guide_out` are those
 *     of the entry point each one mirrors, with its limits.
 *   - Anything else is refused with HDRNET_INVALID_ARGUMENT and a text that names the rule, before any HIP call.
 * Kernel names state byte order and sample width: yuy2 / uyvy / yvyu (uint8), y216 (uint16: 10 and 16 bits share it, as p216
 * does) -- e.g. apply_fwd_io/yuy2->yuy2+nnguide, apply_fwd_io/uyvy->u8, apply_fwd_io/yvyu->f32+curvesguide/cells,
 * apply_fwd_io/y216->y216; the conversion is yuv_packed_to_rgb.
 * Out of scope: packed 4:4:4 (AYUV, Y410, Y416), v210, a surface out of another sample width, byte order or container than
 * the input's, a uint16 RGB frame out, the pyramid model, sited or bilinear chroma. */
#ifndef HDRNET_AMD_YUV_PACKED_H_
#define HDRNET_AMD_YUV_PACKED_H_

#include "hdrnet_amd_yuv_chroma.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HDRNET_PACKED_YUYV 0 /* Y0 U Y1 V: YUY2 (uint8), Y210 / Y216 (uint16) */
#define HDRNET_PACKED_UYVY 1 /* U Y0 V Y1 (uint8 only) */
#define HDRNET_PACKED_YVYU 2 /* Y0 V Y1 U (uint8 only) */

/* hdrnet_yuv_chroma_to_rgb_f32.  Kernel name: yuv_packed_to_rgb. */
int hdrnet_yuv_packed_to_rgb_f32(const void* surface, int sample_dtype, int pitch, long long image_stride, int order, int B,
                                 int H, int W, const float* to_rgb, float* rgb, void* stream);

/* hdrnet_lowres_input_yuv_chroma.  Kernel name: sample_prep. */
int hdrnet_lowres_input_yuv_packed(const void* surface, int sample_dtype, int pitch, long long image_stride, int order, int B,
                                   int H, int W, const float* to_rgb, float* lowres, int net_input_size, void* stream);

/* hdrnet_bilateral_slice_apply_io_yuv_chroma (a guide map or the guide network).  An RGB output: `out` is the frame; out_pitch,
 * out_image_stride, from_rgb and out_bits are ignored (pass 0 / NULL). */
int hdrnet_bilateral_slice_apply_io_yuv_packed(const float* grid, const float* guide, const void* surface, int sample_dtype,
                                               int pitch, long long image_stride, int order, int B, int H, int W,
                                               const float* to_rgb, int GH, int GW, int GD, int Cin, int Cout,
                                               int has_offset, const float* guide_conv1, const float* guide_conv2,
                                               int n_feats, float* guide_out, unsigned flags, int output_kind, void* out,
                                               int out_pitch, long long out_image_stride, const float* from_rgb,
                                               int out_bits, void* stream);

/* hdrnet_bilateral_slice_apply_io_curves_yuv_chroma (`prepared` may be NULL: the sorted tables). */
int hdrnet_bilateral_slice_apply_io_curves_yuv_packed(const float* grid, const void* surface, int sample_dtype, int pitch,
                                                      long long image_stride, int order, int B, int H, int W,
                                                      const float* to_rgb, int GH, int GW, int GD, int Cin, int Cout,
                                                      int has_offset, const float* guide_ccm, const float* guide_shifts,
                                                      const float* guide_slopes, const float* guide_mix, int npts,
                                                      const void* prepared, float* guide_out, int output_kind, void* out,
                                                      int out_pitch, long long out_image_stride, const float* from_rgb,
                                                      int out_bits, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* HDRNET_AMD_YUV_PACKED_H_ */
