/* Semi-planar YUV 4:2:0 surfaces through the wire-format inference path of libhdrnet_amd.so, beside
 * include/hdrnet_amd.h and include/hdrnet_amd_pixel_formats.h: what video decoders and encoders exchange -- NV12 (a uint8 Y
 * plane and an interleaved half-resolution UV plane) and P010 / P016 (the same planes with uint16 samples, the
 * significant bits in the high bits) -- goes through the low-res gather and the fused slice-apply forwards without a
 * conversion pass, and an NV12 surface can come out the same way.  Dtype codes, flags, return codes,
 * hdrnet_last_error() and hdrnet_last_kernel() are those of hdrnet_amd.h.
 *
 * The rules, the same for every entry point below:
 *   - A surface is `y`, `uv` (device pointers, 4-byte aligned), `sample_dtype` (1 uint8, 2 uint16: the codes of
 *     hdrnet_amd.h), `pitch_y`, `pitch_uv` (bytes per row: at least the row's bytes -- W samples in either plane -- and a
 *     multiple of 4), `image_stride_y`, `image_stride_uv` (bytes between the images of a batch: a multiple of 4, and for
 *     B > 1 at least the plane: pitch_y * H, pitch_uv * H / 2), and B, H, W with H % 2 == 0 and W % 4 == 0.  Decoder
 *     surfaces have a pitch wider than the row: padding is never read as pixels and never written.
 *   - Chroma is REPLICATED: chroma sample (y >> 1, x >> 1) serves its 2 x 2 block, as a repeat_interleave of the chroma
 *     plane does.  Sited or bilinear chroma is out of scope.
 *   - The kernels know nothing of colour standards, ranges or bit depths: they apply 12 floats, `to_rgb` / `from_rgb`
 *     (device pointers, 4-byte aligned): a row-major 3 x 3 matrix m, then 3 biases.  hdrnet_amd.yuv.yuv_coefficients
 *     computes them for BT.601 / BT.709 / BT.2020, limited or full range, 8 / 10 / 16 bits.
 *   - In, for every entry point, one function (csrc/yuv_convert.hip.h) in exactly this form, Y, U, V being the samples
 *     AS STORED converted to float (P010: code << 6):
 *         c_i = fmed3(fmaf(m_i2, V, fmaf(m_i1, U, fmaf(m_i0, Y, bias_i))), 0, 1)        i = R, G, B
 *   - Out (HDRNET_YUV_OUT_NV12; uint8 code values, the + 0.5 of the rounding folded into from_rgb's biases), with
 *     c = clip(out, 0, 1) per pixel and channel:
 *         Y  = (uint8) fmed3(fmaf(f_02, c_B, fmaf(f_01, c_G, fmaf(f_00, c_R, bias_0))), 0, 255)              per pixel
 *         l_i(pixel) = fmaf(f_i2, c_B, fmaf(f_i1, c_G, f_i0 * c_R))                                          i = U, V
 *         s_i = (l_i(2j, 2k) + l_i(2j, 2k + 1)) + (l_i(2j + 1, 2k) + l_i(2j + 1, 2k + 1))
 *         U, V = (uint8) fmed3(fmaf(s_i, 0.25, bias_i), 0, 255)                                   per 2 x 2 block
 *     -- the mean of the block's four pixels: horizontal pair first, even row then odd row, x 0.25, + bias -- stored as
 *     one interleaved UV row per row pair.  (uint8) truncates.  The output is NV12 for either input depth.
 *   - The op is Cin = Cout = 3 with offset; the grid and every guide parameter are those of the entry point each one
 *     extends, and see R, G, B.
 *   - Anything else is refused with HDRNET_INVALID_ARGUMENT and a text that names the rule, before any HIP call.  B = 0 is
 *     a no-op (kernel name "noop").
 * A P010 / P016 surface OUT (from a uint16 surface) is include/hdrnet_amd_u16_out.h's; the entry points below keep
 * refusing any other output_kind than the three defined here.
 * Planar surfaces (I420, yuv420p10le / yuv420p16le: three planes) are include/hdrnet_amd_yuv_planar.h's.
 * 4:2:2 surfaces (NV16, P210 / P216) and planar 4:4:4 ones are include/hdrnet_amd_yuv_chroma.h's: these entry points with a
 * `chroma` argument.  The entry points below keep refusing them (H % 2, the UV plane's rows).
 * The pyramid model on these surfaces is include/hdrnet_amd_pyramid_yuv.h's.
 * Out of scope: sited / bilinear chroma, a uint16 RGB frame out of a surface, NV12 in -> P010 / P016 out. */
#ifndef HDRNET_AMD_YUV_H_
#define HDRNET_AMD_YUV_H_

#include "hdrnet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HDRNET_YUV_OUT_RGB_F32 0 /* out: float32 [B][H][W][3] RGB */
#define HDRNET_YUV_OUT_RGB_U8 1  /* out: uint8 [B][H][W][3] RGB = (uint8)(255 * clip(v, 0, 1)) */
#define HDRNET_YUV_OUT_NV12 2    /* out / out_uv: an NV12 uint8 surface with pitches and strides of its own */

/* surface -> float32 [B][H][W][3] RGB (16-byte aligned).  The yardstick of the fused paths, and usable on its own.
 * Kernel name: yuv_to_rgb. */
int hdrnet_yuv_to_rgb_f32(const void* y, const void* uv, int sample_dtype, int pitch_y, int pitch_uv,
                          long long image_stride_y, long long image_stride_uv, int B, int H, int W, const float* to_rgb,
                          float* rgb, void* stream);

/* surface -> lowres [B][n][n][3] float32 (16-byte aligned): the nearest gather of hdrnet_lowres_input -- the same source
 * pixel per output sample -- with the chroma from (y >> 1, x >> 1): the bits of hdrnet_lowres_input on the frame
 * hdrnet_yuv_to_rgb_f32 writes.  Kernel name: sample_prep. */
int hdrnet_lowres_input_yuv(const void* y, const void* uv, int sample_dtype, int pitch_y, int pitch_uv,
                            long long image_stride_y, long long image_stride_uv, int B, int H, int W, const float* to_rgb,
                            float* lowres, int net_input_size, void* stream);

/* hdrnet_bilateral_slice_apply_io_ex for a surface in: grid, guide (or NULL and the guide network), guide_out and flags
 * as there.  output_kind HDRNET_YUV_OUT_RGB_F32 / _RGB_U8: `out` is the frame, the out_* surface arguments and from_rgb
 * are ignored (pass NULL / 0).  HDRNET_YUV_OUT_NV12: `out` is the Y plane and `out_uv` the UV plane of a uint8 surface of
 * the same B, H, W with out_pitch_y, out_pitch_uv, out_image_stride_y, out_image_stride_uv under the rules above, and
 * from_rgb its constants.  Kernel names: apply_fwd_io/<nv12|p016>-><f32|u8|nv12> with the guide suffixes of
 * hdrnet_bilateral_slice_apply_io_ex, e.g. apply_fwd_io/nv12->u8+nnguide. */
int hdrnet_bilateral_slice_apply_io_yuv(const float* grid, const float* guide, const void* y, const void* uv,
                                        int sample_dtype, int pitch_y, int pitch_uv, long long image_stride_y,
                                        long long image_stride_uv, int B, int H, int W, const float* to_rgb, int GH, int GW,
                                        int GD, int Cin, int Cout, int has_offset, const float* guide_conv1,
                                        const float* guide_conv2, int n_feats, float* guide_out, unsigned flags,
                                        int output_kind, void* out, void* out_uv, int out_pitch_y, int out_pitch_uv,
                                        long long out_image_stride_y, long long out_image_stride_uv,
                                        const float* from_rgb, void* stream);

/* hdrnet_bilateral_slice_apply_io_curves_prepared (`prepared` may be NULL: the sorted tables) for a surface in, outputs as
 * above.  Kernel names: e.g. apply_fwd_io/p016->nv12+curvesguide/cells. */
int hdrnet_bilateral_slice_apply_io_curves_yuv(const float* grid, const void* y, const void* uv, int sample_dtype,
                                               int pitch_y, int pitch_uv, long long image_stride_y,
                                               long long image_stride_uv, int B, int H, int W, const float* to_rgb, int GH,
                                               int GW, int GD, int Cin, int Cout, int has_offset, const float* guide_ccm,
                                               const float* guide_shifts, const float* guide_slopes,
                                               const float* guide_mix, int npts, const void* prepared, float* guide_out,
                                               int output_kind, void* out, void* out_uv, int out_pitch_y,
                                               int out_pitch_uv, long long out_image_stride_y,
                                               long long out_image_stride_uv, const float* from_rgb, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* HDRNET_AMD_YUV_H_ */
