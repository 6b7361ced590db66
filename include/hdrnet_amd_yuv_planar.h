/* Planar YUV 4:2:0 surfaces through the wire-format inference path of libhdrnet_amd.so, beside include/hdrnet_amd_yuv.h
 * (semi-planar surfaces) and include/hdrnet_amd_u16_out.h: what SOFTWARE decoders and raw .yuv / .y4m files deliver -- I420
 * (FFmpeg's yuv420p: three uint8 planes) and yuv420p10le / yuv420p16le (three uint16 planes, the code in the LOW bits) --
 * goes through the low-res gather and the fused slice-apply forwards without an interleaving or shifting pass, and a
 * planar surface of the same sample width can come out the same way.  Dtype codes, flags, return codes,
 * hdrnet_last_error() and hdrnet_last_kernel() are those of hdrnet_amd.h.
 *
 * The rules, the same for every entry point below:
 *   - A planar surface is `y` [B][H][W], `u` [B][H/2][W/2] and `v` [B][H/2][W/2] (device pointers), each plane with its own
 *     row pitch (`pitch_y`, `pitch_u`, `pitch_v`: bytes per row, at least the row's bytes -- W samples of luma, W / 2 of
 *     chroma) and image stride (`image_stride_y`, `image_stride_u`, `image_stride_v`: bytes between the images of a batch,
 *     non-negative, and for B > 1 at least the plane: pitch_y * H, pitch_u * H / 2, pitch_v * H / 2), and B, H, W with
 *     H % 2 == 0 and W % 4 == 0.  YV12 is the same surface with the caller passing the planes in the other order.
 *   - `sample_dtype` (the codes of hdrnet_amd.h): 1 uint8 (I420), 2 uint16 (yuv420p10le / yuv420p16le).  A 16-bit sample
 *     carries its code in the LOW bits; the kernels see "the sample as stored", as everywhere else.
 *   - Alignment.  The Y plane follows hdrnet_amd_yuv.h: base, pitch and image stride are multiples of 4.  A chroma plane
 *     holds W / 2 samples per row and a lane touches 2 of them: base, pitch and image stride are multiples of 2 for uint8
 *     samples and of 4 for uint16 samples.  This admits tight planes as torch and FFmpeg allocate them (W = 100: a tight
 *     uint8 chroma row is 50 bytes, so every other row starts 2 bytes past a dword boundary).  Padding beyond a row's
 *     samples is never read as pixels and never written.
 *   - Chroma is REPLICATED, as for NV12: chroma sample (y >> 1, x >> 1) serves its 2 x 2 block.
 *   - The kernels apply 12 floats, `to_rgb` / `from_rgb` (device pointers, 4-byte aligned): a row-major 3 x 3 matrix, then 3
 *     biases.  Conversion in is hdrnet_amd_yuv.h's one function on the samples as stored, unchanged:
 *         c_i = fmed3(fmaf(m_i2, V, fmaf(m_i1, U, fmaf(m_i0, Y, bias_i))), 0, 1)        i = R, G, B
 *     hdrnet_amd.yuv.yuv_coefficients(standard, full_range, bits, msb_aligned=False) computes `to_rgb` for codes in the low
 *     bits (for bits = 10 its matrix is exactly 64 x the P010 one and the biases are equal).
 *   - Conversion out (HDRNET_YUV_PLANAR_OUT_PLANAR) is the rule of hdrnet_amd_yuv.h / hdrnet_amd_u16_out.h, with the same
 *     row-pair sums in the same order (horizontal pair first, even row then odd row, x 0.25, + bias): `from_rgb` is in code
 *     units of `out_bits` bits (hdrnet_amd.yuv.yuv_encode_coefficients), codes are clamped to 2^out_bits - 1, truncated and
 *     stored with shift 0, U codes into the `out_u` plane and V codes into the `out_v` plane.  So a planar surface and the
 *     semi-planar surface with the same samples give the same codes (P010's shifted up by 6).
 *   - Outputs, `output_kind`: a float32 RGB frame, a uint8 RGB frame, or a planar surface of the INPUT's sample dtype with
 *     `out_bits` 8 for uint8 samples and 10 or 16 for uint16 samples.
 *   - The op is Cin = Cout = 3 with offset; the grid and every guide parameter are those of the entry point each one
 *     extends, and see R, G, B.
 *   - Anything else is refused with HDRNET_INVALID_ARGUMENT and a text that names the rule, before any HIP call.  B = 0 is
 *     a no-op (kernel name "noop").
 * 4:2:2 and 4:4:4 planar surfaces (yuv422p..., yuv444p...) are include/hdrnet_amd_yuv_chroma.h's: these entry points with a
 * `chroma` argument.  The entry points below keep refusing them.
 * Out of scope: 12-bit depth, sited or bilinear chroma, uint16 planar in -> uint8 planar out, planar in -> semi-planar out
 * and semi-planar in -> planar out.  The pyramid model on these surfaces is include/hdrnet_amd_pyramid_yuv.h's. */
#ifndef HDRNET_AMD_YUV_PLANAR_H_
#define HDRNET_AMD_YUV_PLANAR_H_

#include "hdrnet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HDRNET_YUV_PLANAR_OUT_RGB_F32 0 /* out: float32 [B][H][W][3] RGB (16-byte aligned) */
#define HDRNET_YUV_PLANAR_OUT_RGB_U8 1  /* out: uint8 [B][H][W][3] RGB = (uint8)(255 * clip(v, 0, 1)) (4-byte aligned) */
#define HDRNET_YUV_PLANAR_OUT_PLANAR 2  /* out / out_u / out_v: a planar surface of the input's sample dtype */

/* planar surface -> float32 [B][H][W][3] RGB (16-byte aligned): the bits of hdrnet_yuv_to_rgb_f32 on the interleaved
 * surface.  Kernel name: yuv_planar_to_rgb. */
int hdrnet_yuv_planar_to_rgb_f32(const void* y, const void* u, const void* v, int sample_dtype, int pitch_y, int pitch_u,
                                 int pitch_v, long long image_stride_y, long long image_stride_u,
                                 long long image_stride_v, int B, int H, int W, const float* to_rgb, float* rgb,
                                 void* stream);

/* planar surface -> lowres [B][n][n][3] float32 (16-byte aligned): hdrnet_lowres_input_yuv with the chroma of a pixel from
 * (y >> 1, x >> 1) of the two chroma planes.  Kernel name: sample_prep. */
int hdrnet_lowres_input_yuv_planar(const void* y, const void* u, const void* v, int sample_dtype, int pitch_y, int pitch_u,
                                   int pitch_v, long long image_stride_y, long long image_stride_u,
                                   long long image_stride_v, int B, int H, int W, const float* to_rgb, float* lowres,
                                   int net_input_size, void* stream);

/* hdrnet_bilateral_slice_apply_io_yuv for a planar surface in: grid, guide (or NULL and the guide network), guide_out and
 * flags as there.  output_kind HDRNET_YUV_PLANAR_OUT_RGB_F32 / _RGB_U8: `out` is the frame; out_u, out_v, the out_*
 * pitches and strides, from_rgb and out_bits are ignored (pass NULL / 0).  HDRNET_YUV_PLANAR_OUT_PLANAR: `out`, `out_u`,
 * `out_v` are the planes of a surface of the same sample dtype and B, H, W under the rules above, `from_rgb` its constants
 * and `out_bits` the depth of its codes.  Kernel names: apply_fwd_io/<i420|i016>-><f32|u8|i420|i016> with the guide
 * suffixes of hdrnet_bilateral_slice_apply_io_ex, e.g. apply_fwd_io/i420->i420+nnguide; the label states the sample width
 * (i420: uint8, i016: uint16), not the bit depth. */
int hdrnet_bilateral_slice_apply_io_yuv_planar(const float* grid, const float* guide, const void* y, const void* u,
                                               const void* v, int sample_dtype, int pitch_y, int pitch_u, int pitch_v,
                                               long long image_stride_y, long long image_stride_u,
                                               long long image_stride_v, int B, int H, int W, const float* to_rgb, int GH,
                                               int GW, int GD, int Cin, int Cout, int has_offset,
                                               const float* guide_conv1, const float* guide_conv2, int n_feats,
                                               float* guide_out, unsigned flags, int output_kind, void* out, void* out_u,
                                               void* out_v, int out_pitch_y, int out_pitch_u, int out_pitch_v,
                                               long long out_image_stride_y, long long out_image_stride_u,
                                               long long out_image_stride_v, const float* from_rgb, int out_bits,
                                               void* stream);

/* hdrnet_bilateral_slice_apply_io_curves_yuv (`prepared` may be NULL: the sorted tables) for a planar surface in, outputs
 * as above.  Kernel names: e.g. apply_fwd_io/i016->i016+curvesguide/cells. */
int hdrnet_bilateral_slice_apply_io_curves_yuv_planar(const float* grid, const void* y, const void* u, const void* v,
                                                      int sample_dtype, int pitch_y, int pitch_u, int pitch_v,
                                                      long long image_stride_y, long long image_stride_u,
                                                      long long image_stride_v, int B, int H, int W, const float* to_rgb,
                                                      int GH, int GW, int GD, int Cin, int Cout, int has_offset,
                                                      const float* guide_ccm, const float* guide_shifts,
                                                      const float* guide_slopes, const float* guide_mix, int npts,
                                                      const void* prepared, float* guide_out, int output_kind, void* out,
                                                      void* out_u, void* out_v, int out_pitch_y, int out_pitch_u,
                                                      int out_pitch_v, long long out_image_stride_y,
                                                      long long out_image_stride_u, long long out_image_stride_v,
                                                      const float* from_rgb, int out_bits, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* HDRNET_AMD_YUV_PLANAR_H_ */
