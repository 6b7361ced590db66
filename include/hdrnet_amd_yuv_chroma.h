/* YUV 4:2:2 and 4:4:4 surfaces through the wire-format inference path of libhdrnet_amd.so, beside include/hdrnet_amd_yuv.h
 * (semi-planar 4:2:0), include/hdrnet_amd_yuv_planar.h (planar 4:2:0) and include/hdrnet_amd_u16_out.h (P010 / P016 out): what
 * capture cards and mezzanine codecs (10-bit 4:2:2: P210, yuv422p10le), broadcast chains (NV16, yuv422p) and screen capture
 * or intermediate renders (4:4:4) deliver goes through the conversion, the low-res gather and the fused slice-apply forwards
 * without dropping chroma rows and without a float32 frame in between, and a surface of the input's container and chroma
 * layout can come out the same way.  Every entry point below is one of those three headers' with a `chroma` argument (and, for
 * a surface output, `out_bits`).  Dtype codes, flags, return codes, hdrnet_last_error() and hdrnet_last_kernel() are those of
 * hdrnet_amd.h.
 *
 * The rules, the same for every entry point below:
 *   - `chroma`: HDRNET_CHROMA_420, HDRNET_CHROMA_422 or HDRNET_CHROMA_444.  With HDRNET_CHROMA_420 an entry point forwards to
 *     the one it mirrors: its rules, its refusals, its kernel, its kernel name, its bits.
 *   - Surfaces (device pointers; B, H, W with W % 4 == 0 -- a lane owns four pixels -- and, for 4:2:2 and 4:4:4, ANY H: there
 *     is no row pair):
 *       semi-planar 4:2:2   `y` [B][H][W], `uv` [B][H][W] interleaved U, V, full height.  uint8: NV16.  uint16: P210 / P216,
 *                           the code in the HIGH bits, as P010 / P016.
 *       planar 4:2:2        `y` [B][H][W], `u` and `v` [B][H][W/2].  uint8: yuv422p.  uint16: yuv422p10le / yuv422p16le, the code
 *                           in the LOW bits.
 *       planar 4:4:4        `y`, `u` and `v` [B][H][W].  uint8: yuv444p.  uint16: yuv444p10le / yuv444p16le, low bits.
 *     Semi-planar 4:4:4 (NV24, P410) is refused, with a text that says so.
 *   - Pitches (bytes per row, at least the row's samples), image strides (bytes between the images of a batch, non-negative,
 *     for B > 1 at least pitch * rows -- a chroma plane of these layouts has H rows), padding that is never read and never
 *     written, and B = 0 as a no-op (kernel name "noop") are as in hdrnet_amd_yuv.h and hdrnet_amd_yuv_planar.h.
 *   - Alignment follows the samples a lane touches per row.  The Y plane, the NV16 / P210 `uv` plane and a 4:4:4 chroma plane
 *     hold four samples per lane: base, pitch and image stride are multiples of 4.  A 4:2:2 planar chroma plane holds two: 2
 *     bytes for uint8 samples, 4 bytes for uint16 -- the 4:2:0 planar rule, which admits tight planes (W = 100: a tight uint8
 *     chroma row is 50 bytes).
 *   - Chroma is REPLICATED, as it is for 4:2:0: for 4:2:2, chroma sample (y, x >> 1) serves pixels (y, 2 (x >> 1)) and
 *     (y, 2 (x >> 1) + 1); for 4:4:4, chroma sample (y, x) serves pixel (y, x).
 *   - The 12 floats `to_rgb` / `from_rgb` (hdrnet_amd.yuv.yuv_coefficients / yuv_encode_coefficients) are used as they are: the
 *     chroma layout does not enter the colour constants.  Conversion in is hdrnet_amd_yuv.h's one function, unchanged:
 *         c_i = fmed3(fmaf(m_i2, V, fmaf(m_i1, U, fmaf(m_i0, Y, bias_i))), 0, 1)        i = R, G, B
 *     Only which chroma sample a pixel reads differs.
 *   - Conversion out keeps the rule of hdrnet_amd_yuv.h: luma per pixel; with l_i the linear chroma term of a pixel, the sum
 *     over the chroma sample's footprint in a fixed order, scaled by the reciprocal of the footprint size in the fmaf that
 *     adds the bias:
 *         4:2:0 (unchanged)   s = (l(2j,2k) + l(2j,2k+1)) + (l(2j+1,2k) + l(2j+1,2k+1)),   w = 0.25
 *         4:2:2               s = l(y,2k) + l(y,2k+1),                                      w = 0.5
 *         4:4:4               s = l(y,x),                                                   w = 1
 *         code = (T) fmed3(fmaf(s, w, bias_i), 0, code_max) << shift
 *     with code_max = 2^out_bits - 1 and shift = 16 - out_bits for a semi-planar uint16 surface, 0 otherwise.
 *   - Outputs, `output_kind`: HDRNET_CHROMA_OUT_RGB_F32, HDRNET_CHROMA_OUT_RGB_U8, or a surface of the INPUT's container and
 *     chroma layout, B, H, W:
 *       semi-planar   HDRNET_CHROMA_OUT_SURFACE_U8 (NV16; out_bits ignored) from either sample width, as NV12 is;
 *                     HDRNET_CHROMA_OUT_SURFACE_U16 (P210 / P216: out_bits 10 or 16, in the high bits) from a uint16 surface.
 *       planar        of the input's sample dtype and depth: HDRNET_CHROMA_OUT_SURFACE_U8 with out_bits 8 from uint8 planes,
 *                     HDRNET_CHROMA_OUT_SURFACE_U16 with out_bits 10 or 16 from uint16 planes.
 *   - The op is Cin = Cout = 3 with offset; the grid and every guide parameter are those of the entry point each one mirrors.
 *   - Anything else is refused with HDRNET_INVALID_ARGUMENT and a text that names the rule, before any HIP call.
 * Kernel names state container, layout and sample width: nv16 / p216 (semi-planar 4:2:2, uint8 / uint16), i422 / i216 (planar
 * 4:2:2), i444 / i416 (planar 4:4:4) -- e.g. apply_fwd_io/nv16->nv16+nnguide, apply_fwd_io/p216->u8, apply_fwd_io/i422->i422,
 * apply_fwd_io/i444->f32+curvesguide/cells, apply_fwd_io/i416->i416.
 * (The entry points of include/hdrnet_amd_yuv_packed.h read and write the semi-planar 4:2:2 surface with its two planes woven
 * into one, under these rules.)
 * Out of scope: packed 4:2:2 / 4:4:4 (YUY2, UYVY, Y210, AYUV, Y410), semi-planar 4:4:4 (NV24, P410), 12-bit depth, sited or
 * bilinear chroma, a surface out in another container, chroma layout or (planar) sample width than the input's, the pyramid
 * model. */
#ifndef HDRNET_AMD_YUV_CHROMA_H_
#define HDRNET_AMD_YUV_CHROMA_H_

#include "hdrnet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HDRNET_CHROMA_420 0 /* chroma sample (y >> 1, x >> 1): the layout of the three headers above */
#define HDRNET_CHROMA_422 1 /* chroma sample (y, x >> 1) */
#define HDRNET_CHROMA_444 2 /* chroma sample (y, x): planar surfaces only */

#define HDRNET_CHROMA_OUT_RGB_F32 0     /* out: float32 [B][H][W][3] RGB (16-byte aligned) */
#define HDRNET_CHROMA_OUT_RGB_U8 1      /* out: uint8 [B][H][W][3] RGB = (uint8)(255 * clip(v, 0, 1)) (4-byte aligned) */
#define HDRNET_CHROMA_OUT_SURFACE_U8 2  /* a uint8 surface of the input's container and chroma layout */
#define HDRNET_CHROMA_OUT_SURFACE_U16 3 /* a uint16 surface of the input's container and chroma layout, out_bits deep */

/* ---- semi-planar surfaces: hdrnet_amd_yuv.h / hdrnet_amd_u16_out.h with `chroma` (HDRNET_CHROMA_420 or _422) ------------------ */

/* hdrnet_yuv_to_rgb_f32.  Kernel name: yuv_422_to_rgb. */
int hdrnet_yuv_chroma_to_rgb_f32(const void* y, const void* uv, int sample_dtype, int pitch_y, int pitch_uv,
                                 long long image_stride_y, long long image_stride_uv, int chroma, int B, int H, int W,
                                 const float* to_rgb, float* rgb, void* stream);

/* hdrnet_lowres_input_yuv.  Kernel name: sample_prep. */
int hdrnet_lowres_input_yuv_chroma(const void* y, const void* uv, int sample_dtype, int pitch_y, int pitch_uv,
                                   long long image_stride_y, long long image_stride_uv, int chroma, int B, int H, int W,
                                   const float* to_rgb, float* lowres, int net_input_size, void* stream);

/* hdrnet_bilateral_slice_apply_io_yuv / ..._yuv_p016.  An RGB output: `out` is the frame; out_uv, the out_* pitches and
 * strides, from_rgb and out_bits are ignored (pass NULL / 0). */
int hdrnet_bilateral_slice_apply_io_yuv_chroma(const float* grid, const float* guide, const void* y, const void* uv,
                                               int sample_dtype, int pitch_y, int pitch_uv, long long image_stride_y,
                                               long long image_stride_uv, int chroma, int B, int H, int W,
                                               const float* to_rgb, int GH, int GW, int GD, int Cin, int Cout,
                                               int has_offset, const float* guide_conv1, const float* guide_conv2,
                                               int n_feats, float* guide_out, unsigned flags, int output_kind, void* out,
                                               void* out_uv, int out_pitch_y, int out_pitch_uv,
                                               long long out_image_stride_y, long long out_image_stride_uv,
                                               const float* from_rgb, int out_bits, void* stream);

/* hdrnet_bilateral_slice_apply_io_curves_yuv / ..._curves_yuv_p016 (`prepared` may be NULL: the sorted tables). */
int hdrnet_bilateral_slice_apply_io_curves_yuv_chroma(const float* grid, const void* y, const void* uv, int sample_dtype,
                                                      int pitch_y, int pitch_uv, long long image_stride_y,
                                                      long long image_stride_uv, int chroma, int B, int H, int W,
                                                      const float* to_rgb, int GH, int GW, int GD, int Cin, int Cout,
                                                      int has_offset, const float* guide_ccm, const float* guide_shifts,
                                                      const float* guide_slopes, const float* guide_mix, int npts,
                                                      const void* prepared, float* guide_out, int output_kind, void* out,
                                                      void* out_uv, int out_pitch_y, int out_pitch_uv,
                                                      long long out_image_stride_y, long long out_image_stride_uv,
                                                      const float* from_rgb, int out_bits, void* stream);

/* ---- planar surfaces: hdrnet_amd_yuv_planar.h with `chroma` (HDRNET_CHROMA_420, _422 or _444) ---------------------------------- */

/* hdrnet_yuv_planar_to_rgb_f32.  Kernel names: yuv_planar_422_to_rgb, yuv_planar_444_to_rgb. */
int hdrnet_yuv_planar_chroma_to_rgb_f32(const void* y, const void* u, const void* v, int sample_dtype, int pitch_y,
                                        int pitch_u, int pitch_v, long long image_stride_y, long long image_stride_u,
                                        long long image_stride_v, int chroma, int B, int H, int W, const float* to_rgb,
                                        float* rgb, void* stream);

/* hdrnet_lowres_input_yuv_planar.  Kernel name: sample_prep. */
int hdrnet_lowres_input_yuv_planar_chroma(const void* y, const void* u, const void* v, int sample_dtype, int pitch_y,
                                          int pitch_u, int pitch_v, long long image_stride_y, long long image_stride_u,
                                          long long image_stride_v, int chroma, int B, int H, int W, const float* to_rgb,
                                          float* lowres, int net_input_size, void* stream);

/* hdrnet_bilateral_slice_apply_io_yuv_planar.  An RGB output: `out` is the frame; out_u, out_v, the out_* pitches and strides,
 * from_rgb and out_bits are ignored (pass NULL / 0). */
int hdrnet_bilateral_slice_apply_io_yuv_planar_chroma(const float* grid, const float* guide, const void* y, const void* u,
                                                      const void* v, int sample_dtype, int pitch_y, int pitch_u,
                                                      int pitch_v, long long image_stride_y, long long image_stride_u,
                                                      long long image_stride_v, int chroma, int B, int H, int W,
                                                      const float* to_rgb, int GH, int GW, int GD, int Cin, int Cout,
                                                      int has_offset, const float* guide_conv1, const float* guide_conv2,
                                                      int n_feats, float* guide_out, unsigned flags, int output_kind,
                                                      void* out, void* out_u, void* out_v, int out_pitch_y, int out_pitch_u,
                                                      int out_pitch_v, long long out_image_stride_y,
                                                      long long out_image_stride_u, long long out_image_stride_v,
                                                      const float* from_rgb, int out_bits, void* stream);

/* hdrnet_bilateral_slice_apply_io_curves_yuv_planar (`prepared` may be NULL: the sorted tables). */
int hdrnet_bilateral_slice_apply_io_curves_yuv_planar_chroma(const float* grid, const void* y, const void* u, const void* v,
                                                             int sample_dtype, int pitch_y, int pitch_u, int pitch_v,
                                                             long long image_stride_y, long long image_stride_u,
                                                             long long image_stride_v, int chroma, int B, int H, int W,
                                                             const float* to_rgb, int GH, int GW, int GD, int Cin, int Cout,
                                                             int has_offset, const float* guide_ccm,
                                                             const float* guide_shifts, const float* guide_slopes,
                                                             const float* guide_mix, int npts, const void* prepared,
                                                             float* guide_out, int output_kind, void* out, void* out_u,
                                                             void* out_v, int out_pitch_y, int out_pitch_u, int out_pitch_v,
                                                             long long out_image_stride_y, long long out_image_stride_u,
                                                             long long out_image_stride_v, const float* from_rgb,
                                                             int out_bits, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* HDRNET_AMD_YUV_CHROMA_H_ */
