/* The pyramid model (HDRNetGaussianPyrNN, hdrnet/models.py:213-289) on YUV 4:2:0 video surfaces, beside
 * include/hdrnet_amd_pyramid_io.h (its uint8 / uint16 RGB frames) and include/hdrnet_amd_yuv.h, hdrnet_amd_u16_out.h,
 * hdrnet_amd_yuv_planar.h (the single-level models' surfaces): the two launches the pyramid's inference was missing to
 * take an NV12 / P010 / P016 / I420 / yuv420p10le / yuv420p16le surface in and give a frame or a surface of the same
 * container out WITHOUT an RGB frame in memory -- the resize that builds level 1 from the surface, and the finest level's
 * slice-apply + up-add with the surface load and store of the single-level forwards.  The launch sequence is
 * hdrnet_amd_pyramid_io.h's with these two in place of its two:
 *     lowres = hdrnet_lowres_input_yuv[_planar](surface)            grids = hdrnet_coefficients_f32(lowres)
 *     l1 = hdrnet_resize_bilinear_yuv[_planar](surface -> H/2 x W/2)        l2 = hdrnet_resize_bilinear_f32(l1 -> H/4 x W/4)
 *     cur = ..._nnguide_f32_ex(grids[0], l2);  cur = ..._upadd_f32_ex(grids[1], l1, cur)
 *     out = hdrnet_bilateral_slice_apply_upadd_io_yuv[_p016 | _planar](grids[2], surface, cur)
 *
 * The rules:
 *   - A surface, its constants (`to_rgb`, `from_rgb`), the conversion in, the encode out, alignment, pitches and image
 *     strides are those of hdrnet_amd_yuv.h (semi-planar), hdrnet_amd_u16_out.h (a P010 / P016 surface out) and
 *     hdrnet_amd_yuv_planar.h (planar), unchanged: H % 2 == 0, W % 4 == 0, replicated chroma.
 *   - The resize is hdrnet_resize_bilinear_f32's arithmetic, tap for tap, on the frame hdrnet_yuv_to_rgb_f32 /
 *     hdrnet_yuv_planar_to_rgb_f32 writes: each of the four taps is a converted pixel -- luma (row, x), chroma (row >> 1,
 *     x >> 1), clamped to [0, 1] BEFORE the blend.
 *   - The finest level: out = wire_out(bilateral_slice_apply(grid, guide, to_rgb(surface)) + resize_bilinear(coarse -> H x W))
 *     with coarse [B][Hc][Wc][3] float32 (4-byte aligned), Hc, Wc >= 1.  The clip of a uint8 frame, the luma code and the
 *     2 x 2 chroma sums of a surface all see the value AFTER the add.  Cin = Cout = 3 with offset.
 *   - The guide is EITHER a [B][H][W] map OR the folded guide network (guide_conv1 [n][4], guide_conv2 [n + 1], n_feats), never
 *     both; flags: HDRNET_GUIDE_SIGMOID_FAST, HDRNET_GUIDE_RELU_PRESCALED (guide network only).  The curves guide belongs to
 *     the single-level models: there is no entry point for it here.  There is no guide_out.
 *   - Input -> output: NV12 -> float32 RGB, uint8 RGB, NV12;  P010 / P016 -> float32 RGB, uint8 RGB, NV12, and (..._p016)
 *     P010 / P016;  I420 -> float32 RGB, uint8 RGB, I420;  uint16 planar -> float32 RGB, uint8 RGB, uint16 planar.
 *   - Anything else is refused with HDRNET_INVALID_ARGUMENT and a text that names the rule, before any HIP call.
 *     B * H * W == 0 (the resize: an empty output) is a no-op (kernel name "noop").
 * Out of scope: 4:2:2 / 4:4:4 surfaces, a uint16 RGB frame out, BGR / RGBA frames, the curves guide, training. */
#ifndef HDRNET_AMD_PYRAMID_YUV_H_
#define HDRNET_AMD_PYRAMID_YUV_H_

#include "hdrnet_amd.h"
#include "hdrnet_amd_u16_out.h"
#include "hdrnet_amd_yuv.h"
#include "hdrnet_amd_yuv_planar.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out [B][Hout][Wout][3] float32 (4-byte aligned) = resize_bilinear(hdrnet_yuv_to_rgb_f32(surface)), align_corners = true.
 * The surface is [B][H][W] under the rules of hdrnet_amd_yuv.h; any Hout, Wout >= 0, an empty output is a no-op.  Stores are
 * 16 bytes wide when Wout % 4 == 0 and `out` is 16-byte aligned, scalar otherwise.  Kernel names: resize_bilinear_yuv/nv12
 * (uint8 samples), /p016 (uint16). */
int hdrnet_resize_bilinear_yuv(const void* y, const void* uv, int sample_dtype, int pitch_y, int pitch_uv,
                               long long image_stride_y, long long image_stride_uv, int B, int H, int W, const float* to_rgb,
                               float* out, int Hout, int Wout, void* stream);

/* ... of a planar surface (hdrnet_amd_yuv_planar.h): the bits of hdrnet_resize_bilinear_yuv on the interleaved surface.
 * Kernel names: resize_bilinear_yuv/i420 (uint8 samples), /i016 (uint16). */
int hdrnet_resize_bilinear_yuv_planar(const void* y, const void* u, const void* v, int sample_dtype, int pitch_y, int pitch_u,
                                      int pitch_v, long long image_stride_y, long long image_stride_u,
                                      long long image_stride_v, int B, int H, int W, const float* to_rgb, float* out,
                                      int Hout, int Wout, void* stream);

/* hdrnet_bilateral_slice_apply_io_yuv + the up-add of `coarse`: its argument list with coarse, Hc, Wc after to_rgb and
 * without guide_out; output_kind HDRNET_YUV_OUT_RGB_F32 / _RGB_U8 / _NV12 and the output arguments as there.  Kernel names:
 * apply_fwd_io/<nv12|p016>-><f32|u8|nv12>[+nnguide]+upadd, e.g. apply_fwd_io/nv12->nv12+nnguide+upadd. */
int hdrnet_bilateral_slice_apply_upadd_io_yuv(const float* grid, const float* guide, const void* y, const void* uv,
                                              int sample_dtype, int pitch_y, int pitch_uv, long long image_stride_y,
                                              long long image_stride_uv, int B, int H, int W, const float* to_rgb,
                                              const float* coarse, int Hc, int Wc, int GH, int GW, int GD, int Cin, int Cout,
                                              int has_offset, const float* guide_conv1, const float* guide_conv2, int n_feats,
                                              unsigned flags, int output_kind, void* out, void* out_uv, int out_pitch_y,
                                              int out_pitch_uv, long long out_image_stride_y, long long out_image_stride_uv,
                                              const float* from_rgb, void* stream);

/* hdrnet_bilateral_slice_apply_io_yuv_p016 + the up-add, changed the same way: a uint16 surface in (sample_dtype 2), a
 * P010 / P016 surface of `out_bits` (10 or 16) out.  Kernel names: apply_fwd_io/p016->p016[+nnguide]+upadd. */
int hdrnet_bilateral_slice_apply_upadd_io_yuv_p016(const float* grid, const float* guide, const void* y, const void* uv,
                                                   int sample_dtype, int pitch_y, int pitch_uv, long long image_stride_y,
                                                   long long image_stride_uv, int B, int H, int W, const float* to_rgb,
                                                   const float* coarse, int Hc, int Wc, int GH, int GW, int GD, int Cin,
                                                   int Cout, int has_offset, const float* guide_conv1,
                                                   const float* guide_conv2, int n_feats, unsigned flags, void* out_y,
                                                   void* out_uv, int out_pitch_y, int out_pitch_uv,
                                                   long long out_image_stride_y, long long out_image_stride_uv,
                                                   const float* from_rgb, int out_bits, void* stream);

/* hdrnet_bilateral_slice_apply_io_yuv_planar + the up-add, changed the same way; output_kind HDRNET_YUV_PLANAR_OUT_* and
 * the output arguments as there.  Kernel names: apply_fwd_io/<i420|i016>-><f32|u8|i420|i016>[+nnguide]+upadd. */
int hdrnet_bilateral_slice_apply_upadd_io_yuv_planar(const float* grid, const float* guide, const void* y, const void* u,
                                                     const void* v, int sample_dtype, int pitch_y, int pitch_u, int pitch_v,
                                                     long long image_stride_y, long long image_stride_u,
                                                     long long image_stride_v, int B, int H, int W, const float* to_rgb,
                                                     const float* coarse, int Hc, int Wc, int GH, int GW, int GD, int Cin,
                                                     int Cout, int has_offset, const float* guide_conv1,
                                                     const float* guide_conv2, int n_feats, unsigned flags, int output_kind,
                                                     void* out, void* out_u, void* out_v, int out_pitch_y, int out_pitch_u,
                                                     int out_pitch_v, long long out_image_stride_y,
                                                     long long out_image_stride_u, long long out_image_stride_v,
                                                     const float* from_rgb, int out_bits, void* stream);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* HDRNET_AMD_PYRAMID_YUV_H_ */
