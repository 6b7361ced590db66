// Argument bundles and launcher prototypes shared by the kernel translation
// units and the C-ABI front-end (capi.hip).  All pointers are device pointers in
// the layouts documented in include/hdrnet_amd.h.
#pragma once

#include <hip/hip_runtime.h>

#include <stddef.h>

#include "../../include/hdrnet_amd.h"
#include "../../include/hdrnet_amd_train.h"
#include "coeff_fc_train.hip.h"
#include "row_geom.h"
#include "yuv_convert.hip.h"

namespace hdrnet_amd {

struct ApplyArgs {
  const float* grid;
  const float* guide;
  const float* input;
  float* out;
  int B, H, W, GH, GW, GD, Cin, Cout, Cj;  // Cj = Cin + has_offset
  bool has_offset;
  int variant;  // 0 = library default; >0 selects a kernel variant (flags bits 8..15)
  // Row-split launch (hdrnet_bilateral_slice_apply_rows_f32): the buffers hold rows y0 .. y0 + H - 1 of a
  // frame that is H_total rows high; gyf = (y0 + y + .5) * GH / H_total (bilateral_slice_apply.cc:38,42).
  // H_total = 0: a whole frame (H_total = H, y0 = 0).
  int y0 = 0, H_total = 0;
  int frame_rows() const { return H_total > 0 ? H_total : H; }
  // fused guide network: v_exp_f32 + v_rcp_f32 sigmoid (HDRNET_GUIDE_SIGMOID_FAST) instead of expf + IEEE divide
  bool fast_sigmoid = false;
  // fused guide network: conv1 / conv2 are the PRESCALED arrays of hdrnet_guide_nn_prescale_f32 (HDRNET_GUIDE_RELU_PRESCALED)
  bool guide_prescaled = false;
};

// Forward with wire-format conversion and / or the fused guide network (apply_fwd_io.hip).
struct ApplyIoArgs {
  const float* grid;
  const float* guide;  // null => guide network (guide_conv1 / guide_conv2)
  const void* input;   // input_dtype: 0 f32, 1 u8, 2 u16; value / white_level
  void* out;           // output_dtype: 0 f32, 1 u8 = (uint8)(255 * clip(v, 0, 1)),
                       //   2 u16 = (uint16)(output_white_level * clip(v, 0, 1)) (apply_fwd_io_u16.hip only)
  int B, H, W, GH, GW, GD, Cin, Cout;
  bool has_offset;
  int input_dtype, output_dtype;
  float white_level;
  const float* guide_conv1;  // NN: conv1 [n][Cin+1]; curves: ccm [Cin][Cin+1]
  const float* guide_conv2;  // NN: conv2 [n+1];      curves: mix [Cin+1]
  int n_feats;               // NN: features;         curves: knots per channel
  float* guide_out;  // optional
  const float* guide_shifts = nullptr;  // non-null selects the curves guide: [n][Cin]
  const float* guide_slopes = nullptr;  //                                    [n][Cin]
  bool fast_sigmoid = false;            // guide network: as ApplyArgs::fast_sigmoid
  bool guide_prescaled = false;         // guide network: as ApplyArgs::guide_prescaled
  const float* guide_prepared = nullptr;  // curves guide: the cell tables of hdrnet_curves_guide_prepare_f32, or null
  // how `input` stores a pixel, HDRNET_PX_* (include/hdrnet_amd_pixel_formats.h): 0 RGB, 1 BGR, 2 RGBA, 3 BGRA; a uint8
  // `out` has the same format, a float32 one is RGB.  Cin / Cout stay the op's 3 whatever the format (apply_fwd_io.hip only)
  int pixel_format = 0;
  // a semi-planar YUV surface in place of `input` (include/hdrnet_amd_yuv.h; apply_fwd_io_yuv.hip): input_dtype is then the
  // surface's sample dtype (1 u8 = NV12, 2 u16 = P010 / P016), `input` is unused, and `out` is the RGB frame of
  // output_dtype -- or, with yuv->out_kind == HDRNET_YUV_OUT_NV12 (output_dtype = 1), unused too
  const struct YuvIo* yuv = nullptr;
  // ... or a PLANAR one (include/hdrnet_amd_yuv_planar.h; apply_fwd_io_yuv_planar.hip): input_dtype is the sample dtype
  // (1 u8 = I420, 2 u16), `out` the RGB frame of output_dtype -- or, with yuvp->out_kind == kYuvPlanarOutPlanar
  // (output_dtype = input_dtype), unused
  const struct YuvPlanarIo* yuvp = nullptr;
  // ... or a PACKED 4:2:2 one (include/hdrnet_amd_yuv_packed.h; apply_fwd_io_yuv_packed.hip): input_dtype is the sample dtype
  // (1 u8 = YUY2 / UYVY / YVYU, 2 u16 = Y210 / Y216), `out` the RGB frame of output_dtype -- or, with a surface output
  // (output_dtype = input_dtype), unused
  const struct YuvPackedIo* yuvk = nullptr;
  // output_dtype == 2 (include/hdrnet_amd_u16_out.h): the white level of the uint16 frame, which has the input's pixel format
  float output_white_level = 0.0f;
};

// YuvIo::out_kind beyond the HDRNET_YUV_OUT_* codes, which hdrnet_amd_yuv.h's entry points refuse: a P010 / P016 surface
// out (include/hdrnet_amd_u16_out.h; output_dtype = 2, YuvIo::out_bits)
constexpr int kYuvOutP016 = 3;

struct YuvIo {
  YuvSurface in;
  const float* to_rgb;    // device, 12 floats
  int out_kind;           // HDRNET_YUV_OUT_*, or kYuvOutP016
  YuvSurface out;         // out_kind == HDRNET_YUV_OUT_NV12 / kYuvOutP016
  const float* from_rgb;  // device, 12 floats
  int out_bits = 0;       // kYuvOutP016: 10 or 16 significant bits per sample, in the high bits
  int chroma = kChroma420;  // both surfaces' chroma layout (include/hdrnet_amd_yuv_chroma.h): kChroma420 / kChroma422
};

// The planar counterpart (include/hdrnet_amd_yuv_planar.h): out_kind is HDRNET_YUV_PLANAR_OUT_* -- a float32 / uint8 RGB
// frame, or a planar surface of the input's sample dtype
constexpr int kYuvPlanarOutPlanar = 2;

struct YuvPlanarIo {
  YuvPlanarSurface in;
  const float* to_rgb;    // device, 12 floats
  int out_kind;           // HDRNET_YUV_PLANAR_OUT_*
  YuvPlanarSurface out;   // out_kind == kYuvPlanarOutPlanar
  const float* from_rgb;  // device, 12 floats
  int out_bits = 0;       // kYuvPlanarOutPlanar: 8 (uint8 samples), 10 or 16 (uint16): the code's bits, in the LOW bits
  int chroma = kChroma420;  // both surfaces' chroma layout (include/hdrnet_amd_yuv_chroma.h): kChroma420 / 422 / 444
};

// The packed 4:2:2 counterpart (include/hdrnet_amd_yuv_packed.h): out_kind is HDRNET_CHROMA_OUT_* -- a float32 / uint8 RGB
// frame, or a packed surface of the input's sample width and order
struct YuvPackedIo {
  YuvPackedSurface in;
  const float* to_rgb;    // device, 12 floats
  int out_kind;           // HDRNET_CHROMA_OUT_*
  YuvPackedSurface out;   // out_kind == HDRNET_CHROMA_OUT_SURFACE_U8 / _U16
  const float* from_rgb;  // device, 12 floats
  int out_bits = 0;       // HDRNET_CHROMA_OUT_SURFACE_U16: 10 (Y210) or 16 (Y216) significant bits, in the high bits
};

// Gradients of BilateralSliceApply, and of BilateralSlice as the apply op without an input: slice = true,
// input = dinput = null, Cin = 0, Cout = C, Cj = 1.  The tag, not the channel counts, says which op it is: the apply
// entry point itself takes Cin = 0 with offset, and the two ops differ in fast shapes, generic kernel and kernel names.
struct ApplyGradArgs {
  const float* grid;
  const float* guide;
  const float* input;
  const float* dout;
  float* dgrid;   // may be null
  float* dguide;  // may be null
  float* dinput;  // may be null
  int B, H, W, GH, GW, GD, Cin, Cout, Cj;
  bool has_offset;
  void* workspace;
  size_t workspace_bytes;
  int variant = 0;  // tools build A/B: 3 = separate (un-fused) kernels, 11 = apply_vjp_rows (include/hdrnet_amd_tools.h)
  bool slice = false;
};

// Training side of the point-wise guide network (guide_grad.hip).
struct GuideGradArgs {
  const float* input;   // [npx][Cin]
  const float* guide;   // [npx] the forward's guide (sigmoid output)
  const float* dguide;  // [npx]
  const float* conv1;   // [n][Cin + 1]
  const float* conv2;   // [n + 1]
  float* dinput;        // [npx][Cin] or null
  bool accumulate_dinput;  // true: dinput += guide path's share; false: dinput = it
  float* dconv1;        // [n][Cin + 1]
  float* dconv2;        // [n + 1]
  long long npx;
  int Cin, n_feats;
  void* workspace;
  size_t workspace_bytes;
};

// VJP of the curves guide (guide_grad.hip).  Parameter layouts as exported by the reference.
struct CurvesGradArgs {
  const float* input;   // [npx][3]
  const float* dguide;  // [npx]
  const float *ccm, *shifts, *slopes, *mix;  // [3][4], [16][3], [16][3], [4]
  float* dinput;        // [npx][3] or null
  bool accumulate_dinput;
  float *dccm, *dshifts, *dslopes, *dmix;
  long long npx;
  int Cin, npts;
  void* workspace;
  size_t workspace_bytes;
};

struct SliceArgs {
  const float* grid;
  const float* guide;
  float* out;
  int B, H, W, GH, GW, GD, C;
};

// The (Cin, Cout, has_offset) shapes every fast BilateralSliceApply path specialises -- ONE table for the
// forward (apply_fwd_seg / apply_fwd_rows), the per-pixel VJPs (apply_vjp_seg / apply_vjp_rows) and the
// grid VJP (grid_grad_mfma: one 16-column MFMA tile for C = Cout * Cj <= 16, fused with the per-pixel VJPs where Cj = 4;
// (4, 4, offset) has C = 20 and runs dgrid as two channel windows beside apply_vjp_seg).  X(CIN, COUT, OFFSET).
#define HDRNET_APPLY_FAST_SHAPES(X) \
  X(3, 3, true) X(3, 3, false) X(3, 4, true) X(1, 1, true) X(1, 1, false) X(1, 3, true) X(4, 4, true) X(4, 4, false)

inline bool apply_fast_shape(int Cin, int Cout, bool has_offset) {
#define HDRNET_SHAPE_EQ(CI, CO, OFF) if (Cin == CI && Cout == CO && has_offset == OFF) return true;
  HDRNET_APPLY_FAST_SHAPES(HDRNET_SHAPE_EQ)
#undef HDRNET_SHAPE_EQ
  return false;
}

// The grid channel counts the fast BilateralSlice paths specialise -- ONE table for the forward (slice_fwd_rows) and the
// gradients (apply_bwd_rows / grid_grad_mfma).  X(C).
#define HDRNET_SLICE_FAST_CHANNELS(X) X(1) X(2) X(4) X(8) X(12) X(16)

inline bool slice_fast_channels(int C) {
#define HDRNET_CHANNELS_EQ(CC) if (C == CC) return true;
  HDRNET_SLICE_FAST_CHANNELS(HDRNET_CHANNELS_EQ)
#undef HDRNET_CHANNELS_EQ
  return false;
}

inline bool grad_fast_shape(const ApplyGradArgs& a) {
  return a.slice ? slice_fast_channels(a.Cout) : apply_fast_shape(a.Cin, a.Cout, a.has_offset);
}

// generic_kernels.hip -- any shape, bit-exact vs the reference CPU op.
hipError_t launch_apply_fwd_generic(const ApplyArgs& a, hipStream_t s);
hipError_t launch_apply_grad_generic(const ApplyGradArgs& a, hipStream_t s);
hipError_t launch_slice_fwd_generic(const SliceArgs& a, hipStream_t s);
hipError_t launch_slice_grad_generic(const ApplyGradArgs& a, hipStream_t s);  // a.slice

// The row-segment families below (apply_fwd_rows / _seg / _io, apply_bwd_rows, apply_vjp_seg, slice_fwd_rows) take their
// launch geometry -- row plan, LDS layout and bytes, limits -- from row_geom.h: a `*_supported` predicate and its
// launcher read the same result.
//
// apply_fwd_rows.hip -- LDS-staged row-segment forward.  `*_supported` says whether a
// specialisation exists for the shape; `name` receives a static string naming
// the variant launched.
bool apply_fwd_rows_supported(const ApplyArgs& a);
hipError_t launch_apply_fwd_rows(const ApplyArgs& a, hipStream_t s, const char** name);
// apply_fwd_seg.hip -- the product forward for 16-B-aligned, W % 4 == 0 inputs: padded LDS image,
// LDS-DMA nontemporal pixel loads, streaming (write-through / nontemporal) buffer stores.  launch_apply_fwd_rows routes here
// when supported (else the scalar kernel of apply_fwd_rows.hip).
bool apply_fwd_seg_supported(const ApplyArgs& a);
hipError_t launch_apply_fwd_seg(const ApplyArgs& a, hipStream_t s, const char** name);
// the same kernel with the guide network evaluated in registers / the coarser pyramid level added
bool apply_fwd_seg_nnguide_supported(const ApplyArgs& a, const float* guide_out);
hipError_t launch_apply_fwd_seg_nnguide(const ApplyArgs& a, const float* conv1, const float* conv2, int n_feats,
                                        float* guide_out, hipStream_t s, const char** name);
bool apply_fwd_seg_upadd_supported(const ApplyArgs& a, const float* coarse, bool guide_nn);
hipError_t launch_apply_fwd_seg_upadd(const ApplyArgs& a, const float* coarse, int Hc, int Wc, const float* conv1,
                                      const float* conv2, int n_feats, hipStream_t s, const char** name);
#ifdef HDRNET_TOOLS_BUILD
// apply_fwd_skeletons.hip -- the memory skeletons (variants 106 and 108: a.variant says which).  They do not compute the
// op; a shape or alignment without a skeleton is refused by the entry point, never served by the product kernel.
bool apply_fwd_skeleton_supported(const ApplyArgs& a);
hipError_t launch_apply_fwd_skeleton(const ApplyArgs& a, hipStream_t s, const char** name);
void tools_set_knob(int idx, int value);  // grid_grad_mfma.hip: experiment knobs (include/hdrnet_amd_tools.h)
int tools_knob(int idx);
void coeff_net_set_trace(long long* device_buf);
#endif

// Fused point-wise-NN guide + slice-apply forward (apply_fwd_rows.hip, GUIDE_NN).
bool apply_fwd_nnguide_supported(const ApplyArgs& a, const float* guide_out);
hipError_t launch_apply_fwd_nnguide(const ApplyArgs& a, const float* conv1, const float* conv2,
                                    int n_feats, float* guide_out, hipStream_t s,
                                    const char** name);

// Slice-apply + bilinear (align_corners) up-add of the coarser pyramid level (apply_fwd_rows.hip,
// UPADD); conv1 != null additionally fuses the guide network.
bool apply_fwd_upadd_supported(const ApplyArgs& a, const float* coarse, bool guide_nn);
hipError_t launch_apply_fwd_upadd(const ApplyArgs& a, const float* coarse, int Hc, int Wc,
                                  const float* conv1, const float* conv2, int n_feats,
                                  hipStream_t s, const char** name);

// resize_bilinear.hip -- NHWC bilinear resize, align_corners = true (TF legacy semantics).
hipError_t launch_resize_bilinear(const float* in, float* out, int B, int Hin, int Win, int Hout,
                                  int Wout, int C, hipStream_t s, const char** name);
// ... of a wire-format frame: in / white_level, input_dtype 0 f32 (the launch above) / 1 u8 / 2 u16; three channels,
// a 4-byte aligned base (include/hdrnet_amd_pyramid_io.h)
hipError_t launch_resize_bilinear_io(const void* in, int input_dtype, float white_level, float* out, int B, int Hin, int Win,
                                     int Hout, int Wout, hipStream_t s, const char** name);

// Sample preparation (sample_prep.hip): wire-format sources -> the fp32 NHWC tensors of a batch, one launch.
struct SamplePrepArgs {
  const void* src_input;   // [N][Hs][Ws][3], input_dtype: 0 f32, 1 u8, 2 u16
  const void* src_target;  // same extents, target_dtype; null without image_target
  int input_dtype, target_dtype;
  float input_white_level, target_white_level;
  int N, Hs, Ws;
  const int* ops;  // device [B][8] = {index, flip_lr, flip_ud, rot90, crop_y, crop_x, 0, 0}; null: identity, index = b
  int B, H, W;
  float* image_input;   // [B][H][W][3] or null
  float* image_target;  // [B][H][W][3] or null
  float* lowres_input;  // [B][n][n][3] or null
  int n;
  bool even_turns_only;
  // the ragged flavour (images != null): src_* are flat buffers of n_samples samples each, images back to back, and
  // Hs / Ws are unused
  const int* images = nullptr;  // device [N][4] = {offset_lo, offset_hi, Hs, Ws}, the offset in samples
  long long n_samples = 0;
  // the low-res gather alone (hdrnet_lowres_input_px): how src_input stores a pixel, HDRNET_PX_* as ApplyIoArgs::pixel_format
  int pixel_format = 0;
  // the low-res gather of a YUV surface (hdrnet_lowres_input_yuv): src_input is unused, input_dtype the sample dtype
  const YuvSurface* yuv = nullptr;
  const float* yuv_to_rgb = nullptr;
  // ... or of a planar one (hdrnet_lowres_input_yuv_planar): yuv_to_rgb as above
  const YuvPlanarSurface* yuv_planar = nullptr;
  // the surface's chroma layout (include/hdrnet_amd_yuv_chroma.h): kChroma420 / kChroma422 / kChroma444 (planar only)
  int yuv_chroma = kChroma420;
  // ... or of a packed 4:2:2 one (hdrnet_lowres_input_yuv_packed): yuv_to_rgb as above
  const YuvPackedSurface* yuv_packed = nullptr;
};
hipError_t launch_sample_prep(const SamplePrepArgs& a, hipStream_t s);

bool apply_fwd_io_supported(const ApplyIoArgs& a);
hipError_t launch_apply_fwd_io(const ApplyIoArgs& a, hipStream_t s, const char** name);
rows::RowGeom apply_fwd_io_geom(const ApplyIoArgs& a);  // the launch geometry both of them, and the sibling below, read
// apply_fwd_io_yuv.hip -- the same forward reading a YUV surface (a.yuv), and the surface -> float32 RGB conversion
bool apply_fwd_io_yuv_supported(const ApplyIoArgs& a);
hipError_t launch_apply_fwd_io_yuv(const ApplyIoArgs& a, hipStream_t s, const char** name);
hipError_t launch_yuv_to_rgb(const YuvSurface& in, int sample_dtype, const float* to_rgb, float* rgb, int B, int H, int W,
                             hipStream_t s);
// apply_fwd_io_yuv_planar.hip -- the same forward reading a PLANAR YUV surface (a.yuvp), and its surface -> float32 RGB
// conversion
bool apply_fwd_io_yuv_planar_supported(const ApplyIoArgs& a);
hipError_t launch_apply_fwd_io_yuv_planar(const ApplyIoArgs& a, hipStream_t s, const char** name);
hipError_t launch_yuv_planar_to_rgb(const YuvPlanarSurface& in, int sample_dtype, const float* to_rgb, float* rgb, int B, int H,
                                    int W, hipStream_t s);
// apply_fwd_io_yuv_422.hip, apply_fwd_io_yuv_planar_422.hip / _444.hip -- the same forwards and conversions for surfaces of
// another chroma layout (include/hdrnet_amd_yuv_chroma.h: a.yuv->chroma / a.yuvp->chroma != kChroma420), every output kind
// of theirs, the P210 / P216 one (kYuvOutP016) included
bool apply_fwd_io_yuv_422_supported(const ApplyIoArgs& a);
hipError_t launch_apply_fwd_io_yuv_422(const ApplyIoArgs& a, hipStream_t s, const char** name);
hipError_t launch_yuv_422_to_rgb(const YuvSurface& in, int sample_dtype, const float* to_rgb, float* rgb, int B, int H, int W,
                                 hipStream_t s);
// apply_fwd_io_yuv_packed.hip -- ... and for packed 4:2:2 surfaces (include/hdrnet_amd_yuv_packed.h: a.yuvk)
bool apply_fwd_io_yuv_packed_supported(const ApplyIoArgs& a);
hipError_t launch_apply_fwd_io_yuv_packed(const ApplyIoArgs& a, hipStream_t s, const char** name);
hipError_t launch_yuv_packed_to_rgb(const YuvPackedSurface& in, int sample_dtype, const float* to_rgb, float* rgb, int B, int H,
                                    int W, hipStream_t s);
bool apply_fwd_io_yuv_planar_chroma_supported(const ApplyIoArgs& a);
hipError_t launch_apply_fwd_io_yuv_planar_422(const ApplyIoArgs& a, hipStream_t s, const char** name);
hipError_t launch_apply_fwd_io_yuv_planar_444(const ApplyIoArgs& a, hipStream_t s, const char** name);
hipError_t launch_yuv_planar_422_to_rgb(const YuvPlanarSurface& in, int sample_dtype, const float* to_rgb, float* rgb, int B,
                                        int H, int W, hipStream_t s);
hipError_t launch_yuv_planar_444_to_rgb(const YuvPlanarSurface& in, int sample_dtype, const float* to_rgb, float* rgb, int B,
                                        int H, int W, hipStream_t s);
// apply_fwd_io_u16.hip -- the same forward with a 16-bit output (a.output_dtype == 2): a uint16 frame in the input's pixel
// format, or (a.yuv, out_kind == kYuvOutP016) a P010 / P016 surface
bool apply_fwd_io_u16_supported(const ApplyIoArgs& a);
hipError_t launch_apply_fwd_io_u16(const ApplyIoArgs& a, hipStream_t s, const char** name);
// apply_fwd_io_upadd.hip -- the same forward + the up-add of the coarser pyramid level (guide map or guide network; every
// dtype pair but f32 -> f32, which is launch_apply_fwd_upadd's)
bool apply_fwd_io_upadd_supported(const ApplyIoArgs& a, const float* coarse);
hipError_t launch_apply_fwd_io_upadd(const ApplyIoArgs& a, const float* coarse, int Hc, int Wc, hipStream_t s,
                                     const char** name);
// apply_fwd_io_upadd_yuv.hip -- ... and the same up-add on a 4:2:0 surface (a.yuv / a.yuvp; include/hdrnet_amd_pyramid_yuv.h):
// every output kind of the single-level surface forwards, a.yuv->out_kind == kYuvOutP016 among them
bool apply_fwd_io_upadd_yuv_supported(const ApplyIoArgs& a, const float* coarse);
hipError_t launch_apply_fwd_io_upadd_yuv(const ApplyIoArgs& a, const float* coarse, int Hc, int Wc, hipStream_t s,
                                         const char** name);
// resize_bilinear_yuv.hip -- resize_bilinear of the frame launch_yuv_to_rgb / launch_yuv_planar_to_rgb write, read from the
// surface (sample_dtype 1 u8 / 2 u16; an empty output is a no-op)
hipError_t launch_resize_bilinear_yuv(const YuvSurface& in, int sample_dtype, const float* to_rgb, float* out, int B, int Hin,
                                      int Win, int Hout, int Wout, hipStream_t s, const char** name);
hipError_t launch_resize_bilinear_yuv_planar(const YuvPlanarSurface& in, int sample_dtype, const float* to_rgb, float* out,
                                             int B, int Hin, int Win, int Hout, int Wout, hipStream_t s, const char** name);
// apply_fwd_io.hip -- what the C ABI calls: the pair of whichever of the families above the call belongs to (the
// 16-bit output's, else the pixel source's; `coarse`: the up-add's coarser level, or null)
bool apply_fwd_io_family_supported(const ApplyIoArgs& a, const float* coarse);
hipError_t launch_apply_fwd_io_family(const ApplyIoArgs& a, const float* coarse, int Hc, int Wc, hipStream_t s,
                                      const char** name);
// the curves guide's uniform cell tables (apply_fwd_io.hip: CurveCells), prepared once per parameter set
size_t curves_guide_prepared_bytes(int Cin);  // 0: no cell tables for this channel count
size_t curves_guide_prepared_ok_offset(int Cin);  // float index of the buffer's `ok` word
hipError_t launch_curves_guide_prepare(const float* shifts, const float* slopes, int npts, int Cin, float* prepared,
                                       hipStream_t s);

// apply_bwd_rows.hip -- LDS-staged per-pixel VJPs: dguide and dinput in one pass
// (BilateralSliceApply), dguide (BilateralSlice).  dgrid is not their business.
bool vjp_rows_supported(const ApplyGradArgs& a);
hipError_t launch_vjp_rows(const ApplyGradArgs& a, hipStream_t s, const char** name);
// BilateralSliceApply's on the product forward's core (apply_vjp_seg.hip); launch_vjp_rows routes here when it applies
bool apply_vjp_seg_supported(const ApplyGradArgs& a);
hipError_t launch_apply_vjp_seg(const ApplyGradArgs& a, hipStream_t s, const char** name);

// slice_fwd_rows.hip -- LDS-staged BilateralSlice forward with lane-contiguous stores.
bool slice_fwd_rows_supported(const SliceArgs& a);
hipError_t launch_slice_fwd_rows(const SliceArgs& a, hipStream_t s, const char** name);

// grid_grad_mfma.hip -- deterministic two-stage dgrid: per-row-run fp32 MFMA contraction over
// the pixels + fixed-order reduction of partial tiles held in the caller's workspace.
// The workspace bound of a grid with C channels, whichever op (0: GD > 16, C > 32 or extents out of range); whether
// the op has a fast kernel for its channel counts is grad_fast_shape's business.
size_t grid_grad_mfma_workspace(int B, int H, int W, int GH, int GW, int GD, int C);
bool grid_grad_mfma_supported(const ApplyGradArgs& a);  // shape AND workspace large enough
hipError_t launch_grid_grad_mfma(const ApplyGradArgs& a, hipStream_t s, const char** name);
// The same pass also producing dguide / dinput (fused backward: pixels read once for all gradients).
bool bwd_fused_supported(const ApplyGradArgs& a);
hipError_t launch_bwd_fused(const ApplyGradArgs& a, hipStream_t s, const char** name);

// guide_grad.hip -- VJP of the folded point-wise guide network; input moments for batch norm.
size_t guide_grad_workspace_bytes(long long npx, int Cin, int n);
bool guide_grad_supported(const GuideGradArgs& a);
hipError_t launch_guide_grad(const GuideGradArgs& a, hipStream_t s, const char** name);
size_t curves_grad_workspace_bytes(long long npx, int Cin, int npts);
bool curves_grad_supported(const CurvesGradArgs& a);
hipError_t launch_curves_grad(const CurvesGradArgs& a, hipStream_t s, const char** name);
size_t input_moments_workspace_bytes(long long npx, int Cin);
hipError_t launch_input_moments(const float* input, long long npx, int Cin, float* sums, float* moments,
                                void* workspace, hipStream_t s, const char** name);

// guide_grad.hip -- training-mode fold of the guide network's batch norm (statistics from the input's moments) and its VJP.
hipError_t launch_guide_nn_prescale(const float* conv1, const float* conv2, int n_feats, float x_max, float* conv1_out,
                                    float* conv2_out, hipStream_t s);
hipError_t launch_guide_fold_batch(const float* sums, const float* moments, long long npx, const float* w1,
                                   const float* gamma, const float* beta, const float* w2, const float* b2, double eps,
                                   double momentum, int Cin, int n, float* conv1, float* conv2, float* running_mean,
                                   float* running_var, long long* num_batches_tracked, hipStream_t s);
hipError_t launch_guide_fold_batch_grad(const float* sums, const float* moments, long long npx, const float* w1,
                                        const float* gamma, const float* beta, double eps, int Cin, int n,
                                        const float* dconv1, const float* dconv2, float* dw1, float* dbeta, float* dw2,
                                        float* db2, hipStream_t s);

// metrics.hip -- hdrnet/metrics.py's l2 loss and its gradient with respect to the prediction.
size_t l2_loss_workspace_bytes(long long n);
hipError_t launch_l2_loss(const float* pred, const float* target, long long n, float* loss, void* workspace,
                          hipStream_t s);
hipError_t launch_l2_loss_grad(const float* pred, const float* target, const float* grad_output, long long n,
                               float* dpred, hipStream_t s);

// coeff_net.hip -- the low-resolution coefficient network (hdrnet/models.py:62-142) as inference kernels.
bool coefficients_supported(const hdrnet_coeff_net& net);
// unsupported because of a limit of the kernels rather than the shape rules: the limit in words; else null
const char* coefficients_limit(const hdrnet_coeff_net& net);
const char* coefficients_grad_limit(const hdrnet_coeff_net& net, int B, int max_b = kCoeffNarrowMaxB);
size_t coefficients_workspace_bytes(const hdrnet_coeff_net& net, int B);  // 0: unsupported hyper-parameters
hipError_t launch_coefficients(const float* lowres, const hdrnet_coeff_net& net, float* coeffs, int B, void* workspace,
                               hipStream_t s, const char** name);
// coeff_net_train.hip -- its VJP with respect to the parameters (no batch norm); fwd_ws = the forward's workspace.
// `max_b`: the largest batch the caller admits, 8 (the C-ABI's first entry points) or 32 (their ..._wide twins); the
// launches of a batch are the same through both.
size_t coefficients_grad_workspace_bytes(const hdrnet_coeff_net& net, int B, int max_b = kCoeffNarrowMaxB);  // 0: not supported
hipError_t launch_coefficients_grad(const float* lowres, const hdrnet_coeff_net& net, const hdrnet_coeff_net_grads& gr,
                                    const float* dcoeffs, int B, const void* fwd_ws, void* workspace, hipStream_t s,
                                    const char** name, int max_b = kCoeffNarrowMaxB);
// The same network trained WITH batch norm (coeff_net_bn.hip's kernels between the launches of the two files above);
// the workspace queries return 0 outside 2 <= B <= max_b or what the gradient above supports.
size_t coefficients_bn_workspace_bytes(const hdrnet_coeff_net& net, int B, int max_b = kCoeffNarrowMaxB);
hipError_t launch_coefficients_bn(const float* lowres, const hdrnet_coeff_net_bn& bn, float* coeffs, int B,
                                  void* workspace, hipStream_t s, int max_b = kCoeffNarrowMaxB);
size_t coefficients_bn_grad_workspace_bytes(const hdrnet_coeff_net& net, int B, int max_b = kCoeffNarrowMaxB);
hipError_t launch_coefficients_bn_grad(const float* lowres, const hdrnet_coeff_net_bn& bn,
                                       const hdrnet_coeff_net_bn_grads& grads, const float* dcoeffs, int B,
                                       const void* fwd_ws, void* workspace, hipStream_t s, int max_b = kCoeffNarrowMaxB);

// capi.hip -- the tail of every C-ABI entry point, for those defined beside their kernels too.  The error text
// (hdrnet_last_error) is thread-local and the kernel name (hdrnet_last_kernel) optional bookkeeping; both live there.
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));  // sets the text, returns `code`
// e != hipSuccess: HDRNET_RUNTIME_FAILURE and "<what> kernel failed: <HIP's text>"; else clears the text, records
// `name` as the kernel launched (null: leaves the recorded name alone) and returns HDRNET_OK
int finish_launch(hipError_t e, const char* what, const char* name);
int finish_noop();  // the legal no-op: HDRNET_OK, no text, kernel name "noop"

}  // namespace hdrnet_amd
