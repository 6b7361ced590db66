// BilateralSliceApply forward with the product's WIRE FORMATS fused in.
//
// Around the op the reference converts images on the host / in separate TF ops:
//   input  uint8 / uint16  ->  tf.to_float(im) / white_level      hdrnet/data_pipeline.py:202-232
//                                                                  (255 or 65535), :267-274 (HDR+:
//                                                                  32767); run.py:157-164
//   output float -> tf.cast(255 * clip(out, 0, 1), uint8)          hdrnet/bin/run.py:95
// Here both conversions happen in registers: a 4K RGB frame moves 3 (or 6) + 3 bytes per pixel
// instead of 12 + 12 (+ the conversion kernels' own traffic), and, with the guide network fused
// as well (GUIDE_NN, apply_fwd_rows.hip), nothing but the image itself touches HBM.
//
// Geometry and slicing code are those of apply_fwd_rows_vec4 (rows_common.hip.h).  A thread's 4
// pixels are 12 contiguous bytes of uint8 RGB -- per-lane dwordx3 accesses that are contiguous
// across the wave -- so the quantised paths need no LDS transpose; a float output still goes
// through it.
//
// PIXEL FORMATS (include/hdrnet_amd_pixel_formats.h): an integer frame may also be BGR, RGBA or BGRA.  The format is a
// template parameter of the one kernel: it chooses which bytes load_pixels (white_level.hip.h) picks and which bytes the
// uint8 epilogue fills -- 12 bytes per lane without alpha, 16 with (one dwordx4 each way) -- and nothing in between, so
// every format computes the RGB instantiation's values.  Alpha travels in registers from the load to the store.
//
// YUV SURFACES (include/hdrnet_amd_yuv.h): the frame may also be a semi-planar 4:2:0 surface, NV12 or P010 / P016.  PX =
// kPxYuv replaces the load -- a lane's 4 pixels are one dword of Y and one of UV (two each for uint16 samples), converted
// by yuv_convert.hip.h's one function into the same inf[] -- and OUT = kOutNV12 the store: a workgroup then owns a row
// PAIR, runs the stage-image / pixel phase twice over the same LDS region and keeps the 2 x 2 blocks' chroma sums in
// registers in between.  Neither changes a line of what the other instantiations compile.
//
// PACKED 4:2:2 SURFACES (include/hdrnet_amd_yuv_packed.h): YUY2 / UYVY / YVYU / Y210 / Y216, the NV16 / P210 surface with its
// two planes woven into one.  PX = kPxYuvPacked is the surface load from ONE plane -- a lane's 4 pixels are 8 contiguous bytes
// of uint8 samples, 16 of uint16 -- and OUT = kOutYuy2 / kOutY216 a store of its own that weaves the 4:2:2 code words back; the
// byte order is a wave-uniform v_perm_b32 selector, not an instantiation.  Their instantiations are
// apply_fwd_io_yuv_packed.hip's; every instantiation above compiles to the code it was.
//
// This header holds the kernel, its launch and what the front ends share (label, guide-form dispatch, common predicate
// rules); the RGB instantiations are compiled by apply_fwd_io.hip, those of the
// other formats by apply_fwd_io_px.hip (a translation unit of its own: they are twice as many), those of the YUV
// surfaces by apply_fwd_io_yuv.hip, those of the planar surfaces by apply_fwd_io_yuv_planar.hip.
//
// PLANAR SURFACES (include/hdrnet_amd_yuv_planar.h): I420 / yuv420p10le / yuv420p16le, three planes each way.  PX =
// kPxYuvPlanar is the surface load with one narrower access into each of the U and V planes in place of the interleaved
// one (yuv_convert.hip.h), and OUT = kOutI420 / kOutI016 the row-pair store above with the chroma code words split the
// same way; everything between load and store is the semi-planar instantiation's, so the two give the same bits.
//
// CHROMA LAYOUTS (include/hdrnet_amd_yuv_chroma.h): CH = kChroma422 / kChroma444 is one more compile-time axis of the surface
// load and store: which chroma sample a pixel reads, and the footprint a stored chroma sample is the mean of.  Both have a
// chroma row per image row, so a surface output needs no row pair: one row per workgroup, launch grid y = H.  The default
// CH = kChroma420 compiles every instantiation above to the code it was.
//
// 16-BIT OUTPUT (include/hdrnet_amd_u16_out.h): TO = uint16_t stores a uint16 frame, (uint16)(out_white * clip(v, 0, 1)) in
// the input's pixel format -- the uint8 store's rule with 255 replaced by a run-time constant -- and OUT = kOutP016 a
// P010 / P016 surface, the NV12 store's row-pair structure with uint16 code words.  Each shares its store with the 8-bit
// sibling, written once on sizeof(TO); the 8-bit constants (255, shift 0) stay compile-time literals.  Their instantiations are
// apply_fwd_io_u16.hip's, DELIBERATELY LIMITED to keep the build small: uint16 and float32 RGB frames and uint16 BGR / RGBA
// / BGRA frames to a uint16 frame, a uint16 surface to a uint16 surface.  uint8 -> 16 bit, float32 packed orders, a uint16
// RGB frame out of a YUV surface and the pyramid's up-add are not instantiated and are refused by rule.
//
// THE PYRAMID ON A SURFACE (include/hdrnet_amd_pyramid_yuv.h): UPADD = true adds the bilinearly up-sampled coarser level
// (upadd_quad, rows_common.hip.h; IoUpParams::up) to a lane's pixels between the pixel phase and the store -- the finest level of
// HDRNetGaussianPyrNN reading a 4:2:0 surface.  Its instantiations are apply_fwd_io_upadd_yuv.hip's; UPADD = false, the
// default, compiles every instantiation above to the code it was.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <type_traits>

#include "launch.hip.h"
#include "numerics.hip.h"
#include "rows_common.hip.h"
#include "seg_common.hip.h"
#include "white_level.hip.h"

namespace hdrnet_amd {
namespace {

using namespace rows;

// Guide sources: 0 = a [B][H][W] map in memory; 1 = the folded point-wise guide network
// (HDRNetPointwiseNNGuide._guide, hdrnet/models.py:203-210); 2 = the curves guide of the standard
// model (HDRNetCurves._guide, hdrnet/models.py:145-190: 3x4 colour matrix, npts-knot ReLU curves per
// channel, channel mixing, clip) -- the network the reference's standard GL shader evaluates in its
// slicing pass (benchmark/assets/std.frag:36-45), in the parameter layout
// hdrnet/bin/freeze_graph.py:107-127 exports (guide_ccm_f32_3x4.bin, guide_shifts_f32_16x3.bin,
// guide_slopes_f32_16x3.bin, guide_mix_matrix_f32_1x4.bin).
constexpr int kGuideMap = 0, kGuideNN = 1, kGuideCurves = 2;
constexpr int kGuideCurvesScan = 3;  // the curves guide evaluated knot by knot: more than kCurveMaxKnots knots per channel
constexpr int kGuideCurvesCells = 4;  // the curves guide from the PREPARED uniform cell tables (CurveCells below)

// PX beyond the packed formats of white_level.hip.h: the frame is a YUV surface (IoParams::yin); the op still sees R, G, B
constexpr int kPxYuv = 4;
constexpr int kPxYuvPlanar = 5;  // ... or a PLANAR one (IoParams::pin): the same samples, chroma in two planes
// what the kernel stores: a frame of TO in the input's packed format / RGB -- or an NV12 surface (IoParams::yout)
// ... or a P010 / P016 surface (uint16 code words of IoParams::code_shift's depth in the high bits)
constexpr int kOutFrame = 0, kOutNV12 = 1, kOutP016 = 2;
// ... or a planar surface (IoParams::pout): I420 (uint8 code words) / uint16 code words in the LOW bits (code_shift = 0)
constexpr int kOutI420 = 3, kOutI016 = 4;
// ... or a PACKED 4:2:2 one (IoParams::kin / kout): YUY2 / UYVY / YVYU (uint8), Y210 / Y216 (uint16, the code in the high bits)
constexpr int kPxYuvPacked = 6;
constexpr int kOutYuy2 = 5, kOutY216 = 6;

struct GuideNet {
  const float* conv1;  // NN: [n][CIN + 1]            curves: ccm [CIN][CIN + 1] (row = output channel)
  const float* conv2;  // NN: [n + 1]                 curves: mix [CIN + 1]
  const float* shifts;  //                            curves: [n][CIN]
  const float* slopes;  //                            curves: [n][CIN]
  float* guide_out;    // optional
  int n;               // NN: features                curves: knots per channel
  bool fast_sigmoid;   // NN: GuideNN::fast_sigmoid (rows_common.hip.h)
  bool prescaled;      // NN: GuideNN::prescaled
  const float* prepared;  // curves: the uniform cell tables of hdrnet_curves_guide_prepare_f32 (CurveCells), or null
};

typedef __attribute__((address_space(4))) const float cfloat;  // wave-uniform parameters: s_load

// guide = clip(mix[CIN] + sum_c mix[c] * sum_k slopes[k][c] * relu(t_c - shifts[k][c]), 0, 1),
// t_c = ccm[c][CIN] + sum_j ccm[c][j] * in_j     (models.py:157-188), for a lane's 4 pixels at once: one
// pass over the knots, every parameter read once through the constant address space.  (The SCAN form: 3 operations
// per knot, channel and pixel -- 144 per pixel for the reference's 16 knots.  Kept for more than kCurveMaxKnots
// knots; the product path is the table form below.)
template <int CIN>
__device__ __forceinline__ void guide_curves_scan_quad(const GuideNet& gn, const float* inf, float (&g)[kPxPerThread]) {
  cfloat* ccm = (cfloat*)gn.conv1;
  cfloat* mix = (cfloat*)gn.conv2;
  cfloat* shifts = (cfloat*)gn.shifts;
  cfloat* slopes = (cfloat*)gn.slopes;
  // pixels in pairs on v_pk_fma_f32 / v_pk_add_f32 (the same per-pixel operation chains as the scalar form)
  static_assert(kPxPerThread == 4, "two pixel pairs");
  f32x2 t[2][CIN], cv[2][CIN];
#pragma unroll
  for (int c = 0; c < CIN; ++c) {
    float w[CIN + 1];
#pragma unroll
    for (int j = 0; j <= CIN; ++j) w[j] = ccm[c * (CIN + 1) + j];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x2 hv = {w[CIN], w[CIN]};
#pragma unroll
      for (int j = 0; j < CIN; ++j)
        hv = __builtin_elementwise_fma(f32x2{w[j], w[j]}, f32x2{inf[(2 * h) * CIN + j], inf[(2 * h + 1) * CIN + j]}, hv);
      t[h][c] = hv;
      cv[h][c] = f32x2{0.0f, 0.0f};
    }
  }
#pragma unroll 4
  for (int k = 0; k < gn.n; ++k) {
#pragma unroll
    for (int c = 0; c < CIN; ++c) {
      const float sl = slopes[k * CIN + c], sh = shifts[k * CIN + c];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x2 d = t[h][c] - f32x2{sh, sh};
        const f32x2 r = {fmaxf(d.x, 0.0f), fmaxf(d.y, 0.0f)};
        cv[h][c] = __builtin_elementwise_fma(f32x2{sl, sl}, r, cv[h][c]);
      }
    }
  }
  float m[CIN + 1];
#pragma unroll
  for (int c = 0; c <= CIN; ++c) m[c] = mix[c];
#pragma unroll
  for (int q = 0; q < kPxPerThread; ++q) {
    float v = m[CIN];
#pragma unroll
    for (int c = 0; c < CIN; ++c) v = fmaf(m[c], (q & 1) ? cv[q >> 1][c].y : cv[q >> 1][c].x, v);
    g[q] = fminf(fmaxf(v, 0.0f), 1.0f);  // tf.clip_by_value(guidemap, 0, 1)
  }
}

// ---- the curves guide as a sorted piecewise-linear lookup (round 4) --------------------------------------------------
// sum_k slope_k * relu(t - shift_k) is piecewise linear in t with its breaks at the shifts.  Per workgroup, wave 0
// sorts each channel's knots (rank by counting; ties by index) and tabulates, for the interval that starts at the
// i-th smallest knot s_(i):  the knot, the curve's VALUE there  C_i = sum_{r<i} slope_(r) (s_(i) - s_(r))  and its SLOPE
// from there on  A_i = sum_{r<=i} slope_(r)  (both summed in float64, rounded once).  A pixel then finds its interval
// with a 4-step binary search over the sorted knots (an implicit tree in LDS, Eytzinger order: node e's children are
// 2e and 2e + 1) and evaluates  C_i + A_i * max(t - s_(i), 0)  -- anchored at the interval's own knot, so that the
// result carries one rounding of the curve's value instead of the scan's 16.  15 instead of 48 operations per channel
// and pixel, 4 ds_read_b32 + 1 ds_read_b128 (conflict-free: <= 16 consecutive dwords / 16-B entries per channel).
// Left of the smallest knot every relu is zero: leaf 0 holds C = 0 and the max() clamps the distance.
// Up to kCurveMaxKnots knots per channel (the reference has 16, hdrnet/models.py:150); unused slots are +inf knots
// with slope 0.  The tables sit at the START of dynamic LDS (compile-time addresses); the coefficient image follows.
constexpr int kCurveMaxKnots = 16;
template <int CIN>
struct CurveTab {
  static constexpr int kTree = 0;                    // [CIN][16]: node e of channel c at c * 16 + e (e = 1 .. 15)
  static constexpr int kLeaf = 64;                   // [CIN][16][4]: (knot, value at it, slope after it, 0); >= 64 floats in,
                                                     // so that (leaf base - 256 B) stays a non-negative immediate offset
  static constexpr int kRawS = kLeaf + CIN * 64;     // scratch while building: knots / slopes as given,
  static constexpr int kRawL = kRawS + CIN * 16;
  static constexpr int kSortS = kRawL + CIN * 16;    //   ... and sorted
  static constexpr int kSortL = kSortS + CIN * 16;
  static constexpr int kFloats = kSortL + CIN * 16;  // 16-B multiple
};

// Run by the first CIN * 16 lanes of wave 0 (lane = channel * 16 + knot); the caller's workgroup barrier publishes
// the tables.  CIN * 16 <= 64.
template <int CIN>
__device__ __forceinline__ void curves_build_tables(float* __restrict__ tab, const GuideNet& gn, int lane) {
  static_assert(CIN * 16 <= 64 && CIN * 16 <= CurveTab<CIN>::kLeaf, "one wave builds the tables; the tree fits below the leaves");
  typedef CurveTab<CIN> T;
  const int c = lane >> 4, k = lane & 15;
  const bool mine = lane < CIN * 16;
  float s = __builtin_inff(), sl = 0.0f;
  if (mine && k < gn.n) {
    s = gn.shifts[k * CIN + c];
    sl = gn.slopes[k * CIN + c];
  }
  if (mine) {
    tab[T::kRawS + lane] = s;
    tab[T::kRawL + lane] = sl;
  }
  wave_lds_sync();
  if (mine) {
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float sj = tab[T::kRawS + c * 16 + j];
      rank += (sj < s || (sj == s && j < k)) ? 1 : 0;
    }
    tab[T::kSortS + c * 16 + rank] = s;
    tab[T::kSortL + c * 16 + rank] = sl;
  }
  wave_lds_sync();
  if (mine) {
    const int i = k;
    const float si = tab[T::kSortS + c * 16 + i];
    double A = 0.0, Cv = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float sr = tab[T::kSortS + c * 16 + r], lr = tab[T::kSortL + c * 16 + r];
      if (r < i) Cv += (double)lr * ((double)si - (double)sr);
      if (r <= i) A += (double)lr;
    }
    const bool dead = !(si < __builtin_inff());  // an unused slot (or an infinite / NaN knot): never reached
    float4 leaf = make_float4(si, (float)Cv, (float)A, 0.0f);
    if (dead) leaf = make_float4(__builtin_inff(), 0.0f, 0.0f, 0.0f);
    *reinterpret_cast<float4*>(tab + T::kLeaf + (c * 16 + i) * 4) = leaf;
    if (i >= 1) {
      // sorted key j = i - 1 of the 15 search keys s_(1) .. s_(15) -> its Eytzinger node: with t = ctz(j + 1) the node sits
      // on level 3 - t at position (j + 1) >> (t + 1)
      const int j1 = i;  // j + 1
      const int t = __builtin_ctz(j1);
      const int e = (1 << (3 - t)) + (j1 >> (t + 1));
      tab[T::kTree + c * 16 + e] = si;
    }
  }
}

template <int CIN>
__device__ __forceinline__ float curve_lookup(const float* __restrict__ tab, int c, float v) {
  typedef CurveTab<CIN> T;
  // the walk carries the node's BYTE offset a = 4 * node: a' = 2 a + (v >= key ? 4 : 0) -- compare, select, shift-add --
  // and the ds_read takes it as it is (the channel's base is the instruction's immediate offset)
  const char* tree = reinterpret_cast<const char*>(tab + T::kTree + c * 16);
  unsigned a = 4u;
#pragma unroll
  for (int d = 0; d < 4; ++d) a = (a << 1) + ((v >= *reinterpret_cast<const float*>(tree + a)) ? 4u : 0u);
  // leaf = node - 16, 16 bytes each: byte offset 4 a - 256
  const char* leaves = reinterpret_cast<const char*>(tab + T::kLeaf + c * 64) - 256;
  const f32x4 leaf = *reinterpret_cast<const f32x4*>(leaves + (a << 2));
  return __builtin_fmaf(leaf.z, fmaxf(v - leaf.x, 0.0f), leaf.y);
}

// The guide of a lane's 4 pixels from the tables (same colour matrix / mixing / clip as the scan form).
template <int CIN>
__device__ __forceinline__ void guide_curves_quad(const float* __restrict__ tab, const GuideNet& gn, const float* inf,
                                                  float (&g)[kPxPerThread]) {
  cfloat* ccm = (cfloat*)gn.conv1;
  cfloat* mix = (cfloat*)gn.conv2;
  float w[CIN][CIN + 1], m[CIN + 1];
#pragma unroll
  for (int c = 0; c < CIN; ++c) {
#pragma unroll
    for (int j = 0; j <= CIN; ++j) w[c][j] = ccm[c * (CIN + 1) + j];
  }
#pragma unroll
  for (int c = 0; c <= CIN; ++c) m[c] = mix[c];
  float cv[kPxPerThread][CIN];
#pragma unroll
  for (int q = 0; q < kPxPerThread; ++q) {
#pragma unroll
    for (int c = 0; c < CIN; ++c) {
      float t = w[c][CIN];
#pragma unroll
      for (int j = 0; j < CIN; ++j) t = fmaf(w[c][j], inf[q * CIN + j], t);
      cv[q][c] = curve_lookup<CIN>(tab, c, t);
    }
  }
#pragma unroll
  for (int q = 0; q < kPxPerThread; ++q) {
    float v = m[CIN];
#pragma unroll
    for (int c = 0; c < CIN; ++c) v = fmaf(m[c], cv[q][c], v);
    g[q] = fminf(fmaxf(v, 0.0f), 1.0f);  // tf.clip_by_value(guidemap, 0, 1)
  }
}

// ---- the curves guide through UNIFORM CELL TABLES prepared once per parameter set (round 5) ---------------------------
// The sorted tables above are rebuilt by wave 0 of EVERY workgroup (~150 instructions + two wave barriers before the
// workgroup's barrier) and searched with four dependent LDS reads per channel and pixel.  Both costs go with a table that
// depends on the parameters only and is indexed by arithmetic: hdrnet_curves_guide_prepare_f32 cuts each channel's knot
// range [s_min, s_max] into kCurveCells uniform cells by the MONOTONE map
//     cell(t) = uint(clamp(fma(t, k16, o16), 0, 16 kCurveCells - 1)) >> 4,   k16 = 16 (kCurveCells - 1) / (s_max - s_min)
// (the same fp32 instructions for a knot at prepare time and for a pixel here: t1 <= t2 => cell(t1) <= cell(t2), so every
// knot of an earlier cell is <= t and every knot of a later cell is > t -- exactly, whatever the rounding) and stores per
// cell one 16-byte entry (s, C, A_lo, A_hi): the knot inside the cell, the curve's value at it, the slopes before and
// after it -- or, for a cell without a knot, the last knot to its left with A_lo = A_hi.  A pixel evaluates
//     C + (t >= s ? A_hi : A_lo) (t - s)
// -- one ds_read_b128 and 8 VALU instructions per channel instead of 4 + 1 dependent reads and 16; anchored at a knot at
// most one cell away, with the float64-summed C and A of the sorted tables (curves_build_tables, run once by the prepare
// kernel).  A cell can hold one knot only: if two knots of a channel share a cell (closer than 1/63 of the knot range, or
// equal) the prepare kernel clears the table's `ok` word: the table is NOT USABLE, hdrnet_curves_guide_prepare_f32 reads
// the word back and says so, and its caller passes no prepared buffer -- the sorted tables above, the same results.  (The
// two forms are two kernel instantiations chosen on the host: one kernel with both behind a run-time switch took 70-74
// VGPRs instead of 54-64.)  Layout of the prepared buffer (floats): [CIN][kCurveCells][4] entries, then per channel
// (k16, o16, 0, 0), then (ok, 0, 0, 0).
constexpr int kCurveCells = 64;
template <int CIN>
struct CurveCells {
  static constexpr int kEntries = 0;
  static constexpr int kScale = CIN * kCurveCells * 4;  // [CIN][4]
  static constexpr int kOk = kScale + CIN * 4;          // [4]
  static constexpr int kFloats = kOk + 4;
};

__device__ __forceinline__ unsigned curve_cell_byte(float t, float k16, float o16) {
  const float u = __builtin_amdgcn_fmed3f(__builtin_fmaf(t, k16, o16), 0.0f, (float)(16 * kCurveCells - 1));
  return (unsigned)u & ~15u;
}

template <int CIN>
__global__ __launch_bounds__(256) void curves_prepare_kernel(const GuideNet gn, float* __restrict__ out) {
  typedef CurveTab<CIN> T;
  typedef CurveCells<CIN> L;
  __shared__ __attribute__((aligned(16))) float tab[T::kFloats];
  __shared__ int cell_of[CIN * 16];
  __shared__ float kk[CIN], oo[CIN];
  __shared__ int bad;
  const int tid = threadIdx.x;
  if (tid == 0) bad = 0;
  if (tid < 64) curves_build_tables<CIN>(tab, gn, tid);  // sorted leaves (knot, value at it, slope after it, 0); dead: +inf
  __syncthreads();
  const float inf = __builtin_inff();
  if (tid < CIN) {
    const float* lf = tab + T::kLeaf + tid * 64;
    const float smin = lf[0];
    float smax = smin;
    for (int i = 1; i < 16; ++i) {
      const float s = lf[4 * i];
      if (s < inf) smax = s;
    }
    float k16 = 0.0f, o16 = 0.0f;
    if (smin < inf && smax > smin) {
      k16 = (float)(16 * (kCurveCells - 1)) / (smax - smin);
      o16 = -smin * k16;
      if (!(k16 < inf) || !(fabsf(o16) < inf)) k16 = o16 = 0.0f;  // a range too narrow to scale: one cell (ok only for one knot)
    }
    kk[tid] = k16;
    oo[tid] = o16;
  }
  __syncthreads();
  if (tid < CIN * 16) {
    const float s = tab[T::kLeaf + tid * 4];
    cell_of[tid] = (s < inf) ? (int)(curve_cell_byte(s, kk[tid >> 4], oo[tid >> 4]) >> 4) : 0x7fffffff;  // dead knots: no cell
  }
  __syncthreads();
  for (int e = tid; e < CIN * kCurveCells; e += (int)blockDim.x) {
    const int c = e / kCurveCells, j = e - c * kCurveCells;
    int here = -1, count = 0, last = -1;
    for (int i = 0; i < 16; ++i) {  // sorted knots + a monotone cell map: cell_of is non-decreasing in i
      const int ci = cell_of[c * 16 + i];
      if (ci == j) {
        here = i;
        ++count;
      }
      if (ci < j) last = i;
    }
    if (count > 1) bad = 1;  // (every writer writes 1)
    float4 ent = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // left of every knot: the curve is 0
    const float4* leaves = reinterpret_cast<const float4*>(tab + T::kLeaf + c * 64);
    if (here >= 0) {
      const float4 lf = leaves[here];
      ent = make_float4(lf.x, lf.y, here > 0 ? leaves[here - 1].z : 0.0f, lf.z);
    } else if (last >= 0) {
      const float4 lf = leaves[last];
      ent = make_float4(lf.x, lf.y, lf.z, lf.z);
    }
    reinterpret_cast<float4*>(out + L::kEntries)[e] = ent;
  }
  __syncthreads();
  if (tid < CIN) reinterpret_cast<float4*>(out + L::kScale)[tid] = make_float4(kk[tid], oo[tid], 0.0f, 0.0f);
  if (tid == 0) reinterpret_cast<float4*>(out + L::kOk)[0] = make_float4(bad ? 0.0f : 1.0f, 0.0f, 0.0f, 0.0f);
}

// The guide of a lane's 4 pixels from the cell tables (`cells`: the entries, copied into LDS by the workgroup).  The colour
// matrix and the cell coordinate run on pixel pairs (v_pk_fma_f32, parameters from SGPRs); mixing and clip as above.
template <int CIN>
__device__ __forceinline__ void guide_curves_quad_cells(const float* __restrict__ cells, const GuideNet& gn, const float* inf,
                                                        float (&g)[kPxPerThread]) {
  typedef CurveCells<CIN> L;
  cfloat* ccm = (cfloat*)gn.conv1;
  cfloat* mix = (cfloat*)gn.conv2;
  cfloat* sc = (cfloat*)(gn.prepared + L::kScale);
  static_assert(kPxPerThread == 4, "two pixel pairs");
  float cv[kPxPerThread][CIN];
#pragma unroll
  for (int c = 0; c < CIN; ++c) {
    float w[CIN + 1];
#pragma unroll
    for (int j = 0; j <= CIN; ++j) w[j] = ccm[c * (CIN + 1) + j];
    const float k16 = sc[4 * c], o16 = sc[4 * c + 1];
    const char* base = reinterpret_cast<const char*>(cells + c * kCurveCells * 4);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      f32x2 t = {w[CIN], w[CIN]};
#pragma unroll
      for (int j = 0; j < CIN; ++j)
        t = __builtin_elementwise_fma(f32x2{w[j], w[j]}, f32x2{inf[(2 * h) * CIN + j], inf[(2 * h + 1) * CIN + j]}, t);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const float ti = i ? t.y : t.x;
        const f32x4 e = *reinterpret_cast<const f32x4*>(base + curve_cell_byte(ti, k16, o16));
        const float d = ti - e.x;
        cv[2 * h + i][c] = __builtin_fmaf(d >= 0.0f ? e.w : e.z, d, e.y);
      }
    }
  }
  float m[CIN + 1];
#pragma unroll
  for (int c = 0; c <= CIN; ++c) m[c] = mix[c];
#pragma unroll
  for (int q = 0; q < kPxPerThread; ++q) {
    float v = m[CIN];
#pragma unroll
    for (int c = 0; c < CIN; ++c) v = fmaf(m[c], cv[q][c], v);
    g[q] = fminf(fmaxf(v, 0.0f), 1.0f);  // tf.clip_by_value(guidemap, 0, 1)
  }
}

// div_white / WhiteLevel / io_white_level (tf.to_float(im) / white_level in three instructions) and load_pixels: white_level.hip.h

struct IoParams {
  const float* grid;
  const float* guide;
  const void* input;
  void* out;
  int H, W, GH, GW, GD;
  int seg, slab_off;
  float scale_x, scale_y, inv_col;
  WhiteLevel white;
  int grid_image;  // floats per image of the grid
  SegTab tab;      // (cmin, ncols) per segment, from the host (seg_common.hip.h)
  GuideNet gn;
  // YUV surfaces (PX == kPxYuv / OUT == kOutNV12; unused by every other instantiation)
  // (a packed 4:2:2 surface, PX == kPxYuvPacked / OUT == kOutYuy2, kOutY216, SHARES their bytes: it is one plane of the pair,
  // and a longer IoParams moves the kernel-argument loads of every instantiation -- see IoUpParams below)
  union {
    YuvSurface yin;
    YuvPackedSurface kin;
  };
  union {
    YuvSurface yout;
    YuvPackedSurface kout;
  };
  const float* to_rgb;    // 12 floats each (yuv_convert.hip.h)
  const float* from_rgb;
  // 16-bit output (TO = uint16_t / OUT == kOutP016; read by no other instantiation)
  float out_white;  // a uint16 frame: (uint16)(out_white * clip(v, 0, 1))
  float code_max;   // a P010 / P016 surface: 2^out_bits - 1 ...
  int code_shift;   // ... and 16 - out_bits
  // planar surfaces (PX == kPxYuvPlanar / OUT == kOutI420, kOutI016; read by no other instantiation): to_rgb / from_rgb and,
  // for uint16 code words, code_max are the fields above; code_shift is 0
  YuvPlanarSurface pin, pout;
};

// The pyramid's finest level on a surface (UPADD): the coarser level to up-sample and add, appended at the END.  A type of
// its own, which only the UPADD instantiations take: a longer IoParams moved the kernel-argument loads of instantiations
// that never read the field (the float32 curves forward: 64 -> 63 VGPRs), and every kernel shipped keeps its machine code.
struct IoUpParams : IoParams {
  UpAdd up;
};
template <bool UPADD>
using IoParamsOf = std::conditional_t<UPADD, IoUpParams, IoParams>;

// Geometry, LDS image and pixel core are apply_fwd_seg.hip's (seg_common.hip.h): a workgroup owns a row
// segment, 3-D launch grid (segment, row, image), padded y-pre-lerped coefficient image.
template <int CIN, int COUT, bool OFFSET, int GUIDE, typename TI, typename TO, int PX = kPxRGB, int OUT = kOutFrame,
          int CH = kChroma420, bool UPADD = false>
__global__ __launch_bounds__(256) void apply_fwd_io_rows(const IoParamsOf<UPADD> p) {
  static_assert(PX == kPxRGB || (CIN == 3 && COUT == 3 && sizeof(TI) < 4), "pixel formats: integer frames, 3 -> 3");
  constexpr bool PLANAR = PX == kPxYuvPlanar;  // the input is a planar YUV surface: three planes
  constexpr bool YUVPACKED = PX == kPxYuvPacked;  // ... a packed 4:2:2 one: one plane
  constexpr bool YUV = PX == kPxYuv || PLANAR || YUVPACKED;  // the input is a YUV surface; the frame the kernel stores is RGB
  constexpr bool NV12OUT = OUT == kOutNV12;   // ... unless the output is an NV12 surface: a workgroup owns a row pair
  static_assert(!NV12OUT || (YUV && sizeof(TO) == 1), "NV12 out: uint8 planes, from a YUV surface");
  constexpr bool P016OUT = OUT == kOutP016;   // ... or a P010 / P016 surface: the same row pair, uint16 code words
  static_assert(!P016OUT || (YUV && sizeof(TI) == 2 && sizeof(TO) == 2), "P010 / P016 out: uint16 planes, from a uint16 surface");
  constexpr bool I420OUT = OUT == kOutI420, I016OUT = OUT == kOutI016;  // ... or a planar one, of the input's sample width
  static_assert(!I420OUT || (PLANAR && sizeof(TI) == 1 && sizeof(TO) == 1), "I420 out: uint8 planes, from a uint8 planar surface");
  static_assert(!I016OUT || (PLANAR && sizeof(TI) == 2 && sizeof(TO) == 2), "uint16 planar out: from a uint16 planar surface");
  constexpr bool PLANAROUT = I420OUT || I016OUT;
  constexpr bool SURFOUT = NV12OUT || P016OUT || PLANAROUT;
  constexpr bool PACKEDOUT = OUT == kOutYuy2 || OUT == kOutY216;  // ... or a packed 4:2:2 one, of the input's width and order
  static_assert(!YUVPACKED || CH == kChroma422, "a packed surface is 4:2:2");
  static_assert(!PACKEDOUT || (YUVPACKED && sizeof(TI) == sizeof(TO) && (OUT == kOutYuy2) == (sizeof(TO) == 1)),
                "a packed surface out: from a packed surface of the same sample width");
  // CH: the surfaces' chroma layout (yuv_convert.hip.h).  4:2:2 and 4:4:4 have a chroma row per image row: a surface
  // output is then ONE row per workgroup, as a frame is, and its chroma is stored after that row.
  static_assert(CH == kChroma420 || YUV, "a chroma layout belongs to a YUV surface");
  static_assert(CH != kChroma444 || PLANAR, "4:4:4: planar surfaces only");
  constexpr bool ROWPAIR = SURFOUT && CH == kChroma420;
  // UPADD (apply_fwd_io_upadd_yuv.hip): the pyramid's finest level -- the coarser level's output, up-sampled, is added to
  // the lane's pixels BEFORE any store, so the clip, the luma code and the chroma sums see the sum
  static_assert(!UPADD || (YUV && CH == kChroma420 && (GUIDE == kGuideMap || GUIDE == kGuideNN)),
                "the up-add: 4:2:0 surfaces, a guide map or the guide network");
  constexpr bool PACKED = PX != kPxRGB && !YUV;  // BGR / RGBA / BGRA
  constexpr int SPX = PACKED ? px_stored(PX) : CIN;  // samples per stored pixel of the frame
  constexpr int C = COUT * (CIN + (OFFSET ? 1 : 0));
  constexpr int CB = C * (int)sizeof(float);
  constexpr int NI = CIN * kPxPerThread, NO = COUT * kPxPerThread;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // curves guide: its lookup tables first (compile-time LDS addresses), the coefficient image behind them
  // Integer samples with a guide MAP: the input is used by the affine only, so the white level goes into the staged
  // coefficients (coef / wl) * v, and the 12 divisions per lane (3 instructions each) disappear: u8 -> u8 26.7 -> ... us.
  // (With a guide NETWORK the guide's own input stays v / wl, IEEE-rounded as TensorFlow's division.)
  // (A YUV surface's conversion clamps: its pixels enter as the converted floats, nothing to fold.)
  constexpr bool FOLD_WL = GUIDE == kGuideMap && sizeof(TI) < 4 && C == 12 && !YUV;
  // The curves guide's lookup tables are STATIC LDS: their addresses are compile-time constants, so a table walk's
  // ds_read takes the walked byte offset as its address register and the table's base as its immediate (behind the
  // dynamic array's link-time base every step paid a v_add).  The coefficient image and the slabs stay dynamic.
  // (static LDS costs resident workgroups here: 3 KB more measured 8 %, and a kernel carrying BOTH table forms behind a
  //  run-time switch took 70-74 VGPRs instead of 54-64 -- profiles/r05/f2_prepared_guides.md -- so the two forms are two
  //  instantiations, chosen on the host by whether the caller passed a prepared buffer)
  [[maybe_unused]] float* ctab = nullptr;
  if constexpr (GUIDE == kGuideCurves) {
    __shared__ __attribute__((aligned(16))) float curve_tables[CurveTab<CIN>::kFloats];
    ctab = curve_tables;
  }
  if constexpr (GUIDE == kGuideCurvesCells) {
    __shared__ __attribute__((aligned(16))) float curve_cells[CIN * kCurveCells * 4];
    ctab = curve_cells;
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int xs = blockIdx.x * p.seg;
  const int xe = min(xs + p.seg, p.W);
  const int b = blockIdx.z;
  const float* grid_b = p.grid + (size_t)b * (unsigned)p.grid_image;
  const int x = xs + kPxPerThread * tid;
  const bool active = x < xe;
  // NV12 out: the linear parts of U and V of the lane's two 2 x 2 blocks, summed over the row pair (yuv_convert.hip.h)
  [[maybe_unused]] float csum[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  // One image row per workgroup -- or, for an NV12 output, the two rows of a chroma row, one after the other through the
  // same LDS image.  (The loop's condition is a compile-time `false` for one row: no back edge, r == 0, and the
  // single-row kernels compile to the straight code they were.)
  constexpr int ROWS = ROWPAIR ? 2 : 1;
  int r = 0;
  do {
    const int y = ROWPAIR ? 2 * (int)blockIdx.y + r : (int)blockIdx.y;
    const size_t row = (unsigned)b * (unsigned)p.H + (unsigned)y;  // B, H <= 65535 (kLimBH, row_geom.h)
    const size_t px = row * p.W + x;
    const TI* input = static_cast<const TI*>(p.input);

    float gs[kPxPerThread] = {0.f, 0.f, 0.f, 0.f};
    float inf[NI];
    [[maybe_unused]] uint32_t alpha[kPxPerThread] = {};  // RGBA / BGRA: the 4 pixels' alpha samples as stored
#pragma unroll
    for (int q = 0; q < NI; ++q) inf[q] = 0.0f;
    if (active) {
      if constexpr (GUIDE == kGuideMap) {
        const float4 g4 = *reinterpret_cast<const float4*>(p.guide + px);
        gs[0] = g4.x; gs[1] = g4.y; gs[2] = g4.z; gs[3] = g4.w;
      }
      if constexpr (YUVPACKED) yuv_load_quad<TI>(p.kin, yuv_load_matrix(p.to_rgb), b, y, x, inf);
      else if constexpr (PLANAR) yuv_load_quad<TI, CH>(p.pin, yuv_load_matrix(p.to_rgb), b, y, x, inf);
      else if constexpr (YUV) yuv_load_quad<TI, CH>(p.yin, yuv_load_matrix(p.to_rgb), b, y, x, inf);
      else load_pixels<TI, NI, FOLD_WL, PX>(input, px * SPX, p.white, inf, nullptr, alpha);
    }

    // (the guide's tables depend on the parameters only: built for the first row, read for both)
    if constexpr (GUIDE == kGuideCurves) {
      if (r == 0 && wave == 0) curves_build_tables<CIN>(ctab, p.gn, lane);  // published by the barrier below
    }
    if constexpr (GUIDE == kGuideCurvesCells) {  // the prepared cell tables: 3 KB copied by the whole workgroup (barrier below)
      const f32x4* src = reinterpret_cast<const f32x4*>(p.gn.prepared);
      if (r == 0)
        for (int e = tid; e < CIN * kCurveCells; e += (int)blockDim.x) reinterpret_cast<f32x4*>(ctab)[e] = src[e];
    }
    const SegCols sc = seg_cols_tab(p.tab, blockIdx.x, xs, xe, p.scale_x);
    const int colb = (p.GD + 2) * CB;
    const float gd_f = (float)p.GD, zhi = (float)(p.GD - 1);
    // second row of a pair: the image region is staged AGAIN, once every lane has read the first row's coefficients
    if (r > 0) __syncthreads();
    stage_image<C, FOLD_WL>(lds, grid_b, y, sc.cmin, sc.ncols, p.GH, p.GW, p.GD, p.scale_y, p.inv_col, tid, (int)blockDim.x,
                            p.white.inv);
    // the lean pixel phase of the product forward (seg_common.hip.h)
    XTermLean xt[kPxPerThread];
    const float xf0 = (float)x + 0.5f;  // xf0 + k == (x + k) + 0.5f exactly: x < W <= 2^23 (row_geom.h, kMaxFloatX)
    const float colb_f = (float)colb, xbase_f = (float)(CB - sc.cmin * colb);
#pragma unroll
    for (int k = 0; k < kPxPerThread; ++k) xt[k] = x_term_lean(xf0 + (float)k, p.scale_x, colb_f, xbase_f);
    __syncthreads();

    float of[NO];
    if (active) {
      if constexpr (GUIDE != kGuideMap) {
        if constexpr (GUIDE == kGuideNN)
          guide_nn_quad<CIN>(GuideNN{p.gn.conv1, p.gn.conv2, p.gn.guide_out, p.gn.n, p.gn.fast_sigmoid, p.gn.prescaled}, inf, gs);  // (writes nothing itself)
        else if constexpr (GUIDE == kGuideCurves)
          guide_curves_quad<CIN>(ctab, p.gn, inf, gs);
        else if constexpr (GUIDE == kGuideCurvesCells)
          guide_curves_quad_cells<CIN>(ctab, p.gn, inf, gs);
        else
          guide_curves_scan_quad<CIN>(p.gn, inf, gs);
        if (p.gn.guide_out) *reinterpret_cast<float4*>(p.gn.guide_out + px) = make_float4(gs[0], gs[1], gs[2], gs[3]);
      }
#pragma unroll
      for (int k = 0; k < kPxPerThread; ++k) {
        float in[CIN], o[COUT];
#pragma unroll
        for (int j = 0; j < CIN; ++j) in[j] = inf[k * CIN + j];
        seg_pixel_lean<CIN, COUT, OFFSET, true>(lds, gd_f, zhi, colb, xt[k], gs[k], in, o);
#pragma unroll
        for (int i = 0; i < COUT; ++i) of[k * COUT + i] = o[i];
      }
      if constexpr (UPADD) upadd_quad<COUT>(p.up, b, y, x, of);  // (once per row of a pair, with that row's y)
    }

    if constexpr (PACKEDOUT) {
      // A packed 4:2:2 surface: the NV16 / P210 code words of the branch below -- luma per pixel, chroma from the horizontal
      // pair's sum with weight 0.5, expression for expression -- woven into the lane's two groups Y0 U Y1 V: 2 dwords of
      // uint8 code words (each put into the surface's byte order by the load's selector, which is its own inverse), 4 of
      // uint16 ([Y U][Y V] per group).  8 or 16 contiguous bytes per lane, as dwords.  Padding beyond the row is not written.
      constexpr int S = (int)sizeof(TO);
      if (active) {
        const YuvMatrix fk = yuv_load_matrix(p.from_rgb);
        const float cmax = S == 1 ? 255.0f : p.code_max;  // (YUY2: compile-time constants)
        const int sh = S == 1 ? 0 : p.code_shift;
        uint32_t* wo = reinterpret_cast<uint32_t*>(static_cast<char*>(const_cast<void*>(p.kout.p)) + (long long)b * p.kout.image +
                                                   (long long)y * p.kout.pitch + (size_t)x * 2 * sizeof(TO));
        [[maybe_unused]] const uint32_t sel = yuv_packed_selector(p.kout.order);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          uint32_t ly[2];
          float pu[2], pv[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int k = 2 * h + i;
            float c[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) c[j] = __builtin_amdgcn_fmed3f(of[k * COUT + j], 0.0f, 1.0f);
            ly[i] = yuv_luma_code(fk, c, cmax, sh);
            pu[i] = yuv_chroma_linear(fk, 1, c);
            pv[i] = yuv_chroma_linear(fk, 2, c);
          }
          const uint32_t cu = yuv_chroma_code(fk, 1, pu[0] + pu[1], cmax, sh, 0.5f);  // the horizontal pair is the whole footprint
          const uint32_t cv = yuv_chroma_code(fk, 2, pv[0] + pv[1], cmax, sh, 0.5f);
          if constexpr (S == 1) {
            wo[h] = yuv_packed_perm(ly[0] | (cu << 8) | (ly[1] << 16) | (cv << 24), sel);
          } else {
            wo[2 * h] = ly[0] | (cu << 16);
            wo[2 * h + 1] = ly[1] | (cv << 16);
          }
        }
      }
    } else if constexpr (SURFOUT) {
      // A semi-planar surface, NV12 (uint8 code words) or P010 / P016 (uint16, IoParams::code_max / code_shift): sizeof(TO)
      // dwords of Y per lane and row; the chroma of the lane's two 2 x 2 blocks after the second row, as many dwords (U0 V0
      // U1 V1) into the pair's interleaved UV row (block x / 2 starts at sample x of its row, as the luma does).  Padding
      // beyond the row is not written.
      constexpr int S = (int)sizeof(TO), PER = 4 / S;  // bytes per code word; code words per dword
      if (active) {
        const YuvMatrix fk = yuv_load_matrix(p.from_rgb);
        const float cmax = S == 1 ? 255.0f : p.code_max;  // (NV12: compile-time constants)
        const int sh = S == 1 ? 0 : p.code_shift;
        uint32_t wy[S];
#pragma unroll
        for (int q = 0; q < S; ++q) wy[q] = 0;
        // 4:4:4: a chroma code per pixel (footprint 1), packed as the luma is: S dwords of U and S of V
        [[maybe_unused]] uint32_t wu4[S], wv4[S];
        if constexpr (CH == kChroma444) {
#pragma unroll
          for (int q = 0; q < S; ++q) wu4[q] = wv4[q] = 0;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          float pu[2], pv[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int k = 2 * h + i;
            float c[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) c[j] = __builtin_amdgcn_fmed3f(of[k * COUT + j], 0.0f, 1.0f);
            wy[k / PER] |= yuv_luma_code(fk, c, cmax, sh) << (8 * S * (k % PER));
            pu[i] = yuv_chroma_linear(fk, 1, c);
            pv[i] = yuv_chroma_linear(fk, 2, c);
            if constexpr (CH == kChroma444) {
              wu4[k / PER] |= yuv_chroma_code(fk, 1, pu[i], cmax, sh, 1.0f) << (8 * S * (k % PER));
              wv4[k / PER] |= yuv_chroma_code(fk, 2, pv[i], cmax, sh, 1.0f) << (8 * S * (k % PER));
            }
          }
          if constexpr (CH == kChroma420) {
            csum[h][0] += pu[0] + pu[1];  // horizontal pair first; even row (onto 0), then odd row
            csum[h][1] += pv[0] + pv[1];
          } else if constexpr (CH == kChroma422) {
            csum[h][0] = pu[0] + pu[1];  // the horizontal pair is the whole footprint
            csum[h][1] = pv[0] + pv[1];
          }
        }
        constexpr float CW = CH == kChroma420 ? 0.25f : 0.5f;  // footprint weight of the summed layouts
        const int yc = yuv_chroma_row(CH, y);
        char* yo = static_cast<char*>(const_cast<void*>(p.yout.y)) + (long long)b * p.yout.image_y + (long long)y * p.yout.pitch_y +
                   (size_t)x * sizeof(TO);
        if constexpr (PLANAROUT)  // (the Y plane of the planar surface; the store itself is the same)
          yo = static_cast<char*>(const_cast<void*>(p.pout.y)) + (long long)b * p.pout.image_y + (long long)y * p.pout.pitch_y +
               (size_t)x * sizeof(TO);
#pragma unroll
        for (int q = 0; q < S; ++q) reinterpret_cast<uint32_t*>(yo)[q] = wy[q];  // (dwords: the planes promise 4-byte alignment, not 8)
        if constexpr (PLANAROUT) {
          // A planar surface: the lane's two U code words into the pair's U row and its two V code words into the V row, at
          // sample x / 2 of each -- one 16-bit store each for uint8 code words, one dword each for uint16 (the chroma planes
          // promise 2- / 4-byte alignment).
          // (4:2:2: the same stores into chroma row y.  4:4:4: four code words per plane at sample x of chroma row y, whole
          // dwords as the luma's -- a 4:4:4 chroma plane promises the luma's alignment.)
          if constexpr (CH == kChroma444) {
            char* uo = static_cast<char*>(const_cast<void*>(p.pout.u)) + (long long)b * p.pout.image_u +
                       (long long)yc * p.pout.pitch_u + (size_t)x * sizeof(TO);
            char* vo = static_cast<char*>(const_cast<void*>(p.pout.v)) + (long long)b * p.pout.image_v +
                       (long long)yc * p.pout.pitch_v + (size_t)x * sizeof(TO);
#pragma unroll
            for (int q = 0; q < S; ++q) {
              reinterpret_cast<uint32_t*>(uo)[q] = wu4[q];
              reinterpret_cast<uint32_t*>(vo)[q] = wv4[q];
            }
          } else if (r == ROWS - 1) {
            typedef std::conditional_t<S == 1, uint16_t, uint32_t> TW;  // two code words
            const size_t xc = (size_t)(x >> 1) * sizeof(TO);
            char* uo = static_cast<char*>(const_cast<void*>(p.pout.u)) + (long long)b * p.pout.image_u +
                       (long long)yc * p.pout.pitch_u + xc;
            char* vo = static_cast<char*>(const_cast<void*>(p.pout.v)) + (long long)b * p.pout.image_v +
                       (long long)yc * p.pout.pitch_v + xc;
            const uint32_t wu = yuv_chroma_code(fk, 1, csum[0][0], cmax, sh, CW) | (yuv_chroma_code(fk, 1, csum[1][0], cmax, sh, CW) << (8 * S));
            const uint32_t wv = yuv_chroma_code(fk, 2, csum[0][1], cmax, sh, CW) | (yuv_chroma_code(fk, 2, csum[1][1], cmax, sh, CW) << (8 * S));
            *reinterpret_cast<TW*>(uo) = (TW)wu;
            *reinterpret_cast<TW*>(vo) = (TW)wv;
          }
        } else if (r == ROWS - 1) {
          char* co = static_cast<char*>(const_cast<void*>(p.yout.uv)) + (long long)b * p.yout.image_uv +
                     (long long)yc * p.yout.pitch_uv + (size_t)x * sizeof(TO);
          [[maybe_unused]] uint32_t wc = 0;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const uint32_t uv = yuv_chroma_code(fk, 1, csum[h][0], cmax, sh, CW) | (yuv_chroma_code(fk, 2, csum[h][1], cmax, sh, CW) << (8 * S));
            if constexpr (S == 2) reinterpret_cast<uint32_t*>(co)[h] = uv;
            else wc |= uv << (16 * h);
          }
          if constexpr (S == 1) *reinterpret_cast<uint32_t*>(co) = wc;
        }
      }
    } else if constexpr (sizeof(TO) < 4) {
      // A quantised frame: tf.cast(255 * clip(out, 0, 1), uint8), truncation (hdrnet/bin/run.py:95) -- or, for a uint16
      // frame, (uint16)(out_white * clip(out, 0, 1)): the same multiply and truncation with a run-time white level.  The
      // samples of a lane's 4 pixels are whole dwords, contiguous across the wave: plain per-lane stores are already dense.
      // A packed frame has the input's own pixel format: colour channel c of pixel k goes where load_pixels found it, alpha
      // beside it (copied bit for bit; into a uint8 frame, the upper byte of a uint16 alpha).
      constexpr int S = (int)sizeof(TO), PER = 4 / S;  // bytes per sample; samples per dword
      constexpr int SO = PACKED ? SPX : COUT;          // samples per stored pixel of the output
      constexpr int NW = kPxPerThread * SO / PER;      // dwords per lane
      static_assert(S == 1 || COUT == 3, "16-bit output: the 3 -> 3 op");
      static_assert(S == 1 || !PACKED || sizeof(TI) == 2, "packed 16-bit output: from a uint16 frame");
      static_assert(kPxPerThread * SO % PER == 0, "whole dwords per thread");
      const float wl = S == 1 ? 255.0f : p.out_white;  // (uint8: a compile-time constant)
      if (active) {
        uint32_t w[NW];
#pragma unroll
        for (int q = 0; q < NW; ++q) w[q] = 0;
#pragma unroll
        for (int k = 0; k < kPxPerThread; ++k) {
#pragma unroll
          for (int i = 0; i < COUT; ++i) {
            const float c = __builtin_amdgcn_fmed3f(of[k * COUT + i], 0.0f, 1.0f);  // clip: folds into the affine's last fma (clamp)
            const int pos = PACKED ? px_sample(PX, k, i) : k * COUT + i;
            w[pos / PER] |= ((uint32_t)(wl * c)) << (8 * S * (pos % PER));
          }
          if constexpr (PACKED && SPX == 4)
            w[(4 * k + 3) / PER] |= ((int)sizeof(TI) > S ? alpha[k] >> 8 : alpha[k]) << (8 * S * ((4 * k + 3) % PER));
        }
        uint32_t* op = reinterpret_cast<uint32_t*>(static_cast<TO*>(p.out) + px * SO);
        if constexpr (PACKED && SPX == 4) {  // pixels with alpha: 16-byte stores (written out: a loop moved registers about)
          typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
          reinterpret_cast<u32x4*>(op)[0] = u32x4{w[0], w[1], w[2], w[3]};
          static_assert(NW == 4 * S, "one 16-byte store per lane for uint8 samples, two for uint16");
          if constexpr (S == 2) reinterpret_cast<u32x4*>(op)[1] = u32x4{w[4], w[5], w[6], w[7]};
        } else {
#pragma unroll
          for (int q = 0; q < NW; ++q) op[q] = w[q];
        }
      }
    } else {
      // float output: lane-contiguous nontemporal buffer stores through the per-wave LDS slab
      // (apply_fwd_seg.hip); the descriptor covers exactly the row segment
      float4* slab = reinterpret_cast<float4*>(lds + p.slab_off) + wave * (64 * COUT);
      if (active) {
#pragma unroll
        for (int q = 0; q < COUT; ++q)
          slab[lane * COUT + q] = make_float4(of[4 * q], of[4 * q + 1], of[4 * q + 2], of[4 * q + 3]);
      }
      wave_lds_sync();
      const unsigned wpx = kPxPerThread * 64u * (unsigned)wave;
      float* oseg = static_cast<float*>(p.out) + (row * p.W + xs) * COUT;
      store_slab_seg<COUT>(slab, oseg, (unsigned)(xe - xs), wpx, lane);
    }
  } while (ROWPAIR && ++r < ROWS);
}

// The curves instantiations keep their lookup tables in STATIC LDS: no launch passes those bytes, but the workgroup
// occupies them, so the geometry's `ok` budgets the largest static table of any instantiation.
constexpr int kStaticTabFloats = CurveTab<3>::kFloats > 3 * kCurveCells * 4 ? CurveTab<3>::kFloats : 3 * kCurveCells * 4;
static_assert(kStaticTabFloats == 768, "tests/test_row_geom.py and io_fits of tests/row_plan.py budget 768 floats of static tables");

// Launch geometry (row_geom.h): no dynamic tables in front of the image.
RowGeom io_geom(const ApplyIoArgs& a) {
  return io_fwd_geom(Frame{a.B, a.H, a.W, a.GW, a.GD}, a.Cout * (a.Cin + (a.has_offset ? 1 : 0)), a.Cout, 0,
                     kStaticTabFloats,
                     ptr_bits(a.grid, a.guide, a.guide_out, a.output_dtype == 0 ? a.out : nullptr,
                              a.input_dtype == 0 ? a.input : nullptr));
}

template <int CIN, int COUT, bool OFFSET, int GUIDE, typename TI, typename TO, int PX = kPxRGB, int OUT = kOutFrame,
          int CH = kChroma420, bool UPADD = false>
hipError_t launch_io(const ApplyIoArgs& a, hipStream_t s, const UpAdd* up = nullptr) {
  constexpr int C = COUT * (CIN + (OFFSET ? 1 : 0));
  const RowGeom g = io_geom(a);
  IoParamsOf<UPADD> p;
  p.grid = a.grid;
  p.guide = a.guide;
  p.input = a.input;
  p.out = a.out;
  p.H = a.H; p.W = a.W; p.GH = a.GH; p.GW = a.GW; p.GD = a.GD;
  p.seg = g.pl.seg;
  p.slab_off = g.slab_off;
  p.scale_x = (float)a.GW / a.W;
  p.scale_y = (float)a.GH / a.H;
  p.inv_col = 1.0f / (float)(a.GD * (C / 4));
  p.white = io_white_level(a.white_level);
  p.grid_image = a.GH * a.GW * a.GD * C;
  p.tab = make_seg_tab(a.W, g.pl.seg, g.pl.nseg, p.scale_x);
  p.gn = GuideNet{a.guide_conv1, a.guide_conv2, a.guide_shifts, a.guide_slopes, a.guide_out, a.n_feats, a.fast_sigmoid, a.guide_prescaled,
                     (a.guide_shifts && a.n_feats <= kCurveMaxKnots) ? a.guide_prepared : nullptr};
  p.yin = p.yout = YuvSurface{};
  p.to_rgb = p.from_rgb = nullptr;
  p.out_white = a.output_white_level;
  p.code_max = 0.0f;
  p.code_shift = 0;
  p.pin = p.pout = YuvPlanarSurface{};
  if constexpr (UPADD) p.up = *up;
  if constexpr (PX == kPxYuvPlanar) {
    p.pin = a.yuvp->in;
    p.to_rgb = a.yuvp->to_rgb;
    p.pout = a.yuvp->out;
    p.from_rgb = a.yuvp->from_rgb;
    if constexpr (OUT == kOutI016) p.code_max = (float)((1 << a.yuvp->out_bits) - 1);  // code_shift stays 0: low bits
  }
  if constexpr (PX == kPxYuvPacked) {
    p.kin = a.yuvk->in;
    p.to_rgb = a.yuvk->to_rgb;
    p.kout = a.yuvk->out;
    p.from_rgb = a.yuvk->from_rgb;
    if constexpr (OUT == kOutY216) {
      p.code_max = (float)((1 << a.yuvk->out_bits) - 1);
      p.code_shift = 16 - a.yuvk->out_bits;
    }
  }
  if constexpr (PX == kPxYuv) {
    p.yin = a.yuv->in;
    p.to_rgb = a.yuv->to_rgb;
    p.yout = a.yuv->out;
    p.from_rgb = a.yuv->from_rgb;
    if constexpr (OUT == kOutP016) {
      p.code_max = (float)((1 << a.yuv->out_bits) - 1);
      p.code_shift = 16 - a.yuv->out_bits;
    }
  }
  // a 4:2:0 surface output: one workgroup per row PAIR of a segment (H % 2 == 0); 4:2:2 / 4:4:4: per row, as a frame
  const dim3 grid3((unsigned)g.pl.nseg, (unsigned)(OUT != kOutFrame && CH == kChroma420 ? a.H / 2 : a.H), (unsigned)a.B);
  apply_fwd_io_rows<CIN, COUT, OFFSET, GUIDE, TI, TO, PX, OUT, CH, UPADD><<<grid3, g.pl.threads, g.lds, s>>>(p);
  return hipGetLastError();
}

template <int GUIDE, typename TI, typename TO, int PX = kPxRGB>
hipError_t dispatch_shape(const ApplyIoArgs& a, hipStream_t s) {
  if (a.Cin == 3 && a.Cout == 3 && a.has_offset) return launch_io<3, 3, true, GUIDE, TI, TO, PX>(a, s);
  return hipErrorInvalidValue;
}

template <int GUIDE, int PX = kPxRGB>
hipError_t dispatch_types(const ApplyIoArgs& a, hipStream_t s) {
  const int in = a.input_dtype, out = a.output_dtype;
  if (in == 1 && out == 1) return dispatch_shape<GUIDE, uint8_t, uint8_t, PX>(a, s);
  if (in == 1 && out == 0) return dispatch_shape<GUIDE, uint8_t, float, PX>(a, s);
  if (in == 2 && out == 1) return dispatch_shape<GUIDE, uint16_t, uint8_t, PX>(a, s);
  if (in == 2 && out == 0) return dispatch_shape<GUIDE, uint16_t, float, PX>(a, s);
  if constexpr (PX == kPxRGB) {  // float32 frames are RGB
    if (in == 0 && out == 1) return dispatch_shape<GUIDE, float, uint8_t>(a, s);
    if (in == 0 && out == 0) return dispatch_shape<GUIDE, float, float>(a, s);
  }
  return hipErrorInvalidValue;
}

// The guide source a call selects (the same decision for every pixel format).
inline int io_guide_form(const ApplyIoArgs& a) {
  if (a.guide) return kGuideMap;
  if (!a.guide_shifts) return kGuideNN;
  if (a.n_feats > kCurveMaxKnots) return kGuideCurvesScan;  // knot by knot
  return a.guide_prepared ? kGuideCurvesCells : kGuideCurves;
}

// ... as a compile-time constant: f(std::integral_constant<int, GUIDE>) with the call's guide form.  Every translation
// unit's launch goes through this one switch.
template <class F>
hipError_t with_guide_form(const ApplyIoArgs& a, F&& f) {
  switch (io_guide_form(a)) {
    case kGuideMap: return f(std::integral_constant<int, kGuideMap>{});
    case kGuideNN: return f(std::integral_constant<int, kGuideNN>{});
    case kGuideCurves: return f(std::integral_constant<int, kGuideCurves>{});
    case kGuideCurvesCells: return f(std::integral_constant<int, kGuideCurvesCells>{});
    default: return f(std::integral_constant<int, kGuideCurvesScan>{});
  }
}

template <int PX>
hipError_t dispatch_guides(const ApplyIoArgs& a, hipStream_t s) {
  return with_guide_form(a, [&](auto guide) { return dispatch_types<decltype(guide)::value, PX>(a, s); });
}

// The name hdrnet_last_kernel reports: apply_fwd_io/<in>-><out><guide form><pixel format>, of the call's thread.
inline const char* io_label(const ApplyIoArgs& a) {
  static const char* const frame[3] = {"f32", "u8", "u16"};           // input_dtype / output_dtype
  static const char* const surface[4] = {"f32", "u8", "nv12", "p016"};  // YuvIo::out_kind
  static const char* const suffix[5] = {"", "+nnguide", "+curvesguide", "+curvesguide/scan", "+curvesguide/cells"};
  static const char* const px[4] = {"", "/bgr", "/rgba", "/bgra"};
  static thread_local char label[64];
  // a 4:2:2 / 4:4:4 surface (include/hdrnet_amd_yuv_chroma.h): container, layout and sample width -- nv16 / p216 semi-planar,
  // i422 / i216 / i444 / i416 planar
  // a packed 4:2:2 surface (include/hdrnet_amd_yuv_packed.h): byte order and sample width -- yuy2 / uyvy / yvyu, y216
  if (a.yuvk) {
    static const char* const order[3] = {"yuy2", "uyvy", "yvyu"};
    const char* const in = a.input_dtype == 2 ? "y216" : order[a.yuvk->in.order];
    snprintf(label, sizeof label, "apply_fwd_io/%s->%s%s", in, a.yuvk->out_kind >= 2 ? in : surface[a.yuvk->out_kind],
             suffix[io_guide_form(a)]);
  } else if (a.yuvp && a.yuvp->chroma != kChroma420) {
    static const char* const planar[2][2] = {{"i422", "i216"}, {"i444", "i416"}};
    const char* const in = planar[a.yuvp->chroma == kChroma444][a.input_dtype == 2];
    snprintf(label, sizeof label, "apply_fwd_io/%s->%s%s", in,
             a.yuvp->out_kind == kYuvPlanarOutPlanar ? in : surface[a.yuvp->out_kind], suffix[io_guide_form(a)]);
  } else if (a.yuv && a.yuv->chroma != kChroma420) {
    static const char* const surface422[4] = {"f32", "u8", "nv16", "p216"};
    snprintf(label, sizeof label, "apply_fwd_io/%s->%s%s", a.input_dtype == 1 ? "nv16" : "p216", surface422[a.yuv->out_kind],
             suffix[io_guide_form(a)]);
  } else if (a.yuvp) {  // a planar surface: the label states the sample WIDTH (i420 uint8, i016 uint16), as p016 does
    const char* const in = a.input_dtype == 1 ? "i420" : "i016";
    snprintf(label, sizeof label, "apply_fwd_io/%s->%s%s", in,
             a.yuvp->out_kind == kYuvPlanarOutPlanar ? in : surface[a.yuvp->out_kind], suffix[io_guide_form(a)]);
  } else if (a.yuv)
    snprintf(label, sizeof label, "apply_fwd_io/%s->%s%s", a.input_dtype == 1 ? "nv12" : "p016", surface[a.yuv->out_kind],
             suffix[io_guide_form(a)]);
  else
    snprintf(label, sizeof label, "apply_fwd_io/%s->%s%s%s", frame[a.input_dtype], frame[a.output_dtype],
             suffix[io_guide_form(a)], px[a.pixel_format]);
  return label;
}

// What every predicate asks of a FRAME: the 3 -> 3 op with offset, whole dwords per lane of quantised pixels, the packed
// formats on integer frames only -- with alpha, one 16-byte access per lane each way -- and a launch geometry that fits.
inline bool io_frame_ok(const ApplyIoArgs& a) {
  if (!(a.Cin == 3 && a.Cout == 3 && a.has_offset)) return false;
  if (((uintptr_t)a.input | (uintptr_t)a.out) & 3u) return false;
  if (a.pixel_format != kPxRGB) {
    if (a.pixel_format < 0 || a.pixel_format > kPxBGRA || a.input_dtype == 0) return false;
    if (px_stored(a.pixel_format) == 4 && (((uintptr_t)a.input | (a.output_dtype != 0 ? (uintptr_t)a.out : 0)) & 15u)) return false;
  }
  return io_geom(a).ok;
}

// ... and of a YUV SURFACE: the same op, whole row pairs (4:2:0) and lanes, the same geometry.
inline bool io_surface_ok(const ApplyIoArgs& a, int chroma = kChroma420) {
  return a.Cin == 3 && a.Cout == 3 && a.has_offset && (chroma != kChroma420 || a.H % 2 == 0) && a.W % 4 == 0 && io_geom(a).ok;
}

}  // namespace

// apply_fwd_io_px.hip: the same launch for a frame in BGR, RGBA or BGRA order (a.pixel_format != 0)
hipError_t launch_apply_fwd_io_px(const ApplyIoArgs& a, hipStream_t s);
// apply_fwd_io_yuv.hip (launch.hip.h): the same launch for a YUV surface (a.yuv)
// apply_fwd_io_u16.hip (launch.hip.h): the same launch with a 16-bit output (a.output_dtype == 2)
// apply_fwd_io_yuv_planar.hip (launch.hip.h): the same launch for a planar YUV surface (a.yuvp)
// apply_fwd_io_yuv_422.hip, apply_fwd_io_yuv_planar_422.hip / _444.hip (launch.hip.h): ... of another chroma layout
// apply_fwd_io_yuv_packed.hip (launch.hip.h): the same launch for a packed 4:2:2 surface (a.yuvk)
// apply_fwd_io_upadd_yuv.hip (launch.hip.h): the same launch for a 4:2:0 surface + the pyramid's up-add (`coarse`)

}  // namespace hdrnet_amd
