// The finest level of the pyramid model with the product's WIRE FORMATS fused in: the wire-format forward of
// apply_fwd_io.hip with the bilinear (align_corners) up-add of the coarser level's output applied to a lane's 4 pixels
// before the store -- what apply_fwd_seg.hip does under UPADD (hdrnet/models.py:283-287; upadd_quad, rows_common.hip.h):
//   out = wire_out(slice_apply(grid, guide, input / white_level) + resize_bilinear(coarse -> H x W))
// with wire_out = identity (float32) or (uint8)(255 * clip(., 0, 1)) (hdrnet/bin/run.py:95) -- the clip AFTER the add.
// At 4K the level moves 3 + 3 B/px (uint8 both ways) instead of 12 + 12, plus the quarter-size coarse level from L2.
//
// A file of its own, so that the instantiations of apply_fwd_io.hip keep their device code: geometry (apply_fwd_io_geom:
// the same RowGeom for predicate and launcher), LDS image, pixel phase, white level (FOLD_WL with a guide map) and the
// two store forms are that file's; the up-add touches of[] only and uses no LDS.  Cin = Cout = 3 with offset; the guide
// is a map or the folded point-wise guide network (the curves guide belongs to the single-level models).
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <cstdio>

#include "launch.hip.h"
#include "numerics.hip.h"
#include "rows_common.hip.h"
#include "seg_common.hip.h"
#include "white_level.hip.h"

namespace hdrnet_amd {
namespace {

using namespace rows;

struct IoUpParams {
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
  GuideNN gn;      // GUIDE_NN: the folded point-wise guide network (rows_common.hip.h)
  UpAdd up;        // the coarser pyramid level to up-sample and add
};

template <bool GUIDE_NN, typename TI, typename TO>
__global__ __launch_bounds__(256) void apply_fwd_io_upadd_rows(const IoUpParams p) {
  constexpr int CIN = 3, COUT = 3, C = COUT * (CIN + 1);
  constexpr int CB = C * (int)sizeof(float);
  constexpr int NI = CIN * kPxPerThread, NO = COUT * kPxPerThread;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // integer samples with a guide MAP feed the affine only: the white level goes into the staged coefficients
  constexpr bool FOLD_WL = !GUIDE_NN && sizeof(TI) < 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int xs = blockIdx.x * p.seg;
  const int xe = min(xs + p.seg, p.W);
  const int y = blockIdx.y;
  const int b = blockIdx.z;
  const float* grid_b = p.grid + (size_t)b * (unsigned)p.grid_image;
  const int x = xs + kPxPerThread * tid;
  const bool active = x < xe;
  const size_t row = (unsigned)b * (unsigned)p.H + (unsigned)y;  // B, H <= 65535 (kLimBH, row_geom.h)
  const size_t px = row * p.W + x;

  float gs[kPxPerThread] = {0.f, 0.f, 0.f, 0.f};
  float inf[NI];
#pragma unroll
  for (int q = 0; q < NI; ++q) inf[q] = 0.0f;
  if (active) {
    if constexpr (!GUIDE_NN) {
      const float4 g4 = *reinterpret_cast<const float4*>(p.guide + px);
      gs[0] = g4.x; gs[1] = g4.y; gs[2] = g4.z; gs[3] = g4.w;
    }
    load_pixels<TI, NI, FOLD_WL>(static_cast<const TI*>(p.input), px * CIN, p.white, inf);
  }
  const SegCols sc = seg_cols_tab(p.tab, blockIdx.x, xs, xe, p.scale_x);
  const int colb = (p.GD + 2) * CB;
  const float gd_f = (float)p.GD, zhi = (float)(p.GD - 1);
  stage_image<C, FOLD_WL>(lds, grid_b, y, sc.cmin, sc.ncols, p.GH, p.GW, p.GD, p.scale_y, p.inv_col, tid, (int)blockDim.x,
                          p.white.inv);
  XTermLean xt[kPxPerThread];
  const float xf0 = (float)x + 0.5f;  // xf0 + k == (x + k) + 0.5f exactly: x < W <= 2^23 (row_geom.h, kMaxFloatX)
  const float colb_f = (float)colb, xbase_f = (float)(CB - sc.cmin * colb);
#pragma unroll
  for (int k = 0; k < kPxPerThread; ++k) xt[k] = x_term_lean(xf0 + (float)k, p.scale_x, colb_f, xbase_f);
  __syncthreads();

  float of[NO];
  if (active) {
    if constexpr (GUIDE_NN) guide_nn_quad<CIN>(p.gn, inf, gs);
#pragma unroll
    for (int k = 0; k < kPxPerThread; ++k) {
      float in[CIN], o[COUT];
#pragma unroll
      for (int j = 0; j < CIN; ++j) in[j] = inf[k * CIN + j];
      seg_pixel_lean<CIN, COUT, true, true>(lds, gd_f, zhi, colb, xt[k], gs[k], in, o);
#pragma unroll
      for (int i = 0; i < COUT; ++i) of[k * COUT + i] = o[i];
    }
    upadd_quad<COUT>(p.up, b, y, x, of);
  }

  if constexpr (sizeof(TO) == 1) {
    // tf.cast(255 * clip(out, 0, 1), uint8): truncation; 12 bytes per lane, contiguous across the wave
    if (active) {
      uint32_t w[NO / 4];
#pragma unroll
      for (int q = 0; q < NO / 4; ++q) w[q] = 0;
#pragma unroll
      for (int q = 0; q < NO; ++q) {
        const float c = __builtin_amdgcn_fmed3f(of[q], 0.0f, 1.0f);
        w[q >> 2] |= ((uint32_t)(255.0f * c)) << (8 * (q & 3));
      }
      uint32_t* op = reinterpret_cast<uint32_t*>(static_cast<TO*>(p.out) + px * COUT);
#pragma unroll
      for (int q = 0; q < NO / 4; ++q) op[q] = w[q];
    }
  } else {
    // float output: lane-contiguous nontemporal buffer stores through the per-wave LDS slab; the descriptor covers
    // exactly the row segment
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
}

template <bool GUIDE_NN, typename TI, typename TO>
hipError_t launch_io_upadd(const ApplyIoArgs& a, const UpAdd& up, hipStream_t s) {
  constexpr int C = 12;
  const RowGeom g = apply_fwd_io_geom(a);
  IoUpParams p;
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
  p.gn = GuideNN{a.guide_conv1, a.guide_conv2, nullptr, a.n_feats, a.fast_sigmoid, a.guide_prescaled};
  p.up = up;
  const dim3 grid3((unsigned)g.pl.nseg, (unsigned)a.H, (unsigned)a.B);
  apply_fwd_io_upadd_rows<GUIDE_NN, TI, TO><<<grid3, g.pl.threads, g.lds, s>>>(p);
  return hipGetLastError();
}

template <bool GUIDE_NN>
hipError_t dispatch_types(const ApplyIoArgs& a, const UpAdd& up, hipStream_t s) {
  const int in = a.input_dtype, out = a.output_dtype;
  if (in == 1 && out == 1) return launch_io_upadd<GUIDE_NN, uint8_t, uint8_t>(a, up, s);
  if (in == 1 && out == 0) return launch_io_upadd<GUIDE_NN, uint8_t, float>(a, up, s);
  if (in == 2 && out == 1) return launch_io_upadd<GUIDE_NN, uint16_t, uint8_t>(a, up, s);
  if (in == 2 && out == 0) return launch_io_upadd<GUIDE_NN, uint16_t, float>(a, up, s);
  if (in == 0 && out == 1) return launch_io_upadd<GUIDE_NN, float, uint8_t>(a, up, s);
  return hipErrorInvalidValue;  // float32 -> float32 is launch_apply_fwd_upadd's (apply_fwd_rows.hip)
}

}  // namespace

// The wire-format forward's own predicate (one geometry: apply_fwd_io_geom) + a coarse level readable dword by dword.
bool apply_fwd_io_upadd_supported(const ApplyIoArgs& a, const float* coarse) {
  if (a.guide_shifts || a.guide_out || ((uintptr_t)coarse & 3u)) return false;
  return apply_fwd_io_supported(a);
}

hipError_t launch_apply_fwd_io_upadd(const ApplyIoArgs& a, const float* coarse, int Hc, int Wc, hipStream_t s,
                                     const char** name) {
  if (!apply_fwd_io_upadd_supported(a, coarse) || (a.input_dtype == 0 && a.output_dtype == 0)) return hipErrorInvalidValue;
  static const char* const io[3][2] = {{"f32->f32", "f32->u8"}, {"u8->f32", "u8->u8"}, {"u16->f32", "u16->u8"}};
  static thread_local char label[64];
  snprintf(label, sizeof label, "apply_fwd_io/%s%s+upadd", io[a.input_dtype][a.output_dtype], a.guide ? "" : "+nnguide");
  *name = label;
  const UpAdd up{coarse, Hc, Wc, resize_scale(Hc, a.H), resize_scale(Wc, a.W)};
  return a.guide ? dispatch_types<false>(a, up, s) : dispatch_types<true>(a, up, s);
}

}  // namespace hdrnet_amd
