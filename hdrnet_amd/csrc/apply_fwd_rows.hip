// BilateralSliceApply forward for gfx950 -- the north-star kernel.
//
// Reference semantics: hdrnet/ops/bilateral_slice_apply.cc:24-82 (the CUDA twin,
// bilateral_slice_apply.cu.cc:36-126, assigns one thread per output CHANNEL and
// re-derives all weights for each of its 32 scattered grid loads).
//
// Design: the op is a pure HBM stream -- 4 B guide + 4*Cin B input
// in, 4*Cout B out per pixel -- next to a 96 KiB grid that never leaves L2.  So:
//   * a workgroup owns one SEGMENT OF ONE IMAGE ROW.  For a row, gy0/gy1 and the
//     two y-weights are wave-uniform scalars, so the workgroup first blends the two
//     grid rows it needs into LDS ("y-pre-lerp": colY[gx][gz][c] =
//     wy0*grid[gy0c][gx] + wy1*grid[gy1c][gx], only the gx columns the segment
//     touches).  A pixel then gathers 2(x) x 2(z) coefficient vectors instead of 8.
//   * the LDS image keeps the grid's own [gx][gz][c] order: one (gx,gz) vector is
//     C contiguous floats (48 B for C=12), read as ds_read_b128.  With a 48-B
//     stride the eight gz vectors of a column start at dword banks
//     {0,12,24,36,48,60,8,20} mod 64 -- disjoint 4-bank slots -- so the
//     data-dependent gz gather is conflict-free across a 16-lane b128 group.
//   * a thread owns 4 CONSECUTIVE pixels: guide is one 16-B load, input and output
//     are three 16-B loads / stores each (global_load/store_dwordx4), all issued
//     before the arithmetic; rows are contiguous so every wave streams a dense
//     3 KiB span.  (Scalar variant for W % 4 != 0 or unaligned pointers.)
//   * per pixel: 2 sqrt (the reference: 96), 4 weights, 4*C FMAs for the blend,
//     Cout*Cj FMAs for the affine.  No MFMA: this is a gather/interpolate with 8
//     non-zeros per pixel, not a dense contraction.
//
// Numerics: same coordinate / weight expressions as the reference, evaluated in
// the same order; the only re-association is wy folded into the LDS image, i.e.
// (wy0*g0 + wy1*g1)*(wx*wz) instead of sum((wx*wy)*wz*g).  Differences stay at the
// 1e-7 relative level (tests/test_gpu_parity.py holds rtol=atol=1e-5 and reports
// the reference's own 1e-6 bar).
//
// The alternatives that were measured and rejected (one wave per tile, persistent stream, per-lane stores,
// nontemporal lane-contiguous loads) are not in the tree: DESIGN.md section 4 records why they lost.  The tools
// build keeps two memory skeletons (apply_fwd_skeletons.hip) and can select this file's vec4 kernel as variant 19.
//
// Is the plain apply_fwd_rows_vec4 still reachable in the product once apply_fwd_seg has refused?  Yes.  Both
// predicates ask for a fast shape and read the same Plan (geom_for here, seg_geom there: the same pointers, so the same
// Plan::vec4), but their limits differ (row_geom.h: kSegLimits against kRowsLimits):
//   * LDS.  seg_fwd_geom budgets the PADDED image (seg_cols_for columns, unclamped, of GD + 2 planes) and a slab of
//     guide + input per wave; rows_fwd_geom the clamped one (at most GW columns of GD planes) and a slab without the
//     guide.  3 -> 3 with offset at W = 1024, GW = 64, GD = 16 (one segment of 256 threads): 67 x 18 x 48 B + 16 KB of
//     slabs = 74 272 B, refused against the 64 KB budget; here 64 x 16 x 48 B + 16 B + 12 KB = 61 456 B, served.
//   * the 3-D launch grid.  B or H above 65535 (kLimBH) is refused there; the 1-D grid here takes it (kLimBlocks).
// So the kernel is the product's for deep grids under wide segments and for very tall frames, not only variant 19.
#include <hip/hip_runtime.h>

#include "launch.hip.h"
#include "numerics.hip.h"
#include "rows_common.hip.h"
namespace hdrnet_amd {
namespace {

using namespace rows;

// ---- 4 consecutive pixels per thread, 16-byte global accesses -----------------------
// Requires W % 4 == 0, seg % 4 == 0 and 16-B aligned guide / input / out.
template <int CIN, int COUT, bool OFFSET, bool GUIDE_NN = false, bool UPADD = false>
__global__ __launch_bounds__(256) void apply_fwd_rows_vec4(
    const float* __restrict__ grid, const float* __restrict__ guide,
    const float* __restrict__ input, float* __restrict__ out, int H, int W, int GH, int GW,
    int GD, int nseg, int seg, int slab_offset_floats, float scale_x, float scale_y,
    GuideNN gn = GuideNN{nullptr, nullptr, nullptr, 0}, UpAdd up = UpAdd{nullptr, 0, 0, 0.f, 0.f}) {
  constexpr int C = COUT * (CIN + (OFFSET ? 1 : 0));
  extern __shared__ __attribute__((aligned(16))) float colY[];
  const int bid = blockIdx.x;
  const int segi = bid % nseg;
  const int row = bid / nseg;  // = b * H + y
  const int y = row % H;
  const int b = row / H;
  const int xs = segi * seg;
  const int xe = min(xs + seg, W);
  const float* grid_b = grid + (size_t)b * GH * GW * GD * C;

  const int x = xs + kPxPerThread * threadIdx.x;
  const bool active = x < xe;
  const size_t p = (size_t)row * W + x;

  // Issue this thread's streaming loads before the staging pass so their HBM
  // latency overlaps the (L2-resident) grid reads and the barrier.
  const int lane = threadIdx.x & 63;
  const int wave_x0 = xs + kPxPerThread * (int)(threadIdx.x & ~63u);
  const int wave_px = min(xe, wave_x0 + 64 * kPxPerThread) - wave_x0;  // <= 0 for an idle wave
  float4* slab = reinterpret_cast<float4*>(colY + slab_offset_floats) +
                 (threadIdx.x >> 6) * (64 * (CIN > COUT ? CIN : COUT));
  float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 iv[(CIN * kPxPerThread) / 4];
  if (active) {
    if constexpr (!GUIDE_NN) g4 = *reinterpret_cast<const float4*>(guide + p);
    const float4* ip = reinterpret_cast<const float4*>(input + p * CIN);
#pragma unroll
    for (int q = 0; q < (CIN * kPxPerThread) / 4; ++q) iv[q] = ip[q];
  }

  const RowCtx r = stage_row<C, false>(colY, grid_b, y, xs, xe, GH, GW, GD, scale_x, scale_y);

  float gs[4] = {g4.x, g4.y, g4.z, g4.w};
  const float xf0 = (float)x + 0.5f;  // (x + k) + 0.5f == xf0 + k exactly: x < W <= 2^23 (row_geom.h, kMaxFloatX)
  const float* inf = reinterpret_cast<const float*>(iv);
  float4 ov[(COUT * kPxPerThread) / 4];
  float* of = reinterpret_cast<float*>(ov);
  if (active) {
    if constexpr (GUIDE_NN) {
      guide_nn_quad<CIN>(gn, inf, gs);
      if (gn.guide_out) *reinterpret_cast<float4*>(gn.guide_out + p) = make_float4(gs[0], gs[1], gs[2], gs[3]);
    }
#pragma unroll
    for (int k = 0; k < kPxPerThread; ++k) {
      float in[CIN], o[COUT];
#pragma unroll
      for (int j = 0; j < CIN; ++j) in[j] = inf[k * CIN + j];
      slice_apply_pixel<CIN, COUT, OFFSET>(r, xf0 + (float)k, gs[k], in, o);
#pragma unroll
      for (int i = 0; i < COUT; ++i) of[k * COUT + i] = o[i];
    }
    if constexpr (UPADD) upadd_quad<COUT>(up, b, y, x, of);
  }
  // Store phase.  A lane's 4 pixels are 4*COUT contiguous floats, i.e. per-lane 16-B
  // stores at a 16*COUT-byte stride -- measured 6.5 us slower per 4K frame than
  // lane-contiguous stores (the LOADS do not care).  So each wave transposes its tile
  // through a private LDS slab: ds_write_b128 at the per-pixel stride (conflict-free:
  // 12-dword stride over 8-lane groups), then lane l reads float4 number l + 64k and
  // stores it -- every global_store_dwordx4 covers one dense 1 KiB run.
  if (active) {
#pragma unroll
    for (int q = 0; q < COUT; ++q) slab[lane * COUT + q] = ov[q];
  }
  wave_lds_sync();
  // nontemporal buffer stores on a descriptor over exactly this wave's run (rows_common.hip.h)
  store_slab_run<COUT>(slab, out + ((size_t)row * W + wave_x0) * COUT, wave_px, lane);
}

// ---- scalar variant: any W / alignment; thread t takes pixels xs + t + k*blockDim ------
template <int CIN, int COUT, bool OFFSET>
__global__ __launch_bounds__(256) void apply_fwd_rows_scalar(
    const float* __restrict__ grid, const float* __restrict__ guide,
    const float* __restrict__ input, float* __restrict__ out, int H, int W, int GH, int GW,
    int GD, int nseg, int seg, float scale_x, float scale_y) {
  constexpr int C = COUT * (CIN + (OFFSET ? 1 : 0));
  extern __shared__ __attribute__((aligned(16))) float colY[];
  const int bid = blockIdx.x;
  const int segi = bid % nseg;
  const int row = bid / nseg;
  const int y = row % H;
  const int b = row / H;
  const int xs = segi * seg;
  const int xe = min(xs + seg, W);
  const float* grid_b = grid + (size_t)b * GH * GW * GD * C;
  const size_t prow = (size_t)row * W;

  float gs[kPxPerThread];
  float in[kPxPerThread][CIN];
#pragma unroll
  for (int k = 0; k < kPxPerThread; ++k) {
    const int x = xs + threadIdx.x + k * blockDim.x;
    if (x < xe) {
      gs[k] = guide[prow + x];
#pragma unroll
      for (int j = 0; j < CIN; ++j) in[k][j] = input[(prow + x) * CIN + j];
    }
  }

  const RowCtx r = stage_row<C, false>(colY, grid_b, y, xs, xe, GH, GW, GD, scale_x, scale_y);

#pragma unroll
  for (int k = 0; k < kPxPerThread; ++k) {
    const int x = xs + threadIdx.x + k * blockDim.x;
    if (x < xe) {
      float o[COUT];
      slice_apply_pixel<CIN, COUT, OFFSET>(r, (float)x + 0.5f, gs[k], in[k], o);
#pragma unroll
      for (int i = 0; i < COUT; ++i) out[(prow + x) * COUT + i] = o[i];
    }
  }
}

// Launch geometry (row_geom.h).  A fused guide network reads no guide buffer: its callers pass a.guide = a.input.
RowGeom geom_for(const ApplyArgs& a) {
  return rows_fwd_geom(Frame{a.B, a.H, a.W, a.GW, a.GD}, a.Cin, a.Cout, a.Cj, ptr_bits(a.guide, a.input, a.out, a.grid));
}

unsigned nblocks_of(const ApplyArgs& a, const RowGeom& g) { return (unsigned)((long long)a.B * a.H * g.pl.nseg); }

// One launch of the vec4 kernel, whichever FLAVOUR (GUIDE_NN, UPADD): the kernel's argument list.
template <int CIN, int COUT, bool OFFSET, bool... FLAVOUR>
hipError_t launch_vec4(const ApplyArgs& a, const RowGeom& g, const float* guide, hipStream_t s,
                       const GuideNN& gn = GuideNN{nullptr, nullptr, nullptr, 0},
                       const UpAdd& up = UpAdd{nullptr, 0, 0, 0.f, 0.f}) {
  apply_fwd_rows_vec4<CIN, COUT, OFFSET, FLAVOUR...><<<nblocks_of(a, g), g.pl.threads, g.lds, s>>>(
      a.grid, guide, a.input, a.out, a.H, a.W, a.GH, a.GW, a.GD, g.pl.nseg, g.pl.seg, g.slab_off,
      (float)a.GW / a.W, (float)a.GH / a.H, gn, up);
  return hipGetLastError();
}

template <int CIN, int COUT, bool OFFSET>
hipError_t launch_t(const ApplyArgs& a, hipStream_t s, const char** name) {
  const RowGeom g = geom_for(a);
  *name = g.pl.vec4 ? "apply_fwd_rows/vec4" : "apply_fwd_rows/scalar";
  if (g.pl.vec4) return launch_vec4<CIN, COUT, OFFSET>(a, g, a.guide, s);
  apply_fwd_rows_scalar<CIN, COUT, OFFSET><<<nblocks_of(a, g), g.pl.threads, g.lds, s>>>(
      a.grid, a.guide, a.input, a.out, a.H, a.W, a.GH, a.GW, a.GD, g.pl.nseg, g.pl.seg, (float)a.GW / a.W,
      (float)a.GH / a.H);
  return hipGetLastError();
}

template <bool GUIDE_NN>
hipError_t launch_upadd_t(const ApplyArgs& a, const GuideNN& gn, const float* coarse, int Hc, int Wc,
                          hipStream_t s) {
  const UpAdd up{coarse, Hc, Wc, resize_scale(Hc, a.H), resize_scale(Wc, a.W)};
  return launch_vec4<3, 3, true, GUIDE_NN, true>(a, geom_for(a), a.guide, s, gn, up);
}

// A fast shape whose geometry fits; `vec4`: ... and that the vec4 kernel serves (the fused forwards have no scalar twin).
bool rows_supported(const ApplyArgs& a, bool vec4) {
  if (!apply_fast_shape(a.Cin, a.Cout, a.has_offset)) return false;
  // stage_row reads the grid as float4 when C % 4 == 0.
  if ((a.Cout * a.Cj) % 4 == 0 && ((uintptr_t)a.grid & 15u)) return false;
  const RowGeom g = geom_for(a);
  return g.ok && (g.pl.vec4 || !vec4);
}

}  // namespace

// Fused point-wise-NN guide + slice-apply.  Same shape support as the vec4 row kernel.
bool apply_fwd_nnguide_supported(const ApplyArgs& a, const float* guide_out) {
  if (!((a.Cin == 3 && a.Cout == 3) || (a.Cin == 1 && a.Cout == 1))) return false;
  ApplyArgs t = a;
  t.guide = a.input;  // alignment check stand-in: no guide buffer is read
  if ((uintptr_t)guide_out & 15u) return false;
  return rows_supported(t, true);
}

hipError_t launch_apply_fwd_nnguide(const ApplyArgs& a, const float* conv1, const float* conv2,
                                    int n_feats, float* guide_out, hipStream_t s,
                                    const char** name) {
  if (apply_fwd_seg_nnguide_supported(a, guide_out)) {
    const hipError_t e = launch_apply_fwd_seg_nnguide(a, conv1, conv2, n_feats, guide_out, s, name);
    if (e != hipErrorNotSupported) return e;  // (a network too wide for its LDS copy falls through)
  }
  const GuideNN gn{conv1, conv2, guide_out, n_feats, a.fast_sigmoid, a.guide_prescaled};
  ApplyArgs t = a;
  t.guide = a.input;
  *name = "apply_fwd_rows/vec4+nnguide";
  const RowGeom g = geom_for(t);
  if (a.Cin == 3 && a.Cout == 3 && a.has_offset) return launch_vec4<3, 3, true, true>(t, g, nullptr, s, gn);
  if (a.Cin == 3 && a.Cout == 3 && !a.has_offset) return launch_vec4<3, 3, false, true>(t, g, nullptr, s, gn);
  if (a.Cin == 1 && a.Cout == 1 && a.has_offset) return launch_vec4<1, 1, true, true>(t, g, nullptr, s, gn);
  if (a.Cin == 1 && a.Cout == 1 && !a.has_offset) return launch_vec4<1, 1, false, true>(t, g, nullptr, s, gn);
  return hipErrorInvalidValue;
}

// Slice-apply (+ optional fused guide network) + bilinear up-add of the coarser pyramid level.
// One specialisation: Cin = Cout = 3 with offset (the reference's pyramid model), vec4 geometry.
bool apply_fwd_upadd_supported(const ApplyArgs& a, const float* coarse, bool guide_nn) {
  if (!(a.Cin == 3 && a.Cout == 3 && a.has_offset) || ((uintptr_t)coarse & 3u)) return false;
  ApplyArgs t = a;
  if (guide_nn) t.guide = a.input;
  return rows_supported(t, true);
}

hipError_t launch_apply_fwd_upadd(const ApplyArgs& a, const float* coarse, int Hc, int Wc,
                                  const float* conv1, const float* conv2, int n_feats,
                                  hipStream_t s, const char** name) {
  if (apply_fwd_seg_upadd_supported(a, coarse, conv1 != nullptr)) {
    const hipError_t e = launch_apply_fwd_seg_upadd(a, coarse, Hc, Wc, conv1, conv2, n_feats, s, name);
    if (e != hipErrorNotSupported) return e;
  }
  if (conv1) {
    const GuideNN gn{conv1, conv2, nullptr, n_feats, a.fast_sigmoid, a.guide_prescaled};
    ApplyArgs t = a;
    t.guide = a.input;  // alignment stand-in: no guide buffer is read
    *name = "apply_fwd_rows/vec4+nnguide+upadd";
    return launch_upadd_t<true>(t, gn, coarse, Hc, Wc, s);
  }
  *name = "apply_fwd_rows/vec4+upadd";
  return launch_upadd_t<false>(a, GuideNN{nullptr, nullptr, nullptr, 0}, coarse, Hc, Wc, s);
}

bool apply_fwd_rows_supported(const ApplyArgs& a) { return rows_supported(a, false); }

hipError_t launch_apply_fwd_rows(const ApplyArgs& a, hipStream_t s, const char** name) {
#ifdef HDRNET_TOOLS_BUILD
  const bool round1_kernel = a.variant == 19;  // A/B: the round-1 product kernel below
#else
  const bool round1_kernel = false;
#endif
  // The product kernel for vec4-able inputs lives in apply_fwd_seg.hip; what remains here is the
  // scalar kernel (any W / alignment) and the fused guide-network / pyramid instantiations.
  if (!round1_kernel && apply_fwd_seg_supported(a)) return launch_apply_fwd_seg(a, s, name);
#define HDRNET_CASE(CI, CO, OFF) \
  if (a.Cin == CI && a.Cout == CO && a.has_offset == OFF) return launch_t<CI, CO, OFF>(a, s, name);
  HDRNET_APPLY_FAST_SHAPES(HDRNET_CASE)
#undef HDRNET_CASE
  return hipErrorInvalidValue;
}

}  // namespace hdrnet_amd
