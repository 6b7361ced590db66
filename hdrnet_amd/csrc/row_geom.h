// Launch geometry of the "workgroup owns a segment of an image row" kernels: how a row is cut
// into segments, how large the LDS image of grid columns and the per-wave slabs behind it are, the dynamic-LDS bytes of
// the launch and the limits under which the kernel may run.  ONE place: a `*_supported` predicate and its launcher call
// the same function below with the same arguments and read the same result.
//
// Plain C++17, no HIP and no device code: a host compiler builds it alone (tests/test_row_geom.py).
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace hdrnet_amd {
namespace rows {

constexpr int kPxPerThread = 4;
constexpr int kWaveRun = 64 * kPxPerThread;  // pixels of a wavefront's run
constexpr size_t kMaxLdsBytes = 64 * 1024;   // the LDS budget of a workgroup: keep >= 2 workgroups per CU
inline bool lds_fits(size_t bytes) { return bytes <= kMaxLdsBytes; }

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// The widest row whose pixel centres are formed in float32 lane by lane.  The kernels that give a lane four consecutive
// pixels compute xf0 = (float)x + 0.5f once and take xf0 + k for pixel x + k: equal to the reference's (x + k) + 0.5f
// while x + 0.5 is exact, i.e. for x < 2^23; beyond, the two round differently (ties to even).  The gradient pass
// (grid_grad_mfma.hip) cuts a row into column intervals with the same float coordinate and forms a pixel's byte offset
// with a 24-bit multiply.  None of them runs a wider row: Plan::vec4 is false there and gg_plan refuses.
constexpr int kMaxFloatX = 1 << 23;

// Grid columns `npx` consecutive pixels can touch: floor differences of gx0 over npx-1 pixels (<= floor(d)+1), +1 for
// the upper neighbour, +1 for the count, +1 slack for float rounding of the coordinates.  Unclamped: the padded image
// of the segment family materialises the clamped copies.
inline long long seg_cols_for(int npx, int GW, int W) { return ((long long)(npx - 1) * GW) / W + 4; }

// ... and never more than GW: the row family stages clamped columns.
inline int max_cols_for(int npx, int GW, int W) {
  const long long cols = seg_cols_for(npx, GW, W);
  return (int)(cols < GW ? cols : GW);
}

// How a row is cut into workgroup segments: `threads` lanes x 4 pixels per segment, the
// segment width balanced over the row (e.g. W = 3840 -> 5 segments of 768 px / 192 threads;
// W = 1920 -> 2 x 960 px / 256 threads with 16 idle lanes).
struct Plan {
  int threads, nseg, seg, max_cols;
  bool vec4;  // four pixels per lane, 16-B accesses: W % 4 == 0, 16-B aligned buffers and W <= kMaxFloatX
};

inline Plan make_row_plan(int W, int GW, bool aligned16) {
  Plan best{};
  long long best_waste = -1;
  const int cands[3] = {256, 192, 128};
  for (int T : cands) {
    const int span = T * kPxPerThread;
    const int nseg = (W + span - 1) / span;
    const long long waste = (long long)nseg * span - W;
    if (best_waste < 0 || waste < best_waste) {
      best_waste = waste;
      best.threads = T;
      best.nseg = nseg;
    }
  }
  best.vec4 = aligned16 && (W % 4 == 0) && W <= kMaxFloatX;
  best.seg = round_up((W + best.nseg - 1) / best.nseg, 4);
  // (Round 4: rounding the segments to 32-px multiples -- W = 4000 as 1024 / 1024 / 1024 / 928 instead of 4 x 1000,
  // so that every output run is whole 128-B lines and the forward may store write-through -- measured 61.3 vs
  // 60.7 us at 4000 x 3000, interleaved, the memory skeleton at 61.0: no gain, not kept.  profiles/r04/fwd_launch_shape.md)
  best.threads = round_up((best.seg + kPxPerThread - 1) / kPxPerThread, 64);
  if (best.threads > 256) best.threads = 256;
  best.max_cols = max_cols_for(best.seg, GW, W);
  return best;
}

// OR of the addresses whose low bits a launch cares about (a null pointer contributes nothing).
template <typename... P>
inline uintptr_t ptr_bits(P... p) {
  return (uintptr_t(0) | ... | (uintptr_t)p);
}

// What a launch requires and which limits bind it.
enum : unsigned {
  kNeedAligned = 1u << 0,   // the pointers of `align_bits` 16-B aligned
  kNeedVec4 = 1u << 1,      // ... and W % 4 == 0 (Plan::vec4)
  kLimLds = 1u << 2,        // LDS of a workgroup <= kMaxLdsBytes
  kLimImage = 1u << 3,      // staged image elements < 2^20 (a staging element's column comes from a float multiply)
  kLimBH = 1u << 4,         // B, H <= 65535: the 3-D launch grid (segment, row, image)
  kLimRowBytes = 1u << 5,   // bytes of the widest pixel row < 2^31: 32-bit offsets within a row / descriptor range
  kLimBlocks = 1u << 6,     // B * H * nseg * threads <= 2^32 - 1: the 1-D launch grid of the row family (the HIP runtime
                            // refuses a launch of 2^32 threads or more in a dimension: "invalid configuration argument")
};

struct Frame {
  int B, H, W, GW, GD;
};

// The limits of `limits` that the EXTENTS of a frame break, whatever its channels, alignment or LDS need (0: none).
// kNeedVec4 is reported where the row is wider than kMaxFloatX.  row_geom below decides `ok` with it, and an entry point
// without a fallback names the limit in its refusal with extent_refusal: one function for both.
inline unsigned extent_limits_broken(const Frame& f, int row_channels, const Plan& pl, unsigned limits) {
  unsigned broken = 0;
  if ((limits & kLimBH) && (f.B > 65535 || f.H > 65535)) broken |= kLimBH;
  if ((limits & kLimRowBytes) && (long long)f.W * row_channels * 4 >= (1LL << 31)) broken |= kLimRowBytes;
  if ((limits & kLimBlocks) && (long long)f.B * f.H * pl.nseg * pl.threads > 0xffffffffLL) broken |= kLimBlocks;
  if ((limits & kNeedVec4) && f.W > kMaxFloatX) broken |= kNeedVec4;
  return broken;
}

// ... in words (null: the extents break none of `limits`).
inline const char* extent_refusal(const Frame& f, int row_channels, unsigned limits) {
  const unsigned broken = extent_limits_broken(f, row_channels, make_row_plan(f.W, f.GW, true), limits);
  if (broken & kLimBH) return "B and H may be at most 65535 (the launch grid is segment x row x image)";
  if (broken & kLimRowBytes) return "a pixel row must be shorter than 2^31 bytes (32-bit offsets within a row)";
  if (broken & kNeedVec4) return "W may be at most 2^23 = 8388608 (pixel centres x + 0.5 are formed in float32)";
  if (broken & kLimBlocks)
    return "B * H * (segments of a row) * (threads of a segment) may be at most 2^32 - 1 (the launch grid is one-dimensional)";
  return nullptr;
}

// One row-segment launch.  Dynamic LDS is [tab_floats of tables][the image][one slab per wavefront].
struct RowLaunch {
  Frame f;
  int C;                 // channels per grid cell
  bool padded;           // false: GD planes of at most GW clamped columns (the row family)
                         // true : GD + 2 planes of unclamped columns (the segment family)
  int slab_floats;       // per wavefront
  int row_channels;      // of the widest pixel stream (kLimRowBytes)
  uintptr_t align_bits;  // ptr_bits of the buffers accessed 16 B at a time
  unsigned limits;
  int tab_floats = 0;    // tables in front of the image
  // The predicate's own bound where it is not what the launcher allocates:
  int ok_slab_floats = 0;       // slab floats per wavefront the predicate budgets (0: slab_floats)
  bool ok_image_plus4 = false;  // the predicate budgets the image + 4 floats, the launcher rounds it up to 4
  int ok_static_floats = 0;     // static LDS of the kernel (not part of the bytes a launch passes)
};

struct RowGeom {
  Plan pl;
  int slab_off;  // float offset of the per-wave slabs behind the tables (= the image, rounded up to float4s)
  size_t lds;    // dynamic-LDS bytes the launcher passes
  bool ok;
};

inline RowGeom row_geom(const RowLaunch& d) {
  const Frame& f = d.f;
  RowGeom g{};
  const bool aligned = (d.align_bits & 15u) == 0;
  g.pl = make_row_plan(f.W, f.GW, aligned);
  const long long cols = d.padded ? seg_cols_for(g.pl.seg, f.GW, f.W) : g.pl.max_cols;
  const long long staged = cols * f.GD * d.C;
  const long long image = cols * (f.GD + (d.padded ? 2 : 0)) * d.C;
  const long long image4 = (image + 3) / 4 * 4;
  const long long waves = g.pl.threads / 64;
  const long long lds_floats = d.tab_floats + image4 + waves * d.slab_floats;
  // ok is decided from the predicate's bound ...
  const long long ok_floats = d.ok_static_floats + d.tab_floats + (d.ok_image_plus4 ? image + 4 : image4) +
                              waves * (d.ok_slab_floats ? d.ok_slab_floats : d.slab_floats);
  // ... and lds is the launcher's value (never larger where both are in range).
  g.slab_off = (int)image4;
  g.lds = (size_t)lds_floats * sizeof(float);
  const unsigned lim = d.limits;
  g.ok = (!(lim & kNeedAligned) || aligned) && (!(lim & kNeedVec4) || g.pl.vec4) &&
         (!(lim & kLimLds) || lds_fits((size_t)ok_floats * sizeof(float))) &&
         (!(lim & kLimImage) || staged < (1 << 20)) && extent_limits_broken(f, d.row_channels, g.pl, lim) == 0;
  return g;
}

// ---- the families ----------------------------------------------------------------------------------------------------
constexpr unsigned kSegLimits = kNeedVec4 | kLimLds | kLimImage | kLimBH | kLimRowBytes;  // padded image, 3-D launch grid
constexpr unsigned kRowsLimits = kLimLds | kLimBlocks;                                     // clamped image, 1-D launch grid

// apply_fwd_seg.hip: slab = the wave's input run, then its output run (+ its guide run where LDS-DMA brings a guide map).
inline RowGeom seg_fwd_geom(const Frame& f, int Cin, int Cout, int Cj, bool dma, bool guide_map, uintptr_t align_bits) {
  const int slab = kWaveRun * (Cin > Cout ? Cin : Cout) + ((dma && guide_map) ? kWaveRun : 0);
  return row_geom(RowLaunch{f, Cout * Cj, true, slab, Cout, align_bits, kSegLimits});
}

// apply_fwd_io.hip: slab = the wave's float output run; `tab_floats` of dynamic tables in front of the image, and the
// predicate budgets `static_floats` of static LDS on top (the largest static table of any instantiation).
inline RowGeom io_fwd_geom(const Frame& f, int C, int Cout, int tab_floats, int static_floats, uintptr_t align_bits) {
  RowLaunch d{f, C, true, kWaveRun * Cout, Cout, align_bits, kSegLimits};
  d.tab_floats = tab_floats;
  d.ok_static_floats = static_floats;
  return row_geom(d);
}

// apply_vjp_seg.hip: slab = guide | input (-> dinput) | dout runs of the wave.
inline RowGeom vjp_seg_geom(const Frame& f, int Cin, int Cout, int Cj, uintptr_t align_bits) {
  return row_geom(RowLaunch{f, Cout * Cj, true, kWaveRun * (1 + Cin + Cout), Cin > Cout ? Cin : Cout, align_bits, kSegLimits});
}

// apply_fwd_rows.hip: slab = the wave's input run, then its output run (vec4 kernel).  Unaligned buffers and W % 4 != 0
// are served too (the scalar kernel): Plan::vec4 picks.
inline RowGeom rows_fwd_geom(const Frame& f, int Cin, int Cout, int Cj, uintptr_t align_bits) {
  RowLaunch d{f, Cout * Cj, false, kWaveRun * (Cin > Cout ? Cin : Cout), 0, align_bits, kRowsLimits};
  d.ok_image_plus4 = true;  // the predicate's bound: image + 4 floats; the launcher allocates round_up(image, 4)
  return row_geom(d);
}

// apply_bwd_rows.hip: slab = the wave's dinput run, where dinput is wanted.
inline RowGeom vjp_rows_geom(const Frame& f, int Cin, int Cout, int Cj, bool want_dinput, uintptr_t align_bits) {
  RowLaunch d{f, Cout * Cj, false, want_dinput ? kWaveRun * Cin : 0, 0, align_bits, kNeedVec4 | kRowsLimits};
  d.ok_slab_floats = kWaveRun * (Cin > 0 ? Cin : 1);  // the predicate's bound: a slab whether dinput is wanted or not
  d.ok_image_plus4 = true;                            // ... and image + 4 floats for the launcher's round_up(image, 4)
  return row_geom(d);
}

// slice_fwd_rows.hip: slab = 64 pixels x C floats per wave; the guide is read per pixel, so any W.
inline RowGeom slice_fwd_geom(const Frame& f, int C, uintptr_t align_bits) {
  return row_geom(RowLaunch{f, C, false, 64 * C, 0, align_bits, kNeedAligned | kRowsLimits});
}

}  // namespace rows
}  // namespace hdrnet_amd
