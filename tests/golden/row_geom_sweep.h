// The sweep behind tests/golden/row_geom.json, shared by its recorder (make_row_geom.py: the geometry functions of the
// commit to record from) and by tests/test_row_geom.py (hdrnet_amd/csrc/row_geom.h of the tree), so that both walk the
// same cells in the same order and digest them the same way.  Plain C++17.
//
// The includer defines, before including this file,
//   SWEEP_APPLY_SHAPES(X)    X(CIN, COUT, OFFSET) ...   = HDRNET_APPLY_FAST_SHAPES of launch.hip.h
//   SWEEP_SLICE_CHANNELS(X)  X(C) ...                   = HDRNET_SLICE_FAST_CHANNELS
// and, after it, `Cell cell(const Query&)`: the launch geometry of one family for one call.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace sweep {

enum Family {
  kSegDmaMap, kSegDmaNoMap, kSegLaneMap, kSegLaneNoMap,  // apply_fwd_seg: LDS-DMA or per-lane loads, guide map or network
  kRowsFwd,                                              // apply_fwd_rows
  kIo,                                                   // apply_fwd_io, f32 -> f32 with a guide map
  kVjpSeg,                                               // apply_vjp_seg
  kVjpRowsDinput, kVjpRowsNoDinput,                      // apply_bwd_rows, dguide + dinput / dguide alone
  kSliceFwd,                                             // slice_fwd_rows
  kFamilies
};
static const char* const kFamilyName[kFamilies] = {"seg/dma+map", "seg/dma", "seg/lane+map", "seg/lane", "rows_fwd", "io",
                                                   "vjp_seg", "vjp_rows/dinput", "vjp_rows", "slice_fwd"};

struct Query {
  int family;
  int B, H, W, GW, GD;
  int Cin, Cout, offset;  // the apply families
  int C;                  // kSliceFwd
  uintptr_t out;          // the output buffer (dinput for the VJPs): every other buffer sits at 0x1000
};

struct Cell {
  int threads, nseg, seg, slab_off;
  unsigned long long lds;
  int ok;
};

}  // namespace sweep

sweep::Cell cell(const sweep::Query& q);

namespace sweep {

// (slice_fwd_rows refuses before it plans: only the refusal is compared)
inline Cell cell_of(const Query& q) {
  const Cell c = cell(q);
  return (q.family == kSliceFwd && !c.ok) ? Cell{} : c;
}

struct Digest {
  unsigned long long h = 1469598103934665603ull, cells = 0, ok = 0;  // FNV-1a, 64 bit
  void word(unsigned long long v) {
    for (int i = 0; i < 8; ++i) {
      h ^= (v >> (8 * i)) & 0xffu;
      h *= 1099511628211ull;
    }
  }
  void add(const Cell& c) {
    word((unsigned)c.threads); word((unsigned)c.nseg); word((unsigned)c.seg); word((unsigned)c.slab_off);
    word(c.lds); word((unsigned)c.ok);
    ++cells;
    ok += c.ok ? 1 : 0;
  }
};

static const int kGW[] = {1, 2, 7, 16, 32, 53, 54, 58, 59, 64, 69, 70, 75, 81, 128};
static const int kGWCross[] = {1, 2, 7, 16, 32, 59, 64, 75, 128};
static const int kGD[] = {1, 8, 16};
constexpr int kWMax = 8200;
constexpr uintptr_t kAligned = 0x1000;

inline Query query(int family, int W, int GW, int GD, int Cin, int Cout, int offset, int C = 0) {
  return Query{family, 2, 16, W, GW, GD, Cin, Cout, offset, C, kAligned};
}

template <int N>
inline void sweep_into(Digest& d, const int (&gws)[N], Query q) {
  for (int W = 4; W <= kWMax; W += 4)
    for (int GW : gws)
      for (int GD : kGD) {
        q.W = W; q.GW = GW; q.GD = GD;
        d.add(cell_of(q));
      }
}

inline void print_cell(FILE* f, const Cell& c) {
  fprintf(f, "[%d, %d, %d, %d, %llu, %d]", c.threads, c.nseg, c.seg, c.slab_off, c.lds, c.ok);
}

// The JSON of tests/golden/row_geom.json.
inline void write_json(FILE* f) {
  fprintf(f, "{\n\"families\": {\n");
  for (int fam = 0; fam < kFamilies; ++fam) {
    Digest d;
    if (fam == kSliceFwd) {
#define SWEEP_X(CC) sweep_into(d, kGW, query(fam, 0, 0, 0, 0, 0, 0, CC));
      SWEEP_SLICE_CHANNELS(SWEEP_X)
#undef SWEEP_X
    } else if (fam == kIo) {
      sweep_into(d, kGW, query(fam, 0, 0, 0, 3, 3, 1));  // the one shape the family is built for
    } else {
#define SWEEP_X(CI, CO, OFF) sweep_into(d, kGW, query(fam, 0, 0, 0, CI, CO, OFF ? 1 : 0));
      SWEEP_APPLY_SHAPES(SWEEP_X)
#undef SWEEP_X
    }
    fprintf(f, "  \"%s\": {\"cells\": %llu, \"ok\": %llu, \"digest\": \"%016llx\"}%s\n", kFamilyName[fam], d.cells, d.ok, d.h,
            fam + 1 < kFamilies ? "," : "");
  }
  // the recorder's cross-check: seg_geom, 3 -> 3 with offset, DMA x guide map over the narrower GW list
  Digest x;
  for (int fam = kSegDmaMap; fam <= kSegLaneNoMap; ++fam) sweep_into(x, kGWCross, query(fam, 0, 0, 0, 3, 3, 1));
  fprintf(f, "},\n\"seg_cross_check\": {\"cells\": %llu, \"ok\": %llu},\n\"edges\": [\n", x.cells, x.ok);
  // edge cells, 3 -> 3 with offset (C = 12 for the slice), every family: the row-kernel fallbacks of
  // tests/test_gpu_fused_fullsize.py (FALLBACKS, GD = 16), an unaligned output, W % 4 != 0, B or H at and past 65535,
  // and the limits no frame of the sweep reaches: B * H * nseg at and past 2^31 - 1 (W = 512 is one segment), a row of
  // 3 channels just below and past 2^31 bytes, and a staged image of 2^20 elements and more (which no LDS holds either)
  struct Edge { const char* what; int B, H, W, GW, GD; uintptr_t out; };
  static const Edge edges[] = {
      {"fallback", 1, 12, 256, 75, 16, kAligned},  {"fallback", 1, 12, 1024, 64, 16, kAligned},
      {"fallback", 1, 12, 1024, 59, 16, kAligned}, {"fallback", 1, 12, 1024, 58, 16, kAligned},
      {"fallback", 1, 12, 1024, 54, 16, kAligned}, {"fallback", 1, 12, 1024, 53, 16, kAligned},
      {"fallback", 1, 12, 1024, 69, 16, kAligned}, {"unaligned out", 2, 16, 1920, 16, 8, kAligned + 4},
      {"unaligned out", 1, 12, 256, 75, 16, kAligned + 4}, {"W % 4", 2, 16, 1922, 16, 8, kAligned},
      {"W % 4", 2, 16, 1023, 64, 8, kAligned},    {"B = 65535", 65535, 1, 1920, 16, 8, kAligned},
      {"B = 65536", 65536, 1, 1920, 16, 8, kAligned}, {"H = 65535", 1, 65535, 1920, 16, 8, kAligned},
      {"H = 65536", 1, 65536, 1920, 16, 8, kAligned},
      {"blocks < 2^31", 46340, 46341, 512, 16, 8, kAligned}, {"blocks >= 2^31", 46341, 46341, 512, 16, 8, kAligned},
      {"row bytes < 2^31", 1, 2, 178956968, 16, 8, kAligned}, {"row bytes >= 2^31", 1, 2, 178956972, 16, 8, kAligned},
      {"image >= 2^20", 2, 16, 1920, 16, 32768, kAligned}};
  const int n = (int)(sizeof edges / sizeof edges[0]);
  for (int e = 0; e < n; ++e)
    for (int fam = 0; fam < kFamilies; ++fam) {
      const Edge& E = edges[e];
      const Query q{fam, E.B, E.H, E.W, E.GW, E.GD, 3, 3, 1, 12, E.out};
      fprintf(f, "  {\"family\": \"%s\", \"case\": \"%s\", \"B\": %d, \"H\": %d, \"W\": %d, \"GW\": %d, \"GD\": %d, \"cell\": ",
              kFamilyName[fam], E.what, E.B, E.H, E.W, E.GW, E.GD);
      print_cell(f, cell_of(q));
      fprintf(f, "}%s\n", (e + 1 < n || fam + 1 < kFamilies) ? "," : "");
    }
  fprintf(f, "]\n}\n");
}

}  // namespace sweep
