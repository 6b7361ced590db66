#!/usr/bin/env python
"""Records the launch geometry of the row-segment kernels as the sources of one commit compute it.

    python tests/golden/make_row_geom.py path/to/checkout      # writes tests/golden/row_geom.json

`checkout` is a tree of the commit whose geometry is the one to keep: one from BEFORE hdrnet_amd/csrc/row_geom.h, where
every kernel file still worked its launch out by hand (git worktree add ../parent 8005968).  The recorder builds a
program that #includes that tree's .hip files, one per translation unit, and calls their own geometry functions --
seg_geom, geom_for + apply_fwd_rows_supported, io_geom + plan_io, vjp_geom, vjp_plan, plan_for -- on the CPU, over
the sweep of row_geom_sweep.h.  Built with plain `hipcc --offload-arch=gfx950` the program needs no GPU: it launches
nothing.  tests/test_row_geom.py then holds row_geom.h of the tree to the file.

Where a launcher of that commit sized its LDS inline (apply_bwd_rows.hip: launch_vjp_t), the glue below repeats those
two lines; everything else is the recorded commit's code.
"""
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "row_geom.json")

PRELUDE = """
#include "%(csrc)s/%(src)s"
#define SWEEP_APPLY_SHAPES(X) HDRNET_APPLY_FAST_SHAPES(X)
#define SWEEP_SLICE_CHANNELS(X) HDRNET_SLICE_FAST_CHANNELS(X)
#include "row_geom_sweep.h"
namespace hdrnet_amd {
namespace {
const float* const P = reinterpret_cast<const float*>(sweep::kAligned);
float* const PW = reinterpret_cast<float*>(sweep::kAligned);
[[maybe_unused]] ApplyArgs apply_args(const sweep::Query& q) {
  ApplyArgs a{};
  a.grid = P; a.guide = P; a.input = P; a.out = reinterpret_cast<float*>(q.out);
  a.B = q.B; a.H = q.H; a.W = q.W; a.GH = 8; a.GW = q.GW; a.GD = q.GD;
  a.Cin = q.Cin; a.Cout = q.Cout; a.Cj = q.Cin + q.offset; a.has_offset = q.offset != 0;
  return a;
}
[[maybe_unused]] ApplyGradArgs grad_args(const sweep::Query& q, bool want_dinput) {
  ApplyGradArgs a{};
  a.grid = P; a.guide = P; a.input = P; a.dout = P;
  a.dguide = want_dinput ? PW : reinterpret_cast<float*>(q.out);
  a.dinput = want_dinput ? reinterpret_cast<float*>(q.out) : nullptr;
  a.B = q.B; a.H = q.H; a.W = q.W; a.GH = 8; a.GW = q.GW; a.GD = q.GD;
  a.Cin = q.Cin; a.Cout = q.Cout; a.Cj = q.Cin + q.offset; a.has_offset = q.offset != 0;
  return a;
}
}  // namespace
"""

GLUE = {
    "apply_fwd_seg.hip": """
sweep::Cell cell_seg(const sweep::Query& q) {
  const bool dma = q.family == sweep::kSegDmaMap || q.family == sweep::kSegDmaNoMap;
  const bool map = q.family == sweep::kSegDmaMap || q.family == sweep::kSegLaneMap;
  const SegGeom g = seg_geom(apply_args(q), dma, map);
  return {g.pl.threads, g.pl.nseg, g.pl.seg, g.slab_off, g.lds, g.ok};
}
""",
    "apply_fwd_rows.hip": """
sweep::Cell cell_rows(const sweep::Query& q) {
  const ApplyArgs a = apply_args(q);
  LaunchGeom g{};
#define GLUE_X(CI, CO, OFF) \\
  if (a.Cin == CI && a.Cout == CO && a.has_offset == OFF) g = geom_for<CO * (CI + (OFF ? 1 : 0)), CO>(a);
  HDRNET_APPLY_FAST_SHAPES(GLUE_X)
#undef GLUE_X
  return {g.pl.threads, g.pl.nseg, g.pl.seg, g.slab_off, g.lds, apply_fwd_rows_supported(a)};
}
""",
    "apply_fwd_io.hip": """
sweep::Cell cell_io(const sweep::Query& q) {
  ApplyIoArgs a{};
  a.grid = P; a.guide = P; a.input = P; a.out = reinterpret_cast<void*>(q.out);
  a.B = q.B; a.H = q.H; a.W = q.W; a.GH = 8; a.GW = q.GW; a.GD = q.GD;
  a.Cin = q.Cin; a.Cout = q.Cout; a.has_offset = q.offset != 0;
  a.input_dtype = 0; a.output_dtype = 0; a.white_level = 1.0f;
  Plan pl;
  const bool ok = plan_io(a, &pl);
  const IoGeom g = io_geom(a.W, a.GW, a.GD, 12, 3);  // launch_io, product build, any guide source
  return {g.pl.threads, g.pl.nseg, g.pl.seg, g.slab_off, g.lds, ok};
}
""",
    "apply_vjp_seg.hip": """
sweep::Cell cell_vjp_seg(const sweep::Query& q) {
  const VjpGeom g = vjp_geom(grad_args(q, true));
  return {g.pl.threads, g.pl.nseg, g.pl.seg, g.slab_off, g.lds, g.ok};
}
""",
    "apply_bwd_rows.hip": """
sweep::Cell cell_vjp_rows(const sweep::Query& q) {
  const ApplyGradArgs a = grad_args(q, q.family == sweep::kVjpRowsDinput);
  Plan pl;
  const bool ok = vjp_plan(a, &pl);
  // launch_vjp_t<CIN, COUT, OFFSET, WG, WI>, with WI as launch_vjp_want picks it
  const bool WI = a.dinput != nullptr && a.Cin > 0;
  const int slab_off = round_up(pl.max_cols * a.GD * a.Cout * a.Cj, 4);
  const size_t lds = ((size_t)slab_off + (WI ? (size_t)(pl.threads / 64) * 64 * kPxPerThread * a.Cin : 0)) * sizeof(float);
  return {pl.threads, pl.nseg, pl.seg, slab_off, lds, ok};
}
""",
    "slice_fwd_rows.hip": """
sweep::Cell cell_slice(const sweep::Query& q) {
  const SliceArgs a{P, P, reinterpret_cast<float*>(q.out), q.B, q.H, q.W, 8, q.GW, q.GD, q.C};
  Plan pl{};
  size_t lds = 0;
  int slab_off = 0;
  const bool ok = plan_for(a, &pl, &lds, &slab_off);
  return {pl.threads, pl.nseg, pl.seg, slab_off, lds, ok};
}
""",
}

MAIN = """
#include <stdarg.h>
#include "%(csrc)s/launch.hip.h"
#define SWEEP_APPLY_SHAPES(X) HDRNET_APPLY_FAST_SHAPES(X)
#define SWEEP_SLICE_CHANNELS(X) HDRNET_SLICE_FAST_CHANNELS(X)
#include "row_geom_sweep.h"
namespace hdrnet_amd {
sweep::Cell cell_seg(const sweep::Query&);
sweep::Cell cell_rows(const sweep::Query&);
sweep::Cell cell_io(const sweep::Query&);
sweep::Cell cell_vjp_seg(const sweep::Query&);
sweep::Cell cell_vjp_rows(const sweep::Query&);
sweep::Cell cell_slice(const sweep::Query&);
}
sweep::Cell cell(const sweep::Query& q) {
  using namespace hdrnet_amd;
  switch (q.family) {
    case sweep::kRowsFwd: return cell_rows(q);
    case sweep::kIo: return cell_io(q);
    case sweep::kVjpSeg: return cell_vjp_seg(q);
    case sweep::kVjpRowsDinput: case sweep::kVjpRowsNoDinput: return cell_vjp_rows(q);
    case sweep::kSliceFwd: return cell_slice(q);
    default: return cell_seg(q);
  }
}
int main(int, char** argv) {
  FILE* f = fopen(argv[1], "w");
  if (!f) return 1;
  sweep::write_json(f);
  return fclose(f) != 0;
}
"""


def main():
    root = os.path.abspath(sys.argv[1])
    sys.path.insert(0, root)
    from hdrnet_amd import build as hb  # the recorded commit's flags
    csrc = os.path.join(root, "hdrnet_amd", "csrc")
    include = os.path.join(root, "include")
    flags = dict(hb.SOURCES)
    with tempfile.TemporaryDirectory() as d:
        units = []
        for src, glue in GLUE.items():
            path = os.path.join(d, "glue_" + src)
            with open(path, "w") as fh:
                fh.write(PRELUDE % dict(csrc=csrc, src=src) + glue + "}  // namespace hdrnet_amd\n")
            units.append((path, flags[src]))
        path = os.path.join(d, "main.hip")
        with open(path, "w") as fh:
            fh.write(MAIN % dict(csrc=csrc))
        units.append((path, []))

        def compile_one(unit):
            path, extra = unit
            obj = path + ".o"
            res = subprocess.run([hb.hipcc(), *hb.COMMON, *extra, "-I", csrc, "-I", include, "-I", HERE, "-c", path, "-o", obj],
                                 capture_output=True, text=True)
            if res.returncode != 0:
                raise RuntimeError(path + "\n" + res.stderr[-4000:])
            return obj

        with ThreadPoolExecutor(len(units)) as pool:
            objs = list(pool.map(compile_one, units))
        exe = os.path.join(d, "record_row_geom")
        subprocess.run([hb.hipcc(), f"--offload-arch={hb.ARCH}", "-o", exe, *objs], check=True)
        subprocess.run([exe, OUT], check=True)
    import json
    got = json.load(open(OUT))
    # seg_geom for 3 -> 3 with offset at 8005968: the figures the recorder is checked by
    assert got["seg_cross_check"] == {"cells": 221400, "ok": 216522}, got["seg_cross_check"]
    print("%d families, %d edge cells -> %s" % (len(got["families"]), len(got["edges"]), OUT))


if __name__ == "__main__":
    main()
