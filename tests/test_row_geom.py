"""hdrnet_amd/csrc/row_geom.h -- the one place that lays a row-segment launch out -- built alone with the host compiler
and held to two records:

(a) the tests' own restatement of the plan (tests/row_plan.py), cell by cell: `ok` of the segment forward (with a guide
    map and without), the row forward and the wire-format forward, and `threads`, `nseg`, `seg`, for 3 -> 3 with offset
    over W = 4, 8 .. 8200 x 15 grid widths x 3 grid depths;
(b) tests/golden/row_geom.json: what the kernel files computed by hand BEFORE the header existed (recorded from that
    commit by tests/golden/make_row_geom.py) -- per family the number of cells, of `ok` cells and a 64-bit digest of
    (threads, nseg, seg, slab_off, lds, ok) over the same sweep for every fast shape, and the edge cells in full.  The
    record predates the bound on the width of the four-pixel kernels (kMaxFloatX): its ten edge cells of rows wider
    than 2^23 in a family that needs those kernels are held to everything they recorded but `ok`, which is now 0, and
    so are its four cells of one-dimensional launches between the runtime's 2^32 - 1 threads and 2^31 - 1 workgroups;
(c) the extent limits as tests/row_plan.py restates them, at the shapes of tests/extent_cases.py: Plan::vec4, `ok` of
    every family and the limit extent_refusal names, on either side of each limit.

Host arithmetic only: no GPU, a few seconds.
"""
import json
import os
import re
import shutil
import subprocess

import pytest

import extent_cases
from row_plan import (MAX_FLOAT_X, MAX_LAUNCH_THREADS, extent_limit, io_fits, row_plan, rows_fits, rows_reaches, seg_fits, seg_reaches, slice_kernel,
                      vec4, vjp_kernel)

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hdrnet_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden")

PROBE = r"""
#include <stdlib.h>

#include "row_geom.h"
#include "row_geom_sweep.h"

using namespace hdrnet_amd::rows;

// The probe fills the families of row_geom.h in itself: every buffer at 0x1000 but the output, and 768 floats of static
// tables for the wire-format forward (apply_fwd_io.hip asserts that figure).  What the kernel files' own wrappers pass
// -- their pointer sets, want_dinput -- is NOT checked here: the GPU tests that pin which kernel a call reaches are.
sweep::Cell cell(const sweep::Query& q) {
  const Frame f{q.B, q.H, q.W, q.GW, q.GD};
  const int Cj = q.Cin + q.offset;
  const uintptr_t bits = ptr_bits(sweep::kAligned, q.out);
  RowGeom g{};
  switch (q.family) {
    case sweep::kSegDmaMap: g = seg_fwd_geom(f, q.Cin, q.Cout, Cj, true, true, bits); break;
    case sweep::kSegDmaNoMap: g = seg_fwd_geom(f, q.Cin, q.Cout, Cj, true, false, bits); break;
    case sweep::kSegLaneMap: g = seg_fwd_geom(f, q.Cin, q.Cout, Cj, false, true, bits); break;
    case sweep::kSegLaneNoMap: g = seg_fwd_geom(f, q.Cin, q.Cout, Cj, false, false, bits); break;
    case sweep::kRowsFwd: g = rows_fwd_geom(f, q.Cin, q.Cout, Cj, bits); break;
    case sweep::kIo: g = io_fwd_geom(f, q.Cout * Cj, q.Cout, 0, 768, bits); break;  // 768: the curves guide's static tables
    case sweep::kVjpSeg: g = vjp_seg_geom(f, q.Cin, q.Cout, Cj, bits); break;
    case sweep::kVjpRowsDinput: g = vjp_rows_geom(f, q.Cin, q.Cout, Cj, q.Cin > 0, bits); break;
    case sweep::kVjpRowsNoDinput: g = vjp_rows_geom(f, q.Cin, q.Cout, Cj, false, bits); break;
    case sweep::kSliceFwd: g = slice_fwd_geom(f, q.C, bits); break;
  }
  return {g.pl.threads, g.pl.nseg, g.pl.seg, g.slab_off, g.lds, g.ok};
}

// (c): "B H W GW GD" per argument triple -> vec4, ok of seg+map / seg / rows / io / vjp_seg / vjp_rows / slice (C = 12), and
// the first word of extent_refusal for the segment family and for the row family's four-pixel kernels
static const char* word(const char* text) {
  if (!text) return "-";
  return strstr(text, "65535") ? "65535" : strstr(text, "2^31 bytes") ? "2^31bytes" : strstr(text, "2^23") ? "2^23"
       : strstr(text, "2^32 - 1") ? "2^32-1" : "?";
}

static void extents(int n, char** v) {
  for (int i = 0; i + 4 < n; i += 5) {
    const Frame f{atoi(v[i]), atoi(v[i + 1]), atoi(v[i + 2]), atoi(v[i + 3]), atoi(v[i + 4])};
    const uintptr_t bits = sweep::kAligned;
    printf("%d %d %d %d %d %d %d %d %s %s\n", (int)make_row_plan(f.W, f.GW, true).vec4,
           (int)seg_fwd_geom(f, 3, 3, 4, true, true, bits).ok, (int)seg_fwd_geom(f, 3, 3, 4, true, false, bits).ok,
           (int)rows_fwd_geom(f, 3, 3, 4, bits).ok, (int)io_fwd_geom(f, 12, 3, 0, 768, bits).ok,
           (int)vjp_seg_geom(f, 3, 3, 4, bits).ok, (int)vjp_rows_geom(f, 3, 3, 4, true, bits).ok,
           (int)slice_fwd_geom(f, 12, bits).ok, word(extent_refusal(f, 3, kSegLimits)),
           word(extent_refusal(f, 0, kNeedVec4 | kRowsLimits)));
  }
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "extents")) {
    extents(argc - 2, argv + 2);
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "needs4")) {
    // family; whether it needs the four-pixel lanes (kNeedVec4: takes a small frame at W = 64, refuses it at W = 66);
    // whether its launch grid is one-dimensional (kLimBlocks: takes 1023 x 65536 rows of 4 pixels, refuses 1024 x 65536);
    // whether a refusal carries no plan
    for (int fam = 0; fam < sweep::kFamilies; ++fam) {
      sweep::Query a = sweep::query(fam, 4, 2, 2, 3, 3, 1, 12), b = a;
      a.B = 1023, b.B = 1024, a.H = b.H = 65536;
      printf("%s %d %d %d\n", sweep::kFamilyName[fam], (int)(cell(sweep::query(fam, 64, 16, 8, 3, 3, 1, 12)).ok &&
                                                            !cell(sweep::query(fam, 66, 16, 8, 3, 3, 1, 12)).ok),
             (int)(cell(a).ok && !cell(b).ok), (int)(!cell(b).ok && sweep::cell_of(b).threads == 0));
    }
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "cells")) {  // (a): W GW GD threads nseg seg ok(seg+map) ok(seg) ok(rows) ok(io)
    for (int W = 4; W <= sweep::kWMax; W += 4)
      for (int GW : sweep::kGW)
        for (int GD : sweep::kGD) {
          const sweep::Cell m = cell(sweep::query(sweep::kSegDmaMap, W, GW, GD, 3, 3, 1));
          printf("%d %d %d %d %d %d %d %d %d %d\n", W, GW, GD, m.threads, m.nseg, m.seg, m.ok,
                 cell(sweep::query(sweep::kSegDmaNoMap, W, GW, GD, 3, 3, 1)).ok,
                 cell(sweep::query(sweep::kRowsFwd, W, GW, GD, 3, 3, 1)).ok, cell(sweep::query(sweep::kIo, W, GW, GD, 3, 3, 1)).ok);
        }
    return 0;
  }
  sweep::write_json(stdout);  // (b)
  return 0;
}
"""


def _table(name):
    """The X-macro table `name` of launch.hip.h, as the text of its body."""
    src = open(os.path.join(CSRC, "launch.hip.h")).read()
    body = re.search(r"#define " + name + r"\(X\)((?:[^\n]*\\\n)*[^\n]*)\n", src).group(1)
    return " ".join(body.replace("\\\n", " ").split())


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / c++) on PATH")
    d = tmp_path_factory.mktemp("row_geom")
    src, exe = str(d / "probe.cc"), str(d / "probe")
    with open(src, "w") as fh:
        fh.write(PROBE)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-I", GOLDEN,
                    "-DSWEEP_APPLY_SHAPES(X)=" + _table("HDRNET_APPLY_FAST_SHAPES"),
                    "-DSWEEP_SLICE_CHANNELS(X)=" + _table("HDRNET_SLICE_FAST_CHANNELS"), src, "-o", exe], check=True)
    return exe


def test_against_the_python_restatement(probe):
    out = subprocess.run([probe, "cells"], check=True, capture_output=True, text=True).stdout
    n = 0
    for line in out.splitlines():
        W, GW, GD, threads, nseg, seg, ok_map, ok_nomap, ok_rows, ok_io = map(int, line.split())
        cell = (W, GW, GD)
        assert (threads, nseg, seg) == row_plan(W), cell
        assert bool(ok_map) == seg_fits(W, GW, GD, True), cell
        assert bool(ok_nomap) == seg_fits(W, GW, GD, False), cell
        assert bool(ok_rows) == rows_fits(W, GW, GD), cell
        assert bool(ok_io) == io_fits(W, GW, GD), cell
        n += 1
    assert n == 2050 * 15 * 3


LAUNCH_FOLLOWS = 4  # the "blocks < 2^31" cells of the four families with a one-dimensional launch grid


def test_against_the_recorded_geometry(probe):
    got = json.loads(subprocess.run([probe], check=True, capture_output=True, text=True).stdout)
    want = json.load(open(os.path.join(GOLDEN, "row_geom.json")))
    assert want["seg_cross_check"] == {"cells": 221400, "ok": 216522}  # the recorder's own check
    assert got["families"].keys() == want["families"].keys()
    for fam, rec in want["families"].items():
        assert got["families"][fam] == rec, fam
    assert len(got["edges"]) == len(want["edges"]) == 200
    # which families need the four-pixel lanes: asked of the header (W % 4 != 0 refused), not listed here
    # ... and which launch on a one-dimensional grid, whose bound is now the runtime's 2^32 - 1 threads where the record
    # has 2^31 - 1 workgroups: such a cell is held to its recorded plan with ok = 0 too (to no plan for the slice forward)
    flags = {name: [bool(int(v)) for v in rest] for name, *rest in
             (line.split() for line in subprocess.run([probe, "needs4"], check=True, capture_output=True, text=True).stdout.splitlines())}
    needs4, launch1d, blank = ({name: f[i] for name, f in flags.items()} for i in range(3))
    assert set(needs4) == set(want["families"]) and not needs4["rows_fwd"] and not needs4["slice_fwd"] and sum(needs4.values()) == 8
    assert sorted(n for n, v in launch1d.items() if v) == ["rows_fwd", "slice_fwd", "vjp_rows", "vjp_rows/dinput"]
    follows = launch_follows = 0
    for g, w in zip(got["edges"], want["edges"]):
        threads, nseg = w["cell"][:2]
        if w["cell"][5] == 1 and launch1d[w["family"]] and w["B"] * w["H"] * nseg * threads > MAX_LAUNCH_THREADS:
            w = dict(w, cell=[0] * 6 if blank[w["family"]] else w["cell"][:5] + [0])
            launch_follows += 1
        elif w["W"] > MAX_FLOAT_X and w["cell"][5] == 1 and needs4[w["family"]]:
            # recorded before kMaxFloatX: a family of four-pixel kernels no longer takes a row this wide
            w = dict(w, cell=w["cell"][:5] + [0])
            follows += 1
        assert g == w, (w["family"], w["case"], w["W"], w["GW"])
    assert follows == 10 and launch_follows == LAUNCH_FOLLOWS, (follows, launch_follows)
    assert {k: v for k, v in got.items() if k != "edges"} == {k: v for k, v in want.items() if k != "edges"}


def test_extent_limits_against_the_python_restatement(probe):
    """(c): Plan::vec4, every family's `ok` and the limit extent_refusal names at the wide, tall and deep shapes and at
    the two sides of kMaxFloatX, kLimBlocks and kLimRowBytes."""
    GH, GW, GD = extent_cases.WIDE_GRID
    shapes = [(1, 1, W, GW, GD) for W in extent_cases.WIDE_SIDES]
    shapes += [(1, H, W, GW, GD) for H, W in extent_cases.WIDE + [extent_cases.WIDE_SCALAR_NEIGHBOUR]]
    shapes += [(B, H, W, gw, gd) for B, H, W, _, gw, gd in extent_cases.TALL + extent_cases.DEEP + extent_cases.NYG]
    shapes += [s[:3] + s[4:] for s in extent_cases.LAUNCH] + [(1, 1, 178956968, 16, 8), (1, 1, 178956972, 16, 8)]
    out = subprocess.run([probe, "extents"] + [str(v) for s in shapes for v in s], check=True, capture_output=True,
                         text=True).stdout.splitlines()
    assert len(out) == len(shapes)
    for (B, H, W, gw, gd), line in zip(shapes, out):
        *oks, seg_word, rows_word = line.split()
        v4, ok_map, ok_nomap, ok_rows, ok_io, ok_vjp_seg, ok_vjp_rows, ok_slice = (bool(int(v)) for v in oks)
        cell = (B, H, W, gw, gd)
        assert v4 == vec4(W), cell
        assert ok_map == seg_reaches(B, H, W, gw, gd, True) and ok_nomap == seg_reaches(B, H, W, gw, gd, False), cell
        assert (ok_rows, ok_rows and v4) == rows_reaches(B, H, W, gw, gd), cell
        assert ok_io == seg_reaches(B, H, W, gw, gd, io=True), cell
        assert (ok_vjp_seg, ok_vjp_rows) == (vjp_kernel(B, H, W, gw, gd) == "apply_vjp_seg/vec4",
                                             vjp_kernel(B, H, W, gw, gd) is not None), cell
        assert ok_slice == (slice_kernel(B, H, W, gw, gd, 12) == "slice_fwd_rows"), cell
        assert seg_word.replace("2^31bytes", "2^31 bytes") == (extent_limit(B, H, W, "seg") or "-"), cell
        assert rows_word.replace("2^32-1", "2^32 - 1") == (extent_limit(B, H, W, "rows4") or "-"), cell
