"""hdrnet_amd/csrc/row_geom.h -- the one place that lays a row-segment launch out -- built alone with the host compiler
and held to two records:

(a) the tests' own restatement of the plan (tests/row_plan.py), cell by cell: `ok` of the segment forward (with a guide
    map and without), the row forward and the wire-format forward, and `threads`, `nseg`, `seg`, for 3 -> 3 with offset
    over W = 4, 8 .. 8200 x 15 grid widths x 3 grid depths;
(b) tests/golden/row_geom.json: what the kernel files computed by hand BEFORE the header existed (recorded from that
    commit by tests/golden/make_row_geom.py) -- per family the number of cells, of `ok` cells and a 64-bit digest of
    (threads, nseg, seg, slab_off, lds, ok) over the same sweep for every fast shape, and the edge cells in full.

Host arithmetic only: no GPU, a few seconds.
"""
import json
import os
import re
import shutil
import subprocess

import pytest

from row_plan import io_fits, row_plan, rows_fits, seg_fits

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "hdrnet_amd", "csrc")
GOLDEN = os.path.join(HERE, "golden")

PROBE = r"""
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

int main(int argc, char** argv) {
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


def test_against_the_recorded_geometry(probe):
    got = json.loads(subprocess.run([probe], check=True, capture_output=True, text=True).stdout)
    want = json.load(open(os.path.join(GOLDEN, "row_geom.json")))
    assert want["seg_cross_check"] == {"cells": 221400, "ok": 216522}  # the recorder's own check
    assert got["families"].keys() == want["families"].keys()
    for fam, rec in want["families"].items():
        assert got["families"][fam] == rec, fam
    assert len(got["edges"]) == len(want["edges"]) == 200
    for g, w in zip(got["edges"], want["edges"]):
        assert g == w, (w["family"], w["case"], w["W"], w["GW"])
    assert got == want
