"""The fused gradient pass (grid_grad_mfma.hip: apply_bwd_fused/mfma, slice_bwd_fused/mfma, grid_grad_mfma) under
launch plans other than the one today's register allocation gives on a 256-CU device.

gg_plan fits rg, the rows per workgroup task, to occupancy x CUs of the stage-1 variant it launches.  rg decides which
three clamped grid rows a task's tile holds (stage 1) and which tasks stage 2 adds up for a grid row; the suite's older
small shapes all run rg = cell (fewer tasks than slots), where no task ends inside a cell, and the frame-sized ones run
one plan per variant.  tests/test_grad_plan_host.py holds the float arithmetic of the two stages against each other on
the CPU; here the plans run:

* PRODUCT LIBRARY, which cannot be told a plan: frames with many task columns on few rows (8 images of 96 x 32 and
  128 x 32 on grids of 3 and 4 rows), whose plan is rg < cell at EVERY occupancy 1 .. 8 -- 4 .. 19 rows per task in cells
  of 24, 32 and 42 (128 = 3 x 42 + 2: the last rows lie past the last whole cell).
* TOOLS LIBRARY, knob 3 of hdrnet_tools_set_knob (include/hdrnet_amd_tools.h) forces rg: EVERY rg the planner can
  return, min(cell, 4) .. cell, on frames with cells of 12, 11, 100 (seven values), 3 and 1 (H < GH).  The workspace is
  exactly the forced plan's bytes (tests/row_plan.py: gg_plan_bytes; the query must say the same), prefilled with NaNs,
  between guard bands.

Variants: 3 -> 3 with offset at 8 and 16 planes over every subset of {dgrid, dguide, dinput} that holds dgrid (four
stage-1 instantiations per depth), 4 -> 4 with offset (dgrid as two channel windows) at 8 and 16 planes, the slice op
with 12 channels (dgrid, dgrid + dguide) at 8 and 16 planes and with 2 channels (no float4: dgrid on the contraction
alone).  The slice op with 3 channels has no fast gradient (not one of HDRNET_SLICE_FAST_CHANNELS): it runs beside them
and is held to that -- a workspace of 0 bytes, the generic kernel, under every plan.  Every result against the CPU oracle
at the suite's bars (tests/conftest.py: dgrid rtol 1e-4 + 1e-5 x max|want|, dinput 1e-5 flat; dguide 2e-5 x GD / 8
flat, tests/test_gpu_luma_bins.py), the kernel name asserted -- a fall-back to the generic kernels would pass the
numbers.

dguide and dinput ACROSS PLANS are bit-identical, and asserted so: a pixel's two gradients are computed by the lane
that holds it from (x, y, its own guide / input / dout) and the coefficient image of its row -- the x offsets from the
interval start, the y weights and the two grid rows from y alone -- none of which depends on where the task starts or
which wave of it takes the row.  dgrid's summation order follows rg (rows per wave, tasks per grid row): it is held to
the oracle per plan.
"""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import row_plan  # noqa: E402
from conftest import check_dgrid  # noqa: E402
from grad_plan_cases import (FAMILIES, FORCED_FRAMES, PRODUCT_FRAMES, VARIANTS, Guarded, Problem, frame_id,  # noqa: E402
                             kernel_name, prepare, subsets)
from test_gpu_luma_bins import check_pix  # noqa: E402

FORCE_RG_KNOB = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib
    return prepare(_lib.load())


@pytest.fixture(scope="module")
def tools():
    from hdrnet_amd import _lib
    return prepare(_lib.load_tools())


def variant_id(v):
    return "%s-gd%d" % v


def seed_of(frame, family, GD):
    return sum(frame) * 100 + len(family) * 10 + GD + sorted(FAMILIES).index(family)


@pytest.mark.parametrize("variant", VARIANTS, ids=variant_id)
@pytest.mark.parametrize("frame", PRODUCT_FRAMES, ids=frame_id)
def test_product_library_plans_that_straddle_grid_rows(dev, lib, port, frame, variant):
    family, GD = variant
    B, H, W, GH, GW = frame
    p = Problem(port, dev, frame, family, GD, seed_of(frame, family, GD))
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    rgs = [row_plan.gg_plan(B, H, W, GH, GW, GD, p.C, occ * cus)[0] for occ in range(1, 9)]
    need = p.query(lib)
    print(f"{frame_id(frame)} {variant_id(variant)}: {cus} CUs, rg at occupancy 1 .. 8 = {rgs}, cell {row_plan.gg_cell(H, GH)}, "
          f"workspace {need} bytes")
    # the library's bound is row_plan's for the CU count it runs on
    assert need == (row_plan.gg_ws_bound(B, H, W, GH, GW, GD, p.C, cus) if p.fast else 0)
    assert need > 0 or not p.fast
    if cus == row_plan.MI355X_CUS:
        assert all(rg < row_plan.gg_cell(H, GH) for rg in rgs)
    for wanted in subsets(family):
        ws = Guarded(need, dev)
        name, outs = p.call(lib, wanted, ws)
        what = f"{frame_id(frame)} {variant_id(variant)} [{','.join(wanted)}]"
        assert name == kernel_name(family, wanted), (what, name)
        assert ws.intact(), what + ": guard band of the workspace overwritten"
        p.check(outs, what, check_dgrid, check_pix)
    assert p.inputs_unchanged()


def forced_cases():
    for frame, rgs in FORCED_FRAMES:
        for variant in VARIANTS:
            yield pytest.param(frame, rgs, variant, id=frame_id(frame) + "-" + variant_id(variant))


@pytest.mark.parametrize("frame,rgs,variant", list(forced_cases()))
def test_tools_library_every_plan(dev, tools, port, frame, rgs, variant):
    family, GD = variant
    B, H, W, GH, GW = frame
    cell = row_plan.gg_cell(H, GH)
    rgs = list(row_plan.gg_rg_range(H, GH)) if rgs is None else list(rgs)
    assert rgs and all(min(cell, row_plan.GG_MIN_RG) <= rg <= cell for rg in rgs)   # what the planner can return
    p = Problem(port, dev, frame, family, GD, seed_of(frame, family, GD))
    first = {}
    try:
        for rg in rgs:
            tools.hdrnet_tools_set_knob(FORCE_RG_KNOB, rg)
            need = row_plan.gg_plan_bytes(B, H, GW, GD, p.C, rg) if p.fast else 0
            assert p.query(tools) == need, (frame, variant, rg)
            for wanted in subsets(family):
                ws = Guarded(need, dev)
                name, outs = p.call(tools, wanted, ws)
                what = f"{frame_id(frame)} {variant_id(variant)} rg={rg} [{','.join(wanted)}]"
                assert name == kernel_name(family, wanted), (what, name)
                assert ws.intact(), what + ": guard band of the workspace overwritten"
                p.check(outs, what, check_dgrid, check_pix)
                for o in wanted[1:]:   # per-pixel gradients: the same bits under every plan
                    ref = first.setdefault((wanted, o), (rg, outs[o].t.clone()))
                    assert torch.equal(outs[o].t, ref[1]), f"{what}: {o} differs in bits from the plan rg={ref[0]}"
    finally:
        tools.hdrnet_tools_set_knob(FORCE_RG_KNOB, 0)
    assert p.inputs_unchanged()
    print(f"{frame_id(frame)} {variant_id(variant)}: plans rg = {rgs} (cell {cell})")


def test_forced_plan_is_part_of_the_workspace_query(tools):
    """The knob accepts 1 .. cell; the query follows it from one call to the next (its per-thread cache is keyed on
    it) and returns to the planner's bound with the knob at 0.  Queries only: nothing is launched."""
    frame, family, GD = (2, 37, 52, 3, 5), "apply_3_3_off", 8
    B, H, W, GH, GW = frame
    p = Problem(None, torch.device("cuda:0"), frame, family, GD, 1, oracle=False)
    cell = row_plan.gg_cell(H, GH)
    try:
        planned = p.query(tools)
        assert planned > 0
        for rg in (cell, 1, 5, cell, 4):
            tools.hdrnet_tools_set_knob(FORCE_RG_KNOB, rg)
            assert p.query(tools) == row_plan.gg_plan_bytes(B, H, GW, GD, p.C, rg), rg
        for rg in (cell + 1, -1, 1 << 20):
            tools.hdrnet_tools_set_knob(FORCE_RG_KNOB, rg)
            assert p.query(tools) == 0, rg
        tools.hdrnet_tools_set_knob(FORCE_RG_KNOB, 0)
        assert p.query(tools) == planned
    finally:
        tools.hdrnet_tools_set_knob(FORCE_RG_KNOB, 0)
