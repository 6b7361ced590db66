"""The launch plans of the fused gradient pass (grid_grad_mfma.hip) on the CPU.

gg_plan picks rg, the rows per workgroup task, from the resident-workgroup count of the stage-1 variant it launches
(occupancy x CUs of the device).  Stage 1 keeps, per task, the three clamped grid rows from gy_base_of(first row) on;
stage 2 finds the tasks of a grid row through a float window of row groups and then the exact `rel` test.  Both are
float32 arithmetic on rg, H and GH.  This file holds

* stage 2's window against stage 1's rows for every rg a plan can have (tests/row_plan.py restates both in numpy
  float32): every (row group, grid row) pair a pixel row contributes to lies inside the window of that grid row, and
  every row's two grid rows lie at rel 0 .. 2 of its task's tile -- over every H, GH of the sweep below and every rg
  in 1 .. cell.  tests/test_gpu_grad_plans.py then runs such plans on the device;
* the planner over CU counts 32 .. 304 and occupancies 1 .. 8 for the frames the GPU tests use: a plan exists, rg lies
  in [min(cell, 4), cell], and the workspace bound covers it;
* that the frames tests/test_gpu_grad_plans.py runs on the product library have rg < cell at every occupancy on a
  256-CU device -- the product library cannot be told a plan, so the frames must not depend on the register allocation
  of the day to reach a task that straddles a grid-row boundary inside a cell.
"""
import numpy as np
import pytest

import row_plan

from grad_plan_cases import FAMILIES, FORCED_FRAMES, PRODUCT_FRAMES, VARIANTS, grid_channels  # noqa: E402

# GD, C of the variants the GPU tests run: 3 -> 3 with offset at 8 and 16 planes, 4 -> 4 with offset (two channel
# windows), the slice op with 12 and 3 channels
GRIDS = sorted({(gd, grid_channels(f)) for f, gd in VARIANTS})
assert set(f for f, _ in VARIANTS) == set(FAMILIES) and (16, 20) in GRIDS and (8, 3) in GRIDS
CU_COUNTS = (32, 64, 128, 256, 304)

SWEEP_H = list(range(1, 80)) + [96, 100, 128, 135, 200, 270, 271, 540, 1080, 1081, 2160, 3000]
SWEEP_GH = (1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 32, 64)


def forced_rgs(frame, rgs):
    _, H, _, GH, _ = frame
    return list(row_plan.gg_rg_range(H, GH)) if rgs is None else list(rgs)


def check_window(H, GH, rg):
    """-> the number of (row group, grid row) memberships of the plan; asserts the two properties."""
    scale_y = row_plan.gg_scale_y(H, GH)
    y = np.arange(H)
    yg = y // rg
    nyg = -(-H // rg)
    base = row_plan.gg_gy_base(np.arange(nyg) * rg, scale_y, GH)[yg]       # of each row's task
    gy0 = row_plan.gg_gy0(y, scale_y)
    lo_of, hi_of = row_plan.gg_stage2_window(np.arange(GH), scale_y, rg, nyg)  # of each grid row
    member = np.zeros(nyg * GH, dtype=bool)
    for tap in (0, 1):
        gy = np.clip(gy0 + tap, 0, GH - 1)
        rel = gy - base
        assert rel.min() >= 0 and rel.max() <= 2, (H, GH, rg, "rel", int(rel.min()), int(rel.max()))
        lo, hi = lo_of[gy], hi_of[gy]
        inside = (lo <= yg) & (yg < hi)
        assert inside.all(), (H, GH, rg, "row", int(y[~inside][0]), "outside the window of grid row", int(gy[~inside][0]))
        member[yg * GH + gy] = True
    return int(member.sum())


def test_stage2_window_holds_every_task_of_a_grid_row():
    total = plans = 0
    for H in SWEEP_H:
        for GH in SWEEP_GH:
            for rg in range(1, row_plan.gg_cell(H, GH) + 1):
                total += check_window(H, GH, rg)
                plans += 1
    print(f"{plans} plans, {total} (row group, grid row) memberships, all inside the window")
    assert plans > 20000 and total > 550686


def test_window_of_the_gpu_frames():
    """The frames the GPU sweep runs, by name (they are part of the sweep above as well: H and GH are listed there)."""
    for (_, H, _, GH, _), rgs in [(f, None) for f in PRODUCT_FRAMES] + FORCED_FRAMES:
        assert H in SWEEP_H and GH in SWEEP_GH
        for rg in forced_rgs((0, H, 0, GH, 0), rgs):
            assert 1 <= rg <= row_plan.gg_cell(H, GH)
            check_window(H, GH, rg)


def test_the_window_test_sees_a_window_that_is_too_narrow():
    """The check has teeth: with the `+ 2` of yg_hi taken away the membership fails on a plain shape."""
    real = row_plan.gg_stage2_window

    def narrow(gy, scale_y, rg, nyg):
        lo, hi = real(gy, scale_y, rg, nyg)
        return lo, np.minimum(nyg, hi - 2)

    row_plan.gg_stage2_window = narrow
    try:
        with pytest.raises(AssertionError):
            for rg in range(1, 68):
                check_window(1080, 16, rg)
    finally:
        row_plan.gg_stage2_window = real


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_planner_over_cu_counts_and_occupancies(cus):
    for B, H, W, GH, GW in PRODUCT_FRAMES + [f for f, _ in FORCED_FRAMES]:
        cell = row_plan.gg_cell(H, GH)
        for GD, C in GRIDS:
            bound = row_plan.gg_ws_bound(B, H, W, GH, GW, GD, C, cus)
            assert bound > 0
            for occ in range(1, row_plan.GG_MAX_OCC + 1):
                plan = row_plan.gg_plan(B, H, W, GH, GW, GD, C, occ * cus)
                assert plan is not None, (B, H, W, GH, GW, GD, C, cus, occ)
                rg, nyg = plan
                assert min(cell, row_plan.GG_MIN_RG) <= rg <= cell, (B, H, W, GH, GW, cus, occ, rg)
                assert nyg == -(-H // rg)
                assert bound >= row_plan.gg_plan_bytes(B, H, GW, GD, C, rg)
            # the bound is reached by one of the eight plans, and a forced plan's size is the formula's
            assert bound == max(row_plan.gg_plan_bytes(B, H, GW, GD, C,
                                                       row_plan.gg_plan(B, H, W, GH, GW, GD, C, occ * cus)[0])
                                for occ in range(1, 9))


def test_plan_bytes_formula():
    """ntasks * nh * nw * 3 * 16 * 16 * 4 bytes, spelled out once."""
    assert row_plan.gg_plan_bytes(2, 37, 5, 8, 12, 5) == 2 * 6 * 8 * 3072
    assert row_plan.gg_plan_bytes(2, 37, 5, 16, 12, 5) == 2 * 6 * 8 * 2 * 3072
    assert row_plan.gg_plan_bytes(2, 37, 5, 16, 20, 12) == 2 * 6 * 4 * 2 * 2 * 3072
    assert row_plan.gg_plan_bytes(1, 5, 4, 8, 3, 1) == 5 * 5 * 3072


@pytest.mark.parametrize("frame", PRODUCT_FRAMES, ids=lambda f: "x".join(map(str, f)))
def test_product_frames_straddle_at_every_occupancy(frame):
    """On 256 CUs every occupancy 1 .. 8 plans fewer rows per task than a cell is high: whatever variant runs, and
    however many registers it takes, tasks start and end inside cells."""
    B, H, W, GH, GW = frame
    cell = row_plan.gg_cell(H, GH)
    for GD, C in GRIDS:
        rgs = [row_plan.gg_plan(B, H, W, GH, GW, GD, C, occ * row_plan.MI355X_CUS)[0] for occ in range(1, 9)]
        assert all(rg < cell for rg in rgs), (frame, cell, rgs)
        # ... and some task boundary really falls inside a cell (rg does not divide the cell into whole tasks)
        assert any(cell % rg for rg in rgs), (frame, cell, rgs)


def test_the_dispatch_frame_runs_the_degenerate_plan():
    """Why the frames above exist: tests/test_gpu_grad_dispatch.py's frame has fewer tasks than slots at every
    occupancy, so it runs rg = cell whatever the variant -- no task of it ends inside a cell."""
    B, H, W, GH, GW = 2, 12, 32, 3, 4
    assert {row_plan.gg_plan(B, H, W, GH, GW, 8, 12, occ * 256)[0] for occ in range(1, 9)} == {row_plan.gg_cell(H, GH)}
