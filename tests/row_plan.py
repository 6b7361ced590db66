"""The row plan of the row-segment kernels, restated (hdrnet_amd/csrc/row_geom.h: make_row_plan, seg_fwd_geom,
rows_fwd_geom, io_fwd_geom) for Cin = Cout = 3 with offset (C = 12): the GPU tests predict from it which kernel a shape
reaches (tests/test_gpu_fused_fullsize.py), and tests/test_row_geom.py holds the header to it cell by cell."""
import numpy as np


def _rup(v, m):
    return (v + m - 1) // m * m


def row_plan(W):
    best = None
    for threads in (256, 192, 128):
        nseg = -(-W // (4 * threads))
        waste = nseg * 4 * threads - W
        if best is None or waste < best[0]:
            best = (waste, nseg)
    nseg = best[1]
    seg = _rup(-(-W // nseg), 4)
    return min(_rup(-(-seg // 4), 64), 256), nseg, seg


def seg_fits(W, GW, GD, guide_map, C=12, chan=3):
    """seg_fwd_geom(dma = true, guide_map).ok: (GD + 2) planes of the window's columns + the slabs in 64 KiB.  `C`: grid
    channels, `chan`: max(Cin, Cout), of a fast shape other than 3 -> 3 with offset."""
    threads, _, seg = row_plan(W)
    cols = (seg - 1) * GW // W + 4
    slabw = 256 * chan + (256 if guide_map else 0)
    return (_rup(cols * (GD + 2) * C, 4) + threads // 64 * slabw) * 4 <= 65536


def rows_fits(W, GW, GD, C=12, chan=3):
    """rows_fwd_geom(...).ok: GD planes of at most GW columns + the per-wave slabs in 64 KiB."""
    threads, _, seg = row_plan(W)
    cols = min((seg - 1) * GW // W + 4, GW)
    return (cols * GD * C + 4 + threads // 64 * 256 * chan) * 4 <= 65536


def io_fits(W, GW, GD):
    """io_fwd_geom(...).ok: the curves kernel's static tables (768 floats) + (GD + 2) planes + the slabs in 64 KiB."""
    threads, _, seg = row_plan(W)
    cols = (seg - 1) * GW // W + 4
    return (768 + _rup(cols * (GD + 2) * 12, 4) + threads // 64 * 256 * 3) * 4 <= 65536


# ---- the extent limits (row_geom.h: kMaxFloatX, kLimBH, kLimRowBytes, kLimBlocks, kLimImage; grid_grad_mfma.hip: gg_plan;
# capi.hip: kGenericMaxPixels)
# and, from them, the kernel a 3 -> 3 call with offset on 16-B aligned buffers reaches (tests/extent_cases.py,
# tests/test_gpu_extent_edges.py).
MAX_FLOAT_X = 1 << 23      # widest row of the four-pixels-per-lane kernels and of the gradient pass: x + 0.5f exact
MAX_BH = 65535             # B and H of the 3-D launch grids
MAX_ROW_BYTES = 1 << 31    # a pixel row is shorter than this
MAX_LAUNCH_THREADS = (1 << 32) - 1  # B * H * nseg * threads of the 1-D launch grids (the HIP runtime's bound)
MAX_GENERIC_PIXELS = (1 << 32) - 256  # the generic kernels: one thread per pixel in workgroups of 256
MI355X_CUS = 256


def vec4(W, aligned=True):
    """Plan::vec4."""
    return aligned and W % 4 == 0 and W <= MAX_FLOAT_X


def extent_limit(B, H, W, family, row_channels=3):
    """extent_refusal: the extent limit a frame breaks for `family` ("seg": kSegLimits; "rows4": the four-pixel kernels
    of the row family, kNeedVec4 | kRowsLimits), as the word the refusal text carries; None: it breaks none."""
    if family == "seg":
        if B > MAX_BH or H > MAX_BH:
            return "65535"
        if W * row_channels * 4 >= MAX_ROW_BYTES:
            return "2^31 bytes"
    if W > MAX_FLOAT_X:
        return "2^23"
    if family == "rows4" and not launch_fits(B, H, W):
        return "2^32 - 1"
    return None


def launch_fits(B, H, W):
    """kLimBlocks: the workgroups of a 1-D launch times their threads."""
    threads, nseg, _ = row_plan(W)
    return B * H * nseg * threads <= MAX_LAUNCH_THREADS


# HDRNET_APPLY_FAST_SHAPES of launch.hip.h: (Cin, Cout, has_offset)
APPLY_FAST_SHAPES = ((3, 3, True), (3, 3, False), (3, 4, True), (1, 1, True), (1, 1, False), (1, 3, True), (4, 4, True),
                     (4, 4, False))
SLICE_FAST_CHANNELS = (1, 2, 4, 8, 12, 16)   # HDRNET_SLICE_FAST_CHANNELS


def seg_reaches(B, H, W, GW, GD, guide_map=True, io=False, shape=(3, 3, True)):
    """The segment family's predicate for a frame: shape and LDS as above, and the extents."""
    Cin, Cout, off = shape
    C, chan = Cout * (Cin + off), max(Cin, Cout)
    _, _, seg = row_plan(W)
    staged = ((seg - 1) * GW // W + 4) * GD * C
    fits = io_fits(W, GW, GD) if io else seg_fits(W, GW, GD, guide_map, C, chan)
    return vec4(W) and fits and staged < (1 << 20) and extent_limit(B, H, W, "seg", Cout) is None


def rows_reaches(B, H, W, GW, GD, aligned=True, shape=(3, 3, True)):
    """rows_fwd_geom(...).ok for a frame, and whether the four-pixel kernel serves it."""
    Cin, Cout, off = shape
    ok = rows_fits(W, GW, GD, Cout * (Cin + off), max(Cin, Cout)) and launch_fits(B, H, W)
    return ok, ok and vec4(W, aligned)


def forward_kernel(B, H, W, GW, GD, aligned=True, shape=(3, 3, True)):
    """hdrnet_bilateral_slice_apply_f32 under HDRNET_KERNEL_AUTO for the fast shape `shape` = (Cin, Cout, has_offset)
    (16-B aligned buffers: a grid of C % 4 != 0 channels is staged by single floats)."""
    assert tuple(shape) in APPLY_FAST_SHAPES, shape
    ok, four = rows_reaches(B, H, W, GW, GD, aligned, shape)
    if not ok:
        return "apply_fwd_generic"
    if aligned and seg_reaches(B, H, W, GW, GD, shape=shape):
        return "apply_fwd_seg/vec4"
    return "apply_fwd_rows/vec4" if four else "apply_fwd_rows/scalar"


def fused_forward_kernel(B, H, W, GW, GD, flavour):
    """..._nnguide_f32 / ..._upadd_f32 (`flavour` "nnguide", "upadd", "nnguide+upadd"): the segment kernel, else the
    four-pixel row kernel, else None -- the entry point refuses."""
    if seg_reaches(B, H, W, GW, GD, guide_map="nnguide" not in flavour):
        return "apply_fwd_seg/vec4+" + flavour
    return "apply_fwd_rows/vec4+" + flavour if rows_reaches(B, H, W, GW, GD)[1] else None


def slice_kernel(B, H, W, GW, GD, C):
    """hdrnet_bilateral_slice_f32 for a channel count the row kernel is instantiated for: GD planes of at most GW
    columns + 64 x C floats per wave in 64 KiB, the 1-D launch grid."""
    threads, nseg, seg = row_plan(W)
    cols = min((seg - 1) * GW // W + 4, GW)
    lds = (_rup(cols * GD * C, 4) + threads // 64 * 64 * C) * 4
    return "slice_fwd_rows" if lds <= 65536 and launch_fits(B, H, W) else "slice_fwd_generic"


def gg_plan(B, H, W, GH, GW, GD, C, slots):
    """gg_plan of grid_grad_mfma.hip: (rg, nyg) of the gradient pass on `slots` resident workgroups, or None where it
    refuses."""
    if GD > 16 or C > 32 or C < 1 or W > MAX_FLOAT_X:
        return None
    cell = max(H // GH, 1)
    rg_lo = min(cell, 4)
    cols = B * (GW + 1)
    rg, best = rg_lo, -1.0
    for R in range(1, 7):
        per_col = slots * R // cols
        if per_col < 1:
            continue
        cand = -(-H // per_col)
        if cand > cell:
            continue
        cand = max(cand, rg_lo)
        ntasks = cols * -(-H // cand)
        eff = ntasks / (-(-ntasks // slots) * slots)
        if eff > best + 1e-9:
            best, rg = eff, cand
    if best < 0.0:
        rg = cell
    rg = max(rg, 1)
    nyg = -(-H // rg)
    if cols * nyg > 0x7fffffff or B * GH * GW * GD > 0x7fffffff or nyg > 65535 or B > 65535 or GH > 65535:
        return None
    return rg, nyg


def gg_reaches(B, H, W, GH, GW, GD, C=12, cus=MI355X_CUS):
    """gg_ws_bound: the pass runs where the plan holds for every occupancy (1 .. 8 workgroups per CU) a launch may have."""
    return all(gg_plan(B, H, W, GH, GW, GD, C, occ * cus) is not None for occ in range(1, 9))


def vjp_kernel(B, H, W, GW, GD, want_dinput=True):
    """The per-pixel gradients alone: apply_vjp_seg, the row family's four-pixel kernel, or None (the generic ones)."""
    threads, nseg, seg = row_plan(W)
    if not vec4(W):
        return None
    cols = (seg - 1) * GW // W + 4
    seg_lds = (_rup(cols * (GD + 2) * 12, 4) + threads // 64 * 256 * 7) * 4
    if seg_lds <= 65536 and cols * GD * 12 < (1 << 20) and extent_limit(B, H, W, "seg") is None:
        return "apply_vjp_seg/vec4"
    rows_lds = (min(cols, GW) * GD * 12 + 4 + threads // 64 * 256 * 3) * 4
    return "apply_vjp_rows/vec4" if rows_lds <= 65536 and launch_fits(B, H, W) else None


def grad_kernels(B, H, W, GH, GW, GD, need_guide, need_input):
    """hdrnet_bilateral_slice_apply_grad_f32 asked for dgrid and the given per-pixel gradients, with the workspace its
    query answers: hdrnet_last_kernel()."""
    mfma = gg_reaches(B, H, W, GH, GW, GD)
    if not (need_guide or need_input):
        return "grid_grad_mfma" if mfma else "apply_grad_generic"
    if mfma:
        return "apply_bwd_fused/mfma"
    pix = vjp_kernel(B, H, W, GW, GD, need_input)
    return pix + "+apply_grad_generic" if pix else "apply_grad_generic"


# ---- the gradient pass's workspace and stage 2's view of the row groups (grid_grad_mfma.hip: gg_plan, gg_ws_bound,
# gy_base_of, grid_grad_stage2), restated so that tests/test_grad_plan_host.py can hold the float arithmetic of the two
# stages against each other on the CPU and tests/test_gpu_grad_plans.py can size a workspace for a plan it forces.
GG_TILE_FLOATS = 3 * 16 * 16   # kTileFloats: a task's partial tile, [rel 3][k 16][c 16]
GG_MAX_OCC = 8                 # kMaxOcc: workgroups per CU a stage-1 kernel can have
GG_MIN_RG = 4                  # kMinRg


def gg_cell(H, GH):
    return max(H // GH, 1)


def gg_rg_range(H, GH):
    """The rows per task gg_plan can return: min(cell, 4) .. cell."""
    cell = gg_cell(H, GH)
    return range(min(cell, GG_MIN_RG), cell + 1)


def gg_plan_bytes(B, H, GW, GD, C, rg):
    """GGPlan::ws_bytes of the plan with `rg` rows per task: one tile per task, plane half and channel window."""
    ntasks = B * (GW + 1) * -(-H // rg)
    return ntasks * (2 if GD > 8 else 1) * (2 if C > 16 else 1) * GG_TILE_FLOATS * 4


def gg_ws_bound(B, H, W, GH, GW, GD, C, cus=MI355X_CUS):
    """gg_ws_bound: the largest plan over 1 .. 8 workgroups per CU of a `cus`-CU device; 0 where a plan refuses."""
    worst = 0
    for occ in range(1, GG_MAX_OCC + 1):
        plan = gg_plan(B, H, W, GH, GW, GD, C, occ * cus)
        if plan is None:
            return 0
        worst = max(worst, gg_plan_bytes(B, H, GW, GD, C, plan[0]))
    return worst


def gg_scale_y(H, GH):
    """(float)GH / H, as both stages receive it."""
    return np.float32(GH) / np.float32(H)


def gg_gy0(y, scale_y):
    """floor_to_int(mul_rn(y + 0.5f, scale_y) - 0.5f) of the rows `y` (an integer array), in float32."""
    gyf = (np.asarray(y).astype(np.float32) + np.float32(0.5)) * scale_y
    return np.floor(gyf - np.float32(0.5)).astype(np.int64)


def gg_gy_base(y_first, scale_y, GH):
    """gy_base_of: the first of the three clamped grid rows the tile of the task starting at row `y_first` holds."""
    return np.clip(gg_gy0(y_first, scale_y), 0, GH - 1)


def gg_stage2_window(gy, scale_y, rg, nyg):
    """(yg_lo, yg_hi) of grid_grad_stage2 for the grid rows `gy`: the row groups it looks at.  C's int division
    truncates toward zero, which matters for the negative numerators of gy < 2."""
    gy = np.asarray(gy).astype(np.float32)
    lo = np.floor((gy - np.float32(2.0)) / scale_y).astype(np.int64)
    hi = np.ceil((gy + np.float32(2.5)) / scale_y).astype(np.int64)
    trunc_div = lambda a: np.sign(a) * (np.abs(a) // rg)  # noqa: E731
    return np.maximum(0, trunc_div(lo) - 1), np.minimum(nyg, trunc_div(hi) + 2)
