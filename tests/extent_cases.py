"""The shapes at the ends of the extents the C ABI admits, stated once with the reason for each (plain Python: importable
without a GPU).  tests/test_gpu_extent_edges.py runs them, tests/test_extent_edges_host.py calls the entry points that
refuse them, tests/test_row_geom.py holds hdrnet_amd/csrc/row_geom.h to the predictions.

Every limit, and where it is decided:

  limit                                decided in                                          first shape beyond it
  -----------------------------------  --------------------------------------------------  ---------------------------------
  W <= 2^23 (x + 0.5f exact)           row_geom.h kMaxFloatX: Plan::vec4, gg_plan          W = 2^23 + 4 (four-pixel kernels)
  B, H <= 65535                        row_geom.h kLimBH (segment family: 3-D grid)        H = 65536; B = 65536
  row < 2^31 bytes                     row_geom.h kLimRowBytes (segment family)            W = ceil(2^31 / 12) (3 channels)
  B * H * nseg * threads <= 2^32 - 1   row_geom.h kLimBlocks (row family: 1-D grid)        1024 x 65536 rows of 4 pixels
  B * H * W <= 2^32 - 256              capi.hip kGenericMaxPixels (generic kernels)        65536 x 65536 x 4, no staged kernel
  staged image < 2^20 elements         row_geom.h kLimImage                                (tests/golden/row_geom.json)
  nyg, B, GH <= 65535                  grid_grad_mfma.hip gg_plan                          H = 65536 on GH = 65535; B = 65536
  B * H * W <= 2^31 * 64 - 64          capi.hip check_common                               65536 x 65536 x 32
  image < 2^31 / 12 px, B <= 65535     capi.hip prepare_impl (sample preparation)          10923 x 16384; B = 65536
  B * Hin * Win * 12 < 2^40            capi.hip hdrnet_resize_bilinear_io                  65536 x 65536 x 22

The sides come from the predicates as tests/row_plan.py restates them (LIMIT_SIDES below asserts each pair), not from
trying.  Three axes: wide rows, tall and deep frames, far offsets.
"""
import row_plan as rp

# ---- 1. wide rows ----------------------------------------------------------------------------------------------------
# One row of 2^23 + 8 pixels is the first frame size of the issue beyond kMaxFloatX whose lanes at x >= 2^23 disagree with
# the reference's (x + k) + 0.5f (k = 1, 3: ties to even); 2^24 + 64 is beyond the 24-bit multiplies of the gradient
# pass and beyond the integers a float holds.  GH = 1, GW = 16, GD = 8, 3 -> 3 with offset; B = 1.  A float tensor of
# 3 channels is 0.1 / 0.2 GB per row.
WIDE_W = ((1 << 23) + 8, (1 << 24) + 64)
WIDE_GRID = (1, 16, 8)  # GH, GW, GD
WIDE = [(H, W) for W in WIDE_W for H in (1, 2)]
WIDE_SCALAR_NEIGHBOUR = (1, (1 << 23) + 9)  # W % 4 != 0: the scalar row kernel whatever the width
WIDE_SLICE_C = 12
# the sides of the limit itself (predictions only: the GPU runs the issue's widths)
WIDE_SIDES = ((1 << 23), (1 << 23) + 4)

# ---- 2. tall and deep ------------------------------------------------------------------------------------------------
# kLimBH: H (or B) = 65535 is the last frame of the segment family's 3-D launch grid, 65536 the first of the row
# family's 1-D grid.  W = 4 is one lane of one segment, W = 8 two.  The batch has a 2 x 2 x 2 grid per image (25 MB).
TALL_GRID = (3, 2, 2)
TALL = [(1, H, W) + TALL_GRID for H in (65535, 65536) for W in (4, 8)]
DEEP_GRID = (2, 2, 2)
DEEP = [(B, 1, 4) + DEEP_GRID for B in (65535, 65536)]
# gg_plan's nyg: rows per task rg <= the cell height H / GH, so nyg = ceil(H / rg) > 65535 needs a cell of one row (rg = 1)
# and H > 65535, or a cell of two (rg = 2) and H > 131070; GH <= 65535 leaves GH = 65535 for both.  The one-row cell:
NYG = [(1, 65535, 4, 65535, 2, 2), (1, 65536, 4, 65535, 2, 2)]
NYG_TWO_ROW_CELL = [(1, 131070, 4, 65535, 2, 2), (1, 131071, 4, 65535, 2, 2)]  # predictions only (the same code path)
# kLimBlocks: the runtime refuses a one-dimensional launch of 2^32 threads.  Rows of 4 pixels are one 64-thread
# workgroup each, so 1023 x 65536 rows are the last launch of the row family and 1024 x 65536 the first that the generic
# kernel takes; the slice forward with one channel keeps it at 1 GB for the guide and 1 GB for the output.
LAUNCH = [(1023, 65536, 4, 2, 2, 2), (1024, 65536, 4, 2, 2, 2)]
LAUNCH_SLICE_C = 1


def _check_sides():
    """Each pair stands on either side of its limit, by the restated predicates."""
    GH, GW, GD = WIDE_GRID
    lo, hi = WIDE_SIDES
    assert rp.vec4(lo) and not rp.vec4(hi) and hi % 4 == 0
    assert rp.forward_kernel(1, 1, lo, GW, GD) == "apply_fwd_seg/vec4"
    assert rp.forward_kernel(1, 1, hi, GW, GD) == "apply_fwd_rows/scalar"
    assert rp.gg_reaches(1, 1, lo, GH, GW, GD) and not rp.gg_reaches(1, 1, hi, GH, GW, GD)
    for H, W in WIDE + [WIDE_SCALAR_NEIGHBOUR]:
        assert rp.forward_kernel(1, H, W, GW, GD) == "apply_fwd_rows/scalar"
        assert rp.slice_kernel(1, H, W, GW, GD, WIDE_SLICE_C) == "slice_fwd_rows"
        assert rp.grad_kernels(1, H, W, GH, GW, GD, True, True) == "apply_grad_generic"
        assert rp.fused_forward_kernel(1, H, W, GW, GD, "nnguide") is None
        assert rp.extent_limit(1, H, W, "seg") == "2^23" and rp.extent_limit(1, H, W, "rows4") == "2^23"
    for B, H, W, GH, GW, GD in TALL + DEEP:
        inside = B <= 65535 and H <= 65535
        assert rp.forward_kernel(B, H, W, GW, GD) == ("apply_fwd_seg/vec4" if inside else "apply_fwd_rows/vec4")
        assert rp.fused_forward_kernel(B, H, W, GW, GD, "nnguide") == \
            ("apply_fwd_seg/vec4+nnguide" if inside else "apply_fwd_rows/vec4+nnguide")
        assert (rp.extent_limit(B, H, W, "seg") is None) == inside
        assert rp.seg_reaches(B, H, W, GW, GD, io=True) == inside
        # the gradient pass has no bound on H (a task takes rg rows), one on B
        want = "apply_bwd_fused/mfma" if B <= 65535 else "apply_vjp_rows/vec4+apply_grad_generic"
        assert rp.grad_kernels(B, H, W, GH, GW, GD, True, True) == want
        assert rp.vjp_kernel(B, H, W, GW, GD) == ("apply_vjp_seg/vec4" if inside else "apply_vjp_rows/vec4")
    for pair in (NYG, NYG_TWO_ROW_CELL):
        (a, b) = pair
        assert rp.gg_plan(*a, 12, 8 * rp.MI355X_CUS)[1] == 65535 and rp.gg_plan(*b, 12, 8 * rp.MI355X_CUS) is None
        assert rp.gg_reaches(*a) and not rp.gg_reaches(*b)
    # kLimBlocks: 64 threads per one-lane segment, so 2^26 rows of 4 pixels are the first launch of 2^32 threads
    for B, H, W, GH, GW, GD in LAUNCH:
        fits = B * H * 64 < (1 << 32)
        assert rp.rows_reaches(B, H, W, GW, GD)[0] == fits
        assert rp.slice_kernel(B, H, W, GW, GD, LAUNCH_SLICE_C) == ("slice_fwd_rows" if fits else "slice_fwd_generic")
        assert (rp.extent_limit(B, H, W, "rows4") is None) == fits
    assert [b * h * 64 for b, h, *_ in LAUNCH] == [(1 << 32) - (1 << 22), 1 << 32]
    assert rp.extent_limit(1024, 65536, 4, "rows4") == "2^32 - 1"
    # kLimRowBytes: beyond kMaxFloatX (see UNDEMONSTRATED); the sides by arithmetic
    w = -(-(1 << 31) // 48) * 4
    assert (w - 4) * 12 < (1 << 31) <= w * 12 and rp.extent_limit(1, 1, w, "seg") == "2^31 bytes"


LIMIT_SIDES = _check_sides  # tests/test_extent_edges_host.py calls it

# ---- 3. far offsets --------------------------------------------------------------------------------------------------
# Batches of small images whose LAST image lies wholly beyond byte offset 2^31 (2^32) of the call's widest tensor; image b
# is a copy of base image b % 3, expanded on the device, so the CPU oracle runs on three base images.  An image is
# 90 x 1920: two segments of 960 pixels (a row plan with idle lanes), rows of whole 128-B lines, 172 800 pixels.
FAR_H, FAR_W = 90, 1920
FAR_GRID = (4, 8, 8)  # GH, GW, GD
CAP_BYTES = 8 << 30   # live device memory of one case: a condition, not a goal


def far_batch(bytes_per_px, power):
    """(B, index of the image that straddles 2^power): the smallest multiple of 3 images such that the last one starts
    at or beyond byte 2^power of a tensor of `bytes_per_px`."""
    image = FAR_H * FAR_W * bytes_per_px
    B = -(-(1 << power) // image) + 1
    B += -B % 3
    assert (B - 1) * image >= (1 << power) > (B - 2) * image - 2 * image
    return B, (1 << power) // image


# What a far-offset test holds beside its operands: the grids and their gradients (1038 x 4 x 8 x 8 x 12 floats, twice),
# the workspace of the gradient pass or of a reduction, and the temporaries of its checks, which go over the batch in
# chunks of FAR_CHUNK images (a NaN mask, an inequality mask and a difference of at most 16 B/px each).
FAR_CHUNK = 30
FAR_EXTRA_BYTES = (64 << 20) + FAR_CHUNK * 90 * 1920 * 16 * 3


def _far(name, power, widest, tensors, note=""):
    """`tensors`: bytes per pixel of every operand and output of the call; FAR_EXTRA_BYTES on top."""
    B, straddle = far_batch(widest, power)
    live = B * FAR_H * FAR_W * sum(tensors) + FAR_EXTRA_BYTES
    assert live < CAP_BYTES, (name, live)
    return dict(name=name, power=power, widest=widest, B=B, straddle=straddle, live_bytes=live, note=note)


# name, power, bytes/px of the widest tensor, bytes/px of everything live.  Live device memory per case in the comment.
FAR = {c["name"]: c for c in (
    _far("slice forward C = 12", 32, 48, (4, 48)),                       # 519 images: guide 0.36 + out 4.30 = 4.66 GB
    _far("apply forward 3 -> 3", 31, 12, (4, 12, 12)),                   # 1038 images: 0.72 + 2.15 + 2.15 = 5.02 GB
    _far("all three gradients", 31, 12, (4, 12, 12, 4, 12)),             # + dguide, dinput: 7.89 GB with dout (+ 0.3)
    _far("apply_vjp_seg alone", 31, 12, (4, 12, 12, 4, 12)),             # the same tensors without dgrid
    _far("guide-network forward", 31, 12, (12, 12, 4)),                  # input, out, guide copy: 5.02 GB
    _far("u8 -> f32 wire format", 31, 12, (4, 3, 12)),                   # guide, u8 input, f32 out: 3.41 GB
    _far("u16 -> f32 wire format", 31, 12, (4, 6, 12)),                  # 3.95 GB
    _far("up-add", 31, 12, (4, 12, 12)),                                 # + a 23 x 480 coarse level per image: 5.2 GB
    _far("resize_bilinear (output side)", 31, 12, (12,)),                # out 2.15 GB + the 23 x 480 inputs
    _far("guide-network VJP", 31, 12, (12, 4, 4, 12)),                   # input, guide, dguide, dinput: 5.74 GB
    _far("input_moments", 31, 12, (12,)),                                # 2.15 GB + its workspace
    _far("l2_loss and its gradient", 31, 12, (12, 12, 12)),              # prediction, target, dprediction: 6.46 GB
)}
# The gradient call holds guide, input, dout, dguide, dinput: 44 B/px = 7.9 GB at 1038 images, under the cap; the same
# call beyond 2^32 would need 15.8 GB, so it crosses 2^31 only.  Every 2^31 case above crosses 2^31 only for the same
# reason or because 2^32 adds nothing its 2^31 case and the slice forward do not show: all row bases are 64-bit
# (size_t)row * W products, one code path on either side of 2^32.
COARSE_H, COARSE_W = 23, 480

# What stays undemonstrated, named as such (DESIGN.md section 4.1 repeats it):
UNDEMONSTRATED = (
    "check_common's bound of 2^31 * 64 pixels: 1.6 TB of float32 RGB",
    "kLimRowBytes: a row of 2^31 bytes is beyond kMaxFloatX for every kernel that has the limit; only the refusal is tested",
    "kGenericMaxPixels: a frame of 2^32 pixels is 17 GB for a one-channel slice; only the refusal is tested",
    "hdrnet_resize_bilinear_f32 beyond 2^32 output pixels: the runtime refuses its launch (HDRNET_RUNTIME_FAILURE)",
    "far offsets beyond 2^32 for every family but the slice forward: the 8 GiB cap",
    "sample preparation at far offsets",
    "hdrnet_resize_bilinear_io's 2^40-byte input bound",
)
