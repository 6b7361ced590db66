"""The extent limits of the C ABI without a GPU: validation precedes every HIP call, so an entry point that has no other
kernel to fall back to answers the first extent beyond a limit (tests/extent_cases.py) with rc = 1 and a text that names
the limit that binds -- not the channel counts, W % 4 or alignment its shape rules speak of.  Pointers are dummies, never
dereferenced.  (The entry points WITH a fallback take such a frame on another kernel: tests/test_gpu_extent_edges.py.)"""
import ctypes

import pytest

import extent_cases
import row_plan as rp

A = 0x1000  # a 16-byte aligned non-null "device pointer"
WIDE = (1 << 23) + 4
ROW_2G = -(-(1 << 31) // 48) * 4


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for table in (_lib.SIGNATURES, _lib.TRAIN_SIGNATURES, _lib.PYRAMID_IO_SIGNATURES, _lib.PIXEL_FORMAT_SIGNATURES):
        for name, (res, args) in table.items():
            getattr(lib, name).restype = res
            getattr(lib, name).argtypes = args
    lib.hdrnet_last_error.restype = ctypes.c_char_p
    return lib


def test_every_pair_of_shapes_stands_on_either_side_of_its_limit():
    extent_cases.LIMIT_SIDES()
    for case in extent_cases.FAR.values():
        image = extent_cases.FAR_H * extent_cases.FAR_W
        assert case["live_bytes"] < extent_cases.CAP_BYTES and case["B"] % 3 == 0 and case["B"] <= 65535, case
        assert case["straddle"] < case["B"] - 1, case
        assert image % 4 == 0  # whole 16-byte vectors per image: the reductions' alignment


# ---- the entry points, by the arguments after (B, H, W) ---------------------------------------------------------------
def nnguide(lib, B, H, W, ex):
    if ex:
        return lib.hdrnet_bilateral_slice_apply_nnguide_f32_ex(A, A, A, A, A, None, B, H, W, 2, 2, 2, 3, 3, 1, 16, 0, None)
    return lib.hdrnet_bilateral_slice_apply_nnguide_f32(A, A, A, A, A, None, B, H, W, 2, 2, 2, 3, 3, 1, 16, None)


def upadd(lib, B, H, W, ex):
    if ex:
        return lib.hdrnet_bilateral_slice_apply_upadd_f32_ex(A, A, A, A, 2, 2, A, B, H, W, 2, 2, 2, 3, 3, 1, None, None, 0, 0, None)
    return lib.hdrnet_bilateral_slice_apply_upadd_f32(A, A, A, A, 2, 2, A, B, H, W, 2, 2, 2, 3, 3, 1, None, None, 0, None)


def io(lib, B, H, W, which):
    tail = (B, H, W, 2, 2, 2, 3, 3, 1, 1, 255.0, 1)
    if which == "io":
        return lib.hdrnet_bilateral_slice_apply_io(A, A, A, A, *tail, None, None, 0, None, None)
    if which == "io_ex":
        return lib.hdrnet_bilateral_slice_apply_io_ex(A, A, A, A, *tail, None, None, 0, None, 0, None)
    if which == "io_px":  # BGRA frames
        return lib.hdrnet_bilateral_slice_apply_io_px(A, A, A, A, *tail, None, None, 0, None, 0, 3, 3, None)
    if which == "io_curves":
        return lib.hdrnet_bilateral_slice_apply_io_curves(A, A, A, *tail, A, A, A, A, 16, None, None)
    if which == "io_curves_prepared":
        return lib.hdrnet_bilateral_slice_apply_io_curves_prepared(A, A, A, *tail, A, A, A, A, 16, A, None, None)
    if which == "io_curves_px":  # BGR frames
        return lib.hdrnet_bilateral_slice_apply_io_curves_px(A, A, A, *tail, A, A, A, A, 16, None, None, 1, 1, None)
    assert which == "upadd_io_ex"
    return lib.hdrnet_bilateral_slice_apply_upadd_io_ex(A, A, A, A, 2, 2, A, B, H, W, 2, 2, 2, 3, 3, 1, 1, 255.0, 1, None, None, 0,
                                                        0, None)


ROW_FAMILY = [("nnguide", nnguide, False), ("nnguide_ex", nnguide, True), ("upadd", upadd, False), ("upadd_ex", upadd, True)]
SEG_FAMILY = ["io", "io_ex", "io_px", "io_curves", "io_curves_prepared", "io_curves_px", "upadd_io_ex"]
# (B, H, W) -> the word of the limit, as tests/row_plan.py predicts it
ROW_EXTENTS = [(1, 1, WIDE), (1024, 65536, 4)]
SEG_EXTENTS = [(1, 65536, 4), (65536, 1, 4), (1, 1, WIDE), (1, 1, ROW_2G)]


def refused_by_name(lib, rc, B, H, W, word):
    err = lib.hdrnet_last_error().decode()
    assert rc == 1, (rc, err)
    assert word in err and f"(B={B}, H={H}, W={W})" in err, err
    for other in ("W % 4", "aligned", "Cin"):  # the shape rules are not what binds
        assert other not in err, err


@pytest.mark.parametrize("B,H,W", ROW_EXTENTS)
@pytest.mark.parametrize("name,fn,ex", ROW_FAMILY, ids=[r[0] for r in ROW_FAMILY])
def test_fused_forwards_on_the_row_family_name_the_limit(lib, name, fn, ex, B, H, W):
    word = rp.extent_limit(B, H, W, "rows4")
    assert word is not None
    refused_by_name(lib, fn(lib, B, H, W, ex), B, H, W, word)


@pytest.mark.parametrize("B,H,W", SEG_EXTENTS)
@pytest.mark.parametrize("which", SEG_FAMILY)
def test_wire_format_forwards_name_the_limit(lib, which, B, H, W):
    word = rp.extent_limit(B, H, W, "seg")
    assert word is not None
    refused_by_name(lib, io(lib, B, H, W, which), B, H, W, word)


@pytest.mark.parametrize("which", SEG_FAMILY)
def test_shape_rules_keep_their_own_text(lib, which):
    """Inside the extents the refusal is the entry point's own: W % 4 (a frame of 6 columns)."""
    rc = io(lib, 1, 4, 6, which)
    err = lib.hdrnet_last_error().decode()
    assert rc == 1 and "W % 4" in err and "extents" not in err, (rc, err)


def test_image_too_large_for_every_slice_entry_point(lib):
    """check_common: B * H * W beyond 2^31 * 64 pixels."""
    B, H, W = 65536, 65536, 32
    assert B * H * W > 0x7fffffff * 64 >= 65536 * 65536 * 31
    calls = [
        lambda: lib.hdrnet_bilateral_slice_apply_f32(A, A, A, A, B, H, W, 2, 2, 2, 3, 3, 1, None),
        lambda: lib.hdrnet_bilateral_slice_f32(A, A, A, B, H, W, 2, 2, 2, 12, None),
        lambda: lib.hdrnet_bilateral_slice_apply_grad_f32(A, A, A, A, A, A, A, B, H, W, 2, 2, 2, 3, 3, 1, None, 0, None),
        lambda: lib.hdrnet_bilateral_slice_grad_f32(A, A, A, A, A, B, H, W, 2, 2, 2, 12, None, 0, None),
        lambda: nnguide(lib, B, H, W, True), lambda: upadd(lib, B, H, W, True),
    ] + [lambda w=w: io(lib, B, H, W, w) for w in SEG_FAMILY]
    for call in calls:
        assert call() == 1 and lib.hdrnet_last_error() == b"image too large"


def test_no_kernel_beyond_the_generic_kernels_launch(lib):
    """A frame no LDS-staged kernel takes (2^32 rows of one pixel are 2^38 threads of the row family) falls to the
    generic kernels, which launch one thread per pixel: beyond 2^32 - 256 pixels the entry points refuse by name instead
    of handing the runtime a launch it rejects."""
    B, H, W = 65536, 65536, 1
    assert B * H * W > rp.MAX_GENERIC_PIXELS and not rp.launch_fits(B, H, W)
    for what, call in (("BilateralSliceApply", lambda: lib.hdrnet_bilateral_slice_apply_f32(A, A, A, A, B, H, W, 2, 2, 2, 3, 3, 1, None)),
                       ("BilateralSlice", lambda: lib.hdrnet_bilateral_slice_f32(A, A, A, B, H, W, 2, 2, 2, 12, None))):
        rc, err = call(), lib.hdrnet_last_error().decode()
        assert rc == 1 and err.startswith(what + ": no kernel for this frame") and "2^32 - 256" in err, (rc, err)


@pytest.mark.parametrize("B,H,W,text", [(65536, 64, 64, "image or batch too large"), (1, 10923, 16384, "image or batch too large")])
def test_sample_preparation_extents(lib, B, H, W, text):
    """hdrnet_prepare_batch*, hdrnet_lowres_input*: B <= 65535, an image shorter than 2^31 bytes as float32 RGB."""
    assert B > 65535 or H * W * 12 >= (1 << 31) > (H - 1) * W * 12
    calls = {
        "hdrnet_prepare_batch": lambda: lib.hdrnet_prepare_batch(A, 1, 255.0, A, 1, 255.0, 2, H, W, A, B, A, A, H, W, None, 0, 1, None),
        "hdrnet_prepare_batch_ragged": lambda: lib.hdrnet_prepare_batch_ragged(A, 1, 255.0, A, 1, 255.0, 1000, A, 2, A, B, A, A, H, W,
                                                                               None, 0, 0, None),
        "hdrnet_lowres_input": lambda: lib.hdrnet_lowres_input(A, 1, 255.0, B, H, W, A, 16, None),
        "hdrnet_lowres_input_px": lambda: lib.hdrnet_lowres_input_px(A, 1, 255.0, B, H, W, A, 16, 3, None),
    }
    for name, call in calls.items():
        rc, err = call(), lib.hdrnet_last_error().decode()
        assert rc == 1 and err == f"{name}: {text}", (name, rc, err)


def test_resize_io_input_bound(lib):
    """hdrnet_resize_bilinear_io: B * Hin * Win * 12 < 2^40."""
    B, Hin, Win = 65536, 65536, 22
    assert B * Hin * Win * 12 >= (1 << 40) > B * Hin * (Win - 1) * 12
    assert lib.hdrnet_resize_bilinear_io(A, 1, 255.0, A, B, Hin, Win, 2, 2, 3, None) == 1
    assert lib.hdrnet_last_error() == b"hdrnet_resize_bilinear_io: input too large"
