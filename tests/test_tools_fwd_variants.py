"""Forward variant numbers of the TOOLS library (include/hdrnet_amd_tools.h): 0, 19, 106 and 108 have kernels; 2 .. 11,
101, 103 .. 105 and 107 (the rejected forwards, the other memory skeletons and the empty launch) were retired with theirs.
The tools build must refuse a retired number by name instead of running the product kernel under it -- an old A/B script
would otherwise time the product against itself.

The refusal comes directly after the flags check of the shared forward front-end, before any HIP call and before any
pointer is looked at, so this runs without a GPU on placeholder pointers.  Every call here is shaped so that it cannot
launch even where there is a GPU: a retired number is refused by number, and the variants that remain are called with
grid == NULL, which the front-end refuses ("null buffer") before it picks a kernel."""
import ctypes
import os

import pytest

RETIRED = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 101, 103, 104, 105, 107]
REMAINING = [19, 106, 108]
P = 0x1000  # never dereferenced
B, H, W, GH, GW, GD = 1, 4, 16, 2, 2, 2


@pytest.fixture(scope="module")
def tools():
    from hdrnet_amd import _lib, build
    if not os.path.exists(build.TOOLS_LIB_PATH):
        pytest.skip("tools library not built")
    lib = ctypes.CDLL(build.build(tools=True))
    for fn in ("hdrnet_bilateral_slice_apply_f32_ex", "hdrnet_bilateral_slice_apply_rows_f32_ex"):
        getattr(lib, fn).restype, getattr(lib, fn).argtypes = _lib.SIGNATURES[fn]
    lib.hdrnet_last_error.restype = ctypes.c_char_p
    return lib


def frames(lib, variant, family, grid):
    """3 -> 3 with offset, whole frames."""
    rc = lib.hdrnet_bilateral_slice_apply_f32_ex(grid, P, P, P, B, H, W, GH, GW, GD, 3, 3, 1, family | (variant << 8), None)
    return rc, lib.hdrnet_last_error().decode()


def rows(lib, variant, family, grid):
    """The same frame through the row-band entry point (the whole frame as one band: variants take whole frames)."""
    rc = lib.hdrnet_bilateral_slice_apply_rows_f32_ex(grid, P, P, P, B, H, 0, H, W, GH, GW, GD, 3, 3, 1,
                                                      family | (variant << 8), None)
    return rc, lib.hdrnet_last_error().decode()


def retired_text(variant):
    return (f"forward kernel variant {variant} is not in this library: variants 2..11, 101, 103..105 and 107 were "
            "retired with their kernels, 0, 19, 106 and 108 remain (include/hdrnet_amd_tools.h)")


@pytest.mark.parametrize("entry", [frames, rows], ids=["frames", "rows"])
@pytest.mark.parametrize("variant", RETIRED)
def test_retired_variants_are_refused_by_number(tools, entry, variant):
    from hdrnet_amd import _lib
    for family in (_lib.KERNEL_AUTO, _lib.KERNEL_FAST, _lib.KERNEL_GENERIC):
        for grid in (None, P):  # the first check after the flags: with or without buffers, nothing is dereferenced
            rc, err = entry(tools, variant, family, grid)
            assert rc == _lib.HDRNET_INVALID_ARGUMENT and err == retired_text(variant), (family, rc, err)


@pytest.mark.parametrize("entry", [frames, rows], ids=["frames", "rows"])
@pytest.mark.parametrize("variant", REMAINING)
def test_remaining_variants_pass_the_variant_check(tools, entry, variant):
    """19, 106 and 108 get as far as the front-end's buffer check."""
    from hdrnet_amd import _lib
    for family in (_lib.KERNEL_AUTO, _lib.KERNEL_FAST, _lib.KERNEL_GENERIC):
        rc, err = entry(tools, variant, family, None)
        assert rc == _lib.HDRNET_INVALID_ARGUMENT and err == "null buffer", (family, rc, err)


def test_a_retired_number_on_a_row_band_is_refused_by_number(tools):
    """... before the band check ("kernel variants take whole frames"), which the remaining numbers get."""
    from hdrnet_amd import _lib

    def band(variant):
        rc = tools.hdrnet_bilateral_slice_apply_rows_f32_ex(None, P, P, P, B, 2 * H, H, H, W, GH, GW, GD, 3, 3, 1,
                                                            _lib.KERNEL_FAST | (variant << 8), None)
        return rc, tools.hdrnet_last_error().decode()

    assert band(5) == (_lib.HDRNET_INVALID_ARGUMENT, retired_text(5))
    assert band(106) == (_lib.HDRNET_INVALID_ARGUMENT, "kernel variants take whole frames")
