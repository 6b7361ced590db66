"""Gradient variant numbers of the TOOLS library (include/hdrnet_amd_tools.h): 0, 3 and 11 have kernels; 2 and 4 .. 10
(the split contractions, the timing ablations and the phase trace of the gradient pass) were retired with theirs.  The
tools build must refuse a retired number by name instead of running the product pass under it -- an old A/B script
would otherwise time the product against itself.

The refusal is the first thing the shared gradient dispatch does, before any HIP call and before any pointer is looked
at, so this runs without a GPU on placeholder pointers.  Every call here is shaped so that it cannot launch even where
there is a GPU: dgrid alone on the FAST family without a workspace is refused for the missing workspace by the variants
that remain, and the call with every buffer given is made only after that refusal has been seen for its variant."""
import ctypes
import os

import pytest

RETIRED = [2, 4, 5, 6, 7, 8, 9, 10]
REMAINING = [3, 11]
P = 0x1000  # never dereferenced
B, H, W, GH, GW, GD = 1, 8, 16, 2, 2, 2  # the smallest frame the fast pass admits: rows per task = cell height = 4


@pytest.fixture(scope="module")
def tools():
    from hdrnet_amd import _lib, build
    if not os.path.exists(build.TOOLS_LIB_PATH):
        pytest.skip("tools library not built")
    lib = ctypes.CDLL(build.build(tools=True))
    for fn in ("hdrnet_bilateral_slice_apply_grad_f32_ex", "hdrnet_bilateral_slice_grad_f32_ex"):
        getattr(lib, fn).restype, getattr(lib, fn).argtypes = _lib.SIGNATURES[fn]
    lib.hdrnet_last_error.restype = ctypes.c_char_p
    return lib


def apply_grad(lib, variant, family, dguide, dinput, ws, ws_bytes):
    """3 -> 3 with offset."""
    rc = lib.hdrnet_bilateral_slice_apply_grad_f32_ex(P, P, P, P, P, dguide, dinput, B, H, W, GH, GW, GD, 3, 3, 1, ws, ws_bytes,
                                                      family | (variant << 8), None)
    return rc, lib.hdrnet_last_error().decode()


def slice_grad(lib, variant, family, dguide, dinput, ws, ws_bytes):
    """C = 12 (the op has no dinput)."""
    rc = lib.hdrnet_bilateral_slice_grad_f32_ex(P, P, P, P, dguide, B, H, W, GH, GW, GD, 12, ws, ws_bytes,
                                                family | (variant << 8), None)
    return rc, lib.hdrnet_last_error().decode()


def retired_text(variant):
    return f"gradient kernel variant {variant} is not in this library: variants 2 and 4..10 were retired"


@pytest.mark.parametrize("entry", [apply_grad, slice_grad], ids=["apply", "slice"])
@pytest.mark.parametrize("variant", RETIRED)
def test_retired_variants_are_refused_by_number(tools, entry, variant):
    from hdrnet_amd import _lib
    rc, err = entry(tools, variant, _lib.KERNEL_FAST, None, None, None, 0)
    assert rc == 1 and err.startswith(retired_text(variant)), (rc, err)
    # ... and with every buffer and a workspace given, on every family: still the first check, nothing is dereferenced
    for family in (_lib.KERNEL_AUTO, _lib.KERNEL_GENERIC, _lib.KERNEL_FAST):
        rc, err = entry(tools, variant, family, P, P, P, 1 << 20)
        assert rc == 1 and err.startswith(retired_text(variant)), (family, rc, err)


@pytest.mark.parametrize("entry", [apply_grad, slice_grad], ids=["apply", "slice"])
@pytest.mark.parametrize("variant", REMAINING)
def test_remaining_variants_pass_the_variant_check(tools, entry, variant):
    """The same first call: variants 3 and 11 get as far as the fast pass's own refusal (no workspace)."""
    from hdrnet_amd import _lib
    rc, err = entry(tools, variant, _lib.KERNEL_FAST, None, None, None, 0)
    assert rc == 1 and "retired" not in err and f"variant {variant}" not in err, (rc, err)
    assert err.startswith("no fast grid-gradient variant for this shape"), err
