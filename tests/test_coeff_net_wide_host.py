"""The coefficient network's training entry points for batches up to 32 (include/hdrnet_amd_coeff_wide.h: the ..._wide
twins of hdrnet_coefficients_grad_f32, hdrnet_coefficients_bn_train_f32, hdrnet_coefficients_bn_grad_f32 and of their
workspace queries) without a GPU: the symbols in header, library and binding table, the supported range as the queries
state it, the refusals with their texts -- and that the first entry points still stop at 8 images.  Validation precedes
any HIP call; pointers are small fake addresses."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

P = 0x1000
GRAD_Q, GRAD = "hdrnet_coefficients_grad_wide_workspace_bytes", "hdrnet_coefficients_grad_wide_f32"
BN_Q, BN_TRAIN = "hdrnet_coefficients_bn_wide_workspace_bytes", "hdrnet_coefficients_bn_train_wide_f32"
BN_GRAD_Q, BN_GRAD = "hdrnet_coefficients_bn_grad_wide_workspace_bytes", "hdrnet_coefficients_bn_grad_wide_f32"
NAMES = (GRAD_Q, GRAD, BN_Q, BN_TRAIN, BN_GRAD_Q, BN_GRAD)
NARROW = {n: n.replace("_wide", "") for n in NAMES}


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for n in NAMES:
        getattr(lib, n).restype, getattr(lib, n).argtypes = _lib.COEFF_WIDE_SIGNATURES[n]
        table = _lib.COEFF_BN_SIGNATURES if "_bn_" in n else _lib.SIGNATURES
        getattr(lib, NARROW[n]).restype, getattr(lib, NARROW[n]).argtypes = table[NARROW[n]]
    lib.hdrnet_last_error.restype = ctypes.c_char_p
    return lib


def fill(struct, over):
    """Every pointer a fake address, every field of `over` as given."""
    for name, ftype in struct._fields_:
        if name in over:
            v = over[name]
            setattr(struct, name, ftype(*v) if isinstance(v, list) else v)
        elif hasattr(ftype, "_length_"):
            setattr(struct, name, ftype(*([P] * ftype._length_)))
        elif ftype is ctypes.c_void_p:
            setattr(struct, name, P)
    return struct


HYPER = dict(net_input_size=256, spatial_bin=16, luma_bins=8, channel_multiplier=1, n_out=3, n_in=4, n_levels=1, fc_layout=1)


def describe(bn, **over):
    """The default network (256 -> 16 x 16 x 8, 3 x 4 coefficients), with or without the batch-norm members."""
    from hdrnet_amd import _lib
    fields = dict(HYPER, **(dict(eps=1e-3, momentum=1e-3) if bn else {}))
    fields.update(over)
    return fill(_lib.CoeffNetBn() if bn else _lib.CoeffNet(), fields)


def gradients(bn, **over):
    from hdrnet_amd import _lib
    return fill(_lib.CoeffNetBnGrads() if bn else _lib.CoeffNetGrads(), over)


def queries(lib, bn, B, wide=True, **over):
    net = describe(bn, **over)
    names = (BN_Q, BN_GRAD_Q) if bn else (GRAD_Q,)
    return tuple(getattr(lib, n if wide else NARROW[n])(ctypes.byref(net), B) for n in names)


def call(lib, name, net, gr=None, B=16, ws=P, nbytes=1 << 40, out=P):
    """Calls a forward (gr is None) or gradient entry point; (return code, error text)."""
    netp = ctypes.byref(net) if net is not None else None
    if name in (BN_TRAIN, NARROW[BN_TRAIN]):
        rc = getattr(lib, name)(P, netp, out, B, ws, nbytes, None)
    else:
        rc = getattr(lib, name)(P, netp, P, P, ctypes.byref(gr) if gr is not None else None, B, ws, nbytes, None)
    return rc, lib.hdrnet_last_error().decode()


def test_symbols_in_header_library_and_binding(lib):
    from hdrnet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hdrnet_amd_coeff_wide.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(hdrnet_[a-z0-9_]+)\s*\(", src))) == sorted(NAMES) == sorted(_lib.COEFF_WIDE_SIGNATURES)
    for n in NAMES:
        assert hasattr(lib, n), n
        m = re.search(r"\b" + n + r"\s*\(([^)]*)\)", src)
        assert len(m.group(1).split(",")) == len(_lib.COEFF_WIDE_SIGNATURES[n][1]), n
        # the signature of the twin
        table = _lib.COEFF_BN_SIGNATURES if "_bn_" in n else _lib.SIGNATURES
        assert _lib.COEFF_WIDE_SIGNATURES[n] == table[NARROW[n]], n
        assert n not in _lib.SIGNATURES and n not in _lib.TRAIN_SIGNATURES
    train = open(os.path.join(ROOT, "include", "hdrnet_amd_train.h")).read()
    assert '#include "hdrnet_amd_coeff_wide.h"' in train
    assert hasattr(_lib.load(), GRAD)  # bound by the loader too
    lib.hdrnet_version.restype = ctypes.c_int
    assert lib.hdrnet_version() >= 284


@pytest.mark.parametrize("bn", [False, True])
def test_batches_outside_the_range_have_no_workspace(lib, bn):
    for B in (0, 33, -1, 65536):
        assert not any(queries(lib, bn, B)), B
    assert not any(queries(lib, True, 1))       # a batch of one has no variance
    assert queries(lib, False, 1)[0] > 0
    for n in (GRAD_Q, BN_Q, BN_GRAD_Q):
        assert getattr(lib, n)(None, 16) == 0


@pytest.mark.parametrize("over", [dict(n_levels=3, n_out=9), dict(fc_layout=0), dict(luma_bins=6), dict(net_input_size=100),
                                  dict(n_out=1, n_in=3, luma_bins=2, channel_multiplier=2),
                                  dict(luma_bins=16, channel_multiplier=4)],
                         ids=["n_levels3", "fc_layout0", "luma_bins6", "N100", "pred6_not_x4", "gl512"])
@pytest.mark.parametrize("bn", [False, True])
def test_shapes_the_narrow_queries_refuse_have_no_workspace(lib, bn, over):
    for B in (2, 8):
        assert not any(queries(lib, bn, B, wide=False, **over)), "the case is meant to be one the narrow queries refuse"
    for B in (2, 8, 16, 32):
        assert not any(queries(lib, bn, B, **over)), B


@pytest.mark.parametrize("bn", [False, True])
def test_default_network_has_workspaces_and_agrees_with_the_narrow_queries(lib, bn):
    sizes = {B: queries(lib, bn, B) for B in (2, 8, 9, 16, 32)}
    for B, got in sizes.items():
        assert all(v > 0 and v % 16 == 0 for v in got), (B, got)
    for B in (2, 8):
        assert sizes[B] == queries(lib, bn, B, wide=False)
    for a, b in ((8, 9), (9, 16), (16, 32)):  # every buffer holds the whole batch
        assert all(x < y for x, y in zip(sizes[a], sizes[b]))


def test_refusals_name_the_entry_point_and_the_batch(lib):
    for B in (0, 33):
        rc, err = call(lib, GRAD, describe(False), gradients(False), B=B)
        assert rc == 1 and err.startswith(GRAD + ": ") and "unsupported" in err and f"B={B}" in err and "1 <= B <= 32" in err, err
    for B in (0, 1, 33):
        rc, err = call(lib, BN_TRAIN, describe(True), B=B)
        assert rc == 1 and err.startswith(BN_TRAIN + ": unsupported") and f"B={B}" in err and "2 <= B <= 32" in err, err
        rc, err = call(lib, BN_GRAD, describe(True), gradients(True), B=B)
        assert rc == 1 and err.startswith(BN_GRAD + ": unsupported") and f"B={B}" in err and "2 <= B <= 32" in err, err
    # a limit of the gradient kernels is named as the twin names it
    odd = dict(n_out=1, n_in=3, luma_bins=2, channel_multiplier=2)
    rc, err = call(lib, GRAD, describe(False, **odd), gradients(False))
    rc_n, err_n = call(lib, NARROW[GRAD], describe(False, **odd), gradients(False), B=2)
    assert rc == rc_n == 1 and "multiple of 4" in err_n and err == GRAD + ": " + err_n + "; B=16"
    # null descriptions, parameters, gradients, buffers
    assert call(lib, GRAD, None, gradients(False)) == (1, GRAD + ": null network description")
    assert call(lib, GRAD, describe(False), None) == (1, GRAD + ": null network description")
    assert call(lib, BN_TRAIN, None) == (1, BN_TRAIN + ": null network description")
    assert call(lib, BN_GRAD, describe(True), None) == (1, BN_GRAD + ": null network description")
    rc, err = call(lib, GRAD, describe(False, pred_b=None), gradients(False))
    assert rc == 1 and err == GRAD + ": coefficient network gradient: null parameter"
    rc, err = call(lib, BN_TRAIN, describe(True, pred_b=None))
    assert rc == 1 and err.startswith(BN_TRAIN + ": null parameter")
    rc, err = call(lib, BN_TRAIN, describe(True, local_beta=None))
    assert rc == 1 and err.startswith(BN_TRAIN + ": null beta, running_mean or running_var")
    rc, err = call(lib, BN_GRAD, describe(True), gradients(True, local_beta=None))
    assert rc == 1 and err.startswith(BN_GRAD + ": null gradient")
    rc, err = call(lib, BN_TRAIN, describe(True, eps=0.0))
    assert rc == 1 and err.startswith(BN_TRAIN + ": eps must be positive")
    rc, err = call(lib, BN_TRAIN, describe(True), out=None)
    assert (rc, err) == (1, BN_TRAIN + ": null buffer")


@pytest.mark.parametrize("B", [2, 16, 32])
def test_null_short_and_misaligned_workspaces_are_refused(lib, B):
    (need,) = queries(lib, False, B)
    fwd, bwd = queries(lib, True, B)
    def bad(size):
        return (dict(nbytes=size - 1), dict(ws=None), dict(ws=P + 4))

    for kw in bad(need):
        rc, err = call(lib, GRAD, describe(False), gradients(False), B=B, **kw)
        assert rc == 1 and err.startswith(GRAD + ": ") and GRAD_Q + "()" in err and f"= {need} bytes" in err, err
    for kw in bad(fwd):
        rc, err = call(lib, BN_TRAIN, describe(True), B=B, **kw)
        assert rc == 1 and err.startswith(BN_TRAIN + ": ") and BN_Q + "()" in err and f"= {fwd} bytes" in err, err
    for kw in bad(bwd):
        rc, err = call(lib, BN_GRAD, describe(True), gradients(True), B=B, **kw)
        assert rc == 1 and err.startswith(BN_GRAD + ": ") and BN_GRAD_Q + "()" in err and f"= {bwd} bytes" in err, err
    if B <= 8:  # the twins refuse the same calls
        for kw in bad(need):
            rc, err = call(lib, NARROW[GRAD], describe(False), gradients(False), B=B, **kw)
            assert rc == 1 and f"= {need} bytes" in err, err
        for kw in bad(bwd):
            rc, err = call(lib, NARROW[BN_GRAD], describe(True), gradients(True), B=B, **kw)
            assert rc == 1 and f"= {bwd} bytes" in err, err


def test_the_first_entry_points_still_stop_at_8_images(lib):
    """Their range and their texts are part of the interface (tests/test_coeff_reference.py,
    tests/test_coeff_net_bn_host.py, tests/golden/capi_errors.json pin them too)."""
    assert queries(lib, False, 9, wide=False) == (0,) and queries(lib, True, 9, wide=False) == (0, 0)
    assert queries(lib, False, 8, wide=False)[0] > 0 and all(queries(lib, True, 8, wide=False))
    rc, err = call(lib, NARROW[GRAD], describe(False), gradients(False), B=9)
    assert rc == 1 and err.startswith("coefficient network gradient: unsupported") and "1 <= B <= 8" in err and "B=9" in err
    for name, gr in ((NARROW[BN_TRAIN], None), (NARROW[BN_GRAD], gradients(True))):
        rc, err = call(lib, name, describe(True), gr, B=9)
        assert rc == 1 and err.startswith(name + ": unsupported") and "2 <= B <= 8" in err and "B=9" in err, err
