"""The batch-norm training entry points of the coefficient network (include/hdrnet_amd_coeff_bn.h:
hdrnet_coefficients_bn_train_f32, hdrnet_coefficients_bn_grad_f32 and their workspace queries) without a GPU: the
supported range as the workspace queries state it, the refusals with their texts, and the symbols in header, library and
binding table.  Validation precedes any HIP call; pointers are small fake addresses."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

P = 0x1000
NAMES = ("hdrnet_coefficients_bn_workspace_bytes", "hdrnet_coefficients_bn_train_f32",
         "hdrnet_coefficients_bn_grad_workspace_bytes", "hdrnet_coefficients_bn_grad_f32")
TRAIN, GRAD = NAMES[1], NAMES[3]


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for n in NAMES:
        getattr(lib, n).restype, getattr(lib, n).argtypes = _lib.COEFF_BN_SIGNATURES[n]
    lib.hdrnet_last_error.restype = ctypes.c_char_p
    return lib


def describe(**over):
    """The default network (256 -> 16 x 16 x 8, 3 x 4 coefficients) with every pointer a fake address."""
    from hdrnet_amd import _lib
    net = _lib.CoeffNetBn()
    fields = dict(net_input_size=256, spatial_bin=16, luma_bins=8, channel_multiplier=1, n_out=3, n_in=4, n_levels=1,
                  fc_layout=1, eps=1e-3, momentum=1e-3)
    fields.update(over)
    for name, ftype in net._fields_:
        if name in fields:
            v = fields[name]
            setattr(net, name, ftype(*v) if isinstance(v, list) else v)
        elif hasattr(ftype, "_length_"):
            setattr(net, name, ftype(*([P] * ftype._length_)))
        else:
            setattr(net, name, P)
    return net


def gradients(**over):
    from hdrnet_amd import _lib
    gr = _lib.CoeffNetBnGrads()
    for name, ftype in gr._fields_:
        if name in over:
            v = over[name]
            setattr(gr, name, ftype(*v) if isinstance(v, list) else v)
        elif hasattr(ftype, "_length_"):
            setattr(gr, name, ftype(*([P] * ftype._length_)))
        else:
            setattr(gr, name, P)
    return gr


def queries(lib, net, B):
    return (lib.hdrnet_coefficients_bn_workspace_bytes(ctypes.byref(net), B),
            lib.hdrnet_coefficients_bn_grad_workspace_bytes(ctypes.byref(net), B))


def test_binding_layout_matches_the_nested_c_struct():
    """The binding spells the `net` member out: the fields behind it start where a nested struct would put them."""
    from hdrnet_amd import _lib
    assert _lib.CoeffNetBn.splat_beta.offset == ctypes.sizeof(_lib.CoeffNet)
    assert _lib.CoeffNetBnGrads.splat_beta.offset == ctypes.sizeof(_lib.CoeffNetGrads)
    assert ctypes.sizeof(_lib.CoeffNetBn) == ctypes.sizeof(_lib.CoeffNet) + 8 * (3 * 8 + 3 * 2 + 3 * 2 + 3) + 8


@pytest.mark.parametrize("B", [0, 1, 9])
def test_batches_outside_2_to_8_have_no_workspace(lib, B):
    assert queries(lib, describe(), B) == (0, 0)


@pytest.mark.parametrize("over", [dict(n_levels=3, n_out=9), dict(fc_layout=0), dict(luma_bins=6), dict(net_input_size=100),
                                  dict(n_out=1, n_in=3)],
                         ids=["n_levels3", "fc_layout0", "luma_bins6", "N100", "pred24_not_x4"])
def test_shapes_outside_the_range_have_no_workspace(lib, over):
    """n_levels = 3, fc_layout = 0, shapes net_dims refuses, and a prediction layer the gradient kernels refuse."""
    if "n_in" in over:
        over = dict(over, luma_bins=2, channel_multiplier=2)  # gd * n_out * n_in = 6: no multiple of 4
    assert queries(lib, describe(**over), 2) == (0, 0)
    assert lib.hdrnet_coefficients_bn_workspace_bytes(None, 2) == 0
    assert lib.hdrnet_coefficients_bn_grad_workspace_bytes(None, 2) == 0


@pytest.mark.parametrize("B", [2, 8])
def test_default_network_has_workspaces(lib, B):
    from hdrnet_amd import _lib
    net = describe()
    fwd, bwd = queries(lib, net, B)
    base = _lib.load().hdrnet_coefficients_workspace_bytes(ctypes.byref(net), B)
    plain = _lib.load().hdrnet_coefficients_grad_workspace_bytes(ctypes.byref(net), B)
    # the raw outputs of the seven normalised convolutions alone: splat 1 .. 3, local1, both global convs
    raw = 4 * B * (64 * 64 * 16 + 32 * 32 * 32 + 16 * 16 * 64 + 16 * 16 * 64 + 8 * 8 * 64 + 4 * 4 * 64)
    assert fwd >= base + raw and fwd % 16 == 0
    assert bwd > plain and bwd % 16 == 0


def call_train(lib, net, B=2, coeffs=P, ws=P, nbytes=1 << 30):
    rc = lib.hdrnet_coefficients_bn_train_f32(P, ctypes.byref(net) if net is not None else None, coeffs, B, ws, nbytes, None)
    return rc, lib.hdrnet_last_error().decode()


def call_grad(lib, net, gr, B=2, ws=P, nbytes=1 << 30):
    rc = lib.hdrnet_coefficients_bn_grad_f32(P, ctypes.byref(net), P, P, ctypes.byref(gr) if gr is not None else None, B,
                                             ws, nbytes, None)
    return rc, lib.hdrnet_last_error().decode()


@pytest.mark.parametrize("over", [dict(local_beta=None), dict(fc_beta=[P, None]), dict(splat_beta=[None, P, None, P]),
                                  dict(fc_running_mean=[None, P]), dict(global_conv_running_mean=[P, None]),
                                  dict(local_running_var=None), dict(splat_running_var=[None, None, P, P]),
                                  dict(global_conv_beta=[None, P])],
                         ids=lambda o: next(iter(o)))
def test_null_statistics_are_refused_by_name(lib, over):
    net = describe(**over)
    rc, err = call_train(lib, net)
    assert rc == 1 and err.startswith(TRAIN + ": ") and "null beta, running_mean or running_var" in err, err
    rc, err = call_grad(lib, net, gradients())
    assert rc == 1 and err.startswith(GRAD + ": ") and "null beta, running_mean or running_var" in err, err


def test_unused_slots_may_be_null(lib):
    """Index 0 of the splat arrays and the biases of normalised layers are not read: NULL there reaches the next check."""
    net = describe(splat_beta=[None, P, P, P], splat_running_mean=[None, P, P, P], splat_running_var=[None, P, P, P],
                   splat_b=[P, None, None, None], global_conv_b=[None, None], fc_b=[None, None, P], local_b=[None, None])
    rc, err = call_train(lib, net, coeffs=None)
    assert rc == 1 and err == TRAIN + ": null buffer"


def test_short_and_misaligned_workspaces_are_refused(lib):
    net, gr = describe(), gradients()
    fwd, bwd = queries(lib, net, 2)
    for kw in (dict(nbytes=fwd - 1), dict(ws=None), dict(ws=P + 4)):
        rc, err = call_train(lib, net, **kw)
        assert rc == 1 and err.startswith(TRAIN + ": ") and f"= {fwd} bytes" in err, err
    for kw in (dict(nbytes=bwd - 1), dict(ws=None), dict(ws=P + 4)):
        rc, err = call_grad(lib, net, gr, **kw)
        assert rc == 1 and err.startswith(GRAD + ": ") and f"= {bwd} bytes" in err, err


def test_other_refusals_name_the_entry_point(lib):
    net, gr = describe(), gradients()
    for B in (0, 1, 9):
        rc, err = call_train(lib, net, B=B)
        assert rc == 1 and err.startswith(TRAIN + ": unsupported") and f"B={B}" in err
        rc, err = call_grad(lib, net, gr, B=B)
        assert rc == 1 and err.startswith(GRAD + ": unsupported") and f"B={B}" in err
    assert call_train(lib, None) == (1, TRAIN + ": null network description")
    assert call_grad(lib, net, None) == (1, GRAD + ": null network description")
    rc, err = call_grad(lib, net, gradients(local_beta=None))
    assert rc == 1 and err.startswith(GRAD + ": null gradient")
    # where nothing is written (index 0 of splat_beta, the bias gradients of normalised layers) NULL is no refusal
    rc, err = call_grad(lib, net, gradients(splat_beta=[None, P, P, P], splat_b=[P, None, None, None]), nbytes=16)
    assert rc == 1 and err.startswith(GRAD + ": needs a 16-B aligned workspace")
    rc, err = call_train(lib, describe(eps=0.0))
    assert rc == 1 and err.startswith(TRAIN + ": eps must be positive")
    rc, err = call_train(lib, describe(pred_b=None))
    assert rc == 1 and err.startswith(TRAIN + ": null parameter")


def test_symbols_in_header_library_and_binding(lib):
    from hdrnet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hdrnet_amd_coeff_bn.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", src), n
        assert hasattr(lib, n) and n in _lib.COEFF_BN_SIGNATURES
    assert "hdrnet_coeff_net_bn_grads" in src and "hdrnet_coeff_net net;" in src
    lib.hdrnet_version.restype = ctypes.c_int
    assert lib.hdrnet_version() >= 283
