"""CPU tests around the coefficient network's edges (no GPU call):

* tests/coeff_reference.py -- the float64 reference the GPU tests of tests/test_gpu_coeff_net_edges.py are judged by --
  against the model classes themselves, values and gradients;
* the limits csrc/coeff_net.hip.h: net_dims() and csrc/coeff_net_train.hip: train_supported() enforce: a refused
  configuration reports 0 workspace bytes, its entry point returns 1 and names the limit; the accepted configuration next
  to each limit still reports the workspace of the layout in csrc/coeff_net.hip.h.
"""
import copy
import ctypes

import pytest
import torch

import coeff_reference as cr
from hdrnet_amd import _lib, models
from test_coeff_net import randomize


@pytest.mark.parametrize("cls", [models.HDRNetCurves, models.HDRNetPointwiseNNGuide, models.HDRNetGaussianPyrNN])
def test_reference_reproduces_the_module_and_its_gradients(cls):
    """At the classes' default sizes (256 -> 16 x 16 x 8; the pyramid model: 9 x 4 coefficients) the helper IS the module:
    the float64 values and the float64 autograd gradient of every parameter."""
    torch.manual_seed(5)
    net = randomize(cls(dict(batch_norm=False)), seed=3).coefficients
    shape = cr.module_shape(net)._replace(n_levels=1)  # the module's own output order is the reference's
    low = torch.rand(1, shape.N, shape.N, 3, dtype=torch.float64)
    a, b = copy.deepcopy(net).double(), copy.deepcopy(net).double()
    want = a(low)
    fractions = {}
    got = cr.evaluate(cr.module_weights(b), low, shape, fc_layout=1, relu_fractions=fractions)
    cr.assert_relus_alive(fractions, cls.__name__)
    assert got.shape == want.shape == (1, shape.sb, shape.sb, shape.gd, shape.n_out, shape.n_in)
    scale = float(want.detach().abs().max())
    assert float((got - want).detach().abs().max()) <= 1e-12 * scale
    up = torch.randn(want.shape, dtype=torch.float64)
    (want * up).sum().backward()
    (got * up).sum().backward()
    for (name, p), q in zip(a.named_parameters(), b.parameters()):
        gs = float(p.grad.abs().max())
        assert gs > 0 and float((p.grad - q.grad).abs().max()) <= 1e-11 * gs, name


def test_reference_dims_follow_net_dims():
    assert cr.dims(cr.Shape(256, 1, 4, 1, 3, 4)) == dict(n_ds=8, base=4, feat=512, gl=32, pred=48, g1side=1, gside=1)
    assert cr.dims(cr.Shape(4, 2, 8, 1, 3, 4))["gside"] == 1  # ceil(ceil(2 / 2) / 2), where sb // 4 is 0
    assert cr.dims(cr.Shape(128, 64, 8, 1, 3, 4))["gside"] == 16
    names = [n for n, _, _ in cr.weight_shapes(cr.Shape(16, 4, 2, 2, 3, 4))]
    assert names == ["splat0.w", "splat0.b", "splat1.w", "splat1.b", "global1.w", "global1.b", "global2.w", "global2.b",
                     "fc1.w", "fc1.b", "fc2.w", "fc2.b", "fc3.w", "fc3.b", "local1.w", "local1.b", "local2.w",
                     "pred.w", "pred.b"]


# --------------------------------------------------------------------------------------------------- the limits

def net_of(N, sb, gd, cm, n_out=3, n_in=4, n_levels=1, fc_layout=1):
    net = _lib.CoeffNet()
    net.net_input_size, net.spatial_bin, net.luma_bins, net.channel_multiplier = N, sb, gd, cm
    net.n_out, net.n_in, net.n_levels, net.fc_layout = n_out, n_in, n_levels, fc_layout
    return net


def layout_floats(N, sb, gd, cm):
    """Floats per image of the forward workspace, from the layout of csrc/coeff_net.hip.h (NetWorkspace): every splat
    layer's output, local1, local2, the two global convs, fc1's and fc2's K-split partial sums (16 inputs a chunk)."""
    r4 = lambda n: (n + 3) // 4 * 4
    base, gl = cm * gd, 8 * cm * gd
    total, side, i = 0, N, 0
    while side > sb:
        side //= 2
        total += r4(side * side * (base << i))
        i += 1
    g1 = (sb + 1) // 2
    g2 = (g1 + 1) // 2
    total += 2 * r4(sb * sb * gl) + r4(g1 * g1 * gl) + r4(g2 * g2 * gl)
    s1, s2 = (g2 * g2 * gl + 15) // 16, (4 * gl + 15) // 16
    return total + r4(s1 * 4 * gl) + r4(s2 * 2 * gl)


def forward_call(lib, net):
    rc = lib.hdrnet_coefficients_f32(None, ctypes.byref(net), None, 1, None, 0, None)
    return rc, lib.hdrnet_last_error().decode()


def grad_call(lib, net, B=1):
    grads = _lib.CoeffNetGrads()
    rc = lib.hdrnet_coefficients_grad_f32(None, ctypes.byref(net), None, None, ctypes.byref(grads), B, None, 0, None)
    return rc, lib.hdrnet_last_error().decode()


def test_layout_floats_is_the_documented_layout():
    # the sum spelled out in tests/test_coeff_net.py: test_workspace_and_validation_without_gpu
    assert layout_floats(256, 16, 8, 1) == 131072 + 65536 + 32768 + 16384 + 2 * 16384 + 4096 + 1024 + 16384 + 2048


def test_forward_refuses_products_beyond_an_int_and_a_launch_grid():
    lib = _lib.load()
    # cm * gd = 2^21 (8 * cm * gd and the layer widths derived from it would leave an int)
    net = net_of(4096, 2048, 1 << 11, 1 << 10)
    assert lib.hdrnet_coefficients_workspace_bytes(ctypes.byref(net), 1) == 0
    rc, err = forward_call(lib, net)
    assert rc == 1 and "8 * cm * gd exceeds 1024" in err, err
    # gd * n_out * n_in = 16 * 65535 + 16: one 16-channel group more than a launch grid's y extent holds
    net = net_of(8, 4, 4, 1, n_out=65536, n_in=4)
    assert lib.hdrnet_coefficients_workspace_bytes(ctypes.byref(net), 1) == 0
    rc, err = forward_call(lib, net)
    assert rc == 1 and "gd * n_out * n_in exceeds 1048560" in err, err
    # next to it: 4 * 65535 * 4 = 16 * 65535 channels (the workspace does not depend on them)
    ok = net_of(8, 4, 4, 1, n_out=65535, n_in=4)
    assert lib.hdrnet_coefficients_workspace_bytes(ctypes.byref(ok), 1) == 4 * layout_floats(8, 4, 4, 1)
    rc, err = forward_call(lib, ok)
    assert rc == 1 and "null parameter" in err, err


FORWARD_LIMITS = {
    # the step table's 16-bit filter offset: the last splat layer is 8192 channels wide (gd = 16, cm = 4, N / sb = 256)
    "feat": ((256, 1, 16, 4), (256, 1, 8, 4), "exceed 4096"),
    # the prediction layer's LDS: 8 * cm * gd = 2048
    "gl": ((2, 1, 64, 4), (2, 1, 32, 4), "8 * cm * gd exceeds 1024"),
}


@pytest.mark.parametrize("which", sorted(FORWARD_LIMITS))
def test_forward_refuses_beyond_its_limits(which):
    lib = _lib.load()
    refused, accepted, text = FORWARD_LIMITS[which]
    net = net_of(*refused)
    assert lib.hdrnet_coefficients_workspace_bytes(ctypes.byref(net), 1) == 0
    assert lib.hdrnet_coefficients_grad_workspace_bytes(ctypes.byref(net), 1) == 0
    rc, err = forward_call(lib, net)
    assert rc == 1 and text in err and "net_input_size=%d" % refused[0] in err, err
    assert grad_call(lib, net)[0] == 1
    ok = net_of(*accepted)
    for B in (1, 3):
        assert lib.hdrnet_coefficients_workspace_bytes(ctypes.byref(ok), B) == 4 * B * layout_floats(*accepted)
    rc, err = forward_call(lib, ok)
    assert rc == 1 and "null parameter" in err, err  # past the hyper-parameter checks


def test_forward_accepts_the_widths_next_to_the_limits():
    lib = _lib.load()
    for cfg, what in (((256, 1, 8, 4), dict(feat=4096)), ((2, 1, 16, 4), dict(gl=512)), ((2, 1, 32, 4), dict(gl=1024))):
        d = cr.dims(cr.Shape(*cfg, 3, 4))
        assert all(d[k] == v for k, v in what.items()), (cfg, d)
        net = net_of(*cfg)
        assert lib.hdrnet_coefficients_workspace_bytes(ctypes.byref(net), 2) == 8 * layout_floats(*cfg)


def test_gradient_refuses_prediction_widths_it_cannot_read():
    lib = _lib.load()
    # gd * n_out * n_in = 9: the backward-data kernel's four-channel loads would straddle pixels.  The forward stores per
    # element and keeps the configuration.
    net = net_of(8, 4, 1, 4, n_out=3, n_in=3)
    assert lib.hdrnet_coefficients_workspace_bytes(ctypes.byref(net), 2) == 8 * layout_floats(8, 4, 1, 4)
    assert lib.hdrnet_coefficients_grad_workspace_bytes(ctypes.byref(net), 2) == 0
    rc, err = grad_call(lib, net, 2)
    assert rc == 1 and "multiple of 4" in err and "n_out=3, n_in=3" in err, err
    # 12 channels next to it
    ok = net_of(8, 4, 1, 4, n_out=3, n_in=4)
    assert lib.hdrnet_coefficients_workspace_bytes(ctypes.byref(ok), 2) == 8 * layout_floats(8, 4, 1, 4)
    assert lib.hdrnet_coefficients_grad_workspace_bytes(ctypes.byref(ok), 2) > 0
    rc, err = grad_call(lib, ok, 2)
    assert rc == 1 and "null parameter" in err, err
    # the other, older reasons keep their text (tests/golden/capi_errors.json)
    rc, err = grad_call(lib, ok, 9)
    assert rc == 1 and "1 <= B <= 8" in err, err


def test_gradient_refuses_what_its_magic_divisions_cannot_divide():
    """coeff_recompute divides by gd * n_out * n_in with a magic number that is exact below 2^16."""
    lib = _lib.load()
    net = net_of(8, 4, 8, 1, n_out=128, n_in=64)  # 65536 channels
    assert lib.hdrnet_coefficients_workspace_bytes(ctypes.byref(net), 1) > 0
    assert lib.hdrnet_coefficients_grad_workspace_bytes(ctypes.byref(net), 1) == 0
    rc, err = grad_call(lib, net)
    assert rc == 1 and "below 65536" in err, err
    ok = net_of(8, 4, 8, 1, n_out=128, n_in=63)  # 64512
    assert lib.hdrnet_coefficients_grad_workspace_bytes(ctypes.byref(ok), 1) > 0
    # the case that doubles the slabs (tests/test_gpu_coeff_net_edges.py: slab_doubling) is inside the range
    assert lib.hdrnet_coefficients_grad_workspace_bytes(ctypes.byref(net_of(64, 32, 8, 1, n_out=16, n_in=16)), 1) > 0
