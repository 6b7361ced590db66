"""The coefficient network (hdrnet_amd/models.py: _Coefficients; include/hdrnet_amd.h: hdrnet_coeff_net) evaluated from a
plain list of weight tensors with stock torch ops, for ANY hyper-parameters the C ABI accepts -- the model classes cannot
build spatial_bin < 4 (they size fc1 from sb // 4).  In float64 it is the reference of tests/test_coeff_net.py and
tests/test_gpu_coeff_net_edges.py, under autograd their gradient reference; in float32 it is the yardstick of what
float32 arithmetic costs on the same graph.

Weights, in this order (`weight_shapes`): splat (w, b) x n_ds, global conv (w, b) x 2, fc (w, b) x 3, local1 (w, b),
local2 w, prediction (w, b).  Convolutions are [Cout][kh][kw][Cin]; fc weights [in][out] (fc_layout 0) or [out][in] (1).
"""
import collections
import math

import torch
import torch.nn.functional as F

from hdrnet_amd import models

Shape = collections.namedtuple("Shape", "N sb gd cm n_out n_in n_levels", defaults=(1,))

# every ReLU of the network, in evaluation order (`relu_fractions`)
RELU_LOW, RELU_HIGH = 0.25, 0.75


def dims(s: Shape):
    """What csrc/coeff_net.hip.h: net_dims() derives: splat layers, the widths, the global path's sides (SAME padding,
    stride 2: ceil(n / 2) twice -- not sb // 4)."""
    n_ds = int(round(math.log2(s.N // s.sb)))
    assert s.sb << n_ds == s.N and n_ds >= 1
    base = s.cm * s.gd
    g1side = (s.sb + 1) // 2
    return dict(n_ds=n_ds, base=base, feat=base << (n_ds - 1), gl=8 * base, pred=s.gd * s.n_out * s.n_in,
                g1side=g1side, gside=(g1side + 1) // 2)


def weight_shapes(s: Shape, fc_layout: int = 0):
    """[(name, shape, fan_in or None for a bias)] in the order of the module docstring."""
    d = dims(s)
    gl, out = d["gl"], []

    def conv(name, cout, k, cin, bias=True):
        out.append((name + ".w", (cout, k, k, cin), k * k * cin))
        if bias:
            out.append((name + ".b", (cout,), None))

    def fc(name, cin, cout):
        out.append((name + ".w", (cin, cout) if fc_layout == 0 else (cout, cin), cin))
        out.append((name + ".b", (cout,), None))

    cin = 3
    for i in range(d["n_ds"]):
        conv(f"splat{i}", d["base"] << i, 3, cin)
        cin = d["base"] << i
    conv("global1", gl, 3, cin)
    conv("global2", gl, 3, gl)
    fc("fc1", d["gside"] ** 2 * gl, 4 * gl)
    fc("fc2", 4 * gl, 2 * gl)
    fc("fc3", 2 * gl, gl)
    conv("local1", gl, 3, cin)
    conv("local2", gl, 3, gl, bias=False)
    conv("pred", d["pred"], 1, gl)
    return out


def draw(s: Shape, batch: int, seed: int, fc_layout: int = 0):
    """A seeded draw of (weights, lowres), float32, without a model class: weights randn * sqrt(2 / fan_in), biases
    0.2 * randn, lowres rand in [0, 1)."""
    g = torch.Generator().manual_seed(seed)
    weights = []
    for _, shape, fan_in in weight_shapes(s, fc_layout):
        t = torch.randn(shape, generator=g)
        weights.append(t * math.sqrt(2.0 / fan_in) if fan_in else 0.2 * t)
    low = torch.rand((batch, s.N, s.N, 3), generator=g)
    return weights, low


def evaluate(weights, low, s: Shape, fc_layout: int = 0, relu_fractions=None):
    """lowres [B][N][N][3] -> [B][sb][sb][gd][n_out][n_in] (the reference's order, whatever n_levels) in the dtype of
    `low`.  `relu_fractions`: a dict that receives, per ReLU, the fraction of its outputs that are positive."""
    d = dims(s)
    it = iter(weights)

    def seen(name, y):
        if relu_fractions is not None:
            relu_fractions[name] = float((y.detach() > 0).double().mean())
        return y

    def conv(name, x, stride, relu, bias=True):
        wt = next(it)
        b = next(it) if bias else None
        x = models.tf_same_pad(x, wt.shape[1], stride)
        y = F.conv2d(x, wt.permute(0, 3, 1, 2), b, stride=stride)  # [Cout][kh][kw][Cin] -> OIHW
        return seen(name, F.relu(y)) if relu else y

    x = low.permute(0, 3, 1, 2)
    for i in range(d["n_ds"]):
        x = conv(f"splat{i}", x, 2, True)
    g = conv("global1", x, 2, True)
    g = conv("global2", g, 2, True)
    assert g.shape[2] == g.shape[3] == d["gside"]
    g = g.permute(0, 2, 3, 1).reshape(g.shape[0], -1)  # (h, w, c) flattening
    for i in range(3):
        wt, b = next(it), next(it)
        g = g @ (wt if fc_layout == 0 else wt.t()) + b
        if i < 2:
            g = seen(f"fc{i + 1}", F.relu(g))
    loc = conv("local1", x, 1, True)
    loc = conv("local2", loc, 1, False, bias=False)
    fusion = seen("fusion", F.relu(loc + g[:, :, None, None]))
    pred = conv("pred", fusion, 1, False)
    assert next(it, None) is None
    B, _, GH, GW = pred.shape
    pred = pred.reshape(B, s.n_in, s.n_out, s.gd, GH, GW)  # channel (j * n_out + i) * gd + z
    return pred.permute(0, 4, 5, 3, 2, 1).contiguous()


def assert_relus_alive(fractions, what=""):
    """The condition of every numerical test built on `draw`: no ReLU is dead or all-live in the float64 reference (either
    would hide mask and padding errors behind it)."""
    assert len(fractions) >= 7, fractions
    for name, f in fractions.items():
        assert RELU_LOW <= f <= RELU_HIGH, (what, name, f)


def module_weights(net):
    """The weight list of a batch-norm-free `_Coefficients` module (fc_layout 1: Linear weights as they are), attached to
    its parameters."""
    out = []
    for p in net._train_params():
        out.append(p.permute(0, 2, 3, 1) if p.dim() == 4 else p)
    return out


def module_shape(net) -> Shape:
    h = net.hyper
    return Shape(h["net_input_size"], h["spatial_bin"], h["luma_bins"], h["channel_multiplier"], net.n_out, net.n_in,
                 net.n_levels)
