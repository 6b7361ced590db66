"""Which tensor of the coefficient network lands in which field of the C structs (hdrnet_coeff_net, hdrnet_coeff_net_bn
and their gradient structs, include/hdrnet_amd.h, include/hdrnet_amd_coeff_bn.h), asked of the module BY NAME: the struct
fills of hdrnet_ops (_live_net, _live_net_bn, the autograd path of coefficients_train / coefficients_bn_train,
CoefficientWeights) take a flat list, and a slot swapped there is a gradient written to another tensor of the same size.

No library and no GPU: the fills only take addresses.  The autograd path runs on CPU tensors with a stand-in for the
library that records each call and computes nothing."""
import contextlib
import ctypes

import pytest
import torch

from hdrnet_amd import _lib, models
from hdrnet_amd import hdrnet_ops as ops

NETS = {"4_splat": (16, 256), "5_splat": (8, 256), "1_splat": (16, 32)}  # (spatial_bin, net_input_size)
BN_IDS = {False: "plain", True: "bn"}
both = pytest.mark.parametrize("bn", [False, True], ids=BN_IDS.get)
every_net = pytest.mark.parametrize("size", list(NETS))


def build(bn, size):
    """The module with every parameter and buffer random, so that no two tensors of one shape hold the same values."""
    sb, N = NETS[size]
    torch.manual_seed(5)
    net = models._Coefficients(models.default_params(batch_norm=bn, spatial_bin=sb, net_input_size=N), 3, 4)
    assert len(net.splat) == {"4_splat": 4, "5_splat": 5, "1_splat": 1}[size]
    with torch.no_grad():
        for name, t in list(net.named_parameters()) + list(net.named_buffers()):
            if t.is_floating_point():
                t.copy_(0.5 + torch.rand(t.shape) if name.endswith(("running_var", "bn.weight")) else torch.randn(t.shape))
    return net


def pointers(struct):
    """field -> address (list of addresses for an array field) of every pointer field of a ctypes struct, null as 0."""
    out = {}
    for name, ctype in struct._fields_:
        if ctype is ctypes.c_void_p:
            out[name] = getattr(struct, name) or 0
        elif issubclass(ctype, ctypes.Array):
            out[name] = [p or 0 for p in getattr(struct, name)]
    return out


def want(net, addr):
    """field -> what the field should hold, for every pointer field of the four structs: ``addr(tensor)`` of the module's
    tensor of that NAME, 0 where the network has no such tensor."""
    def a(t):
        return 0 if t is None else addr(t)

    def bn_of(layer, what):
        return 0 if layer.bn is None else a(getattr(layer.bn.bn, what))

    def pad(xs, n):
        return xs + [0] * (n - len(xs))

    s, g, fc = list(net.splat), list(net.global_conv), [net.fc1, net.fc2, net.fc3]
    out = {
        "splat_w": pad([a(m.conv.weight) for m in s], 8), "splat_b": pad([a(m.conv.bias) for m in s], 8),
        "global_conv_w": [a(m.conv.weight) for m in g], "global_conv_b": [a(m.conv.bias) for m in g],
        "fc_w": [a(m.fc.weight) for m in fc], "fc_b": [a(m.fc.bias) for m in fc],
        "local_w": [a(net.local1.conv.weight), a(net.local2.conv.weight)],
        "local_b": [a(net.local1.conv.bias), 0],
        "pred_w": a(net.pred.conv.weight), "pred_b": a(net.pred.conv.bias),
    }
    for field, what in (("beta", "bias"), ("running_mean", "running_mean"), ("running_var", "running_var")):
        out[f"splat_{field}"] = pad([bn_of(m, what) for m in s], 8)
        out[f"global_conv_{field}"] = [bn_of(m, what) for m in g]
        out[f"fc_{field}"] = [bn_of(net.fc1, what), bn_of(net.fc2, what)]
        out[f"local_{field}"] = bn_of(net.local1, what)
    return out


def assert_fields(struct, expected, what):
    got = pointers(struct)
    assert got and set(got) <= set(expected), what
    for field, value in got.items():
        assert value == expected[field], f"{what}: {field}"


def assert_scalars(desc, net, layout):
    h = net.hyper
    assert (desc.net_input_size, desc.spatial_bin, desc.luma_bins, desc.channel_multiplier) == \
        (h["net_input_size"], h["spatial_bin"], h["luma_bins"], h["channel_multiplier"])
    assert (desc.n_out, desc.n_in, desc.n_levels, desc.fc_layout) == (3, 4, 1, layout)


def parameter_list(net, bn):
    """(parameters, running statistics) as the module hands them to hdrnet_ops."""
    return net._train_params_bn() if bn else (net._train_params(), [])


def normalised_layers_present(net, bn, size):
    """With batch norm: splat 1 and up, both global convs, fc1, fc2, local1 -- and nothing else."""
    has = {name for name, m in net.named_modules() if isinstance(m, (models._Conv, models._FC)) and m.bn is not None}
    n = len(net.splat)
    assert has == (({f"splat.{i}" for i in range(1, n)} | {"global_conv.0", "global_conv.1", "fc1", "fc2", "local1"})
                   if bn else set()), size


@both
@every_net
def test_live_description_names_the_modules_tensors(size, bn):
    net = build(bn, size)
    normalised_layers_present(net, bn, size)
    ps, stats = parameter_list(net, bn)
    if bn:
        desc = ops._live_net_bn(net.hyper, net.n_out, net.n_in, ps, len(net.splat), stats, 1e-3, 2e-3)
        assert isinstance(desc, _lib.CoeffNetBn)
        assert desc.eps == ctypes.c_float(1e-3).value and desc.momentum == ctypes.c_float(2e-3).value
        # the examples of a silent swap: same-sized tensors side by side
        assert desc.fc_beta[1] == net.fc2.bn.bn.bias.data_ptr() and desc.fc_b[1] is None
        assert desc.local_running_var == net.local1.bn.bn.running_var.data_ptr()
        for i in range(1, len(net.splat)):
            assert desc.splat_beta[i] == net.splat[i].bn.bn.bias.data_ptr() and desc.splat_b[i] is None
    else:
        assert stats == []
        desc = ops._live_net(net.hyper, net.n_out, net.n_in, ps, len(net.splat))
        assert isinstance(desc, _lib.CoeffNet) and not isinstance(desc, _lib.CoeffNetBn)
    assert desc.fc_b[2] == net.fc3.fc.bias.data_ptr()
    assert desc.splat_b[0] == net.splat[0].conv.bias.data_ptr()
    for i, layer in enumerate(net.splat):
        assert desc.splat_w[i] == layer.conv.weight.data_ptr()
    assert_scalars(desc, net, layout=1)
    assert_fields(desc, want(net, lambda t: t.data_ptr()), f"{size} {BN_IDS[bn]}")
    # the description is as long as the list: every parameter in a field of its own, no field without a parameter
    named = [p for field, v in pointers(desc).items() if "running" not in field for p in (v if isinstance(v, list) else [v])
             if p]
    assert sorted(named) == sorted(p.data_ptr() for p in ps) and len(set(named)) == len(ps)
    assert len(stats) == (len(net.splat) + 4 if bn else 0)


@every_net
def test_one_parameter_list_for_both_networks(size):
    net = build(False, size)
    ps = net._train_params()
    also, stats = net._train_params_bn()
    assert stats == [] and len(ps) == len(also) and all(p is q for p, q in zip(ps, also))
    for bn in (False, True):
        net = build(bn, size)
        ps, stats = net._train_params_bn()
        slots = ops._coeff_slots(len(net.splat), bn)
        assert len(ps) == len(slots)
        assert len(stats) == sum(field == "beta" for _, _, field in slots) == len(net._bn_layers()) * bn


class RecordingLibrary:
    """Stands in for the loaded library: every entry point records its call; a workspace query answers 4096 bytes, every
    other entry point HDRNET_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 4096 if name.endswith("workspace_bytes") else 0
        return entry


@pytest.mark.parametrize("batch", [2, 9], ids=["narrow", "wide"])
@both
@every_net
def test_autograd_path_fills_both_structs_by_name(monkeypatch, size, bn, batch):
    """coefficients_train / coefficients_bn_train on CPU tensors over the recording library: the entry points and labels
    for this batch, the network description of both directions, the gradient struct -- one distinct tensor per parameter,
    handed out by _grad_out once per parameter in parameter order -- and where autograd puts what comes back."""
    net = build(bn, size)
    ps, stats = parameter_list(net, bn)
    lib, labels, handed = RecordingLibrary(), [], []

    def grad_out(p):
        handed.append((p.data_ptr(), torch.full_like(p, float(len(handed)))))
        return handed[-1][1]

    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(_lib, "check", lambda rc, what: labels.append((rc, what)))
    monkeypatch.setattr(ops, "_require_gpu", lambda name, t: None)
    monkeypatch.setattr(ops, "_stream", lambda device: 0)
    monkeypatch.setattr(ops, "_grad_out", grad_out)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())

    N, sb = net.hyper["net_input_size"], net.hyper["spatial_bin"]
    low = torch.zeros(batch, N, N, 3)
    versions = [t._version for st in stats for t in st]
    if bn:
        out = ops.coefficients_bn_train(low, net.hyper, net.n_out, net.n_in, ps, len(net.splat), stats, 1e-3, 2e-3)
    else:
        out = ops.coefficients_train(low, net.hyper, net.n_out, net.n_in, ps, len(net.splat))
    assert tuple(out.shape) == (batch, sb, sb, net.gd, 3, 4)
    assert ("CoefficientsBnTrain" in type(out.grad_fn).__name__) == bn and "CoefficientsTrain" in type(out.grad_fn).__name__.replace("Bn", "")
    assert [t._version for st in stats for t in st] == [v + 1 for v in versions]
    out.backward(torch.ones_like(out))

    w = "_wide" if batch > 8 else ""
    if bn:
        names = [f"hdrnet_coefficients_bn{w}_workspace_bytes", f"hdrnet_coefficients_bn_train{w}_f32",
                 f"hdrnet_coefficients_bn_grad{w}_workspace_bytes", f"hdrnet_coefficients_bn_grad{w}_f32"]
        assert labels == [(0, "CoefficientsBnTrain"), (0, "CoefficientsBnGrad")]
    else:
        names = ["hdrnet_coefficients_workspace_bytes", "hdrnet_coefficients_f32",
                 f"hdrnet_coefficients_grad{w}_workspace_bytes", f"hdrnet_coefficients_grad{w}_f32"]
        assert labels == [(0, "Coefficients"), (0, "CoefficientsGrad")]
    assert [name for name, _ in lib.calls] == names
    (_, fq), (_, fwd), (_, bq), (_, bwd) = lib.calls
    tag = f"{size} {BN_IDS[bn]} batch {batch}"
    here = want(net, lambda t: t.data_ptr())
    for args, where in ((fq, 0), (fwd, 1), (bq, 0), (bwd, 1)):
        desc = args[where]._obj
        assert isinstance(desc, _lib.CoeffNetBn if bn else _lib.CoeffNet) and isinstance(desc, _lib.CoeffNetBn) == bn
        assert_scalars(desc, net, layout=1)
        assert_fields(desc, here, tag)
        if bn:
            assert desc.eps == ctypes.c_float(1e-3).value and desc.momentum == ctypes.c_float(2e-3).value
    assert fq[1] == bq[1] == fwd[3] == bwd[5] == batch
    assert fwd[0] == bwd[0] == low.data_ptr() and fwd[2] == out.data_ptr()
    assert fwd[5] == bwd[7] == 4096 and bwd[2] == fwd[4] and bwd[6] != fwd[4]  # the forward's workspace, kept, and a second one

    assert [p for p, _ in handed] == [p.data_ptr() for p in ps]
    grad_of = {p: g.data_ptr() for p, g in handed}
    gr = bwd[4]._obj
    assert isinstance(gr, _lib.CoeffNetBnGrads if bn else _lib.CoeffNetGrads) and isinstance(gr, _lib.CoeffNetBnGrads) == bn
    assert_fields(gr, want(net, lambda t: grad_of.get(t.data_ptr(), 0)), tag + " gradients")
    if bn:
        assert gr.fc_beta[1] == grad_of[net.fc2.bn.bn.bias.data_ptr()] and gr.fc_b[1] is None
        assert gr.global_conv_beta[0] == grad_of[net.global_conv[0].bn.bn.bias.data_ptr()] and gr.global_conv_b[0] is None
    assert gr.local_b[1] is None and gr.fc_b[2] == grad_of[net.fc3.fc.bias.data_ptr()]
    for k, p in enumerate(ps):  # and autograd hands gradient k to parameter k
        assert p.grad is not None and bool((p.grad == float(k)).all()), k


@both
@every_net
def test_exported_weights_name_the_folded_tensors(size, bn):
    net = build(bn, size).eval()
    w = net.exported()
    desc = w.net
    assert isinstance(desc, _lib.CoeffNet) and w.n_splat == len(net.splat)
    assert_scalars(desc, net, layout=0)
    kept = {t.data_ptr(): t for t in w._keep}
    assert len(kept) == len(w._keep) == 2 * (len(net.splat) + 2 + 3 + 2 + 1) - 1
    for t in w._keep:
        assert t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad
    used = []

    def same(address, tensor, what):
        used.append(address)
        assert address in kept and torch.equal(kept[address], tensor), f"{size} {BN_IDS[bn]}: {what}"

    with torch.no_grad():
        groups = (("splat", list(net.splat), 8), ("global_conv", list(net.global_conv), 2),
                  ("fc", [net.fc1, net.fc2, net.fc3], 3), ("local", [net.local1, net.local2], 2), ("pred", [net.pred], 1))
        for group, layers, room in groups:
            for i, layer in enumerate(layers):
                lin = layer.fc if isinstance(layer, models._FC) else layer.conv
                wt, b = net._fold(lin.weight, lin.bias, layer.bn)
                wt = wt.t() if isinstance(layer, models._FC) else wt.permute(0, 2, 3, 1)
                fw, fb = getattr(desc, f"{group}_w"), getattr(desc, f"{group}_b")
                same(fw if group == "pred" else fw[i], wt, f"{group}_w[{i}]")
                if layer is net.local2:
                    assert b is None and fb[1] is None
                else:
                    same(fb if group == "pred" else fb[i], b, f"{group}_b[{i}]")
            for i in range(len(layers), room):
                assert getattr(desc, f"{group}_w")[i] is None and getattr(desc, f"{group}_b")[i] is None
    assert sorted(used) == sorted(kept)
