"""The coefficient network's kernels (csrc/coeff_net.hip, csrc/coeff_net_train.hip) at the edges of the range the C ABI
accepts -- 1 x 1 and 2 x 2 grids, one and eight splat layers, prediction layers narrower than a channel group, the widest
global path, n_in != 4, batches beyond the workload's -- where the model classes cannot go (they size fc1 from sb // 4) and
tests/test_coeff_net.py therefore never went.  Weights are drawn directly (tests/coeff_reference.py); the reference is
that module's float64 evaluation, the yardstick its float32 evaluation on the CPU.

A case is (N, sb, gd, cm, n_out, n_in[, n_levels]) and a batch size.  Every numerical test first asserts that no ReLU of
the float64 reference is dead or all-live (25 % .. 75 % positive outputs).
"""
import ctypes
import functools

import pytest
import torch

import coeff_reference as cr
from coeff_reference import Shape

SEED = 2024
DEV = "cuda:0"

FORWARD_CASES = {
    # 8 splat layers, a 1 x 1 grid: every tail layer is smaller than a 4 x 4 tile, the global convs read a 1 x 1 input
    "deep_1x1": (Shape(256, 1, 4, 1, 3, 4), 2),
    # coeff_conv_first only; 2 x 2 grid; the global conv 2 x 2 -> 1 x 1 pads 0 before and 1 after
    "one_splat_2x2": (Shape(4, 2, 8, 1, 3, 4), 3),
    "pred24": (Shape(16, 4, 2, 2, 3, 4), 2),         # prediction Cout = 24: one and a half channel groups
    "pred12": (Shape(8, 4, 1, 4, 3, 4), 2),          # prediction Cout = 12 < 16, gd = 1
    "grid64": (Shape(128, 64, 8, 1, 3, 4), 1),       # 256 tiles per layer, fc1 with K = 16384
    "gl256": (Shape(32, 8, 16, 2, 3, 4), 2),         # fc3's input 512 > 256 wide, fc3 on its slow path
    "gl512": (Shape(2, 1, 16, 4, 3, 4), 2),          # fc3's input fills the 1024 floats of the partial tiles exactly
    "wide1024": (Shape(2, 1, 32, 4, 3, 4), 2),       # fc3's input (2048) is what sizes the prediction layer's LDS
    "square_affine": (Shape(16, 4, 4, 1, 3, 3), 2),  # n_in != 4 in the unroll
    "levels3_small": (Shape(8, 4, 4, 1, 9, 4, 3), 3),  # the level-major store away from the pyramid model's size
    "batch33": (Shape(8, 4, 4, 1, 3, 4), 33),        # grid z beyond anything else in the suite
}
GUARDED_FORWARD = ["deep_1x1", "pred12", "grid64", "levels3_small"]

TRAIN_CASES = {
    "deep_1x1": FORWARD_CASES["deep_1x1"],
    "one_splat_2x2": FORWARD_CASES["one_splat_2x2"],
    "pred24": FORWARD_CASES["pred24"],
    "grid64": FORWARD_CASES["grid64"],
    "gl256": FORWARD_CASES["gl256"],               # the training bound: coeff_recompute's x2s[512] is exactly full
    "pred12": (Shape(8, 4, 1, 4, 3, 4), 8),          # the largest batch coeff_fc_bwd<8> holds
    "square_affine": FORWARD_CASES["square_affine"],
    "slab_doubling": (Shape(64, 32, 8, 1, 16, 16), 1),  # coeff_recompute needs more than its 32 slabs per image
    "batch7": (Shape(16, 4, 4, 1, 3, 4), 7),
}
GUARDED_TRAIN = ["deep_1x1", "grid64"]

GUARD = 4096
PATTERN = 0xA5


def hyper_of(s):
    return dict(net_input_size=s.N, spatial_bin=s.sb, luma_bins=s.gd, channel_multiplier=s.cm)


# ------------------------------------------------------------------------------------------------------- forward

@functools.lru_cache(maxsize=None)
def forward_reference(case):
    """(weights, lowres) of the case and the reference's float64 and float32 evaluations; computed once, never modified."""
    s, B = FORWARD_CASES[case]
    weights, low = cr.draw(s, B, SEED)
    fractions = {}
    with torch.no_grad():
        ref64 = cr.evaluate([w.double() for w in weights], low.double(), s, relu_fractions=fractions)
        ref32 = cr.evaluate(weights, low, s)
    return weights, low, ref64, ref32, fractions


def device_weights(case, layout):
    from hdrnet_amd import hdrnet_ops as ops
    s, B = FORWARD_CASES[case]
    weights = forward_reference(case)[0]
    t = dict(zip([n for n, _, _ in cr.weight_shapes(s)], weights))

    def pair(name, bias=True):
        w = t[name + ".w"]
        if name.startswith("fc") and layout == 1:
            w = w.t().contiguous()  # [out][in]
        return w.to(DEV), (t[name + ".b"].to(DEV) if bias else None)

    n_ds = cr.dims(s)["n_ds"]
    w = ops.CoefficientWeights(hyper_of(s), s.n_out, s.n_in, s.n_levels, splat=[pair(f"splat{i}") for i in range(n_ds)],
                               global_conv=[pair("global1"), pair("global2")], fc=[pair("fc1"), pair("fc2"), pair("fc3")],
                               local=[pair("local1"), pair("local2", bias=False)], pred=pair("pred"))
    w.net.fc_layout = layout
    assert w.supported(B), case
    return w


def reference_order(out, s):
    """The level-major output of n_levels > 1 back in the reference's [B, sb, sb, gd, n_out, n_in]."""
    if s.n_levels == 1:
        return out
    L, B, GH, GW, gd, k, n_in = out.shape
    return out.permute(1, 2, 3, 4, 0, 5, 6).reshape(B, GH, GW, gd, L * k, n_in)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(FORWARD_CASES))
def test_forward_vs_float64(case):
    """The rule of tests/test_coeff_net.py: test_native_coefficients_vs_float64, with the reference's own float32
    evaluation on the CPU as the yardstick (no stock GPU module exists for sb < 4); fc_layout 1 gives the same bits."""
    from hdrnet_amd import hdrnet_ops as ops
    s, B = FORWARD_CASES[case]
    weights, low, ref64, ref32, fractions = forward_reference(case)
    cr.assert_relus_alive(fractions, case)
    lowd = low.to(DEV)
    got = ops.coefficients(lowd, device_weights(case, 0)).cpu()
    got1 = ops.coefficients(lowd, device_weights(case, 1)).cpu()
    assert torch.equal(got, got1), "fc_layout 1 differs from fc_layout 0"
    got = reference_order(got, s)
    assert got.shape == ref64.shape == (B, s.sb, s.sb, s.gd, s.n_out, s.n_in)
    scale = float(ref64.abs().max())
    err = float((got.double() - ref64).abs().max())
    err32 = float((ref32.double() - ref64).abs().max())
    print(f"{case}: |coeffs| <= {scale:.3g}; native {err:.3g}, float32 CPU {err32:.3g} from float64 "
          f"(ReLUs {min(fractions.values()):.2f} .. {max(fractions.values()):.2f} positive)")
    assert err <= 2e-6 * scale + 2.0 * err32, (err, err32, scale)
    assert err <= 1e-5 * scale, (err, err32, scale)


def guarded(nbytes, fill_nan=False):
    """A device buffer of `nbytes` between two guards of a bit pattern: (whole uint8 tensor, the inner region)."""
    whole = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    inner = whole[GUARD:GUARD + nbytes]
    if fill_nan:
        inner.view(torch.float32).fill_(float("nan"))
    return whole, inner


def assert_guards(whole, nbytes, what):
    assert bool((whole[:GUARD] == PATTERN).all()), f"{what}: written before the buffer"
    assert bool((whole[GUARD + nbytes:] == PATTERN).all()), f"{what}: written behind the buffer"


@pytest.mark.gpu
@pytest.mark.parametrize("case", GUARDED_FORWARD)
def test_forward_stays_inside_its_workspace_and_writes_every_output(case):
    from hdrnet_amd import _lib
    lib = _lib.load()
    s, B = FORWARD_CASES[case]
    low, ref64 = forward_reference(case)[1], forward_reference(case)[2]
    w = device_weights(case, 0)
    wbytes = lib.hdrnet_coefficients_workspace_bytes(ctypes.byref(w.net), B)
    assert wbytes > 0 and wbytes % 16 == 0
    obytes = 4 * ref64.numel()
    ws_all, ws = guarded(wbytes)
    out_all, out = guarded(obytes, fill_nan=True)
    lowd = low.to(DEV)
    rc = lib.hdrnet_coefficients_f32(lowd.data_ptr(), ctypes.byref(w.net), out.data_ptr(), B, ws.data_ptr(), wbytes, None)
    torch.cuda.synchronize()
    _lib.check(rc, "Coefficients")
    assert_guards(ws_all, wbytes, "workspace")
    assert_guards(out_all, obytes, "output")
    res = out.view(torch.float32)
    assert not bool(torch.isnan(res).any()), "an output element was not written"
    L = s.n_levels
    shape = (B, s.sb, s.sb, s.gd, s.n_out // L, s.n_in)
    res = reference_order(res.reshape((L,) + shape if L > 1 else shape).cpu(), s)
    assert float((res.double() - ref64).abs().max()) <= 1e-5 * float(ref64.abs().max())


# ------------------------------------------------------------------------------------------------------ backward

def upstreams(s, B):
    """The two gradients every case is run with: dense, and zero except the four corner cells (all channels), so that the
    border handling of the backward-data kernels is not averaged away."""
    g = torch.Generator().manual_seed(SEED + 1)
    dense = torch.randn((B, s.sb, s.sb, s.gd, s.n_out, s.n_in), generator=g)
    corners = torch.zeros_like(dense)
    for y in (0, s.sb - 1):
        for x in (0, s.sb - 1):
            corners[:, y, x] = dense[:, y, x]
    return dict(dense=dense, corners=corners)


@functools.lru_cache(maxsize=None)
def train_reference(case):
    """Weights in torch's layouts (fc [out][in]), lowres, and per dtype the output and the parameter gradients of both
    upstream gradients, by CPU autograd over tests/coeff_reference.py."""
    s, B = TRAIN_CASES[case]
    weights, low = cr.draw(s, B, SEED, fc_layout=1)
    ups = upstreams(s, B)
    res = {}
    for dtype in (torch.float64, torch.float32):
        leaves = [w.to(dtype).requires_grad_() for w in weights]
        fractions = {}
        out = cr.evaluate(leaves, low.to(dtype), s, fc_layout=1, relu_fractions=fractions)
        grads = {kind: torch.autograd.grad(out, leaves, up.to(dtype), retain_graph=True) for kind, up in ups.items()}
        res[dtype] = (out.detach(), grads, fractions)
    return weights, low, ups, res


def torch_params(weights):
    """The parameters as a torch module holds them, on the GPU: Conv2d weights [Cout, Cin, k, k] in channels_last memory
    order (= the reference's [Cout][kh][kw][Cin]), Linear weights [out][in]."""
    return [(w.to(DEV).permute(0, 3, 1, 2) if w.dim() == 4 else w.to(DEV)).requires_grad_() for w in weights]


def check_gradients(case, kind, names, native, res):
    """`native`: gradients in the reference's layouts, on the CPU.  e <= 2e-5 + 2 e32 relative to max|g64| per parameter;
    a parameter whose float64 gradient is identically zero must come out exactly zero."""
    g64s, g32s = res[torch.float64][1][kind], res[torch.float32][1][kind]
    worst = (0.0, 0.0, "")
    for name, g, g64, g32 in zip(names, native, g64s, g32s):
        assert g.shape == g64.shape, name
        top = float(g64.abs().max())
        if top == 0.0:
            assert kind == "corners" and not bool(g.any()), (name, "expected an exactly zero gradient")
            continue
        e = float((g.double() - g64).abs().max()) / top
        e32 = float((g32.double() - g64).abs().max()) / top
        worst = max(worst, (e, e32, name))
        assert e <= 2e-5 + 2.0 * e32, (case, kind, name, e, e32)
    print(f"{case} / {kind}: worst relative gradient error: native {worst[0]:.2e}, float32 CPU {worst[1]:.2e} ({worst[2]})")


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(TRAIN_CASES))
def test_gradients_vs_float64(case):
    from hdrnet_amd import hdrnet_ops as ops
    s, B = TRAIN_CASES[case]
    if case == "slab_doubling":  # the case must keep reaching the branch: 32 slabs would hold 2^16 elements each
        assert -(-(s.sb * s.sb) // 32) * (s.gd * s.n_out * s.n_in) >= 65536
        assert -(-1024 // 32) * 2048 >= 65536
    weights, low, ups, res = train_reference(case)
    out64, _, fractions = res[torch.float64]
    cr.assert_relus_alive(fractions, case)
    names = [n for n, _, _ in cr.weight_shapes(s)]
    params = torch_params(weights)
    n_ds = cr.dims(s)["n_ds"]
    assert ops.coefficients_train_supported(hyper_of(s), s.n_out, s.n_in, params, n_ds, B)
    out = ops.coefficients_train(low.to(DEV), hyper_of(s), s.n_out, s.n_in, params, n_ds)
    assert out.grad_fn is not None and "CoefficientsTrain" in type(out.grad_fn).__name__
    scale = float(out64.abs().max())
    err = float((out.detach().cpu().double() - out64).abs().max())
    err32 = float((res[torch.float32][0].double() - out64).abs().max())
    print(f"{case}: |coeffs| <= {scale:.3g}; native {err:.3g}, float32 CPU {err32:.3g} from float64")
    assert err <= 1e-5 * scale, (err, err32, scale)
    for kind, up in ups.items():
        grads = torch.autograd.grad(out, params, up.to(DEV), retain_graph=True)
        for p, g in zip(params, grads):
            assert g.stride() == p.stride()
        native = [(g.permute(0, 2, 3, 1) if g.dim() == 4 else g).cpu() for g in grads]
        check_gradients(case, kind, names, native, res)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GUARDED_TRAIN)
def test_backward_is_deterministic_and_stays_inside_its_buffers(case):
    """Through the C ABI: the backward workspace and every gradient tensor (views into ONE flat buffer) lie between guards
    that stay untouched, every gradient element is written, the forward workspace is only read, and two calls give the
    same bits."""
    from hdrnet_amd import _lib, hdrnet_ops as ops
    lib = _lib.load()
    s, B = TRAIN_CASES[case]
    weights, low, ups, res = train_reference(case)
    cr.assert_relus_alive(res[torch.float64][2], case)
    names = [n for n, _, _ in cr.weight_shapes(s)]
    params = [w.to(DEV) for w in weights]  # the reference's layouts ARE the memory orders the entry points read
    n_ds = cr.dims(s)["n_ds"]
    net = ops._live_net(hyper_of(s), s.n_out, s.n_in, params, n_ds)
    lowd, up = low.to(DEV), ups["dense"].to(DEV)
    fbytes = lib.hdrnet_coefficients_workspace_bytes(ctypes.byref(net), B)
    bbytes = lib.hdrnet_coefficients_grad_workspace_bytes(ctypes.byref(net), B)
    assert fbytes > 0 and bbytes > 0 and bbytes % 16 == 0
    fws = torch.empty((fbytes,), dtype=torch.uint8, device=DEV)
    out = torch.empty(up.shape, dtype=torch.float32, device=DEV)
    _lib.check(lib.hdrnet_coefficients_f32(lowd.data_ptr(), ctypes.byref(net), out.data_ptr(), B, fws.data_ptr(), fbytes,
                                           None), "Coefficients")
    torch.cuda.synchronize()
    fws_before = fws.clone()
    # one flat buffer: guard, gradient, guard, gradient, ..., guard (segments padded to 16 bytes with guard bytes)
    offsets, off = [], GUARD
    for w in weights:
        offsets.append(off)
        off += (4 * w.numel() + 15) // 16 * 16 + GUARD
    flat = torch.full((off,), PATTERN, dtype=torch.uint8, device=DEV)
    keep = torch.ones((off,), dtype=torch.bool, device=DEV)  # True: a guard byte
    views = []
    for w, o in zip(weights, offsets):
        keep[o:o + 4 * w.numel()] = False
        views.append(flat[o:o + 4 * w.numel()].view(torch.float32).view(w.shape))
    gr = _lib.CoeffNetGrads()
    it = iter(views)
    for i in range(n_ds):
        gr.splat_w[i], gr.splat_b[i] = next(it).data_ptr(), next(it).data_ptr()
    for i in range(2):
        gr.global_conv_w[i], gr.global_conv_b[i] = next(it).data_ptr(), next(it).data_ptr()
    for i in range(3):
        gr.fc_w[i], gr.fc_b[i] = next(it).data_ptr(), next(it).data_ptr()
    gr.local_w[0], gr.local_b[0] = next(it).data_ptr(), next(it).data_ptr()
    gr.local_w[1] = next(it).data_ptr()
    gr.pred_w, gr.pred_b = next(it).data_ptr(), next(it).data_ptr()
    runs = []
    for _ in range(2):
        for v in views:
            v.fill_(float("nan"))
        bws_all, bws = guarded(bbytes)
        rc = lib.hdrnet_coefficients_grad_f32(lowd.data_ptr(), ctypes.byref(net), fws.data_ptr(), up.data_ptr(),
                                              ctypes.byref(gr), B, bws.data_ptr(), bbytes, None)
        torch.cuda.synchronize()
        _lib.check(rc, "CoefficientsGrad")
        assert_guards(bws_all, bbytes, "backward workspace")
        assert bool((flat[keep] == PATTERN).all()), "written outside a gradient tensor"
        for name, v in zip(names, views):
            assert not bool(torch.isnan(v).any()), f"{name}: a gradient element was not written"
        assert torch.equal(fws, fws_before), "the backward wrote into the forward's workspace"
        runs.append([v.cpu() for v in views])
    for name, a, b in zip(names, *runs):
        assert torch.equal(a, b), f"{name}: two backward calls differ"
    check_gradients(case, "dense", names, runs[0], res)
