"""The coefficient network trained on the HIP kernels at batches of 9 to 32 images (csrc/coeff_fc_train.hip behind the
``..._wide`` entry points of include/hdrnet_amd_coeff_wide.h; hdrnet_ops.coefficients_train / coefficients_bn_train), with
and without batch norm, against the same module in float64 on the CPU: forward, every gradient, the running statistics;
determinism and buffer bounds through the C ABI; the wide entry points against the first ones where both run; a captured
training step of the whole model; and the cases that must keep running the torch ops.

The bars are those of tests/test_coeff_net.py::test_native_training_gradients_vs_float64 and
tests/test_gpu_coeff_net_bn.py for the same comparisons at batches up to 8."""
import copy
import ctypes
import functools

import pytest
import torch

from hdrnet_amd import models

DEV = "cuda:0"


def randomize(module, seed=0):
    """Move every bias, beta and batch-norm statistic off its initial value (tests/test_coeff_net.py does the same)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if p.dim() == 1 and "bn.weight" not in name:
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
        for name, b in module.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.3 * torch.randn(b.shape, generator=g))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    return module


TINY = dict(net_input_size=64, spatial_bin=8)
# the smallest networks at which each piece can go wrong
CASES = {
    "tiny_b9": (TINY, 9),                                    # the first batch above the narrow kernels' 8
    "tiny_b17": (TINY, 17),                                  # odd, one past a group of 16: the 32-image kernels, half empty
    "tiny_b32": (TINY, 32),                                  # the maximum
    "cm2_b16": (dict(TINY, channel_multiplier=2), 16),       # fc1 has 512 outputs: two 256-output chunks
    "bins4_b12": (dict(TINY, luma_bins=4), 12),              # fc3 with 32 outputs: partial workgroups
    "default_b16": (dict(), 16),                             # the reference's default batch
    # where the first entry points run too (the wide ones must issue their launches)
    "tiny_b2": (TINY, 2),
    "tiny_b8": (TINY, 8),
}
WIDE_CASES = ["tiny_b9", "tiny_b17", "tiny_b32", "cm2_b16", "bins4_b12", "default_b16"]
BN_IDS = {False: "plain", True: "bn"}


def build_model(case, bn, seed=None):
    params, B = CASES[case]
    torch.manual_seed(21 if seed is None else seed)
    m = randomize(models.HDRNetPointwiseNNGuide(dict(batch_norm=bn, **params)), seed=7).train()
    return m, B


def float64_gradients(net, low, wts=None):
    ref = copy.deepcopy(net).double().train()
    out64 = ref(low.double())
    if wts is None:
        wts = torch.randn(out64.shape, dtype=torch.float64)
    (out64 * wts).sum().backward()
    return ref, out64.detach(), wts, {n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None}


NOISE, DRAWS, STABLE = 1e-7, 4, 1e-5


def away_from_kinks(net, low, wts, grads):
    """The gradient of a ReLU network jumps where a pre-activation crosses zero, and at 16 x 256 x 256 the network has four
    million of them: now and then one lies within float32 rounding of zero, and then ANY float32 evaluation -- these
    kernels or the torch ops -- may sit on the other side of the kink, a whole unit's contribution (1e-4 .. 1e-3 of a
    gradient) away from the float64 result.  The comparison below is meaningful only away from such points, so the inputs
    are judged by the float64 module alone: under input noise of the size of the float32 rounding of the input itself
    (1e-7 of its range) every float64 gradient must stay within 1e-5 of its largest magnitude, half the bar's constant,
    in each of four draws.  Between kinks the gradients move by 1 .. 25 times the noise (the larger figure with batch
    norm on the smallest network); across one they jump by 1e-4 or more.  This is a screen, not a proof: a float32
    evaluation rounds every layer, not the input alone.  Measured on the default network at 16 images with batch norm,
    seed 21: the third draw moves splat.2.conv.weight's float64 gradient by 8.1e-4, and the kernels' gradient is 8.07e-4
    off while the torch ops' is 1.1e-6 off; six other seeds at 8 and at 16 images: both within 5e-6.  Without batch norm
    seed 21 passes the screen and both float32 paths cross a kink all the same (local2's weight: kernels 2.0e-3, torch ops
    4.3e-3 off; a batch of 16 equals the sum of two batches of 8 on the narrow kernels to 4.1e-7): the bar is relative to
    the torch ops' own error and holds.  The draws, the seeds and the verdict do not depend on the code under test."""
    g = torch.Generator().manual_seed(99)
    for _ in range(DRAWS):
        noisy = low + NOISE * (2.0 * torch.rand(low.shape, generator=g, dtype=torch.float64) - 1.0)
        _, _, _, moved = float64_gradients(net, noisy, wts)
        for n, ref in grads.items():
            if float((moved[n] - ref).abs().max()) > STABLE * float(ref.abs().max()):
                return False
    return True


@functools.lru_cache(maxsize=None)
def data_seed(case, bn):
    """The first of the seeds 21, 22, .. whose model and batch are `away_from_kinks` (21 is what tests/test_coeff_net.py and
    tests/test_gpu_coeff_net_bn.py use for their batches of up to 8)."""
    if case not in WIDE_CASES:  # compared with another float32 run only, bit for bit
        return 21
    for seed in range(21, 61):
        m, B = build_model(case, bn, seed)
        N = m.params["net_input_size"]
        low = torch.rand(B, N, N, 3)
        _, _, wts, grads = float64_gradients(m.coefficients, low)
        if away_from_kinks(m.coefficients, low.double(), wts, grads):
            return seed
    raise AssertionError(f"{case}: no seed in 21 .. 60 gives a float64 reference away from the ReLU kinks")


@functools.lru_cache(maxsize=None)
def reference(case, bn):
    """(state of the coefficient network, input, cotangent, float64 output, float64 gradients, running statistics after one
    and after three training-mode evaluations -- empty without batch norm); computed once on the CPU, never modified."""
    m, B = build_model(case, bn, data_seed(case, bn))
    N = m.params["net_input_size"]
    low = torch.rand(B, N, N, 3)
    ref, out64, wts, grads = float64_gradients(m.coefficients, low)
    stats1 = {n: b.clone() for n, b in ref.named_buffers() if "running" in n}
    stats3 = {}
    if bn:
        with torch.no_grad():
            ref(low.double())
            ref(low.double())
        stats3 = {n: b.clone() for n, b in ref.named_buffers() if "running" in n}
    return m.coefficients.state_dict(), low, wts, out64, grads, stats1, stats3


def device_net(case, bn):
    m, _ = build_model(case, bn, data_seed(case, bn))
    net = m.coefficients
    net.load_state_dict(reference(case, bn)[0])
    return net.to(DEV).train()


def run(net, low, wts):
    for p in net.parameters():
        p.grad = None
    out = net(low)
    (out * wts).sum().backward()
    return out, {n: p.grad for n, p in net.named_parameters() if p.grad is not None}


def is_native(out, bn):
    name = type(out.grad_fn).__name__ if out.grad_fn is not None else ""
    return ("CoefficientsBnTrain" in name) if bn else ("CoefficientsTrain" in name and "Bn" not in name)


def uses_native(net, low, bn):
    return net._use_native_bn_training(low) if bn else net._use_native_training(low)


@pytest.mark.gpu
@pytest.mark.parametrize("bn", [False, True], ids=BN_IDS.get)
@pytest.mark.parametrize("case", WIDE_CASES)
def test_forward_and_gradients_vs_float64(case, bn):
    """e_native <= 2e-5 + 2 e_stock for every parameter gradient; the output within 1e-5 without batch norm and
    1e-5 + 2 e_stock with it; each error relative to the float64 result's largest magnitude, e_stock the torch ops' on the
    same device."""
    _, low, wts, out64, g64, _, _ = reference(case, bn)
    lowd, wd = low.to(DEV), wts.float().to(DEV)
    net = device_net(case, bn)
    assert uses_native(net, lowd, bn) and not uses_native(net, lowd, not bn)
    out, native = run(net, lowd, wd)
    assert is_native(out, bn), type(out.grad_fn).__name__
    stock_net = device_net(case, bn)
    stock_net.native_training = False
    out_t, stock = run(stock_net, lowd, wd)
    assert not is_native(out_t, bn)
    scale_o = float(out64.abs().max())
    e_out = float((out.detach().cpu().double() - out64).abs().max()) / scale_o
    e_out_t = float((out_t.detach().cpu().double() - out64).abs().max()) / scale_o
    assert set(native) == set(stock) == set(g64)
    worst, worst_t, worst_name, failures = 0.0, 0.0, "", []
    for name, ref in g64.items():
        scale = float(ref.abs().max()) + 1e-30
        e_nat = float((native[name].cpu().double() - ref).abs().max()) / scale
        e_tor = float((stock[name].cpu().double() - ref).abs().max()) / scale
        if e_nat > worst:
            worst, worst_name = e_nat, name
        worst_t = max(worst_t, e_tor)
        assert native[name].stride() == dict(net.named_parameters())[name].stride(), name
        if not e_nat <= 2e-5 + 2.0 * e_tor:
            failures.append((name, e_nat, e_tor))
    print(f"{case} {BN_IDS[bn]}: forward native {e_out:.2e} stock {e_out_t:.2e}; worst gradient native {worst:.2e} "
          f"({worst_name}) stock {worst_t:.2e}")
    assert e_out <= (1e-5 + 2.0 * e_out_t if bn else 1e-5), (e_out, e_out_t)
    assert not failures, failures


def assert_stats(net, want, what):
    got = {n: b for n, b in net.named_buffers() if "running" in n}
    assert set(got) == set(want) and want
    for n, ref in want.items():
        rtol = 1e-5 if n.endswith("running_mean") else 1e-4
        torch.testing.assert_close(got[n].cpu().double(), ref, rtol=rtol, atol=1e-6, msg=lambda m, n=n: f"{what} {n}: {m}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tiny_b9", "tiny_b32", "default_b16"])
def test_running_statistics_after_one_and_three_steps(case):
    _, low, _, _, _, stats1, stats3 = reference(case, True)
    lowd = low.to(DEV)
    net = device_net(case, True)
    assert is_native(net(lowd), True)
    assert_stats(net, stats1, "one step")
    for _ in range(2):
        assert is_native(net(lowd), True)
    assert_stats(net, stats3, "three steps")


GUARD = 4096
PATTERN = 0xA5


def guarded(shape_or_bytes, dtype=torch.uint8, fill=None):
    """A buffer between two guard bands of 0xA5: (the whole allocation, the buffer as `dtype`)."""
    n = int(torch.Size(shape_or_bytes).numel()) if not isinstance(shape_or_bytes, int) else shape_or_bytes
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    whole = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    view = whole[GUARD:GUARD + nbytes].view(dtype)
    if not isinstance(shape_or_bytes, int):
        view = view.view(shape_or_bytes)
    if fill is not None:
        view.fill_(fill)
    return whole, view


def assert_guards(whole, what):
    assert bool((whole[:GUARD] == PATTERN).all()), f"{what}: written before the buffer"
    assert bool((whole[-GUARD:] == PATTERN).all()), f"{what}: written behind the buffer"


def raw_step(case, bn, wide):
    """One forward + backward through the C ABI itself (`wide`: the ..._wide entry points): the output and every gradient
    pre-filled with NaN, both workspaces, the output and every gradient between guard bands.  Returns every result as CPU
    tensors, the running statistics last."""
    from hdrnet_amd import _lib, hdrnet_ops as ops
    _, low, wts, _, _, _, _ = reference(case, bn)
    net = device_net(case, bn)
    B = low.shape[0]
    lowd, dc = low.to(DEV), wts.float().to(DEV).contiguous()
    lib = _lib.load()
    w = "_wide" if wide else ""
    if bn:
        ps, stats = net._train_params_bn()
        desc = ops._live_net_bn(net.hyper, net.n_out, net.n_in, ps, len(net.splat), stats, 1e-3, 1e-3)
        gr = _lib.CoeffNetBnGrads()
        fquery = getattr(lib, f"hdrnet_coefficients_bn{w}_workspace_bytes")
        bquery = getattr(lib, f"hdrnet_coefficients_bn_grad{w}_workspace_bytes")
        fwd = getattr(lib, f"hdrnet_coefficients_bn_train{w}_f32")
        bwd = getattr(lib, f"hdrnet_coefficients_bn_grad{w}_f32")
    else:
        ps, stats = net._train_params(), []
        desc = ops._live_net(net.hyper, net.n_out, net.n_in, ps, len(net.splat))
        gr = _lib.CoeffNetGrads()
        fquery, fwd = lib.hdrnet_coefficients_workspace_bytes, lib.hdrnet_coefficients_f32
        bquery = getattr(lib, f"hdrnet_coefficients_grad{w}_workspace_bytes")
        bwd = getattr(lib, f"hdrnet_coefficients_grad{w}_f32")
    fbytes, bbytes = fquery(ctypes.byref(desc), B), bquery(ctypes.byref(desc), B)
    assert fbytes > 0 and bbytes > 0
    fwhole, fws = guarded(fbytes)
    bwhole, bws = guarded(bbytes)
    sb = net.hyper["spatial_bin"]
    owhole, out = guarded((B, sb, sb, net.gd, net.n_out, net.n_in), torch.float32, float("nan"))
    gwholes, grads = [], []
    for p in ps:
        assert p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last)
        gw, g = guarded(p.numel(), torch.float32, float("nan"))
        gwholes.append(gw)
        grads.append(g)
    it = iter(grads)
    for i in range(len(net.splat)):
        gr.splat_w[i] = next(it).data_ptr()
        if i == 0 or not bn:
            gr.splat_b[i] = next(it).data_ptr()
        else:
            gr.splat_beta[i] = next(it).data_ptr()
    for i in range(2):
        gr.global_conv_w[i] = next(it).data_ptr()
        if bn:
            gr.global_conv_beta[i] = next(it).data_ptr()
        else:
            gr.global_conv_b[i] = next(it).data_ptr()
    for i in range(3):
        gr.fc_w[i] = next(it).data_ptr()
        if bn and i < 2:
            gr.fc_beta[i] = next(it).data_ptr()
        else:
            gr.fc_b[i] = next(it).data_ptr()
    gr.local_w[0] = next(it).data_ptr()
    if bn:
        gr.local_beta = next(it).data_ptr()
    else:
        gr.local_b[0] = next(it).data_ptr()
    gr.local_w[1] = next(it).data_ptr()
    gr.pred_w, gr.pred_b = next(it).data_ptr(), next(it).data_ptr()
    stream = ops._stream(torch.device(DEV))
    rc = fwd(lowd.data_ptr(), ctypes.byref(desc), out.data_ptr(), B, fws.data_ptr(), fbytes, stream)
    _lib.check(rc, "forward")
    rc = bwd(lowd.data_ptr(), ctypes.byref(desc), fws.data_ptr(), dc.data_ptr(), ctypes.byref(gr), B, bws.data_ptr(), bbytes,
             stream)
    _lib.check(rc, "backward")
    torch.cuda.synchronize()
    assert_guards(fwhole, "forward workspace")
    assert_guards(bwhole, "backward workspace")
    assert_guards(owhole, "output")
    assert not bool(torch.isnan(out).any()), "an output element was not written"
    for i, (gw, g) in enumerate(zip(gwholes, grads)):
        assert_guards(gw, f"gradient {i}")
        assert not bool(torch.isnan(g).any()), f"an element of gradient {i} was not written"
    return [out.cpu()] + [g.cpu() for g in grads] + [t.cpu().clone() for st in stats for t in st]


def assert_same_bits(first, second, what):
    assert len(first) == len(second)
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), f"result {i} differs between {what}"


@pytest.mark.gpu
@pytest.mark.parametrize("bn", [False, True], ids=BN_IDS.get)
@pytest.mark.parametrize("case", ["tiny_b9", "tiny_b32", "cm2_b16"])
def test_deterministic_and_within_bounds(case, bn):
    first = raw_step(case, bn, wide=True)
    assert_same_bits(first, raw_step(case, bn, wide=True), "two runs")
    # and the C ABI's results are the autograd Function's
    _, low, wts, _, _, _, _ = reference(case, bn)
    out, _ = run(device_net(case, bn), low.to(DEV), wts.float().to(DEV))
    assert torch.equal(out.detach().cpu(), first[0])


@pytest.mark.gpu
@pytest.mark.parametrize("bn", [False, True], ids=BN_IDS.get)
@pytest.mark.parametrize("case", ["tiny_b2", "tiny_b8"])
def test_wide_entry_points_equal_the_narrow_ones_up_to_8_images(case, bn):
    """Output, every gradient and the running statistics, bit for bit."""
    assert_same_bits(raw_step(case, bn, wide=True), raw_step(case, bn, wide=False), "the wide and the narrow entry points")


@pytest.mark.gpu
@pytest.mark.parametrize("bn", [False, True], ids=BN_IDS.get)
@pytest.mark.parametrize("case", ["tiny_b2", "tiny_b9"])
def test_autograd_path_returns_the_c_abis_bits(case, bn):
    """The module's forward and backward on either side of the narrow / wide switch against `raw_step`, which restates the
    parameter order itself: the output, every parameter gradient and every running statistic, bit for bit (the kernels are
    deterministic).  Each side starts from its own copy of the module, so the statistics move once on each."""
    _, low, wts, _, _, _, _ = reference(case, bn)
    raw = raw_step(case, bn, wide=low.shape[0] > 8)
    net = device_net(case, bn)
    out, _ = run(net, low.to(DEV), wts.float().to(DEV))
    assert is_native(out, bn), type(out.grad_fn).__name__
    ps, stats = net._train_params_bn() if bn else (net._train_params(), [])
    got = [out.detach().cpu()]
    for p in ps:  # raw_step's gradients are flat, in the parameter's memory order
        g = p.grad
        assert g is not None and g.stride() == p.stride()
        got.append((g.permute(0, 2, 3, 1) if g.dim() == 4 else g).contiguous().reshape(-1).cpu())
    got += [t.cpu() for st in stats for t in st]
    assert_same_bits(got, raw, "the autograd path and the C ABI")


@pytest.mark.gpu
@pytest.mark.parametrize("bn", [False, True], ids=BN_IDS.get)
def test_graphed_train_step_matches_eager_native_steps(bn):
    """A captured step of the whole model at 16 x 64 x 64, replayed three times, against the same steps run eagerly
    (compared as tests/test_gpu_coeff_net_bn.py compares the pair at a batch of 2)."""
    from hdrnet_amd.runtime import GraphedTrainStep
    torch.manual_seed(4)
    low = torch.rand(16, 256, 256, 3, device=DEV)
    full = torch.rand(16, 64, 64, 3, device=DEV)
    target = torch.rand(16, 64, 64, 3, device=DEV)

    def loss_fn(out, tgt):
        return (out - tgt).square().mean()

    m0 = models.HDRNetPointwiseNNGuide(dict(batch_norm=bn)).to(DEV).train()
    state = {k: v.clone() for k, v in m0.state_dict().items()}

    def make():
        m = models.HDRNetPointwiseNNGuide(dict(batch_norm=bn)).to(DEV).train()
        m.load_state_dict(state)
        opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-5)
        return m, opt

    me, oe = make()
    assert uses_native(me.coefficients, low, bn)
    assert is_native(me.coefficients(low), bn)
    me, oe = make()  # (with batch norm the probe above moved the running statistics)
    for _ in range(2 + 3):  # GraphedTrainStep warms up with 2 eager steps before capturing
        oe.zero_grad(set_to_none=True)
        le = loss_fn(me(low, full), target)
        le.backward()
        oe.step()
    mg, og = make()
    gstep = GraphedTrainStep(mg, loss_fn, og, [low, full], [target], warmup=2)
    for _ in range(3):
        lg = gstep([low, full], [target])
    torch.testing.assert_close(lg, le, rtol=1e-3, atol=1e-6)
    for (name, p), (_, q) in zip(mg.named_parameters(), me.named_parameters()):
        if not p.requires_grad:
            continue
        p0 = state[name]
        dg, de = p.detach() - p0, q.detach() - p0
        scale = de.abs().max().item()
        assert scale > 0, name
        assert (dg - de).abs().max().item() <= 5e-2 * scale, (name, (dg - de).abs().max().item(), scale)
    moved = False
    for (name, a), (_, b) in zip(mg.named_buffers(), me.named_buffers()):
        if name.endswith("running_mean"):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
            moved = moved or not torch.equal(a, state[name])
        elif name.endswith("running_var"):
            torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)
    assert moved or not bn, "the replays did not move the running statistics"


@pytest.mark.gpu
@pytest.mark.parametrize("bn", [False, True], ids=BN_IDS.get)
def test_fallbacks_keep_the_torch_ops(bn):
    torch.manual_seed(3)
    net = randomize(models.HDRNetPointwiseNNGuide(dict(batch_norm=bn, **TINY)), seed=1).to(DEV).train().coefficients
    low = torch.rand(33, 64, 64, 3, device=DEV)
    assert uses_native(net, low[:32], bn) and is_native(net(low[:32]), bn)
    # a batch of 33: beyond the wide kernels
    assert not net._use_native_training(low) and not net._use_native_bn_training(low)
    out = net(low)
    assert not is_native(out, bn) and out.grad_fn is not None
    out.sum().backward()
    # the switch
    net.native_training = False
    assert not uses_native(net, low[:16], bn) and not is_native(net(low[:16]), bn)
    net.native_training = True
    # the input's own gradient
    lowg = low[:16].clone().requires_grad_(True)
    out = net(lowg)
    assert not uses_native(net, lowg, bn) and not is_native(out, bn)
    out.sum().backward()
    assert lowg.grad is not None
