"""The coefficient network trained WITH batch norm on the HIP kernels (csrc/coeff_net_bn.hip between the launches of
csrc/coeff_net.hip / coeff_net_train.hip; hdrnet_ops.coefficients_bn_train) against the same module in float64 on the CPU:
forward, every gradient, the running statistics; determinism and buffer bounds; the caches that depend on the running
statistics; the whole model, eager and as a captured graph; and the cases that must keep running the torch ops.

The bars are the project's own for the same comparisons without batch norm (tests/test_coeff_net.py:
test_native_training_gradients_vs_float64) and for the guide network's batch norm (tests/test_models.py:
test_training_fused_guide_matches_unfused_module, test_graphed_train_step_matches_eager)."""
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


# the smallest shapes at which each piece can go wrong
CASES = {
    "default_b2": (dict(), 2),                                      # the minimum batch
    "default_b3": (dict(), 3),                                      # odd batch
    "default_b4": (dict(), 4),
    "small_b8": (dict(net_input_size=128, spatial_bin=8), 8),       # the maximum batch
    "tiny_b2": (dict(net_input_size=64, spatial_bin=8), 2),         # the smallest M
    "bins4_b3": (dict(luma_bins=4), 3),                             # C = 4: one float4 per pixel
    "cm2_b2": (dict(channel_multiplier=2), 2),
    "grid32_b2": (dict(spatial_bin=32), 2),
    "pyramid_b2": (dict(_cls="pyramid"), 2),                        # n_out = 9
}


def build_model(case):
    params, B = CASES[case]
    params = dict(params)
    cls = models.HDRNetGaussianPyrNN if params.pop("_cls", "") == "pyramid" else models.HDRNetPointwiseNNGuide
    torch.manual_seed(21)
    m = randomize(cls(dict(batch_norm=True, **params)), seed=7).train()
    return m, B


@functools.lru_cache(maxsize=None)
def reference(case):
    """(state of the coefficient network, inputs, cotangent, float64 results of three training-mode evaluations); computed
    once, never modified.  The first evaluation's output and gradients, and the running statistics after one and after
    three evaluations of the same batch."""
    m, B = build_model(case)
    N = m.params["net_input_size"]
    low = torch.rand(B, N, N, 3)
    ref = copy.deepcopy(m.coefficients).double().train()
    out64 = ref(low.double())
    wts = torch.randn(out64.shape, dtype=torch.float64)
    (out64 * wts).sum().backward()
    grads = {n: p.grad.clone() for n, p in ref.named_parameters() if p.grad is not None}
    stats1 = {n: b.clone() for n, b in ref.named_buffers() if "running" in n}
    with torch.no_grad():
        ref(low.double())
        ref(low.double())
    stats3 = {n: b.clone() for n, b in ref.named_buffers() if "running" in n}
    return m.coefficients.state_dict(), low, wts, out64.detach(), grads, stats1, stats3


def device_net(case):
    m, _ = build_model(case)
    net = m.coefficients
    net.load_state_dict(reference(case)[0])
    return net.to(DEV).train()


def run(net, low, wts):
    for p in net.parameters():
        p.grad = None
    out = net(low)
    (out * wts).sum().backward()
    return out, {n: p.grad for n, p in net.named_parameters() if p.grad is not None}


def is_native(out):
    return out.grad_fn is not None and "CoefficientsBnTrain" in type(out.grad_fn).__name__


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_forward_and_gradients_vs_float64(case):
    """e_native <= 2e-5 + 2 e_stock for every parameter gradient (beta's included) and 1e-5 + 2 e_stock for the output,
    each error relative to the float64 result's largest magnitude."""
    _, low, wts, out64, g64, _, _ = reference(case)
    lowd, wd = low.to(DEV), wts.float().to(DEV)
    net = device_net(case)
    assert net._use_native_bn_training(lowd) and not net._use_native_training(lowd)
    out, native = run(net, lowd, wd)
    assert is_native(out), type(out.grad_fn).__name__
    stock_net = device_net(case)
    stock_net.native_training = False
    out_t, stock = run(stock_net, lowd, wd)
    assert not is_native(out_t)
    scale_o = float(out64.abs().max())
    e_out = float((out.detach().cpu().double() - out64).abs().max()) / scale_o
    e_out_t = float((out_t.detach().cpu().double() - out64).abs().max()) / scale_o
    worst, worst_t, worst_name = 0.0, 0.0, ""
    assert set(native) == set(stock) == set(g64)
    assert any("bn.bias" in n for n in g64) and not any("bn.weight" in n for n in g64)
    failures = []
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
    print(f"{case}: forward native {e_out:.2e} stock {e_out_t:.2e}; worst gradient native {worst:.2e} ({worst_name}) "
          f"stock {worst_t:.2e}")
    assert e_out <= 1e-5 + 2.0 * e_out_t, (e_out, e_out_t)
    assert not failures, failures


def assert_stats(net, want, what):
    got = {n: b for n, b in net.named_buffers() if "running" in n}
    assert set(got) == set(want)
    for n, ref in want.items():
        rtol = 1e-5 if n.endswith("running_mean") else 1e-4
        torch.testing.assert_close(got[n].cpu().double(), ref, rtol=rtol, atol=1e-6, msg=lambda m, n=n: f"{what} {n}: {m}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["default_b2", "default_b3", "small_b8", "bins4_b3"])
def test_running_statistics_after_one_and_three_steps(case):
    _, low, wts, _, _, stats1, stats3 = reference(case)
    lowd = low.to(DEV)
    net = device_net(case)
    versions = {n: b._version for n, b in net.named_buffers() if "running" in n}
    assert is_native(net(lowd))
    assert_stats(net, stats1, "one step")
    assert all(b._version > versions[n] for n, b in net.named_buffers() if "running" in n)
    for _ in range(2):
        assert is_native(net(lowd))
    assert_stats(net, stats3, "three steps")


GUARD = 4096
PATTERN = 0xA5


def guarded(nbytes):
    whole = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
    return whole, whole[GUARD:GUARD + nbytes]


def assert_guards(whole, nbytes, what):
    assert bool((whole[:GUARD] == PATTERN).all()), f"{what}: written before the buffer"
    assert bool((whole[GUARD + nbytes:] == PATTERN).all()), f"{what}: written behind the buffer"


def raw_step(case):
    """One forward + backward through the C ABI itself: outputs and gradients pre-filled with NaN, both workspaces between
    guard bands.  Returns every result as CPU tensors."""
    from hdrnet_amd import _lib, hdrnet_ops as ops
    _, low, wts, _, _, _, _ = reference(case)
    net = device_net(case)
    ps, stats = net._train_params_bn()
    B = low.shape[0]
    lowd, dc = low.to(DEV), wts.float().to(DEV).contiguous()
    desc = ops._live_net_bn(net.hyper, net.n_out, net.n_in, ps, len(net.splat), stats, 1e-3, 1e-3)
    lib = _lib.load()
    fbytes = lib.hdrnet_coefficients_bn_workspace_bytes(ctypes.byref(desc), B)
    bbytes = lib.hdrnet_coefficients_bn_grad_workspace_bytes(ctypes.byref(desc), B)
    assert fbytes > 0 and bbytes > 0
    fwhole, fws = guarded(fbytes)
    bwhole, bws = guarded(bbytes)
    out = torch.full((B, net.hyper["spatial_bin"], net.hyper["spatial_bin"], net.gd, net.n_out, net.n_in), float("nan"),
                     device=DEV)
    grads = [torch.full_like(p, float("nan")) for p in ps]
    gr = _lib.CoeffNetBnGrads()
    it = iter(grads)
    for i in range(len(net.splat)):
        gr.splat_w[i] = next(it).data_ptr()
        if i == 0:
            gr.splat_b[0] = next(it).data_ptr()
        else:
            gr.splat_beta[i] = next(it).data_ptr()
    for i in range(2):
        gr.global_conv_w[i], gr.global_conv_beta[i] = next(it).data_ptr(), next(it).data_ptr()
    for i in range(2):
        gr.fc_w[i], gr.fc_beta[i] = next(it).data_ptr(), next(it).data_ptr()
    gr.fc_w[2], gr.fc_b[2] = next(it).data_ptr(), next(it).data_ptr()
    gr.local_w[0], gr.local_beta = next(it).data_ptr(), next(it).data_ptr()
    gr.local_w[1] = next(it).data_ptr()
    gr.pred_w, gr.pred_b = next(it).data_ptr(), next(it).data_ptr()
    stream = ops._stream(torch.device(DEV))
    rc = lib.hdrnet_coefficients_bn_train_f32(lowd.data_ptr(), ctypes.byref(desc), out.data_ptr(), B, fws.data_ptr(), fbytes,
                                              stream)
    _lib.check(rc, "train")
    rc = lib.hdrnet_coefficients_bn_grad_f32(lowd.data_ptr(), ctypes.byref(desc), fws.data_ptr(), dc.data_ptr(),
                                             ctypes.byref(gr), B, bws.data_ptr(), bbytes, stream)
    _lib.check(rc, "grad")
    torch.cuda.synchronize()
    assert_guards(fwhole, fbytes, "forward workspace")
    assert_guards(bwhole, bbytes, "backward workspace")
    assert not bool(torch.isnan(out).any()), "an output element was not written"
    for p, g in zip(ps, grads):
        assert not bool(torch.isnan(g).any()), "a gradient element was not written"
    return [out.cpu()] + [g.cpu() for g in grads] + [t.cpu().clone() for st in stats for t in st]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["default_b3", "tiny_b2", "small_b8"])
def test_deterministic_and_within_bounds(case):
    first, second = raw_step(case), raw_step(case)
    assert len(first) == len(second)
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), f"result {i} differs between two runs"
    # and the C ABI's results are the autograd Function's
    _, low, wts, _, _, _, _ = reference(case)
    net = device_net(case)
    out, _ = run(net, low.to(DEV), wts.float().to(DEV))
    assert torch.equal(out.detach().cpu(), first[0])


@pytest.mark.gpu
def test_inference_after_a_native_step_folds_the_new_statistics():
    """exported()'s cache is keyed on the buffers' versions: after a native step the native inference path must see the
    statistics that step wrote, as the torch ops do (tests/test_coeff_net.py's tolerance for that pair)."""
    torch.manual_seed(5)
    m = randomize(models.HDRNetPointwiseNNGuide(dict(batch_norm=True)), seed=3).to(DEV)
    for mod in m.coefficients.modules():
        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
            mod.momentum = 0.5  # one step moves the statistics far enough to tell the old fold from the new
    low = torch.rand(2, 256, 256, 3, device=DEV)
    full = torch.rand(2, 136, 240, 3, device=DEV)
    m.eval()
    with torch.no_grad():
        before = m.coefficients(low).clone()  # fills the cache with the old statistics
    m.train()
    out = m.coefficients(low)
    assert is_native(out)
    out.square().sum().backward()
    m.eval()
    with torch.no_grad():
        got_c = m.coefficients(low)
        got = m(low, full)
        m.coefficients.native = False
        want_c = m.coefficients(low)
        want = m(low, full)
        m.coefficients.native = True
    assert not torch.allclose(before, want_c, rtol=1e-4, atol=1e-4), "the step did not move the statistics enough to tell"
    assert torch.allclose(got_c, want_c, rtol=1e-4, atol=1e-4), float((got_c - want_c).abs().max())
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-4), float((got - want).abs().max())


def _whole_model_pair():
    torch.manual_seed(2)
    m = models.HDRNetPointwiseNNGuide(dict(batch_norm=True)).to(DEV).train()
    ref = models.HDRNetPointwiseNNGuide(dict(batch_norm=True)).to(DEV).train()
    ref.load_state_dict(m.state_dict())
    ref.coefficients.native_training = False
    low = torch.rand(2, 256, 256, 3, device=DEV)
    full = torch.rand(2, 136, 240, 3, device=DEV)
    target = torch.rand(2, 136, 240, 3, device=DEV)
    return m, ref, low, full, target


@pytest.mark.gpu
def test_whole_model_matches_the_stock_op_twin():
    m, ref, low, full, target = _whole_model_pair()
    assert m.coefficients._use_native_bn_training(low) and not ref.coefficients._use_native_bn_training(low)
    loss = (m(low, full) - target).square().mean()
    loss.backward()
    loss_ref = (ref(low, full) - target).square().mean()
    loss_ref.backward()
    torch.testing.assert_close(loss, loss_ref, rtol=1e-5, atol=1e-7)
    for (name, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        if not p.requires_grad:
            continue
        assert p.grad is not None, name
        scale = q.grad.abs().max().item()
        err = (p.grad - q.grad).abs().max().item()
        assert err <= 1e-3 * scale + 1e-7, (name, err, scale)
    for (name, a), (_, b) in zip(m.named_buffers(), ref.named_buffers()):
        if name.endswith("running_mean"):
            torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)
        elif name.endswith("running_var"):
            torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-6)


@pytest.mark.gpu
def test_graphed_train_step_matches_eager_native_steps():
    from hdrnet_amd.runtime import GraphedTrainStep
    torch.manual_seed(4)
    low = torch.rand(2, 256, 256, 3, device=DEV)
    full = torch.rand(2, 136, 240, 3, device=DEV)
    target = torch.rand(2, 136, 240, 3, device=DEV)

    def loss_fn(out, tgt):
        return (out - tgt).square().mean()

    m0 = models.HDRNetPointwiseNNGuide(dict(batch_norm=True)).to(DEV).train()
    state = {k: v.clone() for k, v in m0.state_dict().items()}

    def make():
        m = models.HDRNetPointwiseNNGuide(dict(batch_norm=True)).to(DEV).train()
        m.load_state_dict(state)
        opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=1e-5)
        return m, opt

    me, oe = make()
    assert me.coefficients._use_native_bn_training(low)
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
    assert moved, "the replays did not move the running statistics"


@pytest.mark.gpu
def test_fallbacks_keep_the_torch_ops():
    torch.manual_seed(3)
    m = randomize(models.HDRNetPointwiseNNGuide(dict(batch_norm=True)), seed=1).to(DEV).train()
    net = m.coefficients
    low = torch.rand(2, 256, 256, 3, device=DEV)
    assert net._use_native_bn_training(low) and is_native(net(low))
    assert not net._use_native_training(low)
    # a batch of one: torch's own refusal
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        net(low[:1])
    # the input's own gradient
    lowg = low.clone().requires_grad_(True)
    out = net(lowg)
    assert not net._use_native_bn_training(lowg) and not is_native(out)
    out.sum().backward()
    assert lowg.grad is not None
    # the switch
    net.native_training = False
    assert not net._use_native_bn_training(low) and not is_native(net(low))
    net.native_training = True
    # a gamma that is not 1 (the kernels have no scale)
    with torch.no_grad():
        net.local1.bn.bn.weight.fill_(1.5)
    assert not net._use_native_bn_training(low) and not is_native(net(low))
    with torch.no_grad():
        net.local1.bn.bn.weight.fill_(1.0)
    assert net._use_native_bn_training(low)
    # a gamma that is trained, a beta that is not
    net.fc1.bn.bn.weight.requires_grad_(True)
    assert not net._use_native_bn_training(low)
    net.fc1.bn.bn.weight.requires_grad_(False)
    net.fc2.bn.bn.bias.requires_grad_(False)
    assert not net._use_native_bn_training(low)
    net.fc2.bn.bn.bias.requires_grad_(True)
    # inference, no_grad
    with torch.no_grad():
        assert not net._use_native_bn_training(low)
    net.eval()
    assert not net._use_native_bn_training(low)
