"""The training-side kernels of guide_grad.hip -- guide_nn_grad, curves_guide_grad, input_moments -- at config #4's
4 x 1080p (8 294 400 pixels) against float64, where their persistent grid-stride loops make several passes.

They launch at most 4 x CUs workgroups of 256 threads (persistent_blocks): guide_nn_grad and input_moments walk 4-pixel
quads, so one pass covers 4 S pixels (S = workgroups x 256), curves_guide_grad single pixels (S).  The suite's other
tests stay within one pass of the first two.  Bars: a parameter gradient |err| <= 1e-5 x sum_px |term| (the sum taken
in float64); a per-pixel input gradient |err| <= 1e-5 x the sum of its terms' magnitudes.  Where the float32 kernel
and the float64 reference may take a ReLU / clip kink on different sides (|pre-activation| within 1e-6 of the
kink's scale), a pixel's dinput is not compared; those pixels are counted and must be rare.  The planted-spike tests
put the whole dguide on the first and last pixel of every pass: a skipped or repeated pass moves the result by a
whole term."""
import ctypes
import math

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NPX = 4 * 1080 * 1920  # config #4: 4 x 1080p
REL = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from hdrnet_amd import hdrnet_ops
    return hdrnet_ops


def pass_pixels(dev, npx, px_per_thread):
    """Pixels per pass of the persistent loop (guide_grad.hip: persistent_blocks)."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    nb = min(math.ceil(npx / 1024), 4 * cus)
    return nb * 256 * px_per_thread


def spike_pixels(npx, span):
    """0, npx - 1 and both sides of every pass boundary."""
    px = {0, npx - 1}
    for k in range(1, (npx - 1) // span + 1):
        px |= {k * span - 1, k * span}
    return torch.tensor(sorted(p for p in px if p < npx), dtype=torch.long)


def param_close(name, got, want, scale, fp32=None):
    """|got - want| <= 1e-5 x scale elementwise (scale = sum_px |term| in float64)."""
    err = (got.double() - want).abs()
    bar = REL * scale + 1e-30
    worst = float((err / bar).max())
    extra = ""
    if fp32 is not None:
        extra = f"; fp32 torch composition: max|err| = {float((fp32.double() - want).abs().max()):.3e}, " \
                f"worst / bar = {float(((fp32.double() - want).abs() / bar).max()):.2f}"
    print(f"{name}: max|err| = {float(err.max()):.3e}, worst / (1e-5 sum|term|) = {worst:.2f}{extra}")
    assert worst <= 1.0, (name, worst)


def pixel_close(name, got, want, scale, kink):
    """dinput per pixel against float64; `kink`: pixels [npx] left out (a kink within rounding), counted."""
    ok = ~kink
    err = (got.double() - want).abs()
    bar = REL * scale + 1e-30
    worst = float((err / bar)[ok].max())
    n_kink = int(kink.sum())
    print(f"{name}: max|err| = {float(err[ok].max()):.3e}, worst / (1e-5 sum|term|) = {worst:.2f}; "
          f"{n_kink} pixels at a kink left out (max|err| there {float(err[kink].max()) if n_kink else 0.0:.3e})")
    assert worst <= 1.0, (name, worst)
    assert n_kink <= 1e-4 * kink.shape[0], (name, n_kink)


# ---- guide_nn_grad ---------------------------------------------------------------------------------------------------
def nn_reference(x, dguide, c1, c2, chunk=1 << 21):
    """float64 autograd of the folded guide network (tests/test_models.py: _torch_guide), accumulated over pixel chunks:
    dconv1, dconv2, dinput, the sums of |term| for each, the float32 guide the forward would have saved, and the pixels
    whose features sit within rounding of the ReLU's kink."""
    npx, Cin = x.shape
    n = c1.shape[0]
    d1 = c1.double()
    d2 = c2.double()
    out = dict(dc1=torch.zeros_like(d1), dc2=torch.zeros_like(d2), s1=torch.zeros_like(d1), s2=torch.zeros_like(d2))
    din, sin, guide, kink = [], [], [], []
    for a in range(0, npx, chunk):
        xb = x[a:a + chunk].double().requires_grad_(True)
        p1, p2 = d1.clone().requires_grad_(True), d2.clone().requires_grad_(True)
        h = xb @ p1[:, :-1].t() + p1[:, -1]
        g = torch.sigmoid(torch.relu(h) @ p2[:-1] + p2[-1])
        (g * dguide[a:a + chunk].double()).sum().backward()
        out["dc1"] += p1.grad
        out["dc2"] += p2.grad
        din.append(xb.grad)
        with torch.no_grad():
            g = g.detach()
            da = (dguide[a:a + chunk].double() * g * (1 - g)).abs()
            on = (h > 0).double()
            xa = torch.cat([xb.detach().abs(), torch.ones_like(xb[:, :1])], 1)
            out["s1"] += (p2[:-1].abs()[:, None] * ((da[:, None] * on).t() @ xa))
            out["s2"][:-1] += (da[:, None] * torch.relu(h)).sum(0)
            out["s2"][-1] += da.sum()
            sin.append((da[:, None] * on * p2[:-1].abs()) @ d1[:, :-1].abs())
            hs = xb.detach().abs() @ d1[:, :-1].abs().t() + d1[:, -1].abs()
            kink.append(((h.abs() <= 1e-6 * hs).any(1)))
            guide.append(g.float())
    return out, torch.cat(din), torch.cat(sin), torch.cat(guide), torch.cat(kink)


def nn_case(dev, Cin, n, npx, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand((npx, Cin), device=dev, generator=gen)
    c1 = torch.randn((n, Cin + 1), device=dev, generator=gen) * 0.8
    c2 = torch.randn((n + 1,), device=dev, generator=gen) * 0.5
    dguide = torch.randn((npx,), device=dev, generator=gen)
    return x, c1, c2, dguide


@pytest.mark.parametrize("npx", [NPX, NPX + 1])
@pytest.mark.parametrize("Cin,n", [(3, 16), (3, 8), (1, 4)])
def test_guide_nn_grad_4x1080p_vs_float64(dev, ops, Cin, n, npx):
    """hdrnet_ops._guide_backward with dinput None (parameters only), stored, and accumulated into a pre-filled
    buffer; the parameters-only and the with-dinput forms within the same bar of float64 (and so of each other)."""
    x, c1, c2, dguide = nn_case(dev, Cin, n, npx, seed=Cin * 100 + n + npx % 2)
    ref, din64, sin64, guide, kink = nn_reference(x, dguide, c1, c2)
    # the fp32 torch composition the training-side tests compare with, for scale
    xf, f1, f2 = x.clone().requires_grad_(True), c1.clone().requires_grad_(True), c2.clone().requires_grad_(True)
    gf = torch.sigmoid(torch.relu(xf @ f1[:, :-1].t() + f1[:, -1]) @ f2[:-1] + f2[-1])
    (gf * dguide).sum().backward()
    tag = f"guide_nn_grad Cin={Cin} n={n} npx={npx}"
    prefill = torch.randn((npx, Cin), device=dev)
    forms = (("parameters only", None, False), ("dinput stored", torch.empty((npx, Cin), device=dev), False),
             ("dinput accumulated", prefill.clone(), True))
    for form, dinput, acc in forms:
        dc1, dc2 = ops._guide_backward(x, guide, dguide, c1, c2, dinput, accumulate=acc)
        assert ops.last_kernel() == "guide_nn_grad", ops.last_kernel()
        param_close(f"{tag} [{form}] dconv1", dc1, ref["dc1"], ref["s1"], f1.grad)
        param_close(f"{tag} [{form}] dconv2", dc2, ref["dc2"], ref["s2"], f2.grad)
        if dinput is not None:
            got = dinput.double() - prefill.double() if acc else dinput
            scale = sin64 + (prefill.double().abs() * 2 ** -23 / REL if acc else 0)  # + the float32 add's rounding
            pixel_close(f"{tag} [{form}] dinput", got, din64, scale, kink[:, None].expand_as(din64))


@pytest.mark.parametrize("Cin,n", [(3, 16), (1, 4)])
def test_guide_nn_grad_planted_spikes(dev, ops, Cin, n):
    """dguide zero except at pixels 0, npx - 1 and both sides of every pass boundary (4 S k): the parameter gradients
    are the float64 sum over those pixels, to 1e-5 of the sum of their magnitudes."""
    npx = NPX + 1
    x, c1, c2, _ = nn_case(dev, Cin, n, npx, seed=9)
    span = pass_pixels(dev, npx, 4)
    px = spike_pixels(npx, span).to(dev)
    assert len(px) >= 2 * (npx // span) + 2 - 1
    dguide = torch.zeros((npx,), device=dev)
    dguide[px] = 1.0 + torch.rand((len(px),), device=dev)
    ref, _, _, guide, _ = nn_reference(x, dguide, c1, c2)
    sub, _, _, _, _ = nn_reference(x[px], dguide[px], c1, c2)
    for form, dinput in (("parameters only", None), ("dinput stored", torch.empty((npx, Cin), device=dev))):
        dc1, dc2 = ops._guide_backward(x, guide, dguide, c1, c2, dinput, accumulate=False)
        assert ops.last_kernel() == "guide_nn_grad", ops.last_kernel()
        tag = f"spikes guide_nn_grad Cin={Cin} n={n} ({len(px)} pixels, pass = {span} px) [{form}]"
        param_close(tag + " dconv1", dc1, sub["dc1"], sub["s1"])
        param_close(tag + " dconv2", dc2, sub["dc2"], sub["s2"])
    assert torch.allclose(ref["dc1"], sub["dc1"]) and torch.allclose(ref["dc2"], sub["dc2"])


# ---- curves_guide_grad -----------------------------------------------------------------------------------------------
def curves_case(dev, npx, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand((npx, 3), device=dev, generator=gen)
    ccm = torch.cat([torch.eye(3, device=dev), torch.zeros(3, 1, device=dev)], 1) + \
        0.3 * torch.randn((3, 4), device=dev, generator=gen)
    shifts = torch.linspace(0, 1, 17, device=dev)[:-1, None].repeat(1, 3) + \
        0.013 * torch.randn((16, 3), device=dev, generator=gen)
    slopes = 0.1 * torch.randn((16, 3), device=dev, generator=gen)
    slopes[0] += 1.0
    mix = torch.tensor([0.9, 0.8, 0.7, -0.4], device=dev)  # pre-clip range ~[-0.4, 2]: clips on both sides
    dguide = torch.randn((npx,), device=dev, generator=gen)
    return x, (ccm, shifts, slopes, mix), dguide


def curves_reference(x, params, dguide, chunk=1 << 20):
    """float64 autograd of the curves formula (tests/test_models.py: test_fused_curves_apply_gradients_match_composition)
    over pixel chunks: the four parameter gradients and dinput, the sums of |term|, and the pixels at a kink -- within
    rounding of a knot (t - shift) or of either end of the clip, where float32 may take the other side."""
    p64 = [p.double() for p in params]
    grads = [torch.zeros_like(p) for p in p64]
    sums = [torch.zeros_like(p) for p in p64]
    din, sin, kink = [], [], []
    clipped = 0
    for a in range(0, x.shape[0], chunk):
        xb = x[a:a + chunk].double().requires_grad_(True)
        leaves = [p.clone().requires_grad_(True) for p in p64]
        c, sh, sl, mx = leaves
        t = (xb.unsqueeze(-2) * c[:, :3]).sum(-1) + c[:, 3]
        arg = t.unsqueeze(-1) - sh.t()                       # [px, 3, 16]
        cv = (sl.t() * torch.relu(arg)).sum(-1)
        pre = (cv * mx[:3]).sum(-1) + mx[3]
        g = pre.clamp(0.0, 1.0)
        db = dguide[a:a + chunk].double()
        (g * db).sum().backward()
        for k in range(4):
            grads[k] += leaves[k].grad
        din.append(xb.grad)
        with torch.no_grad():
            dgk = db.abs() * ((pre >= 0) & (pre <= 1)).double()    # [px]
            clipped += int(((pre < 0) | (pre > 1)).sum())
            on = (arg > 0).double()
            wm = dgk[:, None] * p64[3][:3].abs()                     # |dgk mix_c| [px, 3]
            dts = wm * (on * p64[2].abs().t()).sum(-1)               # sum of |d t_c| terms [px, 3]
            xa = torch.cat([xb.detach().abs(), torch.ones_like(xb[:, :1])], 1)
            sums[0] += dts.t() @ xa                                  # dccm [3, 4]
            sums[1] += ((wm[:, :, None] * on).sum(0) * p64[2].abs().t()).t()  # dshifts [16, 3]
            # relu(t - shift) is known to the rounding of its operands, not of its value: |t| + |shift| per term
            ts = xb.detach().abs() @ p64[0][:, :3].abs().t() + p64[0][:, 3].abs()        # [px, 3]
            mag = on * (ts.unsqueeze(-1) + p64[1].abs().t())                              # [px, 3, 16]
            sums[2] += (wm[:, :, None] * mag).sum(0).t()                                  # dslopes [16, 3]
            sums[3][:3] += (dgk[:, None] * (p64[2].abs().t() * mag).sum(-1)).sum(0)
            sums[3][3] += dgk.sum()
            sin.append(dts @ p64[0][:, :3].abs())
            near = (arg.abs() <= 1e-6 * (ts.unsqueeze(-1) + p64[1].abs().t())).any(-1).any(-1)
            near |= (pre.abs() <= 1e-6 * 4) | ((pre - 1).abs() <= 1e-6 * 4)
            kink.append(near)
    return grads, sums, torch.cat(din), torch.cat(sin), torch.cat(kink), clipped / x.shape[0]


def curves_grad(dev, x, params, dguide, dinput=None, accumulate=False):
    """hdrnet_curves_guide_grad_f32 through ctypes; returns (dccm, dshifts, dslopes, dmix)."""
    from hdrnet_amd import _lib
    lib = _lib.load()
    npx = x.shape[0]
    outs = [torch.empty_like(p) for p in params]
    with torch.cuda.device(dev):
        wbytes = lib.hdrnet_curves_guide_grad_workspace_bytes(npx, 3, 16)
        ws = torch.empty((max(wbytes, 16),), dtype=torch.uint8, device=dev)
        rc = lib.hdrnet_curves_guide_grad_f32(
            x.data_ptr(), dguide.data_ptr(), *[p.data_ptr() for p in params],
            None if dinput is None else dinput.data_ptr(), int(accumulate), *[o.data_ptr() for o in outs],
            ctypes.c_longlong(npx), 3, 16, ws.data_ptr(), wbytes, torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(rc, "CurvesGuideGrad")
    torch.cuda.synchronize()
    assert _lib.last_kernel() == "curves_guide_grad", _lib.last_kernel()
    return outs


NAMES = ("dccm", "dshifts", "dslopes", "dmix")


@pytest.mark.parametrize("npx", [NPX, NPX + 1])
def test_curves_guide_grad_4x1080p_vs_float64(dev, npx):
    """16 knots, the guide clipped on both sides: dccm, dshifts, dslopes, dmix and dinput (stored, and accumulated into
    a pre-filled buffer) against float64 autograd."""
    x, params, dguide = curves_case(dev, npx, seed=npx % 2 + 40)
    kink = curves_reference(x, params, dguide)[4]
    # a pixel at a kink carries a whole term that float32 and float64 may count differently (measured: ~0.1 each, a
    # few hundred pixels of 8.3 M): its dguide is set to zero, on both sides, so that what is compared is the sums
    dguide = torch.where(kink, torch.zeros_like(dguide), dguide)
    grads, sums, din64, sin64, _, clipped = curves_reference(x, params, dguide)
    print(f"curves npx={npx}: {clipped:.3f} of the pixels clipped, {int(kink.sum())} at a kink (dguide zeroed)")
    assert 0.02 < clipped < 0.9
    assert kink.sum() < 1e-3 * npx
    kink = torch.zeros_like(kink)
    prefill = torch.randn((npx, 3), device=dev)
    for form, dinput, acc in (("dinput stored", torch.empty((npx, 3), device=dev), False),
                              ("dinput accumulated", prefill.clone(), True)):
        outs = curves_grad(dev, x, params, dguide, dinput, acc)
        tag = f"curves_guide_grad npx={npx} [{form}]"
        for nm, o, w, s in zip(NAMES, outs, grads, sums):
            param_close(f"{tag} {nm}", o, w, s)
        got = dinput.double() - prefill.double() if acc else dinput
        scale = sin64 + (prefill.double().abs() * 2 ** -23 / REL if acc else 0)
        pixel_close(f"{tag} dinput", got, din64, scale, kink[:, None].expand_as(din64))


def test_curves_guide_grad_planted_spikes(dev):
    """dguide zero except at pixels 0, npx - 1 and both sides of every pass boundary (S k)."""
    npx = NPX + 1
    x, params, _ = curves_case(dev, npx, seed=41)
    span = pass_pixels(dev, npx, 1)
    px = spike_pixels(npx, span).to(dev)
    px = px[~curves_reference(x[px], params, torch.ones((len(px),), device=dev))[4]]  # (none at a kink, in practice)
    assert len(px) >= 2 * (npx // span)
    dguide = torch.zeros((npx,), device=dev)
    dguide[px] = 1.0 + torch.rand((len(px),), device=dev)
    grads, sums, _, _, _, _ = curves_reference(x[px], params, dguide[px])
    outs = curves_grad(dev, x, params, dguide)
    for nm, o, w, s in zip(NAMES, outs, grads, sums):
        param_close(f"spikes curves_guide_grad ({len(px)} pixels, pass = {span} px) {nm}", o, w, s)


# ---- input_moments and the batch-norm fold ---------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (0.45, 0.55)])
def test_input_moments_4x1080p_and_fold(dev, ops, lo, hi):
    """sum_px x_j and sum_px x_i x_j of a 4 x 1080p batch against float64 sums (rtol 1e-6), and the training-mode fold
    computed from them (guide_fold_batch) against a float64 fold of float64 moments: conv1 and the running variance
    within 1e-4 relative -- Cov = M / N - mu mu^T cancels, worst on the low-contrast input."""
    gen = torch.Generator(device=dev).manual_seed(77)
    x = lo + (hi - lo) * torch.rand((4, 1080, 1920, 3), device=dev, generator=gen)
    x[:, :, -1, :] = hi  # (a few pixels at the top of the range)
    sums, mom = ops.input_moments(x)
    assert ops.last_kernel() == "input_moments", ops.last_kernel()
    flat = x.reshape(-1, 3).double()
    s64, m64 = flat.sum(0), flat.t() @ flat
    for nm, got, want in (("sums", sums, s64), ("moments", mom, m64)):
        err = (got.double() - want).abs()
        worst = float((err / (1e-6 * want.abs())).max())
        print(f"input_moments [{lo}, {hi}] {nm}: max|err| = {float(err.max()):.3e}, worst / (1e-6 |want|) = {worst:.2f}")
        assert worst <= 1.0
    npx, n, eps, momentum = flat.shape[0], 16, 1e-3, 0.1
    w1 = torch.randn((3, n), device=dev, generator=gen)
    beta = 0.3 * torch.randn((n,), device=dev, generator=gen)
    w2 = torch.randn((n,), device=dev, generator=gen)
    b2 = torch.full((1,), 0.2, device=dev)
    gamma = torch.ones((n,), device=dev)
    rmean, rvar = torch.zeros((n,), device=dev), torch.ones((n,), device=dev)
    conv1, _ = ops.guide_fold_batch(w1, beta, w2, b2, gamma, sums, mom, npx, eps, momentum, rmean, rvar)
    mu = s64 / npx
    cov = m64 / npx - mu[:, None] * mu[None, :]
    wd = w1.double()
    var_h = ((cov @ wd) * wd).sum(0)
    inv = gamma.double() / torch.sqrt(var_h + eps)
    want1 = torch.cat([(wd * inv).t(), (beta.double() - (mu @ wd) * inv)[:, None]], 1)
    want_rv = (1 - momentum) + momentum * var_h * npx / (npx - 1)
    for nm, got, want in (("conv1", conv1, want1), ("running_var", rvar, want_rv)):
        err = (got.double() - want).abs()
        worst = float((err / (1e-4 * want.abs())).max())
        print(f"guide_fold_batch [{lo}, {hi}] {nm}: max|err| = {float(err.max()):.3e}, worst / (1e-4 |want|) = {worst:.2f}")
        assert worst <= 1.0
