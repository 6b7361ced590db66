"""csrc/loss_psnr.hip on the MI355X: the loss, the per-image mean squared errors, the PSNR, the unit gradient and the two
state blocks (moving averages, running totals) of hdrnet_loss_psnr_f32, through metrics.loss_and_psnr / Monitor / evaluate
and through the raw C ABI, against float64 on the CPU from torch.rand inputs.

Bars.  Loss 1e-6 x want; unit gradient rtol 1e-6, atol 1e-14; scaled gradient rtol 1e-5, atol 1e-12 (the figures of
tests/test_gpu_train_fullsize.py::test_l2_loss_config_size_vs_float64); image_mse rtol 1e-6; PSNR
(10 / ln 10) x 1e-6 + one fp32 ulp of |psnr| -- what a 1e-6 relative error of an image's mean squared error does to
-10 log10, plus the store's rounding.  Every case prints max|err| and worst / bar.

Shapes: the smallest at which the partition by image can go wrong.  The first pass launches at most K_BLOCKS = 2048
workgroups of 256 float4 threads; image b of B <= 2048 owns share = 2048 // B of them (B > 2048: a workgroup walks whole
images), so one pass over an image covers share x 1024 floats:
    (1, 1, 1, 3)          three scalars, no float4 at all
    (3, 5, 7, 3)          n / B = 105: every image start misaligned differently (heads 0, 3, 2)
    (4, 64, 64, 3)        aligned, 12 float4 blocks per image
    (7, 33, 31, 3)        B does not divide the workgroup count (share 292, 2044 workgroups)
    (2049, 1, 4, 3)       more images than workgroups
    (3, 682 x 1024 + 5)   an image's workgroups make just over one pass, misaligned starts
"""
import math
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

K_BLOCKS, THREADS = 2048, 256   # csrc/loss_psnr.hip: kBlocks, kThreads
DB = -10.0 / math.log(10.0)


def share_of(B):
    return 1 if B >= K_BLOCKS else K_BLOCKS // B


def image_pass(B):
    """Floats of one image that one grid-stride pass of its workgroups covers."""
    return share_of(B) * THREADS * 4


SHAPES = [(1, 1, 1, 3), (3, 5, 7, 3), (4, 64, 64, 3), (7, 33, 31, 3), (2049, 1, 4, 3), (3, image_pass(3) + 5)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib
    return _lib.load()


_CASES = {}


def case(dev, shape):
    """(target, prediction) on the device and the float64 expectations, computed once per shape and left unchanged."""
    if shape not in _CASES:
        gen = torch.Generator(device=dev).manual_seed(len(shape) + shape[0])
        t = torch.rand(shape, device=dev, generator=gen)
        p = torch.rand(shape, device=dev, generator=gen)
        d64 = p.double().cpu() - t.double().cpu()
        mse = d64.square().reshape(shape[0], -1).mean(dim=1)
        _CASES[shape] = dict(t=t, p=p, loss=float(d64.square().mean()), mse=mse.numpy(),
                             psnr=float((DB * torch.log(mse)).mean()), unit=(2.0 / d64.numel()) * d64)
    return _CASES[shape]


def close(name, got, want, rtol, atol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want)
    ratio = err / (rtol * np.abs(want) + atol + 1e-300)
    print(f"{name}: max|err| = {float(err.max()):.3e}, worst / bar = {float(ratio.max()):.3f}")
    assert float(ratio.max()) <= 1.0, (name, float(ratio.max()))


def psnr_bar(want):
    return (10.0 / math.log(10.0)) * 1e-6 + float(np.spacing(np.float32(abs(want))))


def psnr_close(name, got, want):
    close(name, got, want, 0.0, psnr_bar(want))


def ptr(t):
    return None if t is None else t.data_ptr()


def raw(lib, p, t, grad=None, image_mse=None, ema=None, decay=0.99, totals=None, ws=None):
    """hdrnet_loss_psnr_f32 as a C caller reaches it; returns the device tensor {loss, psnr}."""
    n, B = p.numel(), p.shape[0]
    wbytes = lib.hdrnet_loss_psnr_workspace_bytes(n, B)
    if ws is None:
        ws = torch.empty((wbytes,), dtype=torch.uint8, device=p.device)
    out = torch.zeros((2,), device=p.device)
    from hdrnet_amd import _lib
    # a refused call (n = 0) leaves its text, which names the entry point; the successful call below clears it
    assert lib.hdrnet_loss_psnr_f32(p.data_ptr(), t.data_ptr(), 0, B, out.data_ptr(), out.data_ptr() + 4, None, None,
                                    None, decay, None, ws.data_ptr(), wbytes, None) == 1
    assert _lib.last_error().startswith("hdrnet_loss_psnr_f32: "), _lib.last_error()
    rc = lib.hdrnet_loss_psnr_f32(p.data_ptr(), t.data_ptr(), n, B, out.data_ptr(), out.data_ptr() + 4, ptr(image_mse),
                                  ptr(grad), ptr(ema), decay, ptr(totals), ws.data_ptr(), wbytes,
                                  torch.cuda.current_stream(p.device).cuda_stream)
    assert rc == 0, rc
    assert _lib.last_error() == ""
    return out


# ---- values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_values_through_every_backward_path_vs_float64(dev, lib, shape):
    """metrics.loss_and_psnr with the unit gradient reused, recomputed on later backwards, scaled on a first backward,
    and without a gradient; image_mse through the C ABI."""
    from hdrnet_amd import metrics
    c = case(dev, shape)
    t, p = c["t"], c["p"].clone().requires_grad_(True)
    tag = f"loss_psnr {shape} (share {share_of(shape[0])}, n / B = {p.numel() // shape[0]})"

    def values_close(what, loss, q):
        err = abs(float(loss) - c["loss"])
        print(f"{tag} {what}: loss |err| = {err:.3e}, worst / (1e-6 want) = {err / (1e-6 * c['loss']):.3f}")
        assert err <= 1e-6 * c["loss"], (what, float(loss), c["loss"])
        psnr_close(f"{tag} {what}: psnr", float(q), c["psnr"])

    loss, q = metrics.loss_and_psnr(t, p)
    assert "LossPsnr" in type(loss.grad_fn).__name__ and loss.dtype == torch.float32 and loss.dim() == 0
    assert not q.requires_grad and q.grad_fn is None and q.dim() == 0
    values_close("forward with the unit gradient", loss.detach(), q)
    g1, = torch.autograd.grad(loss, p, retain_graph=True)
    close(f"{tag} unit gradient, upstream 1", g1.double().cpu(), c["unit"], 1e-6, 1e-14)
    keep = g1.clone()
    g2, = torch.autograd.grad(loss, p, torch.tensor(-2.5, device=dev), retain_graph=True)   # hdrnet_l2_loss_grad_f32
    close(f"{tag} second backward through the retained graph, upstream -2.5", g2.double().cpu(), -2.5 * c["unit"], 1e-6, 1e-14)
    g3, = torch.autograd.grad(loss, p)
    close(f"{tag} third backward, upstream 1", g3.double().cpu(), c["unit"], 1e-6, 1e-14)
    assert torch.equal(g1, keep)
    for up in (3.5, -2.5):                                             # first backward with a scale: the scale kernel
        loss, _ = metrics.loss_and_psnr(t, p)
        g, = torch.autograd.grad(loss, p, torch.tensor(up, device=dev))
        close(f"{tag} scaled unit gradient, upstream {up}", g.double().cpu(), up * c["unit"], 1e-5, 1e-12)
    with torch.no_grad():
        plain, q0 = metrics.loss_and_psnr(t, p)
    assert plain.grad_fn is None
    values_close("forward without a gradient", plain, q0)
    mse = torch.zeros((shape[0],), device=dev)
    out = raw(lib, p.detach(), t, image_mse=mse)
    close(f"{tag} image_mse", mse.double().cpu(), c["mse"], 1e-6, 0.0)
    values_close("C ABI, no gradient", out[0], out[1])


def test_reference_modules_fixture_through_the_kernel(dev):
    """tests/golden/tf_shim/metrics.npz (hdrnet/metrics.py on the shim) at the bars of
    tests/test_tf_shim_fixtures.py::test_metrics_kernels_match_the_reference_module."""
    from hdrnet_amd import metrics
    with np.load(os.path.join(ROOT, "tests", "golden", "tf_shim", "metrics.npz")) as z:
        fx = {k: z[k] for k in z.files}
    t, p = torch.from_numpy(fx["target"]).to(dev), torch.from_numpy(fx["prediction"]).to(dev)
    loss, q = metrics.loss_and_psnr(t, p)
    mon = metrics.Monitor()
    got = mon(p, t)
    print(f"fixture: loss {float(loss)!r} psnr {float(q)!r}, want {float(fx['l2_loss'])!r} {float(fx['psnr'])!r}")
    for l, v in ((loss, q), (got, mon.psnr)):
        np.testing.assert_allclose(float(l), float(fx["l2_loss"]), rtol=2e-6)
        np.testing.assert_allclose(float(v), float(fx["psnr"]), rtol=2e-6)


# ---- planted spikes ------------------------------------------------------------------------------------------------------
def spikes_of(shape):
    """Per image: its first and last element and both sides of every pass boundary inside it (the float4 body starts
    behind the head that brings the image to a 16-byte boundary); image 1 of a batch is left without spikes."""
    B = shape[0]
    m = int(np.prod(shape[1:]))
    span = image_pass(B)
    out = []
    for b in range(B):
        if B > 1 and b == 1:
            out.append([])
            continue
        head = min((-b * m) % 4, m)
        el = {0, m - 1}
        for k in range(1, (m - head - 1) // span + 1):
            el |= {head + k * span - 1, head + k * span}
        out.append(sorted(e for e in el if 0 <= e < m))
    return m, out


@pytest.mark.parametrize("shape", SHAPES)
def test_planted_spikes_per_image(dev, lib, shape):
    """prediction == target except prediction - target = 1.0 at the spikes: S_b is the image's spike count, so image_mse
    and the loss are exact, and the unit gradient is float32(2 / n) at the spikes and 0 elsewhere -- in the forward with
    and without the gradient and in the recomputing backward.  The image without spikes reports a mean squared error of
    0, which makes the batch's PSNR +inf, and leaves the other images' values untouched."""
    from hdrnet_amd import metrics
    B = shape[0]
    m, per_image = spikes_of(shape)
    n = B * m
    if shape == SHAPES[-1]:
        assert [len(s) for s in per_image] == [4, 0, 4]     # a pass boundary inside images 0 and 2
    gen = torch.Generator(device=dev).manual_seed(3)
    t = torch.rand(shape, device=dev, generator=gen)
    idx = torch.tensor([b * m + e for b, s in enumerate(per_image) for e in s], dtype=torch.long, device=dev)
    t.view(-1)[idx] = 0.25
    p = t.clone()
    p.view(-1)[idx] = 1.25
    p.requires_grad_(True)
    want_mse = np.array([np.float32(len(s) / m) for s in per_image], dtype=np.float32)
    want_loss = np.float32(len(idx) / n)
    want_grad = torch.zeros_like(t)
    want_grad.view(-1)[idx] = float(np.float32(2.0 / n))
    loss, q = metrics.loss_and_psnr(t, p)
    g1, = torch.autograd.grad(loss, p, retain_graph=True)
    g2, = torch.autograd.grad(loss, p)
    mse = torch.full((B,), -1.0, device=dev)
    out = raw(lib, p.detach(), t, image_mse=mse)
    got_mse = mse.cpu().numpy()
    print(f"spikes {shape}: {len(idx)} spikes, loss = {float(loss)!r} / {float(out[0])!r}, want {float(want_loss)!r}; psnr = "
          f"{float(q)!r} / {float(out[1])!r}; image_mse differs in {int((got_mse != want_mse).sum())} images; gradient: "
          f"{int((g1 != want_grad).sum())} / {int((g2 != want_grad).sum())} elements differ")
    assert np.float32(float(loss)) == want_loss and np.float32(float(out[0])) == want_loss
    assert np.array_equal(got_mse, want_mse)
    assert torch.equal(g1, want_grad) and torch.equal(g2, want_grad)
    if B > 1:
        assert got_mse[1] == 0.0 and float(q) == math.inf and float(out[1]) == math.inf
    else:
        want_q = DB * math.log(float(want_mse[0]))
        psnr_close(f"spikes {shape} psnr", float(q), want_q)
        assert float(out[1]) == float(q)


# ---- poisoning -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_nothing_is_written_outside_the_outputs(dev, lib, shape):
    """The gradient, image_mse and the workspace lie inside poisoned allocations; what surrounds them stays untouched."""
    c = case(dev, shape)
    n, B = c["p"].numel(), shape[0]
    PAD, POISON = 64, 1234.5                      # 64 floats = 256 bytes: the 16-byte alignment of the bases is kept
    grad = torch.full((PAD + n + PAD,), POISON, device=dev)
    mse = torch.full((4 + B + PAD,), POISON, device=dev)
    wbytes = lib.hdrnet_loss_psnr_workspace_bytes(n, B)
    ws = torch.full((256 + wbytes + 256,), 0xA5, dtype=torch.uint8, device=dev)
    state = torch.full((4 + 3 + 4,), POISON, device=dev)
    totals = torch.full((2 + 3 + 2,), POISON, device=dev, dtype=torch.float64)
    state[4:7] = 0.0
    totals[2:5] = 0.0
    raw(lib, c["p"], c["t"], grad=grad[PAD:PAD + n], image_mse=mse[4:4 + B], ema=state[4:7], totals=totals[2:5],
        ws=ws[256:256 + wbytes])
    close(f"poison {shape} gradient", grad[PAD:PAD + n].double().cpu(), c["unit"].reshape(-1), 1e-6, 1e-14)
    close(f"poison {shape} image_mse", mse[4:4 + B].double().cpu(), c["mse"], 1e-6, 0.0)
    assert bool((grad[:PAD] == POISON).all()) and bool((grad[PAD + n:] == POISON).all())
    assert bool((mse[:4] == POISON).all()) and bool((mse[4 + B:] == POISON).all())
    assert bool((ws[:256] == 0xA5).all()) and bool((ws[256 + wbytes:] == 0xA5).all())
    assert bool((state[:4] == POISON).all()) and bool((state[7:] == POISON).all()) and float(state[6]) == 1.0
    assert bool((totals[:2] == POISON).all()) and bool((totals[5:] == POISON).all()) and float(totals[4]) == B


# ---- repeatability -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_two_calls_are_bit_equal_in_every_output(dev, lib, shape):
    c = case(dev, shape)
    n, B = c["p"].numel(), shape[0]
    runs = []
    for _ in range(2):
        grad, mse = torch.empty((n,), device=dev), torch.empty((B,), device=dev)
        state = torch.tensor([0.125, 3.0, 7.0], device=dev)
        totals = torch.tensor([10.0, 0.5, 3.0], device=dev, dtype=torch.float64)
        out = raw(lib, c["p"], c["t"], grad=grad, image_mse=mse, ema=state, totals=totals)
        runs.append((out, grad, mse, state, totals))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    print(f"repeat {shape}: loss, psnr, gradient, image_mse, ema block and totals block bit-equal")


# ---- accumulation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 5, 7, 3), (4, 64, 64, 3), (2049, 1, 4, 3)])
def test_state_blocks_accumulate_on_the_device(dev, lib, shape):
    """Three calls on three batches with both state blocks.  The EMA against s <- s - (1 - decay)(s - value) in float64,
    driven by the loss and PSNR the kernel itself stored, decay the float the C ABI carries: one fp32 rounding per step,
    k x 2^-23 x max|value| after k.  The totals against the float64 sums, in index order, of the per-image values the
    kernel reported (image_mse and -10 / ln 10 log of it), to 1e-15 relative."""
    B = shape[0]
    gen = torch.Generator(device=dev).manual_seed(11)
    decay = float(np.float32(0.99))
    state = torch.zeros((3,), device=dev)
    totals = torch.zeros((3,), device=dev, dtype=torch.float64)
    s = np.zeros(2)
    vmax = np.zeros(2)
    sums = [0.0, 0.0]
    for k in range(1, 4):
        t = torch.rand(shape, device=dev, generator=gen)
        p = t + (0.05 * k) * torch.rand(shape, device=dev, generator=gen)
        mse = torch.empty((B,), device=dev)
        out = raw(lib, p, t, image_mse=mse, ema=state, decay=0.99, totals=totals)
        value = out.double().cpu().numpy()
        s = s - (1.0 - decay) * (s - value)
        vmax = np.maximum(vmax, np.abs(value))
        got = state.double().cpu().numpy()
        bar = k * 2.0 ** -23 * vmax
        err = np.abs(got[:2] - s)
        print(f"ema {shape} step {k}: |err| = {err[0]:.3e} / {err[1]:.3e}, worst / bar = {float((err / bar).max()):.3f}")
        assert (err <= bar).all() and got[2] == k
        for v in mse.double().cpu().numpy():
            sums[0] += DB * math.log(v)
            sums[1] += v
        tot = totals.cpu().numpy()
        rel = [abs(tot[i] - sums[i]) / abs(sums[i]) for i in range(2)]
        print(f"totals {shape} step {k}: relative error psnr {rel[0]:.3e}, mse {rel[1]:.3e} (bar 1e-15)")
        assert max(rel) <= 1e-15 and tot[2] == k * B
    assert float(state[2]) == 3.0


# ---- capture -------------------------------------------------------------------------------------------------------------
def test_monitor_in_a_captured_training_step(dev):
    """GraphedTrainStep with a Monitor as loss_fn at the small extents of tests/test_models.py's graph tests, lr = 0:
    five replays count five updates, every replay stores the same loss, the moving average is where five updates from 0
    put it, and the graph's loss and flat gradient bucket are bit-equal to an eager TrainStep twin's with its own
    Monitor; the bucket against a twin on metrics.l2_loss at the unit-gradient bar."""
    from hdrnet_amd import metrics, models, optim
    from hdrnet_amd.runtime import GraphedTrainStep, TrainStep
    gen = torch.Generator(device=dev).manual_seed(9)
    low = torch.rand(2, 256, 256, 3, device=dev, generator=gen)
    full = torch.rand(2, 136, 240, 3, device=dev, generator=gen)
    tgt = torch.rand(2, 136, 240, 3, device=dev, generator=gen)
    torch.manual_seed(12)
    state = {k: v.clone() for k, v in models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).to(dev).state_dict().items()}

    def twin():
        m = models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).to(dev).train()
        m.load_state_dict(state)
        return m, optim.FlatAdam([p for p in m.parameters() if p.requires_grad], lr=0.0)

    (mg, og), (me, oe), (ml, ol) = twin(), twin(), twin()
    mon_g, mon_e = metrics.Monitor(decay=0.99), metrics.Monitor(decay=0.99)
    step = GraphedTrainStep(mg, mon_g, og, [low, full], [tgt], warmup=2)
    assert float(mon_g.updates) >= 2.0          # the warm-up passes ran the kernels on this state
    mon_g.reset()
    eager = TrainStep(me, mon_e, oe)
    plain = TrainStep(ml, lambda out, t: metrics.l2_loss(t, out), ol)
    losses = []
    for k in range(5):
        lg = step([low, full], [tgt])
        assert lg.data_ptr() == mon_g.loss.data_ptr()
        losses.append(float(lg))
    le = eager([low, full], [tgt])
    ll = plain([low, full], [tgt])
    r = mon_g.read()
    print(f"captured Monitor: losses {losses}, eager {float(le)!r}, l2_loss {float(ll)!r}; read() = {r}")
    assert r["updates"] == 5 and len(set(losses)) == 1 and r["loss"] == losses[0]
    want = losses[0] * (1.0 - 0.99 ** 5)
    bar = 5 * 2.0 ** -23 * abs(losses[0])
    print(f"captured Monitor: ema_loss |err| = {abs(r['ema_loss'] - want):.3e}, worst / bar = {abs(r['ema_loss'] - want) / bar:.3f}")
    assert abs(r["ema_loss"] - want) <= bar
    qbar = 5 * 2.0 ** -23 * abs(r["psnr"])
    assert abs(r["ema_psnr"] - r["psnr"] * (1.0 - 0.99 ** 5)) <= qbar
    np.testing.assert_allclose(r["ema_loss_debiased"], r["ema_loss"] / (1.0 - mon_g.decay ** 5), rtol=1e-15)
    assert step.bucket.attached()
    assert float(le) == losses[0] and torch.equal(step.bucket.flat, eager.bucket.flat)
    assert mon_e.read()["updates"] == 1 and mon_e.read()["psnr"] == r["psnr"]
    close("captured Monitor: flat gradient bucket vs the l2_loss twin", step.bucket.flat.double().cpu(),
          plain.bucket.flat.double().cpu(), 1e-6, 1e-14)
    assert abs(float(ll) - losses[0]) <= 1e-6 * abs(float(ll))


# ---- evaluation ----------------------------------------------------------------------------------------------------------
class SecondInput(torch.nn.Module):
    def forward(self, low, full):
        return full


@pytest.mark.parametrize("ragged", [False, True])
def test_evaluate_on_a_device_dataset(dev, ragged):
    """Five small u8 pairs, the model returning its full-resolution input: the mean PSNR at batch = 1 and batch = 2 is the
    same number, bit for bit (per-image sums that do not depend on the batch at these sizes, added image by image in
    order), within the PSNR bar of the float64 value of the prepared fp32 samples."""
    from hdrnet_amd import data, metrics
    gen = torch.Generator().manual_seed(21)
    sizes = [(24, 32), (30, 36), (24, 40), (26, 32), (40, 33)] if ragged else [(24, 32)] * 5
    ins = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen) for h, w in sizes]
    tgs = [(a.int() + torch.randint(-9 * (i + 1), 9 * (i + 1), a.shape, generator=gen)).clamp(0, 255).to(torch.uint8)
           for i, a in enumerate(ins)]
    kw = dict(output_resolution=(24, 32), net_input_size=16, fliplr=False, flipud=False, rotate=False, random_crop=False)

    def make(**over):
        k = dict(kw, order="sequential")
        k.update(over)
        if ragged:
            return data.DeviceDataset.from_images(ins, tgs, device=dev, **k)
        return data.DeviceDataset(torch.stack(ins).to(dev), torch.stack(tgs).to(dev), **k)

    _, full, target = make().next_batch(5)
    mse = (full.double().cpu() - target.double().cpu()).square().reshape(5, -1).mean(dim=1)
    want = float((DB * torch.log(mse)).mean())
    model = SecondInput().to(dev).train()
    got = [metrics.evaluate(model, make(), batch=b) for b in (1, 2, 5)]
    assert model.training
    print(f"evaluate ragged={ragged}: {got!r}, float64 {want!r}")
    psnr_close(f"evaluate ragged={ragged}", got[0], want)
    assert got[0] == got[1] == got[2]
    for over in (dict(order="epoch"), dict(fliplr=True), dict(rotate="even"), dict(random_crop=True)):
        with pytest.raises(ValueError):
            metrics.evaluate(model, make(**over))
