"""The rest of config #4's training step -- the l2 loss, the pyramid's up-add and its transpose, Adam over the flat
buffer, and the step as a whole -- at 4 x 1080p against float64, where the grid-stride loops make several passes and the
float32 coordinate arithmetic is in another regime than at the toy sizes of test_models.py.

A. l2_loss_partial / l2_loss_grad / l2_loss_grad_scale launch kLossBlocks = 2048 workgroups of 256 float4 threads: one
   pass covers 2 097 152 floats, 4 x 1080p takes 12.  Values against float64 at the bars of test_models.py; planted
   unit spikes on both sides of every pass boundary, exact.
B. resize_add_ac / resize_bilinear_grad_ac at the pyramid's extents against oracle/f64_train.py (float32 coordinates,
   float64 sums -- torch's float64 interpolate forms the coordinate in float64 and is 2.8e-4 away at 960 -> 1920), at the
   bars of test_models.py::test_upsample_add_and_its_vjp_vs_torch_float64.  (16 x 16 and 1 x 2 -> 1080 x 1920 sum 37 k
   and 2 M terms per source pixel: a plain float32 running sum missed d coarse's bar 3.4 x and 12.6 x there, hence the
   compensated sum of the kernel's uncached branch.)
C. adam_flat (at most 4096 x 256 float4: 4 194 304 floats per pass) with the benchmark's hyper-parameters, both epsilon
   placements, from zero state and resumed at step 20 000, against oracle/f64_train.adam_step in float64:
   1. the slots, elementwise, each step.  One step (the float64 formula on the kernel's own previous slots): exp_avg_sq
      within rtol 1e-6 + one denormal ulp (1e-20 gradients put it among the denormals, where one step rounds twice);
      exp_avg within 1e-6 of the sum of its two terms' magnitudes + one denormal ulp -- that is rtol 1e-6 of exp_avg
      itself wherever the terms share a sign, and the only scale a float32 sum of terms of both signs can be held to:
      relative to the cancelled sum the float32 numpy restatement of the formula is itself beyond 1e-6 on 0.6 - 0.75 %
      of the elements of a randn stream (the kernel: 0.5 - 0.6 %; both counts printed).  Chained from the seeded state:
      k steps within the same rtol and k denormal ulps (on the denormal grid each step adds up to one ulp), exp_avg's
      scale being the same moving average taken over |g|.
   2. the parameters at rtol 1e-5, atol 1e-7.
   3. the update p_before - p_after: its distance from the float64 update, in units of the update the element would
      take had its gradients not cancelled (lr_t x moving average of |g| / denominator), at most 2 x the largest such
      distance of the float32 numpy restatement, plus half a float32 ulp of the parameter (the kernel's own store).
      Measured on MI355X, worst step of every case: restatement 3.7e-6 .. 3.8e-6, kernel 3.6e-6 .. 3.7e-6 -- at
      t = 2 .. 9, where 1 - 0.999^t cancels in float32 for both (numpy: up to 6.7e-6 relative on the correction, half
      of it on the update); at t = 1 and t = 10 restatement 2.9e-7 / 5.9e-7, kernel 2.6e-7 / 4.5e-7.
   4. the device-side step count.  5. poisoned elements beyond n untouched (raw C ABI).
D. The model's step: fused against composed at low (4, 256, 256, 3), full (4, 1080, 1920, 3) at the bars of
   test_training_fused_guide_matches_unfused_module / test_pyramid_training_fused_matches_composed; the captured graph
   with FlatAdam(epsilon_hat=True) as bench.py runs it against an eager twin (lr = 0: the same gradients every step),
   and at lr = 1e-4 the update inside the graph and the step count under replay against C's float64 restatement driven
   with the gradients the graph left in the bucket.
   Measured: no bar touched.  Worst parameter gradient / bar 0.009 (batch_norm=False), 0.065 (True), 0.022 (pyramid); the
   graph and the eager twin bit-equal in the loss and the whole flat bucket, every replay, both forms; the update under
   replay: restatement 3.16e-6, kernel 3.17e-6.

Every case prints max|err| and worst / bar.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import f64_train  # noqa: E402

# csrc/metrics.hip: l2_loss_* launch kLossBlocks = 2048 workgroups x 256 threads x one float4 per thread and pass
L2_PASS = 2048 * 256 * 4
# csrc/metrics.hip, adam_step: at most 4096 workgroups x 256 threads x one float4
ADAM_PASS = 4096 * 256 * 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from hdrnet_amd import hdrnet_ops
    return hdrnet_ops


def close(name, got, want, rtol, atol, scale=None):
    """|got - want| <= rtol x |want| (or x scale) + atol elementwise, numpy or torch float64; prints the worst case."""
    if isinstance(got, float):
        got, want = np.float64(got), np.float64(want)
    err = abs(got - want)
    bar = rtol * abs(want if scale is None else scale) + atol
    ratio = err / (bar + 1e-300)
    worst = float(ratio.max())
    print(f"{name}: max|err| = {float(err.max()):.3e}, worst / bar = {worst:.3f}")
    assert worst <= 1.0, (name, worst)
    return worst


# ---- A. l2 loss ------------------------------------------------------------------------------------------------------
L2_SHAPES = [(4, 1080, 1920, 3), (1, 2159, 3839, 3), (L2_PASS + 5,)]


@pytest.mark.parametrize("shape", L2_SHAPES)
def test_l2_loss_config_size_vs_float64(dev, shape):
    """metrics.l2_loss through all four entry points at 12 passes, at 12 passes with a three-element tail, and just over
    one pass, against mean(square(t - p)) and (2 / n)(p - t) in float64 on the CPU."""
    from hdrnet_amd import metrics
    gen = torch.Generator(device=dev).manual_seed(len(shape) + shape[0])
    t = torch.rand(shape, device=dev, generator=gen)
    p = torch.rand(shape, device=dev, generator=gen).requires_grad_(True)
    n = p.numel()
    assert n > L2_PASS
    d64 = p.detach().double().cpu() - t.double().cpu()
    want = float(d64.square().mean())
    dwant = (2.0 / n) * d64
    tag = f"l2_loss {shape} ({n / L2_PASS:.2f} passes, n & 3 = {n & 3})"

    def loss_close(what, loss):
        err = abs(float(loss) - want)
        print(f"{tag} {what}: loss |err| = {err:.3e}, worst / (1e-6 want) = {err / (1e-6 * want):.3f}")
        assert err <= 1e-6 * want, (what, float(loss), want)

    def grad_close(what, g, up, rtol, atol):
        close(f"{tag} {what}", g.double().cpu(), up * dwant, rtol, atol)

    loss = metrics.l2_loss(t, p)
    assert "L2Loss" in type(loss.grad_fn).__name__
    loss_close("forward with the unit gradient", loss)
    g1, = torch.autograd.grad(loss, p, retain_graph=True)          # the forward's unit gradient, grad_output = 1
    grad_close("unit gradient, upstream 1", g1, 1.0, 1e-6, 1e-14)
    keep = g1.clone()
    g2, = torch.autograd.grad(loss, p, torch.tensor(-2.5, device=dev), retain_graph=True)   # hdrnet_l2_loss_grad_f32
    grad_close("second backward through the retained graph, upstream -2.5", g2, -2.5, 1e-6, 1e-14)
    g3, = torch.autograd.grad(loss, p)                              # and once more with 1
    grad_close("third backward, upstream 1", g3, 1.0, 1e-6, 1e-14)
    assert torch.equal(g1, keep)                                    # the first result was not scaled again
    print(f"{tag}: recomputed gradient bit-equal to the forward's unit gradient: {torch.equal(g3, g1)}")
    for up in (3.5, -2.5):                                          # first backward with a scale: the scale kernel
        loss = metrics.l2_loss(t, p)
        g, = torch.autograd.grad(loss, p, torch.tensor(up, device=dev))
        grad_close(f"scaled unit gradient, upstream {up}", g, up, 1e-5, 1e-12)
    with torch.no_grad():
        plain = metrics.l2_loss(t, p)
    assert plain.grad_fn is None
    loss_close("forward without a gradient", plain)


def spike_elements(n, span):
    """0, n - 1 and both sides of every pass boundary."""
    el = {0, n - 1}
    for k in range(1, (n - 1) // span + 1):
        el |= {k * span - 1, k * span}
    return torch.tensor(sorted(e for e in el if e < n), dtype=torch.long)


@pytest.mark.parametrize("shape", L2_SHAPES)
def test_l2_loss_planted_spikes(dev, shape):
    """prediction == target except prediction - target = 1.0 at element 0, n - 1 and k L2_PASS - 1, k L2_PASS: the sum of
    squares is the spike count, so the loss is float32(count / n) and the unit gradient float32(2 / n) at the spikes
    and 0 elsewhere, exactly -- in the forward with and without the gradient and in the recomputing backward."""
    from hdrnet_amd import metrics
    gen = torch.Generator(device=dev).manual_seed(3)
    t = torch.rand(shape, device=dev, generator=gen)
    n = t.numel()
    idx = spike_elements(n, L2_PASS).to(dev)
    assert len(idx) == 2 * ((n - 1) // L2_PASS) + 2
    t.view(-1)[idx] = 0.25
    p = t.clone()
    p.view(-1)[idx] = 1.25
    p.requires_grad_(True)
    want_loss = np.float32(len(idx) / n)
    want_grad = torch.zeros_like(t)
    want_grad.view(-1)[idx] = float(np.float32(2.0 / n))
    loss = metrics.l2_loss(t, p)
    g1, = torch.autograd.grad(loss, p, retain_graph=True)
    g2, = torch.autograd.grad(loss, p)                              # recomputed by hdrnet_l2_loss_grad_f32
    with torch.no_grad():
        plain = metrics.l2_loss(t, p)
    print(f"l2 spikes {shape}: {len(idx)} spikes, loss = {float(loss)!r} / {float(plain)!r}, want {float(want_loss)!r}; "
          f"gradient: {int((g1 != want_grad).sum())} / {int((g2 != want_grad).sum())} elements differ")
    assert np.float32(float(loss)) == want_loss and np.float32(float(plain)) == want_loss
    assert torch.equal(g1, want_grad) and torch.equal(g2, want_grad)


# ---- B. up-add and its transpose -------------------------------------------------------------------------------------
UPADD_SHAPES = [
    (4, 270, 480, 540, 960, 3), (4, 540, 960, 1080, 1920, 3),      # the training levels of config #4
    (1, 1080, 1920, 2160, 3840, 3),
    (2, 270, 480, 1080, 1920, 3), (2, 539, 959, 1080, 1920, 3), (1, 16, 16, 1080, 1920, 3),   # windows wider than kW
    (1, 1, 2, 1080, 1920, 3),                                       # one source row: the reciprocal scale is 3e38
    (2, 1080, 1920, 270, 480, 3),                                   # down-sampling
    (1, 1080, 1920, 1080, 1920, 3),                                 # equal sizes
    (1, 540, 960, 1080, 1920, 1), (1, 540, 960, 1080, 1920, 5),     # the dynamic kernel; C = 5: two channel rounds
]


@pytest.mark.parametrize("shape", UPADD_SHAPES)
def test_upsample_add_and_its_vjp_at_pyramid_sizes(dev, ops, shape):
    """Forward within 1e-5, d coarse within 2e-6 max|want| + 1e-6 of the float64 sums over the float32 taps; d fine
    bit-equal to the incoming gradient; a second backward bit-equal to the first."""
    B, ih, iw, oh, ow, C = shape
    gen = torch.Generator(device=dev).manual_seed(sum(shape))
    coarse = torch.randn((B, ih, iw, C), device=dev, generator=gen).requires_grad_(True)
    fine = torch.randn((B, oh, ow, C), device=dev, generator=gen).requires_grad_(True)
    w = torch.randn((B, oh, ow, C), device=dev, generator=gen)
    out = ops.upsample_add(coarse, fine)
    (out * w).sum().backward()
    want = f64_train.upsample_add_f64(coarse.detach().cpu().numpy(), fine.detach().cpu().numpy())
    close(f"upsample_add {shape} forward", out.detach().cpu().numpy().astype(np.float64), want, 0.0, 1e-5)
    del want
    assert torch.equal(fine.grad, w)
    dwant = f64_train.upsample_vjp_f64(w.cpu().numpy(), ih, iw)
    scale = float(np.abs(dwant).max())
    close(f"upsample_add {shape} d coarse (max|want| = {scale:.3g})", coarse.grad.cpu().numpy().astype(np.float64), dwant,
          0.0, 2e-6 * scale + 1e-6)
    g1 = coarse.grad.clone()
    coarse.grad = None
    (ops.upsample_add(coarse, fine.detach()) * w).sum().backward()
    assert torch.equal(coarse.grad, g1)


@pytest.mark.parametrize("shape", UPADD_SHAPES)
def test_upsample_vjp_planted_spikes(dev, ops, shape):
    """The incoming gradient zero except 1.0 at the four corners and at the 3 x 3 destination pixels around the middle
    row and column: d coarse is the corresponding entries of Wy^T G Wx, evaluated in float32 from the float32 lerps
    (products of at most two float32 factors, a few of them summed), within 2e-6 max|want| + 1e-6 -- and exactly zero
    wherever no spike has a tap."""
    B, ih, iw, oh, ow, C = shape
    rows = sorted({0, oh - 1} | {min(max(oh // 2 + d, 0), oh - 1) for d in (-1, 0, 1)})
    cols = sorted({0, ow - 1} | {min(max(ow // 2 + d, 0), ow - 1) for d in (-1, 0, 1)})
    G = np.zeros((B, oh, ow, C), np.float32)
    for y in rows:
        for x in cols:
            if (y in (0, oh - 1)) == (x in (0, ow - 1)):  # corners, and the block in the middle
                G[:, y, x, :] = 1.0
    want = f64_train.upsample_vjp_f64(G, ih, iw, dtype=np.float32)
    assert want.dtype == np.float32
    np.testing.assert_allclose(want.sum(), G.sum(), rtol=1e-5)  # every row of the tap matrices sums to one
    coarse = torch.zeros((B, ih, iw, C), device=dev, requires_grad=True)
    fine = torch.zeros((B, oh, ow, C), device=dev)
    ops.upsample_add(coarse, fine).backward(torch.from_numpy(G).to(dev))
    got = coarse.grad.cpu().numpy()
    scale = float(np.abs(want).max())
    close(f"upsample spikes {shape} ({int(G[0, :, :, 0].sum())} spikes, {int((want[0, :, :, 0] != 0).sum())} source "
          f"pixels touched) d coarse", got.astype(np.float64), want.astype(np.float64), 0.0, 2e-6 * scale + 1e-6)
    assert not got[want == 0].any()


# ---- C. Adam over a flat buffer --------------------------------------------------------------------------------------
HYPER = dict(lr=1e-4, b1=0.9, b2=0.999, eps=1e-8)   # bench.py's: lr 1e-4, FlatAdam's default betas and eps
DENORMAL = 2.0 ** -149


def grad_stream(dev, n, k, seed):
    """Step k of a float32 gradient stream: randn x 1e-2; exact zeros (1 % of the elements on this step only, every
    11th on every step) and 1e-20 entries (every 13th)."""
    gen = torch.Generator(device=dev).manual_seed(seed * 1000 + k)
    g = torch.randn((n,), device=dev, generator=gen) * 1e-2
    g[torch.rand((n,), device=dev, generator=gen) < 0.01] = 0.0
    i = torch.arange(n, device=dev)
    g[i % 11 == 3] = 0.0
    g[i % 13 == 5] = 1e-20
    return g


def resumed_state(dev, n, seed):
    """Non-zero Adam slots of a run 20 000 steps old."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    m = torch.randn((n,), device=dev, generator=gen) * 3e-3
    v = (torch.randn((n,), device=dev, generator=gen) * 1e-2).square()
    i = torch.arange(n, device=dev)
    m[i % 11 == 3] = 0.0
    v[i % 11 == 3] = 0.0
    return m, v, 20000.0


class AdamRef:
    """The float64 restatement (oracle/f64_train.adam_step) and its float32 numpy form, stepped beside the kernel from
    the same state with the same float32 gradients; check() applies C.1 - C.3 to the kernel's state after a step."""

    CALIBRATION = 65536

    def __init__(self, p, m, v, t, epsilon_hat):
        p, m, v = (a.cpu().numpy().copy() for a in (p, m, v))
        # The yardstick of C.3 is the LARGEST distance of the float32 restatement, and the largest of n rounding errors
        # grows with n: over the 1..7 elements of the short buffers it says little about the arithmetic.  The two
        # restatements therefore carry extra elements of the same stream (which the kernel never sees), so that the
        # yardstick is taken over at least 65 536.
        self.n = len(p)
        extra = max(0, self.CALIBRATION - self.n)
        self.rng = np.random.default_rng(self.n)
        if extra:
            r = lambda scale: (self.rng.standard_normal(extra) * scale).astype(np.float32)  # noqa: E731
            fresh = not m.any() and not v.any()
            p = np.concatenate([p, r(1e-3)])
            m = np.concatenate([m, r(0.0 if fresh else 3e-3)])
            v = np.concatenate([v, r(0.0 if fresh else 1e-2) ** 2])
        self.extra = extra
        self.p, self.m, self.v = (a.astype(np.float64) for a in (p, m, v))
        self.p32, self.m32, self.v32 = p, m, v
        self.t, self.s, self.eh = int(t), None, bool(epsilon_hat)
        self.k = 0  # steps since the chain was seeded
        self.worst = dict(d32=0.0, dk=0.0)

    def check(self, tag, g, before, after):
        """before / after: the kernel's (p, m, v) around its step with gradient g."""
        g, pb, mb, vb, pa, ma, va = (a.cpu().numpy() for a in (g, *before, *after))
        self.t += 1
        self.k += 1
        n = self.n
        h = (HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], self.eh)
        gx = np.concatenate([g, (self.rng.standard_normal(self.extra) * 1e-2).astype(np.float32)]) if self.extra else g
        self.p, self.m, self.v, updx, self.s, unitx = f64_train.adam_step(self.p, self.m, self.v, gx, self.t, *h, s=self.s)
        self.p32, self.m32, self.v32, upd32, _, _ = f64_train.adam_step(self.p32, self.m32, self.v32, gx, self.t, *h,
                                                                         dtype=np.float32)
        upd, unit = updx[:n], unitx[:n]
        tag = f"{tag} t={self.t}"
        # 1. the slots: this step alone (the float64 formula on the kernel's own previous slots), then the chain
        _, m1, v1, _, s1, _ = f64_train.adam_step(pb.astype(np.float64), mb.astype(np.float64), vb.astype(np.float64), g,
                                                  self.t, *h)
        ma, va = ma.astype(np.float64), va.astype(np.float64)
        close(f"{tag} exp_avg_sq, one step", va, v1, 1e-6, DENORMAL)
        close(f"{tag} exp_avg, one step (rtol of the terms' magnitudes)", ma, m1, 1e-6, DENORMAL, scale=s1)
        close(f"{tag} exp_avg_sq, {self.k} steps chained ({self.k} denormal ulps)", va, self.v[:n], 1e-6, self.k * DENORMAL)
        close(f"{tag} exp_avg, {self.k} steps chained ({self.k} denormal ulps)", ma, self.m[:n], 1e-6, self.k * DENORMAL,
              scale=self.s[:n])
        lit = 1e-6 * np.abs(m1) + DENORMAL
        print(f"{tag} exp_avg beyond rtol 1e-6 of the cancelled sum, one step: kernel {int((np.abs(ma - m1) > lit).sum())}, "
              f"float32 numpy restatement "
              f"{int((np.abs(f64_train.adam_step(pb, mb, vb, g, self.t, *h, dtype=np.float32)[1] - m1) > lit).sum())} "
              f"of {len(lit)} elements")
        # 2. the parameters
        close(f"{tag} parameters", pa.astype(np.float64), self.p[:n], 1e-5, 1e-7)
        # 3. the update
        onx = unitx > 0
        d32 = float((np.abs(upd32 - updx)[onx] / unitx[onx]).max()) if onx.any() else 0.0
        on = unit > 0
        err = np.abs((pb.astype(np.float64) - pa.astype(np.float64)) - upd)
        half_ulp = 0.5 * np.spacing(np.maximum(np.abs(pb), np.abs(pa))).astype(np.float64)
        dk = float((np.maximum(err - half_ulp, 0.0)[on] / unit[on]).max()) if on.any() else 0.0
        worst = float((err / (2.0 * d32 * unit + half_ulp)).max())
        print(f"{tag} update: float32 numpy restatement {d32:.3e}, kernel {dk:.3e} beyond half an ulp of the parameter "
              f"(both / the uncancelled update); worst / (2 x restatement + ulp / 2) = {worst:.3f}")
        assert worst <= 1.0, (tag, worst)
        self.worst["d32"] = max(self.worst["d32"], d32)
        self.worst["dk"] = max(self.worst["dk"], dk)


class RawAdam:
    """hdrnet_adam_step_f32 / hdrnet_adam_step_tf_f32 on buffers of n + 64 floats, the last 64 poisoned."""
    PAD, POISON = 64, 7.25

    def __init__(self, dev, n, epsilon_hat, seed):
        from hdrnet_amd import _lib
        self.lib, self.dev, self.n, self.eh = _lib.load(), dev, n, epsilon_hat
        gen = torch.Generator(device=dev).manual_seed(seed)
        self.p = torch.full((n + self.PAD,), self.POISON, device=dev)
        self.p[:n] = torch.randn((n,), device=dev, generator=gen) * 1e-3   # small: an ulp of p must not hide the update
        self.p[:n][torch.arange(n, device=dev) % 5 == 1] = 0.0
        self.m = torch.full((n + self.PAD,), self.POISON, device=dev)
        self.v = torch.full((n + self.PAD,), self.POISON, device=dev)
        self.m[:n] = 0.0
        self.v[:n] = 0.0
        self.g = torch.full((n + self.PAD,), 1.0, device=dev)
        self.steps = torch.zeros((1,), device=dev)
        # a refused call (n = 0) leaves its text, which names the entry point; the first successful step clears it
        fn = self.lib.hdrnet_adam_step_tf_f32 if self.eh else self.lib.hdrnet_adam_step_f32
        assert fn(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), ctypes.c_longlong(0),
                  self.steps.data_ptr(), HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], None) == 1
        assert _lib.last_error().startswith(fn.__name__ + ": "), _lib.last_error()

    def step(self, g):
        self.g[:self.n] = g
        fn = self.lib.hdrnet_adam_step_tf_f32 if self.eh else self.lib.hdrnet_adam_step_f32
        from hdrnet_amd import _lib
        with torch.cuda.device(self.dev):
            rc = fn(self.p.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), ctypes.c_longlong(self.n),
                    self.steps.data_ptr(), HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"],
                    torch.cuda.current_stream(self.dev).cuda_stream)
        assert rc == 0, rc
        assert _lib.last_error() == ""
        torch.cuda.synchronize()

    def poison_intact(self):
        return all(bool((a[self.n:] == self.POISON).all()) for a in (self.p, self.m, self.v))


def run_adam(tag, n, steps, take_step, state, ref):
    """`steps` kernel steps, each checked against `ref`; state() -> (p, m, v) tensors of n elements."""
    for k in range(steps):
        g = take_step.grad(k)
        before = [a.clone() for a in state()]
        take_step(g)
        ref.check(tag, g, before, state())
    return ref.worst


ADAM_LENGTHS = [3 * ADAM_PASS + r for r in range(4)] + list(range(1, 8))


@pytest.mark.parametrize("epsilon_hat", [False, True])
@pytest.mark.parametrize("n", ADAM_LENGTHS)
def test_adam_flat_raw_lengths_vs_float64(dev, n, epsilon_hat):
    """The C entry points at several passes plus every tail and at n = 1..7: ten steps from zero state, every one
    checked (1, 2 and 10 among them), then two steps resumed at 20 000, where both float32 bias corrections are 1."""
    seed = n % 1000 + int(epsilon_hat)
    tag = f"adam_flat n={n} ({n / ADAM_PASS:.2f} passes, n & 3 = {n & 3}) {'tensorflow' if epsilon_hat else 'torch'} eps"
    a = RawAdam(dev, n, epsilon_hat, seed)

    def take(g):
        a.step(g)
    take.grad = lambda k: grad_stream(dev, n, k, seed)
    state = lambda: (a.p[:n], a.m[:n], a.v[:n])  # noqa: E731
    w = run_adam(tag, n, 10, take, state, AdamRef(a.p[:n], a.m[:n], a.v[:n], 0, epsilon_hat))
    assert float(a.steps) == 10.0 and a.poison_intact()
    f32 = np.float32
    assert f32(1) - f32(HYPER["b1"]) ** f32(20001) == 1 and f32(1) - f32(HYPER["b2"]) ** f32(20001) == 1
    m, v, t = resumed_state(dev, n, seed + 1)
    a.m[:n], a.v[:n] = m, v
    a.steps.fill_(t)
    take.grad = lambda k: grad_stream(dev, n, 100 + k, seed)
    w2 = run_adam(tag + " resumed", n, 2, take, state, AdamRef(a.p[:n], a.m[:n], a.v[:n], t, epsilon_hat))
    assert float(a.steps) == t + 2 and a.poison_intact()
    print(f"{tag}: update distance / uncancelled update, worst step: float32 numpy restatement "
          f"{max(w['d32'], w2['d32']):.3e}, kernel {max(w['dk'], w2['dk']):.3e}")


@pytest.mark.parametrize("epsilon_hat", [False, True])
@pytest.mark.parametrize("cm", [1, 2])
@pytest.mark.parametrize("cls", ["HDRNetCurves", "HDRNetPointwiseNNGuide", "HDRNetGaussianPyrNN"])
def test_flat_adam_on_the_models_flat_buffers_vs_float64(dev, cls, cm, epsilon_hat):
    """optim.FlatAdam over the real flat buffers of the three models (default parameters and channel_multiplier = 2),
    constructed as bench.py constructs it: ten steps from zero state, then a state of 20 000 steps loaded through
    load_state_dict and two more."""
    from hdrnet_amd import models, optim
    torch.manual_seed(cm)
    model = getattr(models, cls)(dict(channel_multiplier=cm)).to(dev).train()
    opt = optim.FlatAdam([p for p in model.parameters() if p.requires_grad], lr=HYPER["lr"], epsilon_hat=epsilon_hat)
    assert opt.betas == (HYPER["b1"], HYPER["b2"]) and opt.eps == HYPER["eps"]
    n = opt.flat.numel()
    seed = n % 1000 + int(epsilon_hat)
    tag = f"FlatAdam {cls} x{cm} n={n} (n & 3 = {n & 3}) {'tensorflow' if epsilon_hat else 'torch'} eps"

    def take(g):
        opt.bucket.flat.copy_(g)
        opt.step()
        torch.cuda.synchronize()
    take.grad = lambda k: grad_stream(dev, n, k, seed)
    state = lambda: (opt.flat, opt.exp_avg, opt.exp_avg_sq)  # noqa: E731
    w = run_adam(tag, n, 10, take, state, AdamRef(opt.flat, opt.exp_avg, opt.exp_avg_sq, 0, epsilon_hat))
    assert float(opt.steps) == 10.0
    sd = opt.state_dict()
    sd["exp_avg"], sd["exp_avg_sq"], t = resumed_state(dev, n, seed + 1)
    sd["steps"] = torch.full((1,), t, device=dev)
    opt.load_state_dict(sd)
    assert float(opt.steps) == t
    take.grad = lambda k: grad_stream(dev, n, 100 + k, seed)
    w2 = run_adam(tag + " resumed", n, 2, take, state, AdamRef(opt.flat, opt.exp_avg, opt.exp_avg_sq, t, epsilon_hat))
    assert float(opt.steps) == t + 2
    print(f"{tag}: update distance / uncancelled update, worst step: float32 numpy restatement "
          f"{max(w['d32'], w2['d32']):.3e}, kernel {max(w['dk'], w2['dk']):.3e}")


# ---- D. the whole step -----------------------------------------------------------------------------------------------
def config4_batch(dev, seed):
    gen = torch.Generator(device=dev).manual_seed(seed)
    return (torch.rand((4, 256, 256, 3), device=dev, generator=gen), torch.rand((4, 1080, 1920, 3), device=dev, generator=gen),
            torch.rand((4, 1080, 1920, 3), device=dev, generator=gen))


def grads_close(tag, named, rel):
    """Every (name, got, ref): max|got - ref| <= rel x max|ref| + 1e-7; all of them printed before the assertion."""
    bad, equal = [], 0
    for name, a, b in named:
        scale = float(b.abs().max())
        err = float((a - b).abs().max())
        worst = err / (rel * scale + 1e-7)
        equal += int(torch.equal(a, b))
        print(f"{tag} {name}: max|err| = {err:.3e}, max|ref| = {scale:.3e}, worst / bar = {worst:.3f}")
        if not worst <= 1.0:
            bad.append((name, err, scale))
    print(f"{tag}: {equal} of {len(named)} tensors bit-equal")
    assert not bad, bad
    return equal == len(named)


def backward_kernels(ops, root):
    """Hooks on every node of `root`'s autograd graph that belongs to a native autograd.Function (hdrnet_ops): after the
    node's backward has run, (node name, ops.last_kernel()) is appended to the returned list."""
    ran, seen, todo = [], set(), [root.grad_fn]
    while todo:
        node = todo.pop()
        if node is None or node in seen:
            continue
        seen.add(node)
        name = type(node).__name__
        if name.startswith("_") and name.endswith("Backward"):
            node.register_hook(lambda gi, go, name=name: ran.append((name, ops.last_kernel())))
        todo += [nxt for nxt, _ in node.next_functions]
    return ran


@pytest.mark.parametrize("cls,bn", [("HDRNetPointwiseNNGuide", False), ("HDRNetPointwiseNNGuide", True),
                                    ("HDRNetGaussianPyrNN", False)])
def test_training_fused_matches_composed_4x1080p(dev, ops, cls, bn):
    """test_training_fused_guide_matches_unfused_module / test_pyramid_training_fused_matches_composed at config #4's
    batch: loss, every parameter gradient, the batch-norm running statistics, at those tests' own bars."""
    from hdrnet_amd import models
    pyramid = cls == "HDRNetGaussianPyrNN"
    torch.manual_seed(9 if pyramid else 2)
    m = getattr(models, cls)(dict(batch_norm=bn)).to(dev).train()
    ref = getattr(models, cls)(dict(batch_norm=bn)).to(dev).train()
    ref.load_state_dict(m.state_dict())
    ref.fuse_guide = False
    low, full, target = config4_batch(dev, 21)
    loss = (m(low, full) - target).square().mean()
    assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide", ops.last_kernel()
    ran = backward_kernels(ops, loss)
    loss.backward()
    after_bwd = ops.last_kernel()
    loss_ref = (ref(low, full) - target).square().mean()
    composed = ops.last_kernel()
    loss_ref.backward()
    tag = f"{cls} batch_norm={bn} 4 x 1080p fused vs composed"
    print(f"{tag}: kernels after each native backward node: {ran}; at the end: {after_bwd}; composed forward: {composed}")
    assert "nnguide" not in composed, composed
    levels = 3 if pyramid else 1
    # the fused op's backward ends with the guide network's VJP kernel, once per level; the up-add's two kernels carry no
    # label of their own, so its node leaves the name of whatever ran before it
    assert [k for node, k in ran if node == "_BilateralSliceApplyNNGuideBackward"] == ["guide_nn_grad"] * levels, ran
    assert [node for node, _ in ran].count("_UpsampleAddBackward") == levels - 1, ran
    assert [k for node, k in ran if node == "_GuideFoldBatchBackward"] == ["guide_fold_batch_grad"] * levels, ran
    # the native coefficient network trains without batch norm only; its backward is the step's last native node
    assert [(node, k) for node, k in ran if node == "_CoefficientsTrainBackward"] == \
        ([] if bn else [("_CoefficientsTrainBackward", "coeff_net_grad")]), ran
    assert bn or ran[-1][0] == "_CoefficientsTrainBackward", ran
    assert after_bwd == ("guide_fold_batch_grad" if bn else "coeff_net_grad"), after_bwd
    close(f"{tag} loss", float(loss), float(loss_ref), 2e-5 if pyramid else 1e-5, 1e-7)
    named = []
    for (name, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        if not p.requires_grad:
            continue
        assert p.grad is not None and q.grad is not None, name
        named.append((name, p.grad, q.grad))
    assert len(named) > 20
    grads_close(tag, named, 2e-3 if pyramid else 1e-3)
    if bn and not pyramid:
        torch.testing.assert_close(m.guide.bn.running_mean, ref.guide.bn.running_mean, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(m.guide.bn.running_var, ref.guide.bn.running_var, rtol=1e-4, atol=1e-6)
        assert int(m.guide.bn.num_batches_tracked) == int(ref.guide.bn.num_batches_tracked) == 1


def benchmark_twins(dev, lr):
    """Two HDRNetPointwiseNNGuide(batch_norm=False) with identical weights, each with the FlatAdam bench.py builds."""
    from hdrnet_amd import models, optim
    torch.manual_seed(4)
    state = {k: v.clone() for k, v in models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).to(dev).state_dict().items()}
    out = []
    for _ in range(2):
        m = models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).to(dev).train()
        m.load_state_dict(state)
        out.append((m, optim.FlatAdam([p for p in m.parameters() if p.requires_grad], lr=lr, epsilon_hat=True)))
    return out


@pytest.mark.parametrize("flat_bucket", [True, False])
def test_graphed_step_equals_the_eager_step_4x1080p(dev, flat_bucket):
    """GraphedTrainStep(model, l2_loss, FlatAdam(epsilon_hat=True)) as bench.py runs it against an eager TrainStep twin.
    lr = 0: the parameters never move, so each of three replays sees the warm-up's inputs; the flat gradient bucket and
    the loss against the twin's at the fused-versus-composed bars (bit-equality printed, not required)."""
    from hdrnet_amd import metrics
    from hdrnet_amd.runtime import GraphedTrainStep, TrainStep
    low, full, target = config4_batch(dev, 22)
    (me, oe), (mg, og) = benchmark_twins(dev, 0.0)
    loss_fn = lambda out, tgt: metrics.l2_loss(tgt, out)  # noqa: E731
    eager = TrainStep(me, loss_fn, oe)
    flat0 = og.flat.clone()
    step = GraphedTrainStep(mg, loss_fn, og, [low, full], [target], warmup=3, flat_bucket=flat_bucket)
    assert step.split == flat_bucket and step.bucket is og.bucket and eager.bucket is oe.bucket
    names = [n for n, p in mg.named_parameters() if p.requires_grad]
    tag = f"graph vs eager 4 x 1080p flat_bucket={flat_bucket}"
    for k in range(3):
        lg = step([low, full], [target])
        le = eager([low, full], [target])
        torch.cuda.synchronize()
        assert step.bucket.attached()
        close(f"{tag} replay {k} loss", float(lg), float(le), 1e-5, 1e-7)
        same = grads_close(f"{tag} replay {k}", list(zip(names, step.bucket.views, eager.bucket.views)), 1e-3)
        print(f"{tag} replay {k}: loss bit-equal: {float(lg) == float(le)}; flat bucket bit-equal: "
              f"{same and torch.equal(step.bucket.flat, eager.bucket.flat)}")
        assert torch.equal(og.flat, flat0) and torch.equal(oe.flat, flat0)
    assert float(og.steps) == 3 + 3 and float(oe.steps) == 3


@pytest.mark.parametrize("flat_bucket", [True, False])
def test_graphed_adam_update_and_step_count_4x1080p(dev, flat_bucket):
    """lr = 1e-4: the update inside the captured graph (flat_bucket=False) or behind it (True), and the device-side
    step count under replay.  The float64 restatement starts from the parameters and slots as the constructor's warm-up
    left them and is driven with the gradients each replay left in the bucket, so that what is compared is the update
    alone: parameters, slots and update at C's bars, opt.steps == warm-up + replays."""
    from hdrnet_amd import metrics
    from hdrnet_amd.runtime import GraphedTrainStep
    low, full, target = config4_batch(dev, 23)
    (mg, og), _ = benchmark_twins(dev, HYPER["lr"])
    step = GraphedTrainStep(mg, lambda out, tgt: metrics.l2_loss(tgt, out), og, [low, full], [target], warmup=3,
                            flat_bucket=flat_bucket)
    torch.cuda.synchronize()
    assert float(og.steps) == 3.0
    ref = AdamRef(og.flat, og.exp_avg, og.exp_avg_sq, 3, True)
    tag = f"Adam under replay 4 x 1080p flat_bucket={flat_bucket}"
    for k in range(3):
        before = [a.clone() for a in (og.flat, og.exp_avg, og.exp_avg_sq)]
        step([low, full], [target])
        torch.cuda.synchronize()
        ref.check(tag, step.bucket.flat.clone(), before, (og.flat, og.exp_avg, og.exp_avg_sq))
        assert float(og.steps) == 3.0 + k + 1
    print(f"{tag}: update distance / uncancelled update: float32 numpy restatement {ref.worst['d32']:.3e}, "
          f"kernel {ref.worst['dk']:.3e}")
