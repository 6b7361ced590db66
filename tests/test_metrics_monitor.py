"""The training monitors without a GPU: hdrnet_loss_psnr_f32's refusals (include/hdrnet_amd_train.h), and the stock-formula
paths of metrics.loss_and_psnr / Monitor / evaluate on CPU float64 tensors against the reference's formulas
(hdrnet/metrics.py:21-33; hdrnet/bin/train.py:95-96, 117-125, 160-174).  The kernels: tests/test_gpu_metrics_monitor.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

NAMES = ("hdrnet_loss_psnr_workspace_bytes", "hdrnet_loss_psnr_f32")
P = 0x10000  # a 16-byte aligned non-null "pointer": validation precedes any HIP call, nothing is dereferenced
DB = -10.0 / math.log(10.0)


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for n in NAMES:
        getattr(lib, n).restype, getattr(lib, n).argtypes = _lib.TRAIN_SIGNATURES[n]
    return lib


def call(lib, **kw):
    n, batch = kw.get("n", 96), kw.get("batch", 2)
    a = dict(prediction=P, target=P, n=n, batch=batch, loss=P, psnr=P, image_mse=None, dprediction_unit=None, ema=None,
             decay=0.99, totals=None, workspace=P, workspace_bytes=1 << 20, stream=None)
    a.update(kw)
    return lib.hdrnet_loss_psnr_f32(*a.values())


def test_entry_points_are_declared_bound_and_exported(lib):
    from hdrnet_amd import _lib, build, metrics
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hdrnet_amd_train.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b" + n + r"\s*\(", src) and n in _lib.TRAIN_SIGNATURES and hasattr(lib, n)
    params = [p.split()[-1].lstrip("*") for p in re.search(NAMES[1] + r"\s*\(([^)]*)\)", src).group(1).split(",")]
    assert params == ["prediction", "target", "n", "batch", "loss", "psnr", "image_mse", "dprediction_unit", "ema", "decay",
                      "totals", "workspace", "workspace_bytes", "stream"]
    assert {"l2_loss", "psnr", "loss_and_psnr", "Monitor", "evaluate"} <= set(metrics.__all__)
    assert "loss_psnr.hip" in [s for s, _ in build.SOURCES]


def test_refusals_precede_any_hip_call(lib):
    """Every refusal of the header returns 1 with no GPU present (nothing is launched, nothing dereferenced)."""
    assert lib.hdrnet_loss_psnr_workspace_bytes(0, 1) == 0
    for n, b in ((-4, 1), (96, 0), (96, -1), (97, 2)):
        assert lib.hdrnet_loss_psnr_workspace_bytes(n, b) == 0
    need = lib.hdrnet_loss_psnr_workspace_bytes(96, 2)
    assert need >= 2 * 4 and need % 16 == 0
    # what the first pass writes: one float per workgroup, at most 2048 of them or one per image, + two doubles per image
    assert lib.hdrnet_loss_psnr_workspace_bytes(4 * 1080 * 1920 * 3, 4) == 2048 * 4 + 4 * 16
    assert lib.hdrnet_loss_psnr_workspace_bytes(7 * 33 * 31 * 3, 7) == (2048 // 7) * 7 * 4 + 7 * 16
    assert lib.hdrnet_loss_psnr_workspace_bytes(2049 * 12, 2049) == (2049 * 4 + 15) // 16 * 16 + 2049 * 16
    for name in ("prediction", "target", "loss", "psnr", "workspace"):
        assert call(lib, **{name: None}) == 1, name
    assert call(lib, n=0) == 1 and call(lib, n=-96) == 1
    assert call(lib, batch=0) == 1 and call(lib, batch=-2) == 1
    assert call(lib, n=97, batch=2) == 1
    assert call(lib, workspace_bytes=need - 1) == 1 and call(lib, workspace_bytes=0) == 1
    for name in ("prediction", "target", "dprediction_unit"):
        assert call(lib, **{name: P + 4}) == 1, name
    for decay in (1.0, 1.5, -0.01, float("nan")):
        assert call(lib, ema=P, decay=decay) == 1, decay


def reference(t, p):
    """hdrnet/metrics.py:21-33 in float64."""
    sq = (t.double() - p.double()).square()
    per_image = sq.reshape(sq.shape[0], -1).mean(dim=1)
    return float(sq.mean()), float((DB * torch.log(per_image)).mean()), DB * torch.log(per_image)


def test_loss_and_psnr_cpu_float64_is_the_reference_formulas():
    from hdrnet_amd import metrics
    gen = torch.Generator().manual_seed(3)
    t = torch.rand((3, 5, 7, 3), generator=gen, dtype=torch.float64)
    p = torch.rand((3, 5, 7, 3), generator=gen, dtype=torch.float64).requires_grad_(True)
    loss, q = metrics.loss_and_psnr(t, p)
    want_loss, want_q, _ = reference(t, p.detach())
    np.testing.assert_allclose(float(loss.detach()), want_loss, rtol=1e-12)
    np.testing.assert_allclose(float(q), want_q, rtol=1e-12)
    assert not q.requires_grad and loss.requires_grad
    g, = torch.autograd.grad(loss, p)
    np.testing.assert_allclose(g.numpy(), ((2.0 / p.numel()) * (p.detach() - t)).numpy(), rtol=1e-12, atol=0)
    mon = metrics.Monitor()
    got = mon(p, t)
    np.testing.assert_allclose(float(got.detach()), want_loss, rtol=1e-12)
    np.testing.assert_allclose(float(mon.loss), want_loss, rtol=1e-12)
    np.testing.assert_allclose(float(mon.psnr), want_q, rtol=1e-12)
    g2, = torch.autograd.grad(got, p)
    assert torch.equal(g, g2)


def test_loss_and_psnr_match_the_reference_modules_fixture():
    """The values hdrnet/metrics.py computed on the shim (tests/golden/tf_shim/metrics.npz), at the bars of
    tests/test_tf_shim_fixtures.py::test_metrics_match_the_reference_module."""
    from hdrnet_amd import metrics
    with np.load(os.path.join(ROOT, "tests", "golden", "tf_shim", "metrics.npz")) as z:
        fx = {k: z[k] for k in z.files}
    t, p = torch.from_numpy(fx["target"]).double(), torch.from_numpy(fx["prediction"]).double()
    loss, q = metrics.loss_and_psnr(t, p)
    np.testing.assert_allclose(float(loss), float(fx["l2_loss"]), rtol=1e-7)
    np.testing.assert_allclose(float(q), float(fx["psnr"]), rtol=1e-7)
    mon = metrics.Monitor()
    np.testing.assert_allclose(float(mon(p, t)), float(fx["l2_loss"]), rtol=1e-7)
    np.testing.assert_allclose(mon.read()["psnr"], float(fx["psnr"]), rtol=1e-7)


def test_monitor_moving_averages_cpu():
    """Ten steps against s <- s - (1 - decay)(s - value) from 0 in numpy float64, driven by the reference formulas' values;
    the state is float64 for float64 inputs, so the bar is a few roundings of a double."""
    from hdrnet_amd import metrics
    mon = metrics.Monitor(decay=0.99)
    assert mon.decay == float(np.float32(0.99))
    with pytest.raises(RuntimeError):
        mon.read()
    with pytest.raises(ValueError):
        metrics.Monitor(decay=1.0)
    mon.reset()  # nothing to zero yet
    gen = torch.Generator().manual_seed(4)
    s = np.zeros(2)
    for k in range(1, 11):
        t = torch.rand((2, 6, 4, 3), generator=gen, dtype=torch.float64)
        p = t + (0.1 * k) * torch.rand((2, 6, 4, 3), generator=gen, dtype=torch.float64)
        mon(p, t)
        want_loss, want_q, _ = reference(t, p)
        s = s - (1.0 - mon.decay) * (s - np.array([want_loss, want_q]))
        r = mon.read()
        assert r["updates"] == k and isinstance(r["updates"], int)
        np.testing.assert_allclose([r["loss"], r["psnr"]], [want_loss, want_q], rtol=1e-12)
        np.testing.assert_allclose([r["ema_loss"], r["ema_psnr"]], s, rtol=1e-12)
        np.testing.assert_allclose([r["ema_loss_debiased"], r["ema_psnr_debiased"]], s / (1.0 - mon.decay ** k), rtol=1e-12)
    assert float(mon.updates) == 10.0 and float(mon.ema_loss) == r["ema_loss"] and float(mon.ema_psnr) == r["ema_psnr"]
    mon.reset()
    r = mon.read()
    assert r["updates"] == 0 and r["ema_loss"] == 0.0 and r["ema_psnr"] == 0.0 and math.isnan(r["ema_loss_debiased"])
    with pytest.raises(RuntimeError):
        mon(p.float(), t.float())  # another dtype than the state's


class StandInDataset:
    """next_batch / __len__ and the attributes evaluate() inspects, over CPU float64 pairs."""

    def __init__(self, inputs, targets, order="sequential", fliplr=False, flipud=False, rotate=False, random_crop=False):
        self.inputs, self.targets = inputs, targets
        self.order, self.fliplr, self.flipud, self.rotate, self.random_crop = order, fliplr, flipud, rotate, random_crop
        self.next, self.batches = 0, []

    def __len__(self):
        return self.inputs.shape[0]

    def next_batch(self, batch):
        idx = [(self.next + i) % len(self) for i in range(batch)]
        self.next = (self.next + batch) % len(self)
        self.batches.append(batch)
        return self.inputs[idx][:, :2, :2], self.inputs[idx], self.targets[idx]


class SecondInput(torch.nn.Module):
    """`model(lowres, fullres) -> fullres` and a record of the mode it ran in."""

    def __init__(self):
        super().__init__()
        self.modes = []

    def forward(self, low, full):
        self.modes.append((self.training, torch.is_grad_enabled()))
        return full


@pytest.mark.parametrize("batch,groups", [(1, [1] * 5), (2, [2, 2, 1]), (5, [5]), (8, [5])])
def test_evaluate_is_the_mean_of_per_image_psnrs(batch, groups):
    from hdrnet_amd import metrics
    gen = torch.Generator().manual_seed(5)
    tg = torch.rand((5, 6, 8, 3), generator=gen, dtype=torch.float64)
    noise = torch.rand((5, 6, 8, 3), generator=gen, dtype=torch.float64)
    inp = tg + torch.tensor([0.3, 0.01, 0.1, 0.5, 0.05], dtype=torch.float64).reshape(5, 1, 1, 1) * noise
    per_image = [DB * math.log(float((inp[i] - tg[i]).square().mean())) for i in range(5)]
    want = sum(per_image) / 5
    assert abs(want - reference(tg, inp)[1]) < 1e-12
    ds, model = StandInDataset(inp, tg), SecondInput()
    for was in (True, False):
        model.train(was)
        got = metrics.evaluate(model, ds, batch=batch)
        assert isinstance(got, float)
        np.testing.assert_allclose(got, want, rtol=1e-12)
        assert model.training is was
    assert ds.batches == groups * 2 and model.modes == [(False, False)] * len(ds.batches)


def test_evaluate_restores_the_mode_after_an_error_and_refuses_training_pipelines():
    from hdrnet_amd import metrics
    x = torch.rand((3, 4, 4, 3), dtype=torch.float64)

    class Broken(torch.nn.Module):
        def forward(self, low, full):
            raise KeyError("broken")

    model = Broken().train()
    with pytest.raises(KeyError):
        metrics.evaluate(model, StandInDataset(x, x + 0.1))
    assert model.training
    ok = SecondInput()
    for kw in (dict(order="random"), dict(order="epoch"), dict(fliplr=True), dict(flipud=True), dict(rotate=True),
               dict(rotate="even"), dict(random_crop=True)):
        with pytest.raises(ValueError):
            metrics.evaluate(ok, StandInDataset(x, x + 0.1, **kw))
    with pytest.raises(ValueError):
        metrics.evaluate(ok, StandInDataset(x, x + 0.1), batch=0)
    assert ok.modes == []
