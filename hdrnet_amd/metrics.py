"""Image metrics of the reference's training loop (``hdrnet/metrics.py``), on torch tensors.

``l2_loss`` is what ``hdrnet/bin/train.py:95`` minimises.  The literal ``(target - prediction).square().mean()`` is
five bandwidth-bound passes over 100 MB each at 4 x 1080p (240 us of a 1.55-ms training step); ``F.mse_loss`` still is
five launches (the squares written out, a zeros_like of the gradient: 143 us); csrc/metrics.hip does it in two
passes (profiles/r04/train_step.md) -- and when the prediction wants a gradient the forward pass writes the unit gradient
while it has both operands, so the backward has nothing left to read when grad_output is 1.

The reference's loop does not fetch the loss alone: ``train_op`` groups the minimiser with an exponential moving average
(decay 0.99) of the loss AND the PSNR (``hdrnet/bin/train.py:95-96, 117-125``), which is what it logs (``:128-138``), and
its evaluation loop averages the PSNR over a set (``:160-174``).  ``loss_and_psnr``, ``Monitor`` and ``evaluate`` are
those three on csrc/loss_psnr.hip: the loss pass partitioned by image, so that the same two launches also leave the
per-image mean squared errors, the PSNR, the two moving averages and an evaluation set's running sums on the device.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

__all__ = ["l2_loss", "psnr", "loss_and_psnr", "Monitor", "evaluate"]


class _L2Loss(torch.autograd.Function):
    """csrc/metrics.hip.  With a gradient wanted: ``hdrnet_l2_loss_with_grad_f32`` (the loss and the unit gradient
    (2 / n) (prediction - target) in one pass) and ``hdrnet_l2_loss_grad_scale_f32`` in the backward (nothing but a scalar
    read when grad_output is 1); a second backward through a retained graph recomputes with ``hdrnet_l2_loss_grad_f32``.
    Without: ``hdrnet_l2_loss_f32``."""

    @staticmethod
    def forward(ctx, prediction, target):
        from . import _lib
        p, t = prediction.detach().contiguous(), target.detach().contiguous()
        dev, n = p.device, p.numel()
        loss = torch.empty((), dtype=torch.float32, device=dev)
        lib = _lib.load()
        ctx.unit = None
        with torch.cuda.device(dev):
            wbytes = lib.hdrnet_l2_loss_workspace_bytes(n)
            ws = torch.empty((wbytes,), dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            if ctx.needs_input_grad[0]:
                ctx.unit = torch.empty_like(p)
                rc = lib.hdrnet_l2_loss_with_grad_f32(p.data_ptr(), t.data_ptr(), n, loss.data_ptr(), ctx.unit.data_ptr(),
                                                      ws.data_ptr(), wbytes, stream)
                if rc != 0:
                    raise RuntimeError(f"hdrnet_l2_loss_with_grad_f32 failed (rc={rc}): {_lib.last_error()}")
            else:
                _lib.check(lib.hdrnet_l2_loss_f32(p.data_ptr(), t.data_ptr(), n, loss.data_ptr(), ws.data_ptr(), wbytes,
                                                  stream), "L2Loss")
        ctx.save_for_backward(p, t)
        return loss

    @staticmethod
    def backward(ctx, grad_output):
        from . import _lib
        p, t = ctx.saved_tensors
        dev = p.device
        g = grad_output.detach().to(torch.float32).reshape(1).contiguous()
        lib = _lib.load()
        if ctx.unit is not None:  # first backward: the forward's unit gradient, scaled in place
            dpred, ctx.unit = ctx.unit, None
            with torch.cuda.device(dev):
                rc = lib.hdrnet_l2_loss_grad_scale_f32(dpred.data_ptr(), g.data_ptr(), p.numel(),
                                                       torch.cuda.current_stream(dev).cuda_stream)
            if rc != 0:
                raise RuntimeError(f"hdrnet_l2_loss_grad_scale_f32 failed (rc={rc}): {_lib.last_error()}")
            return dpred, None
        dpred = torch.empty_like(p)
        with torch.cuda.device(dev):
            rc = lib.hdrnet_l2_loss_grad_f32(p.data_ptr(), t.data_ptr(), g.data_ptr(), p.numel(), dpred.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(rc, "L2LossGrad")
        return dpred, None


def l2_loss(target: torch.Tensor, prediction: torch.Tensor) -> torch.Tensor:
    """``tf.reduce_mean(tf.square(target - prediction))`` (hdrnet/metrics.py:8-11).  On the GPU in fp32 with no
    gradient wanted for the target: the two-pass HIP kernels; otherwise ``F.mse_loss``."""
    if (prediction.is_cuda and target.is_cuda and prediction.dtype == torch.float32 and target.dtype == torch.float32
            and prediction.shape == target.shape and not target.requires_grad and prediction.numel() > 0
            # the kernels read float4s: a contiguous but offset view (x.flatten()[1:]) takes the stock op instead of
            # failing in the C-ABI's alignment check
            and prediction.is_contiguous() and target.is_contiguous()
            and prediction.data_ptr() % 16 == 0 and target.data_ptr() % 16 == 0):
        return _L2Loss.apply(prediction, target)
    return F.mse_loss(prediction, target)


def psnr(target: torch.Tensor, prediction: torch.Tensor) -> torch.Tensor:
    """Mean PSNR over the batch, ``-10 / ln 10 * log(mean_per_image(square(target - prediction)))``
    (hdrnet/metrics.py:14-20)."""
    squares = (target - prediction).square().reshape(target.shape[0], -1)
    return ((-10.0 / math.log(10.0)) * torch.log(squares.mean(dim=1))).mean()


def _kernel_eligible(target: torch.Tensor, prediction: torch.Tensor) -> bool:
    """``l2_loss``'s conditions for the HIP path, plus a batch dimension to take the images from."""
    return (prediction.is_cuda and target.is_cuda and prediction.dtype == torch.float32 and target.dtype == torch.float32
            and prediction.shape == target.shape and not target.requires_grad and prediction.numel() > 0
            and prediction.is_contiguous() and target.is_contiguous()
            and prediction.data_ptr() % 16 == 0 and target.data_ptr() % 16 == 0 and prediction.dim() >= 2)


def _loss_psnr_call(p: torch.Tensor, t: torch.Tensor, loss_ptr: int, psnr_ptr: int, unit: Optional[torch.Tensor] = None,
                    ema_ptr: Optional[int] = None, decay: float = 0.0, totals: Optional[torch.Tensor] = None,
                    image_mse: Optional[torch.Tensor] = None) -> None:
    """``hdrnet_loss_psnr_f32`` on the current stream of ``p``'s device (include/hdrnet_amd_train.h)."""
    from . import _lib
    lib = _lib.load()
    dev, n, batch = p.device, p.numel(), p.shape[0]
    with torch.cuda.device(dev):
        wbytes = lib.hdrnet_loss_psnr_workspace_bytes(n, batch)
        ws = torch.empty((wbytes,), dtype=torch.uint8, device=dev)
        rc = lib.hdrnet_loss_psnr_f32(p.data_ptr(), t.data_ptr(), n, batch, loss_ptr, psnr_ptr,
                                      None if image_mse is None else image_mse.data_ptr(),
                                      None if unit is None else unit.data_ptr(), ema_ptr, decay,
                                      None if totals is None else totals.data_ptr(), ws.data_ptr(), wbytes,
                                      torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise RuntimeError(f"hdrnet_loss_psnr_f32 failed (rc={rc}): {_lib.last_error()}")


class _LossPsnr(torch.autograd.Function):
    """csrc/loss_psnr.hip: ``hdrnet_loss_psnr_f32`` -- the loss, the PSNR and, with a gradient wanted, the unit gradient in
    one pass; with a ``Monitor`` its state block is updated by the same launches.  The backward is ``_L2Loss``'s."""

    @staticmethod
    def forward(ctx, prediction, target, monitor):
        p, t = prediction.detach().contiguous(), target.detach().contiguous()
        ctx.unit = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        if monitor is None:
            out = torch.empty((2,), dtype=torch.float32, device=p.device)
            _loss_psnr_call(p, t, out.data_ptr(), out.data_ptr() + 4, ctx.unit)
        else:
            out = monitor._state
            _loss_psnr_call(p, t, out.data_ptr(), out.data_ptr() + 4, ctx.unit, out.data_ptr() + 8, monitor.decay)
        ctx.save_for_backward(p, t)
        loss, quality = out[0], out[1]
        ctx.mark_non_differentiable(quality)
        return loss, quality

    @staticmethod
    def backward(ctx, grad_loss, grad_psnr):
        return _L2Loss.backward(ctx, grad_loss) + (None,)


def loss_and_psnr(target: torch.Tensor, prediction: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(l2_loss(target, prediction), psnr(target, prediction))`` from ONE pass over the two tensors
    (``hdrnet/bin/train.py:95-96``).  The loss is differentiable with respect to the prediction exactly as ``l2_loss``'s
    is (the unit gradient written by the forward, scaled, or recomputed on a second backward); the PSNR is detached.
    Where ``l2_loss`` would take its HIP path and the prediction has a batch dimension: csrc/loss_psnr.hip; otherwise
    the two stock formulas."""
    if _kernel_eligible(target, prediction):
        return _LossPsnr.apply(prediction, target, None)
    with torch.no_grad():
        quality = psnr(target, prediction)
    return l2_loss(target, prediction), quality


class Monitor:
    """The training loop's monitored loss: ``Monitor()(output, target) -> loss`` is a ``loss_fn`` for ``runtime.TrainStep``
    / ``GraphedTrainStep`` that also keeps, on the device, what ``hdrnet/bin/train.py:117-138`` logs -- the PSNR of the
    batch and the exponential moving averages of loss and PSNR::

        monitor = metrics.Monitor(decay=0.99)
        step = runtime.GraphedTrainStep(model, monitor, optimizer, [low, full], [target])
        monitor.reset()                      # forget the warm-up and capture passes
        ...
        step(*dataset.feed(step))            # no host work, no synchronisation
        print(monitor.read())                # ONE device-to-host copy

    The state is one small device tensor, created on the first call: ``loss``, ``psnr``, ``ema_loss``, ``ema_psnr`` and
    ``updates`` are views into it (reading them through torch ops synchronises nothing), and the kernel's finishing
    launch updates all five, so a captured graph keeps them current on replay.  ``read()`` returns Python floats,
    including the debiased averages ``ema / (1 - decay ** updates)``; ``reset()`` zeroes the state on the device and is
    legal after capture.

    The averages follow ``tf.train.ExponentialMovingAverage(decay).apply([tensor])`` as remembered from TF 1.x (not
    confirmed against TensorFlow): ``s <- s - (1 - decay)(s - value)`` from ``s = 0``, not debiased.  ``decay`` is
    rounded to float32, the type it reaches the kernel in, so that every path and the debiasing use one value.
    Inputs the kernel does not take (CPU, float64, ...) go through the stock formulas and torch ops on the same state.
    Values are RANK-LOCAL: no collective is added; average ``read()`` across ranks if a global figure is wanted."""

    _FIELDS = ("loss", "psnr", "ema_loss", "ema_psnr", "updates")

    def __init__(self, decay: float = 0.99):
        decay = torch.tensor(float(decay), dtype=torch.float32).item()
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"decay should be in [0, 1), got {decay}")
        self.decay = decay
        self._state: Optional[torch.Tensor] = None  # {loss, psnr, ema_loss, ema_psnr, updates, 0, 0, 0}

    def _state_for(self, prediction: torch.Tensor) -> torch.Tensor:
        dtype = torch.float64 if prediction.dtype == torch.float64 else torch.float32
        if self._state is None:
            self._state = torch.zeros((8,), dtype=dtype, device=prediction.device)
        elif self._state.device != prediction.device or self._state.dtype != dtype:
            raise RuntimeError(f"Monitor: the state is {self._state.dtype} on {self._state.device}, the prediction "
                               f"{prediction.dtype} on {prediction.device}; use one Monitor per stream of batches")
        return self._state

    def __call__(self, output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        state = self._state_for(output)
        if _kernel_eligible(target, output):
            return _LossPsnr.apply(output, target, self)[0]
        loss = l2_loss(target, output)
        with torch.no_grad():
            state[0] = loss
            state[1] = psnr(target, output)
            state[2:4] -= (1.0 - self.decay) * (state[2:4] - state[0:2])
            state[4] += 1
        return loss

    def _view(self, i: int) -> torch.Tensor:
        if self._state is None:
            raise RuntimeError("Monitor: no state before the first call")
        return self._state[i]

    loss = property(lambda self: self._view(0))
    psnr = property(lambda self: self._view(1))
    ema_loss = property(lambda self: self._view(2))
    ema_psnr = property(lambda self: self._view(3))
    updates = property(lambda self: self._view(4))

    def reset(self) -> None:
        """Zero the averages, the count and the last values on the device (a no-op before the first call)."""
        if self._state is not None:
            self._state.zero_()

    def read(self) -> dict:
        """``{loss, psnr, ema_loss, ema_psnr, updates, ema_loss_debiased, ema_psnr_debiased}`` as Python numbers, from
        one device-to-host copy (this synchronises).  The debiased readings are ``nan`` before the first update."""
        if self._state is None:
            raise RuntimeError("Monitor: no state before the first call")
        v = self._state.tolist()
        out = dict(zip(self._FIELDS, v))
        out["updates"] = int(v[4])
        scale = 1.0 - self.decay ** out["updates"]
        for k in ("ema_loss", "ema_psnr"):
            out[k + "_debiased"] = v[self._FIELDS.index(k)] / scale if out["updates"] > 0 else float("nan")
        return out


def evaluate(model: torch.nn.Module, dataset, batch: int = 1) -> float:
    """The mean PSNR of ``model`` over ``dataset`` -- what ``hdrnet/bin/train.py:160-174`` means: every image once through
    the evaluation pipeline (``:79-85``: no shuffle, no flips, no rotation, centre crop), the model in inference mode, the
    per-image PSNRs averaged.  (The reference's own lines compute ``eval_psnr`` from the TRAINING graph's prediction,
    ``:86, :105``, so its loop averages the PSNR of training batches; this is the evaluation those lines intend.)

    ``dataset``: a ``data.DeviceDataset`` / ``RaggedDeviceDataset`` with targets, built with ``order="sequential"``,
    ``fliplr=False``, ``flipud=False``, ``rotate=False``, ``random_crop=False`` -- anything else raises ``ValueError``.
    ``len(dataset)`` images are taken through ``dataset.next_batch`` in groups of ``batch`` (the last group smaller),
    under ``torch.no_grad()`` and ``model.eval()``; the previous mode is restored.  The kernel adds each image's PSNR to
    running sums on the device, image by image in order, and ONE host read at the end returns ``sum / images``."""
    if int(batch) < 1:
        raise ValueError("batch >= 1")
    if getattr(dataset, "order", None) != "sequential":
        raise ValueError(f"evaluate: the dataset should be built with order='sequential', not {getattr(dataset, 'order', None)!r}")
    if dataset.fliplr or dataset.flipud or dataset.rotate or dataset.random_crop:
        raise ValueError("evaluate: the dataset augments (fliplr / flipud / rotate / random_crop); the evaluation "
                         "pipeline takes every image as it is, centre-cropped")
    left = len(dataset)
    if left <= 0:
        raise ValueError("evaluate: an empty dataset")
    was_training = model.training
    model.eval()
    totals = None  # float64 {sum of per-image PSNR, sum of per-image MSE, images}
    try:
        with torch.no_grad():
            while left > 0:
                k = min(int(batch), left)
                low, full, target = dataset.next_batch(k)
                if target is None:
                    raise ValueError("evaluate needs a dataset with targets")
                output = model(low, full)
                if totals is None:
                    totals = torch.zeros((3,), dtype=torch.float64, device=output.device)
                if _kernel_eligible(target, output):
                    scratch = torch.empty((2,), dtype=torch.float32, device=output.device)
                    _loss_psnr_call(output, target, scratch.data_ptr(), scratch.data_ptr() + 4, totals=totals)
                else:
                    mse = (target - output).square().reshape(k, -1).mean(dim=1).double()
                    totals[0] += ((-10.0 / math.log(10.0)) * torch.log(mse)).sum()
                    totals[1] += mse.sum()
                    totals[2] += k
                left -= k
    finally:
        model.train(was_training)
    psnr_sum, _, images = totals.tolist()
    return psnr_sum / images
