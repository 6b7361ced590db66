"""Python interface to the MI355X bilateral-grid ops -- the drop-in for
``hdrnet/hdrnet_ops.py`` of the reference.

Same two callables, same argument order / keyword, same NHWC float32 layouts, same
registered gradients:

=============================================  =======================================
reference (TensorFlow custom op)               here (torch.autograd.Function on ROCm)
=============================================  =======================================
``hdrnet_ops.bilateral_slice(grid, guide)``    ``bilateral_slice(grid, guide)``
  hdrnet/hdrnet_ops.py:30                        -> [B, H, W, C]
``hdrnet_ops.bilateral_slice_apply(grid,       ``bilateral_slice_apply(grid, guide,
  guide, input, has_offset=...)``  :31           input, has_offset=...)`` -> [B, H, W, Cout]
``@RegisterGradient('BilateralSlice')`` :34    ``_BilateralSlice.backward``  (dgrid, dguide)
``@RegisterGradient('BilateralSliceApply')``   ``_BilateralSliceApply.backward``
  :41-48                                         (dgrid, dguide, dinput)
=============================================  =======================================

Shapes (``bilateral_slice_apply_op.cc:147-193``): grid ``[B, GH, GW, GD, Cout*Cj]`` with
``Cj = Cin + has_offset`` and channel ``c = i*Cj + j``; guide ``[B, H, W]``; input
``[B, H, W, Cin]``.  Violations raise ``ValueError`` (TF: ``InvalidArgument``).

Every call goes through the C-ABI of ``include/hdrnet_amd.h`` on the current HIP stream
of the tensors' device, asynchronously.  There is no CPU or eager fallback: tensors
must live on an AMD GPU and ``libhdrnet_amd.so`` must load, otherwise the call raises.
"""
from __future__ import annotations

import contextlib
import ctypes
import functools
import threading
from typing import Optional, Tuple

import torch

from . import _lib

__all__ = ["bilateral_slice", "bilateral_slice_apply", "bilateral_slice_apply_rows", "bilateral_slice_apply_nnguide",
           "bilateral_slice_apply_io", "bilateral_slice_apply_curves", "bilateral_slice_apply_upadd", "resize_bilinear", "input_moments",
           "resize_bilinear_io", "bilateral_slice_apply_upadd_io", "bilateral_slice_apply_io_u16",
           "bilateral_slice_apply_io_yuv_deep", "yuv_planar_to_rgb", "bilateral_slice_apply_io_yuv_planar",
           "CoefficientWeights", "coefficients", "coefficients_train", "coefficients_train_supported", "guide_fold_batch", "guide_nn_prescale", "curves_guide_prepare",
           "kernel_override", "last_kernel"]

_tls = threading.local()


def _flags() -> int:
    return getattr(_tls, "flags", _lib.KERNEL_AUTO)


@contextlib.contextmanager
def kernel_override(which: str, variant: int = 0):
    """Force a kernel family inside the block: 'auto' | 'generic' | 'fast' (tests/bench).
    `variant` > 0 selects a benchmark-only kernel of the TOOLS build (include/hdrnet_amd_tools.h,
    tools/ab_bench.py); the product library these ops call has no variants and answers any non-zero
    variant with HDRNET_INVALID_ARGUMENT (raised as HdrnetInvalidArgument)."""
    table = {"auto": _lib.KERNEL_AUTO, "generic": _lib.KERNEL_GENERIC, "fast": _lib.KERNEL_FAST}
    old = _flags()
    _tls.flags = table[which] | ((int(variant) & 0xFF) << 8)
    try:
        yield
    finally:
        _tls.flags = old


def last_kernel() -> str:
    """Name of the kernel variant this thread's last call launched."""
    return _lib.last_kernel()


# ---- argument checking (mirrors the OP_REQUIRES of the reference op wrappers) --------
def _require_f32(name: str, t: torch.Tensor) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (the op is registered for float only), got {t.dtype}")


def _require_gpu(name: str, t: torch.Tensor) -> None:
    # Checked AFTER the shape rules so that shape errors surface as ValueError on any
    # device (tests/test_host_logic.py runs them without a GPU).
    if not t.is_cuda:
        raise RuntimeError(
            f"{name} is on {t.device}: hdrnet_amd ops run on an MI355X (HIP) device only; "
            "there is no CPU path in this package")


def _check_slice(grid: torch.Tensor, guide: torch.Tensor) -> Tuple[int, ...]:
    _require_f32("grid", grid)
    _require_f32("guide", guide)
    if grid.dim() != 5:
        raise ValueError("Grid should be 5D (batch_size, grid_height, grid_width, grid_depth, "
                         f"grid_channels), got {tuple(grid.shape)}")
    if guide.dim() != 3:
        raise ValueError(f"Guide image should be 3D (batch_size, height, width), got {tuple(guide.shape)}")
    if grid.device != guide.device:
        raise ValueError("grid and guide must be on the same device")
    B, GH, GW, GD, C = grid.shape
    if guide.shape[0] != B:
        raise ValueError("Batch sizes should match.")
    if min(GH, GW, GD, C) <= 0:
        raise ValueError(f"grid extents must be positive, got {tuple(grid.shape)}")
    _require_gpu("grid", grid)
    _require_gpu("guide", guide)
    return B, guide.shape[1], guide.shape[2], GH, GW, GD, C


def _check_apply(grid, guide, inp, has_offset: bool) -> Tuple[int, ...]:
    _require_f32("grid", grid)
    _require_f32("guide", guide)
    _require_f32("input", inp)
    if grid.dim() != 5:
        raise ValueError("Input grid should be 5D (batch_size, height, width, depth, "
                         f"output_channels * input_channels), got {tuple(grid.shape)}")
    if guide.dim() != 3:
        raise ValueError(f"Guide image should be 3D (batch_size, height, width), got {tuple(guide.shape)}")
    if inp.dim() != 4:
        raise ValueError("Input image should be 4D (batch_size, height, width, input_channels), "
                         f"got {tuple(inp.shape)}")
    if not (grid.device == guide.device == inp.device):
        raise ValueError("grid, guide and input must be on the same device")
    B, GH, GW, GD, C = grid.shape
    if tuple(inp.shape[:3]) != tuple(guide.shape):
        raise ValueError("Input and guide size should match.")
    if guide.shape[0] != B:
        raise ValueError("Batch sizes should match.")
    Cin = inp.shape[3]
    Cj = Cin + (1 if has_offset else 0)
    if Cj <= 0 or C % Cj != 0 or C == 0:
        if has_offset:
            raise ValueError("Slicing with affine offset, grid should have "
                             "output_channels * (input_channels + 1) channels.")
        raise ValueError("Slicing without affine offset, grid should have "
                         "output_channels * input_channels channels.")
    if min(GH, GW, GD) <= 0:
        raise ValueError(f"grid extents must be positive, got {tuple(grid.shape)}")
    for n, t in (("grid", grid), ("guide", guide), ("input", inp)):
        _require_gpu(n, t)
    return B, guide.shape[1], guide.shape[2], GH, GW, GD, Cin, C // Cj


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _workspace(query, *args, device):
    """``(workspace, bytes)`` for the size ``query(*args)`` answers on the current device: at least 16 bytes, so that its
    address is never null."""
    wbytes = query(*args)
    return torch.empty((max(wbytes, 16),), dtype=torch.uint8, device=device), wbytes


# ---- raw forward / backward launches (no autograd) ------------------------------------
def _apply_forward(grid, guide, inp, has_offset: bool) -> torch.Tensor:
    B, H, W, GH, GW, GD, Cin, Cout = _check_apply(grid, guide, inp, has_offset)
    grid, guide, inp = grid.contiguous(), guide.contiguous(), inp.contiguous()
    out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=guide.device)
    lib = _lib.load()
    with torch.cuda.device(guide.device):
        rc = lib.hdrnet_bilateral_slice_apply_f32_ex(
            grid.data_ptr(), guide.data_ptr(), inp.data_ptr(), out.data_ptr(),
            B, H, W, GH, GW, GD, Cin, Cout, int(has_offset), _flags(), _stream(guide.device))
    _lib.check(rc, "BilateralSliceApply")
    return out


def _apply_backward(grid, guide, inp, dout, has_offset: bool, need, flags: Optional[int] = None):
    B, H, W, GH, GW, GD, Cin, Cout = _check_apply(grid, guide, inp, has_offset)
    if tuple(dout.shape) != (B, H, W, Cout):
        raise ValueError(f"backprop should have shape {(B, H, W, Cout)}, got {tuple(dout.shape)}")
    _require_f32("backprop", dout)
    _require_gpu("backprop", dout)
    grid, guide, inp, dout = grid.contiguous(), guide.contiguous(), inp.contiguous(), dout.contiguous()
    dev = guide.device
    dgrid = torch.empty_like(grid) if need[0] else None
    dguide = torch.empty_like(guide) if need[1] else None
    dinput = torch.empty_like(inp) if need[2] else None
    lib = _lib.load()
    with torch.cuda.device(dev):  # workspace sizes may depend on the CURRENT device (CU count)
        wbytes = lib.hdrnet_bilateral_slice_apply_grad_workspace_bytes(
            B, H, W, GH, GW, GD, Cin, Cout, int(has_offset)) if need[0] else 0
        ws = torch.empty((wbytes,), dtype=torch.uint8, device=dev) if wbytes else None
        rc = lib.hdrnet_bilateral_slice_apply_grad_f32_ex(
            grid.data_ptr(), guide.data_ptr(), inp.data_ptr(), dout.data_ptr(),
            _ptr(dgrid), _ptr(dguide), _ptr(dinput),
            B, H, W, GH, GW, GD, Cin, Cout, int(has_offset),
            _ptr(ws), wbytes, _flags() if flags is None else flags, _stream(dev))
    _lib.check(rc, "BilateralSliceApplyGrad")
    return dgrid, dguide, dinput


def _slice_forward(grid, guide) -> torch.Tensor:
    B, H, W, GH, GW, GD, C = _check_slice(grid, guide)
    grid, guide = grid.contiguous(), guide.contiguous()
    out = torch.empty((B, H, W, C), dtype=torch.float32, device=guide.device)
    lib = _lib.load()
    with torch.cuda.device(guide.device):
        rc = lib.hdrnet_bilateral_slice_f32_ex(
            grid.data_ptr(), guide.data_ptr(), out.data_ptr(),
            B, H, W, GH, GW, GD, C, _flags(), _stream(guide.device))
    _lib.check(rc, "BilateralSlice")
    return out


def _slice_backward(grid, guide, dout, need, flags: Optional[int] = None):
    B, H, W, GH, GW, GD, C = _check_slice(grid, guide)
    if dout.dim() != 4:
        raise ValueError("Codomain tangent should be 4D (batch, height, width, nchannels).")
    if tuple(dout.shape) != (B, H, W, C):
        raise ValueError(f"backprop should have shape {(B, H, W, C)}, got {tuple(dout.shape)}")
    _require_f32("backprop", dout)
    _require_gpu("backprop", dout)
    grid, guide, dout = grid.contiguous(), guide.contiguous(), dout.contiguous()
    dev = guide.device
    dgrid = torch.empty_like(grid) if need[0] else None
    dguide = torch.empty_like(guide) if need[1] else None
    lib = _lib.load()
    with torch.cuda.device(dev):
        wbytes = lib.hdrnet_bilateral_slice_grad_workspace_bytes(B, H, W, GH, GW, GD, C) if need[0] else 0
        ws = torch.empty((wbytes,), dtype=torch.uint8, device=dev) if wbytes else None
        rc = lib.hdrnet_bilateral_slice_grad_f32_ex(
            grid.data_ptr(), guide.data_ptr(), dout.data_ptr(), _ptr(dgrid), _ptr(dguide),
            B, H, W, GH, GW, GD, C, _ptr(ws), wbytes, _flags() if flags is None else flags, _stream(dev))
    _lib.check(rc, "BilateralSliceGrad")
    return dgrid, dguide


# ---- autograd registration (hdrnet/hdrnet_ops.py:34-48) -------------------------------
class _BilateralSlice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, guide):
        ctx.save_for_backward(grid, guide)
        # autograd runs backward on its own thread: the (thread-local) kernel override in
        # effect at forward time is carried along explicitly.
        ctx.flags = _flags()
        return _slice_forward(grid, guide)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        grid, guide = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not (need[0] or need[1]):
            return None, None
        return _slice_backward(grid, guide, grad, need, ctx.flags)


class _BilateralSliceApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, guide, inp, has_offset):
        ctx.save_for_backward(grid, guide, inp)
        ctx.has_offset = bool(has_offset)
        ctx.flags = _flags()
        return _apply_forward(grid, guide, inp, bool(has_offset))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        grid, guide, inp = ctx.saved_tensors
        need = ctx.needs_input_grad[:3]
        if not any(need):
            return None, None, None, None
        dgrid, dguide, dinput = _apply_backward(grid, guide, inp, grad, ctx.has_offset, need, ctx.flags)
        return dgrid, dguide, dinput, None


def bilateral_slice(grid: torch.Tensor, guide: torch.Tensor, name: Optional[str] = None) -> torch.Tensor:
    """``BilateralSlice``: out[b,y,x,c] = trilinear sample of grid[b,...,c] at
    ((x+.5)*GW/W, (y+.5)*GH/H, guide[b,y,x]*GD).  (bilateral_slice_op.cc:274-290)"""
    del name
    return _BilateralSlice.apply(grid, guide)


def bilateral_slice_apply(grid: torch.Tensor, guide: torch.Tensor, input: torch.Tensor,  # noqa: A002
                          has_offset: bool, name: Optional[str] = None) -> torch.Tensor:
    """``BilateralSliceApply``: slice then per-pixel (Cout x Cj) . [input; 1].
    ``has_offset`` is a required attribute, as in the reference op
    (bilateral_slice_apply_op.cc:382-386)."""
    del name
    return _BilateralSliceApply.apply(grid, guide, input, has_offset)


def bilateral_slice_apply_rows(grid: torch.Tensor, guide_rows: torch.Tensor, input_rows: torch.Tensor,
                               frame_height: int, y0: int, has_offset: bool) -> torch.Tensor:
    """Row-split ``BilateralSliceApply`` forward (the optional intra-image split):
    ``guide_rows`` [B, rows, W] and ``input_rows`` [B, rows, W, Cin] hold rows ``y0 .. y0 + rows - 1`` of
    frames that are ``frame_height`` rows high; the grid is the whole frame's.  The y coordinate is the
    reference's expression on the frame height (bilateral_slice_apply.cc:38,42), so the bands of any
    partition (``dist.row_range``), concatenated, equal the whole-frame op bit for bit.  Forward only."""
    if grid.requires_grad or guide_rows.requires_grad or input_rows.requires_grad:
        if torch.is_grad_enabled():
            raise RuntimeError("bilateral_slice_apply_rows is forward-only (inference); detach the operands")
    B, rows, W, GH, GW, GD, Cin, Cout = _check_apply(grid, guide_rows, input_rows, has_offset)
    frame_height, y0 = int(frame_height), int(y0)
    if y0 < 0 or y0 + rows > frame_height:
        raise ValueError(f"row band [{y0}, {y0 + rows}) outside the frame's {frame_height} rows")
    grid, guide_rows, input_rows = grid.contiguous(), guide_rows.contiguous(), input_rows.contiguous()
    out = torch.empty((B, rows, W, Cout), dtype=torch.float32, device=guide_rows.device)
    lib = _lib.load()
    with torch.cuda.device(guide_rows.device):
        rc = lib.hdrnet_bilateral_slice_apply_rows_f32_ex(
            grid.data_ptr(), guide_rows.data_ptr(), input_rows.data_ptr(), out.data_ptr(),
            B, frame_height, y0, rows, W, GH, GW, GD, Cin, Cout, int(has_offset), _flags(),
            _stream(guide_rows.device))
    _lib.check(rc, "BilateralSliceApplyRows")
    return out


def _guide_flags(fast_sigmoid: bool, prescaled: bool) -> int:
    return (_lib.GUIDE_SIGMOID_FAST if fast_sigmoid else 0) | (_lib.GUIDE_RELU_PRESCALED if prescaled else 0)


def guide_nn_prescale(guide_conv1: torch.Tensor, guide_conv2: torch.Tensor, x_max: float = 65536.0):
    """The PRESCALED form of a folded guide network (``hdrnet_guide_nn_prescale_f32``; Cin = 3): per feature k the
    first-layer row reordered to ``{w0, b, w1, w2} * 2**-e_k`` and the mixing weight ``* 2**e_k`` with
    ``2**e_k >= 2 (|b_k| + x_max sum_j |w_kj|)``.  Passed back to the guide-network forwards with ``prescaled=True``
    (``HDRNET_GUIDE_RELU_PRESCALED``) the guide is the plain evaluation's bit for bit for every input with
    ``|x| <= x_max`` -- the kernels then take ``relu`` from the clamp modifier of the feature's last multiply-add
    (128 instead of 208 vector instructions per 256 pixels).  Returns ``(conv1 [n, 4], conv2 [n + 1])``; prepare once
    per parameter set.  Inference only: the guide network's VJP reads the exported layout."""
    _require_f32("guide_conv1", guide_conv1)
    _require_f32("guide_conv2", guide_conv2)
    _require_gpu("guide_conv1", guide_conv1)
    _require_gpu("guide_conv2", guide_conv2)
    if guide_conv1.dim() != 2 or guide_conv1.shape[1] != 4 or tuple(guide_conv2.shape) != (guide_conv1.shape[0] + 1,):
        raise ValueError(f"guide_nn_prescale: guide_conv1 [n, 4] (Cin = 3) and guide_conv2 [n + 1] expected, got "
                         f"{tuple(guide_conv1.shape)}, {tuple(guide_conv2.shape)}")
    c1, c2 = guide_conv1.detach().contiguous(), guide_conv2.detach().contiguous()
    o1, o2 = torch.empty_like(c1), torch.empty_like(c2)
    dev = c1.device
    with torch.cuda.device(dev):
        rc = _lib.load().hdrnet_guide_nn_prescale_f32(c1.data_ptr(), c2.data_ptr(), c1.shape[0], 3, float(x_max),
                                                      o1.data_ptr(), o2.data_ptr(), _stream(dev))
    _lib.check(rc, "GuideNNPrescale")
    return o1, o2


def _check_nnguide(grid, input, guide_conv1, guide_conv2, has_offset):  # noqa: A002
    _require_f32("guide_conv1", guide_conv1)
    _require_f32("guide_conv2", guide_conv2)
    if input.dim() != 4:
        raise ValueError(f"Input image should be 4D (batch_size, height, width, input_channels), got {tuple(input.shape)}")
    Cin = input.shape[3]
    if guide_conv1.dim() != 2 or guide_conv1.shape[1] != Cin + 1:
        raise ValueError(f"guide_conv1 should be [n, Cin + 1] = [n, {Cin + 1}], got {tuple(guide_conv1.shape)}")
    n = guide_conv1.shape[0]
    if tuple(guide_conv2.shape) != (n + 1,):
        raise ValueError(f"guide_conv2 should be [n + 1] = [{n + 1}], got {tuple(guide_conv2.shape)}")
    fake_guide = input[..., 0]  # shape carrier for the shared rule checks; never read
    dims = _check_apply(grid, fake_guide, input, has_offset)
    for nm, t in (("guide_conv1", guide_conv1), ("guide_conv2", guide_conv2)):
        _require_gpu(nm, t)
    return dims + (n,)


def _nnguide_forward(grid, inp, c1, c2, has_offset: bool, want_guide: bool, fast_sigmoid: bool = False,
                     prescaled: bool = False):
    B, H, W, GH, GW, GD, Cin, Cout, n = _check_nnguide(grid, inp, c1, c2, has_offset)
    grid, inp, c1, c2 = grid.contiguous(), inp.contiguous(), c1.contiguous(), c2.contiguous()
    dev = inp.device
    out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=dev)
    gout = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_guide else None
    lib = _lib.load()
    with torch.cuda.device(dev):
        rc = lib.hdrnet_bilateral_slice_apply_nnguide_f32_ex(
            grid.data_ptr(), inp.data_ptr(), c1.data_ptr(), c2.data_ptr(), out.data_ptr(), _ptr(gout),
            B, H, W, GH, GW, GD, Cin, Cout, int(bool(has_offset)), n,
            _guide_flags(fast_sigmoid, prescaled), _stream(dev))
    _lib.check(rc, "BilateralSliceApplyNNGuide")
    return out, gout


def _guide_backward(inp, guide, dguide, c1, c2, dinput, accumulate: bool):
    """VJP of the folded guide network: returns (dconv1, dconv2); adds the guide path's share to
    ``dinput`` in place (or stores it, or skips it when ``dinput`` is None)."""
    inp, guide, dguide = inp.contiguous(), guide.contiguous(), dguide.contiguous()
    c1, c2 = c1.contiguous(), c2.contiguous()
    dev = inp.device
    npx, Cin, n = guide.numel(), inp.shape[-1], c1.shape[0]
    dc1, dc2 = torch.empty_like(c1), torch.empty_like(c2)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws, wbytes = _workspace(lib.hdrnet_pointwise_guide_grad_workspace_bytes, npx, Cin, n, device=dev)
        rc = lib.hdrnet_pointwise_guide_grad_f32(
            inp.data_ptr(), guide.data_ptr(), dguide.data_ptr(), c1.data_ptr(), c2.data_ptr(),
            _ptr(dinput), int(bool(accumulate)), dc1.data_ptr(), dc2.data_ptr(), npx, Cin, n,
            ws.data_ptr(), wbytes, _stream(dev))
    _lib.check(rc, "PointwiseGuideGrad")
    return dc1, dc2


class _BilateralSliceApplyNNGuide(torch.autograd.Function):
    """guide network + slice-apply as ONE differentiable op: forward = the fused kernel (the
    guide is written once, for the backward); backward = slice-apply VJP, then the guide
    network's VJP, which adds its share into the same dinput buffer."""

    @staticmethod
    def forward(ctx, grid, inp, c1, c2, has_offset):
        out, guide = _nnguide_forward(grid, inp, c1, c2, bool(has_offset), want_guide=True)
        ctx.save_for_backward(grid, inp, c1, c2, guide)
        ctx.has_offset = bool(has_offset)
        ctx.flags = _flags()
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        grid, inp, c1, c2, guide = ctx.saved_tensors
        need_grid, need_inp, need_c1, need_c2 = ctx.needs_input_grad[:4]
        need_net = need_c1 or need_c2
        if not (need_grid or need_inp or need_net):
            return None, None, None, None, None
        dgrid, dguide, dinput = _apply_backward(grid, guide, inp, grad, ctx.has_offset,
                                                (need_grid, need_net or need_inp, need_inp), ctx.flags)
        dc1 = dc2 = None
        if need_net or need_inp:
            dc1, dc2 = _guide_backward(inp, guide, dguide, c1, c2, dinput, accumulate=True)
        return dgrid, dinput, dc1 if need_c1 else None, dc2 if need_c2 else None, None


def bilateral_slice_apply_nnguide(grid: torch.Tensor, input: torch.Tensor,  # noqa: A002
                                  guide_conv1: torch.Tensor, guide_conv2: torch.Tensor,
                                  has_offset: bool = True, return_guide: bool = False, fast_sigmoid: bool = False,
                                  prescaled: bool = False):
    """Fusion of ``HDRNetPointwiseNNGuide._guide`` (hdrnet/models.py:203-210, batch norm folded)
    with ``bilateral_slice_apply``: the guide is computed in registers and sliced immediately.

    ``fast_sigmoid`` (forward without autograd only): the hardware exp / reciprocal sigmoid instead of
    ``tf.nn.sigmoid``'s form -- <= 2 ulp of the guide, ~1e-6 of the output's scale, ~10 % faster; an explicit choice
    (``HDRNET_GUIDE_SIGMOID_FAST``).  A differentiable call always uses the exact form: the backward reads the guide.

    ``prescaled`` (forward without autograd only): ``guide_conv1`` / ``guide_conv2`` are ``guide_nn_prescale``'s arrays
    (``HDRNET_GUIDE_RELU_PRESCALED``) -- the same guide bit for bit for inputs within the prescale's ``x_max``.

    ``guide_conv1`` is ``[n, Cin + 1]`` (weights then bias of feature k) and ``guide_conv2``
    ``[n + 1]`` (mixing weights then bias) -- the layout ``hdrnet/bin/freeze_graph.py:170-184``
    exports as ``guide_conv1.bin`` / ``guide_conv2.bin``.

    Differentiable in ``grid``, ``input``, ``guide_conv1`` and ``guide_conv2`` (the guide is then
    written once for the backward, whose guide-network VJP exists for ``Cin`` in {1, 3} and ``n`` in
    {4, 8, 16}).  ``return_guide=True`` returns ``(out, guide)`` without autograd.  Same shape rules
    as ``bilateral_slice_apply``; raises ``ValueError`` where the fused kernel has no
    specialisation."""
    if return_guide:
        return _nnguide_forward(grid.detach(), input.detach(), guide_conv1.detach(), guide_conv2.detach(),
                                has_offset, want_guide=True, fast_sigmoid=fast_sigmoid, prescaled=prescaled)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (grid, input, guide_conv1, guide_conv2)):
        if prescaled:
            raise ValueError("bilateral_slice_apply_nnguide: prescaled guide parameters are inference-only "
                             "(the guide network's VJP reads the exported layout)")
        dims = _check_nnguide(grid, input, guide_conv1, guide_conv2, has_offset)
        # the guide-network VJP has specialisations for a few widths only: say so NOW, not from
        # inside backward() on the autograd thread
        with torch.cuda.device(input.device):
            if _lib.load().hdrnet_pointwise_guide_grad_workspace_bytes(1024, dims[6], dims[8]) == 0:
                raise ValueError(
                    f"bilateral_slice_apply_nnguide: no guide-network VJP for Cin = {dims[6]}, n_feats = {dims[8]} "
                    "(Cin in {1, 3}, n_feats in {4, 8, 16}); compose the guide network from torch ops and "
                    "call bilateral_slice_apply, or run without autograd")
        return _BilateralSliceApplyNNGuide.apply(grid, input, guide_conv1, guide_conv2, has_offset)
    return _nnguide_forward(grid.detach(), input.detach(), guide_conv1.detach(), guide_conv2.detach(),
                            has_offset, want_guide=False, fast_sigmoid=fast_sigmoid, prescaled=prescaled)[0]


class _BilateralSliceApplyCurves(torch.autograd.Function):
    """curves guide + slice-apply as ONE differentiable op (the standard model's training path):
    forward = the fused kernel (guide written once for the backward); backward = slice-apply VJP,
    then the curves guide's VJP, which adds its share into the same dinput buffer."""

    @staticmethod
    def forward(ctx, grid, inp, ccm, shifts, slopes, mix, has_offset):
        out, guide = bilateral_slice_apply_io(grid, inp, guide_curves=(ccm, shifts, slopes, mix),
                                              has_offset=bool(has_offset), return_guide=True)
        ctx.save_for_backward(grid, inp, ccm, shifts, slopes, mix, guide)
        ctx.has_offset = bool(has_offset)
        ctx.flags = _flags()
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        grid, inp, ccm, shifts, slopes, mix, guide = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_net = any(need[2:6])
        if not (need[0] or need[1] or need_net):
            return (None,) * 7
        dgrid, dguide, dinput = _apply_backward(grid, guide, inp, grad, ctx.has_offset,
                                                (need[0], need_net or need[1], need[1]), ctx.flags)
        grads = [None] * 4
        if need_net or need[1]:
            inp_c, dguide = inp.contiguous(), dguide.contiguous()
            params = [t.contiguous() for t in (ccm, shifts, slopes, mix)]
            outs = [torch.empty_like(t) for t in params]
            npx, npts = dguide.numel(), shifts.shape[0]
            lib = _lib.load()
            with torch.cuda.device(inp.device):
                ws, wbytes = _workspace(lib.hdrnet_curves_guide_grad_workspace_bytes, npx, 3, npts, device=inp.device)
                rc = lib.hdrnet_curves_guide_grad_f32(
                    inp_c.data_ptr(), dguide.data_ptr(), *[t.data_ptr() for t in params], _ptr(dinput), 1,
                    *[t.data_ptr() for t in outs], npx, 3, npts, ws.data_ptr(), wbytes, _stream(inp.device))
            _lib.check(rc, "CurvesGuideGrad")
            grads = [g if n else None for g, n in zip(outs, need[2:6])]
        return (dgrid, dinput, *grads, None)


def bilateral_slice_apply_curves(grid: torch.Tensor, input: torch.Tensor, ccm: torch.Tensor,  # noqa: A002
                                 shifts: torch.Tensor, slopes: torch.Tensor, mix: torch.Tensor,
                                 has_offset: bool = True, prepared: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``HDRNetCurves._guide`` (hdrnet/models.py:145-190) fused with ``bilateral_slice_apply``, fp32,
    differentiable in ``grid``, ``input`` and the four guide parameter arrays (layouts of
    hdrnet/bin/freeze_graph.py:107-127: ccm [3, 4], shifts / slopes [16, 3], mix [4]).  The wire-format
    inference variant is ``bilateral_slice_apply_io(..., guide_curves=...)``.  ``prepared`` (forward without autograd
    only): the tables of ``curves_guide_prepare(shifts, slopes)``."""
    if torch.is_grad_enabled() and any(t.requires_grad for t in (grid, input, ccm, shifts, slopes, mix)):
        if prepared is not None:
            raise ValueError("bilateral_slice_apply_curves: prepared tables are inference-only")
        if input.dim() != 4 or input.shape[3] != 3 or shifts.dim() != 2 or shifts.shape[0] != 16:
            raise ValueError("the differentiable curves-guide op needs Cin = 3 and 16 knots per channel")
        return _BilateralSliceApplyCurves.apply(grid, input, ccm, shifts, slopes, mix, has_offset)
    return bilateral_slice_apply_io(grid, input, guide_curves=(ccm, shifts, slopes, mix), has_offset=has_offset,
                                    curves_prepared=prepared)


def input_moments(input: torch.Tensor):  # noqa: A002
    """``(sum_px in_j [Cin], sum_px in_i * in_j [Cin, Cin])`` over every pixel of ``input``
    ``[..., Cin]`` in one pass.  The first guide convolution is linear, so these give the batch
    statistics its batch norm needs in training mode (hdrnet/layers.py:40-58) without the
    n-channel full-resolution tensor.  No autograd."""
    _require_f32("input", input)
    _require_gpu("input", input)
    inp = input.detach().contiguous()
    Cin = inp.shape[-1]
    npx = inp.numel() // max(Cin, 1)
    dev = inp.device
    sums = torch.empty((Cin,), dtype=torch.float32, device=dev)
    mom = torch.empty((Cin, Cin), dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws, wbytes = _workspace(lib.hdrnet_input_moments_workspace_bytes, npx, Cin, device=dev)
        rc = lib.hdrnet_input_moments_f32(inp.data_ptr(), npx, Cin, sums.data_ptr(), mom.data_ptr(),
                                          ws.data_ptr(), wbytes, _stream(dev))
    _lib.check(rc, "InputMoments")
    return sums, mom


class _GuideFoldBatch(torch.autograd.Function):
    """Training-mode fold of the guide network's batch norm (``hdrnet_guide_fold_batch_f32`` and its VJP): one launch
    each way where the same float64 math on ~100 numbers was 33 + 30 torch launches of a graph-captured step."""

    @staticmethod
    def forward(ctx, w1, beta, w2, b2, gamma, sums, moments, running_mean, running_var, num_batches_tracked,
                npx, eps, momentum):
        Cin, n = w1.shape
        dev = w1.device
        args = [t.detach().contiguous() for t in (sums, moments, w1, gamma, beta, w2, b2.reshape(1))]
        conv1 = torch.empty((n, Cin + 1), dtype=torch.float32, device=dev)
        conv2 = torch.empty((n + 1,), dtype=torch.float32, device=dev)
        lib = _lib.load()
        with torch.cuda.device(dev):
            rc = lib.hdrnet_guide_fold_batch_f32(
                args[0].data_ptr(), args[1].data_ptr(), int(npx), args[2].data_ptr(), args[3].data_ptr(),
                args[4].data_ptr(), args[5].data_ptr(), args[6].data_ptr(), float(eps), float(momentum), Cin, n,
                conv1.data_ptr(), conv2.data_ptr(), _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked),
                _stream(dev))
        _lib.check(rc, "GuideFoldBatch")
        for t in (running_mean, running_var, num_batches_tracked):
            if t is not None:  # written through a raw pointer: tell autograd / the fold caches keyed on ._version
                torch.autograd.graph.increment_version(t)
        ctx.save_for_backward(*args[:5])
        ctx.meta = (int(npx), float(eps), Cin, n, b2.shape)
        ctx.leaves = (w1, beta, w2, b2)  # where their gradients may be written directly (_grad_out)
        return conv1, conv2

    @staticmethod
    def backward(ctx, dconv1, dconv2):
        sums, moments, w1, gamma, beta = ctx.saved_tensors
        npx, eps, Cin, n, b2_shape = ctx.meta
        dev = w1.device
        dconv1, dconv2 = dconv1.contiguous(), dconv2.contiguous()
        outs = []
        for leaf, shape in zip(ctx.leaves, ((Cin, n), (n,), (n,), tuple(b2_shape))):
            g = _grad_out(leaf) if tuple(leaf.shape) == shape and leaf.is_contiguous() else None
            outs.append(g if g is not None and g.is_contiguous() else torch.empty(shape, dtype=torch.float32, device=dev))
        dw1, dbeta, dw2, db2 = outs
        lib = _lib.load()
        with torch.cuda.device(dev):
            rc = lib.hdrnet_guide_fold_batch_grad_f32(
                sums.data_ptr(), moments.data_ptr(), npx, w1.data_ptr(), gamma.data_ptr(), beta.data_ptr(), eps, Cin, n,
                dconv1.data_ptr(), dconv2.data_ptr(), dw1.data_ptr(), dbeta.data_ptr(), dw2.data_ptr(), db2.data_ptr(),
                _stream(dev))
        _lib.check(rc, "GuideFoldBatchGrad")
        return dw1, dbeta, dw2, db2, None, None, None, None, None, None, None, None, None


def guide_fold_batch(w1: torch.Tensor, beta: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor, gamma: torch.Tensor,
                     sums: torch.Tensor, moments: torch.Tensor, npx: int, eps: float, momentum: float = 0.0,
                     running_mean: Optional[torch.Tensor] = None, running_var: Optional[torch.Tensor] = None,
                     num_batches_tracked: Optional[torch.Tensor] = None):
    """``(conv1 [n, Cin + 1], conv2 [n + 1])``: the point-wise guide network with batch norm in TRAINING mode folded
    into its first layer, the batch statistics taken from the input's ``(sums, moments)`` (``input_moments``) --
    ``hdrnet/layers.py:40-58`` with ``is_training=True`` in the export layout of ``freeze_graph.py:170-184``.
    ``w1`` is ``[Cin, n]``.  Differentiable in ``w1``, ``beta``, ``w2``, ``b2``; moves the running statistics in place."""
    for name, t in (("w1", w1), ("beta", beta), ("w2", w2), ("b2", b2), ("gamma", gamma), ("sums", sums), ("moments", moments)):
        _require_f32(name, t)
        _require_gpu(name, t)
    if w1.dim() != 2 or w1.shape[0] not in (1, 3):
        raise ValueError(f"w1 should be [Cin in (1, 3), n_feats], got {tuple(w1.shape)}")
    return _GuideFoldBatch.apply(w1, beta, w2, b2, gamma, sums, moments, running_mean, running_var,
                                 num_batches_tracked, npx, eps, momentum)


# ---- the coefficient network's tensors: their order, stated once ----------------------------------------------------
# The network's tensors travel between ``models._Coefficients``, the four ctypes structs of ``_lib`` and the C ABI as ONE
# flat list, in the order of ``_coeff_slots``: layer by layer (splat x n_splat, global conv x 2, fc x 3, local1, local2,
# prediction) the weight, then the layer's second tensor -- its bias or, where batch norm normalises the layer, beta (such
# a layer has no bias).  local2 has a weight only.  The normalised layers are splat 1 and up, both global convs, fc1, fc2
# and local1: ``models._Coefficients._bn_layers()`` names the same layers in the same order, which is also the order of
# the running statistics.  ``models._Coefficients._train_params_bn()`` builds the list from the module; everything below
# reads it through ``_coeff_fill``, and the network without batch norm is the one in which no layer is normalised.
@functools.lru_cache(maxsize=None)
def _coeff_slots(n_splat: int, bn: bool = False):
    """``(group, index, field)`` of every tensor of the list, ``field`` one of ``w``, ``b``, ``beta``."""
    layers = ([("splat", i, i > 0) for i in range(n_splat)] + [("global_conv", i, True) for i in range(2)]
              + [("fc", i, i < 2) for i in range(3)] + [("local", 0, True), ("local", 1, None), ("pred", 0, False)])
    slots = []
    for group, i, normalised in layers:
        slots.append((group, i, "w"))
        if normalised is not None:  # (None: local2, the reference's use_bias=False)
            slots.append((group, i, "beta" if bn and normalised else "b"))
    return tuple(slots)


@functools.lru_cache(maxsize=None)
def _coeff_members(n_splat: int, bn: bool, with_stats: bool):
    """Where the four structs of ``_lib`` keep each tensor of the list: ``(member, element)``, ``element`` None where the
    member is no array -- ``pred_w``, ``pred_b``, ``local_beta``, ``local_running_mean``, ``local_running_var``.
    ``with_stats``: followed by the same for running_mean and running_var of each normalised layer."""
    def member(group, i, field):
        return f"{group}_{field}", None if group == "pred" or (group == "local" and field not in ("w", "b")) else i

    slots = _coeff_slots(n_splat, bn)
    stats = [(group, i, what) for group, i, field in slots if field == "beta" for what in ("running_mean", "running_var")]
    return tuple(member(*slot) for slot in list(slots) + (stats if with_stats else []))


def _coeff_fill(struct, n_splat: int, tensors, bn: bool = False, stats=None):
    """Write the addresses of ``tensors``, a list in ``_coeff_slots``' order, into ``struct`` -- a ``_lib.CoeffNet``,
    ``CoeffNetBn``, ``CoeffNetGrads`` or ``CoeffNetBnGrads`` -- and, for a ``CoeffNetBn``, those of ``stats``:
    ``(running_mean, running_var)`` per normalised layer.  What the network does not use stays null."""
    if stats is not None:
        tensors = [*tensors, *(t for st in stats for t in st)]
    for (member, element), t in zip(_coeff_members(n_splat, bn, stats is not None), tensors):
        address = None if t is None else t.data_ptr()
        if element is None:
            setattr(struct, member, address)
        else:
            getattr(struct, member)[element] = address
    return struct


def _coeff_struct(cls, hyper, n_out: int, n_in: int, n_levels: int, fc_layout: int):
    net = cls()
    net.net_input_size, net.spatial_bin = int(hyper["net_input_size"]), int(hyper["spatial_bin"])
    net.luma_bins, net.channel_multiplier = int(hyper["luma_bins"]), int(hyper["channel_multiplier"])
    net.n_out, net.n_in, net.n_levels, net.fc_layout = int(n_out), int(n_in), int(n_levels), int(fc_layout)
    return net


class CoefficientWeights:
    """The coefficient network's parameters in the layout ``hdrnet_coefficients_f32`` reads
    (include/hdrnet_amd.h): convolutions ``[Cout][kh][kw][Cin]``, fully connected layers ``[in][out]``,
    batch norm folded, fp32, contiguous, on one device.  Holds the tensors alive next to the C struct.

    ``params``: net_input_size, spatial_bin, luma_bins, channel_multiplier (hdrnet/bin/train.py:227-236);
    ``splat`` / ``global_conv`` / ``fc`` / ``local``: lists of ``(weight, bias)`` (bias ``None`` for the second
    local conv, the reference's ``use_bias=False``); ``pred``: ``(weight, bias)``.
    """

    def __init__(self, params, n_out: int, n_in: int, n_levels: int, splat, global_conv, fc, local, pred):
        self.params = dict(params)
        self.n_out, self.n_in, self.n_levels = int(n_out), int(n_in), int(n_levels)
        splat, global_conv, fc, local = list(splat), list(global_conv), list(fc), list(local)
        if len(global_conv) != 2 or len(fc) != 3 or len(local) != 2 or not 1 <= len(splat) <= 8:
            raise ValueError("coefficient network: 1-8 splat layers, 2 global convs, 3 fc layers, 2 local convs")
        if local[1][1] is not None:
            raise ValueError("coefficient network: the second local conv has no bias")
        self.device = pred[0].device
        self._keep = []

        def prep(t):
            if t is None:
                return None
            if t.dtype != torch.float32:
                raise ValueError(f"coefficient network parameters must be float32, got {t.dtype}")
            if t.device != self.device:
                raise ValueError("coefficient network parameters must live on one device")
            t = t.detach().contiguous()
            self._keep.append(t)
            return t

        pairs = splat + global_conv + fc + [local[0], local[1][:1], pred]
        self.net = _coeff_fill(_coeff_struct(_lib.CoeffNet, self.params, self.n_out, self.n_in, self.n_levels, 0),
                               len(splat), [prep(t) for pair in pairs for t in pair])
        self.n_splat = len(splat)

    def supported(self, batch: int = 1) -> bool:
        """False: hyper-parameters outside the kernels' reach (run the stock-op graph instead)."""
        return _lib.load().hdrnet_coefficients_workspace_bytes(ctypes.byref(self.net), int(batch)) > 0


def coefficients(lowres_input: torch.Tensor, weights: CoefficientWeights) -> torch.Tensor:
    """``HDRNetCurves._coefficients`` (hdrnet/models.py:62-142) in inference mode, on the HIP kernels of
    csrc/coeff_net.hip: ``lowres_input [B, N, N, 3]`` -> ``[B, sb, sb, gd, n_out, n_in]`` (``n_levels`` > 1:
    ``[n_levels, B, sb, sb, gd, n_out / n_levels, n_in]``, every level's grid contiguous).  No autograd."""
    _require_f32("lowres_input", lowres_input)
    if lowres_input.dim() != 4 or lowres_input.shape[3] != 3:
        raise ValueError(f"lowres_input should be [batch, N, N, 3], got {tuple(lowres_input.shape)}")
    _require_gpu("lowres_input", lowres_input)
    p = weights.params
    N, sb, gd = int(p["net_input_size"]), int(p["spatial_bin"]), int(p["luma_bins"])
    if lowres_input.shape[1] != N or lowres_input.shape[2] != N:
        raise ValueError(f"lowres_input is {tuple(lowres_input.shape[1:3])}, the network was built for {N} x {N}")
    if lowres_input.device != weights.device:
        raise ValueError("lowres_input and the network parameters live on different devices")
    low = lowres_input.detach().contiguous()
    B, dev = low.shape[0], low.device
    L = weights.n_levels
    shape = (B, sb, sb, gd, weights.n_out // L, weights.n_in)
    out = torch.empty((L,) + shape if L > 1 else shape, dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws, wbytes = _workspace(lib.hdrnet_coefficients_workspace_bytes, ctypes.byref(weights.net), B, device=dev)
        rc = lib.hdrnet_coefficients_f32(low.data_ptr(), ctypes.byref(weights.net), out.data_ptr(), B,
                                         ws.data_ptr(), wbytes, _stream(dev))
    _lib.check(rc, "Coefficients")
    return out


def _live_net_bn(hyper, n_out: int, n_in: int, params, n_splat: int, stats, eps: float, momentum: float):
    """``hdrnet_coeff_net_bn`` over the module's LIVE parameters and buffers (no copies): Conv2d weights must be in
    channels_last memory order (= [Cout][kh][kw][Cin]), Linear weights are taken as they are (fc_layout = 1).  ``params``
    in ``_coeff_slots``' order with batch norm; ``stats``: ``(running_mean, running_var)`` of the normalised layers in the
    same order.  ``stats = None``: the plain ``hdrnet_coeff_net`` of the network without batch norm."""
    bn = stats is not None
    net = _coeff_struct(_lib.CoeffNetBn if bn else _lib.CoeffNet, hyper, n_out, n_in, 1, 1)
    if bn:
        net.eps, net.momentum = float(eps), float(momentum)
    return _coeff_fill(net, n_splat, params, bn, stats)


def _live_net(hyper, n_out: int, n_in: int, params, n_splat: int):
    """``hdrnet_coeff_net`` over the LIVE parameters of a network without batch norm, ``params`` in ``_coeff_slots``' order."""
    return _live_net_bn(hyper, n_out, n_in, params, n_splat, None, 0.0, 0.0)


def _params_ok(params) -> bool:
    for p in params:
        if p.dtype != torch.float32 or not p.is_cuda:
            return False
        if p.dim() == 4:
            if not p.is_contiguous(memory_format=torch.channels_last):
                return False
        elif not p.is_contiguous():
            return False
    return True


# The coefficient network's training entry points take batches up to 8; their ``..._wide`` twins
# (include/hdrnet_amd_coeff_wide.h) up to 32, with the same arguments and, up to 8, the same launches.  The forward
# without batch norm is the inference one, which has no twin: it takes 32 images as it is.
_COEFF_NARROW_BATCH = 8
_COEFF_WIDE = {
    "hdrnet_coefficients_grad_workspace_bytes": "hdrnet_coefficients_grad_wide_workspace_bytes",
    "hdrnet_coefficients_grad_f32": "hdrnet_coefficients_grad_wide_f32",
    "hdrnet_coefficients_bn_workspace_bytes": "hdrnet_coefficients_bn_wide_workspace_bytes",
    "hdrnet_coefficients_bn_train_f32": "hdrnet_coefficients_bn_train_wide_f32",
    "hdrnet_coefficients_bn_grad_workspace_bytes": "hdrnet_coefficients_bn_grad_wide_workspace_bytes",
    "hdrnet_coefficients_bn_grad_f32": "hdrnet_coefficients_bn_grad_wide_f32",
}
# batch norm? -> (forward's workspace query, forward, its label; the gradient's workspace query, gradient, its label)
_COEFF_TRAIN = {
    False: ("hdrnet_coefficients_workspace_bytes", "hdrnet_coefficients_f32", "Coefficients",
            "hdrnet_coefficients_grad_workspace_bytes", "hdrnet_coefficients_grad_f32", "CoefficientsGrad"),
    True: ("hdrnet_coefficients_bn_workspace_bytes", "hdrnet_coefficients_bn_train_f32", "CoefficientsBnTrain",
           "hdrnet_coefficients_bn_grad_workspace_bytes", "hdrnet_coefficients_bn_grad_f32", "CoefficientsBnGrad"),
}


def _coeff_entry(lib, name: str, batch: int):
    """The training entry point ``name`` for this batch: itself up to 8 images, its wide twin (if it has one) above."""
    return getattr(lib, name if int(batch) <= _COEFF_NARROW_BATCH else _COEFF_WIDE.get(name, name))


def coefficients_train_supported(hyper, n_out: int, n_in: int, params, n_splat: int, batch: int) -> bool:
    """True if ``coefficients_train`` can run this network (no batch norm is the caller's business): parameters fp32 on
    the GPU in torch's own layouts, hyper-parameters within the kernels' reach, 1 <= batch <= 32."""
    params = list(params)
    if len(params) != len(_coeff_slots(n_splat)) or not _params_ok(params):
        return False
    net = _live_net(hyper, n_out, n_in, params, n_splat)
    query = _coeff_entry(_lib.load(), "hdrnet_coefficients_grad_workspace_bytes", batch)
    return query(ctypes.byref(net), int(batch)) > 0


def _grad_out(p: torch.Tensor) -> torch.Tensor:
    """Where a kernel-computed gradient of parameter ``p`` goes: a fresh alias of the parameter's segment of a flat
    gradient bucket (``dist.GradBucket`` registers it) while ``.grad`` is released -- autograd ASSIGNS a gradient it is
    handed when ``.grad`` is None, adopting the alias, so the bucket's gather has nothing to copy for this parameter --
    otherwise (no bucket, ``.grad`` bound: accumulation, or the segment already handed out since the release: the parameter
    is used twice and autograd must ADD the second gradient) a new tensor in the parameter's layout.

    That autograd adopts (rather than copies) a gradient it is handed for a leaf whose ``.grad`` is None is PyTorch's current
    behaviour, not a documented contract.  Nothing here depends on it for correctness: should a version copy instead,
    ``.grad`` is a tensor of its own holding the same values, and ``GradBucket.gather()`` -- which compares data pointers,
    not flags -- copies it into the segment as it does for every gradient autograd computed itself; the only loss is the
    copy this alias saves (``tests/test_coeff_net.py`` asserts the adopted case so that a change is noticed)."""
    v = getattr(p, "_hdrnet_grad_view", None)
    if (v is not None and p.grad is None and not getattr(p, "_hdrnet_grad_claimed", True) and v.device == p.device
            and v.dtype == p.dtype and v.shape == p.shape and v.stride() == p.stride()):
        p._hdrnet_grad_claimed = True
        return v.detach()
    return torch.empty_like(p)  # preserve_format: channels_last weights get channels_last grads


class _CoefficientsTrain(torch.autograd.Function):
    """The coefficient network on its live parameters, for training.  Without batch norm (``stats = None``): forward = the
    inference launch sequence, its workspace kept; backward = ``hdrnet_coefficients_grad_f32`` (csrc/coeff_net_train.hip).
    With batch norm in training mode: ``hdrnet_coefficients_bn_train_f32`` / ``hdrnet_coefficients_bn_grad_f32``
    (csrc/coeff_net_bn.hip between the launches of coeff_net.hip / coeff_net_train.hip), which move the running
    statistics of ``stats`` in place.  Above 8 images the ``..._wide`` twins (``_coeff_entry``)."""

    @staticmethod
    def forward(ctx, lowres, hyper, n_out, n_in, n_splat, stats, eps, momentum, *params):
        low = lowres.detach().contiguous()
        B, dev = low.shape[0], low.device
        net = _live_net_bn(hyper, n_out, n_in, params, n_splat, stats, eps, momentum)
        sb, gd = int(hyper["spatial_bin"]), int(hyper["luma_bins"])
        out = torch.empty((B, sb, sb, gd, n_out, n_in), dtype=torch.float32, device=dev)
        query, run, label = _COEFF_TRAIN[stats is not None][:3]
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws, wbytes = _workspace(_coeff_entry(lib, query, B), ctypes.byref(net), B, device=dev)
            rc = _coeff_entry(lib, run, B)(low.data_ptr(), ctypes.byref(net), out.data_ptr(), B, ws.data_ptr(), wbytes,
                                           _stream(dev))
        _lib.check(rc, label)
        for st in stats or ():
            for t in st:  # written through a raw pointer: tell autograd / the fold caches keyed on ._version
                torch.autograd.graph.increment_version(t)
        ctx.save_for_backward(low, ws, *params)
        ctx.stats = stats  # (the backward reads none of them: the struct wants their addresses)
        ctx.meta = (dict(hyper), int(n_out), int(n_in), int(n_splat), float(eps), float(momentum))
        return out

    @staticmethod
    def backward(ctx, dcoeffs):
        low, ws, *params = ctx.saved_tensors
        hyper, n_out, n_in, n_splat, eps, momentum = ctx.meta
        bn = ctx.stats is not None
        B, dev = low.shape[0], low.device
        net = _live_net_bn(hyper, n_out, n_in, params, n_splat, ctx.stats, eps, momentum)
        grads = [_grad_out(p) for p in params]
        gr = _coeff_fill(_lib.CoeffNetBnGrads() if bn else _lib.CoeffNetGrads(), n_splat, grads, bn)
        dc = dcoeffs.contiguous()
        query, run, label = _COEFF_TRAIN[bn][3:]
        lib = _lib.load()
        with torch.cuda.device(dev):
            ws2, wbytes = _workspace(_coeff_entry(lib, query, B), ctypes.byref(net), B, device=dev)
            rc = _coeff_entry(lib, run, B)(
                low.data_ptr(), ctypes.byref(net), ws.data_ptr(), dc.data_ptr(), ctypes.byref(gr), B, ws2.data_ptr(), wbytes,
                _stream(dev))
        _lib.check(rc, label)
        return (None, None, None, None, None, None, None, None, *grads)


class _CoefficientsBnTrain(_CoefficientsTrain):
    """The same function under a name of its own: the autograd graph then says which of the two paths a step took."""


def coefficients_train(lowres_input: torch.Tensor, hyper, n_out: int, n_in: int, params, n_splat: int) -> torch.Tensor:
    """``HDRNetCurves._coefficients`` (hdrnet/models.py:62-142) WITHOUT batch norm, differentiable in its parameters:
    forward and backward on the HIP kernels of csrc/coeff_net.hip / coeff_net_train.hip, reading the parameters and
    writing their gradients in torch's own layouts.  ``lowres_input [B, N, N, 3]`` (no gradient) ->
    ``[B, sb, sb, gd, n_out, n_in]``."""
    _require_f32("lowres_input", lowres_input)
    _require_gpu("lowres_input", lowres_input)
    return _CoefficientsTrain.apply(lowres_input, hyper, n_out, n_in, n_splat, None, 0.0, 0.0, *params)


def coefficients_bn_train_supported(hyper, n_out: int, n_in: int, params, n_splat: int, stats, batch: int) -> bool:
    """True if ``coefficients_bn_train`` can run this network: parameters and running statistics fp32 on the GPU in
    torch's own layouts, hyper-parameters within the kernels' reach, 2 <= batch <= 32."""
    params, stats = list(params), [tuple(st) for st in stats]
    slots = _coeff_slots(n_splat, True)
    if len(params) != len(slots) or len(stats) != sum(field == "beta" for _, _, field in slots) or not _params_ok(params):
        return False
    if not _params_ok([t for st in stats for t in st]):
        return False
    net = _live_net_bn(hyper, n_out, n_in, params, n_splat, stats, 1e-3, 1e-3)
    lib = _lib.load()
    return (_coeff_entry(lib, "hdrnet_coefficients_bn_workspace_bytes", batch)(ctypes.byref(net), int(batch)) > 0
            and _coeff_entry(lib, "hdrnet_coefficients_bn_grad_workspace_bytes", batch)(ctypes.byref(net), int(batch)) > 0)


def coefficients_bn_train(lowres_input: torch.Tensor, hyper, n_out: int, n_in: int, params, n_splat: int, stats,
                          eps: float = 1e-3, momentum: float = 1e-3) -> torch.Tensor:
    """``HDRNetCurves._coefficients`` (hdrnet/models.py:62-142) WITH batch norm in training mode (``--batch_norm``,
    hdrnet/layers.py:30-54), differentiable in its weights, biases and betas, on the HIP kernels; moves the running
    statistics of ``stats`` in place.  ``params`` / ``stats`` as ``_live_net_bn`` takes them.  ``lowres_input [B, N, N, 3]``
    (no gradient, 2 <= B <= 32) -> ``[B, sb, sb, gd, n_out, n_in]``."""
    _require_f32("lowres_input", lowres_input)
    _require_gpu("lowres_input", lowres_input)
    stats = tuple(tuple(st) for st in stats)
    return _CoefficientsBnTrain.apply(lowres_input, hyper, n_out, n_in, n_splat, stats, eps, momentum, *params)


def resize_bilinear(input: torch.Tensor, height: int, width: int) -> torch.Tensor:  # noqa: A002
    """NHWC ``tf.image.resize_images(input, (height, width), BILINEAR, align_corners=True)`` --
    the resize that builds HDRNetGaussianPyrNN's multi-scale input (hdrnet/models.py:253-266).
    No autograd."""
    _require_f32("input", input)
    if input.dim() != 4:
        raise ValueError(f"input should be 4D (batch, height, width, channels), got {tuple(input.shape)}")
    _require_gpu("input", input)
    inp = input.detach().contiguous()
    B, Hin, Win, C = inp.shape
    out = torch.empty((B, int(height), int(width), C), dtype=torch.float32, device=inp.device)
    lib = _lib.load()
    with torch.cuda.device(inp.device):
        rc = lib.hdrnet_resize_bilinear_f32(inp.data_ptr(), out.data_ptr(), B, Hin, Win, int(height),
                                            int(width), C, _stream(inp.device))
    _lib.check(rc, "ResizeBilinear")
    return out


class _UpsampleAdd(torch.autograd.Function):
    """``resize(coarse -> fine's size, bilinear, align_corners) + fine`` in one pass; backward: d fine = the incoming gradient
    itself, d coarse = the resize's transpose as a fixed-order gather (csrc/resize_bilinear.hip)."""

    @staticmethod
    def forward(ctx, coarse, fine):
        c, f = coarse.detach().contiguous(), fine.detach().contiguous()
        B, IH, IW, C = c.shape
        OH, OW = f.shape[1], f.shape[2]
        out = torch.empty_like(f)
        with torch.cuda.device(f.device):
            rc = _lib.load().hdrnet_resize_add_f32(c.data_ptr(), f.data_ptr(), out.data_ptr(), B, IH, IW, OH, OW, C,
                                                   _stream(f.device))
        if rc != 0:
            raise RuntimeError(f"hdrnet_resize_add_f32 failed (rc={rc}): {_lib.last_error()}")
        ctx.dims = (B, IH, IW, OH, OW, C)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        B, IH, IW, OH, OW, C = ctx.dims
        g = grad.contiguous()
        dcoarse = None
        if ctx.needs_input_grad[0]:
            dcoarse = torch.empty((B, IH, IW, C), dtype=torch.float32, device=g.device)
            with torch.cuda.device(g.device):
                rc = _lib.load().hdrnet_resize_bilinear_grad_f32(g.data_ptr(), dcoarse.data_ptr(), B, IH, IW, OH, OW, C,
                                                                 _stream(g.device))
            if rc != 0:
                raise RuntimeError(f"hdrnet_resize_bilinear_grad_f32 failed (rc={rc}): {_lib.last_error()}")
        return dcoarse, (g if ctx.needs_input_grad[1] else None)


def upsample_add(coarse: torch.Tensor, fine: torch.Tensor) -> torch.Tensor:
    """``tf.image.resize_images(coarse, fine's size, BILINEAR, align_corners=True) + fine`` -- the up-add of
    HDRNetGaussianPyrNN's output pyramid (hdrnet/models.py:283-287) -- NHWC fp32 on the GPU, differentiable in both."""
    for name, t in (("coarse", coarse), ("fine", fine)):
        _require_f32(name, t)
        _require_gpu(name, t)
    if coarse.dim() != 4 or fine.dim() != 4 or coarse.shape[0] != fine.shape[0] or coarse.shape[3] != fine.shape[3]:
        raise ValueError(f"upsample_add: [B, h, w, C] and [B, H, W, C] expected, got {tuple(coarse.shape)}, {tuple(fine.shape)}")
    return _UpsampleAdd.apply(coarse, fine)


def bilateral_slice_apply_upadd(grid: torch.Tensor, input: torch.Tensor, coarse: torch.Tensor,  # noqa: A002
                                guide: Optional[torch.Tensor] = None,
                                guide_conv1: Optional[torch.Tensor] = None,
                                guide_conv2: Optional[torch.Tensor] = None,
                                has_offset: bool = True, fast_sigmoid: bool = False,
                                prescaled: bool = False) -> torch.Tensor:
    """One level of ``HDRNetGaussianPyrNN._output`` (hdrnet/models.py:277-289) in one pass:
    ``bilateral_slice_apply(grid, guide, input) + resize_bilinear(coarse -> H x W, align_corners)``.
    Give either a ``guide`` map or the folded guide network (``guide_conv1``, ``guide_conv2``), which
    is then evaluated in registers (``fast_sigmoid``, ``prescaled``: as ``bilateral_slice_apply_nnguide``).  Inference
    only (no autograd)."""
    if (guide is None) == (guide_conv1 is None):
        raise ValueError("give either guide or (guide_conv1, guide_conv2)")
    if input.dim() != 4:
        raise ValueError(f"Input image should be 4D (batch_size, height, width, input_channels), got {tuple(input.shape)}")
    if guide is None:
        B, H, W, GH, GW, GD, Cin, Cout, n = _check_nnguide(grid, input, guide_conv1, guide_conv2, has_offset)
    else:
        B, H, W, GH, GW, GD, Cin, Cout = _check_apply(grid, guide, input, has_offset)
        n = 0
    _require_f32("coarse", coarse)
    _require_gpu("coarse", coarse)
    if coarse.dim() != 4 or coarse.shape[0] != B or coarse.shape[3] != Cout:
        raise ValueError(f"coarse should be [B, Hc, Wc, Cout] = [{B}, *, *, {Cout}], got {tuple(coarse.shape)}")
    grid, inp, coarse = grid.detach().contiguous(), input.detach().contiguous(), coarse.detach().contiguous()
    gd = None if guide is None else guide.detach().contiguous()
    c1 = None if guide_conv1 is None else guide_conv1.detach().contiguous()
    c2 = None if guide_conv2 is None else guide_conv2.detach().contiguous()
    dev = inp.device
    out = torch.empty((B, H, W, Cout), dtype=torch.float32, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        rc = lib.hdrnet_bilateral_slice_apply_upadd_f32_ex(
            grid.data_ptr(), _ptr(gd), inp.data_ptr(), coarse.data_ptr(), coarse.shape[1], coarse.shape[2],
            out.data_ptr(), B, H, W, GH, GW, GD, Cin, Cout, int(bool(has_offset)), _ptr(c1), _ptr(c2), n,
            _guide_flags(fast_sigmoid, prescaled and guide is None), _stream(dev))
    _lib.check(rc, "BilateralSliceApplyUpAdd")
    return out


_DTYPE_CODE = {torch.float32: 0, torch.uint8: 1, torch.uint16: 2}
_DEFAULT_WHITE = {torch.float32: 1.0, torch.uint8: 255.0, torch.uint16: 65535.0}


def _frame_head(input, white_level, out_dtype=torch.float32, rank_text=None):  # noqa: A002
    """What every op on a wire-format frame asks first: rank 4, float32 / uint8 / uint16, ``out_dtype`` float32 or
    uint8.  Returns the white level: the dtype's default where None."""
    if not isinstance(input, torch.Tensor) or input.dim() != 4:
        raise ValueError(rank_text or "Input image should be 4D (batch_size, height, width, input_channels), got "
                         f"{tuple(input.shape) if isinstance(input, torch.Tensor) else type(input).__name__}")
    if input.dtype not in _DTYPE_CODE:
        raise TypeError(f"input must be float32, uint8 or uint16, got {input.dtype}")
    if out_dtype not in (torch.float32, torch.uint8):
        raise TypeError(f"out_dtype must be float32 or uint8, got {out_dtype}")
    return _DEFAULT_WHITE[input.dtype] if white_level is None else white_level


def _check_io(grid, input, has_offset, pixel_format="rgb"):  # noqa: A002
    """Batch / channel rules shared by the wire-format entry points (the OP_REQUIRES of
    bilateral_slice_apply_op.cc:147-193 on an input that ``_frame_head`` has passed), for a frame in ``pixel_format``: the
    op sees three channels whatever another format than RGB stores.  Returns (B, H, W, GH, GW, GD, Cin, Cout)."""
    _require_f32("grid", grid)
    if grid.dim() != 5:
        raise ValueError(f"Input grid should be 5D, got {tuple(grid.shape)}")
    B, H, W, Cin = input.shape
    if pixel_format != "rgb":
        Cin = min(Cin, 3)
    if grid.shape[0] != B:
        raise ValueError("Batch sizes should match.")
    GH, GW, GD, C = grid.shape[1:]
    Cj = Cin + (1 if has_offset else 0)
    if Cj <= 0 or C % Cj:
        raise ValueError(
            "Slicing with affine offset, grid should have output_channels * (input_channels + 1) channels."
            if has_offset else
            "Slicing without affine offset, grid should have output_channels * input_channels channels.")
    if pixel_format != "rgb" and ((Cin, C // Cj) != (3, 3) or not has_offset):
        raise ValueError(f"pixel_format={pixel_format!r} needs the 3 -> 3 op with offset (a [.., 12] grid), got Cout = {C // Cj}, "
                         f"has_offset = {bool(has_offset)}")
    return B, H, W, GH, GW, GD, Cin, C // Cj


_ONE_GUIDE = "give exactly one of guide, (guide_conv1, guide_conv2), guide_curves"
_MAP_OR_NETWORK = "give either a guide map or both guide_conv1 and guide_conv2"


def _guide_source(guide, guide_conv1, guide_conv2, guide_curves, curves_prepared, return_guide, bhw, Cin,
                  map_or_network=_MAP_OR_NETWORK, lone_conv_ok=True, prepared_name="prepared"):
    """The guide of a wire-format forward: exactly one of a ``guide`` map, the guide network (``guide_conv1``,
    ``guide_conv2``) and ``guide_curves`` (with ``curves_prepared``), checked against the frame's ``bhw`` and ``Cin``.
    Returns ``(False, (guide map, None, None), 0)``, ``(False, (None, guide_conv1, guide_conv2), n)`` or ``(True, (ccm,
    shifts, slopes, mix, curves_prepared), npts)`` -- whether to call the curves entry points, the tensors detached and
    contiguous in the order those take them, and the feature / knot count.  ``map_or_network``: the caller's wording for
    neither or both of the first two; ``lone_conv_ok``: half a network beside a map is ignored (the map wins, as in the C
    ABI) rather than refused; ``prepared_name``: what the caller calls ``curves_prepared``."""
    half = (guide_conv1 is None) != (guide_conv2 is None)
    n_given = sum(x is not None for x in (guide, guide_curves)) + int(guide_conv1 is not None and guide_conv2 is not None)
    if guide_curves is not None and (n_given != 1 or half):
        raise ValueError(_ONE_GUIDE)
    if n_given != 1 or (half and not lone_conv_ok):
        raise ValueError(map_or_network)
    if return_guide and guide is not None:
        raise ValueError("return_guide needs a guide computed by the kernel (guide network or guide_curves)")
    if guide is not None:
        _require_f32("guide", guide)
        if tuple(guide.shape) != tuple(bhw):
            raise ValueError("Input and guide size should match.")
        _require_gpu("guide", guide)
        return False, (guide.detach().contiguous(), None, None), 0
    if guide_curves is None:
        _require_f32("guide_conv1", guide_conv1)
        _require_f32("guide_conv2", guide_conv2)
        n = guide_conv1.shape[0]
        if guide_conv1.dim() != 2 or guide_conv1.shape[1] != Cin + 1 or tuple(guide_conv2.shape) != (n + 1,):
            raise ValueError("guide_conv1 should be [n, Cin + 1] and guide_conv2 [n + 1]")
        return False, (None, guide_conv1.detach().contiguous(), guide_conv2.detach().contiguous()), n
    if len(guide_curves) != 4:
        raise ValueError("guide_curves should be (ccm, shifts, slopes, mix)")
    shifts = guide_curves[1]
    npts = shifts.shape[0] if shifts.dim() == 2 else -1
    for nm, t, shape in zip(("ccm", "shifts", "slopes", "mix"), guide_curves,
                            ((Cin, Cin + 1), (npts, Cin), (npts, Cin), (Cin + 1,))):
        _require_f32(f"guide_curves.{nm}", t)
        if tuple(t.shape) != shape or npts <= 0:
            raise ValueError(f"guide_curves.{nm} should be {list(shape)}, got {list(t.shape)}")
    for nm, t in zip(("ccm", "shifts", "slopes", "mix"), guide_curves):
        _require_gpu(f"guide_curves.{nm}", t)
    if curves_prepared is not None:
        _require_f32(prepared_name, curves_prepared)
        _require_gpu(prepared_name, curves_prepared)
        if (not curves_prepared.is_contiguous()
                or curves_prepared.numel() * 4 < _lib.load().hdrnet_curves_guide_prepared_bytes(Cin)):
            raise ValueError(f"{prepared_name} should be the tensor curves_guide_prepare returned")
    return True, (*(t.detach().contiguous() for t in guide_curves), curves_prepared), npts


def curves_guide_prepare(shifts: torch.Tensor, slopes: torch.Tensor) -> Optional[torch.Tensor]:
    """The curves guide's lookup tables, PREPARED once per parameter set (``hdrnet_curves_guide_prepare_f32``; Cin = 3,
    at most 16 knots per channel): each channel's knot range cut into 64 uniform cells, per cell the knot inside it, the
    curve's float64-summed value there and the slopes on either side.  Passed to ``bilateral_slice_apply_curves`` /
    ``bilateral_slice_apply_io`` as ``prepared`` / ``curves_prepared``, a pixel finds its cell by arithmetic and reads ONE
    table entry, where the plain call has every workgroup sort the knots and every pixel walk a search tree.  Same guide to
    1e-6.  A SET-UP call: it waits for the stream (one word comes back -- whether the cells separate the knots) and must not
    run inside a stream capture.  Returns an opaque float32 tensor, or ``None`` when two knots of a channel share a cell
    (closer than 1/63 of the channel's knot range): call the ops without ``prepared`` then.  ``shifts`` / ``slopes``:
    ``[npts, 3]`` (hdrnet/bin/freeze_graph.py:107-127)."""
    _require_f32("shifts", shifts)
    _require_f32("slopes", slopes)
    _require_gpu("shifts", shifts)
    _require_gpu("slopes", slopes)
    if shifts.dim() != 2 or shifts.shape[1] != 3 or tuple(slopes.shape) != tuple(shifts.shape) or not 0 < shifts.shape[0] <= 16:
        raise ValueError(f"curves_guide_prepare: shifts / slopes [npts <= 16, 3] expected, got {tuple(shifts.shape)}, "
                         f"{tuple(slopes.shape)}")
    sh, sl = shifts.detach().contiguous(), slopes.detach().contiguous()
    dev = sh.device
    lib = _lib.load()
    nbytes = lib.hdrnet_curves_guide_prepared_bytes(3)
    out = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
    usable = ctypes.c_int(0)
    with torch.cuda.device(dev):
        rc = lib.hdrnet_curves_guide_prepare_f32(sh.data_ptr(), sl.data_ptr(), sh.shape[0], 3, out.data_ptr(), nbytes,
                                                 ctypes.byref(usable), _stream(dev))
    _lib.check(rc, "CurvesGuidePrepare")
    return out if usable.value else None


def _out_channels(pixel_format: str, out_dtype, Cout: int) -> int:
    """Channels of the output tensor: a uint8 / uint16 output has the input's pixel format, a float32 output is RGB."""
    return _lib.PIXEL_FORMAT_CHANNELS[pixel_format] if (pixel_format != "rgb" and out_dtype != torch.float32) else Cout


def _px_codes(pixel_format: str, out_dtype):
    """``(input_format, output_format)`` of the ..._px / ..._px_u16 entry points (HDRNET_PX_*)."""
    code = _lib.PIXEL_FORMATS[pixel_format]
    return code, (code if out_dtype != torch.float32 else _lib.PIXEL_FORMATS["rgb"])


def _output_white_level(value, what: str) -> float:
    """The white level of a uint16 output (include/hdrnet_amd_u16_out.h): finite, 0 < value <= 65535."""
    v = float(value)
    if not (0.0 < v <= 65535.0):  # (false for NaN)
        raise ValueError(f"{what}: output_white_level must be finite with 0 < output_white_level <= 65535, got {value!r}")
    return v


def _apply_io_frame(u16, grid, input, guide, guide_conv1, guide_conv2, input_white_level, out_dtype, has_offset,  # noqa: A002
                    guide_curves, return_guide, fast_sigmoid, prescaled, curves_prepared, pixel_format,
                    output_white_level=None):
    """The body of ``bilateral_slice_apply_io`` and (``u16``: ``out_dtype`` uint16, scaled to ``output_white_level``) of
    ``bilateral_slice_apply_io_u16``: the uint16 output's own rules stand beside the shared ones, in the order the C ABI
    checks them."""
    what = "bilateral_slice_apply_io_u16" if u16 else "bilateral_slice_apply_io"
    input_white_level = _frame_head(input, input_white_level, torch.float32 if u16 else out_dtype)
    if u16:
        if input.dtype == torch.uint8:
            raise TypeError(f"{what}: a uint16 output needs a uint16 or float32 frame, got uint8 (no kernel goes from 8 to 16 bits)")
        output_white_level = _output_white_level(output_white_level, what)
    plain = pixel_format == "rgb" and not u16  # the entry points without format codes: every rule is the one it always was
    if not plain:
        pixel_format = _lib.pixel_format(pixel_format, input.shape[3], input.dtype == torch.float32, what)
    B, H, W, GH, GW, GD, Cin, Cout = _check_io(grid, input, has_offset, pixel_format)
    if u16 and ((Cin, Cout) != (3, 3) or not has_offset):
        raise ValueError(f"{what}: the 3 -> 3 op with offset (a [.., 12] grid) only, got Cin = {Cin}, Cout = {Cout}, "
                         f"has_offset = {bool(has_offset)}")
    curves, g, n = _guide_source(guide, guide_conv1, guide_conv2, guide_curves, curves_prepared, return_guide, (B, H, W), Cin)
    _require_gpu("grid", grid)
    _require_gpu("input", input)
    grid, inp = grid.detach().contiguous(), input.detach().contiguous()
    dev = inp.device
    out = torch.empty((B, H, W, _out_channels(pixel_format, out_dtype, Cout)), dtype=out_dtype, device=dev)
    gout = torch.empty((B, H, W), dtype=torch.float32, device=dev) if return_guide else None
    frame = (inp.data_ptr(), out.data_ptr(), B, H, W, GH, GW, GD, Cin, Cout, int(bool(has_offset)),
             _DTYPE_CODE[input.dtype], float(input_white_level), output_white_level if u16 else _DTYPE_CODE[out_dtype])
    suffix = "_px_u16" if u16 else "_px" if not plain else "_prepared" if curves else "_ex"
    if curves:
        fn = "hdrnet_bilateral_slice_apply_io_curves" + suffix
        args = (grid.data_ptr(), *frame, *(t.data_ptr() for t in g[:4]), n, _ptr(g[4]), _ptr(gout))
    else:
        fn = "hdrnet_bilateral_slice_apply_io" + suffix
        args = (grid.data_ptr(), _ptr(g[0]), *frame, _ptr(g[1]), _ptr(g[2]), n, _ptr(gout),
                _guide_flags(fast_sigmoid, prescaled and g[0] is None))
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), fn)(*args, *(() if plain else _px_codes(pixel_format, out_dtype)), _stream(dev))
    _lib.check(rc, "BilateralSliceApplyIOCurves" if curves else "BilateralSliceApplyIO")
    return (out, gout) if return_guide else out


def bilateral_slice_apply_io(grid: torch.Tensor, input: torch.Tensor,  # noqa: A002
                             guide: Optional[torch.Tensor] = None,
                             guide_conv1: Optional[torch.Tensor] = None,
                             guide_conv2: Optional[torch.Tensor] = None,
                             input_white_level: Optional[float] = None,
                             out_dtype: torch.dtype = torch.float32,
                             has_offset: bool = True,
                             guide_curves: Optional[Tuple[torch.Tensor, ...]] = None,
                             return_guide: bool = False, fast_sigmoid: bool = False, prescaled: bool = False,
                             curves_prepared: Optional[torch.Tensor] = None, pixel_format: str = "rgb"):
    """Inference forward with the product's wire formats fused in: ``input`` may be uint8 / uint16
    (``value / input_white_level``: 255, 65535, or 32767 for HDR+ -- hdrnet/data_pipeline.py:202-232,
    :267-274) and the output may be uint8 ``= (uint8)(255 * clip(out, 0, 1))`` (hdrnet/bin/run.py:95).
    The guide is ONE of: a ``guide`` map; the folded point-wise guide network (``guide_conv1``,
    ``guide_conv2``); or ``guide_curves = (ccm [Cin, Cin+1], shifts [npts, Cin], slopes [npts, Cin],
    mix [Cin+1])``, the standard model's curves guide (hdrnet/models.py:145-190) in the layout
    hdrnet/bin/freeze_graph.py:107-127 exports -- then evaluated in registers, as the reference's
    standard GL shader does (benchmark/assets/std.frag:36-45).  ``return_guide`` (guide network or curves) also
    returns the guide map the kernel computed.  ``fast_sigmoid`` (guide network): the hardware exp / reciprocal
    sigmoid, <= 2 ulp of the guide away from the default (tf.nn.sigmoid's form) and ~10 % faster -- an explicit
    choice of the caller (HDRNET_GUIDE_SIGMOID_FAST), never implied by another argument.  ``prescaled`` (guide network):
    ``guide_conv1`` / ``guide_conv2`` are ``guide_nn_prescale``'s arrays (HDRNET_GUIDE_RELU_PRESCALED).
    ``curves_prepared`` (``guide_curves``): the tables of ``curves_guide_prepare``.  No autograd.

    ``pixel_format`` says how ``input`` stores a pixel (include/hdrnet_amd_pixel_formats.h): ``"rgb"`` (default),
    ``"bgr"``, ``"rgba"`` or ``"bgra"`` -- ``[B, H, W, 3 or 4]`` as OpenCV, decoders and display surfaces deliver frames.
    The op always sees R, G, B (a ``[.., 12]`` grid, the guide parameters in that order): the bytes are permuted in the
    kernel's load and store, with every guide source.  uint8 / uint16 frames take all four, float32 frames ``"rgb"``
    only.  A uint8 output has the input's format, with alpha carried over (the byte of a uint8 frame, ``alpha >> 8`` of a
    uint16 one: alpha is never divided by the white level or quantised); a float32 output is ``[B, H, W, 3]`` RGB.
    4-channel frames must be 16-byte aligned.  A uint16 frame out is ``bilateral_slice_apply_io_u16``'s.  Out of scope:
    float32 frames in other orders."""
    return _apply_io_frame(False, grid, input, guide, guide_conv1, guide_conv2, input_white_level, out_dtype, has_offset,
                           guide_curves, return_guide, fast_sigmoid, prescaled, curves_prepared, pixel_format)


def bilateral_slice_apply_io_u16(grid: torch.Tensor, input: torch.Tensor,  # noqa: A002
                                 guide: Optional[torch.Tensor] = None,
                                 guide_conv1: Optional[torch.Tensor] = None,
                                 guide_conv2: Optional[torch.Tensor] = None,
                                 input_white_level: Optional[float] = None,
                                 output_white_level: float = 65535.0,
                                 has_offset: bool = True,
                                 guide_curves: Optional[Tuple[torch.Tensor, ...]] = None,
                                 return_guide: bool = False, fast_sigmoid: bool = False, prescaled: bool = False,
                                 curves_prepared: Optional[torch.Tensor] = None, pixel_format: str = "rgb"):
    """``bilateral_slice_apply_io`` with a UINT16 frame out (include/hdrnet_amd_u16_out.h): per sample
    ``(uint16)(output_white_level * clip(out, 0, 1))`` -- one float32 multiply, then truncation: the uint8 store's rule
    with 255 replaced by ``output_white_level`` (finite, 0 < . <= 65535; 32767 for HDR+, 1023 for a 10-bit range).  The
    arithmetic before the store is that of ``bilateral_slice_apply_io`` on the same arguments, so the result equals its
    float32 output quantised by that rule, without the float32 frame.  ``input`` is uint16 (any ``pixel_format``) or
    float32 (``"rgb"``); the output has the input's pixel format, with the alpha of a uint16 frame copied bit for bit.
    Every other argument is ``bilateral_slice_apply_io``'s; the 3 -> 3 op with offset only.  No autograd.
    Out of scope: uint8 frames (no kernel goes from 8 to 16 bits), float32 frames in other orders, more than 16 curve
    knots on a BGR / RGBA / BGRA frame."""
    return _apply_io_frame(True, grid, input, guide, guide_conv1, guide_conv2, input_white_level, torch.uint16, has_offset,
                           guide_curves, return_guide, fast_sigmoid, prescaled, curves_prepared, pixel_format,
                           output_white_level)


# ---- semi-planar YUV 4:2:0 surfaces (include/hdrnet_amd_yuv.h) ------------------------------------------------------------
_YUV_SAMPLE = {torch.uint8: 1, torch.uint16: 2}


def _check_chroma(what: str, chroma, planar: bool) -> str:
    """The ``chroma`` keyword of the surface paths (include/hdrnet_amd_yuv_chroma.h): ``"420"`` (the default), ``"422"``, or
    -- planar surfaces only -- ``"444"``.  The layout is NAMED by the caller; it is never guessed from the plane shapes."""
    if chroma not in _lib.CHROMA:
        raise ValueError(f"{what}: unknown chroma {chroma!r} (takes '420', '422', '444')")
    if not planar and chroma == "444":
        raise ValueError(f"{what}: semi-planar 4:4:4 (NV24 / P410) is out of scope: 4:4:4 surfaces are planar "
                         "(yuv_planar_to_rgb, bilateral_slice_apply_io_yuv_planar, process_yuv_planar)")
    return chroma


def _yuv_surface(y, uv, what: str, names=("y", "uv"), chroma: str = "420"):
    """The rules of a surface, on the host: ``y`` ``[B, H, W]`` and ``uv`` ``[B, H / 2, W]`` (interleaved U, V; or
    ``[B, H / 2, W / 2, 2]``) of one dtype, uint8 or uint16, last-dimension stride 1, row stride >= W samples.  Returns
    ``(y, uv, B, H, W, (sample_dtype, pitch_y, pitch_uv, image_stride_y, image_stride_uv))``, pitches in bytes.
    ``chroma="422"`` (NV16 / P210 / P216): ``uv`` is ``[B, H, W]`` and H is any positive number."""
    ny, nuv = names
    if chroma != "420":
        return _yuv_surface_422(y, uv, what, names)
    for nm, t in ((ny, y), (nuv, uv)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {nm} must be a torch.Tensor, got {type(t).__name__}")
    if y.dim() != 3:
        raise ValueError(f"{what}: {ny} should be [B, H, W], got {tuple(y.shape)}")
    B, H, W = y.shape
    if uv.dim() == 4 and uv.shape[3] == 2 and uv.stride(3) == 1 and uv.stride(2) == 2:
        uv = uv.as_strided((uv.shape[0], uv.shape[1], 2 * uv.shape[2]), (uv.stride(0), uv.stride(1), 1))
    if y.dtype not in _YUV_SAMPLE or uv.dtype != y.dtype:
        raise TypeError(f"{what}: {ny} and {nuv} must both be uint8 (NV12) or uint16 (P010 / P016), got {y.dtype}, {uv.dtype}")
    if H % 2 != 0:
        raise ValueError(f"{what}: H must be even (a chroma row serves two image rows), got H = {H}")
    if W % 4 != 0:
        raise ValueError(f"{what}: W % 4 != 0 (W = {W})")
    if uv.dim() != 3 or tuple(uv.shape) != (B, H // 2, W):
        raise ValueError(f"{what}: {nuv} should be [B, H / 2, W] = {[B, H // 2, W]} (interleaved U, V), got {list(uv.shape)}")
    size = y.element_size()
    for nm, t in ((ny, y), (nuv, uv)):
        if B * H * W and (t.stride(2) != 1 or t.stride(1) < W or (t.stride(1) * size) % 4 or (t.stride(0) * size) % 4):
            raise ValueError(f"{what}: {nm} must have last-dimension stride 1, a row stride >= W samples and pitches that are "
                             f"multiples of 4 bytes, got strides {tuple(t.stride())}")
    return y, uv, B, H, W, (_YUV_SAMPLE[y.dtype], y.stride(1) * size, uv.stride(1) * size, y.stride(0) * size,
                            uv.stride(0) * size)


def _yuv_surface_422(y, uv, what: str, names):
    """``_yuv_surface`` for a semi-planar 4:2:2 surface: the same rules with a chroma row per image row."""
    ny, nuv = names
    for nm, t in ((ny, y), (nuv, uv)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {nm} must be a torch.Tensor, got {type(t).__name__}")
    if y.dim() != 3:
        raise ValueError(f"{what}: {ny} should be [B, H, W], got {tuple(y.shape)}")
    B, H, W = y.shape
    if uv.dim() == 4 and uv.shape[3] == 2 and uv.stride(3) == 1 and uv.stride(2) == 2:
        uv = uv.as_strided((uv.shape[0], uv.shape[1], 2 * uv.shape[2]), (uv.stride(0), uv.stride(1), 1))
    if y.dtype not in _YUV_SAMPLE or uv.dtype != y.dtype:
        raise TypeError(f"{what}: {ny} and {nuv} must both be uint8 (NV16) or uint16 (P210 / P216), got {y.dtype}, {uv.dtype}")
    if W % 4 != 0:
        raise ValueError(f"{what}: W % 4 != 0 (W = {W})")
    if uv.dim() != 3 or tuple(uv.shape) != (B, H, W):
        raise ValueError(f"{what}: chroma='422': {nuv} should be [B, H, W] = {[B, H, W]} (interleaved U, V, full height), got "
                         f"{list(uv.shape)}")
    size = y.element_size()
    for nm, t in ((ny, y), (nuv, uv)):
        if B * H * W and (t.stride(2) != 1 or t.stride(1) < W or (t.stride(1) * size) % 4 or (t.stride(0) * size) % 4):
            raise ValueError(f"{what}: {nm} must have last-dimension stride 1, a row stride >= W samples and pitches that are "
                             f"multiples of 4 bytes, got strides {tuple(t.stride())}")
    return y, uv, B, H, W, (_YUV_SAMPLE[y.dtype], y.stride(1) * size, uv.stride(1) * size, y.stride(0) * size,
                            uv.stride(0) * size)


def _yuv_constants(name: str, t, what: str) -> torch.Tensor:
    _require_f32(name, t)
    if t.numel() != 12:
        raise ValueError(f"{what}: {name} should hold 12 floats (yuv.yuv_coefficients), got {tuple(t.shape)}")
    return t


def yuv_to_rgb(y: torch.Tensor, uv: torch.Tensor, to_rgb: torch.Tensor, chroma: str = "420") -> torch.Tensor:
    """A semi-planar YUV 4:2:0 surface -> float32 ``[B, H, W, 3]`` RGB in [0, 1] (``hdrnet_yuv_to_rgb_f32``): ``y``
    ``[B, H, W]``, ``uv`` ``[B, H / 2, W]`` (interleaved), uint8 (NV12) or uint16 (P010 / P016); ``to_rgb`` the 12 floats of
    ``yuv.yuv_coefficients`` on the device.  Chroma is replicated over its 2 x 2 block; the result is clamped.  Planes may
    be pitched (row stride > W); padding is not read.  The yardstick of ``bilateral_slice_apply_io_yuv``.  No autograd.
    ``chroma="422"`` (include/hdrnet_amd_yuv_chroma.h): an NV16 / P210 / P216 surface, ``uv`` ``[B, H, W]``, any H; chroma
    sample ``(y, x >> 1)`` serves its horizontal pair."""
    what = "yuv_to_rgb"
    chroma = _check_chroma(what, chroma, False)
    y, uv, B, H, W, surf = _yuv_surface(y, uv, what, chroma=chroma)
    to_rgb = _yuv_constants("to_rgb", to_rgb, what)
    for nm, t in (("y", y), ("uv", uv), ("to_rgb", to_rgb)):
        _require_gpu(nm, t)
    dev = y.device
    k = to_rgb.detach().contiguous()
    out = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if chroma != "420":
            rc = _lib.load().hdrnet_yuv_chroma_to_rgb_f32(y.data_ptr(), uv.data_ptr(), *surf, _lib.CHROMA[chroma], B, H, W,
                                                          k.data_ptr(), out.data_ptr(), _stream(dev))
        else:
            rc = _lib.load().hdrnet_yuv_to_rgb_f32(y.data_ptr(), uv.data_ptr(), *surf, B, H, W, k.data_ptr(), out.data_ptr(),
                                                   _stream(dev))
    _lib.check(rc, "YuvToRgb")
    return out


def _apply_io_surface(what, surface_dtype, out_dtype, grid, y, uv, to_rgb, guide, guide_conv1, guide_conv2, guide_curves,
                      return_guide, fast_sigmoid, prescaled, curves_prepared, from_rgb, out_planes, out_bits=None,
                      chroma: str = "420", coarse=None):
    """The body of ``bilateral_slice_apply_io_yuv`` and ``bilateral_slice_apply_io_yuv_deep`` (``what``), once each has
    checked the arguments that say what comes out.  ``surface_dtype``: None for an RGB frame of ``out_dtype``, uint8 for an
    NV12 surface, uint16 for a P010 / P016 surface of ``out_bits`` from a uint16 surface.  ``coarse``: the call is
    ``bilateral_slice_apply_upadd_io_yuv`` (4:2:0, a guide map or the network): the coarser pyramid level to up-add."""
    deep = surface_dtype == torch.uint16
    y, uv, B, H, W, surf = _yuv_surface(y, uv, what, chroma=chroma)
    if deep and y.dtype != torch.uint16:
        raise TypeError(f"{what}: a {'P010 / P016' if chroma == '420' else 'P210 / P216'} output needs a uint16 surface in, got "
                        f"{y.dtype} (no kernel goes from 8 to 16 bits)")
    to_rgb = _yuv_constants("to_rgb", to_rgb, what)
    if deep:  # (names its encode constants before the grid; the NV12 output after it)
        from_rgb = _yuv_constants("from_rgb", from_rgb, what)
    _require_f32("grid", grid)
    if grid.dim() != 5 or grid.shape[0] != B or grid.shape[4] != 12:
        raise ValueError(f"{what}: grid should be [B, GH, GW, GD, 12] (the 3 -> 3 op with offset) with B = {B}, got "
                         f"{tuple(grid.shape)}")
    GH, GW, GD = grid.shape[1:4]
    tensors = [("grid", grid), ("y", y), ("uv", uv), ("to_rgb", to_rgb)]
    if coarse is not None:
        tensors.append(("coarse", _check_coarse(what, coarse, B)))
    oy = ouv = None
    if surface_dtype is not None:
        if not deep:
            from_rgb = _yuv_constants("from_rgb", from_rgb, what)
        tensors.append(("from_rgb", from_rgb))
        if out_planes is not None:
            oy, ouv, oB, oH, oW, osurf = _yuv_surface(out_planes[0], out_planes[1], what, ("out_planes[0]", "out_planes[1]"),
                                                      chroma=chroma)
            if (oB, oH, oW) != (B, H, W) or oy.dtype != surface_dtype:
                raise ValueError(f"{what}: out_planes should be a {'uint16' if deep else 'uint8'} surface of {[B, H, W]}, got "
                                 f"{oy.dtype} {[oB, oH, oW]}")
            tensors += [("out_planes[0]", oy), ("out_planes[1]", ouv)]
    curves, g, n = _guide_source(guide, guide_conv1, guide_conv2, guide_curves, curves_prepared, return_guide, (B, H, W), 3,
                                 map_or_network=_ONE_GUIDE, lone_conv_ok=False, prepared_name="curves_prepared")
    for nm, t in tensors:
        _require_gpu(nm, t)
    dev = y.device
    grid = grid.detach().contiguous()
    k_in = to_rgb.detach().contiguous()
    if surface_dtype is not None:
        if oy is None:  # tight planes
            size = _YUV_SAMPLE[surface_dtype]
            oy = torch.empty((B, H, W), dtype=surface_dtype, device=dev)
            crows = H // 2 if chroma == "420" else H
            ouv = torch.empty((B, crows, W), dtype=surface_dtype, device=dev)
            osurf = (size, size * W, size * W, size * H * W, size * crows * W)
        k_out = from_rgb.detach().contiguous()
        planes = (oy.data_ptr(), ouv.data_ptr(), *osurf[1:], k_out.data_ptr())
        if chroma != "420":  # (one entry point for both surface widths: the kind says which)
            output = (_lib.CHROMA_OUT["surface_u16" if deep else "surface_u8"], *planes, int(out_bits) if deep else 0)
        else:
            output = (*planes, int(out_bits)) if deep else (_lib.YUV_OUT["nv12"], *planes)
        result = (oy, ouv)
    else:
        result = torch.empty((B, H, W, 3), dtype=out_dtype, device=dev)
        output = (_lib.YUV_OUT["rgb_f32" if out_dtype == torch.float32 else "rgb_u8"], result.data_ptr(), None, 0, 0, 0, 0, None)
        if chroma != "420":
            output += (0,)
    gout = torch.empty((B, H, W), dtype=torch.float32, device=dev) if return_guide else None
    surface = (y.data_ptr(), uv.data_ptr(), *surf, *(() if chroma == "420" else (_lib.CHROMA[chroma],)), B, H, W, k_in.data_ptr())
    head = (*surface, GH, GW, GD, 3, 3, 1)
    if coarse is not None:  # (the up-add entry points: the coarse level after to_rgb, no guide_out)
        coarse = coarse.detach().contiguous()
        fn = "hdrnet_bilateral_slice_apply_upadd_io_yuv"
        args = (grid.data_ptr(), _ptr(g[0]), *surface, coarse.data_ptr(), coarse.shape[1], coarse.shape[2], GH, GW, GD, 3, 3, 1,
                _ptr(g[1]), _ptr(g[2]), n, _guide_flags(fast_sigmoid, prescaled and g[0] is None))
    elif curves:
        fn = "hdrnet_bilateral_slice_apply_io_curves_yuv"
        args = (grid.data_ptr(), *head, *(t.data_ptr() for t in g[:4]), n, _ptr(g[4]), _ptr(gout))
    else:
        fn = "hdrnet_bilateral_slice_apply_io_yuv"
        args = (grid.data_ptr(), _ptr(g[0]), *head, _ptr(g[1]), _ptr(g[2]), n, _ptr(gout),
                _guide_flags(fast_sigmoid, prescaled and g[0] is None))
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), fn + ("_chroma" if chroma != "420" else "_p016" if deep else ""))(*args, *output, _stream(dev))
    _lib.check(rc, "BilateralSliceApplyUpAddIOYuv" if coarse is not None else "BilateralSliceApplyIOYuv")
    return (result, gout) if return_guide else result


def bilateral_slice_apply_io_yuv(grid: torch.Tensor, y: torch.Tensor, uv: torch.Tensor, to_rgb: torch.Tensor,
                                 guide: Optional[torch.Tensor] = None,
                                 guide_conv1: Optional[torch.Tensor] = None,
                                 guide_conv2: Optional[torch.Tensor] = None,
                                 guide_curves: Optional[Tuple[torch.Tensor, ...]] = None,
                                 return_guide: bool = False, fast_sigmoid: bool = False, prescaled: bool = False,
                                 curves_prepared: Optional[torch.Tensor] = None,
                                 out: str = "rgb", out_dtype: Optional[torch.dtype] = None,
                                 from_rgb: Optional[torch.Tensor] = None, out_planes=None, chroma: str = "420"):
    """``bilateral_slice_apply_io`` for a semi-planar YUV 4:2:0 surface in (include/hdrnet_amd_yuv.h): ``y`` ``[B, H, W]``,
    ``uv`` ``[B, H / 2, W]``, uint8 (NV12) or uint16 (P010 / P016), converted in the kernel's load by ``to_rgb`` (12
    floats, ``yuv.yuv_coefficients``) -- exactly ``bilateral_slice_apply_io(grid, yuv_to_rgb(y, uv, to_rgb), ...)`` on
    the float32 frame, bit for bit, without that frame.  The guide arguments are those of ``bilateral_slice_apply_io``.

    ``out="rgb"``: ``[B, H, W, 3]`` RGB, ``out_dtype`` float32 (default) or uint8 ``= (uint8)(255 * clip(., 0, 1))``.
    ``out="nv12"``: an NV12 uint8 surface, returned as ``(y_out [B, H, W], uv_out [B, H / 2, W])``, encoded by
    ``from_rgb`` (12 floats): Y per pixel, U and V from the mean of each 2 x 2 block, truncated.  ``out_planes``: a
    ``(y_out, uv_out)`` pair to write into (pitched planes are fine; padding is not written).  Planes of the input may be
    pitched too.  ``return_guide`` appends the guide map.  Cin = Cout = 3 with offset, H even, W % 4 == 0.  No autograd.
    A P010 / P016 surface out is ``bilateral_slice_apply_io_yuv_deep``'s; a uint16 RGB frame out is out of scope.

    ``chroma="422"`` (include/hdrnet_amd_yuv_chroma.h): an NV16 / P210 / P216 surface in, ``uv`` ``[B, H, W]``, any H;
    ``out="nv16"`` is then the uint8 surface out, ``(y_out [B, H, W], uv_out [B, H, W])``, U and V from the mean of each
    horizontal pair.  Exactly ``bilateral_slice_apply_io(grid, yuv_to_rgb(y, uv, to_rgb, chroma="422"), ...)``."""
    what = "bilateral_slice_apply_io_yuv"
    chroma = _check_chroma(what, chroma, False)
    if chroma != "420":
        if out not in ("rgb", "nv16"):
            raise ValueError(f"{what}: unknown out {out!r} (chroma='422' takes 'rgb', 'nv16')")
        if out == "nv16":
            if out_dtype not in (None, torch.uint8):
                raise TypeError(f"{what}: an NV16 output is uint8, got out_dtype = {out_dtype}")
            if from_rgb is None:
                raise ValueError(f"{what}: out='nv16' needs from_rgb (yuv.yuv_coefficients)")
    elif out not in ("rgb", "nv12"):
        raise ValueError(f"{what}: unknown out {out!r} (takes 'rgb', 'nv12')")
    if out == "rgb":
        out_dtype = torch.float32 if out_dtype is None else out_dtype
        if out_dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"{what}: out_dtype must be float32 or uint8, got {out_dtype}")
        if from_rgb is not None or out_planes is not None:
            raise ValueError(f"{what}: from_rgb / out_planes belong to out='nv12'")
    elif chroma == "420":
        if out_dtype not in (None, torch.uint8):
            raise TypeError(f"{what}: an NV12 output is uint8, got out_dtype = {out_dtype}")
        if from_rgb is None:
            raise ValueError(f"{what}: out='nv12' needs from_rgb (yuv.yuv_coefficients)")
    return _apply_io_surface(what, None if out == "rgb" else torch.uint8, out_dtype, grid, y, uv, to_rgb, guide, guide_conv1,
                             guide_conv2, guide_curves, return_guide, fast_sigmoid, prescaled, curves_prepared, from_rgb,
                             out_planes, chroma=chroma)


def bilateral_slice_apply_io_yuv_deep(grid: torch.Tensor, y: torch.Tensor, uv: torch.Tensor, to_rgb: torch.Tensor,
                                      guide: Optional[torch.Tensor] = None,
                                      guide_conv1: Optional[torch.Tensor] = None,
                                      guide_conv2: Optional[torch.Tensor] = None,
                                      guide_curves: Optional[Tuple[torch.Tensor, ...]] = None,
                                      return_guide: bool = False, fast_sigmoid: bool = False, prescaled: bool = False,
                                      curves_prepared: Optional[torch.Tensor] = None,
                                      from_rgb: Optional[torch.Tensor] = None, out_bits: Optional[int] = None,
                                      out_planes=None, chroma: str = "420"):
    """``bilateral_slice_apply_io_yuv`` for a uint16 surface in (P010 / P016) with a P010 / P016 surface OUT
    (include/hdrnet_amd_u16_out.h), returned as ``(y_out [B, H, W], uv_out [B, H / 2, W])`` uint16.  ``out_bits`` is 10
    (P010) or 16 (P016): the codes have that many bits and sit in the high bits of the sample.  ``from_rgb``: the 12
    floats of ``yuv.yuv_encode_coefficients(standard, full_range, out_bits)`` on the device -- code units of ``out_bits``
    bits, the + 0.5 folded in; the kernel clamps to ``[0, 2 ** out_bits - 1]`` and truncates: Y per pixel, U and V from
    the mean of each 2 x 2 block, in the NV12 store's operation order.  ``out_planes``: a ``(y_out, uv_out)`` pair to write
    into (pitched planes are fine; padding is not written); tight planes are allocated when none are given.  The guide
    arguments and the arithmetic before the store are ``bilateral_slice_apply_io_yuv``'s.  ``return_guide`` appends the
    guide map.  No autograd.  Out of scope: an NV12 surface in, a uint16 RGB frame out of a surface.
    ``chroma="422"`` (include/hdrnet_amd_yuv_chroma.h): P210 / P216 in and out, ``uv`` planes ``[B, H, W]``, any H; U and V
    from the mean of each horizontal pair."""
    what = "bilateral_slice_apply_io_yuv_deep"
    chroma = _check_chroma(what, chroma, False)
    if from_rgb is None:
        raise ValueError(f"{what}: needs from_rgb (yuv.yuv_encode_coefficients)")
    if out_bits not in (10, 16):
        raise ValueError(f"{what}: out_bits must be 10 (P010) or 16 (P016), got {out_bits!r}")
    return _apply_io_surface(what, torch.uint16, None, grid, y, uv, to_rgb, guide, guide_conv1, guide_conv2, guide_curves,
                             return_guide, fast_sigmoid, prescaled, curves_prepared, from_rgb, out_planes, out_bits,
                             chroma=chroma)


# ---- packed YUV 4:2:2 surfaces (include/hdrnet_amd_yuv_packed.h) -----------------------------------------------------------
_PACKED_DTYPE = {"yuy2": torch.uint8, "yuyv": torch.uint8, "uyvy": torch.uint8, "yvyu": torch.uint8,
                 "y210": torch.uint16, "y216": torch.uint16}


def packed_format(what: str, format) -> str:  # noqa: A002
    """The ``format`` of a packed 4:2:2 surface: ``"yuy2"`` (= ``"yuyv"``), ``"uyvy"``, ``"yvyu"`` (uint8) or ``"y210"`` /
    ``"y216"`` (uint16).  NAMED by the caller; it is never guessed from the tensor."""
    if not isinstance(format, str) or format not in _lib.PACKED_ORDER:
        raise ValueError(f"{what}: unknown format {format!r} (takes {', '.join(repr(k) for k in _lib.PACKED_ORDER)})")
    return format


def _yuv_packed_surface(surface, format, what: str, name: str = "surface"):  # noqa: A002
    """The rules of a packed surface, on the host: ``[B, H, 2 W]`` samples (or ``[B, H, W, 2]`` viewed as that) of the
    format's dtype, last-dimension stride 1, row stride >= 2 W samples, pitches multiples of 4 bytes, W % 4 == 0.  Returns
    ``(surface, B, H, W, (sample_dtype, pitch, image_stride, order))``, pitches in bytes."""
    if not isinstance(surface, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a torch.Tensor, got {type(surface).__name__}")
    want = _PACKED_DTYPE[format]
    if surface.dtype != want:
        raise TypeError(f"{what}: format={format!r} is a {str(want).replace('torch.', '')} format, {name} is {surface.dtype} "
                        "('yuy2' / 'uyvy' / 'yvyu' need uint8, 'y210' / 'y216' need uint16)")
    if surface.dim() == 4 and surface.shape[3] == 2 and surface.stride(3) == 1 and surface.stride(2) == 2:
        surface = surface.as_strided((surface.shape[0], surface.shape[1], 2 * surface.shape[2]),
                                     (surface.stride(0), surface.stride(1), 1))
    if surface.dim() != 3 or surface.shape[2] % 2:
        raise ValueError(f"{what}: {name} should be [B, H, 2 W] samples (or [B, H, W, 2] with unit sample strides), got "
                         f"{tuple(surface.shape)} with strides {tuple(surface.stride())}")
    B, H, W = surface.shape[0], surface.shape[1], surface.shape[2] // 2
    if W % 4 != 0:
        raise ValueError(f"{what}: W % 4 != 0 (W = {W})")
    size = surface.element_size()
    if B * H * W and (surface.stride(2) != 1 or surface.stride(1) < 2 * W or (surface.stride(1) * size) % 4
                      or (surface.stride(0) * size) % 4):
        raise ValueError(f"{what}: {name} must have last-dimension stride 1, a row stride >= 2 W samples and pitches that are "
                         f"multiples of 4 bytes, got strides {tuple(surface.stride())}")
    return surface, B, H, W, (_YUV_SAMPLE[want], surface.stride(1) * size, surface.stride(0) * size, _lib.PACKED_ORDER[format])


def packed_default_bits(format: str) -> int:  # noqa: A002
    """Significant bits per sample a packed format implies: 8, 10 (``"y210"``) or 16 (``"y216"``)."""
    return 10 if format == "y210" else 16 if format == "y216" else 8


def yuv_packed_to_rgb(surface: torch.Tensor, to_rgb: torch.Tensor, format: str) -> torch.Tensor:  # noqa: A002
    """A packed YUV 4:2:2 surface -> float32 ``[B, H, W, 3]`` RGB in [0, 1] (``hdrnet_yuv_packed_to_rgb_f32``): ``surface``
    ``[B, H, 2 W]`` (or ``[B, H, W, 2]``), ``format`` ``"yuy2"`` / ``"uyvy"`` / ``"yvyu"`` (uint8) or ``"y210"`` / ``"y216"``
    (uint16, the code in the high bits); ``to_rgb`` the 12 floats of ``yuv.yuv_coefficients`` on the device.  Exactly
    ``yuv_to_rgb(y, uv, to_rgb, chroma="422")`` on the de-interleaved planes, bit for bit.  The surface may be pitched;
    padding is not read.  No autograd."""
    what = "yuv_packed_to_rgb"
    format = packed_format(what, format)  # noqa: A001
    surface, B, H, W, surf = _yuv_packed_surface(surface, format, what)
    to_rgb = _yuv_constants("to_rgb", to_rgb, what)
    for nm, t in (("surface", surface), ("to_rgb", to_rgb)):
        _require_gpu(nm, t)
    dev = surface.device
    k = to_rgb.detach().contiguous()
    out = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().hdrnet_yuv_packed_to_rgb_f32(surface.data_ptr(), *surf, B, H, W, k.data_ptr(), out.data_ptr(),
                                                      _stream(dev))
    _lib.check(rc, "YuvPackedToRgb")
    return out


def bilateral_slice_apply_io_yuv_packed(grid: torch.Tensor, surface: torch.Tensor, to_rgb: torch.Tensor, format: str,  # noqa: A002
                                        guide: Optional[torch.Tensor] = None,
                                        guide_conv1: Optional[torch.Tensor] = None,
                                        guide_conv2: Optional[torch.Tensor] = None,
                                        guide_curves: Optional[Tuple[torch.Tensor, ...]] = None,
                                        return_guide: bool = False, fast_sigmoid: bool = False, prescaled: bool = False,
                                        curves_prepared: Optional[torch.Tensor] = None,
                                        out: str = "rgb", out_dtype: Optional[torch.dtype] = None,
                                        from_rgb: Optional[torch.Tensor] = None, out_surface=None,
                                        out_bits: Optional[int] = None):
    """``bilateral_slice_apply_io_yuv(..., chroma="422")`` for a PACKED 4:2:2 surface (include/hdrnet_amd_yuv_packed.h):
    ``surface`` ``[B, H, 2 W]`` in the NAMED ``format`` -- the NV16 / P210 pair woven into one plane, read as it is; the same
    bits as that call on the de-interleaved planes.  The guide arguments are those of ``bilateral_slice_apply_io``.

    ``out="rgb"``: ``[B, H, W, 3]`` RGB, ``out_dtype`` float32 (default) or uint8.  ``out="packed"``: a packed surface of the
    input's format ``[B, H, 2 W]``, encoded by ``from_rgb`` (12 floats; for uint16 formats those of
    ``yuv.yuv_encode_coefficients(..., out_bits)``): Y per pixel, U and V from the mean of each horizontal pair, truncated.
    ``out_bits``: 10 or 16 for ``"y210"`` / ``"y216"`` (default: the format's), 8 otherwise.  ``out_surface``: a surface to
    write into (pitched is fine; padding is not written).  ``return_guide`` appends the guide map.  Cin = Cout = 3 with
    offset, any H, W % 4 == 0.  No autograd."""
    what = "bilateral_slice_apply_io_yuv_packed"
    format = packed_format(what, format)  # noqa: A001
    if out not in ("rgb", "packed"):
        raise ValueError(f"{what}: unknown out {out!r} (takes 'rgb', 'packed')")
    surface, B, H, W, surf = _yuv_packed_surface(surface, format, what)
    deep = surface.dtype == torch.uint16
    if out == "rgb":
        out_dtype = torch.float32 if out_dtype is None else out_dtype
        if out_dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"{what}: out_dtype must be float32 or uint8, got {out_dtype}")
        if from_rgb is not None or out_surface is not None or out_bits is not None:
            raise ValueError(f"{what}: from_rgb / out_surface / out_bits belong to out='packed'")
    else:
        if out_dtype not in (None, surface.dtype):
            raise TypeError(f"{what}: a packed output has the input's sample dtype {surface.dtype}, got out_dtype = {out_dtype}")
        if from_rgb is None:
            raise ValueError(f"{what}: out='packed' needs from_rgb (yuv.yuv_encode_coefficients)")
        out_bits = packed_default_bits(format) if out_bits is None else out_bits
        if out_bits not in ((10, 16) if deep else (8,)):
            raise ValueError(f"{what}: out_bits must be {'10 (Y210) or 16 (Y216)' if deep else '8'} for format={format!r}, got "
                             f"{out_bits!r}")
    to_rgb = _yuv_constants("to_rgb", to_rgb, what)
    _require_f32("grid", grid)
    if grid.dim() != 5 or grid.shape[0] != B or grid.shape[4] != 12:
        raise ValueError(f"{what}: grid should be [B, GH, GW, GD, 12] (the 3 -> 3 op with offset) with B = {B}, got "
                         f"{tuple(grid.shape)}")
    GH, GW, GD = grid.shape[1:4]
    tensors = [("grid", grid), ("surface", surface), ("to_rgb", to_rgb)]
    osurf = None
    if out == "packed":
        from_rgb = _yuv_constants("from_rgb", from_rgb, what)
        tensors.append(("from_rgb", from_rgb))
        if out_surface is not None:
            out_surface, oB, oH, oW, osurf = _yuv_packed_surface(out_surface, format, what, "out_surface")
            if (oB, oH, oW) != (B, H, W):
                raise ValueError(f"{what}: out_surface should be a surface of {[B, H, 2 * W]}, got {list(out_surface.shape)}")
            tensors.append(("out_surface", out_surface))
    curves, g, n = _guide_source(guide, guide_conv1, guide_conv2, guide_curves, curves_prepared, return_guide, (B, H, W), 3,
                                 map_or_network=_ONE_GUIDE, lone_conv_ok=False, prepared_name="curves_prepared")
    for nm, t in tensors:
        _require_gpu(nm, t)
    dev = surface.device
    grid = grid.detach().contiguous()
    k_in = to_rgb.detach().contiguous()
    if out == "packed":
        if out_surface is None:  # a tight surface
            size = surface.element_size()
            out_surface = torch.empty((B, H, 2 * W), dtype=surface.dtype, device=dev)
            osurf = (surf[0], 2 * W * size, 2 * W * H * size, surf[3])
        k_out = from_rgb.detach().contiguous()
        output = (_lib.CHROMA_OUT["surface_u16" if deep else "surface_u8"], out_surface.data_ptr(), osurf[1], osurf[2],
                  k_out.data_ptr(), int(out_bits) if deep else 0)
        result = out_surface
    else:
        result = torch.empty((B, H, W, 3), dtype=out_dtype, device=dev)
        output = (_lib.CHROMA_OUT["rgb_f32" if out_dtype == torch.float32 else "rgb_u8"], result.data_ptr(), 0, 0, None, 0)
    gout = torch.empty((B, H, W), dtype=torch.float32, device=dev) if return_guide else None
    head = (surface.data_ptr(), *surf, B, H, W, k_in.data_ptr(), GH, GW, GD, 3, 3, 1)
    with torch.cuda.device(dev):
        if curves:
            rc = _lib.load().hdrnet_bilateral_slice_apply_io_curves_yuv_packed(
                grid.data_ptr(), *head, *(t.data_ptr() for t in g[:4]), n, _ptr(g[4]), _ptr(gout), *output, _stream(dev))
        else:
            rc = _lib.load().hdrnet_bilateral_slice_apply_io_yuv_packed(
                grid.data_ptr(), _ptr(g[0]), *head, _ptr(g[1]), _ptr(g[2]), n, _ptr(gout),
                _guide_flags(fast_sigmoid, prescaled and g[0] is None), *output, _stream(dev))
    _lib.check(rc, "BilateralSliceApplyIOYuvPacked")
    return (result, gout) if return_guide else result


# ---- planar YUV 4:2:0 surfaces (include/hdrnet_amd_yuv_planar.h) -----------------------------------------------------------
def _yuv_planar_surface(y, u, v, what: str, names=("y", "u", "v"), chroma: str = "420"):
    """The rules of a planar surface, on the host: ``y`` ``[B, H, W]``, ``u`` and ``v`` ``[B, H / 2, W / 2]`` of one dtype,
    uint8 or uint16, last-dimension stride 1; the luma's row and image strides multiples of 4 bytes, the chroma's of 2
    bytes (uint8) / 4 bytes (uint16).  Returns ``(B, H, W, (sample_dtype, pitch_y, pitch_u, pitch_v, image_stride_y,
    image_stride_u, image_stride_v))``, in bytes.  ``chroma="422"``: ``u`` and ``v`` are ``[B, H, W / 2]``; ``"444"``:
    ``[B, H, W]`` with the luma's alignment; both take any H."""
    if chroma != "420":
        return _yuv_planar_surface_chroma(y, u, v, what, names, chroma)
    planes = tuple(zip(names, (y, u, v)))
    for nm, t in planes:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {nm} must be a torch.Tensor, got {type(t).__name__}")
    if y.dim() != 3:
        raise ValueError(f"{what}: {names[0]} should be [B, H, W], got {tuple(y.shape)}")
    B, H, W = y.shape
    if y.dtype not in _YUV_SAMPLE or u.dtype != y.dtype or v.dtype != y.dtype:
        raise TypeError(f"{what}: {', '.join(names)} must all be uint8 (I420) or all uint16 (yuv420p10le / yuv420p16le), got "
                        f"{y.dtype}, {u.dtype}, {v.dtype}")
    if H % 2 != 0:
        raise ValueError(f"{what}: H must be even (a chroma row serves two image rows), got H = {H}")
    if W % 4 != 0:
        raise ValueError(f"{what}: W % 4 != 0 (W = {W})")
    for nm, t in planes[1:]:
        if t.dim() != 3 or tuple(t.shape) != (B, H // 2, W // 2):
            raise ValueError(f"{what}: {nm} should be [B, H / 2, W / 2] = {[B, H // 2, W // 2]}, got {list(t.shape)}")
    size = y.element_size()
    for i, (nm, t) in enumerate(planes):
        row, unit = (W, 4) if i == 0 else (W // 2, 2 * size)
        if B * H * W and (t.stride(2) != 1 or t.stride(1) < row or (t.stride(1) * size) % unit or (t.stride(0) * size) % unit):
            raise ValueError(f"{what}: {nm} must have last-dimension stride 1, a row stride >= {row} samples and pitches that "
                             f"are multiples of {unit} bytes, got strides {tuple(t.stride())}")
    return B, H, W, (_YUV_SAMPLE[y.dtype], *(t.stride(1) * size for t in (y, u, v)), *(t.stride(0) * size for t in (y, u, v)))


def _yuv_planar_surface_chroma(y, u, v, what: str, names, chroma: str):
    """``_yuv_planar_surface`` for a 4:2:2 or 4:4:4 planar surface: a chroma row per image row, and for 4:4:4 a chroma
    sample per pixel (whole dwords per lane: the luma's alignment)."""
    planes = tuple(zip(names, (y, u, v)))
    for nm, t in planes:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: {nm} must be a torch.Tensor, got {type(t).__name__}")
    if y.dim() != 3:
        raise ValueError(f"{what}: {names[0]} should be [B, H, W], got {tuple(y.shape)}")
    B, H, W = y.shape
    fmt = "yuv%sp" % chroma
    if y.dtype not in _YUV_SAMPLE or u.dtype != y.dtype or v.dtype != y.dtype:
        raise TypeError(f"{what}: {', '.join(names)} must all be uint8 ({fmt}) or all uint16 ({fmt}10le / {fmt}16le), got "
                        f"{y.dtype}, {u.dtype}, {v.dtype}")
    if W % 4 != 0:
        raise ValueError(f"{what}: W % 4 != 0 (W = {W})")
    cw = W if chroma == "444" else W // 2
    for nm, t in planes[1:]:
        if t.dim() != 3 or tuple(t.shape) != (B, H, cw):
            raise ValueError(f"{what}: chroma={chroma!r}: {nm} should be [B, H, {'W' if chroma == '444' else 'W / 2'}] = "
                             f"{[B, H, cw]}, got {list(t.shape)}")
    size = y.element_size()
    for i, (nm, t) in enumerate(planes):
        row, unit = (W, 4) if i == 0 or chroma == "444" else (cw, 2 * size)
        if B * H * W and (t.stride(2) != 1 or t.stride(1) < row or (t.stride(1) * size) % unit or (t.stride(0) * size) % unit):
            raise ValueError(f"{what}: {nm} must have last-dimension stride 1, a row stride >= {row} samples and pitches that "
                             f"are multiples of {unit} bytes, got strides {tuple(t.stride())}")
    return B, H, W, (_YUV_SAMPLE[y.dtype], *(t.stride(1) * size for t in (y, u, v)), *(t.stride(0) * size for t in (y, u, v)))


def yuv_planar_to_rgb(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, to_rgb: torch.Tensor,
                      chroma: str = "420") -> torch.Tensor:
    """``yuv_to_rgb`` for a PLANAR YUV 4:2:0 surface (``hdrnet_yuv_planar_to_rgb_f32``, include/hdrnet_amd_yuv_planar.h):
    ``y`` ``[B, H, W]``, ``u`` and ``v`` ``[B, H / 2, W / 2]``, uint8 (I420; YV12 with the planes swapped) or uint16 with the
    code in the low bits (yuv420p10le / yuv420p16le); ``to_rgb`` the 12 floats of ``yuv.yuv_coefficients(...,
    msb_aligned=False)`` on the device.  The bits of ``yuv_to_rgb`` on the interleaved surface.  Planes may be pitched;
    padding is not read.  No autograd.  ``chroma`` (include/hdrnet_amd_yuv_chroma.h): ``"422"`` -- yuv422p..., ``u`` and ``v``
    ``[B, H, W / 2]`` -- or ``"444"`` -- yuv444p..., ``[B, H, W]`` -- with any H."""
    what = "yuv_planar_to_rgb"
    chroma = _check_chroma(what, chroma, True)
    B, H, W, surf = _yuv_planar_surface(y, u, v, what, chroma=chroma)
    to_rgb = _yuv_constants("to_rgb", to_rgb, what)
    for nm, t in (("y", y), ("u", u), ("v", v), ("to_rgb", to_rgb)):
        _require_gpu(nm, t)
    dev = y.device
    k = to_rgb.detach().contiguous()
    out = torch.empty((B, H, W, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        if chroma != "420":
            rc = _lib.load().hdrnet_yuv_planar_chroma_to_rgb_f32(y.data_ptr(), u.data_ptr(), v.data_ptr(), *surf,
                                                                 _lib.CHROMA[chroma], B, H, W, k.data_ptr(), out.data_ptr(),
                                                                 _stream(dev))
        else:
            rc = _lib.load().hdrnet_yuv_planar_to_rgb_f32(y.data_ptr(), u.data_ptr(), v.data_ptr(), *surf, B, H, W,
                                                          k.data_ptr(), out.data_ptr(), _stream(dev))
    _lib.check(rc, "YuvPlanarToRgb")
    return out


def bilateral_slice_apply_io_yuv_planar(grid: torch.Tensor, y: torch.Tensor, u: torch.Tensor, v: torch.Tensor,
                                        to_rgb: torch.Tensor,
                                        guide: Optional[torch.Tensor] = None,
                                        guide_conv1: Optional[torch.Tensor] = None,
                                        guide_conv2: Optional[torch.Tensor] = None,
                                        guide_curves: Optional[Tuple[torch.Tensor, ...]] = None,
                                        return_guide: bool = False, fast_sigmoid: bool = False, prescaled: bool = False,
                                        curves_prepared: Optional[torch.Tensor] = None,
                                        out: str = "rgb", out_dtype: Optional[torch.dtype] = None,
                                        from_rgb: Optional[torch.Tensor] = None, out_bits: Optional[int] = None,
                                        out_planes=None, chroma: str = "420"):
    """``bilateral_slice_apply_io_yuv`` for a PLANAR YUV 4:2:0 surface in (include/hdrnet_amd_yuv_planar.h): ``y``
    ``[B, H, W]``, ``u`` and ``v`` ``[B, H / 2, W / 2]``, uint8 (I420) or uint16 with the code in the low bits
    (yuv420p10le / yuv420p16le), converted in the kernel's load by ``to_rgb`` (``yuv.yuv_coefficients(...,
    msb_aligned=False)``): the bits of ``bilateral_slice_apply_io_yuv`` on the interleaved surface.  The guide arguments
    are those of ``bilateral_slice_apply_io``.

    ``out="rgb"``: ``[B, H, W, 3]`` RGB, ``out_dtype`` float32 (default) or uint8.  ``out="planar"``: a planar surface of the
    input's dtype, returned as ``(y_out, u_out, v_out)``, encoded by ``from_rgb`` (``yuv.yuv_encode_coefficients(standard,
    full_range, out_bits)``) with ``out_bits`` 8 for uint8 planes and 10 or 16 for uint16 planes: codes clamped to
    ``2 ** out_bits - 1``, truncated, in the low bits.  ``out_planes``: a ``(y_out, u_out, v_out)`` triple to write into
    (pitched planes are fine; padding is not written); tight planes are allocated when none are given.  ``return_guide``
    appends the guide map.  Cin = Cout = 3 with offset, H even, W % 4 == 0.  No autograd.  Out of scope: uint16 planes in ->
    uint8 planes out, a semi-planar surface out.

    ``chroma`` (include/hdrnet_amd_yuv_chroma.h): ``"422"`` -- yuv422p / yuv422p10le / yuv422p16le, ``u`` and ``v``
    ``[B, H, W / 2]`` -- or ``"444"`` -- yuv444p..., ``[B, H, W]`` -- with any H; ``out="planar"`` is then a surface of the
    same layout, U and V from the mean of each horizontal pair (4:2:2) or per pixel (4:4:4)."""
    return _apply_io_planar("bilateral_slice_apply_io_yuv_planar", grid, y, u, v, to_rgb, guide, guide_conv1, guide_conv2,
                            guide_curves, return_guide, fast_sigmoid, prescaled, curves_prepared, out, out_dtype, from_rgb,
                            out_bits, out_planes, chroma)


def _apply_io_planar(what, grid, y, u, v, to_rgb, guide, guide_conv1, guide_conv2, guide_curves, return_guide, fast_sigmoid,
                     prescaled, curves_prepared, out, out_dtype, from_rgb, out_bits, out_planes, chroma, coarse=None):
    """The body of ``bilateral_slice_apply_io_yuv_planar`` (``what``).  ``coarse``: the call is
    ``bilateral_slice_apply_upadd_io_yuv_planar`` (4:2:0, a guide map or the network): the coarser pyramid level to up-add."""
    chroma = _check_chroma(what, chroma, True)
    if out not in ("rgb", "planar"):
        raise ValueError(f"{what}: unknown out {out!r} (takes 'rgb', 'planar')")
    planar = out == "planar"
    if not planar:
        out_dtype = torch.float32 if out_dtype is None else out_dtype
        if out_dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"{what}: out_dtype must be float32 or uint8, got {out_dtype}")
        if from_rgb is not None or out_planes is not None or out_bits is not None:
            raise ValueError(f"{what}: from_rgb / out_bits / out_planes belong to out='planar'")
    elif from_rgb is None:
        raise ValueError(f"{what}: out='planar' needs from_rgb (yuv.yuv_encode_coefficients)")
    B, H, W, surf = _yuv_planar_surface(y, u, v, what, chroma=chroma)
    if planar:
        if out_dtype not in (None, y.dtype):
            raise TypeError(f"{what}: a planar output has the input's dtype ({y.dtype}), got out_dtype = {out_dtype}")
        if out_bits is None:
            out_bits = 8 if y.dtype == torch.uint8 else 16
        if out_bits not in ((8,) if y.dtype == torch.uint8 else (10, 16)):
            raise ValueError(f"{what}: out_bits = {out_bits!r} does not fit {y.dtype} planes (uint8: 8; uint16: 10 or 16)")
    to_rgb = _yuv_constants("to_rgb", to_rgb, what)
    _require_f32("grid", grid)
    if grid.dim() != 5 or grid.shape[0] != B or grid.shape[4] != 12:
        raise ValueError(f"{what}: grid should be [B, GH, GW, GD, 12] (the 3 -> 3 op with offset) with B = {B}, got "
                         f"{tuple(grid.shape)}")
    GH, GW, GD = grid.shape[1:4]
    tensors = [("grid", grid), ("y", y), ("u", u), ("v", v), ("to_rgb", to_rgb)]
    if coarse is not None:
        tensors.append(("coarse", _check_coarse(what, coarse, B)))
    planes = osurf = None
    if planar:
        from_rgb = _yuv_constants("from_rgb", from_rgb, what)
        tensors.append(("from_rgb", from_rgb))
        if out_planes is not None:
            planes = tuple(out_planes)
            if len(planes) != 3:
                raise ValueError(f"{what}: out_planes should be a (y_out, u_out, v_out) triple, got {len(planes)} planes")
            names = tuple(f"out_planes[{i}]" for i in range(3))
            oB, oH, oW, osurf = _yuv_planar_surface(*planes, what, names, chroma=chroma)
            if (oB, oH, oW) != (B, H, W) or planes[0].dtype != y.dtype:
                raise ValueError(f"{what}: out_planes should be a {str(y.dtype).replace('torch.', '')} planar surface of "
                                 f"{[B, H, W]}, got {planes[0].dtype} {[oB, oH, oW]}")
            tensors += list(zip(names, planes))
    curves, g, n = _guide_source(guide, guide_conv1, guide_conv2, guide_curves, curves_prepared, return_guide, (B, H, W), 3,
                                 map_or_network=_ONE_GUIDE, lone_conv_ok=False, prepared_name="curves_prepared")
    for nm, t in tensors:
        _require_gpu(nm, t)
    dev = y.device
    grid = grid.detach().contiguous()
    k_in = to_rgb.detach().contiguous()
    if planar:
        if planes is None:  # tight planes
            size = _YUV_SAMPLE[y.dtype]
            ch, cw = (H // 2 if chroma == "420" else H), (W if chroma == "444" else W // 2)
            planes = (torch.empty((B, H, W), dtype=y.dtype, device=dev),
                      torch.empty((B, ch, cw), dtype=y.dtype, device=dev),
                      torch.empty((B, ch, cw), dtype=y.dtype, device=dev))
            cw, cp = size * cw, size * ch * cw
            osurf = (size, size * W, cw, cw, size * H * W, cp, cp)
        k_out = from_rgb.detach().contiguous()
        kind = (_lib.YUV_PLANAR_OUT["planar"] if chroma == "420"
                else _lib.CHROMA_OUT["surface_u8" if y.dtype == torch.uint8 else "surface_u16"])
        output = (kind, *(t.data_ptr() for t in planes), *osurf[1:], k_out.data_ptr(), int(out_bits))
        result = planes
    else:
        result = torch.empty((B, H, W, 3), dtype=out_dtype, device=dev)
        output = (_lib.YUV_PLANAR_OUT["rgb_f32" if out_dtype == torch.float32 else "rgb_u8"], result.data_ptr(), None, None,
                  0, 0, 0, 0, 0, 0, None, 0)
    gout = torch.empty((B, H, W), dtype=torch.float32, device=dev) if return_guide else None
    surface = (y.data_ptr(), u.data_ptr(), v.data_ptr(), *surf, *(() if chroma == "420" else (_lib.CHROMA[chroma],)), B, H, W,
               k_in.data_ptr())
    head = (*surface, GH, GW, GD, 3, 3, 1)
    if coarse is not None:  # (the up-add entry point: the coarse level after to_rgb, no guide_out)
        coarse = coarse.detach().contiguous()
        fn = "hdrnet_bilateral_slice_apply_upadd_io_yuv_planar"
        args = (grid.data_ptr(), _ptr(g[0]), *surface, coarse.data_ptr(), coarse.shape[1], coarse.shape[2], GH, GW, GD, 3, 3, 1,
                _ptr(g[1]), _ptr(g[2]), n, _guide_flags(fast_sigmoid, prescaled and g[0] is None))
    elif curves:
        fn = "hdrnet_bilateral_slice_apply_io_curves_yuv_planar"
        args = (grid.data_ptr(), *head, *(t.data_ptr() for t in g[:4]), n, _ptr(g[4]), _ptr(gout))
    else:
        fn = "hdrnet_bilateral_slice_apply_io_yuv_planar"
        args = (grid.data_ptr(), _ptr(g[0]), *head, _ptr(g[1]), _ptr(g[2]), n, _ptr(gout),
                _guide_flags(fast_sigmoid, prescaled and g[0] is None))
    with torch.cuda.device(dev):
        rc = getattr(_lib.load(), fn + ("_chroma" if chroma != "420" else ""))(*args, *output, _stream(dev))
    _lib.check(rc, "BilateralSliceApplyUpAddIOYuvPlanar" if coarse is not None else "BilateralSliceApplyIOYuvPlanar")
    return (result, gout) if return_guide else result


def resize_bilinear_io(input: torch.Tensor, height: int, width: int,  # noqa: A002
                       white_level: Optional[float] = None) -> torch.Tensor:
    """``resize_bilinear(input / white_level, height, width)`` of a wire-format RGB frame in one pass: ``input``
    ``[B, Hin, Win, 3]`` uint8 / uint16 / float32 (``white_level`` 255 / 65535 / 1 by default; float32 is never scaled),
    float32 ``[B, height, width, 3]`` out -- level 1 of ``HDRNetGaussianPyrNN``'s input pyramid without a float32 copy of
    the frame (``hdrnet_resize_bilinear_io``, include/hdrnet_amd_pyramid_io.h).  Same taps and lerp as
    ``resize_bilinear``; the division is the wire-format forward's IEEE-rounded one.  No autograd."""
    white_level = _frame_head(input, white_level, rank_text="input should be 4D (batch, height, width, channels)")
    if input.shape[3] != 3:
        raise ValueError(f"resize_bilinear_io takes RGB frames (C = 3), got C = {input.shape[3]}")
    if min(input.shape[1], input.shape[2]) < 1 or int(height) < 0 or int(width) < 0:
        raise ValueError(f"bad extents: in {tuple(input.shape)}, out {height} x {width}")
    _require_gpu("input", input)
    inp = input.detach().contiguous()
    B, Hin, Win, C = inp.shape
    out = torch.empty((B, int(height), int(width), C), dtype=torch.float32, device=inp.device)
    lib = _lib.load()
    with torch.cuda.device(inp.device):
        rc = lib.hdrnet_resize_bilinear_io(inp.data_ptr(), _DTYPE_CODE[input.dtype], float(white_level), out.data_ptr(), B,
                                           Hin, Win, int(height), int(width), C, _stream(inp.device))
    _lib.check(rc, "ResizeBilinearIO")
    return out


def bilateral_slice_apply_upadd_io(grid: torch.Tensor, input: torch.Tensor, coarse: torch.Tensor,  # noqa: A002
                                   guide: Optional[torch.Tensor] = None,
                                   guide_conv1: Optional[torch.Tensor] = None,
                                   guide_conv2: Optional[torch.Tensor] = None,
                                   input_white_level: Optional[float] = None,
                                   out_dtype: torch.dtype = torch.float32,
                                   has_offset: bool = True, fast_sigmoid: bool = False, prescaled: bool = False,
                                   guide_curves=None) -> torch.Tensor:
    """The finest level of ``HDRNetGaussianPyrNN._output`` with the wire formats of ``bilateral_slice_apply_io``:
    ``wire_out(bilateral_slice_apply(grid, guide, input / input_white_level) + resize_bilinear(coarse -> H x W))`` in one
    pass.  ``input`` uint8 / uint16 / float32 ``[B, H, W, 3]``, ``coarse`` float32 ``[B, Hc, Wc, 3]``; ``out_dtype``
    float32, or uint8 ``= (uint8)(255 * clip(., 0, 1))`` with the clip after the up-add.  The guide is a ``guide`` map or
    the folded guide network (``guide_conv1``, ``guide_conv2``; ``fast_sigmoid`` / ``prescaled`` as in
    ``bilateral_slice_apply_io``); the curves guide belongs to the single-level models and is refused.  Cin = Cout = 3 with
    offset.  float32 in with float32 out is ``bilateral_slice_apply_upadd`` itself.  No autograd."""
    input_white_level = _frame_head(input, input_white_level, out_dtype)
    if guide_curves is not None:
        raise ValueError("bilateral_slice_apply_upadd_io takes a guide map or the guide network: the curves guide has no "
                         "up-add form")
    B, H, W, GH, GW, GD, Cin, Cout = _check_io(grid, input, has_offset)
    if (Cin, Cout) != (3, 3) or not has_offset:
        raise ValueError(f"bilateral_slice_apply_upadd_io supports Cin = Cout = 3 with offset, got Cin = {Cin}, "
                         f"Cout = {Cout}, has_offset = {bool(has_offset)}")
    _require_f32("coarse", coarse)
    if coarse.dim() != 4 or coarse.shape[0] != B or coarse.shape[3] != Cout or min(coarse.shape[1], coarse.shape[2]) < 1:
        raise ValueError(f"coarse should be [B, Hc, Wc, Cout] = [{B}, >= 1, >= 1, {Cout}], got {tuple(coarse.shape)}")
    (guide, c1, c2), n = _guide_source(guide, guide_conv1, guide_conv2, None, None, False, (B, H, W), Cin)[1:]
    for nm, t in (("grid", grid), ("input", input), ("coarse", coarse)):
        _require_gpu(nm, t)
    grid, inp, coarse = grid.detach().contiguous(), input.detach().contiguous(), coarse.detach().contiguous()
    dev = inp.device
    out = torch.empty((B, H, W, Cout), dtype=out_dtype, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        rc = lib.hdrnet_bilateral_slice_apply_upadd_io_ex(
            grid.data_ptr(), _ptr(guide), inp.data_ptr(), coarse.data_ptr(), coarse.shape[1], coarse.shape[2],
            out.data_ptr(), B, H, W, GH, GW, GD, Cin, Cout, int(bool(has_offset)), _DTYPE_CODE[input.dtype],
            float(input_white_level), _DTYPE_CODE[out_dtype], _ptr(c1), _ptr(c2), n,
            _guide_flags(fast_sigmoid, prescaled and guide is None), _stream(dev))
    _lib.check(rc, "BilateralSliceApplyUpAddIO")
    return out


# ---- the pyramid model on YUV 4:2:0 surfaces (include/hdrnet_amd_pyramid_yuv.h) ---------------------------------------------
def _check_coarse(what: str, coarse, B: int) -> torch.Tensor:
    """The coarser pyramid level of an up-add on a surface: float32 ``[B, Hc, Wc, 3]`` with Hc, Wc >= 1."""
    _require_f32("coarse", coarse)
    if coarse.dim() != 4 or coarse.shape[0] != B or coarse.shape[3] != 3 or min(coarse.shape[1], coarse.shape[2]) < 1:
        raise ValueError(f"{what}: coarse should be [B, Hc, Wc, 3] = [{B}, >= 1, >= 1, 3], got {tuple(coarse.shape)}")
    return coarse


def _resize_extents(what: str, height, width):
    if int(height) < 0 or int(width) < 0:
        raise ValueError(f"{what}: bad output extents {height} x {width}")
    return int(height), int(width)


def resize_bilinear_yuv(y: torch.Tensor, uv: torch.Tensor, to_rgb: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """``resize_bilinear(yuv_to_rgb(y, uv, to_rgb), height, width)`` in one pass, without the RGB frame
    (``hdrnet_resize_bilinear_yuv``, include/hdrnet_amd_pyramid_yuv.h): ``y`` ``[B, H, W]``, ``uv`` ``[B, H / 2, W]``, uint8
    (NV12) or uint16 (P010 / P016), float32 ``[B, height, width, 3]`` out -- level 1 of ``HDRNetGaussianPyrNN``'s input
    pyramid from a decoder surface.  Taps and lerps are ``resize_bilinear``'s; each tap is a pixel converted as
    ``yuv_to_rgb`` converts it (chroma from ``(row >> 1, x >> 1)``, clamped before the blend).  Planes may be pitched (taken
    as views); padding is not read.  An empty output is a no-op.  No autograd.  Out of scope: 4:2:2 / 4:4:4 surfaces."""
    what = "resize_bilinear_yuv"
    y, uv, B, H, W, surf = _yuv_surface(y, uv, what)
    to_rgb = _yuv_constants("to_rgb", to_rgb, what)
    height, width = _resize_extents(what, height, width)
    for nm, t in (("y", y), ("uv", uv), ("to_rgb", to_rgb)):
        _require_gpu(nm, t)
    dev = y.device
    k = to_rgb.detach().contiguous()
    out = torch.empty((B, height, width, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().hdrnet_resize_bilinear_yuv(y.data_ptr(), uv.data_ptr(), *surf, B, H, W, k.data_ptr(), out.data_ptr(),
                                                    height, width, _stream(dev))
    _lib.check(rc, "ResizeBilinearYuv")
    return out


def resize_bilinear_yuv_planar(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, to_rgb: torch.Tensor, height: int,
                               width: int) -> torch.Tensor:
    """``resize_bilinear_yuv`` for a PLANAR 4:2:0 surface (``hdrnet_resize_bilinear_yuv_planar``): ``y`` ``[B, H, W]``, ``u``
    and ``v`` ``[B, H / 2, W / 2]``, uint8 (I420) or uint16 with the code in the low bits; ``to_rgb`` of
    ``yuv.yuv_coefficients(..., msb_aligned=False)``.  The bits of ``resize_bilinear_yuv`` on the interleaved surface.  No
    autograd.  Out of scope: 4:2:2 / 4:4:4 surfaces."""
    what = "resize_bilinear_yuv_planar"
    B, H, W, surf = _yuv_planar_surface(y, u, v, what)
    to_rgb = _yuv_constants("to_rgb", to_rgb, what)
    height, width = _resize_extents(what, height, width)
    for nm, t in (("y", y), ("u", u), ("v", v), ("to_rgb", to_rgb)):
        _require_gpu(nm, t)
    dev = y.device
    k = to_rgb.detach().contiguous()
    out = torch.empty((B, height, width, 3), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.load().hdrnet_resize_bilinear_yuv_planar(y.data_ptr(), u.data_ptr(), v.data_ptr(), *surf, B, H, W,
                                                           k.data_ptr(), out.data_ptr(), height, width, _stream(dev))
    _lib.check(rc, "ResizeBilinearYuvPlanar")
    return out


def bilateral_slice_apply_upadd_io_yuv(grid: torch.Tensor, y: torch.Tensor, uv: torch.Tensor, to_rgb: torch.Tensor,
                                       coarse: torch.Tensor,
                                       guide: Optional[torch.Tensor] = None,
                                       guide_conv1: Optional[torch.Tensor] = None,
                                       guide_conv2: Optional[torch.Tensor] = None,
                                       fast_sigmoid: bool = False, prescaled: bool = False,
                                       out: str = "rgb", out_dtype: Optional[torch.dtype] = None,
                                       from_rgb: Optional[torch.Tensor] = None, out_bits: Optional[int] = None,
                                       out_planes=None, guide_curves=None):
    """The finest level of ``HDRNetGaussianPyrNN._output`` on a semi-planar YUV 4:2:0 surface
    (include/hdrnet_amd_pyramid_yuv.h): ``bilateral_slice_apply_upadd_io`` with the load and the stores of
    ``bilateral_slice_apply_io_yuv`` / ``..._yuv_deep`` --
    ``wire_out(bilateral_slice_apply(grid, guide, yuv_to_rgb(y, uv, to_rgb)) + resize_bilinear(coarse -> H x W))`` in one pass,
    without the RGB frame.  ``coarse`` float32 ``[B, Hc, Wc, 3]``.  ``out="rgb"``: ``[B, H, W, 3]``, ``out_dtype`` float32
    (default) or uint8; ``out="nv12"``: an NV12 uint8 surface ``(y_out, uv_out)`` encoded by ``from_rgb``; ``out="p010"`` /
    ``"p016"`` (from a uint16 surface): a uint16 surface of 10- / 16-bit codes in the high bits, ``from_rgb`` of
    ``yuv.yuv_encode_coefficients`` (``out_bits`` may repeat the depth).  The clip, the luma code and the 2 x 2 chroma sums
    see the value after the add.  ``out_planes``: the pair to write into (pitched planes are fine).  The guide is a ``guide``
    map or the folded guide network (``fast_sigmoid`` / ``prescaled`` as everywhere); the curves guide belongs to the
    single-level models and is refused.  Cin = Cout = 3 with offset, H even, W % 4 == 0.  No autograd.  Out of scope:
    4:2:2 / 4:4:4 surfaces, a uint16 RGB frame out, BGR / RGBA frames, the curves guide, training."""
    what = "bilateral_slice_apply_upadd_io_yuv"
    if guide_curves is not None:
        raise ValueError(f"{what} takes a guide map or the guide network: the curves guide has no up-add form")
    if out not in ("rgb", "nv12", "p010", "p016"):
        raise ValueError(f"{what}: unknown out {out!r} (takes 'rgb', 'nv12', 'p010', 'p016')")
    if coarse is None:
        raise ValueError(f"{what}: needs coarse, the coarser pyramid level [B, Hc, Wc, 3]")
    if out in ("p010", "p016"):
        bits = 10 if out == "p010" else 16
        if out_bits not in (None, bits):
            raise ValueError(f"{what}: out={out!r} has out_bits = {bits}, got {out_bits!r}")
        if out_dtype not in (None, torch.uint16):
            raise TypeError(f"{what}: a {out.upper()} output is uint16, got out_dtype = {out_dtype}")
        if from_rgb is None:
            raise ValueError(f"{what}: out={out!r} needs from_rgb (yuv.yuv_encode_coefficients)")
        return _apply_io_surface(what, torch.uint16, None, grid, y, uv, to_rgb, guide, guide_conv1, guide_conv2, None, False,
                                 fast_sigmoid, prescaled, None, from_rgb, out_planes, bits, coarse=coarse)
    if out_bits is not None:
        raise ValueError(f"{what}: out_bits belongs to out='p010' / 'p016'")
    if out == "rgb":
        out_dtype = torch.float32 if out_dtype is None else out_dtype
        if out_dtype not in (torch.float32, torch.uint8):
            raise TypeError(f"{what}: out_dtype must be float32 or uint8, got {out_dtype}")
        if from_rgb is not None or out_planes is not None:
            raise ValueError(f"{what}: from_rgb / out_planes belong to a surface output")
    else:
        if out_dtype not in (None, torch.uint8):
            raise TypeError(f"{what}: an NV12 output is uint8, got out_dtype = {out_dtype}")
        if from_rgb is None:
            raise ValueError(f"{what}: out='nv12' needs from_rgb (yuv.yuv_coefficients)")
    return _apply_io_surface(what, None if out == "rgb" else torch.uint8, out_dtype, grid, y, uv, to_rgb, guide, guide_conv1,
                             guide_conv2, None, False, fast_sigmoid, prescaled, None, from_rgb, out_planes, coarse=coarse)


def bilateral_slice_apply_upadd_io_yuv_planar(grid: torch.Tensor, y: torch.Tensor, u: torch.Tensor, v: torch.Tensor,
                                              to_rgb: torch.Tensor, coarse: torch.Tensor,
                                              guide: Optional[torch.Tensor] = None,
                                              guide_conv1: Optional[torch.Tensor] = None,
                                              guide_conv2: Optional[torch.Tensor] = None,
                                              fast_sigmoid: bool = False, prescaled: bool = False,
                                              out: str = "rgb", out_dtype: Optional[torch.dtype] = None,
                                              from_rgb: Optional[torch.Tensor] = None, out_bits: Optional[int] = None,
                                              out_planes=None, guide_curves=None):
    """``bilateral_slice_apply_upadd_io_yuv`` for a PLANAR 4:2:0 surface (I420, yuv420p10le / yuv420p16le): the load and the
    stores of ``bilateral_slice_apply_io_yuv_planar`` with the up-add of ``coarse`` before any store -- the bits of the
    semi-planar op on the interleaved surface.  ``out="rgb"`` (float32 / uint8) or ``out="planar"``: a planar surface
    ``(y_out, u_out, v_out)`` of the input's dtype, ``from_rgb`` / ``out_bits`` / ``out_planes`` as there.  No autograd.  Out
    of scope: 4:2:2 / 4:4:4 surfaces, a uint16 RGB frame out, the curves guide, training."""
    what = "bilateral_slice_apply_upadd_io_yuv_planar"
    if guide_curves is not None:
        raise ValueError(f"{what} takes a guide map or the guide network: the curves guide has no up-add form")
    if coarse is None:
        raise ValueError(f"{what}: needs coarse, the coarser pyramid level [B, Hc, Wc, 3]")
    return _apply_io_planar(what, grid, y, u, v, to_rgb, guide, guide_conv1, guide_conv2, None, False, fast_sigmoid, prescaled,
                            None, out, out_dtype, from_rgb, out_bits, out_planes, "420", coarse=coarse)
