"""Sample preparation on the device -- the reference's ``hdrnet/data_pipeline.py`` from the decoded image onwards.

The reference decodes a ``uint8`` / ``uint16`` image pair, divides by the white level, flips, rotates by quarter turns,
crops, and takes a nearest-neighbour ``net_input_size`` copy as ``lowres_input`` (``data_pipeline.py:126-171, 228-241,
267-287``; per inference frame ``hdrnet/bin/run.py:166-169`` and ``benchmark/src/processor.cc:109-122``).  Here the
images stay in device memory in their wire format and ONE HIP launch (``csrc/sample_prep.hip``,
``hdrnet_prepare_batch`` / ``hdrnet_lowres_input``) writes the fp32 NHWC tensors the models and the training step
consume, bit for bit the reference's arithmetic:

* ``lowres_input(frames)``: the inference half -- a frame in, the coefficient network's input out;
* ``draw_ops`` + ``prepare_batch``: the training half -- a table of per-sample records (source index, flips, quarter
  turns, crop offsets) drawn on the host, read on the device, so that a captured graph replays with new draws after a
  128-byte copy;
* ``DeviceDataset``: both around a set of images, with ``feed(step)`` writing straight into a ``GraphedTrainStep``'s
  static buffers.

The nearest-neighbour rule is TF1's ``ResizeNearestNeighbor(align_corners=False)`` = OpenCV's ``INTER_NEAREST``:
``src = min(floor(dst * (size / float32(n))), size - 1)`` in fp32.  ``run.py``'s ``skimage`` resize is centre-aligned and
is not what the training pipeline or the benchmark computes; it is not followed.

There is no CPU or eager path: tensors must live on the GPU.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _lib

__all__ = ["lowres_input", "draw_ops", "prepare_batch", "DeviceDataset"]

_DTYPE_CODE = {torch.float32: 0, torch.uint8: 1, torch.uint16: 2}
_WHITE = {torch.float32: 1.0, torch.uint8: 255.0, torch.uint16: 65535.0}
OPS_FIELDS = ("index", "flip_lr", "flip_ud", "rot90", "crop_y", "crop_x", "reserved0", "reserved1")


def _stream(device: torch.device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _check_sources(name: str, t: torch.Tensor) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[3] != 3:
        raise ValueError(f"{name} should be [N, H, W, 3], got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.dtype not in _DTYPE_CODE:
        raise TypeError(f"{name} must be float32, uint8 or uint16, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: sample preparation runs on an MI355X (HIP) device only")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous (NHWC)")


def _check_out(name: str, t: torch.Tensor, shape: Tuple[int, ...], device: torch.device) -> None:
    if tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != device or not t.is_contiguous():
        raise ValueError(f"out: {name} should be a contiguous float32 {list(shape)} tensor on {device}, got "
                         f"{list(t.shape)} {t.dtype} on {t.device}")


def lowres_input(frames: torch.Tensor, net_input_size: int = 256, white_level: Optional[float] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``[B, H, W, 3]`` frames (uint8 / uint16 / float32, on the device) -> the coefficient network's input
    ``[B, n, n, 3]`` float32: nearest neighbour (TF1 / OpenCV rule, see the module text) of ``frames / white_level``.
    Default white levels are those of ``hdrnet_ops.bilateral_slice_apply_io``: 255 / 65535 / 1 (float32 is copied
    unscaled).  One launch on the current stream; capturable."""
    _check_sources("frames", frames)
    B, H, W, _ = frames.shape
    n = int(net_input_size)
    if white_level is None:
        white_level = _WHITE[frames.dtype]
    if out is None:
        out = torch.empty((B, n, n, 3), dtype=torch.float32, device=frames.device)
    else:
        _check_out("lowres_input", out, (B, n, n, 3), frames.device)
    with torch.cuda.device(frames.device):
        rc = _lib.load().hdrnet_lowres_input(frames.data_ptr(), _DTYPE_CODE[frames.dtype], float(white_level), B, H, W,
                                             out.data_ptr(), n, _stream(frames.device))
    _lib.check(rc, "LowresInput")
    return out


def _rotate_mode(rotate) -> str:
    if rotate == "even":
        return "even"
    return "all" if rotate else "none"


def draw_ops(batch: int, n_sources: int, source_hw: Sequence[int], crop_hw: Sequence[int], fliplr: bool = True,
             flipud: bool = True, rotate=True, random_crop: bool = True,
             generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """A CPU int32 ``[batch, 8]`` table of records ``{index, flip_lr, flip_ud, rot90, crop_y, crop_x, 0, 0}`` drawn
    uniformly with ``generator``: what ``_augment_data`` draws per sample (``data_pipeline.py:126-158``), plus the
    source index.  ``rotate``: ``True`` (0 .. 3 quarter turns, counter-clockwise), ``"even"`` (0 or 2) or ``False``.
    Without ``random_crop`` the crop is the reference's centre crop, ``int((dim - size) / 2)`` of the extents AFTER the
    rotation.  Raises ``ValueError`` where the crop does not fit the source, or a requested rotation cannot fit."""
    Hs, Ws = (int(v) for v in source_hw)
    H, W = (int(v) for v in crop_hw)
    batch, n_sources = int(batch), int(n_sources)
    if batch < 0 or n_sources <= 0 or min(Hs, Ws, H, W) <= 0:
        raise ValueError("draw_ops: non-positive extent")
    if H > Hs or W > Ws:
        raise ValueError(f"draw_ops: the crop {H} x {W} does not fit the {Hs} x {Ws} source")
    mode = _rotate_mode(rotate)
    if mode == "all" and (H > Ws or W > Hs):
        raise ValueError(f"draw_ops: the crop {H} x {W} does not fit the source turned by 90 degrees ({Ws} x {Hs}); "
                         "use rotate='even' or rotate=False")

    def rnd(high: int) -> torch.Tensor:
        return torch.randint(0, high, (batch,), generator=generator, dtype=torch.int64)

    ops = torch.zeros((batch, 8), dtype=torch.int64)
    ops[:, 0] = rnd(n_sources)
    if fliplr:
        ops[:, 1] = rnd(2)
    if flipud:
        ops[:, 2] = rnd(2)
    if mode == "all":
        ops[:, 3] = rnd(4)
    elif mode == "even":
        ops[:, 3] = 2 * rnd(2)
    odd = (ops[:, 3] & 1).bool()
    room_y = torch.where(odd, Ws - H, Hs - H)  # extents after the rotation
    room_x = torch.where(odd, Hs - W, Ws - W)
    if random_crop:
        # one uniform draw per offset, scaled to the sample's own room (which depends on its turn)
        uy = torch.rand((batch,), generator=generator, dtype=torch.float64)
        ux = torch.rand((batch,), generator=generator, dtype=torch.float64)
        ops[:, 4] = torch.minimum((uy * (room_y + 1).double()).floor().long(), room_y)
        ops[:, 5] = torch.minimum((ux * (room_x + 1).double()).floor().long(), room_x)
    else:
        ops[:, 4] = room_y // 2  # int((dim - size) / 2), data_pipeline.py:154-158 (room >= 0)
        ops[:, 5] = room_x // 2
    return ops.to(torch.int32)


def check_ops(ops: torch.Tensor, n_sources: int, source_hw: Sequence[int], crop_hw: Sequence[int],
              even_turns_only: bool = False) -> None:
    """Raise ``ValueError`` unless every record of a CPU table is in range and its crop fits the turned source."""
    if ops.dim() != 2 or ops.shape[1] != 8 or ops.dtype != torch.int32:
        raise ValueError(f"ops should be int32 [batch, 8], got {ops.dtype} {list(ops.shape)}")
    Hs, Ws = (int(v) for v in source_hw)
    H, W = (int(v) for v in crop_hw)
    o = ops.long()
    if o.numel() == 0:
        return
    rot = o[:, 3]
    if ((o[:, 0] < 0) | (o[:, 0] >= n_sources)).any():
        raise ValueError(f"ops: a source index outside [0, {n_sources})")
    if ((o[:, 1] < 0) | (o[:, 1] > 1) | (o[:, 2] < 0) | (o[:, 2] > 1) | (rot < 0) | (rot > 3)).any():
        raise ValueError("ops: flips must be 0 / 1 and rot90 0 .. 3")
    if even_turns_only and (rot & 1).any():
        raise ValueError("ops: an odd quarter turn with even_turns_only")
    odd = (rot & 1).bool()
    room_y = torch.where(odd, Ws - H, Hs - H)
    room_x = torch.where(odd, Hs - W, Ws - W)
    if ((o[:, 4] < 0) | (o[:, 4] > room_y) | (o[:, 5] < 0) | (o[:, 5] > room_x)).any():
        raise ValueError(f"ops: a crop {H} x {W} at its offset does not fit the (turned) {Hs} x {Ws} source")
    if (o[:, 6:] != 0).any():
        raise ValueError("ops: the two reserved fields must be 0")


def prepare_batch(src_input: torch.Tensor, src_target: Optional[torch.Tensor], ops: Optional[torch.Tensor],
                  crop_hw: Sequence[int], net_input_size: int = 256, input_white_level: Optional[float] = None,
                  target_white_level: Optional[float] = None, out: Optional[Sequence[Optional[torch.Tensor]]] = None,
                  even_turns_only: bool = False):
    """One launch: ``(lowres_input [B, n, n, 3], image_input [B, H, W, 3], image_target [B, H, W, 3])`` float32 from the
    wire-format sources ``src_input`` / ``src_target`` ``[N, Hs, Ws, 3]`` (uint8 / uint16 / float32, each with its own
    white level; ``src_target`` may be ``None``: no ``image_target``) and the table ``ops`` (``draw_ops``).

    ``ops``: a CPU table is validated (``ValueError``) and copied to the device; a DEVICE table is used as it is -- the
    kernel reads it, so a captured graph follows later copies into it -- and its records are clamped on the device
    (index, crop offsets) or masked (turns, flips): a bad record is a caller error whose result is the clamped sample,
    never an out-of-bounds access.  ``None``: the identity, sample b = source b (needs ``crop_hw`` = the source's).
    ``out``: ``(lowres_input, image_input, image_target)`` destination tensors, e.g. the static buffers of a
    ``GraphedTrainStep``; an entry ``None`` skips that output.  ``even_turns_only``: the device reads ``rot90 & 2`` -- for
    crops that do not fit the source turned by 90 degrees."""
    _check_sources("src_input", src_input)
    dev = src_input.device
    N, Hs, Ws, _ = src_input.shape
    if src_target is not None:
        _check_sources("src_target", src_target)
        if tuple(src_target.shape) != tuple(src_input.shape) or src_target.device != dev:
            raise ValueError("src_target should have src_input's shape and device")
    H, W = (int(v) for v in crop_hw)
    n = int(net_input_size)
    if ops is None:
        B = N
    else:
        if ops.dim() != 2 or ops.shape[1] != 8 or ops.dtype != torch.int32:
            raise ValueError(f"ops should be int32 [batch, 8], got {ops.dtype} {list(ops.shape)}")
        B = ops.shape[0]
        if not ops.is_cuda:
            check_ops(ops, N, (Hs, Ws), (H, W), even_turns_only)
            ops = ops.to(dev, non_blocking=True)
        elif ops.device != dev or not ops.is_contiguous():
            raise ValueError("a device ops table must be contiguous and on the sources' device")
    if input_white_level is None:
        input_white_level = _WHITE[src_input.dtype]
    if target_white_level is None:
        target_white_level = _WHITE[src_target.dtype] if src_target is not None else 1.0
    shapes = ((B, n, n, 3), (B, H, W, 3), (B, H, W, 3))
    names = ("lowres_input", "image_input", "image_target")
    if out is None:
        res = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
        if src_target is None:
            res[2] = None
    else:
        res = list(out)
        if len(res) != 3:
            raise ValueError("out should be (lowres_input, image_input, image_target); None skips an output")
        for nm, t, s in zip(names, res, shapes):
            if t is not None:
                _check_out(nm, t, s, dev)
        if res[2] is not None and src_target is None:
            raise ValueError("out: image_target given without src_target")
    ptr = [None if t is None else t.data_ptr() for t in res]
    with torch.cuda.device(dev):
        rc = _lib.load().hdrnet_prepare_batch(
            src_input.data_ptr(), _DTYPE_CODE[src_input.dtype], float(input_white_level),
            None if src_target is None else src_target.data_ptr(),
            0 if src_target is None else _DTYPE_CODE[src_target.dtype], float(target_white_level), N, Hs, Ws,
            None if ops is None else ops.data_ptr(), B, ptr[1], ptr[2], H, W, ptr[0], n,
            _lib.SAMPLE_EVEN_TURNS_ONLY if even_turns_only else 0, _stream(dev))
    _lib.check(rc, "PrepareBatch")
    return tuple(res)


class DeviceDataset:
    """A set of image pairs held on the device in their wire format (u8: 6 bytes per pixel pair instead of the 24 of
    prepared fp32 samples) and expanded there: ``next_batch`` draws a table (``draw_ops``) and prepares the batch in one
    launch; ``feed(step)`` does so straight into a ``runtime.GraphedTrainStep``'s static buffers.

    ``inputs`` / ``targets``: ``[N, Hs, Ws, 3]`` uint8 / uint16 / float32 device tensors (``targets`` may be ``None``);
    ``output_resolution``: the crop ``(H, W)``; the augmentation switches are ``draw_ops``'s.  With ``rotate='even'`` the
    crop may exceed the source's transposed extents (the kernel then masks odd turns)."""

    def __init__(self, inputs: torch.Tensor, targets: Optional[torch.Tensor] = None,
                 input_white_level: Optional[float] = None, target_white_level: Optional[float] = None,
                 output_resolution: Optional[Sequence[int]] = None, net_input_size: int = 256, fliplr: bool = True,
                 flipud: bool = True, rotate=True, random_crop: bool = True,
                 generator: Optional[torch.Generator] = None):
        _check_sources("inputs", inputs)
        if targets is not None:
            _check_sources("targets", targets)
            if tuple(targets.shape) != tuple(inputs.shape) or targets.device != inputs.device:
                raise ValueError("targets should have inputs' shape and device")
        self.inputs, self.targets = inputs, targets
        self.input_white_level, self.target_white_level = input_white_level, target_white_level
        self.source_hw = (inputs.shape[1], inputs.shape[2])
        self.output_resolution = tuple(int(v) for v in (output_resolution or self.source_hw))
        self.net_input_size = int(net_input_size)
        self.fliplr, self.flipud, self.rotate, self.random_crop = fliplr, flipud, rotate, random_crop
        self.generator = generator
        self._tables: dict = {}  # batch -> the device table this dataset's launches read
        draw_ops(0, len(self), self.source_hw, self.output_resolution, rotate=rotate)  # does the geometry fit at all?

    def __len__(self) -> int:
        return self.inputs.shape[0]

    def draw(self, batch: int) -> torch.Tensor:
        return draw_ops(batch, len(self), self.source_hw, self.output_resolution, self.fliplr, self.flipud, self.rotate,
                        self.random_crop, self.generator)

    def next_batch(self, batch: int, out: Optional[Sequence[Optional[torch.Tensor]]] = None, ops: Optional[torch.Tensor] = None):
        """Draw ``batch`` records (or take the CPU table ``ops``) and prepare them:
        ``(lowres_input, image_input, image_target)``, into ``out`` if given."""
        table = self.draw(batch) if ops is None else ops
        check_ops(table, len(self), self.source_hw, self.output_resolution, _rotate_mode(self.rotate) == "even")
        dev_table = self._tables.get(batch)
        if dev_table is None:
            dev_table = self._tables[batch] = torch.zeros((batch, 8), dtype=torch.int32, device=self.inputs.device)
        dev_table.copy_(table, non_blocking=True)
        return prepare_batch(self.inputs, self.targets, dev_table, self.output_resolution, self.net_input_size,
                             self.input_white_level, self.target_white_level, out=out,
                             even_turns_only=_rotate_mode(self.rotate) == "even")

    def feed(self, step, ops: Optional[torch.Tensor] = None):
        """Prepare the next batch INTO ``step``'s current static buffers (``static_inputs = [lowres, fullres]``,
        ``static_targets = [target]``) and return ``(inputs, targets)`` to pass to ``step(inputs, targets)``, which then
        finds its own buffers (``data_ptr()`` identity) and copies nothing."""
        if self.targets is None:
            raise ValueError("feed() needs a dataset with targets")
        low, full = step.static_inputs
        (target,) = step.static_targets
        self.next_batch(full.shape[0], out=(low, full, target), ops=ops)
        return [low, full], [target]
