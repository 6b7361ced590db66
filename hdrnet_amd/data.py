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
  static buffers;
* ``pack_images`` + ``prepare_batch_ragged`` + ``DeviceDataset.from_images``: the same for a set of images of MIXED
  extents (the reference's pipelines decode files of any size and crop each to ``output_resolution``,
  ``data_pipeline.py:143-158, 183-287``): the images lie back to back in one flat buffer, a table of
  ``{offset, Hs, Ws}`` descriptors says where, and every crop is drawn from its own image's extents;
* ``order=`` of the dataset classes: ``"random"`` draws, ``"epoch"`` (a shuffled pass with every image once,
  ``data_pipeline.py:190-200``) or ``"sequential"`` (the evaluation pipeline's ``shuffle=False``).

The nearest-neighbour rule is TF1's ``ResizeNearestNeighbor(align_corners=False)`` = OpenCV's ``INTER_NEAREST``:
``src = min(floor(dst * (size / float32(n))), size - 1)`` in fp32.  ``run.py``'s ``skimage`` resize is centre-aligned and
is not what the training pipeline or the benchmark computes; it is not followed.

There is no CPU or eager path: tensors must live on the GPU.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _lib

__all__ = ["lowres_input", "lowres_input_yuv", "lowres_input_yuv_planar", "draw_ops", "check_ops", "prepare_batch", "DeviceDataset", "pack_images",
           "prepare_batch_ragged", "RaggedDeviceDataset"]

_DTYPE_CODE = {torch.float32: 0, torch.uint8: 1, torch.uint16: 2}
_WHITE = {torch.float32: 1.0, torch.uint8: 255.0, torch.uint16: 65535.0}
OPS_FIELDS = ("index", "flip_lr", "flip_ud", "rot90", "crop_y", "crop_x", "reserved0", "reserved1")
IMAGE_FIELDS = ("offset_lo", "offset_hi", "Hs", "Ws")  # a descriptor of the ragged flavour; the offset in samples
ORDERS = ("random", "epoch", "sequential")


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
                 out: Optional[torch.Tensor] = None, pixel_format: str = "rgb") -> torch.Tensor:
    """``[B, H, W, 3]`` frames (uint8 / uint16 / float32, on the device) -> the coefficient network's input
    ``[B, n, n, 3]`` float32: nearest neighbour (TF1 / OpenCV rule, see the module text) of ``frames / white_level``.
    Default white levels are those of ``hdrnet_ops.bilateral_slice_apply_io``: 255 / 65535 / 1 (float32 is copied
    unscaled).  One launch on the current stream; capturable.

    ``pixel_format``: ``"rgb"`` (default), ``"bgr"``, or ``"rgba"`` / ``"bgra"`` for ``[B, H, W, 4]`` frames
    (uint8 / uint16 only; ``hdrnet_lowres_input_px``).  The result is RGB whatever the format -- the bits of this call on
    the repacked frame -- and alpha is not read.  Training-side sample preparation (``prepare_batch``) stays RGB."""
    if pixel_format != "rgb":
        if not isinstance(frames, torch.Tensor) or frames.dim() != 4:
            raise ValueError(f"frames should be [N, H, W, 3 or 4], got "
                             f"{tuple(frames.shape) if isinstance(frames, torch.Tensor) else type(frames).__name__}")
        pixel_format = _lib.pixel_format(pixel_format, frames.shape[3], frames.dtype == torch.float32, "lowres_input")
    if pixel_format != "rgb":
        return _lowres_input_px(frames, int(net_input_size), white_level, out, pixel_format)
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


def _lowres_input_px(frames, n: int, white_level, out, pixel_format: str) -> torch.Tensor:
    if frames.dtype not in _DTYPE_CODE:
        raise TypeError(f"frames must be float32, uint8 or uint16, got {frames.dtype}")
    if not frames.is_cuda:
        raise RuntimeError(f"frames is on {frames.device}: sample preparation runs on an MI355X (HIP) device only")
    if not frames.is_contiguous():
        raise ValueError("frames must be contiguous (NHWC)")
    B, H, W, _ = frames.shape
    if white_level is None:
        white_level = _WHITE[frames.dtype]
    if out is None:
        out = torch.empty((B, n, n, 3), dtype=torch.float32, device=frames.device)
    else:
        _check_out("lowres_input", out, (B, n, n, 3), frames.device)
    with torch.cuda.device(frames.device):
        rc = _lib.load().hdrnet_lowres_input_px(frames.data_ptr(), _DTYPE_CODE[frames.dtype], float(white_level), B, H, W,
                                                out.data_ptr(), n, _lib.PIXEL_FORMATS[pixel_format],
                                                _stream(frames.device))
    _lib.check(rc, "LowresInput")
    return out


def lowres_input_yuv(y: torch.Tensor, uv: torch.Tensor, to_rgb: torch.Tensor, net_input_size: int = 256,
                     out: Optional[torch.Tensor] = None, chroma: str = "420") -> torch.Tensor:
    """``lowres_input`` of a semi-planar YUV 4:2:0 surface (``hdrnet_lowres_input_yuv``, include/hdrnet_amd_yuv.h): ``y``
    ``[B, H, W]``, ``uv`` ``[B, H / 2, W]`` (interleaved U, V), uint8 (NV12) or uint16 (P010 / P016), possibly pitched;
    ``to_rgb`` the 12 floats of ``yuv.yuv_coefficients`` on the device.  The same source pixel per output sample as
    ``lowres_input``, its chroma from ``(y >> 1, x >> 1)``: the bits of ``lowres_input(hdrnet_ops.yuv_to_rgb(y, uv,
    to_rgb))`` without the float32 frame.  One launch on the current stream; capturable.  ``chroma="422"``
    (include/hdrnet_amd_yuv_chroma.h): an NV16 / P210 / P216 surface, ``uv`` ``[B, H, W]``, chroma from ``(y, x >> 1)``."""
    from . import hdrnet_ops
    what = "lowres_input_yuv"
    chroma = hdrnet_ops._check_chroma(what, chroma, False)
    y, uv, B, H, W, surf = hdrnet_ops._yuv_surface(y, uv, what, chroma=chroma)
    to_rgb = hdrnet_ops._yuv_constants("to_rgb", to_rgb, what)
    n = int(net_input_size)
    if n <= 0:
        raise ValueError(f"{what}: net_input_size must be positive, got {net_input_size}")
    for nm, t in (("y", y), ("uv", uv), ("to_rgb", to_rgb)):
        if not t.is_cuda:
            raise RuntimeError(f"{nm} is on {t.device}: sample preparation runs on an MI355X (HIP) device only")
    k = to_rgb.detach().contiguous()
    if out is None:
        out = torch.empty((B, n, n, 3), dtype=torch.float32, device=y.device)
    else:
        _check_out("lowres_input", out, (B, n, n, 3), y.device)
    with torch.cuda.device(y.device):
        if chroma != "420":
            rc = _lib.load().hdrnet_lowres_input_yuv_chroma(y.data_ptr(), uv.data_ptr(), *surf, _lib.CHROMA[chroma], B, H, W,
                                                            k.data_ptr(), out.data_ptr(), n, _stream(y.device))
        else:
            rc = _lib.load().hdrnet_lowres_input_yuv(y.data_ptr(), uv.data_ptr(), *surf, B, H, W, k.data_ptr(), out.data_ptr(),
                                                     n, _stream(y.device))
    _lib.check(rc, "LowresInput")
    return out


def lowres_input_yuv_planar(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, to_rgb: torch.Tensor,
                            net_input_size: int = 256, out: Optional[torch.Tensor] = None,
                            chroma: str = "420") -> torch.Tensor:
    """``lowres_input_yuv`` of a PLANAR YUV 4:2:0 surface (``hdrnet_lowres_input_yuv_planar``,
    include/hdrnet_amd_yuv_planar.h): ``y`` ``[B, H, W]``, ``u`` and ``v`` ``[B, H / 2, W / 2]``, uint8 (I420) or uint16 with
    the code in the low bits, possibly pitched; ``to_rgb`` the 12 floats of ``yuv.yuv_coefficients(...,
    msb_aligned=False)`` on the device.  The bits of ``lowres_input_yuv`` on the interleaved surface.  One launch on the
    current stream; capturable.  ``chroma`` (include/hdrnet_amd_yuv_chroma.h): ``"422"`` -- ``u`` and ``v`` ``[B, H, W / 2]``,
    chroma from ``(y, x >> 1)`` -- or ``"444"`` -- ``[B, H, W]``, chroma from ``(y, x)``."""
    from . import hdrnet_ops
    what = "lowres_input_yuv_planar"
    chroma = hdrnet_ops._check_chroma(what, chroma, True)
    B, H, W, surf = hdrnet_ops._yuv_planar_surface(y, u, v, what, chroma=chroma)
    to_rgb = hdrnet_ops._yuv_constants("to_rgb", to_rgb, what)
    n = int(net_input_size)
    if n <= 0:
        raise ValueError(f"{what}: net_input_size must be positive, got {net_input_size}")
    for nm, t in (("y", y), ("u", u), ("v", v), ("to_rgb", to_rgb)):
        if not t.is_cuda:
            raise RuntimeError(f"{nm} is on {t.device}: sample preparation runs on an MI355X (HIP) device only")
    k = to_rgb.detach().contiguous()
    if out is None:
        out = torch.empty((B, n, n, 3), dtype=torch.float32, device=y.device)
    else:
        _check_out("lowres_input", out, (B, n, n, 3), y.device)
    with torch.cuda.device(y.device):
        if chroma != "420":
            rc = _lib.load().hdrnet_lowres_input_yuv_planar_chroma(y.data_ptr(), u.data_ptr(), v.data_ptr(), *surf,
                                                                   _lib.CHROMA[chroma], B, H, W, k.data_ptr(), out.data_ptr(), n,
                                                                   _stream(y.device))
        else:
            rc = _lib.load().hdrnet_lowres_input_yuv_planar(y.data_ptr(), u.data_ptr(), v.data_ptr(), *surf, B, H, W,
                                                            k.data_ptr(), out.data_ptr(), n, _stream(y.device))
    _lib.check(rc, "LowresInput")
    return out


def lowres_input_yuv_packed(surface: torch.Tensor, to_rgb: torch.Tensor, format: str,  # noqa: A002
                            net_input_size: int = 256, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``lowres_input_yuv(..., chroma="422")`` of a PACKED 4:2:2 surface (``hdrnet_lowres_input_yuv_packed``,
    include/hdrnet_amd_yuv_packed.h): ``surface`` ``[B, H, 2 W]`` in the NAMED ``format`` (``"yuy2"`` / ``"uyvy"`` /
    ``"yvyu"`` uint8, ``"y210"`` / ``"y216"`` uint16), possibly pitched; ``to_rgb`` the 12 floats of
    ``yuv.yuv_coefficients`` on the device.  The bits of ``lowres_input_yuv`` on the de-interleaved planes.  One launch on
    the current stream; capturable."""
    from . import hdrnet_ops
    what = "lowres_input_yuv_packed"
    format = hdrnet_ops.packed_format(what, format)  # noqa: A001
    surface, B, H, W, surf = hdrnet_ops._yuv_packed_surface(surface, format, what)
    to_rgb = hdrnet_ops._yuv_constants("to_rgb", to_rgb, what)
    n = int(net_input_size)
    if n <= 0:
        raise ValueError(f"{what}: net_input_size must be positive, got {net_input_size}")
    for nm, t in (("surface", surface), ("to_rgb", to_rgb)):
        if not t.is_cuda:
            raise RuntimeError(f"{nm} is on {t.device}: sample preparation runs on an MI355X (HIP) device only")
    k = to_rgb.detach().contiguous()
    if out is None:
        out = torch.empty((B, n, n, 3), dtype=torch.float32, device=surface.device)
    else:
        _check_out("lowres_input", out, (B, n, n, 3), surface.device)
    with torch.cuda.device(surface.device):
        rc = _lib.load().hdrnet_lowres_input_yuv_packed(surface.data_ptr(), *surf, B, H, W, k.data_ptr(), out.data_ptr(), n,
                                                        _stream(surface.device))
    _lib.check(rc, "LowresInput")
    return out


def _rotate_mode(rotate) -> str:
    if rotate == "even":
        return "even"
    return "all" if rotate else "none"


def _per_source_extents(source_hw, n_sources: int) -> Optional[torch.Tensor]:
    """``None`` for a plain ``(Hs, Ws)`` pair, else the CPU int64 ``[n_sources, 2]`` table of per-source extents."""
    if isinstance(source_hw, torch.Tensor):
        t = source_hw.detach().cpu()
    else:
        t = torch.as_tensor(source_hw)
    if t.dim() == 1:
        return None
    if t.dim() != 2 or t.shape[1] != 2 or t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError(f"source_hw should be (Hs, Ws) or an integer [N, 2] table, got {t.dtype} {list(t.shape)}")
    if t.shape[0] != n_sources:
        raise ValueError(f"source_hw lists {t.shape[0]} sources, n_sources is {n_sources}")
    return t.long()


def draw_ops(batch: int, n_sources: int, source_hw, crop_hw: Sequence[int], fliplr: bool = True,
             flipud: bool = True, rotate=True, random_crop: bool = True,
             generator: Optional[torch.Generator] = None, indices: Optional[Sequence[int]] = None) -> torch.Tensor:
    """A CPU int32 ``[batch, 8]`` table of records ``{index, flip_lr, flip_ud, rot90, crop_y, crop_x, 0, 0}`` drawn
    uniformly with ``generator``: what ``_augment_data`` draws per sample (``data_pipeline.py:126-158``), plus the
    source index.  ``rotate``: ``True`` (0 .. 3 quarter turns, counter-clockwise), ``"even"`` (0 or 2) or ``False``.
    Without ``random_crop`` the crop is the reference's centre crop, ``int((dim - size) / 2)`` of the extents AFTER the
    rotation.  Raises ``ValueError`` where the crop does not fit the source, or a requested rotation cannot fit.

    ``source_hw``: the ``(Hs, Ws)`` all sources share, or an integer ``[n_sources, 2]`` array / tensor of per-source
    extents: crop room, centre crop and the fit checks are then those of each record's OWN source, and the error names
    the first source that cannot hold the crop.  ``indices``: ``batch`` source indices to use instead of drawing them
    (nothing is then drawn for column 0).  The order of the draws is: indices, flip_lr, flip_ud, turns, crop_y, crop_x,
    each only when its switch is on."""
    H, W = (int(v) for v in crop_hw)
    batch, n_sources = int(batch), int(n_sources)
    mode = _rotate_mode(rotate)
    sizes = _per_source_extents(source_hw, n_sources) if n_sources > 0 else None
    if sizes is None:
        Hs, Ws = (int(v) for v in source_hw)
        if batch < 0 or n_sources <= 0 or min(Hs, Ws, H, W) <= 0:
            raise ValueError("draw_ops: non-positive extent")
        if H > Hs or W > Ws:
            raise ValueError(f"draw_ops: the crop {H} x {W} does not fit the {Hs} x {Ws} source")
        if mode == "all" and (H > Ws or W > Hs):
            raise ValueError(f"draw_ops: the crop {H} x {W} does not fit the source turned by 90 degrees ({Ws} x {Hs}); "
                             "use rotate='even' or rotate=False")
    else:
        if batch < 0 or min(H, W) <= 0 or int(sizes.min()) <= 0:
            raise ValueError("draw_ops: non-positive extent")
        bad = (sizes[:, 0] < H) | (sizes[:, 1] < W)
        if bad.any():
            i = int(bad.nonzero()[0])
            raise ValueError(f"draw_ops: the crop {H} x {W} does not fit source {i} ({int(sizes[i, 0])} x {int(sizes[i, 1])})")
        bad = (sizes[:, 1] < H) | (sizes[:, 0] < W)
        if mode == "all" and bad.any():
            i = int(bad.nonzero()[0])
            raise ValueError(f"draw_ops: the crop {H} x {W} does not fit source {i} turned by 90 degrees "
                             f"({int(sizes[i, 1])} x {int(sizes[i, 0])}); use rotate='even' or rotate=False")

    def rnd(high: int) -> torch.Tensor:
        return torch.randint(0, high, (batch,), generator=generator, dtype=torch.int64)

    ops = torch.zeros((batch, 8), dtype=torch.int64)
    if indices is None:
        ops[:, 0] = rnd(n_sources)
    else:
        idx = torch.as_tensor(indices, dtype=torch.int64).reshape(-1)
        if idx.numel() != batch:
            raise ValueError(f"draw_ops: {idx.numel()} indices for a batch of {batch}")
        if batch and (int(idx.min()) < 0 or int(idx.max()) >= n_sources):
            raise ValueError(f"draw_ops: an index outside [0, {n_sources})")
        ops[:, 0] = idx
    if fliplr:
        ops[:, 1] = rnd(2)
    if flipud:
        ops[:, 2] = rnd(2)
    if mode == "all":
        ops[:, 3] = rnd(4)
    elif mode == "even":
        ops[:, 3] = 2 * rnd(2)
    odd = (ops[:, 3] & 1).bool()
    if sizes is not None:  # the record's own source
        Hs, Ws = sizes[ops[:, 0], 0], sizes[ops[:, 0], 1]
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


def check_ops(ops: torch.Tensor, n_sources: int, source_hw, crop_hw: Sequence[int],
              even_turns_only: bool = False) -> None:
    """Raise ``ValueError`` unless every record of a CPU table is in range and its crop fits the turned source
    (``source_hw``: a pair, or per-source extents ``[n_sources, 2]`` -- the record's own source then)."""
    if ops.dim() != 2 or ops.shape[1] != 8 or ops.dtype != torch.int32:
        raise ValueError(f"ops should be int32 [batch, 8], got {ops.dtype} {list(ops.shape)}")
    sizes = _per_source_extents(source_hw, int(n_sources))
    if sizes is None:
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
    if sizes is not None:
        Hs, Ws = sizes[o[:, 0], 0], sizes[o[:, 0], 1]
    room_y = torch.where(odd, Ws - H, Hs - H)
    room_x = torch.where(odd, Hs - W, Ws - W)
    bad = (o[:, 4] < 0) | (o[:, 4] > room_y) | (o[:, 5] < 0) | (o[:, 5] > room_x)
    if bad.any():
        if sizes is None:
            raise ValueError(f"ops: a crop {H} x {W} at its offset does not fit the (turned) {Hs} x {Ws} source")
        b = int(bad.nonzero()[0])
        i = int(o[b, 0])
        raise ValueError(f"ops: record {b}: a crop {H} x {W} at its offset does not fit the (turned) "
                         f"{int(sizes[i, 0])} x {int(sizes[i, 1])} source {i}")
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
    res = _outputs(out, ((B, n, n, 3), (B, H, W, 3), (B, H, W, 3)), dev, src_target is not None)
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


def _outputs(out, shapes, dev, have_target: bool):
    names = ("lowres_input", "image_input", "image_target")
    if out is None:
        res = [torch.empty(s, dtype=torch.float32, device=dev) for s in shapes]
        if not have_target:
            res[2] = None
        return res
    res = list(out)
    if len(res) != 3:
        raise ValueError("out should be (lowres_input, image_input, image_target); None skips an output")
    for nm, t, s in zip(names, res, shapes):
        if t is not None:
            _check_out(nm, t, s, dev)
    if res[2] is not None and not have_target:
        raise ValueError("out: image_target given without src_target")
    return res


def pack_images(images: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """``[H_i, W_i, 3]`` tensors of ONE dtype (uint8 / uint16 / float32, any device) -> ``(flat, table)``: the 1-D tensor
    of that dtype with the images back to back, no padding between them, and the CPU int32 ``[N, 4]`` descriptor table
    ``{offset_lo, offset_hi, Hs, Ws}`` of ``hdrnet_prepare_batch_ragged`` -- the offset is the image's first SAMPLE (3
    per pixel), a 64-bit count split in two words, so one table serves an input and a target buffer of equal extents."""
    images = list(images)
    if not images:
        raise ValueError("pack_images: an empty list of images")
    rows, parts, off = [], [], 0
    for i, t in enumerate(images):
        if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[2] != 3 or t.shape[0] <= 0 or t.shape[1] <= 0:
            raise ValueError(f"pack_images: image {i} should be [H, W, 3], got "
                             f"{list(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        if t.dtype not in _DTYPE_CODE:
            raise TypeError(f"pack_images: image {i} must be float32, uint8 or uint16, got {t.dtype}")
        if t.dtype != images[0].dtype:
            raise ValueError(f"pack_images: mixed dtypes (image 0 is {images[0].dtype}, image {i} {t.dtype})")
        if t.shape[0] * t.shape[1] * 12 >= 2 ** 31:
            raise ValueError(f"pack_images: image {i} is too large")
        lo = off & 0xFFFFFFFF
        rows.append([lo - (1 << 32) if lo >= (1 << 31) else lo, off >> 32, t.shape[0], t.shape[1]])
        flat = t.contiguous().reshape(-1)
        parts.append(flat.view(torch.int16) if flat.dtype == torch.uint16 else flat)  # cat has no uint16 kernel
        off += flat.numel()
    flat = torch.cat(parts)
    if images[0].dtype == torch.uint16:
        flat = flat.view(torch.uint16)
    return flat, torch.tensor(rows, dtype=torch.int32)


def image_offsets(table: torch.Tensor) -> torch.Tensor:
    """The int64 sample offsets of a CPU descriptor table."""
    t = table.long()
    return (t[:, 1] << 32) | (t[:, 0] & 0xFFFFFFFF)


def check_images(table: torch.Tensor, n_samples: int, crop_hw: Sequence[int], even_turns_only: bool = False) -> None:
    """Raise ``ValueError`` unless a CPU descriptor table is int32 ``[N, 4]`` with non-negative offsets and positive
    extents, every image ends inside a buffer of ``n_samples`` samples and holds the crop (turned by 90 degrees too,
    unless ``even_turns_only``)."""
    if table.dim() != 2 or table.shape[1] != 4 or table.dtype != torch.int32 or table.shape[0] == 0:
        raise ValueError(f"images should be a non-empty int32 [N, 4] table, got {table.dtype} {list(table.shape)}")
    H, W = (int(v) for v in crop_hw)
    t = table.long()
    if (t[:, 1] < 0).any():
        raise ValueError("images: a negative offset")
    if (t[:, 2:] <= 0).any():
        raise ValueError("images: non-positive extents")
    bad = image_offsets(table) + t[:, 2] * t[:, 3] * 3 > int(n_samples)
    if bad.any():
        raise ValueError(f"images: image {int(bad.nonzero()[0])} ends outside the buffer of {int(n_samples)} samples")
    bad = (t[:, 2] < H) | (t[:, 3] < W)
    if bad.any():
        i = int(bad.nonzero()[0])
        raise ValueError(f"images: the crop {H} x {W} does not fit image {i} ({int(t[i, 2])} x {int(t[i, 3])})")
    bad = (t[:, 3] < H) | (t[:, 2] < W)
    if not even_turns_only and bad.any():
        i = int(bad.nonzero()[0])
        raise ValueError(f"images: the crop {H} x {W} does not fit image {i} turned by 90 degrees "
                         f"({int(t[i, 3])} x {int(t[i, 2])}); pass even_turns_only")


def _check_flat(name: str, t: torch.Tensor) -> None:
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() == 0:
        raise ValueError(f"{name} should be a non-empty 1-D buffer (pack_images), got "
                         f"{list(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
    if t.dtype not in _DTYPE_CODE:
        raise TypeError(f"{name} must be float32, uint8 or uint16, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: sample preparation runs on an MI355X (HIP) device only")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def prepare_batch_ragged(flat_input: torch.Tensor, flat_target: Optional[torch.Tensor], images: torch.Tensor,
                         ops: torch.Tensor, crop_hw: Sequence[int], net_input_size: int = 256,
                         input_white_level: Optional[float] = None, target_white_level: Optional[float] = None,
                         out: Optional[Sequence[Optional[torch.Tensor]]] = None, even_turns_only: bool = False):
    """``prepare_batch`` from a set of images of mixed extents: ``flat_input`` / ``flat_target`` are the 1-D buffers and
    ``images`` the int32 ``[N, 4]`` descriptor table of ``pack_images`` (one table for both: a pair has equal extents;
    the dtypes may differ).  One launch, ``(lowres_input, image_input, image_target)``; every crop offset is relative to
    its record's own image.

    ``images``: a CPU table is validated (``check_images``: offsets, extents, every image inside the buffer and holding
    the crop) and copied; a DEVICE table is used as it is.  ``ops`` is required and follows ``prepare_batch``'s rules: a
    CPU table is checked against each record's own source (a device ``images`` table is read back for that) and copied,
    a DEVICE table is read by the kernel and its records clamped there.  The kernel's memory safety depends on neither
    table.  The remaining arguments and ``out`` are ``prepare_batch``'s."""
    _check_flat("flat_input", flat_input)
    dev = flat_input.device
    n_samples = flat_input.numel()
    if flat_target is not None:
        _check_flat("flat_target", flat_target)
        if flat_target.numel() != n_samples or flat_target.device != dev:
            raise ValueError("flat_target should have flat_input's length and device")
    H, W = (int(v) for v in crop_hw)
    n = int(net_input_size)
    if not isinstance(images, torch.Tensor) or images.dim() != 2 or images.shape[1] != 4 or images.dtype != torch.int32:
        raise ValueError("images should be the int32 [N, 4] table of pack_images")
    if ops is None:
        raise ValueError("ops is required: there is no identity geometry over images of mixed extents")
    if ops.dim() != 2 or ops.shape[1] != 8 or ops.dtype != torch.int32:
        raise ValueError(f"ops should be int32 [batch, 8], got {ops.dtype} {list(ops.shape)}")
    N, B = images.shape[0], ops.shape[0]
    host_images = None
    if not images.is_cuda:
        check_images(images, n_samples, (H, W), even_turns_only)
        host_images = images
        images = images.to(dev, non_blocking=True)
    elif images.device != dev or not images.is_contiguous():
        raise ValueError("a device images table must be contiguous and on the sources' device")
    if not ops.is_cuda:
        if host_images is None:
            host_images = images.cpu()
        check_ops(ops, N, host_images[:, 2:], (H, W), even_turns_only)
        ops = ops.to(dev, non_blocking=True)
    elif ops.device != dev or not ops.is_contiguous():
        raise ValueError("a device ops table must be contiguous and on the sources' device")
    if input_white_level is None:
        input_white_level = _WHITE[flat_input.dtype]
    if target_white_level is None:
        target_white_level = _WHITE[flat_target.dtype] if flat_target is not None else 1.0
    res = _outputs(out, ((B, n, n, 3), (B, H, W, 3), (B, H, W, 3)), dev, flat_target is not None)
    ptr = [None if t is None else t.data_ptr() for t in res]
    with torch.cuda.device(dev):
        rc = _lib.load().hdrnet_prepare_batch_ragged(
            flat_input.data_ptr(), _DTYPE_CODE[flat_input.dtype], float(input_white_level),
            None if flat_target is None else flat_target.data_ptr(),
            0 if flat_target is None else _DTYPE_CODE[flat_target.dtype], float(target_white_level), n_samples,
            images.data_ptr(), N, ops.data_ptr(), B, ptr[1], ptr[2], H, W, ptr[0], n,
            _lib.SAMPLE_EVEN_TURNS_ONLY if even_turns_only else 0, _stream(dev))
    _lib.check(rc, "PrepareBatchRagged")
    return tuple(res)


class _Walk:
    """Which sources the next records take (``order=`` of the dataset classes): ``"random"`` leaves the draw to
    ``draw_ops`` (uniform, with replacement); ``"epoch"`` consumes a fresh permutation of ``range(N)`` from the
    generator per epoch, across batch boundaries, so that every image appears exactly once per ``N`` samples
    (``data_pipeline.py:190-200``); ``"sequential"`` walks ``0, 1, ...`` and wraps (``shuffle=False``)."""

    def __init__(self, order: str, n_sources: int, generator: Optional[torch.Generator]):
        if order not in ORDERS:
            raise ValueError(f"order should be one of {ORDERS}, got {order!r}")
        self.order, self.n, self.generator = order, int(n_sources), generator
        self._pending: list = []  # the rest of the current epoch
        self._next = 0

    def take(self, batch: int) -> Optional[list]:
        if self.order == "random":
            return None
        got: list = []
        while len(got) < batch:
            if self.order == "sequential":
                got.append(self._next)
                self._next = (self._next + 1) % self.n
                continue
            if not self._pending:
                self._pending = torch.randperm(self.n, generator=self.generator).tolist()
            k = batch - len(got)
            got += self._pending[:k]
            del self._pending[:k]
        return got


class DeviceDataset:
    """A set of image pairs held on the device in their wire format (u8: 6 bytes per pixel pair instead of the 24 of
    prepared fp32 samples) and expanded there: ``next_batch`` draws a table (``draw_ops``) and prepares the batch in one
    launch; ``feed(step)`` does so straight into a ``runtime.GraphedTrainStep``'s static buffers.

    ``inputs`` / ``targets``: ``[N, Hs, Ws, 3]`` uint8 / uint16 / float32 device tensors (``targets`` may be ``None``);
    ``output_resolution``: the crop ``(H, W)``; the augmentation switches are ``draw_ops``'s.  With ``rotate='even'`` or
    ``rotate=False`` the crop may exceed the source's transposed extents (the kernel then masks odd turns).  ``order``: how the source
    indices are chosen, ``"random"`` (uniform draws), ``"epoch"`` or ``"sequential"`` (see ``_Walk``).
    ``DeviceDataset.from_images`` holds a set of images of mixed extents instead."""

    def __init__(self, inputs: torch.Tensor, targets: Optional[torch.Tensor] = None,
                 input_white_level: Optional[float] = None, target_white_level: Optional[float] = None,
                 output_resolution: Optional[Sequence[int]] = None, net_input_size: int = 256, fliplr: bool = True,
                 flipud: bool = True, rotate=True, random_crop: bool = True,
                 generator: Optional[torch.Generator] = None, order: str = "random"):
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
        self._walk = _Walk(order, len(self), generator)

    @classmethod
    def from_images(cls, inputs: Sequence[torch.Tensor], targets: Optional[Sequence[torch.Tensor]] = None,
                    device=None, **kwargs) -> "RaggedDeviceDataset":
        """A ``RaggedDeviceDataset`` of the image pairs ``inputs[i]`` / ``targets[i]`` (``[H_i, W_i, 3]``, any sizes,
        one dtype per list), packed and moved to ``device``; the keywords are this class's."""
        return RaggedDeviceDataset(inputs, targets, device=device, **kwargs)

    def __len__(self) -> int:
        return self.inputs.shape[0]

    @property
    def order(self) -> str:
        return self._walk.order

    def draw(self, batch: int) -> torch.Tensor:
        return draw_ops(batch, len(self), self.source_hw, self.output_resolution, self.fliplr, self.flipud, self.rotate,
                        self.random_crop, self.generator, indices=self._walk.take(batch))

    def next_batch(self, batch: int, out: Optional[Sequence[Optional[torch.Tensor]]] = None, ops: Optional[torch.Tensor] = None):
        """Draw ``batch`` records (or take the CPU table ``ops``) and prepare them:
        ``(lowres_input, image_input, image_target)``, into ``out`` if given."""
        table = self.draw(batch) if ops is None else ops
        even = self._even_turns_only()
        check_ops(table, len(self), self.source_hw, self.output_resolution, even)
        dev_table = self._tables.get(batch)
        if dev_table is None:
            dev_table = self._tables[batch] = torch.zeros((batch, 8), dtype=torch.int32, device=self.inputs.device)
        dev_table.copy_(table, non_blocking=True)
        return prepare_batch(self.inputs, self.targets, dev_table, self.output_resolution, self.net_input_size,
                             self.input_white_level, self.target_white_level, out=out, even_turns_only=even)

    def _even_turns_only(self) -> bool:
        """May the device mask odd turns?  With ``rotate='even'``; and with ``rotate=False`` where the crop does not fit
        the source turned by 90 degrees (no turn is drawn, and the kernel refuses such a crop otherwise: the evaluation
        pipeline's 1080 x 1920 frames).  A crop that fits both ways keeps the full check of a caller's own table."""
        mode = _rotate_mode(self.rotate)
        (Hs, Ws), (H, W) = self.source_hw, self.output_resolution
        return mode == "even" or (mode == "none" and (H > Ws or W > Hs))

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


class RaggedDeviceDataset:
    """``DeviceDataset`` for image pairs of mixed extents (``DeviceDataset.from_images``): the pairs are packed back to
    back into one flat wire-format buffer per side (``pack_images``) and every crop is drawn from its own image's
    extents, as the reference's file pipelines do.  ``__len__``, ``draw``, ``next_batch`` and ``feed`` are the uniform
    class's.  Read-only: ``sizes`` (CPU int64 ``[N, 2]``), ``images`` (the device descriptor table), ``flat_inputs`` /
    ``flat_targets`` (the device buffers).  A pair must have equal extents; its dtypes may differ."""

    def __init__(self, inputs: Sequence[torch.Tensor], targets: Optional[Sequence[torch.Tensor]] = None, device=None,
                 input_white_level: Optional[float] = None, target_white_level: Optional[float] = None,
                 output_resolution: Optional[Sequence[int]] = None, net_input_size: int = 256, fliplr: bool = True,
                 flipud: bool = True, rotate=True, random_crop: bool = True,
                 generator: Optional[torch.Generator] = None, order: str = "random"):
        inputs = list(inputs)
        flat_in, table = pack_images(inputs)
        flat_tg = None
        if targets is not None:
            targets = list(targets)
            if len(targets) != len(inputs):
                raise ValueError(f"{len(inputs)} inputs and {len(targets)} targets")
            for i, (a, b) in enumerate(zip(inputs, targets)):
                if not isinstance(b, torch.Tensor) or tuple(a.shape) != tuple(b.shape):
                    raise ValueError(f"pair {i}: the target should have the input's extents {list(a.shape)}")
            flat_tg, _ = pack_images(targets)
        if output_resolution is None:
            raise ValueError("output_resolution (the crop) is required for a set of mixed extents")
        if device is None:
            device = flat_in.device if flat_in.is_cuda else torch.device("cuda")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"device is {device}: sample preparation runs on an MI355X (HIP) device only")
        self._sizes = table[:, 2:].long().contiguous()
        self.output_resolution = tuple(int(v) for v in output_resolution)
        self.net_input_size = int(net_input_size)
        self.input_white_level, self.target_white_level = input_white_level, target_white_level
        self.fliplr, self.flipud, self.rotate, self.random_crop = fliplr, flipud, rotate, random_crop
        self.generator = generator
        draw_ops(0, len(self), self._sizes, self.output_resolution, rotate=rotate)  # does every image hold the crop?
        check_images(table, flat_in.numel(), self.output_resolution, _rotate_mode(rotate) != "all")
        self._walk = _Walk(order, len(self), generator)
        self._flat_inputs = flat_in.to(device)
        self._flat_targets = None if flat_tg is None else flat_tg.to(device)
        self._images = table.to(device)
        self._tables: dict = {}

    sizes = property(lambda self: self._sizes)
    images = property(lambda self: self._images)
    flat_inputs = property(lambda self: self._flat_inputs)
    flat_targets = property(lambda self: self._flat_targets)
    order = property(lambda self: self._walk.order)

    def __len__(self) -> int:
        return self._sizes.shape[0]

    def draw(self, batch: int) -> torch.Tensor:
        return draw_ops(batch, len(self), self._sizes, self.output_resolution, self.fliplr, self.flipud, self.rotate,
                        self.random_crop, self.generator, indices=self._walk.take(batch))

    def next_batch(self, batch: int, out: Optional[Sequence[Optional[torch.Tensor]]] = None, ops: Optional[torch.Tensor] = None):
        """Draw ``batch`` records (or take the CPU table ``ops``) and prepare them:
        ``(lowres_input, image_input, image_target)``, into ``out`` if given."""
        table = self.draw(batch) if ops is None else ops
        even = _rotate_mode(self.rotate) != "all"  # no odd turn is drawn: the device may mask them
        check_ops(table, len(self), self._sizes, self.output_resolution, even)
        dev_table = self._tables.get(batch)
        if dev_table is None:
            dev_table = self._tables[batch] = torch.zeros((batch, 8), dtype=torch.int32, device=self._images.device)
        dev_table.copy_(table, non_blocking=True)
        return prepare_batch_ragged(self._flat_inputs, self._flat_targets, self._images, dev_table,
                                    self.output_resolution, self.net_input_size, self.input_white_level,
                                    self.target_white_level, out=out, even_turns_only=even)

    def feed(self, step, ops: Optional[torch.Tensor] = None):
        """``DeviceDataset.feed``: the next batch INTO ``step``'s static buffers; returns ``(inputs, targets)``."""
        if self._flat_targets is None:
            raise ValueError("feed() needs a dataset with targets")
        low, full = step.static_inputs
        (target,) = step.static_targets
        self.next_batch(full.shape[0], out=(low, full, target), ops=ops)
        return [low, full], [target]
