"""The pixel-format rules of include/hdrnet_amd_pixel_formats.h, stated once in numpy for
tests/test_pixel_formats_host.py and tests/test_gpu_pixel_formats.py.

A frame is ``[..., 3]`` (``rgb``, ``bgr``) or ``[..., 4]`` (``rgba``, ``bgra``: alpha last).  The model sees R, G, B.
A uint8 output has the input's format with the input's alpha -- the byte of a uint8 frame, ``alpha >> 8`` of a uint16
one: alpha is not an image sample, it is never divided by the white level and never quantised.  A float32 output is RGB
and has no alpha."""
import numpy as np

FORMATS = ("rgb", "bgr", "rgba", "bgra")
CODE = {"rgb": 0, "bgr": 1, "rgba": 2, "bgra": 3}
CHANNELS = {"rgb": 3, "bgr": 3, "rgba": 4, "bgra": 4}
B_FIRST = {"rgb": False, "bgr": True, "rgba": False, "bgra": True}


def to_rgb(frame, fmt):
    """The ``[..., 3]`` RGB frame the model sees (contiguous copy)."""
    frame = np.asarray(frame)
    assert frame.shape[-1] == CHANNELS[fmt], (frame.shape, fmt)
    colour = frame[..., :3]
    return np.ascontiguousarray(colour[..., ::-1] if B_FIRST[fmt] else colour)


def alpha_of(frame, fmt):
    """The frame's alpha plane as stored, or None for a 3-channel format."""
    return np.ascontiguousarray(np.asarray(frame)[..., 3]) if CHANNELS[fmt] == 4 else None


def alpha_u8(alpha):
    """Alpha as it appears in a uint8 output: copied from a uint8 frame, ``>> 8`` from a uint16 one."""
    alpha = np.asarray(alpha)
    if alpha.dtype == np.uint8:
        return alpha
    assert alpha.dtype == np.uint16, alpha.dtype
    return (alpha >> 8).astype(np.uint8)


def from_rgb(out_rgb, fmt, alpha):
    """What the op returns for a frame in ``fmt`` given what it returns for the RGB frame: a uint8 output in the input's
    format with ``alpha`` (the INPUT's alpha plane) in place, a float32 output as it is (RGB, no alpha)."""
    out_rgb = np.asarray(out_rgb)
    if out_rgb.dtype != np.uint8:
        return out_rgb
    colour = out_rgb[..., ::-1] if B_FIRST[fmt] else out_rgb
    if CHANNELS[fmt] == 3:
        return np.ascontiguousarray(colour)
    return np.concatenate([colour, alpha_u8(alpha)[..., None]], axis=-1)


def random_frame(rng, shape_bhw, fmt, dtype, white_level):
    """Random samples in [0, white_level] and, with alpha, random alpha over the dtype's whole range."""
    hi = 256 if dtype == "uint8" else int(white_level) + 1
    frame = rng.integers(0, hi, tuple(shape_bhw) + (CHANNELS[fmt],)).astype(dtype)
    if CHANNELS[fmt] == 4:
        frame[..., 3] = rng.integers(0, 256 if dtype == "uint8" else 65536, tuple(shape_bhw)).astype(dtype)
    return frame
