"""Planar YUV 4:2:0 surfaces (include/hdrnet_amd_yuv_planar.h), stated once in numpy for the tests: the same samples as a
semi-planar surface of tests/yuv_cases.py with the chroma split into two planes -- and, for 10-bit, the codes in the LOW
bits -- so that every planar path has the pinned semi-planar one as its yardstick.  Layouts: tight planes, pitched planes,
three planes in one allocation.  No GPU, no package import."""
import numpy as np

import yuv_cases as yc

POISON = yc.POISON
GUARD_BYTES = 4096    # behind every buffer
FILLS = (0xA5, 0x5A)  # byte fills of outputs: a sample never written cannot equal the expected one under both
LAYOUTS = ("tight", "pitch64", "one_allocation")


def interleave(u, v):
    """U, V ``[B, H / 2, W / 2]`` -> the interleaved UV plane ``[B, H / 2, W]`` of a semi-planar surface."""
    assert u.shape == v.shape and u.dtype == v.dtype
    uv = np.empty(u.shape[:2] + (2 * u.shape[2],), u.dtype)
    uv[:, :, 0::2] = u
    uv[:, :, 1::2] = v
    return uv


def split(uv):
    """The interleaved UV plane ``[B, H / 2, W]`` -> contiguous U, V ``[B, H / 2, W / 2]``."""
    return np.ascontiguousarray(uv[:, :, 0::2]), np.ascontiguousarray(uv[:, :, 1::2])


def random_planar(rng, shape, bits):
    """A planar surface with the samples of ``yuv_cases.random_surface`` (the whole code range, the image corners pinned to
    the extreme codes), the codes in the LOW bits: ``(y, u, v)`` tight, and ``(y_semi, uv_semi)``, the semi-planar surface
    of the same codes as its own rules store them (P010: ``code << 6``)."""
    y_semi, uv_semi = yc.random_surface(rng, shape, bits)
    sh = yc.stored_shift(bits)
    u, v = split(uv_semi >> sh)
    return (y_semi >> sh, u, v), (y_semi, uv_semi)


def fill_value(dtype, fill):
    """The sample whose bytes are all ``fill``."""
    return np.dtype(dtype).type(fill * (0x101 if np.dtype(dtype).itemsize == 2 else 1))


def planar_layout(shape, size, layout):
    """Where the three planes of a ``shape = (B, H, W)`` surface of ``size``-byte samples lie: ``(buffer lengths, y, u, v)``
    with each plane = ``(buffer index, offset, shape, strides)``, everything in SAMPLES.  Each buffer ends in GUARD_BYTES
    of guard.  "pitch64": every row 64 bytes wider than its samples.  "one_allocation": Y, then U, then V per image, as
    FFmpeg lays out a frame (linesize = row + 64 bytes; both chroma image strides equal the luma's)."""
    B, H, W = shape
    assert H % 2 == 0 and W % 4 == 0
    guard = GUARD_BYTES // size
    hc, wc = H // 2, W // 2
    if layout == "tight":
        return ([B * H * W + guard, B * hc * wc + guard, B * hc * wc + guard],
                (0, 0, (B, H, W), (H * W, W, 1)), (1, 0, (B, hc, wc), (hc * wc, wc, 1)), (2, 0, (B, hc, wc), (hc * wc, wc, 1)))
    py, pc = W + 64 // size, wc + 64 // size
    if layout == "pitch64":
        return ([B * H * py + guard, B * hc * pc + guard, B * hc * pc + guard],
                (0, 0, (B, H, W), (H * py, py, 1)), (1, 0, (B, hc, wc), (hc * pc, pc, 1)), (2, 0, (B, hc, wc), (hc * pc, pc, 1)))
    assert layout == "one_allocation", layout
    image = H * py + 2 * hc * pc  # (a multiple of 4 bytes: py and pc are)
    return ([B * image + guard],
            (0, 0, (B, H, W), (image, py, 1)), (0, H * py, (B, hc, wc), (image, pc, 1)),
            (0, H * py + hc * pc, (B, hc, wc), (image, pc, 1)))


def plane(bufs, spec):
    """The numpy view of a plane in its flat buffer."""
    i, off, shape, strides = spec
    flat = bufs[i]
    return np.lib.stride_tricks.as_strided(flat[off:], shape, tuple(s * flat.itemsize for s in strides))


def lay_planar(y, u, v, layout, fill=POISON):
    """The surface's samples in ``layout``, everything around them (padding, guards) filled with ``fill`` bytes:
    ``(flat buffers, (y spec, u spec, v spec))``."""
    lengths, *specs = planar_layout(y.shape, y.itemsize, layout)
    bufs = [np.full(n, fill_value(y.dtype, fill), y.dtype) for n in lengths]
    for spec, t in zip(specs, (y, u, v)):
        plane(bufs, spec)[...] = t
    return bufs, tuple(specs)


def outside_planes(bufs, specs):
    """Per buffer, the boolean mask of the samples that belong to no plane."""
    masks = [np.ones(b.shape, bool) for b in bufs]
    for spec in specs:
        plane(masks, spec)[...] = False
    return masks
