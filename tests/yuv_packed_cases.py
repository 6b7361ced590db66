"""Packed YUV 4:2:2 surfaces (include/hdrnet_amd_yuv_packed.h), stated once in numpy for tests/test_yuv_packed_host.py and
tests/test_gpu_yuv_packed.py: the weave of an NV16 / P210 / P216 plane pair into one plane and its inverse, for the three
byte orders and the two sample widths; random surfaces through yuv_chroma_cases.random_planar(..., "422"), so that every
chroma sample is its own draw; layouts through yuv_chroma_cases.plane_layout.  A packed surface holds exactly the samples of
the semi-planar 4:2:2 surface, so the existing 4:2:2 path on the unwoven pair is the oracle for every output, bit for bit.
No GPU, no package import."""
import numpy as np

import yuv_chroma_cases as cc
import yuv_planar_cases as pc

# format -> (byte order code, significant bits, numpy dtype)
FORMATS = {"yuy2": (0, 8, np.uint8), "uyvy": (1, 8, np.uint8), "yvyu": (2, 8, np.uint8),
           "y210": (0, 10, np.uint16), "y216": (0, 16, np.uint16)}
# position of (Y0, U, Y1, V) within a group of four samples, per byte order code
POSITIONS = {0: (0, 1, 2, 3), 1: (1, 0, 3, 2), 2: (0, 3, 2, 1)}
LAYOUTS = cc.LAYOUTS
FILLS = cc.FILLS
GUARD_BYTES = cc.GUARD_BYTES


def order_of(fmt):
    return FORMATS[fmt][0]


def bits_of(fmt):
    return FORMATS[fmt][1]


def dtype_of(fmt):
    return FORMATS[fmt][2]


def weave(y, uv, order):
    """The semi-planar 4:2:2 pair ``y`` ``[B, H, W]``, ``uv`` ``[B, H, W]`` (interleaved U, V) -> the packed surface
    ``[B, H, 2 W]`` in byte order ``order``.  Samples travel as they are (a uint16 code stays in the high bits)."""
    assert y.shape == uv.shape and y.dtype == uv.dtype and y.shape[2] % 2 == 0
    B, H, W = y.shape
    py0, pu, py1, pv = POSITIONS[order]
    out = np.empty((B, H, 2 * W), y.dtype)
    out[:, :, py0::4] = y[:, :, 0::2]
    out[:, :, py1::4] = y[:, :, 1::2]
    out[:, :, pu::4] = uv[:, :, 0::2]
    out[:, :, pv::4] = uv[:, :, 1::2]
    return out


def unweave(surface, order):
    """The inverse: ``(y, uv)`` of the packed surface ``[B, H, 2 W]``."""
    B, H, W2 = surface.shape
    assert W2 % 4 == 0
    py0, pu, py1, pv = POSITIONS[order]
    y = np.empty((B, H, W2 // 2), surface.dtype)
    uv = np.empty((B, H, W2 // 2), surface.dtype)
    y[:, :, 0::2] = surface[:, :, py0::4]
    y[:, :, 1::2] = surface[:, :, py1::4]
    uv[:, :, 0::2] = surface[:, :, pu::4]
    uv[:, :, 1::2] = surface[:, :, pv::4]
    return y, uv


def random_codes(rng, shape, bits, corners=True):
    """``(y, u, v)`` codes of ``bits`` bits in the low bits: yuv_chroma_cases.random_planar for 4:2:2."""
    return cc.random_planar(rng, shape, bits, "422", corners=corners)


def semi(codes, bits):
    """The NV16 / P210 / P216 pair ``(y, uv)`` of the codes as that container stores them (uint16: the high bits)."""
    return cc.semi(*codes, bits)


def packed(codes, fmt):
    """The packed surface of the codes in format ``fmt``."""
    return weave(*semi(codes, bits_of(fmt)), order_of(fmt))


def surface_layout(shape, size, layout):
    """Where a packed surface of ``shape = (B, H, W)`` PIXELS lies (yuv_chroma_cases.plane_layout on its one plane of
    ``2 W`` samples): ``(buffer lengths, spec)``."""
    B, H, W = shape
    lengths, specs = cc.plane_layout([(B, H, 2 * W)], size, layout)
    return lengths, specs[0]


def lay(surface, layout, fill=pc.POISON):
    """The surface's samples in ``layout``, everything around them filled with ``fill`` bytes: ``(flat buffers, spec)``."""
    bufs, specs = cc.lay((surface,), layout, fill)
    return bufs, specs[0]
