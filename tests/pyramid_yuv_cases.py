"""Inputs and references of the pyramid model on YUV 4:2:0 surfaces (include/hdrnet_amd_pyramid_yuv.h), stated once in numpy
for tests/test_pyramid_yuv_host.py (the caps, from the reference alone) and tests/test_gpu_pyramid_yuv.py.  Every reference
is computed once per process and shared; callers do not modify what they get.

One case = (shape, surface kind, guide kind).  The surface is yuv_chroma_cases.random_planar(..., "420") -- the whole code
range, pinned corners -- held BOTH as the planar surface (codes in the low bits) and as the semi-planar surface of the same
codes (yuv_planar_cases.interleave; P010: code << 6), so that a planar kind and its semi-planar twin share every reference.
Grid and coarse level are pyramid_io_cases.inputs': a near-identity affine and a coarse level ~ 0.3 N(0, 1), so that the sum
leaves [0, 1] on both sides and the clip AFTER the up-add decides the quantised outputs."""
import functools

import numpy as np

import pyramid_io_cases as pio
import u16_out_cases as uc
import yuv_cases as yc
import yuv_chroma_cases as ycc
import yuv_planar_cases as ypc

GH, GW, GD = pio.GH, pio.GW, pio.GD
TOL = pio.TOL
# (B, H, W, Hc, Wc): two segments on 192 threads, idle lanes, a second image, three row pairs; one segment, a partly filled
# wave; a one-column coarse level
SHAPES = [(2, 6, 1040, 3, 520), (1, 4, 96, 2, 48), (1, 4, 1024, 2, 1)]
PADS = (0, 64)  # bytes per row beyond the samples
FILLS = ypc.FILLS
GUARD_BYTES = ypc.GUARD_BYTES

# kind -> (bits, standard, full range, planar, kernel label of the input, the surface output: (out=, label, bits))
KINDS = {
    "nv12": (8, "bt709", False, False, "nv12", ("nv12", "nv12", 8)),
    "p016": (16, "bt601", True, False, "p016", ("nv12", "nv12", 8)),    # a uint16 surface in, NV12 out
    "p010": (10, "bt709", False, False, "p016", ("p010", "p016", 10)),  # codes in the high bits, in and out
    "i420": (8, "bt709", False, True, "i420", ("planar", "i420", 8)),
    "i010": (10, "bt709", False, True, "i016", ("planar", "i016", 10)),  # yuv420p10le: codes in the low bits
}
TWIN = {"i420": "nv12", "i010": "p010"}  # the semi-planar kind of the same codes, standard and range


def bits_of(kind):
    return KINDS[kind][0]


def constants(kind):
    """(to_rgb, from_rgb of the kind's surface output): 12 float32 numbers each (hdrnet_amd/yuv.py)."""
    from hdrnet_amd import yuv
    bits, standard, full, planar, _, (_, _, out_bits) = KINDS[kind]
    to_rgb = yuv.yuv_coefficients(standard, full, bits, msb_aligned=not planar)[0]
    return to_rgb, yuv.yuv_encode_coefficients(standard, full, out_bits)


def surface(rng, shape, bits):
    """``((y, u, v) planar, codes in the low bits; (y, uv) semi-planar as stored)`` of one random content."""
    y, u, v = ycc.random_planar(rng, shape, bits, "420")
    sh = yc.stored_shift(bits)
    return (y, u, v), ((y << sh).astype(y.dtype), (ypc.interleave(u, v) << sh).astype(y.dtype))


@functools.lru_cache(maxsize=None)
def inputs(shape, kind, nn):
    """dict: grid, coarse, conv1, conv2, guide, planar = (y, u, v), semi = (y, uv), inp_f (the float32 frame the conversion
    gives, from float64).  A planar kind returns its twin's arrays."""
    import oracle
    kind = TWIN.get(kind, kind)
    B, H, W, Hc, Wc = shape
    bits = bits_of(kind)
    rng = np.random.default_rng([2000, SHAPES.index(shape), bits, int(nn)])
    grid6 = np.zeros((B, GH, GW, GD, 3, 4), np.float32)
    for i in range(3):
        grid6[..., i, i] = 1.0
    grid = (grid6 + 0.15 * rng.standard_normal(grid6.shape)).astype(np.float32).reshape(B, GH, GW, GD, 12)
    planar, semi = surface(rng, (B, H, W), bits)
    inp_f = yc.to_rgb64(semi[0], semi[1], constants(kind)[0]).astype(np.float32)
    coarse = (0.3 * rng.standard_normal((B, Hc, Wc, 3))).astype(np.float32)
    conv1 = (rng.standard_normal((16, 4)) * 0.8).astype(np.float32)
    conv2 = (rng.standard_normal(17) * 0.5).astype(np.float32)
    guide = oracle.pointwise_nn_guide(inp_f, conv1, conv2) if nn else rng.random((B, H, W)).astype(np.float32)
    c = dict(grid=grid, coarse=coarse, conv1=conv1, conv2=conv2, guide=guide, planar=planar, semi=semi, inp_f=inp_f)
    for a in (grid, coarse, conv1, conv2, guide, inp_f, *planar, *semi):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def want_f32(shape, kind, nn):
    """The composed CPU oracle: port.bilateral_slice_apply on the converted float32 frame with the case's guide map, +
    oracle.resize_bilinear_align_corners(coarse), added in float32."""
    import oracle
    kind = TWIN.get(kind, kind)
    c = inputs(shape, kind, nn)
    B, H, W, _, _ = shape
    out = oracle.port().bilateral_slice_apply(c["grid"], c["guide"], c["inp_f"], True)
    out = (out + oracle.resize_bilinear_align_corners(c["coarse"], H, W)).astype(np.float32)
    out.setflags(write=False)
    return out


def encode(rgb, kind):
    """The float64 encoder of the kind's surface output on ``rgb``: ``((y, u, v) codes in the low bits, pre-truncation
    values, decided masks, bits)`` (yuv_chroma_cases.encode64 with the 2 x 2 footprint; u16_out_cases.decided)."""
    bits = KINDS[kind][5][2]
    codes, pre = ycc.encode64(rgb, constants(kind)[1], bits, "420")
    return codes, pre, tuple(uc.decided(p, bits) for p in pre), bits


def stored_planes(kind, planes):
    """The planes a surface output returned, as numpy, -> ``(y, u, v)`` codes in the low bits."""
    bits = KINDS[kind][5][2]
    if KINDS[kind][3]:
        return tuple(planes)
    sh = yc.stored_shift(bits)
    y, uv = planes
    assert not (y & ((1 << sh) - 1)).any() and not (uv & ((1 << sh) - 1)).any(), "bits below the code are set"
    u, v = ypc.split(uv >> sh)
    return y >> sh, u, v


def pitched(plane, pad_bytes, fill=yc.POISON):
    """``plane`` ``[B, rows, cols]`` inside rows ``pad_bytes`` wider, the padding filled with ``fill`` bytes: the buffer
    ``[B, rows, cols + pad]``; the plane is ``buffer[:, :, :cols]``."""
    size = plane.itemsize
    assert pad_bytes % size == 0
    buf = np.full(plane.shape[:2] + (plane.shape[2] + pad_bytes // size,), ypc.fill_value(plane.dtype, fill), plane.dtype)
    buf[:, :, :plane.shape[2]] = plane
    return buf


def picture(rng, shape, bits):
    """A surface that is a picture -- smooth ramps + noise in luma, gentle ramps around neutral in chroma, inside the
    limited range -- so that the low-res input and the guide see an image rather than white noise.  ``((y, u, v) codes in
    the low bits, (y, uv) semi-planar as stored)``."""
    B, H, W = shape
    dt = np.uint8 if bits == 8 else np.uint16
    unit = 2 ** (bits - 8)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    luma = 0.15 + 0.7 * (0.6 * xx / W + 0.4 * yy / H)[None] * (0.7 + 0.3 * rng.random((B, 1, 1)))
    y = np.clip(np.round((16 + 219 * np.clip(luma + 0.05 * rng.standard_normal((B, H, W)), 0, 1)) * unit), 0, 2 ** bits - 1)
    cy, cx = np.mgrid[0:H // 2, 0:W // 2].astype(np.float64)
    u = np.round((128 + 40 * (cx / (W // 2) - 0.5)[None] + 4 * rng.standard_normal((B, H // 2, W // 2))) * unit)
    v = np.round((128 + 40 * (0.5 - cy / (H // 2))[None] + 4 * rng.standard_normal((B, H // 2, W // 2))) * unit)
    y, u, v = (np.clip(p, 0, 2 ** bits - 1).astype(dt) for p in (y, u, v))
    sh = yc.stored_shift(bits)
    return (y, u, v), ((y << sh).astype(dt), (ypc.interleave(u, v) << sh).astype(dt))
