"""YUV 4:2:2 and 4:4:4 surfaces (include/hdrnet_amd_yuv_chroma.h), stated once in numpy for tests/test_yuv_chroma_host.py and
tests/test_gpu_yuv_chroma.py: plane shapes per chroma layout, random surfaces with INDEPENDENT chroma in every row (4:2:2)
and every pixel (4:4:4), the float64 evaluation of the conversion, the float64 encoder of the header's rule generalised from
the 2 x 2 block (yuv_cases.encode_nv12_64 / u16_out_cases.encode_p016_64) to the chroma sample's footprint, the replication
of a 4:2:0 surface into the other layouts, and the layouts of tests/yuv_planar_cases.py for the new plane shapes.  Codes
are in the LOW bits throughout (planar surfaces as stored; a semi-planar uint16 surface stores ``code << (16 - bits)``).
No GPU, no package import."""
import numpy as np

import u16_out_cases as uc
import yuv_planar_cases as pc

CHROMAS = ("422", "444")
FOOTPRINT = {"420": (2, 2), "422": (1, 2), "444": (1, 1)}  # image rows, columns served by one chroma sample
LAYOUTS = pc.LAYOUTS
FILLS = pc.FILLS
GUARD_BYTES = pc.GUARD_BYTES


def chroma_shape(shape, chroma):
    B, H, W = shape
    fy, fx = FOOTPRINT[chroma]
    assert H % fy == 0 and W % 4 == 0
    return (B, H // fy, W // fx)


def replicate(plane, chroma):
    """A chroma plane -> ``[B, H, W]``: each sample over its footprint."""
    fy, fx = FOOTPRINT[chroma]
    return plane.repeat(fy, axis=1).repeat(fx, axis=2)


def random_planar(rng, shape, bits, chroma, corners=True):
    """``(y, u, v)`` with codes of ``bits`` bits in the low bits, drawn over the WHOLE code range, every chroma sample its
    own draw -- so a kernel that reads chroma row ``y >> 1`` or sample ``x >> 1`` of a 4:4:4 plane cannot pass -- and, with
    ``corners``, yuv_cases.random_surface's pinned corners: black and white luma over neutral chroma in the first row,
    extreme chroma under the other two."""
    B, H, W = shape
    dt = np.uint8 if bits == 8 else np.uint16
    top = 2 ** bits
    cs = chroma_shape(shape, chroma)
    y = rng.integers(0, top, shape).astype(dt)
    u = rng.integers(0, top, cs).astype(dt)
    v = rng.integers(0, top, cs).astype(dt)
    if corners:
        lo, hi, mid = dt(0), dt(top - 1), dt(top // 2)
        y[:, 0, 0], y[:, 0, W - 1], y[:, H - 1, 0], y[:, H - 1, W - 1] = lo, hi, hi, lo
        for p in (u, v):
            p[:, 0, 0] = p[:, 0, -1] = mid
        u[:, -1, 0], v[:, -1, 0], u[:, -1, -1], v[:, -1, -1] = lo, hi, hi, lo
    return y, u, v


def from_420(y, u, v, chroma):
    """The 4:2:2 / 4:4:4 surface that REPLICATES a 4:2:0 one: each chroma row stored twice (and, for 4:4:4, each sample
    twice along the row).  Through every path it must give the bits of the 4:2:0 path on the original."""
    fx = 2 if chroma == "444" else 1
    return y, u.repeat(2, axis=1).repeat(fx, axis=2), v.repeat(2, axis=1).repeat(fx, axis=2)


def to_rgb64(y, u, v, chroma, to_rgb):
    """float64 evaluation of the conversion on the float32 constants as given: ``[B, H, W, 3]`` in [0, 1]."""
    k = np.asarray(to_rgb, np.float64)
    Y, U, V = y.astype(np.float64), replicate(u, chroma).astype(np.float64), replicate(v, chroma).astype(np.float64)
    out = np.stack([k[3 * i] * Y + k[3 * i + 1] * U + k[3 * i + 2] * V + k[9 + i] for i in range(3)], axis=-1)
    return np.clip(out, 0.0, 1.0)


def encode64(rgb, from_rgb, bits, chroma):
    """float64 encoder of the header's rule on ``rgb`` ``[B, H, W, 3]``: clip to [0, 1], Y per pixel, U and V from the mean
    over the chroma sample's footprint, + bias (the + 0.5 is in it), clamp to [0, 2^bits - 1], truncate.  Returns
    ``((y, u, v) codes in the low bits, (y, u, v) float64 values before the clamp and the truncation)``.  With
    ``chroma="420"`` it is encode_nv12_64 / encode_p016_64 with the UV plane split."""
    k = np.asarray(from_rgb, np.float64)
    c = np.clip(np.asarray(rgb, np.float64), 0.0, 1.0)
    B, H, W, _ = c.shape
    fy, fx = FOOTPRINT[chroma]
    mean = c.reshape(B, H // fy, fy, W // fx, fx, 3).mean(axis=(2, 4))
    pre = (c @ k[0:3] + k[9], mean @ k[3:6] + k[10], mean @ k[6:9] + k[11])
    dt = np.uint8 if bits == 8 else np.uint16
    return tuple(np.floor(np.clip(t, 0.0, uc.code_max(bits))).astype(dt) for t in pre), pre


def decided(pre, bits):
    """u16_out_cases.decided (eps_of(8) is yuv_cases.decided's 1e-3): the code is the same for every value within eps."""
    return uc.decided(pre, bits)


def semi(y, u, v, bits):
    """The semi-planar 4:2:2 surface of the same codes as its own rules store them: U, V interleaved ``[B, H, W]``, a
    uint16 code in the HIGH bits (P210: ``code << 6``)."""
    sh = 0 if bits == 8 else 16 - bits
    return (y << sh).astype(y.dtype), (pc.interleave(u, v) << sh).astype(y.dtype)


# ---- layouts: tests/yuv_planar_cases.py's, for chroma planes of any shape ---------------------------------------------------
def plane_layout(shapes, size, layout):
    """Where planes of ``shapes`` (each ``(B, rows, cols)``, one B) lie: ``(buffer lengths, spec per plane)`` with spec =
    ``(buffer index, offset, shape, strides)`` in SAMPLES, as yuv_planar_cases.planar_layout: "tight", "pitch64" (every row
    64 bytes wider than its samples), "one_allocation" (all planes of an image back to back, pitched, one image stride).
    Each buffer ends in GUARD_BYTES of guard."""
    guard = GUARD_BYTES // size
    B = shapes[0][0]
    if layout == "tight":
        return [B * r * c + guard for _, r, c in shapes], [(i, 0, s, (s[1] * s[2], s[2], 1)) for i, s in enumerate(shapes)]
    pitch = [c + 64 // size for _, _, c in shapes]
    if layout == "pitch64":
        return ([B * r * p + guard for (_, r, _), p in zip(shapes, pitch)],
                [(i, 0, s, (s[1] * p, p, 1)) for i, (s, p) in enumerate(zip(shapes, pitch))])
    assert layout == "one_allocation", layout
    image = sum(r * p for (_, r, _), p in zip(shapes, pitch))
    assert image * size % 4 == 0
    specs, off = [], 0
    for s, p in zip(shapes, pitch):
        specs.append((0, off, s, (image, p, 1)))
        off += s[1] * p
    return [B * image + guard], specs


def lay(planes, layout, fill=pc.POISON):
    """The planes' samples in ``layout``, everything around them filled with ``fill`` bytes: ``(flat buffers, specs)``."""
    dt = planes[0].dtype
    lengths, specs = plane_layout([p.shape for p in planes], dt.itemsize, layout)
    bufs = [np.full(n, pc.fill_value(dt, fill), dt) for n in lengths]
    for spec, t in zip(specs, planes):
        pc.plane(bufs, spec)[...] = t
    return bufs, tuple(specs)
