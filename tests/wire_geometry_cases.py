"""The geometries, memory layouts and contents of tests/test_gpu_wire_geometry.py, stated once in numpy: that file runs the
packed (BGR / RGBA / BGRA), YUV-surface and 16-bit-output forwards of csrc/apply_fwd_io.hip.h at them, and
tests/test_wire_geometry_host.py holds this table to what its comments say.  No GPU, no package import.

Each geometry isolates one regime that tests/test_gpu_pixel_formats.py, test_gpu_yuv.py and test_gpu_u16_out.py -- two
shapes, (2, 6, 1040) and (1, 4 | 5, 96), on one grid, 16 x 16 x 8 -- do not reach.  Every frame is under 100 k pixels; H is
even and W % 4 == 0 everywhere, so every family is legal at every geometry (no pair is left out)."""
import numpy as np

import pixel_format_cases as px
import yuv_cases as yc

# id -> ((B, H, W), (GH, GW, GD)).  gy = (y + 0.5) * GH / H - 0.5 in float32 (seg_common.hip.h); the clamp is reached where
# gy < 0 or gy > GH - 1.
GEOMETRIES = {
    # 3 segments of 684 px: the narrowest row with an INTERIOR segment (cmin > 0, full width, a right neighbour).
    # scale_y = 0.4: row 0 (gy = -0.3) and row 39 (gy = 15.3) clamp; of the 20 chroma pairs some lie inside one grid row
    # (rows 2, 3: gy 0.5, 0.9; rows 4, 5: 1.3, 1.7), some straddle a boundary (rows 8, 9: gy 2.9, 3.3) -- the surface
    # stores restage the LDS image between the two rows of a pair, so the straddling pair is their own code path.
    "interior": ((1, 40, 2052), (16, 16, 8)),
    # 5 segments of 768 px, the row of a 4K frame, with the host's column table.  16 planes, GH != GW, a second image,
    # both vertical clamps (rows 0 and 11: gy = -0.17, 7.17 > 7).
    "uhd_row": ((2, 12, 3840), (8, 32, 16)),
    # 11 segments of 748 px: more than the host table's 8, so the column windows are computed on the device.  Odd grid
    # extents, GH < H (rows 0 and 3 clamp: gy = -0.125, 2.125 > 2).
    "many_seg": ((1, 4, 8196), (3, 5, 7)),
    # One cell: every tap clamped in x, y and z; GD = 1 (zhi = 0).  65 of 128 lanes active.  Three images.
    "one_cell": ((3, 6, 260), (1, 1, 1)),
    # 33 row pairs of one short segment; 4 planes; a 32 x 32 grid (gy runs from -0.26 to 31.26: rows 0 and 65 clamp).
    "tall": ((1, 66, 96), (32, 32, 4)),
}
GEOMETRY_IDS = list(GEOMETRIES)

# A geometry no wire-format kernel takes (io_fits is false: 42 planes of 35 columns exceed 64 KiB of LDS) and that has no
# fallback: every family must refuse it and leave its outputs alone.
REFUSED = ((1, 4, 96), (16, 32, 40))

# ---- layouts -----------------------------------------------------------------------------------------------------------
# Packed frames: contiguous, and -- 3-channel integer frames only (check_pixel_buffers: RGBA / BGRA stay 16-byte aligned)
# -- the same samples in storage that starts 4 bytes past a 16-byte boundary.
PACKED_LAYOUTS = ("contiguous", "off4")
# Surfaces: tight planes; pitch = row + 64 bytes; ONE allocation per batch, [B, 3 H / 2 + 2, pitch] with UV behind Y, so
# that both image strides are pitch * (3 H / 2 + 2) > pitch * H (what a decoder delivers; two spare alignment rows); tight
# planes that start 4 bytes past an 8-byte boundary (check_yuv_pointers admits 4-byte alignment: the uint16 paths do
# two-dword accesses for that reason).
SURFACE_LAYOUTS = {"interior": ("tight", "pitch64", "off4"), "uhd_row": ("tight", "pitch64", "one_allocation"),
                   "many_seg": ("tight", "pitch64"), "one_cell": ("tight", "pitch64", "one_allocation"),
                   "tall": ("tight", "pitch64")}
GUARD_BYTES = 4096   # behind every buffer (and the 4 bytes in front of an "off4" one)
FILLS = (0xA5, 0x5A)  # byte fills of outputs: a sample never written cannot equal the expected one under both


def surface_layout(shape, size, layout):
    """Where the two planes of a ``shape = (B, H, W)`` surface of ``size``-byte samples lie: ``(buffer lengths, y, uv)``
    with ``y`` / ``uv`` = ``(buffer index, offset, shape, strides)``, everything in SAMPLES.  Each buffer ends in GUARD_BYTES
    of guard."""
    B, H, W = shape
    assert H % 2 == 0 and W % 4 == 0
    guard = GUARD_BYTES // size
    if layout in ("tight", "off4"):
        off = 4 // size if layout == "off4" else 0
        return ([off + B * H * W + guard, off + B * (H // 2) * W + guard],
                (0, off, (B, H, W), (H * W, W, 1)), (1, off, (B, H // 2, W), ((H // 2) * W, W, 1)))
    pitch = W + 64 // size
    if layout == "pitch64":
        return ([B * H * pitch + guard, B * (H // 2) * pitch + guard],
                (0, 0, (B, H, W), (H * pitch, pitch, 1)), (1, 0, (B, H // 2, W), ((H // 2) * pitch, pitch, 1)))
    assert layout == "one_allocation", layout
    rows = 3 * H // 2 + 2
    return ([B * rows * pitch + guard],
            (0, 0, (B, H, W), (rows * pitch, pitch, 1)), (0, H * pitch, (B, H // 2, W), (rows * pitch, pitch, 1)))


def plane(bufs, spec):
    """The numpy view of a plane in its flat buffer."""
    i, off, shape, strides = spec
    flat = bufs[i]
    return np.lib.stride_tricks.as_strided(flat[off:], shape, tuple(s * flat.itemsize for s in strides))


def fill_value(dtype, fill):
    """The sample whose bytes are all ``fill``."""
    return np.dtype(dtype).type(fill * (0x101 if np.dtype(dtype).itemsize == 2 else 1))


def lay_surface(y, uv, layout, fill=yc.POISON):
    """The surface's samples in ``layout``, everything around them (padding, spare rows, guards) filled with ``fill`` bytes:
    ``(flat buffers, y spec, uv spec)``."""
    lengths, sy, suv = surface_layout(y.shape, y.itemsize, layout)
    bufs = [np.full(n, fill_value(y.dtype, fill), y.dtype) for n in lengths]
    plane(bufs, sy)[...] = y
    plane(bufs, suv)[...] = uv
    return bufs, sy, suv


def outside_planes(bufs, specs):
    """Per buffer, the boolean mask of the samples that belong to no plane."""
    masks = [np.ones(b.shape, bool) for b in bufs]
    for spec in specs:
        plane(masks, spec)[...] = False
    return masks


def lay_packed(frame, layout, fill=yc.POISON):
    """A packed frame in ``layout``: ``(flat buffer, offset in samples)``; GUARD_BYTES of guard behind it."""
    assert layout in PACKED_LAYOUTS and (layout == "contiguous" or frame.shape[-1] == 3)
    off = 4 // frame.itemsize if layout == "off4" else 0
    buf = np.full(off + frame.size + GUARD_BYTES // frame.itemsize, fill_value(frame.dtype, fill), frame.dtype)
    buf[off:off + frame.size] = frame.reshape(-1)
    return buf, off


# ---- contents: the generators of the three existing files, with the grid's extents as an argument ---------------------------
def guides(rng, shape, grid):
    """tests/test_gpu_u16_out.py::_guides: a grid near the identity + 0.15 sigma noise (the output spans [0, 1] and beyond:
    both clips are hit), a guide map and the parameter sets of every guide form."""
    B, H, W = shape
    GH, GW, GD = grid
    grid6 = np.zeros((B, GH, GW, GD, 3, 4), np.float32)
    for i in range(3):
        grid6[..., i, i] = 1.0
    return {"grid": (grid6 + 0.15 * rng.standard_normal(grid6.shape)).astype(np.float32).reshape(B, GH, GW, GD, 12),
            "guide": rng.random((B, H, W)).astype(np.float32),
            "conv1": (rng.standard_normal((16, 4)) * 0.8).astype(np.float32),
            "conv2": (rng.standard_normal(17) * 0.5).astype(np.float32),
            "ccm": (np.eye(3, 4) + 0.1 * rng.standard_normal((3, 4))).astype(np.float32),
            # 16 knots per channel, well apart (the prepared cell tables need >= 1/63 of the knot range between two)
            "shifts": (np.linspace(0.0, 0.9, 16)[:, None] + 0.01 * rng.random((16, 3))).astype(np.float32),
            "slopes": (0.3 * rng.standard_normal((16, 3))).astype(np.float32),
            "shifts20": (np.linspace(0.0, 0.95, 20)[:, None] + 0.01 * rng.random((20, 3))).astype(np.float32),
            "slopes20": (0.25 * rng.standard_normal((20, 3))).astype(np.float32),
            "mix": np.array([0.4, 0.35, 0.3, 0.1], np.float32)}


def curves_of(c, guide):
    """The curves parameters of guide form ``guide``: 20 knots for the knot-by-knot form, 16 otherwise."""
    names = ("ccm", "shifts20", "slopes20", "mix") if guide == "scan" else ("ccm", "shifts", "slopes", "mix")
    return tuple(c[k] for k in names)


_CASES = {}


def _geo_seed(geo):
    return GEOMETRY_IDS.index(geo) if geo in GEOMETRIES else len(GEOMETRY_IDS)


def _extents(geo):
    return GEOMETRIES[geo] if geo in GEOMETRIES else REFUSED


def frame_case(geo, dtype, wl):
    """Guides and, per pixel format, a frame with the SAME colours and alpha (tests/test_gpu_pixel_formats.py::_case; a
    float32 frame is RGB only): deterministic in its arguments, so every format of a case shares one RGB reference."""
    key = ("frame", geo, dtype, wl)
    if key not in _CASES:
        shape, grid = _extents(geo)
        rng = np.random.default_rng([61, _geo_seed(geo), int(wl), {"uint8": 1, "uint16": 2, "float32": 4}[dtype]])
        c = guides(rng, shape, grid)
        if dtype == "float32":
            c["frames"] = {"rgb": rng.random(shape + (3,)).astype(np.float32)}
        else:
            rgba = px.random_frame(rng, shape, "rgba", dtype, wl)
            c["frames"] = {"rgb": np.ascontiguousarray(rgba[..., :3]), "bgr": np.ascontiguousarray(rgba[..., 2::-1]),
                           "rgba": rgba, "bgra": np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])}
            for fmt in px.FORMATS:
                assert np.array_equal(px.to_rgb(c["frames"][fmt], fmt), c["frames"]["rgb"])
        _CASES[key] = c
    return _CASES[key]


def surface_case(geo, bits, seed=0):
    """Guides and ONE surface content (``yuv_cases.random_surface``: the whole code range, the corners pinned to the
    extreme codes) per (geometry, bit depth): every layout holds the same samples, so the layouts share the references.
    ``seed``: raised only if a content fails the caps on undecided samples of the surface-output tests (none does)."""
    key = ("surface", geo, bits, seed)
    if key not in _CASES:
        shape, grid = _extents(geo)
        rng = np.random.default_rng([67, _geo_seed(geo), bits, seed])
        c = guides(rng, shape, grid)
        c["y"], c["uv"] = yc.random_surface(rng, shape, bits)
        _CASES[key] = c
    return _CASES[key]


def f32_frame_case(geo):
    """The anchor's case: a float32 RGB frame in [0, 1) with the guides."""
    return frame_case(geo, "float32", 1.0)


# ---- surfaces out: the float64 encoders of tests/yuv_cases.py / tests/u16_out_cases.py and their rule ------------------------
# pair -> (bits in, standard, full range, bits out).  The kernels know sample widths, not bit depths: P010 in runs the
# p016 instantiations with other constants.
SURFACE_OUT = {"nv12->nv12": (8, "bt709", False, 8), "p016->nv12": (16, "bt601", True, 8),
               "p010->p010": (10, "bt709", False, 10), "p016->p016": (16, "bt601", True, 16)}


def encode64(rgb, from_rgb, out_bits):
    """``(y, uv, y decided, uv decided, low-bit mask)``: the planes AS STORED that the float64 encoder gives for the float32
    frame ``rgb``, and where float64 decides the code by more than eps (1e-3 of an 8-bit code, scaled to the depth)."""
    import u16_out_cases as uc
    if out_bits == 8:
        yq, uvq, y_pre, uv_pre = yc.encode_nv12_64(rgb, from_rgb)
        return yq, uvq, yc.decided(y_pre), yc.decided(uv_pre), 0
    yq, uvq, y_pre, uv_pre = uc.encode_p016_64(rgb, from_rgb, out_bits)
    return yq, uvq, uc.decided(y_pre, out_bits), uc.decided(uv_pre, out_bits), (1 << uc.stored_shift(out_bits)) - 1


def within_cap(out_bits, undecided, total):
    """The condition on the reference alone (test_nv12_output / test_p016_output): under 1 % undecided at 8 bits, under
    2 % at 10, at least 40 % decided at 16 (float32 cannot resolve more there)."""
    if out_bits == 16:
        return total - undecided >= 0.40 * total
    return undecided < (0.01 if out_bits == 8 else 0.02) * total


# ---- the vertical regime, from the kernels' float32 formula -------------------------------------------------------------------
def gy_of_rows(H, GH):
    """gy = (y + 0.5) * (GH / H) - 0.5 of every image row, in float32 as stage_image computes it."""
    scale_y = np.float32(GH) / np.float32(H)
    return (np.arange(H, dtype=np.float32) + np.float32(0.5)) * scale_y - np.float32(0.5)


def clamped_rows(H, GH):
    """``(rows with gy < 0, rows with gy > GH - 1)``."""
    gy = gy_of_rows(H, GH)
    return [int(y) for y in np.nonzero(gy < 0)[0]], [int(y) for y in np.nonzero(gy > np.float32(GH - 1))[0]]


def pair_floors(H, GH):
    """Per chroma pair (rows 2 k, 2 k + 1): whether the two rows share floor(gy)."""
    f = np.floor(gy_of_rows(H, GH)).astype(np.int64)
    return [bool(f[2 * k] == f[2 * k + 1]) for k in range(H // 2)]
