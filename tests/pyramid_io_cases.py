"""Inputs and references of the pyramid model's wire-format up-add (tests/test_gpu_pyramid_io.py on the GPU,
tests/test_pyramid_io_host.py for the CPU-side check of the uint8 rule's cap).  Every reference is computed once per
process and shared; callers do not modify what they get.

One case = (shape, input format, guide kind).  The inputs are those of test_wire_format_forward (a near-identity affine, so
that the output spans [0, 1] and beyond) with a coarse level ~ 0.3 N(0, 1) on top: the sum leaves [0, 1] on both sides and
the clip AFTER the up-add decides the uint8 output."""
import functools

import numpy as np

# (B, H, W, Hc, Wc): the pyramid's 2:1 with two images; several segments per row; a one-column coarse level; a coarse
# level as wide as the fine one (the wide shapes of test_upadd_matches_composed_oracle)
SHAPES = [(2, 36, 64, 18, 32), (1, 6, 3840, 4, 1920), (1, 4, 1024, 2, 1), (1, 3, 1536, 3, 1536)]
# (input dtype, white level)
FORMATS = [("uint8", 255.0), ("uint16", 65535.0), ("uint16", 32767.0), ("float32", 1.0)]
GH, GW, GD = 16, 16, 8
TOL = 1e-5  # the forward's bar (tests/test_gpu_parity.py)


def seed_of(shape, fmt, nn):
    return 1000 + 97 * SHAPES.index(shape) + 11 * FORMATS.index(fmt) + int(nn)


@functools.lru_cache(maxsize=None)
def inputs(shape, fmt, nn):
    """dict: grid, raw (the wire-format input), inp_f (raw / white level in float32), coarse, conv1, conv2, guide."""
    import oracle
    B, H, W, Hc, Wc = shape
    in_dtype, wl = fmt
    rng = np.random.default_rng(seed_of(shape, fmt, nn))
    grid6 = np.zeros((B, GH, GW, GD, 3, 4), np.float32)
    for i in range(3):
        grid6[..., i, i] = 1.0
    grid = (grid6 + 0.15 * rng.standard_normal(grid6.shape)).astype(np.float32).reshape(B, GH, GW, GD, 12)
    if in_dtype == "float32":
        raw = rng.random((B, H, W, 3)).astype(np.float32)
        inp_f = raw
    else:
        hi = 256 if in_dtype == "uint8" else int(wl) + 1
        raw = rng.integers(0, hi, (B, H, W, 3)).astype(in_dtype)
        inp_f = (raw.astype(np.float32) / np.float32(wl)).astype(np.float32)
    coarse = (0.3 * rng.standard_normal((B, Hc, Wc, 3))).astype(np.float32)
    conv1 = (rng.standard_normal((16, 4)) * 0.8).astype(np.float32)
    conv2 = (rng.standard_normal(17) * 0.5).astype(np.float32)
    guide = oracle.pointwise_nn_guide(inp_f, conv1, conv2) if nn else rng.random((B, H, W)).astype(np.float32)
    return dict(grid=grid, raw=raw, inp_f=inp_f, coarse=coarse, conv1=conv1, conv2=conv2, guide=guide)


@functools.lru_cache(maxsize=None)
def want_f32(shape, fmt, nn):
    """The float32 oracle: port.bilateral_slice_apply + oracle.resize_bilinear_align_corners, added in float32."""
    import oracle
    c = inputs(shape, fmt, nn)
    B, H, W, _, _ = shape
    out = oracle.port().bilateral_slice_apply(c["grid"], c["guide"], c["inp_f"], True)
    return (out + oracle.resize_bilinear_align_corners(c["coarse"], H, W)).astype(np.float32)


def quantise(v):
    """tf.cast(255 * clip(v, 0, 1), uint8) in the dtype of v."""
    return (v.dtype.type(255.0) * np.clip(v, 0, 1)).astype(np.uint8)


def check_u8(got, want_f, what=""):
    """The uint8 rule of test_wire_format_forward: at most 1 LSB, only where 255 * clip(want) sits within 255 * 2e-5 of an
    integer, on fewer than 5e-4 of the samples, both ends of the range present.  Returns the share that differs."""
    v = 255.0 * np.clip(want_f.astype(np.float64), 0, 1)
    want_u8 = quantise(want_f)
    diff = np.abs(got.astype(np.int16) - want_u8.astype(np.int16))
    near_edge = np.abs(v - np.round(v)) < 255.0 * 2 * TOL
    share = float((diff > 0).mean())
    print(f"{what}: max LSB {int(diff.max())}, share differing {share:.2e}, off an edge {int(((diff > 0) & ~near_edge).sum())}")
    assert diff.max() <= 1
    assert not np.any((diff > 0) & ~near_edge)
    assert share < 5e-4
    assert got.min() == 0 and got.max() == 255  # the clip is exercised on both sides
    return share


def slice_apply_upadd_f64(c, shape):
    """The same formulas in float64 (bilateral_slice_apply.cc:24-82 + the up-add).  The grid coordinates and the resize
    taps are formed in float32 as the ops form them -- they are part of the semantics (oracle/f64_train.py) -- and
    every weight, blend, affine and sum after them is float64."""
    from oracle.f64_train import upsample_add_f64
    f32, f64 = np.float32, np.float64
    B, H, W, _, _ = shape
    grid = c["grid"].astype(f64).reshape(B, GH, GW, GD, 3, 4)
    gyf = ((np.arange(H, dtype=f32) + f32(0.5)) * (f32(GH) / f32(H))).astype(f32)
    gxf = ((np.arange(W, dtype=f32) + f32(0.5)) * (f32(GW) / f32(W))).astype(f32)
    gzf = (c["guide"] * f32(GD)).astype(f32)                         # [B, H, W]
    y0 = np.floor(gyf - f32(0.5)).astype(np.int64)
    x0 = np.floor(gxf - f32(0.5)).astype(np.int64)
    z0 = np.floor(gzf - f32(0.5)).astype(np.int64)
    out = np.zeros((B, H, W, 3), f64)
    inp1 = np.concatenate([c["inp_f"].astype(f64), np.ones((B, H, W, 1), f64)], axis=-1)
    bi = np.arange(B)[:, None, None]
    for dy in (0, 1):
        wy = np.maximum(1.0 - np.abs((y0 + dy + 0.5) - gyf.astype(f64)), 0.0)[None, :, None]
        yc = np.clip(y0 + dy, 0, GH - 1)[None, :, None]
        for dx in (0, 1):
            wx = np.maximum(1.0 - np.abs((x0 + dx + 0.5) - gxf.astype(f64)), 0.0)[None, None, :]
            xc = np.clip(x0 + dx, 0, GW - 1)[None, None, :]
            for dz in (0, 1):
                d = (z0 + dz + 0.5) - gzf.astype(f64)
                wz = np.maximum(1.0 - np.sqrt(d * d + 1e-8), 0.0)
                zc = np.clip(z0 + dz, 0, GD - 1)
                coef = grid[bi, yc, xc, zc]                          # [B, H, W, 3, 4]
                out += (wy * wx * wz)[..., None] * np.einsum("bhwij,bhwj->bhwi", coef, inp1)
    return upsample_add_f64(c["coarse"], out)
