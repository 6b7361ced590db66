"""Semi-planar YUV 4:2:0 surfaces (include/hdrnet_amd_yuv.h), stated once in numpy for the tests: random surfaces with a
chosen pitch and poisoned padding, the float64 evaluation of the 12-float conversion, and a float64 NV12 encoder that
also returns every value before truncation.  No GPU, no package import: the constants come in as arguments."""
import numpy as np

POISON = 0xA5
SAMPLE = {"uint8": np.uint8, "uint16": np.uint16}


def stored_shift(bits):
    """P010 keeps its 10-bit code in the high bits of the uint16 sample."""
    return 6 if bits == 10 else 0


def random_surface(rng, shape, bits, pad_bytes=0, corners=True):
    """A surface of ``shape = (B, H, W)`` with codes of ``bits`` bits (8: uint8, 10 / 16: uint16) drawn over the WHOLE code
    range -- super-black and super-white included -- and, with ``corners``, the image corners pinned to the extreme codes
    so that the conversion's clamp is exercised on both sides.  Rows are ``pad_bytes`` wider than their samples, the
    padding filled with POISON bytes.  Returns ``(y_buf, uv_buf)``, ``[B, H, pitch]`` and ``[B, H / 2, pitch]`` in
    samples; the planes are ``y_buf[:, :, :W]`` and ``uv_buf[:, :, :W]`` (U, V interleaved)."""
    B, H, W = shape
    dt = np.uint8 if bits == 8 else np.uint16
    size = np.dtype(dt).itemsize
    assert H % 2 == 0 and W % 4 == 0 and pad_bytes % 4 == 0
    pitch = W + pad_bytes // size
    poison = dt(POISON if size == 1 else POISON * 0x101)
    top = 2 ** bits
    y = np.full((B, H, pitch), poison, dt)
    uv = np.full((B, H // 2, pitch), poison, dt)
    y[:, :, :W] = (rng.integers(0, top, (B, H, W)) << stored_shift(bits)).astype(dt)
    uv[:, :, :W] = (rng.integers(0, top, (B, H // 2, W)) << stored_shift(bits)).astype(dt)
    if corners:
        lo, hi = dt(0), dt((top - 1) << stored_shift(bits))
        y[:, 0, 0], y[:, 0, W - 1], y[:, H - 1, 0], y[:, H - 1, W - 1] = lo, hi, hi, lo
        uv[:, 0, 0:2] = (top // 2) << stored_shift(bits)       # neutral chroma under the black / white luma
        uv[:, 0, W - 2:W] = (top // 2) << stored_shift(bits)
        uv[:, H // 2 - 1, 0:2] = lo, hi                         # and extreme chroma under the other two
        uv[:, H // 2 - 1, W - 2:W] = hi, lo
    return y, uv


def padding_intact(buf, W):
    size = buf.dtype.itemsize
    poison = POISON if size == 1 else POISON * 0x101
    return bool((buf[:, :, W:] == poison).all())


def replicate_chroma(uv):
    """``[B, H / 2, W]`` interleaved -> U, V ``[B, H, W]``: chroma sample (y >> 1, x >> 1) serves its 2 x 2 block."""
    u = uv[:, :, 0::2].repeat(2, axis=1).repeat(2, axis=2)
    v = uv[:, :, 1::2].repeat(2, axis=1).repeat(2, axis=2)
    return u, v


def to_rgb64(y, uv, to_rgb):
    """float64 evaluation of the conversion on the float32 constants as given: ``[B, H, W, 3]`` in [0, 1]."""
    k = np.asarray(to_rgb, np.float64)
    u, v = replicate_chroma(uv)
    Y, U, V = (a.astype(np.float64) for a in (y, u, v))
    out = np.stack([k[3 * i] * Y + k[3 * i + 1] * U + k[3 * i + 2] * V + k[9 + i] for i in range(3)], axis=-1)
    return np.clip(out, 0.0, 1.0)


def encode_nv12_64(rgb, from_rgb):
    """float64 NV12 encoder of the header's rule on ``rgb`` ``[B, H, W, 3]``: clip to [0, 1], Y per pixel, U and V from the
    mean of the four pixels of each 2 x 2 block, + bias (the + 0.5 is in it), clamp to [0, 255], truncate.  Returns
    ``(y_code, uv_code, y_pre, uv_pre)``: uint8 planes ``[B, H, W]`` / ``[B, H / 2, W]`` and the float64 values BEFORE the
    clamp and the truncation, in the same layout."""
    k = np.asarray(from_rgb, np.float64)
    c = np.clip(np.asarray(rgb, np.float64), 0.0, 1.0)
    B, H, W, _ = c.shape
    y_pre = c @ k[0:3] + k[9]
    mean = c.reshape(B, H // 2, 2, W // 2, 2, 3).mean(axis=(2, 4))
    uv_pre = np.empty((B, H // 2, W), np.float64)
    uv_pre[:, :, 0::2] = mean @ k[3:6] + k[10]
    uv_pre[:, :, 1::2] = mean @ k[6:9] + k[11]
    code = lambda t: np.floor(np.clip(t, 0.0, 255.0)).astype(np.uint8)  # noqa: E731
    return code(y_pre), code(uv_pre), y_pre, uv_pre


def decided(pre, eps=1e-3):
    """Samples whose code is the same for every value within ``eps`` of the float64 pre-truncation value: further than
    ``eps`` from an integer (or beyond the clamp by more than ``eps``)."""
    lo = np.floor(np.clip(pre - eps, 0.0, 255.0))
    hi = np.floor(np.clip(pre + eps, 0.0, 255.0))
    return lo == hi
