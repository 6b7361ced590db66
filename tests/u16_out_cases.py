"""16-bit output (include/hdrnet_amd_u16_out.h), stated once in numpy for tests/test_u16_out_host.py and
tests/test_gpu_u16_out.py: the uint16 frame store's rule on a float32 frame, and tests/yuv_cases.py's float64 surface
encoder and its margin generalised from NV12 to a code maximum and a shift (P010 / P016).  No GPU, no package import."""
import numpy as np


def quantise_u16(f, white_level):
    """The frame store's rule on the float32 output ``f`` of the existing path: ONE float32 multiply of the clipped value
    by the white level, then truncation."""
    f = np.asarray(f)
    assert f.dtype == np.float32
    return (np.float32(white_level) * np.clip(f, np.float32(0), np.float32(1))).astype(np.uint16)


def code_max(bits):
    return float(2 ** bits - 1)


def stored_shift(bits):
    """A code of ``bits`` bits sits in the high bits of its uint16 sample."""
    return 16 - bits


def eps_of(bits):
    """tests/yuv_cases.py's margin of 1e-3 of an 8-bit code, carried to the same number of float32 ulps of the code
    range of ``bits`` bits."""
    return 1e-3 * 2 ** (bits - 8)


def encode_p016_64(rgb, from_rgb, bits):
    """``yuv_cases.encode_nv12_64`` with a code maximum and a shift: float64 encoder of the header's rule on ``rgb``
    ``[B, H, W, 3]`` -- clip to [0, 1], Y per pixel, U and V from the mean of each 2 x 2 block, + bias (the + 0.5 is in
    it), clamp to [0, 2^bits - 1], truncate, shift into the high bits.  Returns ``(y_sample, uv_sample, y_pre, uv_pre)``:
    uint16 planes ``[B, H, W]`` / ``[B, H / 2, W]`` AS STORED and the float64 values before the clamp and the truncation, in
    code units."""
    k = np.asarray(from_rgb, np.float64)
    c = np.clip(np.asarray(rgb, np.float64), 0.0, 1.0)
    B, H, W, _ = c.shape
    y_pre = c @ k[0:3] + k[9]
    mean = c.reshape(B, H // 2, 2, W // 2, 2, 3).mean(axis=(2, 4))
    uv_pre = np.empty((B, H // 2, W), np.float64)
    uv_pre[:, :, 0::2] = mean @ k[3:6] + k[10]
    uv_pre[:, :, 1::2] = mean @ k[6:9] + k[11]
    top, shift = code_max(bits), stored_shift(bits)
    sample = lambda t: (np.floor(np.clip(t, 0.0, top)).astype(np.uint32) << shift).astype(np.uint16)  # noqa: E731
    return sample(y_pre), sample(uv_pre), y_pre, uv_pre


def decided(pre, bits):
    """Samples whose code is the same for every value within ``eps_of(bits)`` of the float64 pre-truncation value."""
    eps, top = eps_of(bits), code_max(bits)
    return np.floor(np.clip(pre - eps, 0.0, top)) == np.floor(np.clip(pre + eps, 0.0, top))


def code_diff(plane, want, bits):
    """|difference| of two planes of stored samples in CODES of ``bits`` bits (the low bits must be zero in both)."""
    shift = stored_shift(bits)
    return np.abs((plane.astype(np.int64) >> shift) - (want.astype(np.int64) >> shift))
