"""Colour constants of the YUV surface paths (include/hdrnet_amd_yuv.h, include/hdrnet_amd_yuv_planar.h).

The kernels know nothing of colour standards, ranges or bit depths: they apply 12 floats to the samples as stored.
``yuv_coefficients`` computes those floats from the published BT.601 / BT.709 / BT.2020 luma weights (ITU-R BT.601-7,
BT.709-6, BT.2020-2: Kr, Kb; Kg = 1 - Kr - Kb) and the two quantisation ranges of those recommendations: "limited"
(luma 16 .. 235, chroma 16 .. 240 around 128, times ``2 ** (bits - 8)``) and "full" (0 .. ``2 ** bits - 1``, chroma around
``2 ** (bits - 1)``).  Host-side, float64, rounded to float32 once.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

__all__ = ["STANDARDS", "BITS", "yuv_coefficients", "yuv_encode_coefficients", "code_ranges"]

# (Kr, Kb) of the luma equation  Y' = Kr R' + Kg G' + Kb B'
STANDARDS = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
BITS = (8, 10, 16)


def code_ranges(full_range: bool, bits: int) -> Tuple[float, float, float, float]:
    """``(y_offset, y_scale, c_offset, c_scale)`` in CODE values of ``bits`` bits: luma code = y_offset + y_scale * Y'
    (Y' in [0, 1]), chroma code = c_offset + c_scale * C' (C' in [-0.5, 0.5])."""
    if full_range:
        top = float(2 ** bits - 1)
        return 0.0, top, float(2 ** (bits - 1)), top
    unit = float(2 ** (bits - 8))
    return 16.0 * unit, 219.0 * unit, 128.0 * unit, 224.0 * unit


def yuv_coefficients(standard: str = "bt709", full_range: bool = False, bits: int = 8,
                     msb_aligned: bool = True) -> Tuple[np.ndarray, np.ndarray]:
    """``(to_rgb, from_rgb)``: two float32 arrays of 12 numbers, a row-major 3 x 3 matrix then 3 biases.

    ``to_rgb`` applied to the RAW STORED samples (Y, U, V) as floats gives R, G, B, nominally in [0, 1]: range scaling and
    the chroma offset are in the numbers, and for ``bits = 10`` so is P010's placement of the code in the high bits (the
    sample as stored is ``code << 6``).  ``bits = 8`` is NV12, ``bits = 16`` P016.

    ``msb_aligned=False``: the code sits in the LOW bits of the sample, as in the planar ``yuv420p10le`` surfaces of
    include/hdrnet_amd_yuv_planar.h (the sample as stored is the code).  Only ``bits = 10`` differs: the matrix is exactly
    64 x the default one and the biases are equal (scaling by a power of two commutes with the float64 division and with
    the rounding to float32).

    ``from_rgb`` applied to R, G, B in [0, 1] gives Y, U, V in UINT8 code values of the same standard and range (the
    output surface is NV12 whatever the input's depth), with the + 0.5 of the rounding folded into the biases: the
    kernel truncates."""
    if standard not in STANDARDS:
        raise ValueError(f"yuv_coefficients: unknown standard {standard!r} (takes {', '.join(repr(k) for k in STANDARDS)})")
    if bits not in BITS:
        raise ValueError(f"yuv_coefficients: bits must be one of {BITS}, got {bits!r}")
    kr, kb = STANDARDS[standard]
    kg = 1.0 - kr - kb
    y_off, y_scale, c_off, c_scale = code_ranges(bool(full_range), bits)
    stored = 64.0 if bits == 10 and msb_aligned else 1.0  # P010: code << 6
    # R = Y' + 2 (1 - Kr) Cr',  B = Y' + 2 (1 - Kb) Cb',  G from the luma equation
    cu = np.array([0.0, -2.0 * kb * (1.0 - kb) / kg, 2.0 * (1.0 - kb)])  # weight of Cb' in R, G, B
    cv = np.array([2.0 * (1.0 - kr), -2.0 * kr * (1.0 - kr) / kg, 0.0])  # weight of Cr'
    to_rgb = np.zeros(12, np.float64)
    for i in range(3):
        to_rgb[3 * i] = 1.0 / (y_scale * stored)
        to_rgb[3 * i + 1] = cu[i] / (c_scale * stored)
        to_rgb[3 * i + 2] = cv[i] / (c_scale * stored)
        to_rgb[9 + i] = -y_off / y_scale - (cu[i] + cv[i]) * c_off / c_scale
    return to_rgb.astype(np.float32), yuv_encode_coefficients(standard, full_range, 8)


def yuv_encode_coefficients(standard: str = "bt709", full_range: bool = False, bits: int = 8) -> np.ndarray:
    """``from_rgb``: 12 float32 numbers, a row-major 3 x 3 matrix then 3 biases, that applied to R, G, B in [0, 1] give
    Y, U, V in CODE values of ``bits`` bits (8: NV12, 10: P010, 16: P016) of ``standard`` and range, with the + 0.5 of the
    rounding folded into the biases: the kernel clamps to ``[0, 2 ** bits - 1]`` and truncates, and for P010 places the
    code in the high bits itself (``out_bits``).  ``bits = 8`` is ``yuv_coefficients(...)[1]``, bit for bit."""
    if standard not in STANDARDS:
        raise ValueError(f"yuv_encode_coefficients: unknown standard {standard!r} (takes "
                         f"{', '.join(repr(k) for k in STANDARDS)})")
    if bits not in BITS:
        raise ValueError(f"yuv_encode_coefficients: bits must be one of {BITS}, got {bits!r}")
    kr, kb = STANDARDS[standard]
    kg = 1.0 - kr - kb
    y_off, y_scale, c_off, c_scale = code_ranges(bool(full_range), bits)
    luma = np.array([kr, kg, kb])
    from_rgb = np.zeros(12, np.float64)
    from_rgb[0:3] = y_scale * luma
    from_rgb[3:6] = c_scale * (np.array([0.0, 0.0, 1.0]) - luma) / (2.0 * (1.0 - kb))  # Cb' = (B - Y') / (2 (1 - Kb))
    from_rgb[6:9] = c_scale * (np.array([1.0, 0.0, 0.0]) - luma) / (2.0 * (1.0 - kr))  # Cr' = (R - Y') / (2 (1 - Kr))
    from_rgb[9:12] = [y_off + 0.5, c_off + 0.5, c_off + 0.5]
    return from_rgb.astype(np.float32)
