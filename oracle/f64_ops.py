"""TEST INFRASTRUCTURE: float64 evaluation of BilateralSliceApply and BilateralSlice, forward and every VJP.

The formulas of hdrnet/ops/bilateral_slice_apply.cc:24-259 and hdrnet/ops/bilateral_slice.cc:25-168 for any B, H, W, GH,
GW, GD, Cin, Cout, with and without the affine offset -- oracle/f64_vjps.py generalised from (dguide, dinput) of the 3 -> 3
op with offset to both ops and all outputs.  The rules are that file's:

* the coordinates ((x + .5) * (GW / W), guide * GD), the tap indices, (float)gz + 0.5f - gzf and the decision where the
  derivative of the smoothed tent is cut to 0 are formed in FLOAT32 as the reference forms them: they select WHICH
  function is evaluated and are part of the op's semantics, not of its rounding noise;
* every weight, product and sum is float64;
* grid channel c = i * Cj + j (output i, input j; j == Cin is the offset); the taps are clamped in x, y and z;
* dgrid is the exact TRANSPOSE of the forward: dout_i * in_j * wx * wy * wz scattered to the clamped tap.  It is not a
  restatement of the reference's gather over a mirrored pixel window (bilateral_slice_apply.cc:84-138) -- that the two
  agree is what tests/test_f64_ops.py checks;
* row chunks, so that a 1080p frame fits in memory.

A float64 `guide` is taken as exact: gzf = guide * GD stays float64 (the tap index and the cut decision are still taken
from its float32 rounding).  That is what a finite difference in the guide needs -- a step of 1e-6 does not survive a
float32 guide -- and changes nothing for float32 guides, which is what every other caller passes.

Used by tests/ to measure how far a float32 implementation -- the reference's own arithmetic (the C oracle) or the HIP
kernels -- is from the exact value of the reference's formulas.
"""
import numpy as np


def _xy_taps(n, gn):
    """Along one spatial axis: the float32 coordinate of every pixel, and for the two taps the clamped cell index and the
    float64 tent weight."""
    f32 = np.float32
    c = (np.arange(n, dtype=f32) + f32(0.5)) * (f32(gn) / f32(n))
    g0 = np.floor(c - f32(0.5)).astype(np.int64)
    taps = []
    for d in (0, 1):
        g = g0 + d
        w = np.maximum(1 - np.abs((g.astype(f32) + f32(0.5)) - c).astype(np.float64), 0)
        taps.append((np.clip(g, 0, gn - 1), w))
    return taps


def f64_slice_apply(grid, guide, inp, dout=None, has_offset=True, rows_per_chunk=128):
    """-> (out, dgrid, dguide, dinput) in float64; the three gradients are None where `dout` is None."""
    f32 = np.float32
    B, GH, GW, GD, C = grid.shape
    _, H, W = guide.shape
    Cin = inp.shape[3]
    Cj = Cin + (1 if has_offset else 0)
    Cout = C // Cj
    assert Cout * Cj == C and inp.shape[:3] == guide.shape and guide.shape[0] == B
    G = grid.astype(np.float64).reshape(B, GH, GW, GD, Cout, Cj)
    eps = np.float64(np.float32(1e-8))
    xt, yt = _xy_taps(W, GW), _xy_taps(H, GH)
    exact_guide = guide.dtype == np.float64
    out = np.zeros((B, H, W, Cout))
    grads = dout is not None
    dgrid = np.zeros((B, GH * GW * GD, C)) if grads else None
    dg = np.zeros((B, H, W)) if grads else None
    di = np.zeros((B, H, W, Cin)) if grads else None
    for b in range(B):
        for r0 in range(0, H, rows_per_chunk):
            r1 = min(H, r0 + rows_per_chunk)
            if exact_guide:
                gzf = guide[b, r0:r1] * np.float64(GD)
                gzf32 = gzf.astype(f32)
            else:
                gzf = gzf32 = (guide[b, r0:r1] * f32(GD)).astype(f32)
            gz0 = np.floor(gzf32 - f32(0.5)).astype(np.int64)
            inh = inp[b, r0:r1].astype(np.float64)
            if has_offset:
                inh = np.concatenate([inh, np.ones((r1 - r0, W, 1))], -1)
            if grads:
                d64 = dout[b, r0:r1].astype(np.float64)
                outer = (d64[..., :, None] * inh[..., None, :]).reshape(r1 - r0, W, C)   # dout_i in_j at c = i Cj + j
            for gyc, wy in yt:
                for gxc, wx in xt:
                    w2 = wy[r0:r1, None] * wx[None, :]
                    for dz in (0, 1):
                        gz = gz0 + dz
                        if exact_guide:
                            d = (gz.astype(np.float64) + 0.5) - gzf
                            d32 = d.astype(f32)
                        else:
                            d32 = (gz.astype(f32) + f32(0.5)) - gzf
                            d = d32.astype(np.float64)
                        s = np.sqrt(d * d + eps)
                        wz = np.maximum(1 - s, 0)                # numerics.h:108-113
                        gzc = np.clip(gz, 0, GD - 1)
                        g = G[b][gyc[r0:r1, None], gxc[None, :], gzc]  # [rows, W, Cout, Cj]
                        out[b, r0:r1] += np.einsum("hwij,hwj->hwi", g, inh) * (w2 * wz)[..., None]
                        if not grads:
                            continue
                        # numerics.h:116-126: the derivative is CUT to 0 where the smoothed |d| exceeds 1.  That decision
                        # is taken in float32 as the reference takes it (a tap exactly one cell away has
                        # sqrtf(1 + 1e-8f) == 1.0f: not cut, while sqrt(1 + 1e-8) > 1 in float64); the value is then
                        # formed in float64
                        cut = np.sqrt((d32 * d32).astype(f32) + f32(1e-8), dtype=f32) > f32(1)
                        dw = np.where(cut, 0.0, d / s) * GD     # x GD (bilateral_slice_apply.cc:186)
                        dg[b, r0:r1] += np.einsum("hwij,hwj,hwi->hw", g, inh, d64) * (w2 * dw)
                        di[b, r0:r1] += np.einsum("hwij,hwi->hwj", g[..., :Cin], d64) * (w2 * wz)[..., None]
                        cell = ((gyc[r0:r1, None] * GW + gxc[None, :]) * GD + gzc).ravel()
                        val = (outer * (w2 * wz)[..., None]).reshape(-1, C)
                        for c in range(C):  # the transpose of the forward's gather, summed in float64
                            dgrid[b, :, c] += np.bincount(cell, weights=val[:, c], minlength=GH * GW * GD)
    if grads:
        dgrid = dgrid.reshape(B, GH, GW, GD, C)
    return out, dgrid, dg, di


def f64_slice(grid, guide, dout=None, rows_per_chunk=128):
    """BilateralSlice -> (out, dgrid, dguide) in float64: the apply op with no input channel and the offset alone
    (Cj = 1, the offset's input is the constant 1, and x * 1.0 is exact)."""
    B, H, W = guide.shape
    out, dgrid, dg, _ = f64_slice_apply(grid, guide, np.zeros((B, H, W, 0), np.float32), dout, True, rows_per_chunk)
    return out, dgrid, dg
