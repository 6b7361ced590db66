"""oracle/f64_ops.py -- the float64 restatement of BilateralSliceApply / BilateralSlice, forward and every VJP -- pinned
on the CPU, and the reference's own float32 arithmetic (the C oracle) measured against it:

* bit-equal with oracle/f64_vjps.py (dguide, dinput of the 3 -> 3 op with offset) on that file's domain;
* the adjoint identities of the forward in float64, relative 1e-12: both ops, with and without offset, four channel shapes;
* a central finite difference of the float64 forward in the guide against dguide, relative 1e-6;
* the C oracle within the suite's bars (tests/conftest.py) of float64 on frame-like shapes -- on a path that shares
  nothing with it, which also shows that the reference's gather over a MIRRORED pixel window
  (bilateral_slice_apply.cc:84-138) is the transpose of its CLAMPED forward;
* the factors GD / 8 and C / 12 that the GPU suite puts on the dguide bar (tests/test_gpu_luma_bins.py::check_pix,
  tests/test_gpu_fuzz.py), measured on the reference alone.
"""
import functools

import numpy as np
import pytest

from conftest import DGUIDE_ATOL, DINPUT_ATOL, GRAD_RTOL

from oracle.f64_ops import f64_slice, f64_slice_apply
from oracle.f64_vjps import f64_vjps


def draw(seed, B, H, W, GH, GW, GD, Cin, Cout, off, lo=-0.02, hi=1.02):
    """The suite's data: grid in [0, 1), guide a little past [0, 1] (the clamped half cells at both ends of z), input in
    [0, 1), dout ~ N(0, 1).  Cin = None: the slice op with Cout channels."""
    rng = np.random.default_rng(seed)
    C = Cout if Cin is None else Cout * (Cin + (1 if off else 0))
    grid = rng.random((B, GH, GW, GD, C), dtype=np.float32)
    guide = (rng.random((B, H, W), dtype=np.float32) * (hi - lo) + lo).astype(np.float32)
    inp = None if Cin is None else rng.random((B, H, W, Cin), dtype=np.float32)
    dout = rng.standard_normal((B, H, W, Cout)).astype(np.float32)
    return grid, guide, inp, dout


# ---- 1. bit-equal with f64_vjps on its domain ------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,GH,GW,GD", [(1, 45, 64, 4, 4, 8), (2, 37, 52, 3, 5, 16)])
def test_bit_equal_with_f64_vjps(B, H, W, GH, GW, GD):
    grid, guide, inp, dout = draw(11 * B + GD, B, H, W, GH, GW, GD, 3, 3, True, -0.1, 1.1)
    dg, di = f64_vjps(grid, guide, inp, dout)
    _, _, dg2, di2 = f64_slice_apply(grid, guide, inp, dout, True)
    assert np.array_equal(dg, dg2)
    assert np.array_equal(di, di2)
    # the chunking is bookkeeping only
    _, _, dg3, di3 = f64_slice_apply(grid, guide, inp, dout, True, rows_per_chunk=7)
    assert np.array_equal(dg, dg3) and np.array_equal(di, di3)


# ---- 2. adjoint identities, float64 ------------------------------------------------------------------------------------
def _rel(a, b, scale):
    print(f"   {a!r} vs {b!r}: |diff| / scale = {abs(a - b) / scale:.2e}")
    return abs(a - b) / scale


@pytest.mark.parametrize("off", [True, False])
@pytest.mark.parametrize("Cin,Cout", [(3, 3), (4, 4), (1, 3), (2, 5)])
def test_apply_adjoints_float64(Cin, Cout, off):
    """<dgrid, grid> == <dout, out> (the op is linear in the grid) and <dinput, input> + <dout, out(input = 0)> ==
    <dout, out> (affine in the input), both sides float64 sums of float64 values."""
    grid, guide, inp, dout = draw(100 * Cin + Cout + off, 2, 23, 41, 3, 5, 7, Cin, Cout, off, -0.2, 1.2)
    out, dgrid, _, dinput = f64_slice_apply(grid, guide, inp, dout, off)
    d = dout.astype(np.float64)
    rhs = float((d * out).sum())
    scale = float((np.abs(d) * np.abs(out)).sum())
    assert _rel(float((dgrid * grid).sum()), rhs, scale) <= 1e-12
    out0 = f64_slice_apply(grid, guide, np.zeros_like(inp), None, off)[0]
    assert _rel(float((dinput * inp).sum()) + float((d * out0).sum()), rhs, scale) <= 1e-12


@pytest.mark.parametrize("C", [1, 2, 12, 5])
def test_slice_adjoint_float64(C):
    grid, guide, _, dout = draw(200 + C, 2, 23, 41, 3, 5, 7, None, C, False, -0.2, 1.2)
    out, dgrid, _ = f64_slice(grid, guide, dout)
    d = dout.astype(np.float64)
    assert _rel(float((dgrid * grid).sum()), float((d * out).sum()), float((np.abs(d) * np.abs(out)).sum())) <= 1e-12


# ---- 3. finite difference in the guide -----------------------------------------------------------------------------------
def _away_from_kinks(guide, GD):
    """tests/test_oracle_pinning.py::_fd_case: every sample >= 0.1 cell from a half-integer of guide * GD."""
    t = guide.astype(np.float64) * GD - 0.5
    frac = t - np.floor(t)
    return (np.floor(t) + np.clip(frac, 0.1, 0.9) + 0.5) / GD


@pytest.mark.parametrize("op,Cin,Cout,off", [("apply", 3, 3, True), ("apply", 2, 5, False), ("apply", 4, 4, True),
                                             ("slice", None, 12, False), ("slice", None, 1, False)])
def test_guide_finite_difference_float64(op, Cin, Cout, off):
    """(L(guide + h) - L(guide - h)) / 2h per pixel, L = <dout, out>, h = 1e-6, float64 guide (taken as exact by
    f64_ops), against dguide: relative 1e-6 of max|dguide|.  Away from the kinks the tent is 1 - sqrt(d^2 + 1e-8): its
    third derivative is ~1e-5 there, so the truncation error is ~1e-17 and what is left is the rounding of L, ~1e-16 / h."""
    GD = 7
    grid, guide, inp, dout = draw(300 + Cout, 2, 19, 33, 3, 4, GD, Cin, Cout, off, 0.0, 1.0)
    guide = _away_from_kinks(guide, GD)   # float64
    d = dout.astype(np.float64)
    if op == "apply":
        fwd = lambda gu: f64_slice_apply(grid, gu, inp, None, off)[0]  # noqa: E731
        dguide = f64_slice_apply(grid, guide, inp, dout, off)[2]
    else:
        fwd = lambda gu: f64_slice(grid, gu)[0]  # noqa: E731
        dguide = f64_slice(grid, guide, dout)[2]
    h = 1e-6
    fd = ((fwd(guide + h) - fwd(guide - h)) * d).sum(-1) / (2 * h)
    err = np.abs(fd - dguide).max() / np.abs(dguide).max()
    print(f"{op} {Cin}->{Cout} off={off}: max|fd - dguide| / max|dguide| = {err:.2e} (max|dguide| = {np.abs(dguide).max():.3g})")
    assert err <= 1e-6


# ---- 4. the C oracle against float64, at the suite's bars ------------------------------------------------------------------
# (B, H, W, GH, GW, GD, Cin, Cout): the apply op with offset; Cin None: the slice op
SHAPES = {
    "apply 135x240 GD8": (1, 135, 240, 16, 16, 8, 3, 3),
    "apply 135x240 GD16": (1, 135, 240, 16, 16, 16, 3, 3),
    "apply 135x240 GD4": (1, 135, 240, 16, 16, 4, 3, 3),
    "apply 135x240 GD12": (1, 135, 240, 16, 16, 12, 3, 3),
    "apply 270x480 GD8": (1, 270, 480, 16, 16, 8, 3, 3),
    "apply 270x480 GD16": (1, 270, 480, 16, 16, 16, 3, 3),
    "apply 4->4 135x240 GD8": (1, 135, 240, 16, 16, 8, 4, 4),
    "apply 2x96x128 grid 3x8 GD16": (2, 96, 128, 3, 8, 16, 3, 3),
    "slice C12 135x240 GD8": (1, 135, 240, 16, 16, 8, None, 12),
    "slice C12 135x240 GD16": (1, 135, 240, 16, 16, 16, None, 12),
    "slice C2 135x240 GD8": (1, 135, 240, 16, 16, 8, None, 2),
    "slice C12 135x240 GD4": (1, 135, 240, 16, 16, 4, None, 12),
    "slice C12 135x240 GD12": (1, 135, 240, 16, 16, 12, None, 12),
    "slice C16 135x240 GD8": (1, 135, 240, 16, 16, 8, None, 16),
    "slice C20 135x240 GD8": (1, 135, 240, 16, 16, 8, None, 20),
}


@functools.lru_cache(maxsize=None)
def distances(name):
    """{output: (max|port - f64|, rms, max|f64|)} of one shape; float64 and the C oracle are computed once per session."""
    import oracle
    port = oracle.port()
    B, H, W, GH, GW, GD, Cin, Cout = SHAPES[name]
    grid, guide, inp, dout = draw(sum(map(ord, name)), B, H, W, GH, GW, GD, Cin, Cout, True)
    if Cin is None:
        want = dict(zip(("out", "dgrid", "dguide"), f64_slice(grid, guide, dout)))
        got = dict(zip(("dgrid", "dguide"), port.bilateral_slice_grad(grid, guide, dout)), out=port.bilateral_slice(grid, guide))
    else:
        want = dict(zip(("out", "dgrid", "dguide", "dinput"), f64_slice_apply(grid, guide, inp, dout, True)))
        got = dict(zip(("dgrid", "dguide", "dinput"), port.bilateral_slice_apply_grad(grid, guide, inp, dout, True)),
                   out=port.bilateral_slice_apply(grid, guide, inp, True))
    res = {}
    for o, w in want.items():
        err = np.abs(got[o] - w)
        res[o] = (float(err.max()), float(np.sqrt((err * err).mean())), float(np.abs(w).max()),
                  float((err - GRAD_RTOL * np.abs(w)).max()))
    return res


TABLE = ["apply 135x240 GD8", "apply 135x240 GD16", "apply 135x240 GD4", "apply 270x480 GD8", "apply 270x480 GD16",
         "apply 4->4 135x240 GD8", "apply 2x96x128 grid 3x8 GD16", "slice C12 135x240 GD8", "slice C12 135x240 GD16",
         "slice C2 135x240 GD8"]


@pytest.mark.parametrize("name", TABLE)
def test_reference_float32_within_the_suite_s_bars_of_float64(name):
    """forward 1e-5, dinput 1e-5, dguide 2e-5 x max(1, GD / 8), dgrid 1e-4 |want| + 1e-5 max(1, max|want|): the bars the
    GPU suite holds the HIP kernels to against this same C oracle, here held by the oracle against the exact value."""
    GD = SHAPES[name][5]
    res = distances(name)
    for o, (mx, rms, scale, over_rtol) in res.items():
        print(f"{name} {o}: max|f32 - f64| = {mx:.3e}, rms = {rms:.3e}, max|want| = {scale:.3g}")
    assert res["out"][0] <= 1e-5
    if "dinput" in res:
        assert res["dinput"][0] <= DINPUT_ATOL
    assert res["dguide"][0] <= DGUIDE_ATOL * max(1.0, GD / 8.0)
    assert res["dgrid"][3] <= 1e-5 * max(1.0, res["dgrid"][2])   # max(err - 1e-4 |want|) <= atol


# ---- 5. the factors on the dguide bar, measured on the reference alone ---------------------------------------------------------
@pytest.mark.parametrize("name", ["apply 135x240 GD4", "apply 135x240 GD8", "apply 135x240 GD12", "apply 135x240 GD16",
                                  "slice C12 135x240 GD4", "slice C12 135x240 GD8", "slice C12 135x240 GD12",
                                  "slice C12 135x240 GD16", "slice C16 135x240 GD8", "slice C20 135x240 GD8"])
def test_reference_dguide_noise_behind_the_depth_and_channel_factors(name):
    """The GPU suite's dguide bar is DGUIDE_ATOL x max(1, GD / 8), and x max(1, C / 12) in the slice fuzz.  The
    reference's own float32 dguide must sit under it at every depth and channel count the factors are used for --
    otherwise the bar would ask a kernel for less noise than the reference has."""
    _, _, _, _, _, GD, Cin, Cout = SHAPES[name]
    C = 12 if Cin is not None else Cout
    mx, rms, scale, _ = distances(name)["dguide"]
    bar = DGUIDE_ATOL * max(1.0, GD / 8.0) * max(1.0, C / 12.0)
    print(f"{name}: reference dguide max|f32 - f64| = {mx:.3e} (rms {rms:.3e}, max|dguide| = {scale:.3g}), bar {bar:.2e}, "
          f"noise / bar = {mx / bar:.2f}")
    assert mx <= bar
