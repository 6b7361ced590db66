"""Every kernel family against answers a reader can check by hand (tests/closed_form.py; the CPU oracles are held to
the same answers in tests/test_closed_form.py).

Every other numerical GPU test compares a kernel with an oracle written from the same reading of the reference's layout
as the kernel, on uniform random data: a shared misreading -- gy and gx exchanged, c = j * Cout + i, z from the other end,
centres at p, mirrored borders, a BGR frame read as RGB -- would pass.  Here:

(i)   ADDRESS CODES (test_codes_*): the grid holds 1 + its own linear index, the guide sits on a plane centre, the input is
      zero or one-hot, and out / PEAK at the pixels on cell centres must read back code(b, gy, gx, gz, i * Cj + j) for
      every cell, plane, i and j -- through the plain ops (all eight fast apply shapes, slice with 1, 2, 12 and 16
      channels; generic kernels and auto dispatch, kernel name asserted; two more grids for the row-family forwards the
      16 x 16 x 8 grid never reaches) and through every other float32-out forward
      that takes a guide map (row bands, wire formats in all four pixel orders, the up-add forwards with a zero coarse
      level).  The integer-output entry points are left out: a truncating store cannot carry a code, and they are held
      equal to the quantised float32 result elsewhere (tests/test_gpu_wire_geometry.py, test_gpu_u16_out.py).
      Bar: |out / PEAK - integer| < 0.25 and every decode right -- a condition, not a measurement.
(ii)  ONE AXIS AT A TIME and (iii) ONE PLANE (test_axes_and_planes): forward and backward through the public autograd
      ops -- all three gradients together (the fused MFMA pass), dguide + dinput alone (apply_vjp_seg), the slice op
      with 12 channels -- at luma_bins 8 and 16, at 48 x 1040 and 64 x 256 (W = GW * 2^k: exact coordinates), under auto
      dispatch and under kernel_override("generic").  Bars: the suite's fixed ones (forward rtol = atol = 1e-5;
      conftest.check_pixel_grad; conftest.check_dgrid), taken against the closed form; the port's distance is printed
      beside each.  dgrid outside the guide's plane: exactly zero from the generic kernels, <= 1e-5 x scale from the
      fast pass.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import closed_form as cf  # noqa: E402
import row_plan as rp  # noqa: E402
from conftest import check_dgrid, check_pixel_grad  # noqa: E402

FWD_TOL = dict(rtol=1e-5, atol=1e-5)
B = 2
GRID = (16, 16, 8)                       # GH, GW, GD of family (i)
FRAMES = {"48x1040": (48, 1040), "16x16": (16, 16)}   # my = 3, mx = 65; one pixel per cell (exact coordinates)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from hdrnet_amd import hdrnet_ops
    return hdrnet_ops


@pytest.fixture(scope="module")
def mt_port(port):
    port.set_threads(min(os.cpu_count() or 1, 16))
    yield port
    port.set_threads(1)


def T(a, dev):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)
    return torch.from_numpy(a).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def read_back(run, codes, H, W, Cin, off, name):
    """Family (i) through `run(guide map on the device, j)` -> the output tensor; asserts the decode."""
    Cj = Cin + (1 if off else 0)
    got, dev_ = cf.decode(run, codes.shape, H, W, Cin, off)
    wrong, worst = cf.check_decode(got, dev_, codes, Cj, name)
    assert wrong == 0 and worst < cf.DECODE_BAR, name


def one_hot(dev, H, W, Cin, j, value=1.0, dtype=np.float32, channels=None, at=None, alpha=None):
    """[B, H, W, channels] of `dtype`: `value` at position `at` (default j) of every pixel for j not None, else zeros;
    `alpha`: the fourth component of a frame with alpha, which the op must not read."""
    a = np.zeros((B, H, W, channels or Cin), dtype)
    if alpha is not None:
        a[..., 3] = alpha
    if j is not None:
        a[..., j if at is None else at] = value
    return T(a, dev)


# ---- (i) the plain ops -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frame", sorted(FRAMES))
@pytest.mark.parametrize("shape", rp.APPLY_FAST_SHAPES, ids=lambda s: f"{s[0]}to{s[1]}{'_offset' if s[2] else ''}")
def test_codes_apply(dev, ops, shape, frame):
    Cin, Cout, off = shape
    H, W = FRAMES[frame]
    GH, GW, GD = GRID
    codes = cf.address_codes(B, GH, GW, GD, Cout * (Cin + off))
    tgrid = T(codes, dev)
    for which, kern in (("generic", "apply_fwd_generic"), ("auto", rp.forward_kernel(B, H, W, GW, GD, shape=shape))):
        assert which == "generic" or kern != "apply_fwd_generic"   # the shapes are chosen to reach a fast kernel

        def run(guide, j):
            with ops.kernel_override(which):
                out = ops.bilateral_slice_apply(tgrid, T(guide, dev), one_hot(dev, H, W, Cin, j), has_offset=off)
            assert ops.last_kernel() == kern, (which, ops.last_kernel(), kern)
            return N(out)

        read_back(run, codes, H, W, Cin, off, f"apply {Cin}->{Cout} offset={off} {frame} {which} [{kern}]")


#                B  H   W    GH GW  GD
ROW_FAMILY = {"apply_fwd_rows/scalar": (2, 24, 35, 8, 5, 8),       # W % 4 != 0 (mx = 7 against a grid 5 wide)
              "apply_fwd_rows/vec4": (2, 12, 320, 4, 64, 16)}      # 16 planes of a segment's columns: too much LDS for
#                                                                    the segment kernel's padded image


@pytest.mark.parametrize("kern", sorted(ROW_FAMILY))
def test_codes_apply_row_family(dev, ops, kern):
    """The two forward kernels the 16 x 16 x 8 grid never reaches under auto dispatch (3 -> 3 with offset)."""
    B_, H, W, GH, GW, GD = ROW_FAMILY[kern]
    assert B_ == B and rp.forward_kernel(B, H, W, GW, GD) == kern
    codes = cf.address_codes(B, GH, GW, GD, 12)
    tgrid = T(codes, dev)

    def run(guide, j):
        out = ops.bilateral_slice_apply(tgrid, T(guide, dev), one_hot(dev, H, W, 3, j), has_offset=True)
        assert ops.last_kernel() == kern, (ops.last_kernel(), kern)
        return N(out)

    read_back(run, codes, H, W, 3, True, f"apply 3->3 offset {H}x{W} grid {GH}x{GW}x{GD} auto [{kern}]")


@pytest.mark.parametrize("frame", sorted(FRAMES))
@pytest.mark.parametrize("C", [1, 2, 12, 16])
def test_codes_slice(dev, ops, C, frame):
    H, W = FRAMES[frame]
    GH, GW, GD = GRID
    codes = cf.address_codes(B, GH, GW, GD, C)
    tgrid = T(codes, dev)
    for which, kern in (("generic", "slice_fwd_generic"), ("auto", rp.slice_kernel(B, H, W, GW, GD, C))):
        assert which == "generic" or kern == "slice_fwd_rows"

        def run(guide, j):
            with ops.kernel_override(which):
                out = ops.bilateral_slice(tgrid, T(guide, dev))
            assert ops.last_kernel() == kern, (which, ops.last_kernel(), kern)
            return N(out)

        read_back(run, codes, H, W, 0, True, f"slice C={C} {frame} {which} [{kern}]")


# ---- (i) every other float32-out forward with a guide map: 3 -> 3 with offset --------------------------------------------
@pytest.fixture(scope="module")
def codes12(dev):
    codes = cf.address_codes(B, *GRID, 12)
    return codes, T(codes, dev)


@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_codes_row_bands(dev, ops, codes12, frame):
    """bilateral_slice_apply_rows: two bands of the frame; at 48 rows (three per grid row) the cut at row 25 lies inside
    grid row 8, so the second band starts between two cell centres and its y coordinate must come from the frame."""
    codes, tgrid = codes12
    H, W = FRAMES[frame]
    cut = 25 if H == 48 else 7
    assert H != 48 or (cut % 3 != 0 and (cut // 3) == 8)
    for which in ("generic", "auto"):
        kern = "apply_fwd_generic" if which == "generic" else "apply_fwd_seg/vec4"
        assert rp.seg_reaches(B, H, W, GRID[1], GRID[2])

        def run(guide, j):
            tguide, tin = T(guide, dev), one_hot(dev, H, W, 3, j)
            bands = []
            for a, b in ((0, cut), (cut, H)):
                with ops.kernel_override(which):
                    bands.append(ops.bilateral_slice_apply_rows(tgrid, tguide[:, a:b], tin[:, a:b], H, a, True))
                assert ops.last_kernel() == kern, (which, ops.last_kernel())
            return N(torch.cat(bands, dim=1))

        read_back(run, codes, H, W, 3, True, f"row bands {frame} cut at {cut} {which} [{kern}]")


#        dtype       white level  label
WIRE = [("float32", 1.0, "f32"), ("uint8", 255.0, "u8"), ("uint16", 65535.0, "u16"), ("uint16", 32767.0, "u16")]
#          stored channels, position of R, G, B, label suffix
ORDERS = {"rgb": (3, (0, 1, 2), ""), "bgr": (3, (2, 1, 0), "/bgr"), "rgba": (4, (0, 1, 2), "/rgba"),
          "bgra": (4, (2, 1, 0), "/bgra")}


@pytest.mark.parametrize("frame", sorted(FRAMES))
@pytest.mark.parametrize("dtype, white, label", WIRE, ids=[f"{w[0]}_{int(w[1])}" for w in WIRE])
def test_codes_wire_formats(dev, ops, codes12, dtype, white, label, frame):
    """bilateral_slice_apply_io -> float32 from float32, uint8 and uint16 frames: the one-hot is the white level, at the
    position the pixel order gives the channel (which pins the permutation); alpha, where stored, is never read."""
    codes, tgrid = codes12
    H, W = FRAMES[frame]
    assert rp.seg_reaches(B, H, W, GRID[1], GRID[2], io=True)
    for order, (stored, pos, suffix) in ORDERS.items():
        if dtype == "float32" and order != "rgb":
            continue   # float32 frames are RGB only (include/hdrnet_amd_pixel_formats.h)
        kern = f"apply_fwd_io/{label}->f32{suffix}"

        def run(guide, j):
            tin = one_hot(dev, H, W, 3, j, white, np.dtype(dtype), stored, None if j is None else pos[j],
                          alpha=(int(white) // 3 if stored == 4 else None))
            out = ops.bilateral_slice_apply_io(tgrid, tin, guide=T(guide, dev), input_white_level=white,
                                               pixel_format=order)
            assert ops.last_kernel() == kern, (ops.last_kernel(), kern)
            assert out.dtype == torch.float32 and tuple(out.shape) == (B, H, W, 3)
            return N(out)

        read_back(run, codes, H, W, 3, True, f"io {dtype} white {white:g} {order} {frame} [{kern}]")


@pytest.mark.parametrize("frame", sorted(FRAMES))
def test_codes_upadd(dev, ops, codes12, frame):
    """bilateral_slice_apply_upadd and bilateral_slice_apply_upadd_io -> float32 with a zero coarse level: the slice-apply
    term alone."""
    codes, tgrid = codes12
    H, W = FRAMES[frame]
    coarse = torch.zeros((B, 5, 7, 3), dtype=torch.float32, device=dev)
    kern = rp.fused_forward_kernel(B, H, W, GRID[1], GRID[2], "upadd")
    assert kern == "apply_fwd_seg/vec4+upadd"

    def run(guide, j):
        out = ops.bilateral_slice_apply_upadd(tgrid, one_hot(dev, H, W, 3, j), coarse, guide=T(guide, dev))
        assert ops.last_kernel() == kern, ops.last_kernel()
        return N(out)

    read_back(run, codes, H, W, 3, True, f"upadd {frame} [{kern}]")
    for dtype, white, label in WIRE:
        kern_io = kern if dtype == "float32" else f"apply_fwd_io/{label}->f32+upadd"

        def run_io(guide, j):
            tin = one_hot(dev, H, W, 3, j, white, np.dtype(dtype))
            out = ops.bilateral_slice_apply_upadd_io(tgrid, tin, coarse, guide=T(guide, dev), input_white_level=white)
            assert ops.last_kernel() == kern_io, (ops.last_kernel(), kern_io)
            assert out.dtype == torch.float32
            return N(out)

        read_back(run_io, codes, H, W, 3, True, f"upadd_io {dtype} white {white:g} {frame} [{kern_io}]")


# ---- (ii) and (iii): forward and backward through the autograd ops --------------------------------------------------------
GRAD_FRAMES = {"48x1040": (48, 1040), "64x256": (64, 256)}
GH2, GW2 = 8, 16                        # GH != GW, H != W
#            Cin Cout offset  gradients asked       fast backward
GRAD_OPS = {
    "apply_all": (3, 3, True, ("grid", "guide", "input")),    # one fused MFMA pass
    "apply_pixel": (3, 3, True, ("guide", "input")),          # apply_vjp_seg
    "slice12": (0, 12, True, ("grid", "guide")),
}


def expected_kernels(op, which, H, W, GD):
    """(forward, backward) kernel names under `which`."""
    slice_op = op == "slice12"
    if which == "generic":
        return ("slice_fwd_generic", "slice_grad_generic") if slice_op else ("apply_fwd_generic", "apply_grad_generic")
    if slice_op:
        assert rp.gg_reaches(B, H, W, GH2, GW2, GD, 12)
        return rp.slice_kernel(B, H, W, GW2, GD, 12), "slice_bwd_fused/mfma"
    fwd = rp.forward_kernel(B, H, W, GW2, GD)
    if op == "apply_all":
        return fwd, rp.grad_kernels(B, H, W, GH2, GW2, GD, True, True)
    return fwd, rp.vjp_kernel(B, H, W, GW2, GD)


def run_op(dev, ops, op, which, case, kernels):
    """The public op forward and backward on `case` under `which`; -> dict of numpy results (only the gradients asked)."""
    Cin, Cout, off, wanted = GRAD_OPS[op]
    tg = T(case["grid"], dev).requires_grad_("grid" in wanted)
    tgu = T(case["guide"], dev).requires_grad_("guide" in wanted)
    ti = T(case["inp"], dev).requires_grad_("input" in wanted) if Cin else None
    with ops.kernel_override(which):
        out = ops.bilateral_slice_apply(tg, tgu, ti, has_offset=off) if Cin else ops.bilateral_slice(tg, tgu)
        assert ops.last_kernel() == kernels[0], (op, which, ops.last_kernel(), kernels[0])
        out.backward(T(case["dout"], dev))
        assert ops.last_kernel() == kernels[1], (op, which, ops.last_kernel(), kernels[1])
    res = dict(out=N(out))
    for key, t in (("dgrid", tg), ("dguide", tgu), ("dinput", ti)):
        if t is not None and t.grad is not None:
            res[key] = N(t.grad)
    return res


def port_results(P, case, Cin, off):
    if Cin:
        out = P.bilateral_slice_apply(case["grid"], case["guide"], case["inp"], off)
        dgrid, dguide, dinput = P.bilateral_slice_apply_grad(case["grid"], case["guide"], case["inp"], case["dout"], off)
        return dict(out=out, dgrid=dgrid, dguide=dguide, dinput=dinput)
    dgrid, dguide = P.bilateral_slice_grad(case["grid"], case["guide"], case["dout"])
    return dict(out=P.bilateral_slice(case["grid"], case["guide"]), dgrid=dgrid, dguide=dguide)


def dist(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max())


@pytest.mark.parametrize("frame", sorted(GRAD_FRAMES))
@pytest.mark.parametrize("GD", [8, 16])
@pytest.mark.parametrize("op", sorted(GRAD_OPS))
@pytest.mark.parametrize("family", ["axes", "planes"])
def test_axes_and_planes(dev, ops, mt_port, family, op, GD, frame):
    Cin, Cout, off, wanted = GRAD_OPS[op]
    H, W = GRAD_FRAMES[frame]
    dims = (B, H, W, GH2, GW2, GD)
    if family == "axes":
        # (dguide under a grid constant in z is the difference of two equal taps, noise around zero: "xyz" holds it)
        cases = [(f"{axis} varies", cf.axis_case(axis, *dims, Cin, Cout, off, seed=7 + GD + k), cf.axis_expected,
                  ("dguide", "dinput") if "z" in axis else ("dinput",)) for k, axis in enumerate(("z", "x", "y", "xyz"))]
    else:   # both border planes (the far tap is clamped onto the near one) and an inner one
        cases = [(f"plane {gz}", cf.plane_case(gz, *dims, Cin, Cout, off, seed=70 + gz), cf.plane_expected, ("dinput",))
                 for gz in (0, GD // 2 - 1, GD - 1)]
    for label, case, expected, pixel_grads in cases:
        want = expected(case)
        port = port_results(mt_port, case, Cin, off)
        for which in ("auto", "generic"):
            kernels = expected_kernels(op, which, H, W, GD)
            got = run_op(dev, ops, op, which, case, kernels)
            name = f"{op} GD={GD} {frame} {label} {which} [{kernels[0]} | {kernels[1]}]"
            print(f"{name} forward: max|err| = {dist(got['out'], want['out']):.3e} (port {dist(port['out'], want['out']):.3e})")
            np.testing.assert_allclose(got["out"], want["out"], err_msg=name, **FWD_TOL)
            for what in pixel_grads:
                if what in got:
                    print(f"  port's distance: {dist(port[what], want[what]):.3e}")
                    check_pixel_grad(got[what], want[what], name, what)
            if "dgrid" in got and "dgrid" in want:
                print(f"  port's distance: {dist(port['dgrid'], want['dgrid']):.3e}")
                check_dgrid(got["dgrid"], want["dgrid"], name)
                others = np.abs(np.delete(got["dgrid"], case["gz"], axis=3)).max()
                scale = max(1.0, float(np.abs(want["dgrid"]).max()))
                print(f"  dgrid outside plane {case['gz']}: max {others:.3e} (port "
                      f"{np.abs(np.delete(port['dgrid'], case['gz'], axis=3)).max():.3e})")
                assert others <= (0.0 if which == "generic" else 1e-5 * scale), (name, others)
