"""Every CPU oracle against answers that do not pass through any of them (tests/closed_form.py).

The C99 port, oracle/_ref (the reference's .cc over this repository's stand-in array.h), the numpy twin of the JAX code
and the float64 restatements were all written from one reading of the reference's layout and sampling rules, and the
rest of the suite drives them with uniform random data: were that reading wrong -- gy and gx exchanged, c = j * Cout + i,
z counted from the other end, pixel centres at p instead of p + 0.5, mirrored borders -- they would agree with each
other and with the kernels.  Here the expected values come from the documented layout alone:

(i)   address codes read back cell by cell (test_address_codes_read_back), and the proof that this notices a permuted grid
      (test_decode_notices_a_permuted_grid);
(ii)  grids that vary along one axis (test_one_axis): centre convention, scale direction and clamp-not-mirror on each
      axis separately, the z tent and its derivative with the factor GD -- and along all three as a product, which holds
      the x and y weights of the guide derivative;
(iii) a constant guide at a plane centre with random data (test_one_plane): forward, dgrid (its other planes exactly
      zero) and dinput as matrix products.

Bars: (i) |out / PEAK - integer| < 0.25 with every decode right; (ii) / (iii) the suite's fixed bars (forward rtol = atol
= 1e-5; check_pixel_grad; check_dgrid).
"""
import numpy as np
import pytest

import closed_form as cf
from conftest import check_dgrid, check_pixel_grad

FWD_RTOL = FWD_ATOL = 1e-5   # the suite's forward bar (tests/test_gpu_parity.py)


# ---- one call surface over the four oracles ------------------------------------------------------------------------------
class _CApi:
    """The port or oracle/_ref.  Cin = 0 with offset is the slice op."""

    def __init__(self, oracle, name):
        self.o, self.name = oracle, name
        self.plane_dgrid_factor = 1.0

    def forward(self, grid, guide, inp, has_offset):
        if inp.shape[-1] == 0:
            return self.o.bilateral_slice(grid, guide)
        return self.o.bilateral_slice_apply(grid, guide, inp, has_offset)

    def grads(self, grid, guide, inp, dout, has_offset):
        if inp.shape[-1] == 0:
            dgrid, dguide = self.o.bilateral_slice_grad(grid, guide, dout)
            return dgrid, dguide, None
        return self.o.bilateral_slice_apply_grad(grid, guide, inp, dout, has_offset)


class _JaxNp:
    """oracle/jax_np.py: the slice op only (the reference's JAX code has no apply form), one image at a time.

    plane_dgrid_factor: the reference's JAX grid VJP splats a pixel's range weight to floor(gz - 0.5) and to
    ceil(gz - 0.5) (jax/bilateral_slice.py:213-252).  At a guide EXACTLY on a plane centre the two are the same plane and
    it receives the weight twice, where the C++ op (the transpose of its forward: taps floor and floor + 1) gives it
    once.  That is the reference's JAX code, not this twin's reading of it, and it concerns a set of guides of measure
    zero -- which is where family (iii) sits.  The twin is held to 2 x the closed form there: layout and weights are
    pinned all the same."""
    name, plane_dgrid_factor = "jax_np", 2.0

    def forward(self, grid, guide, inp, has_offset):
        from oracle import jax_np as J
        assert inp.shape[-1] == 0
        return J.batched(J.bilateral_slice, grid, guide)

    def grads(self, grid, guide, inp, dout, has_offset):
        from oracle import jax_np as J
        assert inp.shape[-1] == 0
        dguide = J.batched(J.bilateral_slice_guide_vjp, grid, guide, dout)
        dgrid = J.batched(J.bilateral_slice_grid_vjp, guide, dout, grid_shape=grid.shape[1:])
        return dgrid, dguide, None


class _F64:
    """oracle/f64_ops.py: the yardstick most GPU bars are measured against."""
    name, plane_dgrid_factor = "f64_ops", 1.0

    def forward(self, grid, guide, inp, has_offset):
        from oracle.f64_ops import f64_slice, f64_slice_apply
        if inp.shape[-1] == 0:
            return f64_slice(grid, guide)[0]
        return f64_slice_apply(grid, guide, inp, None, has_offset)[0]

    def grads(self, grid, guide, inp, dout, has_offset):
        from oracle.f64_ops import f64_slice, f64_slice_apply
        if inp.shape[-1] == 0:
            return f64_slice(grid, guide, dout)[1:] + (None,)
        return f64_slice_apply(grid, guide, inp, dout, has_offset)[1:]


IMPLS = ("port", "ref", "jax_np", "f64_ops")


@pytest.fixture
def impl(request, port, ref_or_none):
    """The oracle a test's `impl` parameter names (indirect); only the oracle/_ref legs can skip."""
    if request.param == "port":
        return _CApi(port, "port")
    if request.param == "ref":
        if ref_or_none is None:
            pytest.skip("oracle/_ref is not built here")
        return _CApi(ref_or_none, "ref")
    return _JaxNp() if request.param == "jax_np" else _F64()


def impl_by(ops):
    """(impl, op) pairs for `ops` {name: (.., Cin, Cout, offset)}: every oracle with every op it has -- the JAX twin has
    the slice op (Cin = 0) only."""
    return [(i, o) for i in IMPLS for o in sorted(ops) if i != "jax_np" or ops[o][-3] == 0]


def one_hot_runner(impl, grid, Cin, has_offset):
    def run(guide, j):
        inp = np.zeros(guide.shape + (Cin,), np.float32)
        if j is not None:
            inp[..., j] = 1.0
        return impl.forward(grid, guide, inp, has_offset)
    return run


# ---- (i) address codes -----------------------------------------------------------------------------------------------------
#              B  H    W    GH  GW  GD  Cin Cout offset
CODE_SHAPES = {
    "3to3_offset_48x1040": (2, 48, 1040, 16, 16, 8, 3, 3, True),
    "3to3_offset_16x16": (2, 16, 16, 16, 16, 8, 3, 3, True),      # one pixel per cell: every coordinate is exact
    "4to4_plain_40x132": (2, 40, 132, 8, 4, 16, 4, 4, False),
    "1to3_offset_48x1040": (2, 48, 1040, 16, 16, 8, 1, 3, True),
    "slice12_48x1040": (2, 48, 1040, 16, 16, 8, 0, 12, True),     # BilateralSlice: the offset column alone
    "slice5_40x132": (2, 40, 132, 8, 4, 16, 0, 5, True),
}


@pytest.mark.parametrize("impl, shape", impl_by(CODE_SHAPES), indirect=["impl"])
def test_address_codes_read_back(impl, shape):
    B, H, W, GH, GW, GD, Cin, Cout, off = CODE_SHAPES[shape]
    Cj = Cin + (1 if off else 0)
    codes = cf.address_codes(B, GH, GW, GD, Cout * Cj)
    got, dev = cf.decode(one_hot_runner(impl, codes, Cin, off), codes.shape, H, W, Cin, off)
    wrong, worst = cf.check_decode(got, dev, codes, Cj, f"{impl.name} {shape}")
    assert wrong == 0 and worst < cf.DECODE_BAR


def _permuted(codes, how, Cj):
    if how == "gy<->gx":
        return np.ascontiguousarray(codes.transpose(0, 2, 1, 3, 4))
    if how == "(Cout, Cj) transposed":
        m = cf.as_matrix(codes, Cj)
        return np.ascontiguousarray(m.swapaxes(-1, -2)).reshape(codes.shape)
    assert how == "z reversed"
    return np.ascontiguousarray(codes[:, :, :, ::-1])


@pytest.mark.parametrize("how", ["gy<->gx", "(Cout, Cj) transposed", "z reversed"])
def test_decode_notices_a_permuted_grid(port, how):
    """The pin has teeth: the port reading a grid whose codes were permuted -- what an implementation with that
    misreading of the layout would see of the true grid -- fails the decode, on the square 16 x 16 x 8 grid where every
    permutation keeps the shape."""
    B, H, W, GH, GW, GD, Cin, Cout, off = CODE_SHAPES["3to3_offset_16x16"]
    Cj = Cin + 1
    codes = cf.address_codes(B, GH, GW, GD, Cout * Cj)
    impl = _CApi(port, "port")
    got, dev = cf.decode(one_hot_runner(impl, _permuted(codes, how, Cj), Cin, off), codes.shape, H, W, Cin, off)
    wrong, worst = cf.check_decode(got, dev, codes, Cj, f"port, {how}")
    assert worst < cf.DECODE_BAR          # it still reads single entries ...
    assert wrong > got.size // 2, wrong   # ... the wrong ones


def test_axis_matrix_by_hand():
    """The matrices themselves, where they can be checked by hand: rows sum to 1, column sums are the pixels per cell (at
    the edges too: the clamped tap returns what the missing neighbour would have taken), 2 pixels per cell read
    3/4 + 1/4, and the first pixel reads the first cell alone (clamp; a mirror would give the same here, a zero
    border would not)."""
    for n, gn in ((48, 16), (1040, 16), (40, 8), (132, 4), (64, 8), (256, 16), (37, 5), (53, 7), (16, 16)):
        M = cf.axis_matrix(n, gn)
        np.testing.assert_allclose(M.sum(1), 1.0, rtol=0, atol=1e-6)
        if n % gn == 0:
            np.testing.assert_allclose(M.sum(0), n / gn, rtol=0, atol=1e-4)
    M = cf.axis_matrix(8, 4)
    want = np.zeros((8, 4))
    want[0, 0] = want[7, 3] = 1.0
    for p, (a, b) in {1: (0, 1), 2: (1, 0), 3: (1, 2), 4: (2, 1), 5: (2, 3), 6: (3, 2)}.items():
        want[p, a], want[p, b] = 0.75, 0.25
    np.testing.assert_array_equal(M, want)
    np.testing.assert_array_equal(cf.axis_matrix(5, 5), np.eye(5))
    np.testing.assert_array_equal(cf.centre_pixels(1040, 16)[:3], [32, 97, 162])


# ---- (ii) one axis at a time ---------------------------------------------------------------------------------------------
#             B  H   W     GH GW  GD
AXIS_FRAMES = {"48x1040": (2, 48, 1040, 8, 16, 8), "37x53": (1, 37, 53, 5, 7, 4)}   # GH != GW, H != W; the second: no
OPS = {"apply3to3": (3, 3, True), "apply4to2_plain": (4, 2, False), "slice12": (0, 12, True)}   # pixel on a cell centre


@pytest.mark.parametrize("impl, op", impl_by(OPS), indirect=["impl"])
@pytest.mark.parametrize("frame", sorted(AXIS_FRAMES))
@pytest.mark.parametrize("axis", ["z", "x", "y", "xyz"])
def test_one_axis(impl, axis, frame, op):
    Cin, Cout, off = OPS[op]
    case = cf.axis_case(axis, *AXIS_FRAMES[frame], Cin, Cout, off, seed=len(frame) + len(op))
    want = cf.axis_expected(case)
    name = f"{impl.name} {op} {frame} {axis}-only"
    out = impl.forward(case["grid"], case["guide"], case["inp"], off)
    print(f"{name} forward: max|err| = {np.abs(out - want['out']).max():.3e}, max|want| = {np.abs(want['out']).max():.3g}")
    np.testing.assert_allclose(out, want["out"], rtol=FWD_RTOL, atol=FWD_ATOL, err_msg=name)
    _, dguide, dinput = impl.grads(case["grid"], case["guide"], case["inp"], case["dout"], off)
    if "z" in axis:   # the z tent's derivative and its factor GD; "xyz": times the x and y weights
        check_pixel_grad(dguide, want["dguide"], name, "dguide")
    if dinput is not None:
        check_pixel_grad(dinput, want["dinput"], name, "dinput")


# ---- (iii) one plane -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("impl, op", impl_by(OPS), indirect=["impl"])
@pytest.mark.parametrize("frame", sorted(AXIS_FRAMES))
def test_one_plane(impl, frame, op):
    Cin, Cout, off = OPS[op]
    dims = AXIS_FRAMES[frame]
    GD = dims[-1]
    for gz in (0, GD // 2 - 1, GD - 1):   # both border planes (clamped far tap) and an inner one
        case = cf.plane_case(gz, *dims, Cin, Cout, off, seed=100 + gz)
        want = cf.plane_expected(case)
        name = f"{impl.name} {op} {frame} plane {gz}"
        out = impl.forward(case["grid"], case["guide"], case["inp"], off)
        print(f"{name} forward: max|err| = {np.abs(out - want['out']).max():.3e}")
        np.testing.assert_allclose(out, want["out"], rtol=FWD_RTOL, atol=FWD_ATOL, err_msg=name)
        dgrid, _, dinput = impl.grads(case["grid"], case["guide"], case["inp"], case["dout"], off)
        check_dgrid(dgrid, impl.plane_dgrid_factor * want["dgrid"], name)
        others = np.delete(dgrid, gz, axis=3)
        assert not others.any(), f"{name}: dgrid outside plane {gz} up to {np.abs(others).max():.3e}, must be exactly 0"
        if dinput is not None:
            check_pixel_grad(dinput, want["dinput"], name, "dinput")
