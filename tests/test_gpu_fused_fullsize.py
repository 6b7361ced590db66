"""The fused guide kernels -- guide network, curves guide, wire formats, pyramid up-add -- against the CPU oracle at frame
size and at the edges of the row plan (tests/test_gpu_parity.py checks them at toy sizes only).

* Frame size, 1 x 2160 x 3840 and 1 x 1080 x 1920, grid 16 x 16 x 8 x 12: rows of five / two workgroup segments
  (row_geom.h: make_row_plan), so every segment's column window, the u8 stores beside idle lanes and the
  descriptor-bounded f32 stores are compared with something.  Each family is also called once through its C-ABI entry
  point with a POISONED output (NaN for f32; 0x00 and 0xFF for u8, which must give the same bytes): the Python
  wrappers allocate with torch.empty, so an element the kernel never writes would otherwise go unseen.
* Plan edges: rows of more than 8 segments (seg_common.hip.h: no host table, column windows computed on the device),
  the row-kernel fallbacks of the fused forwards (apply_fwd_rows.hip), the knot-by-knot curves guide (> 16 knots),
  and a seeded fuzz of the fused entry points.

References are the oracle alone: oracle.pointwise_nn_guide / curves_guide / resize_bilinear_align_corners and the
port's bilateral_slice_apply, composed in float32 numpy.  Bars are those of the small tests: a guide the kernel computes
1e-6 (NN) / 2e-6 (curves); f32 output rtol = atol = 1e-5; u8 output the rule of test_wire_format_forward."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
from conftest import check_dgrid, check_pixel_grad  # noqa: E402
from row_plan import io_fits, row_plan, rows_fits, seg_fits  # noqa: E402

FWD_TOL = 1e-5
NN_GUIDE_TOL = 1e-6
CURVES_GUIDE_TOL = 2e-6
BAND_ROWS = 120  # numpy guides in row bands: curves_guide on a whole 4K frame allocates ~1.6 GB of temporaries


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from hdrnet_amd import hdrnet_ops
    return hdrnet_ops


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def port16(port):
    port.set_threads(min(16, os.cpu_count() or 1))  # the GPU hosts allow 16 CPUs per command
    yield port
    port.set_threads(1)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def T16(raw, dev):
    return torch.from_numpy(raw.astype(np.int32)).to(dev).to(torch.uint16)


def banded(fn, x, *args):
    """fn(x[:, rows], *args) over row bands of an NHWC image -> [B, H, W]."""
    return np.concatenate([fn(x[:, a:a + BAND_ROWS], *args) for a in range(0, x.shape[1], BAND_ROWS)], axis=1)


def near_identity_grid(rng, B, GH, GW, GD):
    """An affine close to the identity (test_wire_format_forward): the output spans [0, 1] and beyond."""
    g6 = np.zeros((B, GH, GW, GD, 3, 4), np.float32)
    for i in range(3):
        g6[..., i, i] = 1.0
    return (g6 + 0.15 * rng.standard_normal(g6.shape)).astype(np.float32).reshape(B, GH, GW, GD, 12)


def nn_params(rng, n, Cin=3):
    return ((rng.standard_normal((n, Cin + 1)) * 0.8).astype(np.float32),
            (rng.standard_normal(n + 1) * 0.5).astype(np.float32))


def curves_params(rng, npts):
    """ccm near the identity, npts knots spread over [0, 1) (the reference's initialisation, hdrnet/models.py:150-154)."""
    ccm = (np.concatenate([np.eye(3), np.zeros((3, 1))], 1) + 0.2 * rng.standard_normal((3, 4))).astype(np.float32)
    shifts = (np.tile(np.linspace(0, 1, npts, endpoint=False)[:, None], (1, 3))
              + 0.16 / npts * rng.standard_normal((npts, 3))).astype(np.float32)
    slopes = (0.3 * rng.standard_normal((npts, 3)) * 16 / npts).astype(np.float32)
    slopes[0] += 1.0
    return ccm, shifts, slopes, np.array([0.4, 0.35, 0.25, 0.02], np.float32)


def close(name, got, want, rtol=FWD_TOL, atol=FWD_TOL):
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / (atol + rtol * np.abs(want))).max()) if err.size else 0.0
    print(f"{name}: max|err| = {err.max():.3e}, worst / (atol {atol:g} + rtol {rtol:g} |want|) = {worst:.2f}")
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=name)


def u8_close(name, got, want_f, clip_ends=True, count=True):
    """tf.cast(255 * clip(out, 0, 1), uint8) from the oracle's float32 output: equal, except by 1 LSB where the float
    result lies within 2e-5 * 255 of a rounding boundary, on fewer than 5e-4 of the samples; both ends of the clip hit.
    (`count` = False: frames too small for the share of samples to mean anything -- the fuzz.)"""
    v = 255.0 * np.clip(want_f.astype(np.float64), 0, 1)
    want = (np.float32(255.0) * np.clip(want_f, 0, 1)).astype(np.uint8)
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    near_edge = np.abs(v - np.round(v)) < 255.0 * 2 * FWD_TOL
    off_edge = int(((diff > 0) & ~near_edge).sum())
    frac = float((diff > 0).mean())
    print(f"{name}: max|diff| = {diff.max()} LSB on {frac:.2e} of samples, {off_edge} away from a rounding edge; "
          f"worst / bar (5e-4 of samples) = {frac / 5e-4:.2f}")
    assert diff.max() <= 1, name
    assert off_edge == 0, name
    assert frac < 5e-4 or not count, name
    if clip_ends:
        assert got.min() == 0 and got.max() == 255, name  # the clip is exercised on both sides


# ---- the C-ABI entry points, called with caller-owned (poisoned) outputs -------------------------------------------
_CODE = {torch.float32: 0, torch.uint8: 1, torch.uint16: 2}


def _p(t):
    return None if t is None else t.data_ptr()


def _check(rc, what):
    from hdrnet_amd import _lib
    _lib.check(rc, what)
    torch.cuda.synchronize()


def poison(shape, dtype, dev, fill):
    return torch.full(shape, fill, dtype=dtype, device=dev)


def abi_nnguide(lib, grid, x, c1, c2, out, gout, flags=0):
    B, H, W, Cin = x.shape
    GH, GW, GD, C = grid.shape[1:]
    with torch.cuda.device(x.device):
        _check(lib.hdrnet_bilateral_slice_apply_nnguide_f32_ex(
            grid.data_ptr(), x.data_ptr(), c1.data_ptr(), c2.data_ptr(), out.data_ptr(), _p(gout),
            B, H, W, GH, GW, GD, Cin, C // (Cin + 1), 1, c1.shape[0], flags,
            torch.cuda.current_stream(x.device).cuda_stream), "nnguide_f32_ex")


def abi_io(lib, grid, x, out, white, guide=None, c1=None, c2=None, gout=None):
    B, H, W, Cin = x.shape
    GH, GW, GD, C = grid.shape[1:]
    with torch.cuda.device(x.device):
        _check(lib.hdrnet_bilateral_slice_apply_io_ex(
            grid.data_ptr(), _p(guide), x.data_ptr(), out.data_ptr(), B, H, W, GH, GW, GD, Cin, C // (Cin + 1), 1,
            _CODE[x.dtype], float(white), _CODE[out.dtype], _p(c1), _p(c2), 0 if c1 is None else c1.shape[0], _p(gout),
            0, torch.cuda.current_stream(x.device).cuda_stream), "io_ex")


def abi_io_curves(lib, grid, x, out, white, curves, prepared=None, gout=None):
    B, H, W, Cin = x.shape
    GH, GW, GD, C = grid.shape[1:]
    ccm, shifts, slopes, mix = curves
    with torch.cuda.device(x.device):
        _check(lib.hdrnet_bilateral_slice_apply_io_curves_prepared(
            grid.data_ptr(), x.data_ptr(), out.data_ptr(), B, H, W, GH, GW, GD, Cin, C // (Cin + 1), 1,
            _CODE[x.dtype], float(white), _CODE[out.dtype], ccm.data_ptr(), shifts.data_ptr(), slopes.data_ptr(),
            mix.data_ptr(), shifts.shape[0], _p(prepared), _p(gout), torch.cuda.current_stream(x.device).cuda_stream),
            "io_curves_prepared")


def abi_upadd(lib, grid, x, coarse, out, guide=None, c1=None, c2=None):
    B, H, W, Cin = x.shape
    GH, GW, GD, C = grid.shape[1:]
    with torch.cuda.device(x.device):
        _check(lib.hdrnet_bilateral_slice_apply_upadd_f32_ex(
            grid.data_ptr(), _p(guide), x.data_ptr(), coarse.data_ptr(), coarse.shape[1], coarse.shape[2],
            out.data_ptr(), B, H, W, GH, GW, GD, Cin, C // (Cin + 1), 1, _p(c1), _p(c2),
            0 if c1 is None else c1.shape[0], 0, torch.cuda.current_stream(x.device).cuda_stream), "upadd_f32_ex")


def u8_poisoned_twice(name, run, shape, dev):
    """run(out) twice, into outputs pre-filled with 0x00 and with 0xFF: every byte is written (the two agree)."""
    outs = []
    for fill in (0, 255):
        out = poison(shape, torch.uint8, dev, fill)
        run(out)
        outs.append(out)
    n_diff = int((outs[0] != outs[1]).sum())
    print(f"{name}: poisoned u8 outputs (0x00 / 0xFF) differ in {n_diff} bytes")
    assert n_diff == 0, name
    return outs[0]


def f32_poisoned(name, out, *more):
    n_nan = sum(int(torch.isnan(t).sum()) for t in (out,) + more)
    print(f"{name}: NaN left in the poisoned f32 outputs: {n_nan}")
    assert n_nan == 0, name


# ---- frame-size data, shared by the tests of one size (oracle results computed once, on demand) --------------------
SIZES = {"4K": (2160, 3840), "1080p": (1080, 1920)}
CURVE_INPUTS = {"f32->f32": ("f32", torch.float32), "u8->u8": ("u8", torch.uint8), "u16->f32": ("u16", torch.float32)}


class Frame:
    def __init__(self, H, W, port):
        rng = np.random.default_rng(H * 3 + W)
        self.H, self.W, self.port = H, W, port
        self.grid = near_identity_grid(rng, 1, 16, 16, 8)
        self.inputs = {"f32": rng.random((1, H, W, 3), dtype=np.float32),
                       "u8": rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8),
                       "u16": rng.integers(0, 32768, (1, H, W, 3), dtype=np.uint16)}
        self.white = {"f32": 1.0, "u8": 255.0, "u16": 32767.0}
        self.conv1, self.conv2 = nn_params(rng, 16)
        self.curves = curves_params(rng, 16)
        self.map = (rng.random((1, H, W), dtype=np.float32) * 1.04 - 0.02).astype(np.float32)
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def x(self, kind):  # value / white level, as the kernels read it (hdrnet/data_pipeline.py:202-232, :267-274)
        raw = self.inputs[kind]
        return raw if kind == "f32" else (raw.astype(np.float32) / np.float32(self.white[kind])).astype(np.float32)

    def t_in(self, kind, dev):
        return T16(self.inputs[kind], dev) if kind == "u16" else T(self.inputs[kind], dev)

    def nn_guide(self, kind):
        return self.memo(("nn_guide", kind), lambda: banded(oracle.pointwise_nn_guide, self.x(kind), self.conv1, self.conv2))

    def curves_guide(self, kind):
        return self.memo(("curves_guide", kind), lambda: banded(oracle.curves_guide, self.x(kind), *self.curves))

    def want(self, kind, guide):
        """The oracle's slice-apply of input `kind` with guide "nn", "curves" or "map"."""
        g = {"nn": lambda: self.nn_guide(kind), "curves": lambda: self.curves_guide(kind), "map": lambda: self.map}[guide]
        return self.memo(("want", kind, guide), lambda: self.port.bilateral_slice_apply(self.grid, g(), self.x(kind), True))


_FRAMES = {}


@pytest.fixture(scope="module")
def frames(port16):
    def get(size):
        if size not in _FRAMES:  # (the references of both sizes together: ~1.3 GB)
            _FRAMES[size] = Frame(*SIZES[size], port16)
        return _FRAMES[size]
    yield get
    _FRAMES.clear()


# ---- 1. fused forwards at frame size --------------------------------------------------------------------------------
@pytest.mark.parametrize("size", list(SIZES))
def test_nnguide_frame_size(dev, ops, lib, frames, size):
    """bilateral_slice_apply_nnguide, n = 16: exported arrays with the exact and the hardware sigmoid, the prescaled
    arrays (same bits as the exported ones), and the C-ABI call with NaN-poisoned output and guide copy."""
    F = frames(size)
    want, guide = F.want("f32", "nn"), F.nn_guide("f32")
    grid, x, c1, c2 = T(F.grid, dev), T(F.x("f32"), dev), T(F.conv1, dev), T(F.conv2, dev)
    p1, p2 = ops.guide_nn_prescale(c1, c2)
    outs = {}
    for fast in (False, True):
        out, g = ops.bilateral_slice_apply_nnguide(grid, x, c1, c2, return_guide=True, fast_sigmoid=fast)
        assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide", ops.last_kernel()
        tag = f"{size} nnguide ({'fast' if fast else 'exact'} sigmoid)"
        close(tag + " guide", N(g), guide, rtol=0, atol=NN_GUIDE_TOL)
        close(tag + " out", N(out), want)
        out_p, g_p = ops.bilateral_slice_apply_nnguide(grid, x, p1, p2, return_guide=True, fast_sigmoid=fast,
                                                       prescaled=True)
        assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide", ops.last_kernel()
        assert torch.equal(out_p, out) and torch.equal(g_p, g), tag + ": prescaled != exported"
        outs[fast] = (out, g)
    out = poison((1, F.H, F.W, 3), torch.float32, dev, float("nan"))
    g = poison((1, F.H, F.W), torch.float32, dev, float("nan"))
    abi_nnguide(lib, grid, x, c1, c2, out, g)
    assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide", ops.last_kernel()
    f32_poisoned(f"{size} nnguide C-ABI", out, g)
    assert torch.equal(out, outs[False][0]) and torch.equal(g, outs[False][1])


def test_nnguide_batch_of_4_1080p_frames(dev, ops, port16):
    """B = 4 x 1080p (config #4's frame batch) with a different grid per image."""
    rng = np.random.default_rng(404)
    B, H, W = 4, 1080, 1920
    grid = rng.random((B, 16, 16, 8, 12), dtype=np.float32)
    x = rng.random((B, H, W, 3), dtype=np.float32)
    c1, c2 = nn_params(rng, 16)
    guide = banded(oracle.pointwise_nn_guide, x, c1, c2)
    want = port16.bilateral_slice_apply(grid, guide, x, True)
    out, g = ops.bilateral_slice_apply_nnguide(T(grid, dev), T(x, dev), T(c1, dev), T(c2, dev), return_guide=True)
    assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide", ops.last_kernel()
    close("4 x 1080p nnguide guide", N(g), guide, rtol=0, atol=NN_GUIDE_TOL)
    close("4 x 1080p nnguide out", N(out), want)


def test_nnguide_one_channel_1080p(dev, ops, port16):
    """Cin = Cout = 1, n = 8 at 1080p."""
    rng = np.random.default_rng(108)
    H, W = 1080, 1920
    grid = rng.random((1, 16, 16, 8, 2), dtype=np.float32)
    x = rng.random((1, H, W, 1), dtype=np.float32)
    c1, c2 = nn_params(rng, 8, Cin=1)
    guide = banded(oracle.pointwise_nn_guide, x, c1, c2)
    want = port16.bilateral_slice_apply(grid, guide, x, True)
    out, g = ops.bilateral_slice_apply_nnguide(T(grid, dev), T(x, dev), T(c1, dev), T(c2, dev), return_guide=True)
    assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide", ops.last_kernel()
    close("1080p Cin=1 n=8 nnguide guide", N(g), guide, rtol=0, atol=NN_GUIDE_TOL)
    close("1080p Cin=1 n=8 nnguide out", N(out), want)


@pytest.mark.parametrize("size", list(SIZES))
def test_io_nnguide_u8_frame_size(dev, ops, lib, frames, size):
    """u8 input -> guide network in registers -> u8 / f32 output, exact and hardware sigmoid; the u8 -> u8 call also
    through the C-ABI into outputs poisoned with 0x00 and 0xFF and a NaN-poisoned guide copy."""
    F = frames(size)
    want, guide = F.want("u8", "nn"), F.nn_guide("u8")
    grid, raw, c1, c2 = T(F.grid, dev), F.t_in("u8", dev), T(F.conv1, dev), T(F.conv2, dev)
    for od, tag in ((torch.uint8, "u8->u8"), (torch.float32, "u8->f32")):
        for fast in (False, True):
            name = f"{size} {tag}+nnguide ({'fast' if fast else 'exact'} sigmoid)"
            out, g = ops.bilateral_slice_apply_io(grid, raw, guide_conv1=c1, guide_conv2=c2, input_white_level=255.0,
                                                  out_dtype=od, return_guide=True, fast_sigmoid=fast)
            assert ops.last_kernel() == f"apply_fwd_io/{tag}+nnguide", ops.last_kernel()
            close(name + " guide", N(g), guide, rtol=0, atol=NN_GUIDE_TOL)
            (u8_close if od == torch.uint8 else close)(name + " out", N(out), want)
    gouts = []

    def run(out):
        gout = poison((1, F.H, F.W), torch.float32, dev, float("nan"))
        abi_io(lib, grid, raw, out, 255.0, c1=c1, c2=c2, gout=gout)
        assert ops.last_kernel() == "apply_fwd_io/u8->u8+nnguide", ops.last_kernel()
        gouts.append(gout)

    out = u8_poisoned_twice(f"{size} u8->u8+nnguide C-ABI", run, (1, F.H, F.W, 3), dev)
    f32_poisoned(f"{size} u8->u8+nnguide C-ABI guide", *gouts)
    close(f"{size} u8->u8+nnguide C-ABI guide", N(gouts[0]), guide, rtol=0, atol=NN_GUIDE_TOL)
    u8_close(f"{size} u8->u8+nnguide C-ABI out", N(out), want)


@pytest.mark.parametrize("size", list(SIZES))
def test_io_guide_map_frame_size(dev, ops, lib, frames, size):
    """A guide map with the wire formats: u8 -> u8, u8 -> f32, u16 (white level 32767) -> u8; the u8 -> u8 call also
    through the C-ABI into poisoned outputs."""
    F = frames(size)
    grid, gmap = T(F.grid, dev), T(F.map, dev)
    for kind, od, tag in (("u8", torch.uint8, "u8->u8"), ("u8", torch.float32, "u8->f32"), ("u16", torch.uint8, "u16->u8")):
        want = F.want(kind, "map")
        out = ops.bilateral_slice_apply_io(grid, F.t_in(kind, dev), guide=gmap, input_white_level=F.white[kind],
                                           out_dtype=od)
        assert ops.last_kernel() == f"apply_fwd_io/{tag}", ops.last_kernel()
        (u8_close if od == torch.uint8 else close)(f"{size} {tag} guide map", N(out), want)
    raw = F.t_in("u8", dev)

    def run(out):
        abi_io(lib, grid, raw, out, 255.0, guide=gmap)
        assert ops.last_kernel() == "apply_fwd_io/u8->u8", ops.last_kernel()

    out = u8_poisoned_twice(f"{size} u8->u8 guide map C-ABI", run, (1, F.H, F.W, 3), dev)
    u8_close(f"{size} u8->u8 guide map C-ABI", N(out), F.want("u8", "map"))


@pytest.mark.parametrize("io", list(CURVE_INPUTS))
@pytest.mark.parametrize("size", list(SIZES))
def test_io_curves_frame_size(dev, ops, lib, frames, size, io):
    """The curves guide in registers, with and without the prepared cell tables; u8 -> u8 also through the C-ABI
    into poisoned outputs and a NaN-poisoned guide copy."""
    F = frames(size)
    kind, od = CURVE_INPUTS[io]
    want, guide = F.want(kind, "curves"), F.curves_guide(kind)
    grid, x = T(F.grid, dev), F.t_in(kind, dev)
    curves = tuple(T(a, dev) for a in F.curves)
    prep = ops.curves_guide_prepare(curves[1], curves[2])
    assert prep is not None  # the cells separate these knots
    check = u8_close if od == torch.uint8 else close
    for prepared, suffix in ((None, ""), (prep, "/cells")):
        name = f"{size} {io}+curvesguide{suffix}"
        out, g = ops.bilateral_slice_apply_io(grid, x, guide_curves=curves, input_white_level=F.white[kind],
                                              out_dtype=od, return_guide=True, curves_prepared=prepared)
        assert ops.last_kernel() == f"apply_fwd_io/{io}+curvesguide{suffix}", ops.last_kernel()
        close(name + " guide", N(g), guide, rtol=0, atol=CURVES_GUIDE_TOL)
        check(name + " out", N(out), want)
    if od != torch.uint8:
        return
    gouts = []

    def run(out):
        gout = poison((1, F.H, F.W), torch.float32, dev, float("nan"))
        abi_io_curves(lib, grid, x, out, F.white[kind], curves, prepared=prep, gout=gout)
        assert ops.last_kernel() == f"apply_fwd_io/{io}+curvesguide/cells", ops.last_kernel()
        gouts.append(gout)

    out = u8_poisoned_twice(f"{size} {io}+curvesguide/cells C-ABI", run, (1, F.H, F.W, 3), dev)
    f32_poisoned(f"{size} {io}+curvesguide/cells C-ABI guide", *gouts)
    close(f"{size} {io}+curvesguide/cells C-ABI guide", N(gouts[0]), guide, rtol=0, atol=CURVES_GUIDE_TOL)
    u8_close(f"{size} {io}+curvesguide/cells C-ABI out", N(out), want)


def test_pyramid_4k(dev, ops, lib, frames, port16):
    """HDRNetGaussianPyrNN's output at 4K: the levels H / 2, H / 4 of the frame from the oracle's resize (and the GPU
    resize of the same against it), the coarsest level through the fused guide network, the other two through the
    fused up-add with the guide network and with a guide map; each level's coarse input is the oracle's result for the
    level below, so that every level is checked on its own.  The finest level also through the C-ABI (NaN poison)."""
    F = frames("4K")
    H, W = F.H, F.W
    rng = np.random.default_rng(3)
    xs = [F.x("f32")]
    for lvl in (1, 2):
        want = oracle.resize_bilinear_align_corners(xs[-1], H >> lvl, W >> lvl)
        got = N(ops.resize_bilinear(T(xs[-1], dev), H >> lvl, W >> lvl))
        assert ops.last_kernel() == "resize_bilinear_ac", ops.last_kernel()
        close(f"resize {W >> (lvl - 1)}x{H >> (lvl - 1)} -> {W >> lvl}x{H >> lvl}", got, want, rtol=0, atol=5e-7)
        xs.append(want)
    grids = [F.grid, near_identity_grid(rng, 1, 16, 16, 8), near_identity_grid(rng, 1, 16, 16, 8)]
    c1, c2 = T(F.conv1, dev), T(F.conv2, dev)
    # coarsest level: slice-apply with the guide network
    g2 = banded(oracle.pointwise_nn_guide, xs[2], F.conv1, F.conv2)
    coarse = port16.bilateral_slice_apply(grids[2], g2, xs[2], True)
    got = ops.bilateral_slice_apply_nnguide(T(grids[2], dev), T(xs[2], dev), c1, c2)
    assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide", ops.last_kernel()
    close("pyramid H/4 nnguide", N(got), coarse)
    for lvl in (1, 0):
        h, w = H >> lvl, W >> lvl
        guide = F.nn_guide("f32") if lvl == 0 else banded(oracle.pointwise_nn_guide, xs[lvl], F.conv1, F.conv2)
        sliced = F.want("f32", "nn") if lvl == 0 else port16.bilateral_slice_apply(grids[lvl], guide, xs[lvl], True)
        want = sliced + oracle.resize_bilinear_align_corners(coarse, h, w)
        tg, tx, tc = T(grids[lvl], dev), T(xs[lvl], dev), T(coarse, dev)
        got = ops.bilateral_slice_apply_upadd(tg, tx, tc, guide_conv1=c1, guide_conv2=c2)
        assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide+upadd", ops.last_kernel()
        close(f"pyramid {w}x{h} nnguide+upadd", N(got), want)
        tgm = T(guide, dev)  # the same guide as a map
        got_m = ops.bilateral_slice_apply_upadd(tg, tx, tc, guide=tgm)
        assert ops.last_kernel() == "apply_fwd_seg/vec4+upadd", ops.last_kernel()
        close(f"pyramid {w}x{h} guide map+upadd", N(got_m), want)
        if lvl == 0:
            for kw, name, ref in ((dict(c1=c1, c2=c2), "apply_fwd_seg/vec4+nnguide+upadd", got),
                                  (dict(guide=tgm), "apply_fwd_seg/vec4+upadd", got_m)):
                out = poison((1, h, w, 3), torch.float32, dev, float("nan"))
                abi_upadd(lib, tg, tx, tc, out, **kw)
                assert ops.last_kernel() == name, ops.last_kernel()
                f32_poisoned(f"pyramid {name} C-ABI", out)
                assert torch.equal(out, ref)
        coarse = want


# ---- 2. plan edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [8196, 12000])
def test_rows_of_more_than_8_segments(dev, ops, lib, port16, W):
    """W = 8196 -> 11 segments of 748 px, W = 12000 -> 12 of 1000 px: past make_seg_tab's 8 (seg_common.hip.h), every
    seg-family kernel computes its column windows on the device.  The plain forward and all three gradients against
    the port, and the fused forwards against the composed oracle."""
    B, H, GH, GW, GD = 2, 8, 4, 24, 8
    assert row_plan(W)[1] > 8
    rng = np.random.default_rng(W)
    grid = near_identity_grid(rng, B, GH, GW, GD)
    x = rng.random((B, H, W, 3), dtype=np.float32)
    guide = (rng.random((B, H, W), dtype=np.float32) * 1.04 - 0.02).astype(np.float32)
    dout = rng.standard_normal((B, H, W, 3)).astype(np.float32)
    tag = f"W={W}"
    tg, tgu, tx = T(grid, dev), T(guide, dev), T(x, dev)
    close(tag + " forward", N(ops.bilateral_slice_apply(tg, tgu, tx, has_offset=True)),
          port16.bilateral_slice_apply(grid, guide, x, True))
    assert ops.last_kernel() == "apply_fwd_seg/vec4", ops.last_kernel()
    wg, wgu, wi = port16.bilateral_slice_apply_grad(grid, guide, x, dout, True)
    lg, lgu, lx = (t.clone().requires_grad_(True) for t in (tg, tgu, tx))
    ops.bilateral_slice_apply(lg, lgu, lx, has_offset=True).backward(T(dout, dev))
    assert ops.last_kernel() == "apply_bwd_fused/mfma", ops.last_kernel()
    check_dgrid(N(lg.grad), wg, tag)
    check_pixel_grad(N(lgu.grad), wgu, tag, "dguide")
    check_pixel_grad(N(lx.grad), wi, tag, "dinput")
    # guide network
    c1, c2 = nn_params(rng, 16)
    g_nn = oracle.pointwise_nn_guide(x, c1, c2)
    want_nn = port16.bilateral_slice_apply(grid, g_nn, x, True)
    out, g = ops.bilateral_slice_apply_nnguide(tg, tx, T(c1, dev), T(c2, dev), return_guide=True)
    assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide", ops.last_kernel()
    close(tag + " nnguide guide", N(g), g_nn, rtol=0, atol=NN_GUIDE_TOL)
    close(tag + " nnguide out", N(out), want_nn)
    # u8 -> u8 with a guide map, into poisoned outputs
    raw = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    x8 = (raw.astype(np.float32) / np.float32(255.0)).astype(np.float32)

    def run(o):
        abi_io(lib, tg, T(raw, dev), o, 255.0, guide=tgu)
        assert ops.last_kernel() == "apply_fwd_io/u8->u8", ops.last_kernel()

    u8_close(tag + " u8->u8 guide map", N(u8_poisoned_twice(tag + " u8->u8 C-ABI", run, (B, H, W, 3), dev)),
             port16.bilateral_slice_apply(grid, guide, x8, True))
    # f32 curves
    curves = curves_params(rng, 16)
    g_cv = oracle.curves_guide(x, *curves)
    out, g = ops.bilateral_slice_apply_io(tg, tx, guide_curves=tuple(T(a, dev) for a in curves), return_guide=True)
    assert ops.last_kernel() == "apply_fwd_io/f32->f32+curvesguide", ops.last_kernel()
    close(tag + " curves guide", N(g), g_cv, rtol=0, atol=CURVES_GUIDE_TOL)
    close(tag + " curves out", N(out), port16.bilateral_slice_apply(grid, g_cv, x, True))
    # up-add, guide network and guide map
    coarse = rng.standard_normal((B, 3, W // 3, 3)).astype(np.float32)
    up = oracle.resize_bilinear_align_corners(coarse, H, W)
    got = ops.bilateral_slice_apply_upadd(tg, tx, T(coarse, dev), guide_conv1=T(c1, dev), guide_conv2=T(c2, dev))
    assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide+upadd", ops.last_kernel()
    close(tag + " nnguide+upadd", N(got), want_nn + up)
    got = ops.bilateral_slice_apply_upadd(tg, tx, T(coarse, dev), guide=tgu)
    assert ops.last_kernel() == "apply_fwd_seg/vec4+upadd", ops.last_kernel()
    close(tag + " guide map+upadd", N(got), port16.bilateral_slice_apply(grid, guide, x, True) + up)


# GD = 16 and a fine grid: the seg kernel's LDS image ((GD + 2) planes of the window + the slabs) no longer fits in
# 64 KiB, the row kernel's (GD planes) still does.  By the restated plan: W = 256 (one 64-lane segment) for GW 70 .. 81,
# W = 1024 (one 256-lane segment) for GW 59 .. 69 -- with a guide map (one more slab column per wave) from GW 54.
FALLBACKS = [(256, 75, False), (1024, 64, False), (1024, 59, False), (1024, 58, False), (1024, 54, True),
             (1024, 53, True), (1024, 69, True)]


@pytest.mark.parametrize("W,GW,guide_map", FALLBACKS)
def test_row_kernel_fallbacks(dev, ops, port16, W, GW, guide_map):
    """apply_fwd_rows/vec4+nnguide, +nnguide+upadd and +upadd against the composed oracle, and the seg kernel just
    below the edge."""
    B, H, GH, GD = 1, 12, 8, 16
    seg = seg_fits(W, GW, GD, guide_map)
    assert rows_fits(W, GW, GD)
    rng = np.random.default_rng(W + GW)
    grid = rng.random((B, GH, GW, GD, 12), dtype=np.float32)
    x = rng.random((B, H, W, 3), dtype=np.float32)
    c1, c2 = nn_params(rng, 16)
    coarse = rng.standard_normal((B, H // 2, W // 2, 3)).astype(np.float32)
    up = oracle.resize_bilinear_align_corners(coarse, H, W)
    tg, tx, tc = T(grid, dev), T(x, dev), T(coarse, dev)
    fam = "apply_fwd_seg/vec4" if seg else "apply_fwd_rows/vec4"
    tag = f"W={W} GW={GW} GD={GD}"
    if guide_map:
        gmap = rng.random((B, H, W), dtype=np.float32)
        got = ops.bilateral_slice_apply_upadd(tg, tx, tc, guide=T(gmap, dev))
        assert ops.last_kernel() == fam + "+upadd", ops.last_kernel()
        close(f"{tag} {fam}+upadd", N(got), port16.bilateral_slice_apply(grid, gmap, x, True) + up)
        return
    g_nn = oracle.pointwise_nn_guide(x, c1, c2)
    want = port16.bilateral_slice_apply(grid, g_nn, x, True)
    out, g = ops.bilateral_slice_apply_nnguide(tg, tx, T(c1, dev), T(c2, dev), return_guide=True)
    assert ops.last_kernel() == fam + "+nnguide", ops.last_kernel()
    close(f"{tag} {fam}+nnguide guide", N(g), g_nn, rtol=0, atol=NN_GUIDE_TOL)
    close(f"{tag} {fam}+nnguide", N(out), want)
    got = ops.bilateral_slice_apply_upadd(tg, tx, tc, guide_conv1=T(c1, dev), guide_conv2=T(c2, dev))
    assert ops.last_kernel() == fam + "+nnguide+upadd", ops.last_kernel()
    close(f"{tag} {fam}+nnguide+upadd", N(got), want + up)


@pytest.mark.parametrize("npts", [17, 24, 32])
def test_curves_guide_more_than_16_knots(dev, ops, port16, npts):
    """More knots than the per-workgroup search tree holds: the knot-by-knot form (kGuideCurvesScan), f32 and u8."""
    B, H, W = 2, 16, 1920
    rng = np.random.default_rng(npts)
    grid = near_identity_grid(rng, B, 16, 16, 8)
    curves = curves_params(rng, npts)
    tc = tuple(T(a, dev) for a in curves)
    x = rng.random((B, H, W, 3), dtype=np.float32)
    guide = oracle.curves_guide(x, *curves)
    assert guide.std() > 0.05
    out, g = ops.bilateral_slice_apply_io(T(grid, dev), T(x, dev), guide_curves=tc, return_guide=True)
    assert ops.last_kernel() == "apply_fwd_io/f32->f32+curvesguide/scan", ops.last_kernel()
    close(f"{npts} knots curves guide", N(g), guide, rtol=0, atol=CURVES_GUIDE_TOL)
    close(f"{npts} knots f32->f32", N(out), port16.bilateral_slice_apply(grid, guide, x, True))
    raw = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    x8 = (raw.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    g8 = oracle.curves_guide(x8, *curves)
    out, g = ops.bilateral_slice_apply_io(T(grid, dev), T(raw, dev), guide_curves=tc, out_dtype=torch.uint8,
                                          return_guide=True)
    assert ops.last_kernel() == "apply_fwd_io/u8->u8+curvesguide/scan", ops.last_kernel()
    close(f"{npts} knots u8 curves guide", N(g), g8, rtol=0, atol=CURVES_GUIDE_TOL)
    u8_close(f"{npts} knots u8->u8", N(out), port16.bilateral_slice_apply(grid, g8, x8, True))


FUZZ_W = [4, 96, 764, 772, 1020, 1028, 1920, 2052, 3844, 8196]
FUZZ_G = [1, 2, 3, 7, 8, 16, 32]


@pytest.mark.parametrize("seed", range(4))
def test_fused_entry_points_fuzz(dev, ops, port16, seed):
    """Random frames / grids / guide-network widths / knot counts / wire formats through the fused entry points
    (bilateral_slice_apply_nnguide, _io, _upadd, _curves) against the composed oracle; the kernel each call reaches is
    predicted from the restated plan (segment kernel, row-kernel fallback) and asserted.  The f32 bar scales with GD / 8
    beyond 8 planes, as tests/test_gpu_fuzz.py's dguide bar does: the guide's float32 rounding reaches the output times
    d out / d guide, which carries a factor GD (the z tent), and the fuzz's grids are random, not near the identity."""
    rng = np.random.default_rng(7000 + seed)
    seen = {}
    done = 0
    while done < 15:
        B, H, W = int(rng.integers(1, 4)), int(rng.integers(1, 25)), int(rng.choice(FUZZ_W))
        GH, GW, GD = (int(rng.choice(FUZZ_G)) for _ in range(3))
        entry = ["nnguide", "io", "upadd", "curves"][done % 4]
        grid = rng.standard_normal((B, GH, GW, GD, 12)).astype(np.float32) * 0.5
        x = rng.random((B, H, W, 3), dtype=np.float32)
        c1, c2 = nn_params(rng, int(rng.choice([4, 5, 8, 12, 16])))
        tg, tx = T(grid, dev), T(x, dev)
        tag = f"seed {seed} {entry} B={B} H={H} W={W} grid {GH}x{GW}x{GD} n={c1.shape[0]}"
        tol = FWD_TOL * max(1.0, GD / 8)
        if entry in ("nnguide", "upadd"):
            guide_map = entry == "upadd" and bool(rng.integers(2))
            if seg_fits(W, GW, GD, guide_map):
                fam = "apply_fwd_seg/vec4"
            elif rows_fits(W, GW, GD):
                fam = "apply_fwd_rows/vec4"
            else:
                continue
            if guide_map:
                guide = rng.random((B, H, W), dtype=np.float32)
            else:
                guide = oracle.pointwise_nn_guide(x, c1, c2)
            want = port16.bilateral_slice_apply(grid, guide, x, True)
            if entry == "nnguide":
                got = ops.bilateral_slice_apply_nnguide(tg, tx, T(c1, dev), T(c2, dev))
                name = fam + "+nnguide"
            else:
                coarse = rng.standard_normal((B, int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1)), 3))
                coarse = coarse.astype(np.float32)
                want = want + oracle.resize_bilinear_align_corners(coarse, H, W)
                kw = dict(guide=T(guide, dev)) if guide_map else dict(guide_conv1=T(c1, dev), guide_conv2=T(c2, dev))
                got = ops.bilateral_slice_apply_upadd(tg, tx, T(coarse, dev), **kw)
                name = fam + ("+upadd" if guide_map else "+nnguide+upadd")
            close(tag, N(got), want, rtol=tol, atol=tol)
        else:
            if not io_fits(W, GW, GD):
                continue
            npts = int(rng.choice([1, 5, 16, 17, 32]))
            curves = curves_params(rng, npts)
            tcv = tuple(T(a, dev) for a in curves)
            scan = "/scan" if npts > 16 else ""
            if entry == "curves":
                guide = oracle.curves_guide(x, *curves)
                got = ops.bilateral_slice_apply_curves(tg, tx, *tcv)
                name = f"apply_fwd_io/f32->f32+curvesguide{scan}"
                want = port16.bilateral_slice_apply(grid, guide, x, True)
                close(tag + f" npts={npts}", N(got), want, rtol=tol, atol=tol)
            else:
                kind = ["f32", "u8", "u16"][int(rng.integers(3))]
                od = [torch.float32, torch.uint8][int(rng.integers(2))]
                src = ["map", "nn", "curves"][int(rng.integers(3))]
                if kind == "f32":
                    raw, xf, wl, t_in = x, x, 1.0, tx
                else:
                    hi = 255 if kind == "u8" else 65535
                    raw = rng.integers(0, hi + 1, (B, H, W, 3)).astype(np.uint8 if kind == "u8" else np.uint16)
                    xf = (raw.astype(np.float32) / np.float32(hi)).astype(np.float32)
                    wl, t_in = float(hi), (T(raw, dev) if kind == "u8" else T16(raw, dev))
                if src == "map":
                    guide = rng.random((B, H, W), dtype=np.float32)
                    kw = dict(guide=T(guide, dev))
                elif src == "nn":
                    guide = oracle.pointwise_nn_guide(xf, c1, c2)
                    kw = dict(guide_conv1=T(c1, dev), guide_conv2=T(c2, dev))
                else:
                    guide = oracle.curves_guide(xf, *curves)
                    kw = dict(guide_curves=tcv)
                got = ops.bilateral_slice_apply_io(tg, t_in, input_white_level=wl, out_dtype=od, **kw)
                io = f"{kind}->{'u8' if od == torch.uint8 else 'f32'}"
                name = f"apply_fwd_io/{io}" + {"map": "", "nn": "+nnguide", "curves": "+curvesguide" + scan}[src]
                want = port16.bilateral_slice_apply(grid, guide, xf, True)
                if od == torch.uint8:
                    u8_close(tag + f" {io} {src}", N(got), want, clip_ends=False, count=False)
                else:
                    close(tag + f" {io} {src}", N(got), want, rtol=tol, atol=tol)
        assert ops.last_kernel() == name, (tag, ops.last_kernel(), name)
        seen[name] = seen.get(name, 0) + 1
        done += 1
    print(f"seed {seed}: kernels reached {seen}")
