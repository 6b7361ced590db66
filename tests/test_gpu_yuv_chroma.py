"""YUV 4:2:2 / 4:4:4 surfaces on the GPU (include/hdrnet_amd_yuv_chroma.h): NV16 / P210 / P216, yuv422p..., yuv444p... through
the conversion kernels, the low-res gather, the fused wire-format forward with RGB and surface outputs, both single-level
models and the captured graphs.

1. the new conversion kernels against a float64 evaluation on the float32 constants, at test_gpu_yuv.py's 2e-6;
2. every fused RGB output == ``bilateral_slice_apply_io(grid, <new conversion>(surface), ...)``, bit for bit, guide included,
   for every kind x {float32, uint8} x the five guide forms; the surfaces have INDEPENDENT chroma in every row (4:2:2) and
   every pixel (4:4:4), and ``last_kernel()`` must carry the new label;
3. a 4:2:2 / 4:4:4 surface that replicates a 4:2:0 one gives the bits of the existing 4:2:0 path (conversion, gather,
   forward), and the Y plane of a surface output equals the 4:2:0 output's;
4. planar == semi-planar for 4:2:2 on the same codes (10-bit shifted by 6 under the P010-style constants);
5. ``chroma = 420`` through the new entry points == the existing entry points, with the existing kernel names;
6. the low-res gather == ``data.lowres_input`` of the converted frame;
7. surface outputs against the float64 encoder of the header's rule on the float32 RGB output of item 2: decided samples
   equal, no sample off by more than one code, the undecided share below 1 % -- asserted on the reference alone, first;
8. the models' ``process_yuv`` / ``process_yuv_planar`` == the ops composed by hand; graph replays == the eager call.

Shapes, grid 16 x 16 x 8: (2, 5, 1040) -- two segments, the second partial, odd H, a second image -- (1, 3, 96) and (1, 3,
100), whose tight uint8 4:2:2 chroma rows are 50 bytes; ``interior`` and ``many_seg`` of tests/wire_geometry_cases.py with one
guide form each.  Layouts: tight, pitch + 64 bytes, all planes in one allocation; outputs land in buffers pre-filled with
0xA5 and with 0x5A, padding and 4096 guard bytes included."""
import numpy as np
import pytest
import torch

import u16_out_cases as uc
import wire_geometry_cases as wg
import yuv_chroma_cases as cc
import yuv_planar_cases as pc
from row_plan import row_plan

pytestmark = pytest.mark.gpu

GRID = (16, 16, 8)
SHAPES = [(2, 5, 1040), (1, 3, 96), (1, 3, 100)]
# kind -> (planar?, chroma, bits, standard, full range, kernel label)
KINDS = {"nv16": (False, "422", 8, "bt709", False, "nv16"), "p210": (False, "422", 10, "bt2020", False, "p216"),
         "p216": (False, "422", 16, "bt601", True, "p216"), "yuv422p": (True, "422", 8, "bt709", False, "i422"),
         "yuv422p10le": (True, "422", 10, "bt2020", False, "i216"), "yuv444p": (True, "444", 8, "bt709", False, "i444"),
         "yuv444p10le": (True, "444", 10, "bt709", False, "i416"), "yuv444p16le": (True, "444", 16, "bt601", True, "i416")}
GUIDES = ["map", "nn", "curves", "cells", "scan"]
GUIDE_LABEL = {"map": "", "nn": "+nnguide", "curves": "+curvesguide", "cells": "+curvesguide/cells",
               "scan": "+curvesguide/scan"}
SHORT = {"uint8": "u8", "float32": "f32"}
GEOMETRY_GUIDES = [("interior", "nn"), ("many_seg", "cells")]
# surface outputs: (kind in, bits out); a semi-planar uint8 surface comes from either sample width
SURFACE_PAIRS = [("nv16", 8), ("p216", 8), ("p210", 10), ("yuv422p", 8), ("yuv422p10le", 10), ("yuv444p", 8), ("yuv444p10le", 10)]
DEEP_PAIRS = [("p216", 16), ("yuv444p16le", 16)]


def test_the_shapes_are_what_the_comment_says():
    assert row_plan(1040) == (192, 2, 520) and row_plan(96) == (64, 1, 96) and row_plan(100) == (64, 1, 100)
    assert (100 // 2) % 4 == 2 and all(s[1] % 2 == 1 for s in SHAPES)
    for geo, _ in GEOMETRY_GUIDES:
        (B, H, W), _ = wg.GEOMETRIES[geo]
        assert B * H * W <= 1 * 40 * 2052


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from hdrnet_amd import hdrnet_ops
    return hdrnet_ops


def T(a, dev):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)
    return torch.from_numpy(a).to(dev)


def N(t):
    if t.dtype == torch.uint16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.detach().cpu().numpy()


def shift_of(kind):
    planar, _, bits = KINDS[kind][:3]
    return 0 if planar or bits == 8 else 16 - bits


def constants(kind, dev, out_bits=None):
    """``(to_rgb in numpy on the codes in the LOW bits, to_rgb of the surface as stored on the device, from_rgb in code
    units of out_bits on the device)``."""
    from hdrnet_amd import yuv
    planar, _, bits, standard, full, _ = KINDS[kind]
    low = yuv.yuv_coefficients(standard, full, bits, msb_aligned=False)[0]
    stored = low if planar else yuv.yuv_coefficients(standard, full, bits)[0]
    return low, T(stored, dev), T(yuv.yuv_encode_coefficients(standard, full, out_bits or bits), dev)


_CASES, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _CASES.clear()
    _REFS.clear()


def extents(where):
    return wg.GEOMETRIES[where] if isinstance(where, str) else (where, GRID)


def case(where, kind):
    """Grid, guide parameters and ONE content per (shape or geometry, chroma, bits): ``codes`` = (y, u, v) in the low bits.
    Kinds of one layout and depth share it (NV16 and yuv422p, P210 and yuv422p10le: item 4)."""
    _, chroma, bits = KINDS[kind][:3]
    key = (where, chroma, bits)
    if key not in _CASES:
        shape, grid = extents(where)
        rng = np.random.default_rng([83, *shape, int(chroma), bits])
        c = wg.guides(rng, shape, grid)
        c["codes"] = cc.random_planar(rng, shape, bits, chroma)
        _CASES[key] = c
    return _CASES[key]


def stored(kind, codes):
    """The planes of the kind's container as it stores them: (y, u, v), or (y, uv) with uint16 codes in the high bits."""
    planar, _, bits = KINDS[kind][:3]
    return tuple(codes) if planar else cc.semi(*codes, bits)


def device_planes(bufs, specs, dev):
    flats = [T(b, dev) for b in bufs]
    return flats, tuple(flats[i].as_strided(shape, strides, off) for i, off, shape, strides in specs)


def planes_in(kind, codes, layout, dev):
    return device_planes(*cc.lay(stored(kind, codes), layout), dev)[1]


def convert(ops, kind, planes, k):
    planar, chroma = KINDS[kind][:2]
    return (ops.yuv_planar_to_rgb if planar else ops.yuv_to_rgb)(*planes, k, chroma=chroma)


def forward(ops, kind, grid, planes, k, **kw):
    planar, chroma = KINDS[kind][:2]
    return (ops.bilateral_slice_apply_io_yuv_planar if planar else ops.bilateral_slice_apply_io_yuv)(grid, *planes, k, chroma=chroma, **kw)


def forward_surface(ops, kind, out_bits, grid, planes, k, k_out, **kw):
    """The surface output of ``out_bits`` of the kind's container; returns the op's result."""
    planar, chroma = KINDS[kind][:2]
    if planar:
        return ops.bilateral_slice_apply_io_yuv_planar(grid, *planes, k, out="planar", from_rgb=k_out, out_bits=out_bits,
                                                       chroma=chroma, **kw)
    if out_bits == 8:
        return ops.bilateral_slice_apply_io_yuv(grid, *planes, k, out="nv16", from_rgb=k_out, chroma=chroma, **kw)
    return ops.bilateral_slice_apply_io_yuv_deep(grid, *planes, k, from_rgb=k_out, out_bits=out_bits, chroma=chroma, **kw)


def surface_label(kind, out_bits):
    planar, label = KINDS[kind][0], KINDS[kind][5]
    return label if planar else ("nv16" if out_bits == 8 else "p216")


def guide_kw(ops, c, guide, dev):
    if guide == "map":
        return dict(guide=T(c["guide"], dev))
    if guide == "nn":
        return dict(guide_conv1=T(c["conv1"], dev), guide_conv2=T(c["conv2"], dev), return_guide=True)
    curves = tuple(T(a, dev) for a in wg.curves_of(c, guide))
    kw = dict(guide_curves=curves, return_guide=True)
    if guide == "cells":
        kw["curves_prepared"] = ops.curves_guide_prepare(curves[1], curves[2])
        assert kw["curves_prepared"] is not None, "the case's knots are apart: the cell tables are usable"
    return kw


def assert_same(got, want, what):
    same = np.array_equal(got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else np.array_equal(got, want)
    if not same:
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} samples differ, first at {bad[0]}: got "
                             f"{got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


def rgb_reference(ops, dev, where, kind, out, guide):
    """``bilateral_slice_apply_io`` on the float32 frame the NEW conversion kernel writes, once per case: (frame, guide)."""
    key = (where, kind, out, guide)
    if key not in _REFS:
        c = case(where, kind)
        _, k, _ = constants(kind, dev)
        frame = convert(ops, kind, planes_in(kind, c["codes"], "tight", dev), k)
        got = ops.bilateral_slice_apply_io(T(c["grid"], dev), frame, out_dtype=getattr(torch, out), **guide_kw(ops, c, guide, dev))
        assert ops.last_kernel() == f"apply_fwd_io/f32->{SHORT[out]}{GUIDE_LABEL[guide]}"
        o, g = got if guide != "map" else (got, None)
        _REFS[key] = (N(o), None if g is None else N(g))
    return _REFS[key]


# ---- 1. the conversion against float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_conversion_against_float64(dev, ops, kind):
    """atol 2e-6 (test_gpu_yuv.py::test_yuv_to_rgb): three fused operations on magnitudes below 4, each within half an ulp
    <= 2.4e-7, on the same float32 constants.  The corners hold super-black and super-white codes: both sides of the clamp."""
    planar, chroma, bits = KINDS[kind][:3]
    low, k, _ = constants(kind, dev)
    name = {(False, "422"): "yuv_422_to_rgb", (True, "422"): "yuv_planar_422_to_rgb", (True, "444"): "yuv_planar_444_to_rgb"}
    for shape in SHAPES:
        c = case(shape, kind)
        want = cc.to_rgb64(*c["codes"], chroma, low)
        assert want.min() == 0.0 and want.max() == 1.0
        for layout in cc.LAYOUTS:
            got = convert(ops, kind, planes_in(kind, c["codes"], layout, dev), k)
            assert ops.last_kernel() == name[planar, chroma] and tuple(got.shape) == shape + (3,) and got.dtype == torch.float32
            g = N(got)
            print(f"conversion {kind} {shape} {layout}: max |err| = {np.abs(g - want).max():.3g}")
            np.testing.assert_allclose(g, want, rtol=0, atol=2e-6)
            if layout == "tight":
                tight = g
            else:
                assert_same(g, tight, f"{kind} {shape} {layout} against the tight planes")


# ---- 2. the fused forward to float32 and uint8 RGB ----------------------------------------------------------------------------
def _rgb_forward(dev, ops, where, kind, out, guide, layouts):
    _, k, _ = constants(kind, dev)
    c = case(where, kind)
    shape, _ = extents(where)
    want, want_guide = rgb_reference(ops, dev, where, kind, out, guide)
    for layout in layouts:
        got = forward(ops, kind, T(c["grid"], dev), planes_in(kind, c["codes"], layout, dev), k, out="rgb",
                      out_dtype=getattr(torch, out), **guide_kw(ops, c, guide, dev))
        assert ops.last_kernel() == f"apply_fwd_io/{KINDS[kind][5]}->{SHORT[out]}{GUIDE_LABEL[guide]}"
        o, g = got if want_guide is not None else (got, None)
        assert tuple(o.shape) == shape + (3,) and o.dtype == getattr(torch, out)
        assert_same(N(o), want, f"{where} {kind} {layout} -> {out} {guide}")
        if want_guide is not None:
            assert_same(N(g), want_guide, f"{where} {kind} {layout} {guide}: the guide the kernel computed")


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("out", ["uint8", "float32"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_rgb_outputs_are_exact(dev, ops, kind, out, guide):
    for shape in SHAPES:
        _rgb_forward(dev, ops, shape, kind, out, guide, cc.LAYOUTS)


# ---- 3. replication identities --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10, 16])
def test_replicated_420_gives_the_bits_of_the_420_path(dev, ops, bits):
    from hdrnet_amd import data, yuv
    shape = (2, 6, 1040)
    rng = np.random.default_rng([89, bits])
    c = wg.guides(rng, shape, GRID)
    (y, u, v), (ys, uvs) = pc.random_planar(rng, shape, bits)
    k_low = T(yuv.yuv_coefficients("bt709", False, bits, msb_aligned=False)[0], dev)
    k_semi = T(yuv.yuv_coefficients("bt709", False, bits)[0], dev)
    k_out = T(yuv.yuv_encode_coefficients("bt709", False, bits), dev)
    grid = T(c["grid"], dev)
    nn = dict(guide_conv1=T(c["conv1"], dev), guide_conv2=T(c["conv2"], dev), return_guide=True)
    p0 = tuple(T(a, dev) for a in (y, u, v))
    want_rgb = ops.yuv_planar_to_rgb(*p0, k_low)
    want_low = data.lowres_input_yuv_planar(*p0, k_low, 6)
    want_fwd, want_g = ops.bilateral_slice_apply_io_yuv_planar(grid, *p0, k_low, **nn)
    want_surf = ops.bilateral_slice_apply_io_yuv_planar(grid, *p0, k_low, guide=T(c["guide"], dev), out="planar", from_rgb=k_out,
                                                        out_bits=bits)
    assert ops.last_kernel() == ("apply_fwd_io/i420->i420" if bits == 8 else "apply_fwd_io/i016->i016")
    surfaces = [(True, ch, tuple(T(a, dev) for a in cc.from_420(y, u, v, ch))) for ch in cc.CHROMAS]
    surfaces.append((False, "422", (T(ys, dev), T(uvs.repeat(2, axis=1), dev))))  # NV12 / P010 / P016 rows stored twice
    for planar, ch, p in surfaces:
        conv, gather, fwd = ((ops.yuv_planar_to_rgb, data.lowres_input_yuv_planar, ops.bilateral_slice_apply_io_yuv_planar)
                             if planar else (ops.yuv_to_rgb, data.lowres_input_yuv, ops.bilateral_slice_apply_io_yuv))
        k = k_low if planar else k_semi
        what = f"{'planar' if planar else 'semi-planar'} {ch} {bits}"
        assert torch.equal(conv(*p, k, chroma=ch).view(torch.int32), want_rgb.view(torch.int32)), what
        assert "420" not in ops.last_kernel() and ops.last_kernel() != "yuv_to_rgb"
        assert torch.equal(gather(*p, k, 6, chroma=ch).view(torch.int32), want_low.view(torch.int32)), what
        o, g = fwd(grid, *p, k, chroma=ch, **nn)
        assert torch.equal(o.view(torch.int32), want_fwd.view(torch.int32)) and torch.equal(g.view(torch.int32), want_g.view(torch.int32)), what
        # a surface out of such an input: the Y plane is the 4:2:0 output's, exactly
        if planar:
            surf = fwd(grid, *p, k, chroma=ch, guide=T(c["guide"], dev), out="planar", from_rgb=k_out, out_bits=bits)
            assert torch.equal(surf[0], want_surf[0]), what
        elif bits == 8:
            surf = fwd(grid, *p, k, chroma=ch, guide=T(c["guide"], dev), out="nv16", from_rgb=k_out)
            assert torch.equal(surf[0], want_surf[0]), what
        else:
            surf = ops.bilateral_slice_apply_io_yuv_deep(grid, *p, k, chroma=ch, guide=T(c["guide"], dev), from_rgb=k_out, out_bits=bits)
            assert np.array_equal(N(surf[0]) >> (16 - bits), N(want_surf[0])), what


# ---- 4. planar == semi-planar for 4:2:2 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [("yuv422p", "nv16", 8), ("yuv422p10le", "p210", 10)])
@pytest.mark.parametrize("guide", ["map", "nn"])
def test_planar_equals_semi_planar_422(dev, ops, pair, guide):
    planar_kind, semi_kind, bits = pair
    sh = shift_of(semi_kind)
    for shape in SHAPES:
        c = case(shape, planar_kind)
        assert c is case(shape, semi_kind)  # the same codes
        grid = T(c["grid"], dev)
        res = {}
        for kind in (planar_kind, semi_kind):
            _, k, k_out = constants(kind, dev)
            p = planes_in(kind, c["codes"], "tight", dev)
            rgb = forward(ops, kind, grid, p, k, **guide_kw(ops, c, guide, dev))
            surf = forward_surface(ops, kind, bits, grid, p, k, k_out, **guide_kw(ops, c, guide, dev))
            assert ops.last_kernel() == f"apply_fwd_io/{KINDS[kind][5]}->{surface_label(kind, bits)}{GUIDE_LABEL[guide]}"
            res[kind] = ((rgb[0] if guide != "map" else rgb), (surf[0] if guide != "map" else surf))
        assert_same(N(res[planar_kind][0]), N(res[semi_kind][0]), f"{pair} {shape} {guide}: RGB")
        py, pu, pv = (N(t) for t in res[planar_kind][1])
        sy, suv = (N(t) for t in res[semi_kind][1])
        assert not (sy & ((1 << sh) - 1)).any() and not (suv & ((1 << sh) - 1)).any()
        su, sv = pc.split(suv >> sh)
        for name, a, b in zip("YUV", (py, pu, pv), (sy >> sh, su, sv)):
            assert_same(a, b, f"{pair} {shape} {guide}: plane {name}")


# ---- 5. chroma = 420 through the new entry points -------------------------------------------------------------------------------
def test_chroma_420_is_the_existing_entry_points(dev, ops):
    from hdrnet_amd import _lib, data, yuv
    lib = _lib.load()
    shape = B, H, W = (2, 6, 1040)
    rng = np.random.default_rng(97)
    c = wg.guides(rng, shape, GRID)
    (y, u, v), (ys, uvs) = pc.random_planar(rng, shape, 16)
    kp = T(yuv.yuv_coefficients("bt709", False, 16, msb_aligned=False)[0], dev)
    ko = T(yuv.yuv_encode_coefficients("bt709", False, 16), dev)
    grid, c1, c2 = T(c["grid"], dev), T(c["conv1"], dev), T(c["conv2"], dev)
    curves = tuple(T(a, dev) for a in wg.curves_of(c, "curves"))
    P = tuple(T(a, dev) for a in (y, u, v))
    S = (T(ys, dev), T(uvs, dev))
    psurf = (*(t.data_ptr() for t in P), 2, 2 * W, W, W, 2 * H * W, H * W // 2, H * W // 2)
    ssurf = (*(t.data_ptr() for t in S), 2, 2 * W, 2 * W, 2 * H * W, H * W)
    stream = torch.cuda.current_stream(dev).cuda_stream
    shape6 = (*GRID, 3, 3, 1)

    def new(n, dt=torch.float32):
        return torch.zeros(n, dtype=dt, device=dev)

    # conversions and gathers
    rgb = new(shape + (3,))
    _lib.check(lib.hdrnet_yuv_planar_chroma_to_rgb_f32(*psurf, 0, B, H, W, kp.data_ptr(), rgb.data_ptr(), stream), "t")
    assert ops.last_kernel() == "yuv_planar_to_rgb" and torch.equal(rgb, ops.yuv_planar_to_rgb(*P, kp))
    rgb2 = new(shape + (3,))
    _lib.check(lib.hdrnet_yuv_chroma_to_rgb_f32(*ssurf, 0, B, H, W, kp.data_ptr(), rgb2.data_ptr(), stream), "t")
    assert ops.last_kernel() == "yuv_to_rgb" and torch.equal(rgb2, ops.yuv_to_rgb(*S, kp))
    low = new((B, 6, 6, 3))
    _lib.check(lib.hdrnet_lowres_input_yuv_planar_chroma(*psurf, 0, B, H, W, kp.data_ptr(), low.data_ptr(), 6, stream), "t")
    assert torch.equal(low, data.lowres_input_yuv_planar(*P, kp, 6))
    low2 = new((B, 6, 6, 3))
    _lib.check(lib.hdrnet_lowres_input_yuv_chroma(*ssurf, 0, B, H, W, kp.data_ptr(), low2.data_ptr(), 6, stream), "t")
    assert torch.equal(low2, data.lowres_input_yuv(*S, kp, 6))
    # the guide network: planar -> planar (surface_u16), semi-planar -> P016 and -> NV12
    oy, ou, ov = new(shape, torch.uint16), new((B, H // 2, W // 2), torch.uint16), new((B, H // 2, W // 2), torch.uint16)
    _lib.check(lib.hdrnet_bilateral_slice_apply_io_yuv_planar_chroma(
        grid.data_ptr(), None, *psurf, 0, B, H, W, kp.data_ptr(), *shape6, c1.data_ptr(), c2.data_ptr(), 16, None, 0,
        3, oy.data_ptr(), ou.data_ptr(), ov.data_ptr(), *psurf[4:], ko.data_ptr(), 16, stream), "t")
    assert ops.last_kernel() == "apply_fwd_io/i016->i016+nnguide"
    want = ops.bilateral_slice_apply_io_yuv_planar(grid, *P, kp, guide_conv1=c1, guide_conv2=c2, out="planar", from_rgb=ko, out_bits=16)
    assert all(torch.equal(a, b) for a, b in zip((oy, ou, ov), want))
    sy, suv = new(shape, torch.uint16), new((B, H // 2, W), torch.uint16)
    _lib.check(lib.hdrnet_bilateral_slice_apply_io_yuv_chroma(
        grid.data_ptr(), None, *ssurf, 0, B, H, W, kp.data_ptr(), *shape6, c1.data_ptr(), c2.data_ptr(), 16, None, 0,
        3, sy.data_ptr(), suv.data_ptr(), *ssurf[3:], ko.data_ptr(), 16, stream), "t")
    assert ops.last_kernel() == "apply_fwd_io/p016->p016+nnguide"
    want = ops.bilateral_slice_apply_io_yuv_deep(grid, *S, kp, guide_conv1=c1, guide_conv2=c2, from_rgb=ko, out_bits=16)
    assert torch.equal(sy, want[0]) and torch.equal(suv, want[1])
    k8 = T(yuv.yuv_encode_coefficients("bt709", False, 8), dev)
    ny, nuv = new(shape, torch.uint8), new((B, H // 2, W), torch.uint8)
    _lib.check(lib.hdrnet_bilateral_slice_apply_io_yuv_chroma(
        grid.data_ptr(), None, *ssurf, 0, B, H, W, kp.data_ptr(), *shape6, c1.data_ptr(), c2.data_ptr(), 16, None, 0,
        2, ny.data_ptr(), nuv.data_ptr(), W, W, H * W, H * W // 2, k8.data_ptr(), 0, stream), "t")
    assert ops.last_kernel() == "apply_fwd_io/p016->nv12+nnguide"
    want = ops.bilateral_slice_apply_io_yuv(grid, *S, kp, guide_conv1=c1, guide_conv2=c2, out="nv12", from_rgb=k8)
    assert torch.equal(ny, want[0]) and torch.equal(nuv, want[1])
    # the curves guide: planar -> float32 RGB, semi-planar -> uint8 RGB
    f = new(shape + (3,))
    _lib.check(lib.hdrnet_bilateral_slice_apply_io_curves_yuv_planar_chroma(
        grid.data_ptr(), *psurf, 0, B, H, W, kp.data_ptr(), *shape6, *(t.data_ptr() for t in curves), 16, None, None,
        0, f.data_ptr(), None, None, 0, 0, 0, 0, 0, 0, None, 0, stream), "t")
    assert ops.last_kernel() == "apply_fwd_io/i016->f32+curvesguide"
    assert torch.equal(f, ops.bilateral_slice_apply_io_yuv_planar(grid, *P, kp, guide_curves=curves))
    q = new(shape + (3,), torch.uint8)
    _lib.check(lib.hdrnet_bilateral_slice_apply_io_curves_yuv_chroma(
        grid.data_ptr(), *ssurf, 0, B, H, W, kp.data_ptr(), *shape6, *(t.data_ptr() for t in curves), 16, None, None,
        1, q.data_ptr(), None, 0, 0, 0, 0, None, 0, stream), "t")
    assert ops.last_kernel() == "apply_fwd_io/p016->u8+curvesguide"
    assert torch.equal(q, ops.bilateral_slice_apply_io_yuv(grid, *S, kp, guide_curves=curves, out_dtype=torch.uint8))


# ---- 6. the low-res gather --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 6, 5])  # 256 and 6: the vector store (n * n % 4 == 0); 5: the scalar tail
@pytest.mark.parametrize("kind", ["nv16", "p210", "yuv422p10le", "yuv444p", "yuv444p16le"])
def test_lowres_gather(dev, ops, kind, n):
    from hdrnet_amd import _lib, data
    planar, chroma, bits = KINDS[kind][:3]
    _, k, _ = constants(kind, dev)
    shape = (2, 37, 52)
    codes = cc.random_planar(np.random.default_rng([101, n, bits]), shape, bits, chroma)
    gather = data.lowres_input_yuv_planar if planar else data.lowres_input_yuv
    want = data.lowres_input(convert(ops, kind, planes_in(kind, codes, "tight", dev), k), n)
    for layout in ("pitch64", "one_allocation"):
        got = gather(*planes_in(kind, codes, layout, dev), k, n, chroma=chroma)
        assert _lib.last_kernel() == "sample_prep" and tuple(got.shape) == (2, n, n, 3)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (kind, layout)
    assert len(torch.unique(got)) > 8


# ---- 7. surface outputs against the rule ------------------------------------------------------------------------------------------
def _surface_reference(ops, dev, where, kind, out_bits, guide):
    """The float64 encoder on the float32 RGB output of item 2 (the fused kernel's, held exact there): codes, decided."""
    key = (where, kind, out_bits, guide, "surface")
    if key not in _REFS:
        c = case(where, kind)
        _, k, _ = constants(kind, dev)
        from hdrnet_amd import yuv
        _, chroma, _, standard, full, _ = KINDS[kind]
        kw = {a: b for a, b in guide_kw(ops, c, guide, dev).items() if a != "return_guide"}
        rgb = N(forward(ops, kind, T(c["grid"], dev), planes_in(kind, c["codes"], "tight", dev), k, **kw))
        codes, pre = cc.encode64(rgb, yuv.yuv_encode_coefficients(standard, full, out_bits), out_bits, chroma)
        _REFS[key] = (codes, tuple(cc.decided(p, out_bits) for p in pre))
    return _REFS[key]


def _check_surface(dev, ops, wheres, kind, out_bits, guide, layouts, cap):
    planar, chroma = KINDS[kind][:2]
    _, k, k_out = constants(kind, dev, out_bits)
    sh = 0 if planar or out_bits == 8 else 16 - out_bits
    dt = np.uint8 if out_bits == 8 else np.uint16
    refs = {w: _surface_reference(ops, dev, w, kind, out_bits, guide) for w in wheres}
    # the condition, on the reference alone and before any output is looked at
    undecided = sum(int((~d).sum()) for _, dec in refs.values() for d in dec)
    total = sum(d.size for _, dec in refs.values() for d in dec)
    print(f"surface {kind} -> {out_bits} bit {guide}: undecided {undecided} of {total} = {undecided / total:.4%}")
    assert cap(undecided, total), (kind, out_bits, undecided, total)
    for where in wheres:
        c = case(where, kind)
        shape, _ = extents(where)
        (wy, wu, wv), (dy, du, dv) = refs[where]
        assert where != SHAPES[0] or (len(np.unique(wy)) > 100 and len(np.unique(wu)) > 50)  # a picture, not a constant
        want = (wy, wu, wv) if planar else (wy, pc.interleave(wu, wv))
        dec = (dy, du, dv) if planar else (dy, pc.interleave(du.astype(np.uint8), dv.astype(np.uint8)).astype(bool))
        blank = tuple(np.zeros(w.shape, dt) for w in want)
        for layout in layouts:
            for fill in cc.FILLS:
                bufs, specs = cc.lay(blank, layout, fill)
                for spec in specs:  # the planes themselves start out as the fill too: a sample never written shows
                    pc.plane(bufs, spec)[...] = pc.fill_value(dt, fill)
                flats, outs = device_planes(bufs, specs, dev)
                kw = {a: b for a, b in guide_kw(ops, c, guide, dev).items() if a != "return_guide"}
                res = forward_surface(ops, kind, out_bits, T(c["grid"], dev), planes_in(kind, c["codes"], layout, dev), k, k_out,
                                      out_planes=outs, **kw)
                assert ops.last_kernel() == f"apply_fwd_io/{KINDS[kind][5]}->{surface_label(kind, out_bits)}{GUIDE_LABEL[guide]}"
                assert len(res) == len(outs) and all(r.data_ptr() == o.data_ptr() for r, o in zip(res, outs))
                for name, plane, ref, d in zip("YUV" if planar else ("Y", "UV"), outs, want, dec):
                    got = N(plane)
                    assert not (got & ((1 << sh) - 1)).any(), f"{kind} plane {name}: low bits set"
                    diff = np.abs((got >> sh).astype(np.int64) - ref.astype(np.int64))
                    what = f"{where} {kind} -> {out_bits} {layout} fill {fill:#x} {guide}: plane {name}"
                    assert diff.max() <= 1, f"{what}: off by {diff.max()} codes"
                    assert not diff[d].any(), f"{what}: {int((diff[d] != 0).sum())} decided samples differ"
                for flat, mask in zip(flats, pc.outside_planes(bufs, specs)):
                    assert (N(flat)[mask] == pc.fill_value(dt, fill)).all(), f"{where} {kind} {layout}: a store left the planes"


def _one_percent(undecided, total):
    return undecided < 0.01 * total


@pytest.mark.parametrize("guide", ["map", "nn"])
@pytest.mark.parametrize("kind,out_bits", SURFACE_PAIRS)
def test_surface_outputs(dev, ops, kind, out_bits, guide):
    """8- and 10-bit codes.  The case is the kind's three shapes together (some 2 x 10^4 samples): the expected undecided
    share is 2 eps per code, 0.2 % at 8 bits and 0.8 % at 10, less where the clamp decides."""
    _check_surface(dev, ops, SHAPES, kind, out_bits, guide, cc.LAYOUTS, _one_percent)


@pytest.mark.parametrize("kind,out_bits", DEEP_PAIRS)
def test_surface_outputs_16_bit(dev, ops, kind, out_bits):
    """16-bit codes (P216, yuv444p16le).  u16_out_cases.eps_of(16) is 0.256 of a code -- float32 resolves no more of a
    16-bit code after three fused operations -- so about half of all samples are undecided BY CONSTRUCTION and the 1 %
    condition of the 8- and 10-bit cases cannot hold for any input.  The condition here is the one test_p016_output has for
    this depth (wire_geometry_cases.within_cap: at least 40 % decided), on the reference alone and first; decided samples
    equal and no sample off by more than one code are asserted as above."""
    _check_surface(dev, ops, SHAPES, kind, out_bits, "nn", cc.LAYOUTS, lambda u, t: wg.within_cap(16, u, t))


@pytest.mark.parametrize("geo,guide", GEOMETRY_GUIDES)
def test_geometries(dev, ops, geo, guide):
    """An interior segment (cmin > 0, a right neighbour) over 40 rows; 11 segments with the column windows computed on the
    device, odd grid extents.  RGB exact, surfaces against the rule."""
    for kind, out_bits in (("nv16", 8), ("yuv422p10le", 10), ("yuv444p", 8)):
        _rgb_forward(dev, ops, geo, kind, "float32", guide, ("tight",))
        _check_surface(dev, ops, [geo], kind, out_bits, guide, ("tight", "pitch64"), _one_percent)
    _rgb_forward(dev, ops, geo, "p216", "uint8", guide, ("pitch64",))
    _rgb_forward(dev, ops, geo, "yuv444p16le", "float32", guide, ("pitch64",))


def test_surface_output_allocates_tight_planes(dev, ops):
    shape = B, H, W = SHAPES[2]
    for kind, bits in (("yuv422p", 8), ("yuv444p10le", 10), ("nv16", 8), ("p210", 10)):
        planar, chroma = KINDS[kind][:2]
        c = case(shape, kind)
        _, k, k_out = constants(kind, dev)
        got = forward_surface(ops, kind, bits, T(c["grid"], dev), planes_in(kind, c["codes"], "tight", dev), k, k_out,
                              guide=T(c["guide"], dev))
        cs = cc.chroma_shape(shape, chroma)
        assert [tuple(t.shape) for t in got] == ([shape, cs, cs] if planar else [shape, shape])
        assert all(t.is_contiguous() and t.dtype == (torch.uint8 if bits == 8 else torch.uint16) for t in got)


# ---- 8. the models and the captured graphs ----------------------------------------------------------------------------------------
def _model(cls, dev, seed=7):
    from hdrnet_amd import models
    torch.manual_seed(seed)
    return getattr(models, cls)(dict(batch_norm=False)).to(dev).eval()


@pytest.mark.parametrize("cls", ["HDRNetCurves", "HDRNetPointwiseNNGuide"])
def test_models_and_runtimes(dev, ops, cls):
    from hdrnet_amd import data
    from hdrnet_amd.runtime import PlanarYuvFrameInference, YuvFrameInference
    m = _model(cls, dev)
    shape = (1, 271, 480)  # odd H
    label = "+curvesguide" if cls == "HDRNetCurves" else "+nnguide"

    def surface(kind, seed):
        codes = cc.random_planar(np.random.default_rng([103, seed]), shape, KINDS[kind][2], KINDS[kind][1], corners=False)
        return tuple(T(a, dev) for a in stored(kind, codes))

    def by_hand(kind, p, out_bits=None, out_dtype=None):
        """lowres gather -> coefficient network -> the op, as process_yuv / process_yuv_planar document it."""
        planar, chroma, bits, standard, full, _ = KINDS[kind]
        to_rgb, _ = m._yuv_constants(standard, full, bits, dev, msb_aligned=not planar)
        gather = data.lowres_input_yuv_planar if planar else data.lowres_input_yuv
        coeffs = m.coefficients(gather(*p, to_rgb, m.params["net_input_size"], chroma=chroma))
        gs = coeffs.shape
        grid = coeffs.reshape(gs[0], gs[1], gs[2], gs[3], gs[4] * gs[5])
        kw = m._process_guide_args()
        if out_bits is None:
            return forward(ops, kind, grid, p, to_rgb, out="rgb", out_dtype=out_dtype, **kw)
        return forward_surface(ops, kind, out_bits, grid, p, to_rgb, m._yuv_encode_constants(standard, full, out_bits, dev), **kw)

    def process(kind, p, **kw):
        planar, chroma, bits, standard, full, _ = KINDS[kind]
        f = m.process_yuv_planar if planar else m.process_yuv
        return f(*p, standard=standard, full_range=full, bits=bits, chroma=chroma, **kw)

    def same(a, b):
        a, b = (a, b) if isinstance(a, tuple) else ((a,), (b,))
        return len(a) == len(b) and all(x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                                                                          y.view(torch.int32) if y.dtype == torch.float32 else y)
                                        for x, y in zip(a, b))

    with torch.no_grad():
        for kind, outs in (("nv16", ["nv16"]), ("p210", ["nv16", "p210"]), ("p216", ["p216"])):
            p = surface(kind, 1)
            assert same(process(kind, p), by_hand(kind, p))
            assert ops.last_kernel().startswith(f"apply_fwd_io/{KINDS[kind][5]}->f32{label}")
            assert same(process(kind, p, out_dtype=torch.uint8), by_hand(kind, p, out_dtype=torch.uint8))
            for out in outs:
                out_bits = {"nv16": 8, "p210": 10, "p216": 16}[out]
                got = process(kind, p, out=out)
                assert ops.last_kernel().startswith(f"apply_fwd_io/{KINDS[kind][5]}->{'nv16' if out_bits == 8 else 'p216'}{label}")
                assert same(got, by_hand(kind, p, out_bits=out_bits)) and len(torch.unique(got[1])) > 8
        for kind in ("yuv422p", "yuv422p10le", "yuv444p", "yuv444p16le"):
            p = surface(kind, 2)
            assert same(process(kind, p, out_dtype=torch.uint8), by_hand(kind, p, out_dtype=torch.uint8))
            got = process(kind, p, out="planar")
            assert ops.last_kernel().startswith(f"apply_fwd_io/{KINDS[kind][5]}->{KINDS[kind][5]}{label}")
            assert same(got, by_hand(kind, p, out_bits=KINDS[kind][2])) and got[1].shape == p[1].shape
    # graphs captured on one surface replay another, copied in -- and the first again
    for kind, out in (("yuv422p10le", "planar"), ("yuv444p", "planar"), ("p210", "p210"), ("nv16", "rgb")):
        planar, chroma, bits, standard, full, _ = KINDS[kind]
        p1, p2 = surface(kind, 3), surface(kind, 4)
        kw = dict(standard=standard, full_range=full, bits=bits, out=out, chroma=chroma)
        fi = (PlanarYuvFrameInference if planar else YuvFrameInference)(m, *p1, **kw)
        with torch.no_grad():
            want1 = process(kind, p1, out=out)
            want2 = process(kind, p2, out=out)
        want1, want2 = (tuple(t.clone() for t in w) if isinstance(w, tuple) else w.clone() for w in (want1, want2))
        assert same(fi(*p2), want2), (kind, "the replay on new plane contents")
        assert same(fi(*p1), want1), (kind, "the second replay")
        assert not same(want1, want2)
