"""Packed YUV 4:2:2 surfaces on the GPU (include/hdrnet_amd_yuv_packed.h): YUY2 / UYVY / YVYU / Y210 / Y216 through the
conversion kernel, the low-res gather, the fused wire-format forward with RGB and packed-surface outputs, both single-level
models and the captured graph.

THE ORACLE is the existing semi-planar 4:2:2 path on the UNWOVEN surface: a packed surface holds exactly the samples of the
NV16 / P210 / P216 pair (tests/yuv_packed_cases.py), the arithmetic is that path's expression for expression, so every output
must equal it bit for bit.  Everything below is ``torch.equal`` / ``np.array_equal``; no tolerance appears in this file.

1. ``yuv_packed_to_rgb`` == ``yuv_to_rgb(unwoven, chroma="422")``;
2. fused RGB outputs == ``bilateral_slice_apply_io_yuv(unwoven, chroma="422")`` for every format x {float32, uint8} x the five
   guide forms, ``guide_out`` included, with the new kernel label;
3. surface outputs, woven back, == the NV16 / P210 / P216 output of the same call on the unwoven surface, in and out
   independently laid out, into buffers pre-filled with 0xA5 and with 0x5A, padding and 4096 guard bytes untouched;
4. the three uint8 orders of the same codes give identical RGB and surfaces that unweave to the same planes;
5. ``data.lowres_input_yuv_packed`` == ``data.lowres_input_yuv(unwoven, chroma="422")``;
6. ``process_yuv_packed`` == the ops composed by hand (and == ``process_yuv(chroma="422")`` on the unwoven surface);
7. ``PackedYuvFrameInference`` replays == the eager call;
8. B = 0 and H = 0 are no-ops.

Shapes, grid 16 x 16 x 8: (2, 5, 1040) -- two row segments, the second partial, odd H, a second image -- (1, 3, 96), one
segment, (1, 3, 100), the last wave's last lane half way through the plan's width, (1, 1, 4), one lane of one row.  ``map``
and ``nn`` run at every shape, the three curves forms at (2, 5, 1040).  Layouts: tight, pitch + 64 bytes, two images in one
allocation."""
import numpy as np
import pytest
import torch

import wire_geometry_cases as wg
import yuv_packed_cases as kc
import yuv_planar_cases as pc
from row_plan import row_plan

pytestmark = pytest.mark.gpu

GRID = (16, 16, 8)
SHAPES = [(2, 5, 1040), (1, 3, 96), (1, 3, 100), (1, 1, 4)]
# format -> (standard, full range, kernel label)
FORMATS = {"yuy2": ("bt709", False, "yuy2"), "uyvy": ("bt601", True, "uyvy"), "yvyu": ("bt709", False, "yvyu"),
           "y210": ("bt2020", False, "y216"), "y216": ("bt601", True, "y216")}
GUIDES = ["map", "nn", "curves", "cells", "scan"]
GUIDE_LABEL = {"map": "", "nn": "+nnguide", "curves": "+curvesguide", "cells": "+curvesguide/cells",
               "scan": "+curvesguide/scan"}
SHORT = {"uint8": "u8", "float32": "f32"}
SEMI_LABEL = {8: "nv16", 10: "p216", 16: "p216"}


def shapes_of(guide):
    return SHAPES if guide in ("map", "nn") else SHAPES[:1]


def test_the_shapes_are_what_the_comment_says():
    assert row_plan(1040) == (192, 2, 520) and row_plan(96) == (64, 1, 96) and row_plan(100) == (64, 1, 100)
    assert 100 // 4 == 25 and 25 % 64 != 0 and SHAPES[0][1] % 2 == 1 and SHAPES[0][0] == 2
    assert [kc.bits_of(f) for f in FORMATS] == [8, 8, 8, 10, 16] and set(FORMATS) == set(kc.FORMATS)


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


def constants(fmt, dev):
    """``(to_rgb of the samples as stored, from_rgb in code units of the format's bits)`` on the device."""
    from hdrnet_amd import yuv
    standard, full, _ = FORMATS[fmt]
    bits = kc.bits_of(fmt)
    return T(yuv.yuv_coefficients(standard, full, bits)[0], dev), T(yuv.yuv_encode_coefficients(standard, full, bits), dev)


_CASES, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _CASES.clear()
    _REFS.clear()


def case(shape, bits):
    """Grid, guide parameters and ONE content per (shape, bits): ``codes`` = (y, u, v) in the low bits.  The three uint8
    orders share it (item 4)."""
    key = (shape, bits)
    if key not in _CASES:
        rng = np.random.default_rng([131, *shape, bits])
        c = wg.guides(rng, shape, GRID)
        c["codes"] = kc.random_codes(rng, shape, bits, corners=shape[1] > 1 and shape[2] > 4)
        _CASES[key] = c
    return _CASES[key]


def device_surface(bufs, spec, dev):
    flats = [T(b, dev) for b in bufs]
    i, off, shape, strides = spec
    return flats, flats[i].as_strided(shape, strides, off)


def surface_in(fmt, codes, layout, dev):
    return device_surface(*kc.lay(kc.packed(codes, fmt), layout), dev)[1]


def unwoven_in(fmt, codes, dev):
    return tuple(T(a, dev) for a in kc.semi(codes, kc.bits_of(fmt)))


def guide_kw(ops, c, guide, dev, want_guide=True):
    if guide == "map":
        return dict(guide=T(c["guide"], dev))
    extra = dict(return_guide=True) if want_guide else {}
    if guide == "nn":
        return dict(guide_conv1=T(c["conv1"], dev), guide_conv2=T(c["conv2"], dev), **extra)
    curves = tuple(T(a, dev) for a in wg.curves_of(c, guide))
    kw = dict(guide_curves=curves, **extra)
    if guide == "cells":
        kw["curves_prepared"] = ops.curves_guide_prepare(curves[1], curves[2])
        assert kw["curves_prepared"] is not None, "the case's knots are apart: the cell tables are usable"
    return kw


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    same = np.array_equal(got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else np.array_equal(got, want)
    if not same:
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} samples differ, first at {bad[0]}: got "
                             f"{got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


def rgb_reference(ops, dev, shape, fmt, out, guide):
    """The existing 4:2:2 semi-planar forward on the unwoven surface, once per (shape, bits, constants, out, guide)."""
    bits = kc.bits_of(fmt)
    key = (shape, bits, FORMATS[fmt][:2], out, guide)
    if key not in _REFS:
        c = case(shape, bits)
        k, _ = constants(fmt, dev)
        got = ops.bilateral_slice_apply_io_yuv(T(c["grid"], dev), *unwoven_in(fmt, c["codes"], dev), k, chroma="422", out="rgb",
                                               out_dtype=getattr(torch, out), **guide_kw(ops, c, guide, dev))
        assert ops.last_kernel() == f"apply_fwd_io/{SEMI_LABEL[bits]}->{SHORT[out]}{GUIDE_LABEL[guide]}"
        o, g = got if guide != "map" else (got, None)
        _REFS[key] = (N(o), None if g is None else N(g))
    return _REFS[key]


def surface_reference(ops, dev, shape, fmt, guide):
    """The NV16 / P210 / P216 output ``(y, uv)`` of the same call on the unwoven surface."""
    bits = kc.bits_of(fmt)
    key = (shape, bits, FORMATS[fmt][:2], "surface", guide)
    if key not in _REFS:
        c = case(shape, bits)
        k, k_out = constants(fmt, dev)
        planes = unwoven_in(fmt, c["codes"], dev)
        kw = guide_kw(ops, c, guide, dev, want_guide=False)
        if bits == 8:
            got = ops.bilateral_slice_apply_io_yuv(T(c["grid"], dev), *planes, k, chroma="422", out="nv16", from_rgb=k_out, **kw)
        else:
            got = ops.bilateral_slice_apply_io_yuv_deep(T(c["grid"], dev), *planes, k, chroma="422", from_rgb=k_out,
                                                        out_bits=bits, **kw)
        assert ops.last_kernel() == f"apply_fwd_io/{SEMI_LABEL[bits]}->{SEMI_LABEL[bits]}{GUIDE_LABEL[guide]}"
        _REFS[key] = tuple(N(t) for t in got)
    return _REFS[key]


# ---- 1. the conversion ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_conversion_is_the_422_conversion(dev, ops, fmt):
    k, _ = constants(fmt, dev)
    for shape in SHAPES:
        c = case(shape, kc.bits_of(fmt))
        want = ops.yuv_to_rgb(*unwoven_in(fmt, c["codes"], dev), k, chroma="422")
        assert ops.last_kernel() == "yuv_422_to_rgb"
        if shape == SHAPES[0]:
            assert want.min() == 0.0 and want.max() == 1.0 and len(torch.unique(want)) > 1000  # a picture, both clamps
        for layout in kc.LAYOUTS:
            got = ops.yuv_packed_to_rgb(surface_in(fmt, c["codes"], layout, dev), k, fmt)
            assert ops.last_kernel() == "yuv_packed_to_rgb" and tuple(got.shape) == shape + (3,) and got.dtype == torch.float32
            assert_same(N(got), N(want), f"conversion {fmt} {shape} {layout}")
    # the 4-D view [B, H, W, 2] is the same surface
    c = case(SHAPES[1], kc.bits_of(fmt))
    s = surface_in(fmt, c["codes"], "tight", dev)
    assert torch.equal(ops.yuv_packed_to_rgb(s.view(1, 3, 96, 2), k, fmt), ops.yuv_packed_to_rgb(s, k, fmt))


# ---- 2. the fused forward to float32 and uint8 RGB ----------------------------------------------------------------------------
@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("out", ["uint8", "float32"])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_rgb_outputs_are_exact(dev, ops, fmt, out, guide):
    k, _ = constants(fmt, dev)
    for shape in shapes_of(guide):
        c = case(shape, kc.bits_of(fmt))
        want, want_guide = rgb_reference(ops, dev, shape, fmt, out, guide)
        for layout in kc.LAYOUTS:
            got = ops.bilateral_slice_apply_io_yuv_packed(T(c["grid"], dev), surface_in(fmt, c["codes"], layout, dev), k, fmt,
                                                          out="rgb", out_dtype=getattr(torch, out), **guide_kw(ops, c, guide, dev))
            assert ops.last_kernel() == f"apply_fwd_io/{FORMATS[fmt][2]}->{SHORT[out]}{GUIDE_LABEL[guide]}"
            o, g = got if want_guide is not None else (got, None)
            assert tuple(o.shape) == shape + (3,) and o.dtype == getattr(torch, out)
            assert_same(N(o), want, f"{shape} {fmt} {layout} -> {out} {guide}")
            if want_guide is not None:
                assert_same(N(g), want_guide, f"{shape} {fmt} {layout} {guide}: the guide the kernel computed")


# ---- 3. surface outputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(kc.LAYOUTS))
@pytest.mark.parametrize("guide", ["map", "nn"])
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_surface_outputs_are_exact(dev, ops, fmt, guide, layout):
    """yuy2 / uyvy / yvyu at 8 bits, y210 at 10, y216 at 16.  The input lies in ``layout``, the output in the NEXT one: the
    two are pitched independently."""
    bits, order, dt = kc.bits_of(fmt), kc.order_of(fmt), kc.dtype_of(fmt)
    out_layout = kc.LAYOUTS[(kc.LAYOUTS.index(layout) + 1) % len(kc.LAYOUTS)]
    k, k_out = constants(fmt, dev)
    for shape in SHAPES:
        c = case(shape, bits)
        wy, wuv = surface_reference(ops, dev, shape, fmt, guide)
        want = kc.weave(wy, wuv, order)
        if shape == SHAPES[0]:
            assert len(np.unique(wy)) > 100 and len(np.unique(wuv)) > 50  # a picture, not a constant
        for fill in kc.FILLS:
            blank = np.full(want.shape, pc.fill_value(dt, fill), dt)  # the surface itself starts out as the fill too
            bufs, spec = kc.lay(blank, out_layout, fill)
            flats, out_surface = device_surface(bufs, spec, dev)
            res = ops.bilateral_slice_apply_io_yuv_packed(T(c["grid"], dev), surface_in(fmt, c["codes"], layout, dev), k, fmt,
                                                          out="packed", from_rgb=k_out, out_surface=out_surface,
                                                          **guide_kw(ops, c, guide, dev, want_guide=False))
            label = FORMATS[fmt][2]
            assert ops.last_kernel() == f"apply_fwd_io/{label}->{label}{GUIDE_LABEL[guide]}"
            assert res.data_ptr() == out_surface.data_ptr() and res.dtype == out_surface.dtype
            what = f"{shape} {fmt} {layout} -> {out_layout} fill {fill:#x} {guide}"
            assert_same(N(out_surface), want, what)
            for flat, mask in zip(flats, pc.outside_planes(bufs, [spec])):
                assert (N(flat)[mask] == pc.fill_value(dt, fill)).all(), f"{what}: a store left the surface"
    # without out_surface: a tight surface of the input's dtype
    c = case(SHAPES[2], bits)
    got = ops.bilateral_slice_apply_io_yuv_packed(T(c["grid"], dev), surface_in(fmt, c["codes"], layout, dev), k, fmt, out="packed",
                                                  from_rgb=k_out, **guide_kw(ops, c, guide, dev, want_guide=False))
    assert got.is_contiguous() and tuple(got.shape) == (1, 3, 200)
    assert_same(N(got), kc.weave(*surface_reference(ops, dev, SHAPES[2], fmt, guide), order), f"{fmt} {guide}: the tight output")


def test_y210_and_y216_codes_sit_in_the_high_bits(dev, ops):
    for fmt, low in (("y210", 0x3f), ("y216", 0)):
        c = case(SHAPES[0], kc.bits_of(fmt))
        k, k_out = constants(fmt, dev)
        got = N(ops.bilateral_slice_apply_io_yuv_packed(T(c["grid"], dev), surface_in(fmt, c["codes"], "tight", dev), k, fmt,
                                                        guide=T(c["guide"], dev), out="packed", from_rgb=k_out))
        assert not (got & low).any() and len(np.unique(got >> (16 - kc.bits_of(fmt)))) > 200


# ---- 4. the three uint8 orders ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guide", ["map", "nn"])
@pytest.mark.parametrize("out", ["float32", "uint8", "packed"])
def test_the_three_orders_agree(dev, ops, out, guide):
    """The same codes in YUYV, UYVY and YVYU order under the SAME constants: identical RGB, and surface outputs that unweave
    to the same planes -- a selector applied on one side only, or the wrong one, cannot pass."""
    k, k_out = constants("yuy2", dev)
    for shape in SHAPES:
        c = case(shape, 8)
        res = {}
        for fmt in ("yuy2", "uyvy", "yvyu"):
            s = surface_in(fmt, c["codes"], "pitch64", dev)
            kw = guide_kw(ops, c, guide, dev, want_guide=False)
            if out == "packed":
                got = ops.bilateral_slice_apply_io_yuv_packed(T(c["grid"], dev), s, k, fmt, out="packed", from_rgb=k_out, **kw)
                res[fmt] = kc.unweave(N(got), kc.order_of(fmt))
            else:
                got = ops.bilateral_slice_apply_io_yuv_packed(T(c["grid"], dev), s, k, fmt, out_dtype=getattr(torch, out), **kw)
                res[fmt] = (N(got),)
        for fmt in ("uyvy", "yvyu"):
            for a, b in zip(res[fmt], res["yuy2"]):
                assert_same(a, b, f"{shape} {fmt} against yuy2 -> {out} {guide}")
        if shape == SHAPES[0]:
            assert all(len(np.unique(a)) > 50 for a in res["yuy2"])


# ---- 5. the low-res gather --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 6, 5])  # 256 and 6: the vector store (n * n % 4 == 0); 5: the scalar tail
@pytest.mark.parametrize("fmt", list(FORMATS))
def test_lowres_gather(dev, fmt, n):
    from hdrnet_amd import _lib, data
    k, _ = constants(fmt, dev)
    shape = (2, 37, 52)
    codes = kc.random_codes(np.random.default_rng([137, n, kc.bits_of(fmt)]), shape, kc.bits_of(fmt))
    want = data.lowres_input_yuv(*unwoven_in(fmt, codes, dev), k, n, chroma="422")
    for layout in kc.LAYOUTS:
        got = data.lowres_input_yuv_packed(surface_in(fmt, codes, layout, dev), k, fmt, n)
        assert _lib.last_kernel() == "sample_prep" and tuple(got.shape) == (2, n, n, 3)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (fmt, layout)
    assert len(torch.unique(got)) > 8


# ---- 6. the models ----------------------------------------------------------------------------------------------------------------
def _model(cls, dev, seed=7):
    from hdrnet_amd import models
    torch.manual_seed(seed)
    return getattr(models, cls)(dict(batch_norm=False)).to(dev).eval()


def _same(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                              b.view(torch.int32) if b.dtype == torch.float32 else b)


def _model_surface(fmt, seed, dev, shape=(1, 271, 480)):
    codes = kc.random_codes(np.random.default_rng([139, seed]), shape, kc.bits_of(fmt), corners=False)
    return codes, T(kc.packed(codes, fmt), dev)


@pytest.mark.parametrize("out", ["rgb", "packed"])
@pytest.mark.parametrize("cls", ["HDRNetCurves", "HDRNetPointwiseNNGuide"])
def test_models(dev, ops, cls, out):
    from hdrnet_amd import data
    m = _model(cls, dev)
    label = "+curvesguide" if cls == "HDRNetCurves" else "+nnguide"
    semi_out = {8: "nv16", 10: "p210", 16: "p216"}
    with torch.no_grad():
        for fmt in FORMATS:
            standard, full, name = FORMATS[fmt]
            bits = kc.bits_of(fmt)
            codes, s = _model_surface(fmt, 1, dev)
            # by hand: lowres gather -> coefficient network -> the op, as process_yuv_packed documents it
            to_rgb, from_rgb = m._yuv_constants(standard, full, bits, dev)
            coeffs = m.coefficients(data.lowres_input_yuv_packed(s, to_rgb, fmt, m.params["net_input_size"]))
            gs = coeffs.shape
            grid = coeffs.reshape(gs[0], gs[1], gs[2], gs[3], gs[4] * gs[5])
            kw = m._process_guide_args()
            planes = unwoven_in(fmt, codes, dev)
            for out_dtype in ((None, torch.uint8) if out == "rgb" else (None,)):
                if out == "rgb":
                    hand = ops.bilateral_slice_apply_io_yuv_packed(grid, s, to_rgb, fmt, out="rgb", out_dtype=out_dtype, **kw)
                else:
                    k_out = from_rgb if bits == 8 else m._yuv_encode_constants(standard, full, bits, dev)
                    hand = ops.bilateral_slice_apply_io_yuv_packed(grid, s, to_rgb, fmt, out="packed", from_rgb=k_out,
                                                                   out_bits=bits, **kw)
                # (bits: the format's default -- 8, 10 for y210, 16 for y216)
                got = m.process_yuv_packed(s, fmt, standard=standard, full_range=full, out=out, out_dtype=out_dtype)
                short = name if out == "packed" else ("u8" if out_dtype == torch.uint8 else "f32")
                assert ops.last_kernel().startswith(f"apply_fwd_io/{name}->{short}{label}")
                assert _same(got, hand), (cls, fmt, out, out_dtype)
                # ... and the existing model path on the unwoven surface
                if out == "rgb":
                    want = m.process_yuv(*planes, standard=standard, full_range=full, bits=bits, chroma="422", out_dtype=out_dtype)
                    assert _same(got, want), (cls, fmt, out_dtype)
                else:
                    wy, wuv = m.process_yuv(*planes, standard=standard, full_range=full, bits=bits, chroma="422",
                                            out=semi_out[bits])
                    assert np.array_equal(N(got), kc.weave(N(wy), N(wuv), kc.order_of(fmt))), (cls, fmt)
                    assert len(torch.unique(got)) > 8


# ---- 7. the captured graph --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["yuy2", "y210"])
def test_graph_replay(dev, fmt):
    from hdrnet_amd.runtime import PackedYuvFrameInference
    m = _model("HDRNetPointwiseNNGuide", dev)
    standard, full, _ = FORMATS[fmt]
    s1, s2 = _model_surface(fmt, 3, dev)[1], _model_surface(fmt, 4, dev)[1]
    fi = PackedYuvFrameInference(m, s1, fmt, standard=standard, full_range=full, out="packed")
    with torch.no_grad():
        want1 = m.process_yuv_packed(s1, fmt, standard=standard, full_range=full, out="packed").clone()
        want2 = m.process_yuv_packed(s2, fmt, standard=standard, full_range=full, out="packed").clone()
    assert _same(fi(s2), want2), (fmt, "the replay on new surface contents")
    assert _same(fi(s1), want1), (fmt, "the second replay")
    assert not _same(want1, want2) and want1.dtype == s1.dtype and want1.shape == s1.shape


# ---- 8. no-ops --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(0, 3, 8), (1, 0, 8)])
def test_empty_extents_are_noops(dev, ops, shape):
    B, H, W = shape
    for fmt in ("uyvy", "y216"):
        k, k_out = constants(fmt, dev)
        s = torch.zeros((B, H, 2 * W), dtype=torch.uint8 if fmt == "uyvy" else torch.uint16, device=dev)
        grid = torch.zeros((B, *GRID, 12), device=dev)
        guide = torch.zeros(shape, device=dev)
        got = ops.yuv_packed_to_rgb(s, k, fmt)
        assert ops.last_kernel() == "noop" and tuple(got.shape) == shape + (3,)
        got = ops.bilateral_slice_apply_io_yuv_packed(grid, s, k, fmt, guide=guide)
        assert ops.last_kernel() == "noop" and tuple(got.shape) == shape + (3,)
        got = ops.bilateral_slice_apply_io_yuv_packed(grid, s, k, fmt, guide=guide, out="packed", from_rgb=k_out)
        assert ops.last_kernel() == "noop" and tuple(got.shape) == (B, H, 2 * W) and got.dtype == s.dtype
