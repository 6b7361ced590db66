"""Planar YUV surfaces on the GPU (include/hdrnet_amd_yuv_planar.h): I420 / yuv420p10le / yuv420p16le planes through the
conversion kernel, the low-res gather, the fused wire-format forward with RGB and planar outputs, both single-level models
and a captured graph.

The yardstick is the code that is already pinned: a planar surface and the semi-planar surface with the same samples
(tests/yuv_planar_cases.py: U and V interleaved; 10-bit codes shifted up by 6 and converted with the P010 constants) must
give the same BITS through ``yuv_to_rgb``, ``lowres_input_yuv``, ``bilateral_slice_apply_io_yuv`` / ``_yuv_deep`` and
``process_yuv`` -- every comparison below is exact.  The anchor to float64 is the conversion (item 1, at test_gpu_yuv.py's
bar); the semi-planar path's own tests carry the float64 encoder rule and its caps on undecided samples, so nothing here
needs a cap.  ``last_kernel()`` must carry the ``i420`` / ``i016`` labels, so an interleaving pass on the side cannot pass.

Geometries: the grid 16 x 16 x 8 with (2, 6, 1040), (1, 4, 96) (test_gpu_yuv.py's) and (1, 4, 100), whose tight uint8
chroma rows are 50 bytes -- every other row starts 2 bytes past a dword boundary; ``interior`` (chroma pairs that straddle
a grid row: the restaging path of the row-pair store) and ``many_seg`` of tests/wire_geometry_cases.py for one guide form
each.  Layouts: tight planes, pitch = row + 64 bytes, three planes in one allocation; outputs lie in buffers pre-filled
with 0xA5 and with 0x5A, padding and 4096 guard bytes behind each included."""
import numpy as np
import pytest
import torch

import wire_geometry_cases as wg
import yuv_cases as yc
import yuv_planar_cases as pc
from row_plan import row_plan

pytestmark = pytest.mark.gpu

GRID = (16, 16, 8)
SHAPES = [(2, 6, 1040), (1, 4, 96), (1, 4, 100)]
# kind -> (bits, standard, full range): the planar surface and the semi-planar twin that is its yardstick
KINDS = {"i420": (8, "bt709", False), "i016": (16, "bt601", True), "i010": (10, "bt709", False)}
LABEL = {"i420": "i420", "i016": "i016", "i010": "i016"}      # the label states the sample width, not the bit depth
SEMI_LABEL = {"i420": "nv12", "i016": "p016", "i010": "p016"}
GUIDES = ["map", "nn", "curves", "cells", "scan"]
GUIDE_LABEL = {"map": "", "nn": "+nnguide", "curves": "+curvesguide", "cells": "+curvesguide/cells",
               "scan": "+curvesguide/scan"}
SHORT = {"uint8": "u8", "float32": "f32"}
GEOMETRY_GUIDES = [("interior", "nn"), ("many_seg", "cells")]


def test_the_shapes_are_what_the_comment_says():
    assert row_plan(1040) == (192, 2, 520) and row_plan(96) == (64, 1, 96) and row_plan(100) == (64, 1, 100)
    assert (100 // 2) % 4 == 2  # tight uint8 chroma rows of W = 100: odd rows start 2 bytes past a dword boundary
    for geo, _ in GEOMETRY_GUIDES:
        (B, H, W), _ = wg.GEOMETRIES[geo]
        assert B * H * W < 100_000
    assert not all(wg.pair_floors(40, 16))  # interior: some chroma pairs straddle a grid row


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


def constants(kind, dev):
    """``(to_rgb of the planar surface in numpy, ... on the device, to_rgb of the semi-planar twin on the device, from_rgb in
    code units of the kind's depth on the device)``."""
    from hdrnet_amd import yuv
    bits, standard, full = KINDS[kind]
    low = yuv.yuv_coefficients(standard, full, bits, msb_aligned=False)[0]
    semi = yuv.yuv_coefficients(standard, full, bits)[0]
    return low, T(low, dev), T(semi, dev), T(yuv.yuv_encode_coefficients(standard, full, bits), dev)


_CASES, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _CASES.clear()
    _REFS.clear()


def extents(where):
    return wg.GEOMETRIES[where] if isinstance(where, str) else (where, GRID)


def case(where, kind):
    """Grid, guide parameters and ONE surface content per (shape or geometry id, kind): ``planar`` = (y, u, v) with the codes
    in the low bits, ``semi`` = (y, uv) of the same codes as a semi-planar surface stores them.  Every layout holds the same
    samples, so the layouts share the references."""
    key = (where, kind)
    if key not in _CASES:
        bits = KINDS[kind][0]
        shape, grid = extents(where)
        if isinstance(where, str):  # the geometry's own content (corners pinned to the extreme codes)
            c = dict(wg.surface_case(where, bits))
            sh = yc.stored_shift(bits)
            c["semi"] = (c["y"], c["uv"])
            c["planar"] = (c["y"] >> sh, *pc.split(c["uv"] >> sh))
        else:
            rng = np.random.default_rng([71, *shape, bits])
            c = wg.guides(rng, shape, grid)
            c["planar"], c["semi"] = pc.random_planar(rng, shape, bits)
        _CASES[key] = c
    return _CASES[key]


def device_planes(bufs, specs, dev):
    """The planes of flat numpy buffers as views of their device copies: ``(flat tensors, plane views)``."""
    flats = [T(b, dev) for b in bufs]
    return flats, tuple(flats[i].as_strided(shape, strides, off) for i, off, shape, strides in specs)


def planes_in(c, layout, dev):
    _, views = device_planes(*pc.lay_planar(*c["planar"], layout), dev)
    return views


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


def semi_reference(ops, dev, where, kind, out, guide):
    """The semi-planar path on the interleaved surface, once per case: ``out`` "float32" / "uint8" -> (frame, guide or
    None); "surface" -> ((Y, U, V), guide or None) with the UV plane split and P010's codes shifted down to the low bits."""
    key = (where, kind, out, guide)
    if key not in _REFS:
        c = case(where, kind)
        bits = KINDS[kind][0]
        _, _, k_semi, k_out = constants(kind, dev)
        y, uv = (T(a, dev) for a in c["semi"])
        kw = guide_kw(ops, c, guide, dev)
        if out != "surface":
            got = ops.bilateral_slice_apply_io_yuv(T(c["grid"], dev), y, uv, k_semi, out="rgb", out_dtype=getattr(torch, out), **kw)
            assert ops.last_kernel() == f"apply_fwd_io/{SEMI_LABEL[kind]}->{SHORT[out]}{GUIDE_LABEL[guide]}"
        elif bits == 8:
            got = ops.bilateral_slice_apply_io_yuv(T(c["grid"], dev), y, uv, k_semi, out="nv12", from_rgb=k_out, **kw)
            assert ops.last_kernel() == f"apply_fwd_io/nv12->nv12{GUIDE_LABEL[guide]}"
        else:
            got = ops.bilateral_slice_apply_io_yuv_deep(T(c["grid"], dev), y, uv, k_semi, from_rgb=k_out, out_bits=bits, **kw)
            assert ops.last_kernel() == f"apply_fwd_io/p016->p016{GUIDE_LABEL[guide]}"
        o, g = got if "return_guide" in kw else (got, None)
        g = None if g is None else N(g)
        if out == "surface":
            sh = yc.stored_shift(bits)
            oy, ouv = N(o[0]), N(o[1])
            assert not (oy & ((1 << sh) - 1)).any() and not (ouv & ((1 << sh) - 1)).any()  # P010: the low 6 bits are 0
            o = (oy >> sh, *pc.split(ouv >> sh))
        else:
            o = N(o)
        _REFS[key] = (o, g)
    return _REFS[key]


def assert_same(got, want, what):
    same = np.array_equal(got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else np.array_equal(got, want)
    if not same:
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} samples differ, first at {bad[0]}: got "
                             f"{got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


# ---- 1. the conversion against float64, and against the semi-planar kernel ----------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_yuv_planar_to_rgb(dev, ops, kind):
    """atol 2e-6 (test_gpu_yuv.py::test_yuv_to_rgb): three fused operations on magnitudes below 4, each within half an ulp
    <= 2.4e-7, on the same float32 constants.  The corners hold super-black and super-white codes: both sides of the clamp
    are reached."""
    low, k, k_semi, _ = constants(kind, dev)
    for shape in SHAPES:
        c = case(shape, kind)
        y, u, v = c["planar"]
        want = yc.to_rgb64(y, pc.interleave(u, v), low)
        assert want.min() == 0.0 and want.max() == 1.0
        assert np.all(want[:, 0, 0] == 0.0) and np.all(want[:, 0, -1] >= 1.0 - 1e-6)
        semi = N(ops.yuv_to_rgb(*(T(a, dev) for a in c["semi"]), k_semi))
        assert ops.last_kernel() == "yuv_to_rgb"
        for layout in pc.LAYOUTS:
            got = ops.yuv_planar_to_rgb(*planes_in(c, layout, dev), k)
            assert ops.last_kernel() == "yuv_planar_to_rgb" and tuple(got.shape) == shape + (3,) and got.dtype == torch.float32
            g = N(got)
            print(f"yuv_planar_to_rgb {kind} {shape} {layout}: max |err| = {np.abs(g - want).max():.3g}")
            np.testing.assert_allclose(g, want, rtol=0, atol=2e-6)
            assert g.min() == 0.0 and g.max() == 1.0
            if layout == "tight":
                tight = g
            else:
                assert_same(g, tight, f"{kind} {shape} {layout} against the tight planes")
            assert_same(g, semi, f"{kind} {shape} {layout} against yuv_to_rgb of the interleaved surface")


# ---- 2. the fused forward to float32 and uint8 RGB: the bits of the semi-planar forward ----------------------------------
def _rgb_forward(dev, ops, where, kind, out, guide, layouts):
    _, k, _, _ = constants(kind, dev)
    c = case(where, kind)
    shape, _ = extents(where)
    want, want_guide = semi_reference(ops, dev, where, kind, out, guide)
    for layout in layouts:
        got = ops.bilateral_slice_apply_io_yuv_planar(T(c["grid"], dev), *planes_in(c, layout, dev), k, out="rgb",
                                                      out_dtype=getattr(torch, out), **guide_kw(ops, c, guide, dev))
        assert ops.last_kernel() == f"apply_fwd_io/{LABEL[kind]}->{SHORT[out]}{GUIDE_LABEL[guide]}"
        o, g = got if want_guide is not None else (got, None)
        assert tuple(o.shape) == shape + (3,) and o.dtype == getattr(torch, out)
        assert_same(N(o), want, f"{where} {kind} {layout} -> {out} {guide}")
        if want_guide is not None:
            assert_same(N(g), want_guide, f"{where} {kind} {layout} {guide}: the guide the kernel computed")


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("out", ["uint8", "float32"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_rgb_bits_equal_the_semi_planar_forward(dev, ops, kind, out, guide):
    for shape in SHAPES:
        _rgb_forward(dev, ops, shape, kind, out, guide, pc.LAYOUTS)


# ---- 3. the low-res gather -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 6, 5])  # 256 and 6: the vector store (n * n % 4 == 0); 5: the scalar tail
@pytest.mark.parametrize("kind", ["i420", "i010"])
def test_lowres_input_yuv_planar(dev, ops, kind, n):
    from hdrnet_amd import _lib, data
    bits = KINDS[kind][0]
    _, k, k_semi, _ = constants(kind, dev)
    shape = (2, 38, 52)
    planar, semi = pc.random_planar(np.random.default_rng([73, n, bits]), shape, bits)
    want = data.lowres_input_yuv(*(T(a, dev) for a in semi), k_semi, n)
    for layout in ("pitch64", "one_allocation"):
        _, (y, u, v) = device_planes(*pc.lay_planar(*planar, layout), dev)
        got = data.lowres_input_yuv_planar(y, u, v, k, n)
        assert _lib.last_kernel() == "sample_prep" and tuple(got.shape) == (2, n, n, 3)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), layout
    assert len(torch.unique(got)) > 8


# ---- 4. a planar surface out ---------------------------------------------------------------------------------------------
def _planar_forward(dev, ops, where, kind, guide, layouts):
    bits = KINDS[kind][0]
    _, k, _, k_out = constants(kind, dev)
    c = case(where, kind)
    shape, _ = extents(where)
    dt = c["planar"][0].dtype
    want, want_guide = semi_reference(ops, dev, where, kind, "surface", guide)
    if where == SHAPES[0]:
        assert len(np.unique(want[0])) > 100 and len(np.unique(want[1])) > 50  # a picture, not a constant
        assert int(want[0].max()) <= 2 ** bits - 1
    for layout in layouts:
        for fill in pc.FILLS:
            blank_y, blank_c = np.zeros(shape, dt), np.zeros((shape[0], shape[1] // 2, shape[2] // 2), dt)
            bufs, specs = pc.lay_planar(blank_y, blank_c, blank_c, layout, fill)
            for spec in specs:  # the planes themselves start out as the fill too: a sample never written shows
                pc.plane(bufs, spec)[...] = pc.fill_value(dt, fill)
            flats, outs = device_planes(bufs, specs, dev)
            got = ops.bilateral_slice_apply_io_yuv_planar(T(c["grid"], dev), *planes_in(c, layout, dev), k, out="planar",
                                                          from_rgb=k_out, out_bits=bits, out_planes=outs,
                                                          **guide_kw(ops, c, guide, dev))
            assert ops.last_kernel() == f"apply_fwd_io/{LABEL[kind]}->{LABEL[kind]}{GUIDE_LABEL[guide]}"
            res, g = got if want_guide is not None else (got, None)
            assert len(res) == 3 and all(r.data_ptr() == o.data_ptr() for r, o in zip(res, outs))  # the planes passed
            for name, plane, ref in zip("YUV", outs, want):
                assert_same(N(plane), ref, f"{where} {kind} {layout} fill {fill:#x} {guide}: plane {name}")
            if g is not None:
                assert_same(N(g), want_guide, f"{where} {kind} {layout} {guide}: the guide the kernel computed")
            # padding and the guard behind each buffer keep their fill
            for flat, mask in zip(flats, pc.outside_planes(bufs, specs)):
                assert (N(flat)[mask] == pc.fill_value(dt, fill)).all(), f"{where} {kind} {layout}: a store left the planes"


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_planar_output(dev, ops, kind, guide):
    """uint8 -> I420, uint16 -> 10-bit and 16-bit codes in the low bits: Y equals the semi-planar output's Y plane, U its
    UV[..., 0::2] and V its UV[..., 1::2] (P010's planes >> 6), exactly."""
    for shape in SHAPES:
        _planar_forward(dev, ops, shape, kind, guide, pc.LAYOUTS)


@pytest.mark.parametrize("geo,guide", GEOMETRY_GUIDES)
def test_geometries(dev, ops, geo, guide):
    """An interior segment with chroma pairs that straddle a grid row (the row-pair store restages the LDS image between the
    two rows); 11 segments with the column windows computed on the device."""
    for kind in KINDS:
        _rgb_forward(dev, ops, geo, kind, "float32", guide, ("tight",))
        _planar_forward(dev, ops, geo, kind, guide, ("tight", "pitch64"))


def test_planar_output_allocates_tight_planes(dev, ops):
    for kind in ("i420", "i010"):
        shape = SHAPES[2]
        B, H, W = shape
        c = case(shape, kind)
        _, k, _, k_out = constants(kind, dev)
        want, _ = semi_reference(ops, dev, shape, kind, "surface", "map")
        got = ops.bilateral_slice_apply_io_yuv_planar(T(c["grid"], dev), *planes_in(c, "tight", dev), k, guide=T(c["guide"], dev),
                                                      out="planar", from_rgb=k_out, out_bits=KINDS[kind][0])
        assert [tuple(t.shape) for t in got] == [(B, H, W), (B, H // 2, W // 2), (B, H // 2, W // 2)]
        assert all(t.is_contiguous() and t.dtype == got[0].dtype for t in got)
        for name, plane, ref in zip("YUV", got, want):
            assert_same(N(plane), ref, f"{kind}: plane {name}")


# ---- 5. the models and the captured graph -------------------------------------------------------------------------------
def _model(cls, dev, seed=7):
    from hdrnet_amd import models
    torch.manual_seed(seed)
    return getattr(models, cls)(dict(batch_norm=False)).to(dev).eval()


@pytest.mark.parametrize("cls", ["HDRNetCurves", "HDRNetPointwiseNNGuide"])
def test_models_process_yuv_planar(dev, ops, cls):
    from hdrnet_amd.runtime import PlanarYuvFrameInference
    m = _model(cls, dev)
    shape = (1, 272, 480)
    label = "+curvesguide" if cls == "HDRNetCurves" else "+nnguide"

    def surfaces(seed, bits):
        rng = np.random.default_rng([79, seed, bits])
        y, uv = yc.random_surface(rng, shape, bits, corners=False)
        sh = yc.stored_shift(bits)
        return tuple(T(a, dev) for a in (y >> sh, *pc.split(uv >> sh))), (T(y, dev), T(uv, dev))

    def same_surface(got, want, sh):
        wy, wuv = N(want[0]), N(want[1])
        wu, wv = pc.split(wuv >> sh)
        for name, plane, ref in zip("YUV", got, (wy >> sh, wu, wv)):
            assert_same(N(plane), ref, f"{cls}: plane {name}")

    (p1, s1), (p2, s2) = surfaces(1, 8), surfaces(2, 8)
    with torch.no_grad():
        # I420 in: float32 and uint8 RGB, I420 against NV12
        got = m.process_yuv_planar(*p1)
        assert ops.last_kernel().startswith("apply_fwd_io/i420->f32" + label) and tuple(got.shape) == shape + (3,)
        assert torch.equal(got.view(torch.int32), m.process_yuv(*s1).view(torch.int32))
        got = m.process_yuv_planar(*p1, out_dtype=torch.uint8)
        assert ops.last_kernel().startswith("apply_fwd_io/i420->u8" + label) and got.dtype == torch.uint8
        assert torch.equal(got, m.process_yuv(*s1, out_dtype=torch.uint8))
        got1 = m.process_yuv_planar(*p1, out="planar")
        assert ops.last_kernel().startswith("apply_fwd_io/i420->i420" + label)
        assert len(torch.unique(got1[0])) > 8
        same_surface(got1, m.process_yuv(*s1, out="nv12"), 0)
        # yuv420p10le, BT.2020, full range: uint8 RGB, and 10-bit planes against P010
        p10, s10 = surfaces(3, 10)
        kw = dict(standard="bt2020", full_range=True, bits=10)
        got = m.process_yuv_planar(*p10, out_dtype=torch.uint8, **kw)
        assert ops.last_kernel().startswith("apply_fwd_io/i016->u8" + label)
        assert torch.equal(got, m.process_yuv(*s10, out_dtype=torch.uint8, **kw))
        got10 = m.process_yuv_planar(*p10, out="planar", **kw)
        assert ops.last_kernel().startswith("apply_fwd_io/i016->i016" + label) and got10[0].dtype == torch.uint16
        same_surface(got10, m.process_yuv(*s10, out="p010", **kw), 6)
    # a graph captured on one surface replays another, copied in -- and the first again
    fi = PlanarYuvFrameInference(m, *p1)
    want2 = [t.clone() for t in m.process_yuv_planar(*p2, out="planar")]
    assert all(torch.equal(r, w) for r, w in zip(fi(*p2), want2))
    assert all(torch.equal(r, w) for r, w in zip(fi(*p1), got1))
    assert not torch.equal(fi.static_output[0], want2[0])
    rgb = PlanarYuvFrameInference(m, *p1, out="rgb", out_dtype=torch.uint8)
    assert torch.equal(rgb(*p2), m.process_yuv_planar(*p2, out_dtype=torch.uint8))
    assert torch.equal(rgb(*p1), m.process_yuv_planar(*p1, out_dtype=torch.uint8))
