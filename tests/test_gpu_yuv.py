"""YUV surfaces on the GPU (include/hdrnet_amd_yuv.h): NV12 / P010 / P016 planes through the conversion kernel, the low-res
gather, the fused wire-format forward with RGB and NV12 outputs, both single-level models and a captured graph.

The yardstick of the fused paths is the path that exists: ``bilateral_slice_apply_io`` on the float32 frame
``yuv_to_rgb`` writes, at ``torch.equal`` -- the conversion is one device function with explicit fmaf, and the arithmetic
behind it is the same code on the same values.  ``last_kernel()`` must carry the ``nv12`` / ``p016`` label, so a
conversion pass on the side cannot pass.  ``yuv_to_rgb`` itself is held against float64 (tests/yuv_cases.py) and one
anchor holds the NV12 kernel against the CPU oracle.  The NV12 output is held against the float64 encoder fed with the
float32 RGB output of the same call: equal wherever float64 decides the code by more than 1e-3, one code elsewhere."""
import numpy as np
import pytest
import torch

import yuv_cases as yc
from row_plan import row_plan

pytestmark = pytest.mark.gpu

GRID = (16, 16, 8)
# (2, 6, 1040): two segments of 520 px on 192 threads -- idle lanes, a second image, a segment that starts in mid-row,
# three row pairs.  (1, 4, 96): one segment, one partly filled wave, two row pairs.
SHAPES = [(2, 6, 1040), (1, 4, 96)]
PADS = [0, 64]  # tight pitch; pitch = row + 64 bytes, the padding poisoned
# (bits, standard, full range): NV12 BT.709 limited, P016 BT.601 full, P010 BT.709 limited
SURFACES = {"nv12": (8, "bt709", False), "p016": (16, "bt601", True), "p010": (10, "bt709", False)}
LABEL_IN = {"nv12": "nv12", "p016": "p016", "p010": "p016"}  # the kernels know sample widths, not bit depths
GUIDES = ["map", "nn", "curves", "cells", "scan"]
GUIDE_LABEL = {"map": "", "nn": "+nnguide", "curves": "+curvesguide", "cells": "+curvesguide/cells",
               "scan": "+curvesguide/scan"}
SHORT = {"uint8": "u8", "float32": "f32"}


def test_the_shapes_are_what_the_comment_says():
    assert row_plan(1040) == (192, 2, 520) and 192 - 520 // 4 == 62
    assert row_plan(96) == (64, 1, 96)


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
    from hdrnet_amd import yuv
    bits, standard, full = SURFACES[kind]
    to_rgb, from_rgb = yuv.yuv_coefficients(standard, full, bits)
    return to_rgb, from_rgb, T(to_rgb, dev), T(from_rgb, dev)


_CASES, _REFS = {}, {}


def case(shape, kind):
    """Grid, guide parameters and ONE surface content per (shape, kind), as numpy buffers per pitch: the padded buffers
    hold the same samples as the tight ones, so every pitch shares the references."""
    key = (shape, kind)
    if key not in _CASES:
        B, H, W = shape
        bits = SURFACES[kind][0]
        rng = np.random.default_rng([23, B, H, W, bits])
        GH, GW, GD = GRID
        grid6 = np.zeros((B, GH, GW, GD, 3, 4), np.float32)  # close to identity: the output spans [0, 1] and beyond
        for i in range(3):
            grid6[..., i, i] = 1.0
        c = {"grid": (grid6 + 0.15 * rng.standard_normal(grid6.shape)).astype(np.float32).reshape(B, GH, GW, GD, 12),
             "guide": rng.random((B, H, W)).astype(np.float32),
             "conv1": (rng.standard_normal((16, 4)) * 0.8).astype(np.float32),
             "conv2": (rng.standard_normal(17) * 0.5).astype(np.float32),
             "ccm": (np.eye(3, 4) + 0.1 * rng.standard_normal((3, 4))).astype(np.float32),
             "shifts": (np.linspace(0.0, 0.9, 16)[:, None] + 0.01 * rng.random((16, 3))).astype(np.float32),
             "slopes": (0.3 * rng.standard_normal((16, 3))).astype(np.float32),
             "shifts20": (np.linspace(0.0, 0.95, 20)[:, None] + 0.01 * rng.random((20, 3))).astype(np.float32),
             "slopes20": (0.25 * rng.standard_normal((20, 3))).astype(np.float32),
             "mix": np.array([0.4, 0.35, 0.3, 0.1], np.float32)}
        y, uv = yc.random_surface(rng, shape, bits)
        c["y"], c["uv"] = y, uv
        c["bufs"] = {}
        for pad in PADS:
            size = y.itemsize
            by, buv = yc.random_surface(rng, shape, bits, pad_bytes=pad)  # for its poisoned padding ...
            by[:, :, :W], buv[:, :, :W] = y, uv                           # ... around the case's samples
            assert by.shape[2] * size == W * size + pad
            c["bufs"][pad] = (by, buv)
        _CASES[key] = c
    return _CASES[key]


def planes(c, pad, W, dev):
    """The device planes of one pitch: views of the padded buffers (row stride > W for pad > 0)."""
    by, buv = c["bufs"][pad]
    ty, tuv = T(by, dev), T(buv, dev)
    return ty[:, :, :W], tuv[:, :, :W]


def guide_kw(ops, c, guide, dev):
    if guide == "map":
        return dict(guide=T(c["guide"], dev))
    if guide == "nn":
        return dict(guide_conv1=T(c["conv1"], dev), guide_conv2=T(c["conv2"], dev), return_guide=True)
    names = ("ccm", "shifts20", "slopes20", "mix") if guide == "scan" else ("ccm", "shifts", "slopes", "mix")
    curves = tuple(T(c[k], dev) for k in names)
    kw = dict(guide_curves=curves, return_guide=True)
    if guide == "cells":
        kw["curves_prepared"] = ops.curves_guide_prepare(curves[1], curves[2])
        assert kw["curves_prepared"] is not None, "the case's knots are apart: the cell tables are usable"
    return kw


def rgb_frame(ops, dev, shape, kind):
    """``yuv_to_rgb`` of the case's tight surface, float32 on the device: computed once, the input of every reference."""
    key = ("frame", shape, kind)
    if key not in _REFS:
        c = case(shape, kind)
        _, _, k, _ = constants(kind, dev)
        _REFS[key] = ops.yuv_to_rgb(T(c["y"], dev), T(c["uv"], dev), k)
        assert ops.last_kernel() == "yuv_to_rgb"
    return _REFS[key]


def rgb_reference(ops, dev, shape, kind, out, guide):
    """The existing path on the converted float32 frame: (output, guide or None) in numpy, once per case."""
    key = (shape, kind, out, guide)
    if key not in _REFS:
        c = case(shape, kind)
        got = ops.bilateral_slice_apply_io(T(c["grid"], dev), rgb_frame(ops, dev, shape, kind), out_dtype=getattr(torch, out),
                                           **guide_kw(ops, c, guide, dev))
        assert ops.last_kernel() == f"apply_fwd_io/f32->{SHORT[out]}{GUIDE_LABEL[guide]}"
        o, g = got if isinstance(got, tuple) else (got, None)
        o, g = N(o), (None if g is None else N(g))
        for a in (o, g):
            if a is not None:
                a.setflags(write=False)
        _REFS[key] = (o, g)
    return _REFS[key]


# ---- 1. the conversion against float64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SURFACES))
def test_yuv_to_rgb(dev, ops, kind):
    """atol 2e-6: three fused operations on magnitudes below 4, each within half an ulp <= 2.4e-7, on the same float32
    constants.  The surfaces' corners hold super-black and super-white codes: the clamp is exercised."""
    to_rgb, _, k, _ = constants(kind, dev)
    for shape in SHAPES:
        c = case(shape, kind)
        want = yc.to_rgb64(c["y"], c["uv"], to_rgb)
        assert want.min() == 0.0 and want.max() == 1.0  # both sides of the clamp are reached ...
        # ... at the corners too: the lowest and the highest code under neutral chroma (full range: white is the top code)
        assert np.all(want[:, 0, 0] == 0.0) and np.all(want[:, 0, -1] >= 1.0 - 1e-6)
        for pad in PADS:
            y, uv = planes(c, pad, shape[2], dev)
            got = ops.yuv_to_rgb(y, uv, k)
            assert ops.last_kernel() == "yuv_to_rgb" and tuple(got.shape) == shape + (3,) and got.dtype == torch.float32
            g = N(got)
            err = np.abs(g - want).max()
            print(f"yuv_to_rgb {kind} {shape} pad {pad}: max |err| = {err:.3g}")
            np.testing.assert_allclose(g, want, rtol=0, atol=2e-6)
            assert g.min() == 0.0 and g.max() == 1.0
            if pad == 0:
                tight = g
            else:
                assert np.array_equal(g, tight), "a pitched surface converts to other bits than the tight one"


# ---- 2. bit equality of the fused forward with the conversion followed by the RGB forward --------------------------------
@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("out", ["uint8", "float32"])
@pytest.mark.parametrize("kind", ["nv12", "p016"])
def test_bits_equal_convert_then_rgb(dev, ops, kind, out, guide):
    _, _, k, _ = constants(kind, dev)
    for shape in SHAPES:
        c = case(shape, kind)
        want, want_guide = rgb_reference(ops, dev, shape, kind, out, guide)
        for pad in PADS:
            y, uv = planes(c, pad, shape[2], dev)
            got = ops.bilateral_slice_apply_io_yuv(T(c["grid"], dev), y, uv, k, out="rgb", out_dtype=getattr(torch, out),
                                                   **guide_kw(ops, c, guide, dev))
            assert ops.last_kernel() == f"apply_fwd_io/{LABEL_IN[kind]}->{SHORT[out]}{GUIDE_LABEL[guide]}"
            o, g = got if isinstance(got, tuple) else (got, None)
            assert tuple(o.shape) == want.shape and o.dtype == getattr(torch, out)
            o = N(o)
            same = np.array_equal(o.view(np.uint32), want.view(np.uint32)) if out == "float32" else np.array_equal(o, want)
            if not same:
                bad = np.argwhere(o != want)
                raise AssertionError(f"{shape} {kind} pad {pad} -> {out} {guide}: {len(bad)} of {o.size} samples differ, "
                                     f"first at {bad[0]}: got {o[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")
            if want_guide is not None:
                assert np.array_equal(N(g), want_guide), f"{shape} {kind} {guide}: the guide the kernel computed differs"
            if out == "uint8" and shape == SHAPES[0]:
                assert o.min() == 0 and o.max() == 255  # the clip is exercised on both sides


# ---- 3. the low-res gather -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 6, 5])  # 256 and 6: the vector store (n * n % 4 == 0); 5: the scalar tail
@pytest.mark.parametrize("kind", ["nv12", "p010"])
def test_lowres_input_yuv(dev, ops, kind, n):
    from hdrnet_amd import _lib, data
    bits = SURFACES[kind][0]
    _, _, k, _ = constants(kind, dev)
    rng = np.random.default_rng([29, n, bits])
    shape = (2, 38, 52)
    by, buv = yc.random_surface(rng, shape, bits, pad_bytes=64)
    y, uv = T(by, dev)[:, :, :52], T(buv, dev)[:, :, :52]
    want = data.lowres_input(ops.yuv_to_rgb(y, uv, k), n)
    got = data.lowres_input_yuv(y, uv, k, n)
    assert _lib.last_kernel() == "sample_prep" and tuple(got.shape) == (2, n, n, 3)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert len(torch.unique(got)) > 8


# ---- 4. NV12 out ---------------------------------------------------------------------------------------------------------
GUARD = 4096


def _out_surface(shape, pad, dev, fill):
    """Poisoned output planes with ``pad`` bytes of row padding and a GUARD behind each plane: (flat buffers, views)."""
    B, H, W = shape
    pitch = W + pad
    flats, views = [], []
    for rows in (H, H // 2):
        flat = torch.full((B * rows * pitch + GUARD,), fill, dtype=torch.uint8, device=dev)
        flats.append(flat)
        views.append(flat[:B * rows * pitch].view(B, rows, pitch)[:, :, :W])
    return flats, views


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("kind", ["nv12", "p016"])
def test_nv12_output(dev, ops, kind, guide):
    _, from_rgb, k_in, k_out = constants(kind, dev)
    refs, undecided, total = {}, 0, 0
    for shape in SHAPES:
        rgb, want_guide = rgb_reference(ops, dev, shape, kind, "float32", guide)  # pinned by the bit-equality test
        yq, uvq, y_pre, uv_pre = yc.encode_nv12_64(rgb, from_rgb)
        dy, duv = yc.decided(y_pre), yc.decided(uv_pre)
        refs[shape] = (want_guide, yq, uvq, dy, duv)
        undecided += int((~dy).sum() + (~duv).sum())
        total += dy.size + duv.size
    # from the reference alone: what the comparison below lets differ by a code is a small share of the test's samples
    assert undecided < 0.01 * total, f"{undecided} of the reference's {total} samples lie within 1e-3 of a code boundary"
    for shape in SHAPES:
        B, H, W = shape
        c = case(shape, kind)
        want_guide, yq, uvq, dy, duv = refs[shape]
        if shape == SHAPES[0]:
            assert len(np.unique(yq)) > 100 and len(np.unique(uvq)) > 50  # a picture, not a constant
        for pad in PADS:
            y, uv = planes(c, pad, W, dev)
            for fill in ((yc.POISON,) if pad == 0 else (yc.POISON, 0x5A)):
                flats, (oy, ouv) = _out_surface(shape, pad, dev, fill)
                got = ops.bilateral_slice_apply_io_yuv(T(c["grid"], dev), y, uv, k_in, out="nv12", from_rgb=k_out,
                                                       out_planes=(oy, ouv), **guide_kw(ops, c, guide, dev))
                assert ops.last_kernel() == f"apply_fwd_io/{LABEL_IN[kind]}->nv12{GUIDE_LABEL[guide]}"
                (ry, ruv), g = got if want_guide is not None else (got, None)
                assert ry.data_ptr() == oy.data_ptr() and ruv.data_ptr() == ouv.data_ptr()
                for name, plane, want, dec in (("Y", N(oy), yq, dy), ("UV", N(ouv), uvq, duv)):
                    diff = np.abs(plane.astype(np.int32) - want.astype(np.int32))
                    print(f"nv12 out {kind} {guide} {shape} pad {pad} {name}: {int((diff > 0).sum())} of {diff.size} differ, "
                          f"max {int(diff.max())}; undecided {int((~dec).sum())}")
                    assert np.array_equal(plane[dec], want[dec]), f"{name}: a sample float64 decides by > 1e-3 differs"
                    assert diff.max() <= 1, f"{name}: off by more than one code"
                if g is not None:
                    assert np.array_equal(N(g), want_guide)
                # padding and the guard behind each plane keep their fill
                for flat, rows in zip(flats, (H, H // 2)):
                    whole = flat.cpu().numpy()
                    body = whole[:B * rows * (W + pad)].reshape(B, rows, W + pad)
                    assert (body[:, :, W:] == fill).all(), "a store went into the row padding"
                    assert (whole[B * rows * (W + pad):] == fill).all(), "a store left the output plane"


def test_nv12_output_allocates_tight_planes(dev, ops):
    shape, kind = SHAPES[1], "nv12"
    B, H, W = shape
    c = case(shape, kind)
    _, _, k_in, k_out = constants(kind, dev)
    y, uv = planes(c, 0, W, dev)
    oy, ouv = ops.bilateral_slice_apply_io_yuv(T(c["grid"], dev), y, uv, k_in, guide=T(c["guide"], dev), out="nv12",
                                               from_rgb=k_out)
    _, (py, puv) = _out_surface(shape, 64, dev, 0x5A)
    ops.bilateral_slice_apply_io_yuv(T(c["grid"], dev), y, uv, k_in, guide=T(c["guide"], dev), out="nv12", from_rgb=k_out,
                                     out_planes=(py, puv))
    assert tuple(oy.shape) == (B, H, W) and tuple(ouv.shape) == (B, H // 2, W) and oy.is_contiguous()
    assert torch.equal(oy, py) and torch.equal(ouv, puv)


# ---- 5. the models and the captured graph -------------------------------------------------------------------------------
def _model(cls, dev, seed=7):
    from hdrnet_amd import models
    torch.manual_seed(seed)
    return getattr(models, cls)(dict(batch_norm=False)).to(dev).eval()


@pytest.mark.parametrize("cls", ["HDRNetCurves", "HDRNetPointwiseNNGuide"])
def test_models_process_yuv(dev, ops, cls):
    from hdrnet_amd import data, yuv
    from hdrnet_amd.runtime import YuvFrameInference
    m = _model(cls, dev)
    rng = np.random.default_rng(47)
    shape = (1, 272, 480)
    W = shape[2]
    label = "+curvesguide" if cls == "HDRNetCurves" else "+nnguide"
    (y1, uv1), (y2, uv2) = (tuple(T(a, dev) for a in yc.random_surface(rng, shape, 8, corners=False)) for _ in range(2))
    to_rgb, from_rgb = (T(a, dev) for a in yuv.yuv_coefficients("bt709", False, 8))

    def composed(y, uv, k_in, **kw):
        coeffs = m.coefficients(data.lowres_input_yuv(y, uv, k_in, m.params["net_input_size"]))
        gs = coeffs.shape
        return ops.bilateral_slice_apply_io_yuv(coeffs.reshape(gs[0], gs[1], gs[2], gs[3], gs[4] * gs[5]), y, uv, k_in,
                                                **kw, **m._process_guide_args())

    with torch.no_grad():
        # NV12 in, NV12 out
        gy, guv = m.process_yuv(y1, uv1, out="nv12")
        assert ops.last_kernel().startswith("apply_fwd_io/nv12->nv12" + label)
        wy, wuv = composed(y1, uv1, to_rgb, out="nv12", from_rgb=from_rgb)
        assert torch.equal(gy, wy) and torch.equal(guv, wuv) and len(torch.unique(gy)) > 8
        # ... the float32 frame equals process() of the converted frame's pieces
        got = m.process_yuv(y1, uv1)
        assert ops.last_kernel().startswith("apply_fwd_io/nv12->f32" + label) and tuple(got.shape) == shape + (3,)
        assert torch.equal(got.view(torch.int32), composed(y1, uv1, to_rgb, out="rgb").view(torch.int32))
        # P010, BT.2020, full range, uint8 RGB out
        y10, uv10 = (T(a, dev) for a in yc.random_surface(rng, shape, 10, corners=False))
        k10 = T(yuv.yuv_coefficients("bt2020", True, 10)[0], dev)
        got10 = m.process_yuv(y10, uv10, standard="bt2020", full_range=True, bits=10, out_dtype=torch.uint8)
        assert ops.last_kernel().startswith("apply_fwd_io/p016->u8" + label) and got10.dtype == torch.uint8
        assert torch.equal(got10, composed(y10, uv10, k10, out="rgb", out_dtype=torch.uint8))
    # a graph captured on one surface replays another, copied in -- and a third time after the static planes were
    # overwritten in place, as a decoder would
    fi = YuvFrameInference(m, y1, uv1, out="nv12")
    want2 = [t.clone() for t in m.process_yuv(y2, uv2, out="nv12")]
    ry, ruv = fi(y2, uv2)
    assert torch.equal(ry, want2[0]) and torch.equal(ruv, want2[1])
    sy, suv = fi.static_inputs
    sy.copy_(y1)
    suv.copy_(uv1)
    ry, ruv = fi(sy, suv)
    assert torch.equal(ry, gy) and torch.equal(ruv, guv)
    assert not torch.equal(ry, want2[0])
    rgb = YuvFrameInference(m, y1, uv1, out="rgb", out_dtype=torch.uint8)
    assert torch.equal(rgb(y2, uv2), m.process_yuv(y2, uv2, out_dtype=torch.uint8))


# ---- 6. one independent anchor -------------------------------------------------------------------------------------------
def test_nv12_against_the_cpu_oracle(dev, ops, port):
    """NV12 uint8 -> float32 RGB with a guide map against the CPU oracle's slice-apply of the helper's float64-converted
    frame, at test_gpu_parity.py::test_wire_format_forward's bar."""
    shape, kind = SHAPES[0], "nv12"
    c = case(shape, kind)
    to_rgb, _, k, _ = constants(kind, dev)
    inp_f = yc.to_rgb64(c["y"], c["uv"], to_rgb).astype(np.float32)
    want = port.bilateral_slice_apply(c["grid"], c["guide"], inp_f, True)
    y, uv = planes(c, 64, shape[2], dev)
    got = ops.bilateral_slice_apply_io_yuv(T(c["grid"], dev), y, uv, k, guide=T(c["guide"], dev))
    assert ops.last_kernel() == "apply_fwd_io/nv12->f32" and tuple(got.shape) == shape + (3,)
    np.testing.assert_allclose(N(got), want, rtol=1e-5, atol=1e-5)
