"""Pixel formats on the GPU (include/hdrnet_amd_pixel_formats.h): frames in BGR, RGBA and BGRA order through the fused
wire-format forward, the low-res gather, both single-level models and a captured graph.

The reference for almost everything here is the path that exists -- the same call on the frame repacked to RGB, its
uint8 output repacked back with the frame's alpha (tests/pixel_format_cases.py) -- and the bar is ``torch.equal``: the
arithmetic between the load and the store is the same code on the same values, so there is no tolerance.
``last_kernel()`` must carry the format's suffix, so a repack on the host cannot pass.  One independent anchor holds the
BGRA kernel against the CPU oracle at test_gpu_parity.py::test_wire_format_forward's own bar."""
import numpy as np
import pytest
import torch

import pixel_format_cases as px
from row_plan import row_plan

pytestmark = pytest.mark.gpu

GRID = (16, 16, 8)
# (2, 6, 1040): two segments of 520 px on 192 threads -- 62 idle lanes per workgroup, a second image, a segment that starts
# in mid-row.  (1, 5, 96): one segment, one partly filled wave.
SHAPES = [(2, 6, 1040), (1, 5, 96)]
WIRE = [("uint8", 255.0), ("uint16", 65535.0), ("uint16", 32767.0)]
GUIDES = ["map", "nn", "curves", "cells"]
GUIDE_LABEL = {"map": "", "nn": "+nnguide", "curves": "+curvesguide", "cells": "+curvesguide/cells"}
SHORT = {"uint8": "u8", "uint16": "u16", "float32": "f32"}


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
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.detach().cpu().numpy()


def _case(shape, dtype, wl):
    """Grid, guide map, guide parameters and, per format, a frame with the SAME colours and alpha (numpy; deterministic in
    its arguments, so that every format of a case shares one RGB reference)."""
    B, H, W = shape
    rng = np.random.default_rng([17, B, H, W, int(wl)])
    GH, GW, GD = GRID
    grid6 = np.zeros((B, GH, GW, GD, 3, 4), np.float32)  # close to identity: the output spans [0, 1] and beyond
    for i in range(3):
        grid6[..., i, i] = 1.0
    c = {"grid": (grid6 + 0.15 * rng.standard_normal(grid6.shape)).astype(np.float32).reshape(B, GH, GW, GD, 12),
         "guide": rng.random((B, H, W)).astype(np.float32),
         "conv1": (rng.standard_normal((16, 4)) * 0.8).astype(np.float32),
         "conv2": (rng.standard_normal(17) * 0.5).astype(np.float32),
         "ccm": (np.eye(3, 4) + 0.1 * rng.standard_normal((3, 4))).astype(np.float32),
         # 16 knots per channel, well apart (the prepared cell tables need >= 1/63 of the knot range between two)
         "shifts": (np.linspace(0.0, 0.9, 16)[:, None] + 0.01 * rng.random((16, 3))).astype(np.float32),
         "slopes": (0.3 * rng.standard_normal((16, 3))).astype(np.float32),
         "mix": np.array([0.4, 0.35, 0.3, 0.1], np.float32)}
    rgba = px.random_frame(rng, shape, "rgba", dtype, wl)
    c["frames"] = {"rgb": np.ascontiguousarray(rgba[..., :3]), "bgr": np.ascontiguousarray(rgba[..., 2::-1]),
                   "rgba": rgba, "bgra": np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])}
    c["alpha"] = np.ascontiguousarray(rgba[..., 3])
    return c


_CASES, _REFS = {}, {}


def case(shape, dtype, wl):
    key = (shape, dtype, wl)
    if key not in _CASES:
        _CASES[key] = _case(shape, dtype, wl)
        for fmt in px.FORMATS:  # the helper's to_rgb of every format's frame is the one RGB frame
            assert np.array_equal(px.to_rgb(_CASES[key]["frames"][fmt], fmt), _CASES[key]["frames"]["rgb"])
    return _CASES[key]


def guide_kw(ops, c, guide, dev):
    if guide == "map":
        return dict(guide=T(c["guide"], dev))
    if guide == "nn":
        return dict(guide_conv1=T(c["conv1"], dev), guide_conv2=T(c["conv2"], dev), return_guide=True)
    curves = tuple(T(c[k], dev) for k in ("ccm", "shifts", "slopes", "mix"))
    kw = dict(guide_curves=curves, return_guide=True)
    if guide == "cells":
        kw["curves_prepared"] = ops.curves_guide_prepare(curves[1], curves[2])
        assert kw["curves_prepared"] is not None, "the case's knots are apart: the cell tables are usable"
    return kw


def rgb_reference(ops, dev, shape, dtype, wl, out, guide):
    """The existing path on the RGB frame: (output, guide or None) in numpy, computed once per case and left alone."""
    key = (shape, dtype, wl, out, guide)
    if key not in _REFS:
        c = case(shape, dtype, wl)
        got = ops.bilateral_slice_apply_io(T(c["grid"], dev), T(c["frames"]["rgb"], dev), input_white_level=wl,
                                           out_dtype=getattr(torch, out), **guide_kw(ops, c, guide, dev))
        assert ops.last_kernel() == f"apply_fwd_io/{SHORT[dtype]}->{SHORT[out]}{GUIDE_LABEL[guide]}"  # RGB: no suffix
        o, g = got if isinstance(got, tuple) else (got, None)
        o, g = N(o), (None if g is None else N(g))
        for a in (o, g):
            if a is not None:
                a.setflags(write=False)
        _REFS[key] = (o, g)
    return _REFS[key]


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("out", ["uint8", "float32"])
@pytest.mark.parametrize("dtype,wl", WIRE)
@pytest.mark.parametrize("fmt", ["bgr", "rgba", "bgra"])
def test_bits_equal_the_rgb_path(dev, ops, fmt, dtype, wl, out, guide):
    for shape in SHAPES:
        c = case(shape, dtype, wl)
        want_rgb, want_guide = rgb_reference(ops, dev, shape, dtype, wl, out, guide)
        frame = c["frames"][fmt]
        got = ops.bilateral_slice_apply_io(T(c["grid"], dev), T(frame, dev), input_white_level=wl,
                                           out_dtype=getattr(torch, out), pixel_format=fmt, **guide_kw(ops, c, guide, dev))
        assert ops.last_kernel() == f"apply_fwd_io/{SHORT[dtype]}->{SHORT[out]}{GUIDE_LABEL[guide]}/{fmt}"
        o, g = got if isinstance(got, tuple) else (got, None)
        want = px.from_rgb(want_rgb, fmt, px.alpha_of(frame, fmt))
        assert tuple(o.shape) == want.shape and o.dtype == getattr(torch, out), (o.shape, want.shape)
        o = N(o)
        if not np.array_equal(o, want):
            bad = np.argwhere(o != want)
            raise AssertionError(f"{shape} {fmt} {dtype}/{wl} -> {out} {guide}: {len(bad)} of {o.size} samples differ, "
                                 f"first at {bad[0]}: got {o[tuple(bad[0])]}, want {want[tuple(bad[0])]}")
        if want_guide is not None:
            assert np.array_equal(N(g), want_guide), f"{shape} {fmt} {guide}: the guide the kernel computed differs"
        if out == "uint8" and shape == SHAPES[0]:
            assert o[..., :3].min() == 0 and o[..., :3].max() == 255  # the clip is exercised on both sides
            if px.CHANNELS[fmt] == 4:
                assert len(np.unique(o[..., 3])) > 100  # alpha is a plane of its own, not a constant


def test_bgra_against_the_cpu_oracle(dev, ops, port):
    """The independent anchor: bgra uint8 -> float32 with a guide map against the CPU oracle's slice-apply of the float RGB
    frame, at test_wire_format_forward's bar."""
    shape, dtype, wl = SHAPES[0], "uint8", 255.0
    c = case(shape, dtype, wl)
    inp_f = (px.to_rgb(c["frames"]["bgra"], "bgra").astype(np.float32) / np.float32(wl)).astype(np.float32)
    want = port.bilateral_slice_apply(c["grid"], c["guide"], inp_f, True)
    got = ops.bilateral_slice_apply_io(T(c["grid"], dev), T(c["frames"]["bgra"], dev), guide=T(c["guide"], dev),
                                       input_white_level=wl, out_dtype=torch.float32, pixel_format="bgra")
    assert ops.last_kernel() == "apply_fwd_io/u8->f32/bgra" and tuple(got.shape) == shape + (3,)
    np.testing.assert_allclose(N(got), want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("fmt", ["bgr", "bgra"])
def test_stores_stay_inside_the_buffer(dev, ops, fmt):
    """One raw C-ABI call per channel count into a pre-filled buffer with 256 guard bytes around it: every output byte is
    written (the whole buffer equals the expected frame, alpha in place) and the guards keep their fill."""
    from hdrnet_amd import _lib
    shape, dtype, wl, guard = SHAPES[0], "uint8", 255.0, 256
    B, H, W = shape
    S = px.CHANNELS[fmt]
    c = case(shape, dtype, wl)
    want_rgb, _ = rgb_reference(ops, dev, shape, dtype, wl, "uint8", "map")
    frame = c["frames"][fmt]
    want = px.from_rgb(want_rgb, fmt, px.alpha_of(frame, fmt))
    n = B * H * W * S
    grid, guide, inp = T(c["grid"], dev), T(c["guide"], dev), T(frame, dev)
    for fill in (0xA5, 0x5A):  # two fills: a byte that was never written cannot equal the expected one both times
        buf = torch.full((n + 2 * guard,), fill, dtype=torch.uint8, device=dev)
        out = buf[guard:guard + n]
        assert out.data_ptr() % 16 == 0
        rc = _lib.load().hdrnet_bilateral_slice_apply_io_px(
            grid.data_ptr(), guide.data_ptr(), inp.data_ptr(), out.data_ptr(), B, H, W, *GRID, 3, 3, 1, 1, wl, 1,
            None, None, 0, None, 0, px.CODE[fmt], px.CODE[fmt], torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0, _lib.last_error()
        assert _lib.last_kernel() == f"apply_fwd_io/u8->u8/{fmt}"
        got = buf.cpu().numpy()
        assert np.array_equal(got[guard:guard + n].reshape(want.shape), want)
        assert (got[:guard] == fill).all() and (got[guard + n:] == fill).all(), "a store left the output buffer"


@pytest.mark.parametrize("n", [256, 6, 5])  # 256 and 6: the vector store (n * n % 4 == 0); 5: the scalar tail
@pytest.mark.parametrize("dtype,wl", [("uint8", 255.0), ("uint16", 65535.0)])
@pytest.mark.parametrize("fmt", ["bgr", "rgba", "bgra"])
def test_lowres_input(dev, fmt, dtype, wl, n):
    from hdrnet_amd import _lib, data
    rng = np.random.default_rng([29, n])
    frame = px.random_frame(rng, (2, 37, 53), fmt, dtype, wl)
    want = data.lowres_input(T(px.to_rgb(frame, fmt), dev), n, wl)
    got = data.lowres_input(T(frame, dev), n, wl, pixel_format=fmt)
    assert _lib.last_kernel() == "sample_prep" and tuple(got.shape) == (2, n, n, 3)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert len(torch.unique(got)) > 8


def _model(cls, dev, seed=7):
    from hdrnet_amd import models
    torch.manual_seed(seed)
    return getattr(models, cls)(dict(batch_norm=False)).to(dev).eval()


@pytest.mark.parametrize("cls", ["HDRNetCurves", "HDRNetPointwiseNNGuide"])
def test_models_process(dev, ops, cls):
    from hdrnet_amd.runtime import FrameInference
    m = _model(cls, dev)
    rng = np.random.default_rng(43)
    shape = (1, 272, 480)
    label = "+curvesguide" if cls == "HDRNetCurves" else "+nnguide"
    # BGRA uint8 in, BGRA uint8 out, the frame's alpha
    first, second = (px.random_frame(rng, shape, "bgra", "uint8", 255.0) for _ in range(2))

    def want_u8(frame):
        rgb = m.process(T(px.to_rgb(frame, "bgra"), dev), out_dtype=torch.uint8)
        return px.from_rgb(N(rgb), "bgra", px.alpha_of(frame, "bgra"))

    got = m.process(T(first, dev), out_dtype=torch.uint8, pixel_format="bgra")
    assert ops.last_kernel().startswith("apply_fwd_io/u8->u8" + label) and ops.last_kernel().endswith("/bgra")
    assert got.dtype == torch.uint8 and tuple(got.shape) == shape + (4,)
    assert np.array_equal(N(got), want_u8(first))
    assert len(np.unique(N(got)[..., :3])) > 8  # a picture, not a constant
    # BGR uint16 at the HDR+ white level in, float32 (RGB) out
    f16 = px.random_frame(rng, shape, "bgr", "uint16", 32767.0)
    want16 = m.process(T(px.to_rgb(f16, "bgr"), dev), white_level=32767.0)
    got16 = m.process(T(f16, dev), white_level=32767.0, pixel_format="bgr")
    assert ops.last_kernel().startswith("apply_fwd_io/u16->f32" + label) and ops.last_kernel().endswith("/bgr")
    assert tuple(got16.shape) == shape + (3,)
    assert torch.equal(got16.view(torch.int32), want16.view(torch.int32))
    # a graph captured on one BGRA frame replays a second
    fi = FrameInference(m, T(first, dev), out_dtype=torch.uint8, pixel_format="bgra")
    assert torch.equal(fi(T(second, dev)), m.process(T(second, dev), out_dtype=torch.uint8, pixel_format="bgra"))
    assert np.array_equal(N(fi(T(second, dev))), want_u8(second))
    assert np.array_equal(N(fi(T(first, dev))), want_u8(first))
