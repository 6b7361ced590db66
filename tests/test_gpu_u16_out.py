"""16-bit output on the GPU (include/hdrnet_amd_u16_out.h): the fused wire-format forward storing a uint16 frame or a
P010 / P016 surface, both single-level models and the captured graphs.

The yardstick of the frame store is the path that exists: the float32 output ``f`` of ``bilateral_slice_apply_io`` on the
same inputs, quantised on the host by the store's rule, ``(np.float32(wl) * np.clip(f, 0, 1)).astype(np.uint16)``, at
``torch.equal`` -- the arithmetic before the store is the same code on the same values, so there is no tolerance.
``last_kernel()`` must carry ``->u16`` and the format's suffix, so a quantisation pass on the side cannot pass.  One
independent anchor holds the store against the CPU oracle.  The surface store is held against a float64 encoder
(tests/u16_out_cases.py) fed with the float32 RGB output of the existing ``out="rgb"`` path on the same surface."""
import numpy as np
import pytest
import torch

import pixel_format_cases as px
import u16_out_cases as uc
import yuv_cases as yc
from row_plan import row_plan

pytestmark = pytest.mark.gpu

GRID = (16, 16, 8)
# (2, 6, 1040): two segments of 520 px on 192 threads -- 62 idle lanes per workgroup, a second image, a segment that starts
# in mid-row, three row pairs.  (1, 4, 96): one segment, one partly filled wave, two row pairs.
SHAPES = [(2, 6, 1040), (1, 4, 96)]
FRAMES = [("uint16", 65535.0), ("uint16", 32767.0), ("float32", 1.0)]
OUT_WHITE = [65535.0, 32767.0, 1023.0]
GUIDES = ["map", "nn", "curves", "cells", "scan"]
GUIDE_LABEL = {"map": "", "nn": "+nnguide", "curves": "+curvesguide", "cells": "+curvesguide/cells",
               "scan": "+curvesguide/scan"}
SHORT = {"uint16": "u16", "float32": "f32"}
# every (frame, pixel format, guide form) that is instantiated: uint16 and float32 RGB frames with the five guide forms,
# uint16 BGR / RGBA / BGRA frames with the four the packed formats have
INSTANTIATED = ([(d, wl, "rgb", g) for d, wl in FRAMES for g in GUIDES] +
                [(d, wl, f, g) for d, wl in FRAMES[:2] for f in ("bgr", "rgba", "bgra") for g in GUIDES[:4]])


def test_the_shapes_are_what_the_comment_says():
    assert row_plan(1040) == (192, 2, 520) and 192 - 520 // 4 == 62
    assert row_plan(96) == (64, 1, 96)
    assert len(INSTANTIATED) == 15 + 24


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


def _guides(rng, shape):
    """Grid (near identity + 0.15 sigma noise: the output spans [0, 1] and beyond, both clips are hit), a guide map and
    the parameters of every guide form."""
    B, H, W = shape
    GH, GW, GD = GRID
    grid6 = np.zeros((B, GH, GW, GD, 3, 4), np.float32)
    for i in range(3):
        grid6[..., i, i] = 1.0
    return {"grid": (grid6 + 0.15 * rng.standard_normal(grid6.shape)).astype(np.float32).reshape(B, GH, GW, GD, 12),
            "guide": rng.random((B, H, W)).astype(np.float32),
            "conv1": (rng.standard_normal((16, 4)) * 0.8).astype(np.float32),
            "conv2": (rng.standard_normal(17) * 0.5).astype(np.float32),
            "ccm": (np.eye(3, 4) + 0.1 * rng.standard_normal((3, 4))).astype(np.float32),
            # 16 knots per channel, well apart (the prepared cell tables need >= 1/63 of the knot range between two)
            "shifts": (np.linspace(0.0, 0.9, 16)[:, None] + 0.01 * rng.random((16, 3))).astype(np.float32),
            "slopes": (0.3 * rng.standard_normal((16, 3))).astype(np.float32),
            "shifts20": (np.linspace(0.0, 0.95, 20)[:, None] + 0.01 * rng.random((20, 3))).astype(np.float32),
            "slopes20": (0.25 * rng.standard_normal((20, 3))).astype(np.float32),
            "mix": np.array([0.4, 0.35, 0.3, 0.1], np.float32)}


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


_CASES, _REFS = {}, {}


def frame_case(shape, dtype, wl):
    """Per format, a frame with the SAME colours and alpha (numpy; deterministic in its arguments)."""
    key = ("frame", shape, dtype, wl)
    if key not in _CASES:
        B, H, W = shape
        rng = np.random.default_rng([31, B, H, W, int(wl)])
        c = _guides(rng, shape)
        if dtype == "float32":
            c["frames"] = {"rgb": rng.random(shape + (3,)).astype(np.float32)}
        else:
            rgba = px.random_frame(rng, shape, "rgba", dtype, wl)
            c["frames"] = {"rgb": np.ascontiguousarray(rgba[..., :3]), "bgr": np.ascontiguousarray(rgba[..., 2::-1]),
                           "rgba": rgba, "bgra": np.ascontiguousarray(rgba[..., [2, 1, 0, 3]])}
            for fmt in px.FORMATS:
                assert np.array_equal(px.to_rgb(c["frames"][fmt], fmt), c["frames"]["rgb"])
        _CASES[key] = c
    return _CASES[key]


def f32_reference(ops, dev, shape, dtype, wl, fmt, guide):
    """The EXISTING entry point on the same inputs, float32 out: (RGB output, guide or None) in numpy, once per case."""
    key = (shape, dtype, wl, fmt, guide)
    if key not in _REFS:
        c = frame_case(shape, dtype, wl)
        got = ops.bilateral_slice_apply_io(T(c["grid"], dev), T(c["frames"][fmt], dev), input_white_level=wl,
                                           out_dtype=torch.float32, pixel_format=fmt, **guide_kw(ops, c, guide, dev))
        assert ops.last_kernel() == f"apply_fwd_io/{SHORT[dtype]}->f32{GUIDE_LABEL[guide]}" + ("" if fmt == "rgb" else "/" + fmt)
        o, g = got if isinstance(got, tuple) else (got, None)
        o, g = N(o), (None if g is None else N(g))
        assert o.dtype == np.float32 and o.shape == shape + (3,)
        for a in (o, g):
            if a is not None:
                a.setflags(write=False)
        _REFS[key] = (o, g)
    return _REFS[key]


# ---- 1. the frame store, exact -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,wl,fmt,guide", INSTANTIATED)
def test_frame_store_equals_the_quantised_f32_path(dev, ops, dtype, wl, fmt, guide):
    for shape in SHAPES:
        c = frame_case(shape, dtype, wl)
        f, want_guide = f32_reference(ops, dev, shape, dtype, wl, fmt, guide)
        frame = c["frames"][fmt]
        for wl_out in OUT_WHITE:
            want = uc.quantise_u16(f, wl_out)
            got = ops.bilateral_slice_apply_io_u16(T(c["grid"], dev), T(frame, dev), input_white_level=wl,
                                                   output_white_level=wl_out, pixel_format=fmt, **guide_kw(ops, c, guide, dev))
            assert ops.last_kernel() == (f"apply_fwd_io/{SHORT[dtype]}->u16{GUIDE_LABEL[guide]}" +
                                         ("" if fmt == "rgb" else "/" + fmt))
            o, g = got if isinstance(got, tuple) else (got, None)
            assert o.dtype == torch.uint16 and tuple(o.shape) == shape + (px.CHANNELS[fmt],), (o.dtype, o.shape)
            o = N(o)
            colour = px.to_rgb(o, fmt)  # the output repacked to RGB: the permutation is the input's
            if not np.array_equal(colour, want):
                bad = np.argwhere(colour != want)
                raise AssertionError(f"{shape} {fmt} {dtype}/{wl} -> u16/{wl_out} {guide}: {len(bad)} of {want.size} samples "
                                     f"differ, first at {bad[0]}: got {colour[tuple(bad[0])]}, want {want[tuple(bad[0])]}")
            if px.CHANNELS[fmt] == 4:  # alpha: the input's, bit for bit
                assert np.array_equal(px.alpha_of(o, fmt), px.alpha_of(frame, fmt))
                assert len(np.unique(px.alpha_of(o, fmt))) > 100
            # ... which is what from_rgb's repacking of a uint8 output does, with the uint16 alpha as it is
            if want_guide is not None:
                assert np.array_equal(N(g), want_guide), f"{shape} {fmt} {guide}: the guide the kernel computed differs"
            if shape == SHAPES[0]:
                assert want.min() == 0 and want.max() == int(wl_out)  # both clips are hit (from the reference alone) ...
                assert colour.min() == 0 and colour.max() == int(wl_out)


# ---- 2. the frame store, independent anchor ------------------------------------------------------------------------------
def test_frame_store_against_the_cpu_oracle(dev, ops, port):
    """uint16 / 32767 -> uint16 / 32767 with a guide map against the CPU oracle's slice-apply of the float frame, at
    test_gpu_parity.py::test_wire_format_forward's bar: rtol = atol = 1e-5 on values in [0, 1] is at most 2e-5 of the float
    result, i.e. ceil(32767 * 2e-5) = 1 code of the truncated product."""
    shape, dtype, wl = SHAPES[0], "uint16", 32767.0
    c = frame_case(shape, dtype, wl)
    inp_f = (c["frames"]["rgb"].astype(np.float32) / np.float32(wl)).astype(np.float32)
    want_f = port.bilateral_slice_apply(c["grid"], c["guide"], inp_f, True)
    want = np.trunc(np.float64(wl) * np.clip(want_f.astype(np.float64), 0.0, 1.0))
    bound = int(np.ceil(wl * 2e-5))
    assert bound == 1
    got = ops.bilateral_slice_apply_io_u16(T(c["grid"], dev), T(c["frames"]["rgb"], dev), guide=T(c["guide"], dev),
                                           input_white_level=wl, output_white_level=wl)
    assert ops.last_kernel() == "apply_fwd_io/u16->u16" and got.dtype == torch.uint16 and tuple(got.shape) == shape + (3,)
    diff = np.abs(N(got).astype(np.float64) - want)
    print(f"u16 -> u16 / 32767 against the oracle: {int((diff > 0).sum())} of {diff.size} differ, max {diff.max():.0f} code")
    assert diff.max() <= bound
    assert want.min() == 0 and want.max() == wl


# ---- 3. the output's bounds ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb", "bgra"])
def test_stores_stay_inside_the_buffer(dev, ops, fmt):
    """One raw C-ABI call per channel count into a pre-filled buffer with guard elements around it: every output sample is
    written (the whole buffer equals the expected frame, alpha in place) and the guards keep their fill."""
    from hdrnet_amd import _lib
    shape, dtype, wl, wl_out, guard = SHAPES[0], "uint16", 65535.0, 32767.0, 128  # 128 uint16 = 256 bytes: 16-B aligned
    B, H, W = shape
    S = px.CHANNELS[fmt]
    c = frame_case(shape, dtype, wl)
    f, _ = f32_reference(ops, dev, shape, dtype, wl, fmt, "map")
    frame = c["frames"][fmt]
    want_rgb = uc.quantise_u16(f, wl_out)
    n = B * H * W * S
    grid, guide, inp = T(c["grid"], dev), T(c["guide"], dev), T(frame, dev)
    for fill in (0xA5A5, 0x5A5A):  # two fills: a sample that was never written cannot equal the expected one both times
        buf = torch.full((n + 2 * guard,), fill - 65536 if fill > 32767 else fill, dtype=torch.int16, device=dev).view(torch.uint16)
        out = buf[guard:guard + n]
        assert out.data_ptr() % 16 == 0
        rc = _lib.load().hdrnet_bilateral_slice_apply_io_px_u16(
            grid.data_ptr(), guide.data_ptr(), inp.data_ptr(), out.data_ptr(), B, H, W, *GRID, 3, 3, 1, 2, wl, wl_out,
            None, None, 0, None, 0, px.CODE[fmt], px.CODE[fmt], torch.cuda.current_stream(dev).cuda_stream)
        assert rc == 0, _lib.last_error()
        assert _lib.last_kernel() == "apply_fwd_io/u16->u16" + ("" if fmt == "rgb" else "/" + fmt)
        got = N(buf)
        body = got[guard:guard + n].reshape(shape + (S,))
        assert np.array_equal(px.to_rgb(body, fmt), want_rgb)
        if S == 4:
            assert np.array_equal(px.alpha_of(body, fmt), px.alpha_of(frame, fmt))
        assert (got[:guard] == fill).all() and (got[guard + n:] == fill).all(), "a store left the output buffer"


# ---- 4. the P010 / P016 store --------------------------------------------------------------------------------------------
PADS = [0, 64]  # tight pitch; pitch = row + 64 bytes, the padding filled
# (bits in = bits out, standard, full range): P010 BT.709 limited, P016 BT.601 full
SURFACES = {"p010": (10, "bt709", False), "p016": (16, "bt601", True)}
GUARD = 2048  # uint16 elements behind each plane


def surface_constants(kind, dev):
    from hdrnet_amd import yuv
    bits, standard, full = SURFACES[kind]
    to_rgb = yuv.yuv_coefficients(standard, full, bits)[0]
    from_rgb = yuv.yuv_encode_coefficients(standard, full, bits)
    return from_rgb, T(to_rgb, dev), T(from_rgb, dev)


def surface_case(shape, kind):
    key = ("surface", shape, kind)
    if key not in _CASES:
        B, H, W = shape
        bits = SURFACES[kind][0]
        rng = np.random.default_rng([37, B, H, W, bits])
        c = _guides(rng, shape)
        y, uv = yc.random_surface(rng, shape, bits)
        c["bufs"] = {}
        for pad in PADS:
            by, buv = yc.random_surface(rng, shape, bits, pad_bytes=pad)  # for its poisoned padding ...
            by[:, :, :W], buv[:, :, :W] = y, uv                           # ... around the case's samples
            c["bufs"][pad] = (by, buv)
        _CASES[key] = c
    return _CASES[key]


def planes(c, pad, W, dev):
    by, buv = c["bufs"][pad]
    return T(by, dev)[:, :, :W], T(buv, dev)[:, :, :W]


def surface_rgb_reference(ops, dev, shape, kind, guide):
    """The existing ``out="rgb"`` float32 path on the same (tight) surface -- itself pinned bit for bit by
    tests/test_gpu_yuv.py: (RGB frame, guide or None) in numpy, once per case."""
    key = ("surface", shape, kind, guide)
    if key not in _REFS:
        c = surface_case(shape, kind)
        _, k_in, _ = surface_constants(kind, dev)
        y, uv = planes(c, 0, shape[2], dev)
        got = ops.bilateral_slice_apply_io_yuv(T(c["grid"], dev), y, uv, k_in, out="rgb", **guide_kw(ops, c, guide, dev))
        assert ops.last_kernel() == f"apply_fwd_io/p016->f32{GUIDE_LABEL[guide]}"
        o, g = got if isinstance(got, tuple) else (got, None)
        o, g = N(o), (None if g is None else N(g))
        for a in (o, g):
            if a is not None:
                a.setflags(write=False)
        _REFS[key] = (o, g)
    return _REFS[key]


def _out_surface(shape, pad, dev, fill):
    """Pre-filled uint16 output planes with ``pad`` bytes of row padding and a GUARD behind each plane: (flats, views)."""
    B, H, W = shape
    pitch = W + pad // 2
    flats, views = [], []
    for rows in (H, H // 2):
        flat = torch.full((B * rows * pitch + GUARD,), fill - 65536 if fill > 32767 else fill, dtype=torch.int16,
                          device=dev).view(torch.uint16)
        flats.append(flat)
        views.append(flat[:B * rows * pitch].view(B, rows, pitch)[:, :, :W])
    return flats, views


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("kind", list(SURFACES))
def test_p016_output(dev, ops, kind, guide):
    """P010 in -> P010 out and P016 in -> P016 out against the float64 encoder of the header's rule.  The low 16 - out_bits
    bits of every sample are zero, no sample is off by more than one code, and a sample is EQUAL wherever float64 decides
    its code by more than eps = 1e-3 * 2^(out_bits - 8) -- tests/yuv_cases.py's margin at the same number of float32 ulps of
    the code range.  How many samples that leaves undecided follows from the reference alone, before the kernel's output is
    looked at: at 10 bits fewer than 2 % (a uniform fraction gives 2 eps = 0.8 %); at 16 bits float32 cannot resolve more
    (2 eps = 51 %): there at least 40 % must be decided -- and equal -- and the rest relies on the one-code bound."""
    bits = SURFACES[kind][0]
    from_rgb, k_in, k_out = surface_constants(kind, dev)
    low_bits = (1 << uc.stored_shift(bits)) - 1
    refs, undecided, total = {}, 0, 0
    for shape in SHAPES:
        rgb, want_guide = surface_rgb_reference(ops, dev, shape, kind, guide)
        yq, uvq, y_pre, uv_pre = uc.encode_p016_64(rgb, from_rgb, bits)
        dy, duv = uc.decided(y_pre, bits), uc.decided(uv_pre, bits)
        refs[shape] = (want_guide, yq, uvq, dy, duv)
        undecided += int((~dy).sum() + (~duv).sum())
        total += dy.size + duv.size
    print(f"{kind} {guide}: {undecided} of the reference's {total} samples undecided ({100.0 * undecided / total:.2f} %)")
    if bits == 10:
        assert undecided < 0.02 * total, f"{undecided} of the reference's {total} samples lie within eps of a code boundary"
    else:
        assert total - undecided >= 0.40 * total, f"only {total - undecided} of the reference's {total} samples are decided"
    for shape in SHAPES:
        B, H, W = shape
        c = surface_case(shape, kind)
        want_guide, yq, uvq, dy, duv = refs[shape]
        if shape == SHAPES[0]:
            assert len(np.unique(yq)) > 100 and len(np.unique(uvq)) > 50  # a picture, not a constant
        for pad in PADS:
            y, uv = planes(c, pad, W, dev)
            for fill in ((0xA5A5,) if pad == 0 else (0xA5A5, 0x5A5A)):
                flats, (oy, ouv) = _out_surface(shape, pad, dev, fill)
                got = ops.bilateral_slice_apply_io_yuv_deep(T(c["grid"], dev), y, uv, k_in, from_rgb=k_out, out_bits=bits,
                                                            out_planes=(oy, ouv), **guide_kw(ops, c, guide, dev))
                assert ops.last_kernel() == f"apply_fwd_io/p016->p016{GUIDE_LABEL[guide]}"
                (ry, ruv), g = got if want_guide is not None else (got, None)
                assert ry.data_ptr() == oy.data_ptr() and ruv.data_ptr() == ouv.data_ptr()
                for name, plane, want, dec in (("Y", N(oy), yq, dy), ("UV", N(ouv), uvq, duv)):
                    assert not np.any(plane & low_bits), f"{name}: a sample has low bits set"
                    diff = uc.code_diff(plane, want, bits)
                    print(f"{kind} out {guide} {shape} pad {pad} {name}: {int((diff > 0).sum())} of {diff.size} differ, "
                          f"max {int(diff.max())}; undecided {int((~dec).sum())}")
                    assert diff.max() <= 1, f"{name}: off by more than one code"
                    assert np.array_equal(plane[dec], want[dec]), f"{name}: a sample float64 decides by > eps differs"
                if g is not None:
                    assert np.array_equal(N(g), want_guide)
                # padding and the guard behind each plane keep their fill
                for flat, rows in zip(flats, (H, H // 2)):
                    whole = N(flat)
                    pitch = W + pad // 2
                    body = whole[:B * rows * pitch].reshape(B, rows, pitch)
                    assert (body[:, :, W:] == fill).all(), "a store went into the row padding"
                    assert (whole[B * rows * pitch:] == fill).all(), "a store left the output plane"


def test_p016_output_allocates_tight_planes(dev, ops):
    shape, kind = SHAPES[1], "p010"
    B, H, W = shape
    c = surface_case(shape, kind)
    _, k_in, k_out = surface_constants(kind, dev)
    y, uv = planes(c, 0, W, dev)
    kw = dict(guide=T(c["guide"], dev), from_rgb=k_out, out_bits=10)
    oy, ouv = ops.bilateral_slice_apply_io_yuv_deep(T(c["grid"], dev), y, uv, k_in, **kw)
    _, (py, puv) = _out_surface(shape, 64, dev, 0x5A5A)
    ops.bilateral_slice_apply_io_yuv_deep(T(c["grid"], dev), y, uv, k_in, out_planes=(py, puv), **kw)
    assert tuple(oy.shape) == (B, H, W) and tuple(ouv.shape) == (B, H // 2, W) and oy.is_contiguous() and ouv.is_contiguous()
    assert oy.dtype == torch.uint16 and ouv.dtype == torch.uint16
    assert np.array_equal(N(oy), N(py)) and np.array_equal(N(ouv), N(puv))


# ---- 5. the models and the captured graphs -------------------------------------------------------------------------------
def _model(cls, dev, seed=7):
    from hdrnet_amd import models
    torch.manual_seed(seed)
    return getattr(models, cls)(dict(batch_norm=False)).to(dev).eval()


@pytest.mark.parametrize("cls", ["HDRNetCurves", "HDRNetPointwiseNNGuide"])
def test_models_process_u16(dev, ops, cls):
    from hdrnet_amd import data
    from hdrnet_amd.runtime import FrameInference
    m = _model(cls, dev)
    rng = np.random.default_rng(53)
    shape = (1, 272, 480)
    label = "+curvesguide" if cls == "HDRNetCurves" else "+nnguide"
    f1, f2 = (T(px.random_frame(rng, shape, "rgb", "uint16", 32767.0), dev) for _ in range(2))

    def composed(frame, wl, wl_out, fmt="rgb"):
        coeffs = m.coefficients(data.lowres_input(frame, m.params["net_input_size"], wl, pixel_format=fmt))
        gs = coeffs.shape
        return ops.bilateral_slice_apply_io_u16(coeffs.reshape(gs[0], gs[1], gs[2], gs[3], gs[4] * gs[5]), frame,
                                                input_white_level=wl, output_white_level=wl_out, pixel_format=fmt,
                                                **m._process_guide_args())

    with torch.no_grad():
        # the HDR+ configuration: white level 32767 in, and out by default
        got = m.process(f1, out_dtype=torch.uint16, white_level=32767.0)
        assert ops.last_kernel().startswith("apply_fwd_io/u16->u16" + label)
        assert got.dtype == torch.uint16 and tuple(got.shape) == shape + (3,)
        assert torch.equal(got.view(torch.int16), composed(f1, 32767.0, 32767.0).view(torch.int16))
        assert int(N(got).max()) <= 32767 and len(np.unique(N(got))) > 1000
        # ... the default white levels of a uint16 frame are 65535 both ways; an explicit out_white_level is passed on
        assert torch.equal(m.process(f1, out_dtype=torch.uint16).view(torch.int16), composed(f1, 65535.0, 65535.0).view(torch.int16))
        assert torch.equal(m.process(f1, out_dtype=torch.uint16, white_level=32767.0, out_white_level=1023.0).view(torch.int16),
                           composed(f1, 32767.0, 1023.0).view(torch.int16))
        # a float32 frame: 65535 by default
        ff = torch.rand(shape + (3,), device=dev)
        gotf = m.process(ff, out_dtype=torch.uint16)
        assert ops.last_kernel().startswith("apply_fwd_io/f32->u16" + label)
        assert torch.equal(gotf.view(torch.int16), composed(ff, None, 65535.0).view(torch.int16))
        # a BGRA frame keeps its format and its alpha
        bgra = T(px.random_frame(rng, shape, "bgra", "uint16", 65535.0), dev)
        gotb = m.process(bgra, out_dtype=torch.uint16, pixel_format="bgra")
        assert ops.last_kernel().startswith("apply_fwd_io/u16->u16" + label) and ops.last_kernel().endswith("/bgra")
        assert tuple(gotb.shape) == shape + (4,) and np.array_equal(N(gotb)[..., 3], N(bgra)[..., 3])
    # a graph captured on one frame replays another
    fi = FrameInference(m, f1, out_dtype=torch.uint16, white_level=32767.0)
    want2 = m.process(f2, out_dtype=torch.uint16, white_level=32767.0).clone()
    assert torch.equal(fi(f2).view(torch.int16), want2.view(torch.int16))
    assert torch.equal(fi(f1).view(torch.int16), got.view(torch.int16)) and not torch.equal(got.view(torch.int16), want2.view(torch.int16))
    fo = FrameInference(m, f1, out_dtype=torch.uint16, white_level=32767.0, out_white_level=1023.0)
    assert torch.equal(fo(f2).view(torch.int16),
                       m.process(f2, out_dtype=torch.uint16, white_level=32767.0, out_white_level=1023.0).view(torch.int16))


@pytest.mark.parametrize("cls", ["HDRNetCurves", "HDRNetPointwiseNNGuide"])
def test_models_process_yuv_p010(dev, ops, cls):
    from hdrnet_amd import data, yuv
    from hdrnet_amd.runtime import YuvFrameInference
    m = _model(cls, dev)
    rng = np.random.default_rng(59)
    shape = (1, 272, 480)
    label = "+curvesguide" if cls == "HDRNetCurves" else "+nnguide"
    (y1, uv1), (y2, uv2) = (tuple(T(a, dev) for a in yc.random_surface(rng, shape, 10, corners=False)) for _ in range(2))

    def composed(y, uv, standard, full, bits):
        k_in = T(yuv.yuv_coefficients(standard, full, bits)[0], dev)
        k_out = T(yuv.yuv_encode_coefficients(standard, full, bits), dev)
        coeffs = m.coefficients(data.lowres_input_yuv(y, uv, k_in, m.params["net_input_size"]))
        gs = coeffs.shape
        return ops.bilateral_slice_apply_io_yuv_deep(coeffs.reshape(gs[0], gs[1], gs[2], gs[3], gs[4] * gs[5]), y, uv, k_in,
                                                     from_rgb=k_out, out_bits=bits, **m._process_guide_args())

    with torch.no_grad():
        gy, guv = m.process_yuv(y1, uv1, bits=10, out="p010")
        assert ops.last_kernel().startswith("apply_fwd_io/p016->p016" + label)
        wy, wuv = composed(y1, uv1, "bt709", False, 10)
        assert gy.dtype == torch.uint16 and tuple(gy.shape) == shape and tuple(guv.shape) == (1, 136, 480)
        assert np.array_equal(N(gy), N(wy)) and np.array_equal(N(guv), N(wuv))
        assert not np.any(N(gy) & 63) and not np.any(N(guv) & 63) and len(np.unique(N(gy))) > 100
        # P016, BT.2020, full range: the output surface takes the standard and range of the input
        y16, uv16 = (T(a, dev) for a in yc.random_surface(rng, shape, 16, corners=False))
        hy, huv = m.process_yuv(y16, uv16, standard="bt2020", full_range=True, out="p016")
        wy, wuv = composed(y16, uv16, "bt2020", True, 16)
        assert np.array_equal(N(hy), N(wy)) and np.array_equal(N(huv), N(wuv))
    # a graph captured on one surface replays another
    fi = YuvFrameInference(m, y1, uv1, bits=10, out="p010")
    want2 = [t.clone() for t in m.process_yuv(y2, uv2, bits=10, out="p010")]
    ry, ruv = fi(y2, uv2)
    assert np.array_equal(N(ry), N(want2[0])) and np.array_equal(N(ruv), N(want2[1]))
    ry, ruv = fi(y1, uv1)
    assert np.array_equal(N(ry), N(gy)) and np.array_equal(N(ruv), N(guv)) and not np.array_equal(N(gy), N(want2[0]))
