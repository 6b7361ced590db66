"""Packed YUV 4:2:2 surfaces without a GPU (include/hdrnet_amd_yuv_packed.h): the four entry points are exported and bound as
declared; the numpy weave / unweave of tests/yuv_packed_cases.py round-trips and unweaves YUY2 to the NV16 pair and Y210 to
the P210 pair of the same codes; every rule of the header is refused through the C ABI with rc = 1 and a text that names it,
before any HIP call (fake pointers, H = 3, W = 8); B H W = 0 is a no-op; the Python layers refuse a format that does not fit
the tensor, accept the 4-D view, refuse a strided last dimension, the pyramid model refuses, and ``bits`` defaults follow the
format."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import yuv_chroma_cases as cc
import yuv_packed_cases as kc
import yuv_planar_cases as pc
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hdrnet_amd_yuv_packed.h")
A = 0x1000  # a 16-byte aligned non-null "device pointer": never dereferenced, every row below is refused first
NAMES = sorted(["hdrnet_yuv_packed_to_rgb_f32", "hdrnet_lowres_input_yuv_packed", "hdrnet_bilateral_slice_apply_io_yuv_packed",
                "hdrnet_bilateral_slice_apply_io_curves_yuv_packed"])
YUYV, UYVY, YVYU = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for name, (res, args) in _lib.YUV_PACKED_SIGNATURES.items():
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    lib.hdrnet_last_error.restype = ctypes.c_char_p
    lib.hdrnet_last_kernel.restype = ctypes.c_char_p
    lib.hdrnet_version.restype = ctypes.c_int
    lib.hdrnet_enable_kernel_names(1)
    return lib


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(hdrnet_[a-z0-9_]+)\s*\(([^)]*)\)", src):
        out[m.group(1)] = [" ".join(p.split()) for p in m.group(2).split(",")]
    return out


# ---- 1. header <-> table ---------------------------------------------------------------------------------------------------------
def test_symbols_exported_and_bound_as_declared(lib):
    from hdrnet_amd import _lib
    decl = _declared()
    assert sorted(decl) == sorted(_lib.YUV_PACKED_SIGNATURES) == NAMES and len(NAMES) == 4
    for name, params in decl.items():
        res, args = _lib.YUV_PACKED_SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for ctype, text in zip(args, params):  # pointer / long long / int / unsigned, position by position
            want = (ctypes.c_void_p if "*" in text else ctypes.c_longlong if text.startswith("long long ")
                    else ctypes.c_uint if text.startswith("unsigned") else ctypes.c_int)
            assert ctype is want, (name, text, ctype)
        assert "int order" in params and "const void* surface" in params and hasattr(lib, name)
    for other in (_lib.SIGNATURES, _lib.YUV_SIGNATURES, _lib.YUV_PLANAR_SIGNATURES, _lib.U16_OUT_SIGNATURES,
                  _lib.YUV_CHROMA_SIGNATURES, _lib.PYRAMID_YUV_SIGNATURES, _lib.PIXEL_FORMAT_SIGNATURES):
        assert not set(decl) & set(other)  # a header and a table of their own
    assert hasattr(_lib.load(), "hdrnet_yuv_packed_to_rgb_f32")  # ... and the package's handle binds them
    assert lib.hdrnet_version() >= 292
    text = open(HEADER).read()
    assert _lib.PACKED_ORDER == {"yuy2": 0, "yuyv": 0, "uyvy": 1, "yvyu": 2, "y210": 0, "y216": 0}
    for name, code in (("YUYV", 0), ("UYVY", 1), ("YVYU", 2)):
        assert re.search(r"#define HDRNET_PACKED_%s %d\b" % (name, code), text), name
        assert _lib.PACKED_ORDER[name.lower()] == code
    assert {kc.order_of(f) for f in kc.FORMATS} == set(_lib.PACKED_ORDER.values())
    assert all(_lib.PACKED_ORDER[f] == kc.order_of(f) for f in kc.FORMATS)
    assert "out of scope" in text.lower()
    scope = text.split("Out of scope")[-1]
    for word in ("AYUV", "Y410", "v210", "uint16 RGB frame", "pyramid", "bilinear chroma"):
        assert word in scope, word
    # the header that called packed 4:2:2 out of scope points here, before its own scope paragraph (which stays)
    chroma = open(os.path.join(ROOT, "include", "hdrnet_amd_yuv_chroma.h")).read()
    assert "hdrnet_amd_yuv_packed.h" in chroma.split("Out of scope")[0] and "YUY2" in chroma.split("Out of scope")[-1]


# ---- 2. weave / unweave -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(kc.FORMATS))
def test_weave_round_trip(fmt):
    rng = np.random.default_rng([3, kc.order_of(fmt), kc.bits_of(fmt)])
    shape = (2, 5, 12)
    bits, order = kc.bits_of(fmt), kc.order_of(fmt)
    codes = kc.random_codes(rng, shape, bits)
    y, uv = kc.semi(codes, bits)
    s = kc.packed(codes, fmt)
    assert s.shape == (2, 5, 24) and s.dtype == kc.dtype_of(fmt) == y.dtype
    ry, ruv = kc.unweave(s, order)
    assert np.array_equal(ry, y) and np.array_equal(ruv, uv)
    assert np.array_equal(kc.weave(ry, ruv, order), s)
    # one group by hand: pixels 4 and 5 of row 3, image 1
    Y0, Y1, U, V = y[1, 3, 4], y[1, 3, 5], uv[1, 3, 4], uv[1, 3, 5]
    want = {0: [Y0, U, Y1, V], 1: [U, Y0, V, Y1], 2: [Y0, V, Y1, U]}[order]
    assert list(s[1, 3, 8:12]) == want
    # every chroma sample is its own draw: neighbouring rows and neighbouring groups differ
    assert not np.array_equal(ruv[:, 1], ruv[:, 2]) and not np.array_equal(ruv[:, :, 0:2], ruv[:, :, 2:4])
    sh = 16 - bits if bits > 8 else 0
    assert not (s & ((1 << sh) - 1)).any() and np.array_equal(ry >> sh, codes[0])


def test_unweaving_gives_the_semi_planar_pair():
    """YUY2 unweaves to the NV16 pair and Y210 to the P210 pair of the same codes; the three uint8 orders hold the same
    samples in other places."""
    rng = np.random.default_rng(5)
    shape = (1, 3, 8)
    c8, c10 = kc.random_codes(rng, shape, 8), kc.random_codes(rng, shape, 10)
    for codes, fmt, bits in ((c8, "yuy2", 8), (c10, "y210", 10)):
        y, uv = kc.unweave(kc.packed(codes, fmt), 0)
        wy, wuv = cc.semi(*codes, bits)
        assert np.array_equal(y, wy) and np.array_equal(uv, wuv)
        assert np.array_equal(uv, pc.interleave(codes[1], codes[2]) << (16 - bits if bits > 8 else 0))
    a, b, c = (kc.packed(c8, f) for f in ("yuy2", "uyvy", "yvyu"))
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)
    assert np.array_equal(np.sort(a.reshape(-1, 4), axis=1), np.sort(b.reshape(-1, 4), axis=1))
    for s, order in ((a, 0), (b, 1), (c, 2)):
        for got, want in zip(kc.unweave(s, order), kc.unweave(a, 0)):
            assert np.array_equal(got, want)
    # layouts: a packed row of W pixels is 2 W samples, pitches stay multiples of 4 bytes
    for size in (1, 2):
        for layout in kc.LAYOUTS:
            lengths, (i, off, shp, strides) = kc.surface_layout((2, 5, 100), size, layout)
            assert shp == (2, 5, 200) and strides[2] == 1 and strides[1] >= 200 and all(s * size % 4 == 0 for s in strides[:2])
            assert (strides[1] == 200) == (layout == "tight") and strides[0] >= 5 * strides[1]


# ---- 3. the C ABI: a surface of H = 3 (odd: no row pair), W = 8 -----------------------------------------------------------------
def _surf(p=A, dt=1, pitch=None, stride=None, order=YUYV):
    pitch = 16 * dt if pitch is None else pitch
    return [p, dt, pitch, 3 * pitch if stride is None else stride, order]


def _out(kind=1, out=A, pitch=0, stride=0, k=None, bits=0):
    return [kind, out, pitch, stride, k, bits]


YUY2_OUT = dict(kind=2, out=A, pitch=16, stride=48, k=A)
Y216_OUT = dict(kind=3, out=A, pitch=32, stride=96, k=A, bits=16)
U16 = dict(dt=2)


def _call(lib, name, surf=None, B=1, H=3, W=8, k=A, grid=A, guide=A, conv=(None, None, 0), GH=2, GW=2, GD=2, Cin=3, Cout=3,
          off=1, flags=0, npts=16, prepared=None, out=None, rgb=A, lowres=A, n=4):
    """One of the four entry points by its role (``name``: "to_rgb", "lowres", "io", "curves")."""
    surf = surf if surf is not None else _surf()
    head = [*surf, B, H, W, k]
    if name == "to_rgb":
        fn, args = "hdrnet_yuv_packed_to_rgb_f32", [*head, rgb, None]
    elif name == "lowres":
        fn, args = "hdrnet_lowres_input_yuv_packed", [*head, lowres, n, None]
    else:
        out = out if out is not None else _out()
        shape = [GH, GW, GD, Cin, Cout, off]
        if name == "io":
            fn, args = "hdrnet_bilateral_slice_apply_io_yuv_packed", [grid, guide, *head, *shape, *conv, None, flags, *out, None]
        else:
            fn, args = ("hdrnet_bilateral_slice_apply_io_curves_yuv_packed",
                        [grid, *head, *shape, A, A, A, A, npts, prepared, None, *out, None])
    rc = getattr(lib, fn)(*args)
    return rc, lib.hdrnet_last_error().decode(), fn


ROLES = ["to_rgb", "lowres", "io", "curves"]
# rules of the input surface, the same for all four roles: (keywords, text)
SURFACE_REFUSALS = [
    (dict(surf=_surf(p=None)), "null input surface"),
    (dict(W=6), "W % 4 != 0"),
    (dict(W=10), "W % 4 != 0"),
    (dict(surf=_surf(pitch=12)), "below the row's 16 bytes"),          # a packed row is 2 W samples
    (dict(surf=_surf(pitch=28, **U16)), "below the row's 32 bytes"),
    (dict(surf=_surf(pitch=18)), "pitch of the input surface must be a multiple of 4"),
    (dict(surf=_surf(p=A + 2)), "input surface and its constants must be 4-B aligned"),
    (dict(surf=_surf(stride=50)), "image stride of the input surface must be a non-negative multiple of 4"),
    (dict(surf=_surf(stride=-4)), "image stride of the input surface must be a non-negative multiple of 4"),
    (dict(B=2, surf=_surf(stride=32)), "image stride of the input surface is below its plane"),
    (dict(surf=_surf(order=3)), "unknown byte order code 3"),
    (dict(surf=_surf(order=-1)), "unknown byte order code -1"),
    (dict(surf=_surf(order=UYVY, **U16)), "uint16 samples (Y210 / Y216) take HDRNET_PACKED_YUYV only"),
    (dict(surf=_surf(order=YVYU, **U16)), "uint16 samples (Y210 / Y216) take HDRNET_PACKED_YUYV only"),
    (dict(surf=_surf(dt=0)), "unknown sample dtype code of the input surface (0"),  # float samples
    (dict(surf=_surf(dt=3)), "unknown sample dtype code"),
    (dict(k=None), "null constants of the input surface"),
]
IO_REFUSALS = SURFACE_REFUSALS + [
    (dict(out=_out(kind=4)), "unknown output kind"),
    (dict(out=_out(kind=-1)), "unknown output kind"),
    # a surface out has the input's sample width
    (dict(out=_out(**Y216_OUT)), "a packed surface output has the input's sample width"),            # uint8 in, uint16 out
    (dict(surf=_surf(**U16), out=_out(**dict(YUY2_OUT, pitch=32, stride=96))), "a packed surface output has the input's sample width"),
    (dict(surf=_surf(**U16), out=_out(**dict(Y216_OUT, bits=12))), "out_bits must be 10 (Y210) or 16 (Y216), got 12"),
    (dict(surf=_surf(**U16), out=_out(**dict(Y216_OUT, bits=8))), "out_bits must be 10 (Y210) or 16 (Y216)"),
    # the output surface under the same rules
    (dict(out=_out(**dict(YUY2_OUT, pitch=12))), "pitch of the output surface is below the row"),
    (dict(out=_out(**dict(YUY2_OUT, pitch=18))), "pitch of the output surface must be a multiple of 4"),
    (dict(B=2, out=_out(**dict(YUY2_OUT, stride=32))), "image stride of the output surface is below its plane"),
    (dict(out=_out(**dict(YUY2_OUT, out=None))), "null output surface"),
    (dict(out=_out(**dict(YUY2_OUT, out=A + 1))), "output surface and its constants must be 4-B aligned"),
    (dict(out=_out(**dict(YUY2_OUT, k=None))), "null constants of the output surface"),
    (dict(out=_out(out=None)), "null or misaligned out"),
    (dict(out=_out(kind=0, out=A + 4)), "null or misaligned out"),
    (dict(Cin=4), "Cin = Cout = 3 with offset"),
    (dict(Cout=4), "Cin = Cout = 3 with offset"),
    (dict(off=0), "Cin = Cout = 3 with offset"),
    (dict(grid=None), "null buffer"),
]


@pytest.mark.parametrize("kw,text", IO_REFUSALS)
@pytest.mark.parametrize("role", ["io", "curves"])
def test_fused_forward_refusals(lib, role, kw, text):
    rc, err, fn = _call(lib, role, **kw)
    assert rc == 1 and text in err and err.startswith(fn + ": "), (rc, err)


@pytest.mark.parametrize("kw,text", SURFACE_REFUSALS)
@pytest.mark.parametrize("role", ["to_rgb", "lowres"])
def test_conversion_and_gather_refusals(lib, role, kw, text):
    rc, err, fn = _call(lib, role, **kw)
    assert rc == 1 and text in err and err.startswith(fn + ": "), (rc, err)


def test_other_refusals(lib):
    assert "rgb must be" in _call(lib, "to_rgb", rgb=None)[1]
    for role in ROLES:
        rc, err, _ = _call(lib, role, H=-1)
        assert rc == 1 and "negative image extent" in err
    assert "lowres must be" in _call(lib, "lowres", lowres=A + 4)[1]
    assert "non-positive extent" in _call(lib, "lowres", n=0)[1]
    # neither guide, both guides, half a network
    rc, err, _ = _call(lib, "io", guide=None)
    assert rc == 1 and "either a guide map or the guide network must be given" in err
    rc, err, _ = _call(lib, "io", guide=A, conv=(A, A, 16))
    assert rc == 1 and "either a guide map or the guide network must be given, not both" in err
    rc, err, _ = _call(lib, "io", guide=None, conv=(A, None, 16))
    assert rc == 1 and "either a guide map or the guide network must be given" in err
    assert "unknown flags" in _call(lib, "io", flags=0x40000)[1]
    assert "curve knots" in _call(lib, "curves", npts=0)[1]
    assert "prepared curves tables" in _call(lib, "curves", prepared=A + 4)[1]


def test_what_the_rules_admit_gets_as_far_as_the_grid(lib):
    """Every order at 8 bits, YUYV at 16, a pitched surface, odd H, B = 2, both surface outputs with 10 and 16 bits: the
    call passes every surface rule and stops at the null grid."""
    for order in (YUYV, UYVY, YVYU):
        rc, err, _ = _call(lib, "io", surf=_surf(order=order, pitch=80, stride=240), B=2, grid=None,
                           out=_out(**dict(YUY2_OUT, pitch=20, stride=60)))
        assert rc == 1 and "null buffer (grid)" in err, err
    for bits in (10, 16):
        rc, err, _ = _call(lib, "curves", surf=_surf(**U16), grid=None, out=_out(**dict(Y216_OUT, bits=bits)))
        assert rc == 1 and "null buffer (grid" in err, err
    rc, err, _ = _call(lib, "io", surf=_surf(pitch=200), W=100, H=1, grid=None)
    assert rc == 1 and "null buffer (grid)" in err, err


def test_empty_extents_are_a_noop(lib):
    nothing = dict(surf=_surf(p=None), k=None, out=_out(out=None), rgb=None, lowres=None, grid=None, guide=None)
    for role in ROLES:
        rc, err, fn = _call(lib, role, B=0, **nothing)
        assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop", (fn, err)
    for role in ("to_rgb", "io", "curves"):  # (the gather needs a source: H = 0 is refused there, as in the entry point it mirrors)
        rc, err, fn = _call(lib, role, H=0, **nothing)
        assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop", (fn, err)


# ---- 4. the Python layers ---------------------------------------------------------------------------------------------------------
def test_python_argument_rules():
    from hdrnet_amd import data, hdrnet_ops as ops
    k = torch.zeros(12)
    grid = torch.zeros(1, 2, 2, 2, 12)
    guide = torch.zeros(1, 3, 8)
    s8, s16 = torch.zeros(1, 3, 16, dtype=torch.uint8), torch.zeros(1, 3, 16, dtype=torch.uint16)
    calls = [lambda s, f, **kw: ops.yuv_packed_to_rgb(s, k, f, **kw), lambda s, f, **kw: data.lowres_input_yuv_packed(s, k, f, **kw),
             lambda s, f, **kw: ops.bilateral_slice_apply_io_yuv_packed(grid, s, k, f, guide=guide, **kw)]
    for f in calls:
        # the format is named and must fit the dtype
        for fmt in ("yuy2", "yuyv", "uyvy", "yvyu"):
            with pytest.raises(TypeError, match=f"format='{fmt}' is a uint8 format, surface is torch.uint16"):
                f(s16, fmt)
        for fmt in ("y210", "y216"):
            with pytest.raises(TypeError, match=f"format='{fmt}' is a uint16 format, surface is torch.uint8"):
                f(s8, fmt)
        with pytest.raises(ValueError, match="unknown format 'nv16'"):
            f(s8, "nv16")
        with pytest.raises(ValueError, match="unknown format None"):
            f(s8, None)
        with pytest.raises(TypeError, match="is a uint8 format, surface is torch.float32"):
            f(torch.zeros(1, 3, 16), "yuy2")
        # shapes and strides
        with pytest.raises(ValueError, match="W % 4 != 0"):
            f(torch.zeros(1, 3, 12, dtype=torch.uint8), "yuy2")
        with pytest.raises(ValueError, match=r"should be \[B, H, 2 W\]"):
            f(torch.zeros(3, 16, dtype=torch.uint8), "yuy2")
        with pytest.raises(ValueError, match="last-dimension stride 1"):
            f(torch.zeros(1, 3, 32, dtype=torch.uint8)[:, :, ::2], "uyvy")  # a non-unit last stride
        with pytest.raises(ValueError, match="multiples of 4 bytes"):
            f(torch.zeros(1, 3, 18, dtype=torch.uint8)[:, :, :16], "yuy2")  # a pitch of 18 bytes
        # what fits gets as far as asking for the device: tight, pitched, the 4-D view, uint16
        for s, fmt in ((s8, "yvyu"), (torch.zeros(1, 3, 80, dtype=torch.uint8)[:, :, :16], "yuy2"),
                       (torch.zeros(1, 3, 8, 2, dtype=torch.uint8), "uyvy"), (s16, "y210"),
                       (torch.zeros(1, 3, 8, 2, dtype=torch.uint16), "y216")):
            with pytest.raises(RuntimeError, match="MI355X"):
                f(s, fmt)
    # the 4-D view is the same memory as [B, H, 2 W]
    v4 = torch.arange(48, dtype=torch.uint8).reshape(1, 3, 8, 2)
    v3, B, H, W, (dt, pitch, stride, order) = ops._yuv_packed_surface(v4, "uyvy", "t")
    assert (B, H, W) == (1, 3, 8) and tuple(v3.shape) == (1, 3, 16) and v3.data_ptr() == v4.data_ptr()
    assert (dt, pitch, stride, order) == (1, 16, 48, 1) and torch.equal(v3.reshape(-1), v4.reshape(-1))
    assert ops._yuv_packed_surface(torch.zeros(2, 3, 40, dtype=torch.uint16)[:, :, :16], "y216", "t")[4] == (2, 80, 240, 0)
    # the output's arguments
    fwd = ops.bilateral_slice_apply_io_yuv_packed
    with pytest.raises(ValueError, match="takes 'rgb', 'packed'"):
        fwd(grid, s8, k, "yuy2", guide=guide, out="nv16")
    with pytest.raises(ValueError, match="out='packed' needs from_rgb"):
        fwd(grid, s8, k, "yuy2", guide=guide, out="packed")
    with pytest.raises(ValueError, match="belong to out='packed'"):
        fwd(grid, s8, k, "yuy2", guide=guide, from_rgb=k)
    with pytest.raises(ValueError, match="out_bits must be 8"):
        fwd(grid, s8, k, "yuy2", guide=guide, out="packed", from_rgb=k, out_bits=10)
    with pytest.raises(ValueError, match=r"out_bits must be 10 \(Y210\) or 16 \(Y216\)"):
        fwd(grid, s16, k, "y216", guide=guide, out="packed", from_rgb=k, out_bits=12)
    with pytest.raises(TypeError, match="a packed output has the input's sample dtype"):
        fwd(grid, s8, k, "yuy2", guide=guide, out="packed", from_rgb=k, out_dtype=torch.uint16)
    with pytest.raises(TypeError, match="format='yuy2' is a uint8 format, out_surface is torch.uint16"):
        fwd(grid, s8, k, "yuy2", guide=guide, out="packed", from_rgb=k, out_surface=s16)
    with pytest.raises(ValueError, match="out_surface should be a surface of"):
        fwd(grid, s8, k, "yuy2", guide=guide, out="packed", from_rgb=k, out_surface=torch.zeros(1, 4, 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="exactly one of guide"):
        fwd(grid, s8, k, "yuy2")
    with pytest.raises(ValueError, match="exactly one of guide"):
        fwd(grid, s8, k, "yuy2", guide=guide, guide_conv1=torch.zeros(16, 4), guide_conv2=torch.zeros(17))


def test_models_bits_defaults_and_the_pyramid():
    from hdrnet_amd import hdrnet_ops as ops, models
    torch.manual_seed(0)
    s8, s16 = torch.zeros(1, 3, 16, dtype=torch.uint8), torch.zeros(1, 3, 16, dtype=torch.uint16)
    for cls in ("HDRNetCurves", "HDRNetPointwiseNNGuide"):
        m = getattr(models, cls)(dict(batch_norm=False)).eval()
        assert [m._packed_bits("t", f, None) for f in ("yuy2", "yuyv", "uyvy", "yvyu", "y210", "y216")] == [8, 8, 8, 8, 10, 16]
        assert m._packed_bits("t", "y216", 10) == 10 and m._packed_bits("t", "y210", 16) == 16
        for fmt, bits in (("yuy2", 10), ("y210", 8), ("y216", 12)):
            with pytest.raises(ValueError, match="does not fit format"):
                m.process_yuv_packed(s8 if fmt == "yuy2" else s16, fmt, bits=bits)
        with pytest.raises(TypeError, match="format='y210' is a uint16 format"):
            m.process_yuv_packed(s8, "y210")
        with pytest.raises(ValueError, match="takes 'rgb', 'packed'"):
            m.process_yuv_packed(s8, "yuy2", out="nv16")
        with pytest.raises(ValueError, match="unknown standard"):
            m.process_yuv_packed(s8, "yuy2", standard="bt470")
        with pytest.raises(TypeError, match="a packed output has the input's dtype"):
            m.process_yuv_packed(s8, "yuy2", out="packed", out_dtype=torch.uint16)
        with pytest.raises(RuntimeError, match="MI355X"):  # as far as asking for the device
            m.process_yuv_packed(s16, "y210", out="packed")
    assert [ops.packed_default_bits(f) for f in ("uyvy", "y210", "y216")] == [8, 10, 16]
    pyr = models.HDRNetGaussianPyrNN(dict(batch_norm=False)).eval()
    for s, fmt in ((s8, "yuy2"), (s16, "y216")):
        with pytest.raises(ValueError, match="process_wire_yuv"):
            pyr.process_yuv_packed(s, fmt)
