"""Pixel formats without a GPU (include/hdrnet_amd_pixel_formats.h): the three entry points are exported and bound as
declared, refuse what the format rules exclude with rc = 1 and a text that names the rule before any HIP call, and the
Python layers above them (hdrnet_ops.bilateral_slice_apply_io, data.lowres_input, model.process, process_wire) raise
before anything touches the device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pixel_format_cases as px
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hdrnet_amd_pixel_formats.h")
A = 0x1000  # a 16-byte aligned non-null "device pointer": never dereferenced, every row below is refused first
RGB, BGR, RGBA, BGRA = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for name, (res, args) in _lib.PIXEL_FORMAT_SIGNATURES.items():
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
        out[m.group(1)] = [p.strip() for p in m.group(2).split(",")]
    return out


def test_symbols_exported_and_bound_as_declared(lib):
    from hdrnet_amd import _lib
    decl = _declared()
    assert sorted(decl) == sorted(_lib.PIXEL_FORMAT_SIGNATURES) == [
        "hdrnet_bilateral_slice_apply_io_curves_px", "hdrnet_bilateral_slice_apply_io_px", "hdrnet_lowres_input_px"]
    for name, params in decl.items():
        res, args = _lib.PIXEL_FORMAT_SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for ctype, text in zip(args, params):  # pointer / int / float / unsigned, position by position
            want = (ctypes.c_void_p if "*" in text else ctypes.c_float if text.startswith("float ")
                    else ctypes.c_uint if text.startswith("unsigned") else ctypes.c_int)
            assert ctype is want, (name, text, ctype)
        assert hasattr(lib, name)
    assert not set(decl) & set(_lib.SIGNATURES)  # a header of their own: the first table still mirrors hdrnet_amd.h
    assert hasattr(_lib.load(), "hdrnet_lowres_input_px")  # ... and the package's handle binds them
    assert lib.hdrnet_version() >= 286
    # the codes of the header, the binding and the tests' statement of the rules are the same
    text = open(HEADER).read()
    for name, code in px.CODE.items():
        assert re.search(r"#define HDRNET_PX_%s %d\b" % (name.upper(), code), text), name
        assert _lib.PIXEL_FORMATS[name] == code and _lib.PIXEL_FORMAT_CHANNELS[name] == px.CHANNELS[name]


def _io(lib, grid=A, guide=A, inp=A, out=A, B=1, H=4, W=8, GH=2, GW=2, GD=2, Cin=3, Cout=3, off=1, idt=1, wl=255.0,
        odt=1, c1=None, c2=None, n=0, gout=None, flags=0, ifmt=BGRA, ofmt=BGRA):
    rc = lib.hdrnet_bilateral_slice_apply_io_px(grid, guide, inp, out, B, H, W, GH, GW, GD, Cin, Cout, off, idt, wl, odt,
                                                c1, c2, n, gout, flags, ifmt, ofmt, None)
    return rc, lib.hdrnet_last_error().decode()


def _curves(lib, grid=A, inp=A, out=A, B=1, H=4, W=8, GH=2, GW=2, GD=2, Cin=3, Cout=3, off=1, idt=1, wl=255.0, odt=1,
            npts=16, prepared=None, gout=None, ifmt=BGRA, ofmt=BGRA):
    rc = lib.hdrnet_bilateral_slice_apply_io_curves_px(grid, inp, out, B, H, W, GH, GW, GD, Cin, Cout, off, idt, wl, odt,
                                                       A, A, A, A, npts, prepared, gout, ifmt, ofmt, None)
    return rc, lib.hdrnet_last_error().decode()


def _lowres(lib, frames=A, dtype=1, wl=255.0, B=1, H=8, W=8, lowres=A, n=4, fmt=BGRA):
    rc = lib.hdrnet_lowres_input_px(frames, dtype, wl, B, H, W, lowres, n, fmt, None)
    return rc, lib.hdrnet_last_error().decode()


IO_REFUSALS = [
    (dict(ifmt=4, ofmt=4), "unknown pixel format code"),
    (dict(ifmt=-1, ofmt=-1), "unknown pixel format code"),
    (dict(ifmt=RGB, ofmt=7, odt=0), "unknown pixel format code"),
    (dict(idt=0, wl=1.0, ifmt=BGR, ofmt=BGR), "float32 frames take HDRNET_PX_RGB only"),
    (dict(idt=0, wl=1.0, odt=0, ifmt=BGRA, ofmt=RGB), "float32 frames take HDRNET_PX_RGB only"),
    (dict(ifmt=BGRA, ofmt=RGBA), "a uint8 output has the input's pixel format"),
    (dict(ifmt=BGR, ofmt=RGB), "a uint8 output has the input's pixel format"),
    (dict(ifmt=RGB, ofmt=BGR), "a uint8 output has the input's pixel format"),
    (dict(odt=0, ifmt=BGRA, ofmt=BGRA), "a float32 output is [B][H][W][3] in RGB order"),
    (dict(odt=0, ifmt=RGB, ofmt=BGR), "a float32 output is [B][H][W][3] in RGB order"),
    (dict(inp=A + 4), "must be 16-B aligned"),                 # 4 channels at a 4-byte but not 16-byte address
    (dict(out=A + 8), "must be 16-B aligned"),
    (dict(idt=2, wl=65535.0, inp=A + 4), "must be 16-B aligned"),
    (dict(ifmt=BGR, ofmt=BGR, inp=A + 2), "must be 4-B aligned"),
    (dict(W=6), "W % 4 != 0"),
    (dict(W=6, ifmt=BGR, ofmt=BGR), "W % 4 != 0"),
    (dict(Cin=4, Cout=4), "Cin = Cout = 3 with offset"),       # the format is not a channel count of the op
    (dict(off=0), "Cin = Cout = 3 with offset"),
    (dict(idt=3), "unknown dtype code"),
    (dict(odt=2), "unknown dtype code"),
    (dict(inp=None), "null buffer"),
]


@pytest.mark.parametrize("kw,text", IO_REFUSALS)
def test_io_px_refusals(lib, kw, text):
    rc, err = _io(lib, **kw)
    assert rc == 1 and text in err, (rc, err)


@pytest.mark.parametrize("kw,text", IO_REFUSALS)
def test_io_curves_px_refusals(lib, kw, text):
    rc, err = _curves(lib, **kw)
    assert rc == 1 and text in err, (rc, err)


@pytest.mark.parametrize("kw,text", [
    (dict(fmt=4), "unknown pixel format code"),
    (dict(fmt=-2), "unknown pixel format code"),
    (dict(dtype=0, wl=1.0, fmt=BGR), "float32 frames take HDRNET_PX_RGB only"),
    (dict(dtype=0, wl=1.0, fmt=RGBA), "float32 frames take HDRNET_PX_RGB only"),
    (dict(frames=A + 4), "must be 16-B aligned"),
    (dict(frames=A + 2, fmt=BGR), "4-B aligned"),
    (dict(dtype=5), "unknown dtype code"),
    (dict(lowres=None), "null buffer"),
    (dict(n=0), "non-positive extent"),
])
def test_lowres_px_refusals(lib, kw, text):
    rc, err = _lowres(lib, **kw)
    assert rc == 1 and err.startswith("hdrnet_lowres_input_px: ") and text in err, (rc, err)


def test_empty_batch_is_a_noop(lib):
    for call in (_io, _curves):
        rc, err = call(lib, B=0, inp=None, out=None)
        assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"
        rc, err = call(lib, B=0, inp=None, out=None, ifmt=BGR, ofmt=RGB, odt=0)
        assert rc == 0 and err == ""
    rc, err = _lowres(lib, B=0, frames=None, lowres=None)
    assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"


def test_rgb_is_the_existing_entry_point(lib):
    """With both formats HDRNET_PX_RGB the call is the one it extends: its refusal texts come back."""
    rc, err = _io(lib, ifmt=RGB, ofmt=RGB, W=6)
    assert rc == 1 and "the wire-format forward supports Cin = Cout = 3 with offset" in err
    rc, err = _curves(lib, ifmt=RGB, ofmt=RGB, W=6)
    assert rc == 1 and "the fused curves-guide forward supports" in err
    rc, err = _lowres(lib, fmt=RGB, n=0)
    assert rc == 1 and err.startswith("hdrnet_lowres_input: ")


# ---- the helper's own statement of the rules ---------------------------------------------------------------------------
def test_helper_round_trip():
    rng = np.random.default_rng(5)
    for fmt in px.FORMATS:
        for dtype, wl in (("uint8", 255.0), ("uint16", 65535.0)):
            f = px.random_frame(rng, (2, 3, 4), fmt, dtype, wl)
            rgb = px.to_rgb(f, fmt)
            assert rgb.shape == (2, 3, 4, 3) and rgb.dtype == f.dtype
            r_at = 2 if px.B_FIRST[fmt] else 0
            assert np.array_equal(rgb[..., 0], f[..., r_at]) and np.array_equal(rgb[..., 1], f[..., 1])
            out = rng.integers(0, 256, (2, 3, 4, 3)).astype(np.uint8)
            back = px.from_rgb(out, fmt, px.alpha_of(f, fmt))
            assert back.shape[-1] == px.CHANNELS[fmt] and np.array_equal(px.to_rgb(back, fmt), out)
            if px.CHANNELS[fmt] == 4:
                want = f[..., 3] if dtype == "uint8" else (f[..., 3] >> 8)
                assert np.array_equal(back[..., 3], want.astype(np.uint8))
            fl = rng.random((2, 3, 4, 3)).astype(np.float32)
            assert px.from_rgb(fl, fmt, px.alpha_of(f, fmt)) is fl  # float32 out: RGB, no alpha


# ---- Python refusals on CPU tensors: raised before anything touches the device ------------------------------------------
def test_ops_refuse(lib):
    from hdrnet_amd import data, hdrnet_ops as ops
    grid = torch.zeros(1, 2, 2, 2, 12)
    guide = torch.zeros(1, 4, 8)
    f3 = torch.zeros(1, 4, 8, 3, dtype=torch.uint8)
    f4 = torch.zeros(1, 4, 8, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="unknown pixel_format 'argb'"):
        ops.bilateral_slice_apply_io(grid, f4, guide=guide, pixel_format="argb")
    with pytest.raises(ValueError, match="pixel_format='rgba' is a 4-channel format"):
        ops.bilateral_slice_apply_io(grid, f3, guide=guide, pixel_format="rgba")
    with pytest.raises(ValueError, match="pixel_format='bgr' is a 3-channel format"):
        ops.bilateral_slice_apply_io(grid, f4, guide=guide, pixel_format="bgr")
    with pytest.raises(ValueError, match="float32 frames take pixel_format='rgb' only"):
        ops.bilateral_slice_apply_io(grid, f3.float(), guide=guide, pixel_format="bgr")
    with pytest.raises(ValueError, match="needs the 3 -> 3 op with offset"):
        ops.bilateral_slice_apply_io(torch.zeros(1, 2, 2, 2, 9), f4, guide=guide, pixel_format="bgra", has_offset=False)
    with pytest.raises(RuntimeError, match="no CPU path"):  # everything else in order: only the device is missing
        ops.bilateral_slice_apply_io(grid, f4, guide=guide, pixel_format="bgra", out_dtype=torch.uint8)
    with pytest.raises(ValueError, match="unknown pixel_format"):
        data.lowres_input(f4, 4, pixel_format="abgr")
    with pytest.raises(ValueError, match="pixel_format='bgra' is a 4-channel format"):
        data.lowres_input(f3, 4, pixel_format="bgra")
    with pytest.raises(ValueError, match="float32 frames take pixel_format='rgb' only"):
        data.lowres_input(f4.float(), 4, pixel_format="rgba")
    with pytest.raises(RuntimeError, match="HIP"):
        data.lowres_input(f4, 4, pixel_format="rgba")
    with pytest.raises(ValueError, match=r"\[N, H, W, 3\]"):  # the default keeps today's rule and text
        data.lowres_input(f4, 4)


@pytest.mark.parametrize("cls", ["HDRNetCurves", "HDRNetPointwiseNNGuide"])
def test_process_refuses(lib, cls):
    from hdrnet_amd import models
    torch.manual_seed(3)
    m = getattr(models, cls)(dict(batch_norm=False)).eval()
    f3 = torch.zeros(1, 32, 48, 3, dtype=torch.uint8)
    f4 = torch.zeros(1, 32, 48, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="4-channel frame needs pixel_format='rgba' or pixel_format='bgra'"):
        m.process(f4, out_dtype=torch.uint8)
    with pytest.raises(ValueError, match="pixel_format='rgba' is a 4-channel format"):
        m.process(f3, out_dtype=torch.uint8, pixel_format="rgba")
    with pytest.raises(ValueError, match="pixel_format='bgr' is a 3-channel format"):
        m.process(f4, pixel_format="bgr")
    with pytest.raises(ValueError, match="float32 frames take pixel_format='rgb' only"):
        m.process(f3.float(), pixel_format="bgr")
    with pytest.raises(ValueError, match="unknown pixel_format 'yuv'"):
        m.process(f3, pixel_format="yuv")
    with pytest.raises(ValueError, match=r"\[B, H, W, 3\]"):
        m.process(torch.zeros(1, 32, 48, 5, dtype=torch.uint8))


def test_pyramid_process_wire_refuses(lib):
    from hdrnet_amd import models
    from hdrnet_amd.runtime import _Process
    torch.manual_seed(3)
    m = models.HDRNetGaussianPyrNN(dict(batch_norm=False)).eval()
    frame = torch.zeros(1, 32, 48, 3, dtype=torch.uint8)
    for fmt in ("bgr", "rgba", "bgra"):
        with pytest.raises(ValueError, match="process_wire takes pixel_format='rgb' only"):
            m.process_wire(frame, out_dtype=torch.uint8, pixel_format=fmt)
    with pytest.raises(ValueError, match="process_wire takes pixel_format='rgb' only"):  # ... through the runtime too
        _Process(m, torch.uint8, None, "bgr")(frame)
    # FrameInference's module hands the format to a single-level model's process()
    seen = []
    single = models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).eval()
    single.process = lambda f, o, w, pixel_format=None: seen.append(pixel_format)
    _Process(single, torch.uint8, None, "bgra")(frame)
    _Process(single, torch.uint8, None)(frame)
    assert seen == ["bgra", None]
