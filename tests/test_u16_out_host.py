"""16-bit output without a GPU (include/hdrnet_amd_u16_out.h): the four entry points are exported and bound as declared,
refuse what the rules exclude with rc = 1 and a text that names the rule before any HIP call, the Python layers above them
raise before anything touches the device, the entry points of the older headers still refuse a 16-bit output, and
``yuv.yuv_encode_coefficients`` is ``yuv_coefficients``' encoder at 8 bits and inverts the decoder at 10 and 16."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import u16_out_cases as uc
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hdrnet_amd_u16_out.h")
A = 0x1000  # a 16-byte aligned non-null "device pointer": never dereferenced, every row below is refused first
NAMES = ["hdrnet_bilateral_slice_apply_io_curves_px_u16", "hdrnet_bilateral_slice_apply_io_curves_yuv_p016",
         "hdrnet_bilateral_slice_apply_io_px_u16", "hdrnet_bilateral_slice_apply_io_yuv_p016"]


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for name, (res, args) in _lib.U16_OUT_SIGNATURES.items():
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    lib.hdrnet_last_error.restype = ctypes.c_char_p
    lib.hdrnet_last_kernel.restype = ctypes.c_char_p
    lib.hdrnet_version.restype = ctypes.c_int
    lib.hdrnet_enable_kernel_names(1)
    return lib


def _declared(header=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\b(hdrnet_[a-z0-9_]+)\s*\(([^)]*)\)", src):
        out[m.group(1)] = [" ".join(p.split()) for p in m.group(2).split(",")]
    return out


def test_symbols_exported_and_bound_as_declared(lib):
    from hdrnet_amd import _lib
    decl = _declared()
    assert sorted(decl) == sorted(_lib.U16_OUT_SIGNATURES) == NAMES
    for name, params in decl.items():
        res, args = _lib.U16_OUT_SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for ctype, text in zip(args, params):  # pointer / long long / float / unsigned / int, position by position
            want = (ctypes.c_void_p if "*" in text else ctypes.c_longlong if text.startswith("long long ")
                    else ctypes.c_float if text.startswith("float ") else ctypes.c_uint if text.startswith("unsigned")
                    else ctypes.c_int)
            assert ctype is want, (name, text, ctype)
        assert hasattr(lib, name)
    # a header and a table of their own: the other tables still mirror their headers
    for other in (_lib.SIGNATURES, _lib.PIXEL_FORMAT_SIGNATURES, _lib.YUV_SIGNATURES, _lib.PYRAMID_IO_SIGNATURES):
        assert not set(decl) & set(other)
    assert hasattr(_lib.load(), "hdrnet_bilateral_slice_apply_io_px_u16")  # ... and the package's handle binds them
    assert lib.hdrnet_version() >= 288
    text = open(HEADER).read().lower()
    assert "out of scope" in text and "output_white_level" in text and "out_bits" in text
    # the library still exports every symbol of every public header
    inc = os.path.join(ROOT, "include")
    for h in sorted(os.listdir(inc)):
        if h.endswith(".h") and h != "hdrnet_amd_tools.h":
            for name in _declared(os.path.join(inc, h)):
                assert hasattr(lib, name), f"{name} declared in include/{h} but not exported"


# ---- the frame entry points ----------------------------------------------------------------------------------------------
def _px(lib, grid=A, guide=A, inp=A, out=A, B=1, H=4, W=8, GH=2, GW=2, GD=2, Cin=3, Cout=3, off=1, dt=2, iwl=65535.0,
        owl=65535.0, c1=None, c2=None, n=0, gout=None, flags=0, fin=0, fout=None):
    rc = lib.hdrnet_bilateral_slice_apply_io_px_u16(grid, guide, inp, out, B, H, W, GH, GW, GD, Cin, Cout, off, dt, iwl, owl,
                                                    c1, c2, n, gout, flags, fin, fin if fout is None else fout, None)
    return rc, lib.hdrnet_last_error().decode()


def _px_curves(lib, grid=A, guide=None, inp=A, out=A, B=1, H=4, W=8, GH=2, GW=2, GD=2, Cin=3, Cout=3, off=1, dt=2,
               iwl=65535.0, owl=65535.0, npts=16, prepared=None, gout=None, fin=0, fout=None):
    rc = lib.hdrnet_bilateral_slice_apply_io_curves_px_u16(grid, inp, out, B, H, W, GH, GW, GD, Cin, Cout, off, dt, iwl, owl,
                                                           A, A, A, A, npts, prepared, gout, fin, fin if fout is None else fout,
                                                           None)
    return rc, lib.hdrnet_last_error().decode()


FRAME_REFUSALS = [
    (dict(owl=0.0), "0 < output_white_level <= 65535"),
    (dict(owl=-1.0), "0 < output_white_level <= 65535"),
    (dict(owl=float("inf")), "0 < output_white_level <= 65535"),
    (dict(owl=float("nan")), "0 < output_white_level <= 65535"),
    (dict(owl=65536.0), "0 < output_white_level <= 65535"),
    (dict(dt=1, iwl=255.0), "a uint16 output needs a uint16 or float32 frame"),
    (dict(dt=3), "unknown dtype code"),
    (dict(iwl=0.0), "input_white_level must be positive"),
    (dict(dt=0, iwl=1.0, fin=1), "float32 frames take HDRNET_PX_RGB only"),
    (dict(fin=4), "unknown pixel format code"),
    (dict(fin=3, fout=2), "a uint16 output has the input's pixel format"),
    (dict(fin=2, out=A + 8), "4-channel frames (RGBA / BGRA) must be 16-B aligned"),
    (dict(fin=3, inp=A + 4), "4-channel frames (RGBA / BGRA) must be 16-B aligned"),
    (dict(fin=1, out=A + 2), "3-channel integer frames must be 4-B aligned"),
    (dict(fin=1, W=6), "W % 4 != 0"),
    (dict(fin=1, Cout=4), "need Cin = Cout = 3 with offset"),
    (dict(out=None), "null buffer"),
    (dict(grid=None), "null buffer"),
    (dict(GD=0), "grid extents must be positive"),
    (dict(out=A + 2), "the wire-format forward supports"),  # RGB: the predicate's rule, in the launch tail's words
]


@pytest.mark.parametrize("kw,text", FRAME_REFUSALS)
def test_px_u16_refusals(lib, kw, text):
    rc, err = _px(lib, **kw)
    assert rc == 1 and text in err, (rc, err)
    if "output_white_level" in text or "pixel format" in text or "HDRNET_PX_RGB only" in text or "uint16 or float32" in text:
        assert err.startswith("hdrnet_bilateral_slice_apply_io_px_u16: "), err


@pytest.mark.parametrize("kw,text", [r for r in FRAME_REFUSALS if "supports" not in r[1]])
def test_curves_px_u16_refusals(lib, kw, text):
    rc, err = _px_curves(lib, **kw)
    assert rc == 1 and text in err, (rc, err)
    if "output_white_level" in text or "pixel format" in text:
        assert err.startswith("hdrnet_bilateral_slice_apply_io_curves_px_u16: "), err


def test_other_frame_refusals(lib):
    rc, err = _px(lib, guide=None)
    assert rc == 1 and "either a guide map or the guide network" in err
    rc, err = _px(lib, flags=0x40000)
    assert rc == 1 and "unknown flags" in err
    rc, err = _px_curves(lib, npts=0)
    assert rc == 1 and "curve knots" in err
    rc, err = _px_curves(lib, prepared=A + 4)
    assert rc == 1 and "prepared curves tables" in err
    rc, err = _px_curves(lib, out=A + 2)
    assert rc == 1 and "the fused curves-guide forward supports" in err
    # more than 16 knots on a packed frame: not instantiated, refused by rule in the launch tail's words
    rc, err = _px_curves(lib, npts=20, fin=1)
    assert rc == 1 and "the fused curves-guide forward supports" in err


# ---- the surface entry points --------------------------------------------------------------------------------------------
# a uint16 surface of W = 8: rows of 16 bytes
def _surf(y=A, uv=A, dt=2, py=16, puv=16, sy=64, suv=32):
    return [y, uv, dt, py, puv, sy, suv]


def _p016_out(y=A, uv=A, py=16, puv=16, sy=64, suv=32, k=A, bits=10):
    return [y, uv, py, puv, sy, suv, k, bits]


def _yuv(lib, grid=A, guide=A, surf=None, B=1, H=4, W=8, k=A, GH=2, GW=2, GD=2, Cin=3, Cout=3, off=1, c1=None, c2=None, n=0,
         gout=None, flags=0, out=None):
    rc = lib.hdrnet_bilateral_slice_apply_io_yuv_p016(grid, guide, *(surf or _surf()), B, H, W, k, GH, GW, GD, Cin, Cout, off,
                                                      c1, c2, n, gout, flags, *(out or _p016_out()), None)
    return rc, lib.hdrnet_last_error().decode()


def _yuv_curves(lib, grid=A, guide=None, surf=None, B=1, H=4, W=8, k=A, GH=2, GW=2, GD=2, Cin=3, Cout=3, off=1, npts=16,
                prepared=None, gout=None, out=None):
    rc = lib.hdrnet_bilateral_slice_apply_io_curves_yuv_p016(grid, *(surf or _surf()), B, H, W, k, GH, GW, GD, Cin, Cout, off,
                                                             A, A, A, A, npts, prepared, gout, *(out or _p016_out()), None)
    return rc, lib.hdrnet_last_error().decode()


SURFACE_REFUSALS = [
    (dict(out=_p016_out(bits=8)), "out_bits must be 10 (P010) or 16 (P016), got 8"),
    (dict(out=_p016_out(bits=12)), "out_bits must be 10 (P010) or 16 (P016), got 12"),
    (dict(surf=_surf(dt=1, py=8, puv=8)), "a P010 / P016 output needs a uint16 surface in"),
    (dict(out=_p016_out(py=8)), "a pitch of the output surface is below the row's 16 bytes"),
    (dict(out=_p016_out(puv=12)), "a pitch of the output surface is below the row's 16 bytes"),
    (dict(out=_p016_out(py=18)), "the pitches of the output surface must be multiples of 4"),
    (dict(B=2, out=_p016_out(suv=16)), "an image stride of the output surface is below its plane"),
    (dict(out=_p016_out(k=None)), "null constants of the output surface"),
    (dict(out=_p016_out(y=None)), "null plane of the output surface"),
    (dict(out=_p016_out(uv=A + 2)), "the planes and constants of the output surface must be 4-B aligned"),
    (dict(surf=_surf(py=8)), "a pitch of the input surface is below the row"),
    (dict(k=None), "null constants of the input surface"),
    (dict(H=5), "H % 2 != 0"),
    (dict(W=6), "W % 4 != 0"),
    (dict(Cout=4), "Cin = Cout = 3 with offset"),
    (dict(grid=None), "null buffer"),
]


@pytest.mark.parametrize("kw,text", SURFACE_REFUSALS)
def test_yuv_p016_refusals(lib, kw, text):
    rc, err = _yuv(lib, **kw)
    assert rc == 1 and err.startswith("hdrnet_bilateral_slice_apply_io_yuv_p016: ") and text in err, (rc, err)


@pytest.mark.parametrize("kw,text", SURFACE_REFUSALS)
def test_curves_yuv_p016_refusals(lib, kw, text):
    rc, err = _yuv_curves(lib, **kw)
    assert rc == 1 and err.startswith("hdrnet_bilateral_slice_apply_io_curves_yuv_p016: ") and text in err, (rc, err)


def test_other_surface_refusals(lib):
    rc, err = _yuv(lib, guide=None)
    assert rc == 1 and "either a guide map or the guide network" in err
    rc, err = _yuv(lib, flags=0x40000)
    assert rc == 1 and "unknown flags" in err
    rc, err = _yuv_curves(lib, npts=0)
    assert rc == 1 and "curve knots" in err
    rc, err = _yuv_curves(lib, prepared=A + 4)
    assert rc == 1 and "prepared curves tables" in err


def test_zero_size_is_a_noop(lib):
    for call in (_px, _px_curves):
        rc, err = call(lib, B=0, grid=None, inp=None, out=None)
        assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"
        rc, err = call(lib, B=0, owl=0.0)  # ... but the values are checked first
        assert rc == 1 and "output_white_level" in err
    empty = _surf(y=None, uv=None)
    for call in (_yuv, _yuv_curves):
        rc, err = call(lib, B=0, grid=None, surf=empty, k=None, out=_p016_out(y=None, uv=None, k=None))
        assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"
        rc, err = call(lib, B=0, surf=empty, out=_p016_out(bits=12))
        assert rc == 1 and "out_bits" in err


# ---- Python refusals on CPU tensors: raised before anything touches the device ------------------------------------------
def test_ops_refuse(lib):
    from hdrnet_amd import hdrnet_ops as ops
    grid = torch.zeros(1, 2, 2, 2, 12)
    guide = torch.zeros(1, 4, 8)
    f16 = torch.zeros(1, 4, 8, 3, dtype=torch.int16).view(torch.uint16)
    with pytest.raises(TypeError, match="a uint16 output needs a uint16 or float32 frame, got uint8"):
        ops.bilateral_slice_apply_io_u16(grid, torch.zeros(1, 4, 8, 3, dtype=torch.uint8), guide=guide)
    for wl in (0.0, -1.0, float("inf"), float("nan"), 65536.0):
        with pytest.raises(ValueError, match="0 < output_white_level <= 65535"):
            ops.bilateral_slice_apply_io_u16(grid, f16, guide=guide, output_white_level=wl)
    with pytest.raises(ValueError, match="float32 frames take pixel_format='rgb' only"):
        ops.bilateral_slice_apply_io_u16(grid, torch.zeros(1, 4, 8, 3), guide=guide, pixel_format="bgr")
    with pytest.raises(ValueError, match="a 4-channel format, the frame has 3 channels"):
        ops.bilateral_slice_apply_io_u16(grid, f16, guide=guide, pixel_format="bgra")
    with pytest.raises(ValueError, match="3 -> 3 op with offset"):
        ops.bilateral_slice_apply_io_u16(torch.zeros(1, 2, 2, 2, 9), f16, guide=guide, has_offset=False)
    with pytest.raises(ValueError, match="either a guide map or both"):
        ops.bilateral_slice_apply_io_u16(grid, f16)
    with pytest.raises(RuntimeError, match="no CPU path"):  # everything else in order: only the device is missing
        ops.bilateral_slice_apply_io_u16(grid, f16, guide=guide, output_white_level=1023.0)
    # the surface twin
    y16, uv16 = (torch.zeros(1, r, 8, dtype=torch.int16).view(torch.uint16) for r in (4, 2))
    y8, uv8 = torch.zeros(1, 4, 8, dtype=torch.uint8), torch.zeros(1, 2, 8, dtype=torch.uint8)
    k = torch.zeros(12)
    with pytest.raises(ValueError, match="needs from_rgb"):
        ops.bilateral_slice_apply_io_yuv_deep(grid, y16, uv16, k, guide=guide, out_bits=10)
    for bits in (8, 12, None):
        with pytest.raises(ValueError, match="out_bits must be 10"):
            ops.bilateral_slice_apply_io_yuv_deep(grid, y16, uv16, k, guide=guide, from_rgb=k, out_bits=bits)
    with pytest.raises(TypeError, match="needs a uint16 surface in"):
        ops.bilateral_slice_apply_io_yuv_deep(grid, y8, uv8, k, guide=guide, from_rgb=k, out_bits=10)
    with pytest.raises(ValueError, match="out_planes should be a uint16 surface"):
        ops.bilateral_slice_apply_io_yuv_deep(grid, y16, uv16, k, guide=guide, from_rgb=k, out_bits=10, out_planes=(y8, uv8))
    with pytest.raises(ValueError, match="exactly one of"):
        ops.bilateral_slice_apply_io_yuv_deep(grid, y16, uv16, k, from_rgb=k, out_bits=16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.bilateral_slice_apply_io_yuv_deep(grid, y16, uv16, k, guide=guide, from_rgb=k, out_bits=16)
    # the existing functions keep refusing a 16-bit output
    with pytest.raises(TypeError, match="out_dtype must be float32 or uint8"):
        ops.bilateral_slice_apply_io_yuv(grid, y16, uv16, k, guide=guide, out_dtype=torch.uint16)
    with pytest.raises(TypeError, match="out_dtype must be float32 or uint8"):
        ops.bilateral_slice_apply_io(grid, f16, guide=guide, out_dtype=torch.uint16)
    with pytest.raises(ValueError, match="unknown out 'p010'"):
        ops.bilateral_slice_apply_io_yuv(grid, y16, uv16, k, guide=guide, out="p010", from_rgb=k)


@pytest.mark.parametrize("cls", ["HDRNetCurves", "HDRNetPointwiseNNGuide"])
def test_models_refuse(lib, cls):
    from hdrnet_amd import models
    torch.manual_seed(3)
    m = getattr(models, cls)(dict(batch_norm=False)).eval()
    f8 = torch.zeros(1, 32, 48, 3, dtype=torch.uint8)
    f16 = torch.zeros(1, 32, 48, 3, dtype=torch.int16).view(torch.uint16)
    with pytest.raises(TypeError, match="a uint16 output needs a uint16 or float32 frame, got uint8"):
        m.process(f8, out_dtype=torch.uint16)
    with pytest.raises(ValueError, match="out_white_level belongs to out_dtype=torch.uint16"):
        m.process(f16, out_dtype=torch.uint8, out_white_level=1023.0)
    with pytest.raises(ValueError, match="0 < output_white_level <= 65535"):
        m.process(f16, out_dtype=torch.uint16, out_white_level=0.0)
    with pytest.raises(TypeError, match="out_dtype must be float32, uint8 or uint16"):
        m.process(f16, out_dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP|no CPU path"):  # everything else in order: only the device is missing
        m.process(f16, out_dtype=torch.uint16)
    y8, uv8 = torch.zeros(1, 32, 48, dtype=torch.uint8), torch.zeros(1, 16, 48, dtype=torch.uint8)
    y16, uv16 = (t.to(torch.int16).view(torch.uint16) for t in (y8, uv8))
    with pytest.raises(TypeError, match="out='p010' needs a uint16 surface in"):
        m.process_yuv(y8, uv8, out="p010")
    with pytest.raises(TypeError, match="a P016 output is uint16"):
        m.process_yuv(y16, uv16, out="p016", out_dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP|no CPU path"):
        m.process_yuv(y16, uv16, bits=10, out="p010")


def test_pyramid_keeps_refusing(lib):
    from hdrnet_amd import models
    torch.manual_seed(3)
    m = models.HDRNetGaussianPyrNN(dict(batch_norm=False)).eval()
    f16 = torch.zeros(1, 32, 48, 3, dtype=torch.int16).view(torch.uint16)
    with pytest.raises(TypeError, match="out_dtype must be float32 or uint8"):
        m.process_wire(f16, out_dtype=torch.uint16)
    with pytest.raises(TypeError, match="returns float32 frames only"):
        m.process(torch.zeros(1, 32, 48, 3), out_dtype=torch.uint16)


# ---- the encoder's constants ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full_range", [False, True])
@pytest.mark.parametrize("standard", ["bt601", "bt709", "bt2020"])
def test_encode_coefficients(standard, full_range):
    from hdrnet_amd import yuv
    k8 = yuv.yuv_encode_coefficients(standard, full_range, 8)
    assert k8.dtype == np.float32 and k8.shape == (12,)
    assert np.array_equal(k8.view(np.uint32), yuv.yuv_coefficients(standard, full_range, 8)[1].view(np.uint32))
    for bits in (10, 16):
        # the encoder in code units of the decoder's depth, whatever depth yuv_coefficients' own (8-bit) encoder has
        for dec_bits in (8, bits):
            assert np.array_equal(yuv.yuv_coefficients(standard, full_range, dec_bits)[1].view(np.uint32), k8.view(np.uint32))
        to_rgb = np.asarray(yuv.yuv_coefficients(standard, full_range, bits)[0], np.float64)
        from_rgb = np.asarray(yuv.yuv_encode_coefficients(standard, full_range, bits), np.float64)
        # every grey code of the legal range: float64 decoding, then float64 encoding, returns the code
        unit = 2 ** (bits - 8)
        lo, hi, mid = (0, 2 ** bits - 1, 2 ** (bits - 1)) if full_range else (16 * unit, 235 * unit, 128 * unit)
        codes = np.arange(lo, hi + 1, dtype=np.float64)
        stored = codes * (64.0 if bits == 10 else 1.0)  # the decoder reads the sample AS STORED (P010: code << 6)
        mid_s = mid * (64.0 if bits == 10 else 1.0)
        rgb = np.stack([to_rgb[3 * i] * stored + (to_rgb[3 * i + 1] + to_rgb[3 * i + 2]) * mid_s + to_rgb[9 + i]
                        for i in range(3)], axis=-1)
        assert rgb.min() > -1e-6 and rgb.max() < 1 + 1e-6 and np.ptp(rgb, axis=-1).max() < 1e-6  # grey, inside [0, 1]
        rgb = np.clip(rgb, 0.0, 1.0)
        yuv_pre = np.stack([rgb @ from_rgb[3 * i:3 * i + 3] + from_rgb[9 + i] for i in range(3)], axis=-1)
        got = np.floor(np.clip(yuv_pre, 0.0, uc.code_max(bits)))
        assert np.array_equal(got[:, 0], codes), (bits, np.argwhere(got[:, 0] != codes)[:4])
        assert np.all(got[:, 1:] == mid)
        assert np.abs(yuv_pre[:, 0] - codes - 0.5).max() < 0.02 * unit ** 0  # ... decided by the + 0.5, not by luck


def test_encode_coefficients_refuse():
    from hdrnet_amd import yuv
    with pytest.raises(ValueError, match="unknown standard"):
        yuv.yuv_encode_coefficients("bt470")
    with pytest.raises(ValueError, match="bits must be one of"):
        yuv.yuv_encode_coefficients("bt709", False, 12)


# ---- the helper's own statement of the rules ---------------------------------------------------------------------------
def test_helper():
    import yuv_cases as yc
    from hdrnet_amd import yuv
    f = np.array([-0.5, 0.0, 0.25, 0.99999, 1.0, 7.0], np.float32)
    assert list(uc.quantise_u16(f, 65535.0)) == [0, 0, 16383, 65534, 65535, 65535]
    assert list(uc.quantise_u16(f, 1023.0)) == [0, 0, 255, 1022, 1023, 1023]
    rng = np.random.default_rng(5)
    rgb = rng.random((2, 4, 8, 3))
    # at 8 bits and shift 8 the generalised encoder is yuv_cases' NV12 encoder
    k8 = yuv.yuv_encode_coefficients("bt709", False, 8)
    y8, uv8, y_pre8, _ = yc.encode_nv12_64(rgb, k8)
    y, uv, y_pre, _ = uc.encode_p016_64(rgb, k8, 8)
    assert np.array_equal(y >> 8, y8) and np.array_equal(uv >> 8, uv8) and np.array_equal(y_pre, y_pre8)
    assert np.array_equal(uc.decided(y_pre, 8), yc.decided(y_pre8))
    for bits in (10, 16):
        y, uv, y_pre, uv_pre = uc.encode_p016_64(rgb, yuv.yuv_encode_coefficients("bt709", False, bits), bits)
        assert y.dtype == np.uint16 and y.shape == (2, 4, 8) and uv.shape == (2, 2, 8)
        assert not np.any(y & ((1 << (16 - bits)) - 1)) and not np.any(uv & ((1 << (16 - bits)) - 1))
        assert np.array_equal(y >> (16 - bits), np.floor(np.clip(y_pre, 0, 2 ** bits - 1)).astype(np.uint16))
        assert uc.code_diff(y, y, bits).max() == 0
    assert uc.eps_of(8) == 1e-3 and uc.eps_of(10) == 4e-3 and uc.eps_of(16) == 0.256
