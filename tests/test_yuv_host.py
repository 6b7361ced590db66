"""YUV surfaces without a GPU (include/hdrnet_amd_yuv.h): the four entry points are exported and bound as declared, refuse
what the rules exclude with rc = 1 and a text that names the rule before any HIP call, the Python layers above them raise
before anything touches the device, and ``yuv.yuv_coefficients`` holds its anchors for every standard, range and depth."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import yuv_cases as yc
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hdrnet_amd_yuv.h")
A = 0x1000  # a 16-byte aligned non-null "device pointer": never dereferenced, every row below is refused first
NAMES = ["hdrnet_bilateral_slice_apply_io_curves_yuv", "hdrnet_bilateral_slice_apply_io_yuv", "hdrnet_lowres_input_yuv",
         "hdrnet_yuv_to_rgb_f32"]


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for name, (res, args) in _lib.YUV_SIGNATURES.items():
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


def test_symbols_exported_and_bound_as_declared(lib):
    from hdrnet_amd import _lib
    decl = _declared()
    assert sorted(decl) == sorted(_lib.YUV_SIGNATURES) == NAMES
    for name, params in decl.items():
        res, args = _lib.YUV_SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for ctype, text in zip(args, params):  # pointer / long long / int / unsigned, position by position
            want = (ctypes.c_void_p if "*" in text else ctypes.c_longlong if text.startswith("long long ")
                    else ctypes.c_uint if text.startswith("unsigned") else ctypes.c_int)
            assert ctype is want, (name, text, ctype)
        assert hasattr(lib, name)
    # a header and a table of their own: the other tables still mirror their headers
    assert not set(decl) & set(_lib.SIGNATURES) and not set(decl) & set(_lib.PIXEL_FORMAT_SIGNATURES)
    assert hasattr(_lib.load(), "hdrnet_yuv_to_rgb_f32")  # ... and the package's handle binds them
    assert lib.hdrnet_version() >= 287
    text = open(HEADER).read()
    for name, code in _lib.YUV_OUT.items():
        assert re.search(r"#define HDRNET_YUV_OUT_%s %d\b" % (name.upper(), code), text), name
    assert "replicated" in text.lower() and "out of scope" in text.lower()


# a surface: y, uv, dtype, pitch_y, pitch_uv, image_stride_y, image_stride_uv
def _surf(y=A, uv=A, dt=1, py=8, puv=8, sy=32, suv=16):
    return [y, uv, dt, py, puv, sy, suv]


def _out(kind=1, out=A, out_uv=None, py=0, puv=0, sy=0, suv=0, k=None):
    return [kind, out, out_uv, py, puv, sy, suv, k]


def _io(lib, grid=A, guide=A, surf=None, B=1, H=4, W=8, k=A, GH=2, GW=2, GD=2, Cin=3, Cout=3, off=1, c1=None, c2=None, n=0,
        gout=None, flags=0, out=None):
    rc = lib.hdrnet_bilateral_slice_apply_io_yuv(grid, guide, *(surf or _surf()), B, H, W, k, GH, GW, GD, Cin, Cout, off, c1,
                                                 c2, n, gout, flags, *(out or _out()), None)
    return rc, lib.hdrnet_last_error().decode()


def _curves(lib, grid=A, guide=None, surf=None, B=1, H=4, W=8, k=A, GH=2, GW=2, GD=2, Cin=3, Cout=3, off=1, npts=16,
            prepared=None, gout=None, out=None):
    rc = lib.hdrnet_bilateral_slice_apply_io_curves_yuv(grid, *(surf or _surf()), B, H, W, k, GH, GW, GD, Cin, Cout, off, A, A,
                                                        A, A, npts, prepared, gout, *(out or _out()), None)
    return rc, lib.hdrnet_last_error().decode()


def _to_rgb(lib, surf=None, B=1, H=4, W=8, k=A, rgb=A):
    rc = lib.hdrnet_yuv_to_rgb_f32(*(surf or _surf()), B, H, W, k, rgb, None)
    return rc, lib.hdrnet_last_error().decode()


def _lowres(lib, surf=None, B=1, H=4, W=8, k=A, lowres=A, n=4):
    rc = lib.hdrnet_lowres_input_yuv(*(surf or _surf()), B, H, W, k, lowres, n, None)
    return rc, lib.hdrnet_last_error().decode()


NV12_OUT = dict(kind=2, out=A, out_uv=A, py=8, puv=8, sy=32, suv=16, k=A)
SURFACE_REFUSALS = [  # the rules of the input surface: the same for all four entry points
    (dict(H=5), "H % 2 != 0"),
    (dict(W=6), "W % 4 != 0"),
    (dict(surf=_surf(py=4)), "below the row"),
    (dict(surf=_surf(puv=4)), "below the row"),
    (dict(surf=_surf(dt=2, sy=64, suv=32)), "below the row"),       # uint16: 8 samples are 16 bytes
    (dict(surf=_surf(py=10)), "multiples of 4"),
    (dict(surf=_surf(puv=14)), "multiples of 4"),
    (dict(surf=_surf(sy=30)), "image strides"),
    (dict(B=2, surf=_surf(sy=16)), "below its plane"),
    (dict(surf=_surf(y=None)), "null plane"),
    (dict(surf=_surf(uv=None)), "null plane"),
    (dict(k=None), "null constants"),
    (dict(surf=_surf(y=A + 2)), "4-B aligned"),
    (dict(surf=_surf(dt=0)), "unknown sample dtype"),
    (dict(surf=_surf(dt=3)), "unknown sample dtype"),
]
IO_REFUSALS = SURFACE_REFUSALS + [
    (dict(out=_out(kind=3)), "unknown output kind"),
    (dict(out=_out(kind=-1)), "unknown output kind"),
    (dict(Cin=4, Cout=4), "Cin = Cout = 3 with offset"),
    (dict(Cout=4), "Cin = Cout = 3 with offset"),
    (dict(off=0), "Cin = Cout = 3 with offset"),
    (dict(out=_out(out=None)), "null or misaligned out"),
    (dict(out=_out(kind=0, out=A + 4)), "null or misaligned out"),
    (dict(out=_out(**dict(NV12_OUT, py=4))), "below the row"),
    (dict(out=_out(**dict(NV12_OUT, puv=10))), "multiples of 4"),
    (dict(out=_out(**dict(NV12_OUT, out_uv=None))), "null plane of the output surface"),
    (dict(out=_out(**dict(NV12_OUT, k=None))), "null constants of the output surface"),
    (dict(grid=None), "null buffer"),
]


@pytest.mark.parametrize("kw,text", IO_REFUSALS)
def test_io_yuv_refusals(lib, kw, text):
    rc, err = _io(lib, **kw)
    assert rc == 1 and err.startswith("hdrnet_bilateral_slice_apply_io_yuv: ") and text in err, (rc, err)


@pytest.mark.parametrize("kw,text", IO_REFUSALS)
def test_io_curves_yuv_refusals(lib, kw, text):
    rc, err = _curves(lib, **kw)
    assert rc == 1 and err.startswith("hdrnet_bilateral_slice_apply_io_curves_yuv: ") and text in err, (rc, err)


@pytest.mark.parametrize("kw,text", SURFACE_REFUSALS + [(dict(rgb=None), "rgb must be"), (dict(rgb=A + 4), "rgb must be")])
def test_yuv_to_rgb_refusals(lib, kw, text):
    rc, err = _to_rgb(lib, **kw)
    assert rc == 1 and err.startswith("hdrnet_yuv_to_rgb_f32: ") and text in err, (rc, err)


@pytest.mark.parametrize("kw,text", SURFACE_REFUSALS + [(dict(lowres=None), "lowres must be"), (dict(n=0), "non-positive extent")])
def test_lowres_yuv_refusals(lib, kw, text):
    rc, err = _lowres(lib, **kw)
    assert rc == 1 and err.startswith("hdrnet_lowres_input_yuv: ") and text in err, (rc, err)


def test_other_refusals(lib):
    rc, err = _io(lib, guide=None)
    assert rc == 1 and "either a guide map or the guide network" in err
    rc, err = _io(lib, flags=0x40000)
    assert rc == 1 and "unknown flags" in err
    rc, err = _curves(lib, npts=0)
    assert rc == 1 and "curve knots" in err
    rc, err = _curves(lib, prepared=A + 4)
    assert rc == 1 and "prepared curves tables" in err


def test_empty_batch_is_a_noop(lib):
    empty = _surf(y=None, uv=None)
    for call in (_io, _curves):
        rc, err = call(lib, B=0, surf=empty, k=None, out=_out(out=None))
        assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"
        rc, err = call(lib, B=0, surf=empty, k=None, out=_out(**dict(NV12_OUT, out=None, out_uv=None, k=None)))
        assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"
    rc, err = _to_rgb(lib, B=0, surf=empty, k=None, rgb=None)
    assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"
    rc, err = _lowres(lib, B=0, surf=empty, k=None, lowres=None)
    assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"


# ---- Python refusals on CPU tensors: raised before anything touches the device ------------------------------------------
def test_ops_refuse(lib):
    from hdrnet_amd import data, hdrnet_ops as ops
    grid = torch.zeros(1, 2, 2, 2, 12)
    guide = torch.zeros(1, 4, 8)
    y, uv = torch.zeros(1, 4, 8, dtype=torch.uint8), torch.zeros(1, 2, 8, dtype=torch.uint8)
    k = torch.zeros(12)
    with pytest.raises(ValueError, match="H must be even"):
        ops.yuv_to_rgb(y[:, :3], uv, k)
    with pytest.raises(ValueError, match="W % 4 != 0"):
        ops.yuv_to_rgb(y[:, :, :6], uv[:, :, :6], k)
    with pytest.raises(ValueError, match=r"uv should be \[B, H / 2, W\]"):
        ops.yuv_to_rgb(y, uv[:, :1], k)
    with pytest.raises(TypeError, match="must both be uint8"):
        ops.yuv_to_rgb(y, uv.to(torch.int16), k)
    with pytest.raises(TypeError, match="must both be uint8"):
        ops.yuv_to_rgb(y.float(), uv.float(), k)
    with pytest.raises(ValueError, match="last-dimension stride 1"):
        ops.yuv_to_rgb(torch.zeros(1, 4, 16, dtype=torch.uint8)[:, :, ::2], uv, k)
    with pytest.raises(ValueError, match="12 floats"):
        ops.yuv_to_rgb(y, uv, torch.zeros(9))
    with pytest.raises(RuntimeError, match="no CPU path"):  # everything else in order: only the device is missing
        ops.yuv_to_rgb(y, uv, k)
    with pytest.raises(ValueError, match="unknown out 'i420'"):
        ops.bilateral_slice_apply_io_yuv(grid, y, uv, k, guide=guide, out="i420")
    with pytest.raises(ValueError, match="needs from_rgb"):
        ops.bilateral_slice_apply_io_yuv(grid, y, uv, k, guide=guide, out="nv12")
    with pytest.raises(TypeError, match="an NV12 output is uint8"):
        ops.bilateral_slice_apply_io_yuv(grid, y, uv, k, guide=guide, out="nv12", out_dtype=torch.float32, from_rgb=k)
    with pytest.raises(TypeError, match="out_dtype must be float32 or uint8"):
        ops.bilateral_slice_apply_io_yuv(grid, y, uv, k, guide=guide, out_dtype=torch.uint16)
    with pytest.raises(ValueError, match="3 -> 3 op with offset"):
        ops.bilateral_slice_apply_io_yuv(torch.zeros(1, 2, 2, 2, 9), y, uv, k, guide=guide)
    with pytest.raises(ValueError, match="exactly one of"):
        ops.bilateral_slice_apply_io_yuv(grid, y, uv, k)
    with pytest.raises(ValueError, match="out_planes should be a uint8 surface"):
        ops.bilateral_slice_apply_io_yuv(grid, y, uv, k, guide=guide, out="nv12", from_rgb=k,
                                         out_planes=(torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 4, 8, dtype=torch.uint8)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.bilateral_slice_apply_io_yuv(grid, y, uv, k, guide=guide, out="nv12", from_rgb=k)
    with pytest.raises(ValueError, match="H must be even"):
        data.lowres_input_yuv(y[:, :3], uv, k, 4)
    with pytest.raises(RuntimeError, match="HIP"):
        data.lowres_input_yuv(y, uv, k, 4)


@pytest.mark.parametrize("cls", ["HDRNetCurves", "HDRNetPointwiseNNGuide"])
def test_process_yuv_refuses(lib, cls):
    from hdrnet_amd import models
    torch.manual_seed(3)
    m = getattr(models, cls)(dict(batch_norm=False)).eval()
    y, uv = torch.zeros(1, 32, 48, dtype=torch.uint8), torch.zeros(1, 16, 48, dtype=torch.uint8)
    with pytest.raises(ValueError, match="unknown standard 'bt470'"):
        m.process_yuv(y, uv, standard="bt470")
    with pytest.raises(ValueError, match="unknown out 'bgr'"):
        m.process_yuv(y, uv, out="bgr")
    with pytest.raises(ValueError, match="does not fit torch.uint8 planes"):
        m.process_yuv(y, uv, bits=10)
    with pytest.raises(ValueError, match="does not fit torch.uint16 planes"):
        m.process_yuv(y.to(torch.int16).view(torch.uint16), uv.to(torch.int16).view(torch.uint16), bits=8)
    with pytest.raises(ValueError, match="H must be even"):
        m.process_yuv(y[:, :31], uv)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.process_yuv(y, uv)
    # the RGB front door is what it was: "yuv" is no pixel format
    with pytest.raises(ValueError, match="unknown pixel_format 'yuv'"):
        m.process(torch.zeros(1, 32, 48, 3, dtype=torch.uint8), pixel_format="yuv")


def test_pyramid_process_yuv_refuses(lib):
    from hdrnet_amd import models
    torch.manual_seed(3)
    m = models.HDRNetGaussianPyrNN(dict(batch_norm=False)).eval()
    y, uv = torch.zeros(1, 32, 48, dtype=torch.uint8), torch.zeros(1, 16, 48, dtype=torch.uint8)
    with pytest.raises(ValueError, match="the pyramid model's resize and up-add kernels read RGB frames only"):
        m.process_yuv(y, uv)


# ---- the colour constants ------------------------------------------------------------------------------------------------
def _apply(k, v):
    k = np.asarray(k, np.float64)
    return np.array([k[3 * i] * v[0] + k[3 * i + 1] * v[1] + k[3 * i + 2] * v[2] + k[9 + i] for i in range(3)])


@pytest.mark.parametrize("bits", [8, 10, 16])
@pytest.mark.parametrize("full_range", [False, True])
@pytest.mark.parametrize("standard", ["bt601", "bt709", "bt2020"])
def test_coefficient_anchors(standard, full_range, bits):
    from hdrnet_amd import yuv
    to_rgb, from_rgb = yuv.yuv_coefficients(standard, full_range, bits)
    assert to_rgb.dtype == np.float32 and from_rgb.dtype == np.float32 and to_rgb.shape == from_rgb.shape == (12,)
    shift = yc.stored_shift(bits)
    unit = 2 ** (bits - 8)
    black, white, mid = (0, 2 ** bits - 1, 2 ** (bits - 1)) if full_range else (16 * unit, 235 * unit, 128 * unit)
    stored = lambda *codes: [c << shift for c in codes]  # noqa: E731
    # black and white code points map to 0 and 1
    np.testing.assert_allclose(_apply(to_rgb, stored(black, mid, mid)), 0.0, atol=1e-6)
    np.testing.assert_allclose(_apply(to_rgb, stored(white, mid, mid)), 1.0, atol=1e-6)
    # neutral chroma gives R = G = B
    for code in (black + 7 * unit, (black + white) // 2, white - 3 * unit):
        c = _apply(to_rgb, stored(code, mid, mid))
        assert np.ptp(c) < 1e-6, (code, c)
    # from_rgb o to_rgb is the identity on (uint8-equivalent) code values, the + 0.5 of the rounding included: in-gamut
    # codes, i.e. those of RGB triples inside the unit cube
    rng = np.random.default_rng([11, bits, int(full_range)])
    kr, kb = yuv.STANDARDS[standard]
    lum = np.array([kr, 1.0 - kr - kb, kb])
    y_off, y_scale, c_off, c_scale = yuv.code_ranges(full_range, bits)
    y8_off, y8_scale, c8_off, c8_scale = yuv.code_ranges(full_range, 8)
    for rgb in rng.random((64, 3)) * 0.9 + 0.05:
        yl = float(lum @ rgb)
        nominal = np.array([yl, (rgb[2] - yl) / (2 * (1 - kb)), (rgb[0] - yl) / (2 * (1 - kr))])  # Y', Cb', Cr'
        codes = np.rint(np.array([y_off, c_off, c_off]) + np.array([y_scale, c_scale, c_scale]) * nominal)  # of `bits` bits
        back_nominal = (codes - np.array([y_off, c_off, c_off])) / np.array([y_scale, c_scale, c_scale])
        want8 = np.array([y8_off, c8_off, c8_off]) + np.array([y8_scale, c8_scale, c8_scale]) * back_nominal
        got = _apply(from_rgb, _apply(to_rgb, stored(*[int(c) for c in codes])))
        assert np.all(np.abs(got - want8) <= 0.51), (rgb, codes, got, want8)
        assert np.all(np.abs(got - 0.5 - want8) <= 0.01)  # ... of which 0.5 is the rounding term
    if standard == "bt601" and not full_range:  # the textbook point: red (1, 0, 0) -> (81, 90, 240)
        code = np.floor(_apply(from_rgb, [1.0, 0.0, 0.0]))
        assert np.all(np.abs(code - np.array([81, 90, 240])) <= 1), code


def test_coefficients_refuse():
    from hdrnet_amd import yuv
    with pytest.raises(ValueError, match="unknown standard"):
        yuv.yuv_coefficients("bt470")
    with pytest.raises(ValueError, match="bits must be one of"):
        yuv.yuv_coefficients("bt709", False, 12)


# ---- the helper's own statement of the rules ---------------------------------------------------------------------------
def test_helper():
    from hdrnet_amd import yuv
    rng = np.random.default_rng(5)
    for bits in (8, 10, 16):
        y, uv = yc.random_surface(rng, (2, 4, 8), bits, pad_bytes=64)
        W = 8
        assert y.shape == (2, 4, 8 + 64 // y.itemsize) and uv.shape == (2, 2, y.shape[2])
        assert yc.padding_intact(y, W) and yc.padding_intact(uv, W)
        assert int(y[:, :, :W].max()) == (2 ** bits - 1) << yc.stored_shift(bits) and int(y[:, :, :W].min()) == 0
        to_rgb, from_rgb = yuv.yuv_coefficients("bt709", False, bits)
        rgb = yc.to_rgb64(y[:, :, :W], uv[:, :, :W], to_rgb)
        assert rgb.shape == (2, 4, 8, 3) and rgb.min() == 0.0 and rgb.max() == 1.0  # the corners clamp
        assert np.array_equal(rgb[:, 0, 0], rgb[:, 0, 1] * 0) and np.array_equal(rgb[:, 0, W - 1], np.ones((2, 3)))
        yq, uvq, y_pre, uv_pre = yc.encode_nv12_64(rgb, from_rgb)
        assert yq.shape == (2, 4, 8) and uvq.shape == (2, 2, 8) and yq.dtype == np.uint8
        assert np.array_equal(yq, np.floor(np.clip(y_pre, 0, 255)).astype(np.uint8))
        assert yq[0, 0, 0] == 16 and yq[0, 0, W - 1] == 235
    assert list(yc.decided(np.array([3.5, 4.0005, 3.9995, 300.0, 255.0004, -7.0]))) == [True, False, False, True, False, True]
