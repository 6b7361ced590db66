"""Planar YUV surfaces without a GPU (include/hdrnet_amd_yuv_planar.h): the four entry points are exported and bound as
declared, refuse what the rules exclude with rc = 1 and a text that names the rule before any HIP call, the Python layers
above them raise before anything touches the device, ``yuv.yuv_coefficients(..., msb_aligned=False)`` is the default's
numbers with the P010 shift taken out, and the numpy helpers of tests/yuv_planar_cases.py say what their comments say."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import yuv_cases as yc
import yuv_planar_cases as pc
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hdrnet_amd_yuv_planar.h")
A = 0x1000  # a 16-byte aligned non-null "device pointer": never dereferenced, every row below is refused first
NAMES = ["hdrnet_bilateral_slice_apply_io_curves_yuv_planar", "hdrnet_bilateral_slice_apply_io_yuv_planar",
         "hdrnet_lowres_input_yuv_planar", "hdrnet_yuv_planar_to_rgb_f32"]


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for name, (res, args) in _lib.YUV_PLANAR_SIGNATURES.items():
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
    assert sorted(decl) == sorted(_lib.YUV_PLANAR_SIGNATURES) == NAMES
    for name, params in decl.items():
        res, args = _lib.YUV_PLANAR_SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for ctype, text in zip(args, params):  # pointer / long long / int / unsigned, position by position
            want = (ctypes.c_void_p if "*" in text else ctypes.c_longlong if text.startswith("long long ")
                    else ctypes.c_uint if text.startswith("unsigned") else ctypes.c_int)
            assert ctype is want, (name, text, ctype)
        assert hasattr(lib, name)
    # a header and a table of their own: the other tables still mirror their headers
    assert not set(decl) & set(_lib.SIGNATURES) and not set(decl) & set(_lib.YUV_SIGNATURES)
    assert hasattr(_lib.load(), "hdrnet_yuv_planar_to_rgb_f32")  # ... and the package's handle binds them
    assert lib.hdrnet_version() >= 289
    text = open(HEADER).read()
    for name, code in _lib.YUV_PLANAR_OUT.items():
        assert re.search(r"#define HDRNET_YUV_PLANAR_OUT_%s %d\b" % (name.upper(), code), text), name
    assert "replicated" in text.lower() and "out of scope" in text.lower() and "low bits" in text.lower()
    # the semi-planar header no longer lists planar surfaces as out of scope
    semi = open(os.path.join(ROOT, "include", "hdrnet_amd_yuv.h")).read()
    assert "planar (I420)" not in semi and "hdrnet_amd_yuv_planar.h" in semi


# a planar surface of H = 4, W = 8: y, u, v, dtype, pitch_y, pitch_u, pitch_v, image strides y, u, v
def _surf(y=A, u=A, v=A, dt=1, py=8, pu=4, pv=4, sy=32, su=8, sv=8):
    return [y, u, v, dt, py, pu, pv, sy, su, sv]


U16 = dict(dt=2, py=16, pu=8, pv=8, sy=64, su=16, sv=16)


def _out(kind=1, out=A, out_u=None, out_v=None, py=0, pu=0, pv=0, sy=0, su=0, sv=0, k=None, bits=0):
    return [kind, out, out_u, out_v, py, pu, pv, sy, su, sv, k, bits]


def _io(lib, grid=A, guide=A, surf=None, B=1, H=4, W=8, k=A, GH=2, GW=2, GD=2, Cin=3, Cout=3, off=1, c1=None, c2=None, n=0,
        gout=None, flags=0, out=None):
    rc = lib.hdrnet_bilateral_slice_apply_io_yuv_planar(grid, guide, *(surf or _surf()), B, H, W, k, GH, GW, GD, Cin, Cout,
                                                        off, c1, c2, n, gout, flags, *(out or _out()), None)
    return rc, lib.hdrnet_last_error().decode()


def _curves(lib, grid=A, guide=None, surf=None, B=1, H=4, W=8, k=A, GH=2, GW=2, GD=2, Cin=3, Cout=3, off=1, npts=16,
            prepared=None, gout=None, out=None):
    rc = lib.hdrnet_bilateral_slice_apply_io_curves_yuv_planar(grid, *(surf or _surf()), B, H, W, k, GH, GW, GD, Cin, Cout,
                                                               off, A, A, A, A, npts, prepared, gout, *(out or _out()), None)
    return rc, lib.hdrnet_last_error().decode()


def _to_rgb(lib, surf=None, B=1, H=4, W=8, k=A, rgb=A):
    rc = lib.hdrnet_yuv_planar_to_rgb_f32(*(surf or _surf()), B, H, W, k, rgb, None)
    return rc, lib.hdrnet_last_error().decode()


def _lowres(lib, surf=None, B=1, H=4, W=8, k=A, lowres=A, n=4):
    rc = lib.hdrnet_lowres_input_yuv_planar(*(surf or _surf()), B, H, W, k, lowres, n, None)
    return rc, lib.hdrnet_last_error().decode()


PLANAR_OUT = dict(kind=2, out=A, out_u=A, out_v=A, py=8, pu=4, pv=4, sy=32, su=8, sv=8, k=A, bits=8)
PLANAR_OUT16 = dict(kind=2, out=A, out_u=A, out_v=A, py=16, pu=8, pv=8, sy=64, su=16, sv=16, k=A, bits=16)
SURFACE_REFUSALS = [  # the rules of the input surface: the same for all four entry points
    (dict(H=5), "H % 2 != 0"),
    (dict(W=6), "W % 4 != 0"),
    (dict(surf=_surf(py=4)), "below the row"),
    (dict(surf=_surf(pu=2)), "below the row"),
    (dict(surf=_surf(pv=2)), "below the row"),
    (dict(surf=_surf(**dict(U16, py=8))), "below the row"),          # uint16: 8 samples are 16 bytes ...
    (dict(surf=_surf(**dict(U16, pv=4))), "below the row"),          # ... and 4 chroma samples are 8
    (dict(surf=_surf(py=10)), "must be multiples of 4 (luma) and of 2 (uint8 chroma)"),
    (dict(surf=_surf(pu=5)), "must be multiples of 4 (luma) and of 2 (uint8 chroma)"),
    (dict(surf=_surf(**dict(U16, pu=10))), "must be multiples of 4 (luma) and of 4 (uint16 chroma)"),
    (dict(surf=_surf(sy=30)), "image strides"),
    (dict(surf=_surf(sv=9)), "image strides"),
    (dict(surf=_surf(**dict(U16, su=18))), "image strides"),
    (dict(surf=_surf(su=-2)), "image strides"),
    (dict(B=2, surf=_surf(sy=16)), "below its plane"),
    (dict(B=2, surf=_surf(su=6)), "below its plane"),
    (dict(B=2, surf=_surf(sv=4)), "below its plane"),
    (dict(surf=_surf(y=None)), "null plane"),
    (dict(surf=_surf(u=None)), "null plane"),
    (dict(surf=_surf(v=None)), "null plane"),
    (dict(k=None), "null constants"),
    (dict(surf=_surf(y=A + 2)), "Y plane and constants of the input surface must be 4-B aligned"),
    (dict(surf=_surf(u=A + 1)), "chroma planes of the input surface must be 2-B aligned"),
    (dict(surf=_surf(**dict(U16, v=A + 2))), "chroma planes of the input surface must be 4-B aligned"),
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
    # a depth that does not fit the sample dtype: 10 or 16 bits for uint8 samples, 8 for uint16 (no 16 -> 8 bit kernel)
    (dict(out=_out(**dict(PLANAR_OUT, bits=10))), "out_bits does not fit the sample dtype"),
    (dict(out=_out(**dict(PLANAR_OUT, bits=16))), "out_bits does not fit the sample dtype"),
    (dict(surf=_surf(**U16), out=_out(**dict(PLANAR_OUT16, bits=8))), "out_bits does not fit the sample dtype"),
    (dict(surf=_surf(**U16), out=_out(**dict(PLANAR_OUT16, bits=12))), "out_bits does not fit the sample dtype"),
    (dict(out=_out(**dict(PLANAR_OUT, py=4))), "below the row"),
    (dict(out=_out(**dict(PLANAR_OUT, pv=3))), "below the row"),
    (dict(out=_out(**dict(PLANAR_OUT, pu=7))), "the pitches of the output surface"),
    (dict(surf=_surf(**U16), out=_out(**dict(PLANAR_OUT16, pu=10))), "the pitches of the output surface"),
    (dict(B=2, out=_out(**dict(PLANAR_OUT, sv=6))), "an image stride of the output surface is below its plane"),
    (dict(out=_out(**dict(PLANAR_OUT, out_u=None))), "null plane of the output surface"),
    (dict(out=_out(**dict(PLANAR_OUT, out_v=None))), "null plane of the output surface"),
    (dict(out=_out(**dict(PLANAR_OUT, out_v=A + 1))), "chroma planes of the output surface must be 2-B aligned"),
    (dict(out=_out(**dict(PLANAR_OUT, k=None))), "null constants of the output surface"),
    (dict(grid=None), "null buffer"),
]


@pytest.mark.parametrize("kw,text", IO_REFUSALS)
def test_io_yuv_planar_refusals(lib, kw, text):
    rc, err = _io(lib, **kw)
    assert rc == 1 and err.startswith("hdrnet_bilateral_slice_apply_io_yuv_planar: ") and text in err, (rc, err)


@pytest.mark.parametrize("kw,text", IO_REFUSALS)
def test_io_curves_yuv_planar_refusals(lib, kw, text):
    rc, err = _curves(lib, **kw)
    assert rc == 1 and err.startswith("hdrnet_bilateral_slice_apply_io_curves_yuv_planar: ") and text in err, (rc, err)


@pytest.mark.parametrize("kw,text", SURFACE_REFUSALS + [(dict(rgb=None), "rgb must be"), (dict(rgb=A + 4), "rgb must be")])
def test_yuv_planar_to_rgb_refusals(lib, kw, text):
    rc, err = _to_rgb(lib, **kw)
    assert rc == 1 and err.startswith("hdrnet_yuv_planar_to_rgb_f32: ") and text in err, (rc, err)


@pytest.mark.parametrize("kw,text", SURFACE_REFUSALS + [(dict(lowres=None), "lowres must be"), (dict(n=0), "non-positive extent")])
def test_lowres_yuv_planar_refusals(lib, kw, text):
    rc, err = _lowres(lib, **kw)
    assert rc == 1 and err.startswith("hdrnet_lowres_input_yuv_planar: ") and text in err, (rc, err)


def test_other_refusals(lib):
    rc, err = _io(lib, guide=None)
    assert rc == 1 and "either a guide map or the guide network" in err
    rc, err = _io(lib, flags=0x40000)
    assert rc == 1 and "unknown flags" in err
    rc, err = _curves(lib, npts=0)
    assert rc == 1 and "curve knots" in err
    rc, err = _curves(lib, prepared=A + 4)
    assert rc == 1 and "prepared curves tables" in err


def test_tight_planes_of_w_100_pass_the_surface_rules(lib):
    """W = 100: a tight uint8 chroma row is 50 bytes, so rows start 2 bytes past a dword boundary -- admitted; the call gets
    as far as the null grid.  A chroma base 2 bytes past a dword boundary likewise."""
    tight = _surf(u=A + 2, v=A + 6, py=100, pu=50, pv=50, sy=400, su=100, sv=100)
    rc, err = _io(lib, grid=None, surf=tight, W=100)
    assert rc == 1 and "null buffer (grid)" in err, err
    out = _out(kind=2, out=A, out_u=A + 2, out_v=A + 6, py=100, pu=50, pv=50, sy=400, su=100, sv=100, k=A, bits=8)
    rc, err = _io(lib, grid=None, surf=tight, W=100, out=out)
    assert rc == 1 and "null buffer (grid)" in err, err


def test_empty_batch_is_a_noop(lib):
    empty = _surf(y=None, u=None, v=None)
    for call in (_io, _curves):
        rc, err = call(lib, B=0, surf=empty, k=None, out=_out(out=None))
        assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"
        rc, err = call(lib, B=0, surf=empty, k=None, out=_out(**dict(PLANAR_OUT, out=None, out_u=None, out_v=None, k=None)))
        assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"
    rc, err = _to_rgb(lib, B=0, surf=empty, k=None, rgb=None)
    assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"
    rc, err = _lowres(lib, B=0, surf=empty, k=None, lowres=None)
    assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"


# ---- Python refusals on CPU tensors: raised before anything touches the device ------------------------------------------
def _u16(t):
    return t.to(torch.int16).view(torch.uint16)


def test_ops_refuse(lib):
    from hdrnet_amd import data, hdrnet_ops as ops
    grid = torch.zeros(1, 2, 2, 2, 12)
    guide = torch.zeros(1, 4, 8)
    y, u, v = (torch.zeros(s, dtype=torch.uint8) for s in ((1, 4, 8), (1, 2, 4), (1, 2, 4)))
    k = torch.zeros(12)
    with pytest.raises(ValueError, match="H must be even"):
        ops.yuv_planar_to_rgb(y[:, :3], u, v, k)
    with pytest.raises(ValueError, match="W % 4 != 0"):
        ops.yuv_planar_to_rgb(y[:, :, :6], u[:, :, :3], v[:, :, :3], k)
    with pytest.raises(ValueError, match=r"u should be \[B, H / 2, W / 2\]"):
        ops.yuv_planar_to_rgb(y, torch.zeros(1, 2, 8, dtype=torch.uint8), v, k)  # an interleaved UV plane is not a U plane
    with pytest.raises(ValueError, match=r"v should be \[B, H / 2, W / 2\]"):
        ops.yuv_planar_to_rgb(y, u, v[:, :1], k)
    with pytest.raises(TypeError, match="must all be uint8"):
        ops.yuv_planar_to_rgb(y, u, _u16(v), k)
    with pytest.raises(TypeError, match="must all be uint8"):
        ops.yuv_planar_to_rgb(y.float(), u.float(), v.float(), k)
    with pytest.raises(ValueError, match="last-dimension stride 1"):
        ops.yuv_planar_to_rgb(y, torch.zeros(1, 2, 8, dtype=torch.uint8)[:, :, ::2], v, k)
    with pytest.raises(ValueError, match="multiples of 2 bytes"):
        ops.yuv_planar_to_rgb(y, torch.zeros(1, 2, 5, dtype=torch.uint8)[:, :, :4], v, k)
    with pytest.raises(ValueError, match="12 floats"):
        ops.yuv_planar_to_rgb(y, u, v, torch.zeros(9))
    with pytest.raises(RuntimeError, match="no CPU path"):  # everything else in order: only the device is missing
        ops.yuv_planar_to_rgb(y, u, v, k)
    io = ops.bilateral_slice_apply_io_yuv_planar
    with pytest.raises(ValueError, match="unknown out 'nv12'"):  # planar in -> semi-planar out: out of scope
        io(grid, y, u, v, k, guide=guide, out="nv12")
    with pytest.raises(ValueError, match="needs from_rgb"):
        io(grid, y, u, v, k, guide=guide, out="planar")
    with pytest.raises(TypeError, match="a planar output has the input's dtype"):
        io(grid, y, u, v, k, guide=guide, out="planar", out_dtype=torch.uint16, from_rgb=k)
    with pytest.raises(ValueError, match="out_bits = 10 does not fit torch.uint8 planes"):
        io(grid, y, u, v, k, guide=guide, out="planar", from_rgb=k, out_bits=10)
    with pytest.raises(ValueError, match="out_bits = 8 does not fit torch.uint16 planes"):
        io(grid, _u16(y), _u16(u), _u16(v), k, guide=guide, out="planar", from_rgb=k, out_bits=8)
    with pytest.raises(TypeError, match="out_dtype must be float32 or uint8"):
        io(grid, y, u, v, k, guide=guide, out_dtype=torch.uint16)
    with pytest.raises(ValueError, match="belong to out='planar'"):
        io(grid, y, u, v, k, guide=guide, out_bits=8)
    with pytest.raises(ValueError, match="3 -> 3 op with offset"):
        io(torch.zeros(1, 2, 2, 2, 9), y, u, v, k, guide=guide)
    with pytest.raises(ValueError, match="exactly one of"):
        io(grid, y, u, v, k)
    with pytest.raises(ValueError, match="triple"):
        io(grid, y, u, v, k, guide=guide, out="planar", from_rgb=k, out_planes=(y, u))
    with pytest.raises(ValueError, match="out_planes should be a uint8 planar surface"):
        io(grid, y, u, v, k, guide=guide, out="planar", from_rgb=k,
           out_planes=tuple(torch.zeros(s, dtype=torch.uint8) for s in ((1, 8, 8), (1, 4, 4), (1, 4, 4))))
    with pytest.raises(ValueError, match="out_planes should be a uint8 planar surface"):
        io(grid, y, u, v, k, guide=guide, out="planar", from_rgb=k, out_planes=(_u16(y), _u16(u), _u16(v)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        io(grid, y, u, v, k, guide=guide, out="planar", from_rgb=k)
    with pytest.raises(ValueError, match="H must be even"):
        data.lowres_input_yuv_planar(y[:, :3], u, v, k, 4)
    with pytest.raises(RuntimeError, match="HIP"):
        data.lowres_input_yuv_planar(y, u, v, k, 4)


@pytest.mark.parametrize("cls", ["HDRNetCurves", "HDRNetPointwiseNNGuide"])
def test_process_yuv_planar_refuses(lib, cls):
    from hdrnet_amd import models
    torch.manual_seed(3)
    m = getattr(models, cls)(dict(batch_norm=False)).eval()
    y, u, v = (torch.zeros(s, dtype=torch.uint8) for s in ((1, 32, 48), (1, 16, 24), (1, 16, 24)))
    with pytest.raises(ValueError, match="unknown standard 'bt470'"):
        m.process_yuv_planar(y, u, v, standard="bt470")
    with pytest.raises(ValueError, match="unknown out 'nv12'"):
        m.process_yuv_planar(y, u, v, out="nv12")
    with pytest.raises(ValueError, match="does not fit torch.uint8 planes"):
        m.process_yuv_planar(y, u, v, bits=10)
    with pytest.raises(ValueError, match="does not fit torch.uint16 planes"):
        m.process_yuv_planar(_u16(y), _u16(u), _u16(v), bits=8)
    with pytest.raises(TypeError, match="must all be uint8"):
        m.process_yuv_planar(y, _u16(u), _u16(v))
    with pytest.raises(ValueError, match=r"u should be \[B, H / 2, W / 2\]"):
        m.process_yuv_planar(y, torch.zeros(1, 16, 48, dtype=torch.uint8), v)
    with pytest.raises(TypeError, match="a planar output has the input's dtype"):
        m.process_yuv_planar(y, u, v, out="planar", out_dtype=torch.uint16)
    with pytest.raises(ValueError, match="H must be even"):
        m.process_yuv_planar(y[:, :31], u, v)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.process_yuv_planar(y, u, v)


def test_pyramid_process_yuv_planar_refuses(lib):
    from hdrnet_amd import models
    torch.manual_seed(3)
    m = models.HDRNetGaussianPyrNN(dict(batch_norm=False)).eval()
    y, u, v = (torch.zeros(s, dtype=torch.uint8) for s in ((1, 32, 48), (1, 16, 24), (1, 16, 24)))
    with pytest.raises(ValueError, match="the pyramid model's resize and up-add kernels read RGB frames only"):
        m.process_yuv_planar(y, u, v)


# ---- the colour constants ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full_range", [False, True])
@pytest.mark.parametrize("standard", ["bt601", "bt709", "bt2020"])
def test_low_bit_coefficients(standard, full_range):
    """Codes in the low bits: for 10 bits the matrix is float32(64) x the default (P010) one, entry by entry, and the biases
    are equal -- scaling by a power of two commutes with the float64 division and the rounding to float32; 8 and 16 bits
    are unchanged by the flag, and the default call is what it was."""
    from hdrnet_amd import yuv
    for bits in (8, 10, 16):
        to_rgb, from_rgb = yuv.yuv_coefficients(standard, full_range, bits)
        named, from_named = yuv.yuv_coefficients(standard, full_range, bits, msb_aligned=True)
        assert to_rgb.tobytes() == named.tobytes() and from_rgb.tobytes() == from_named.tobytes()
        low, from_low = yuv.yuv_coefficients(standard, full_range, bits, msb_aligned=False)
        assert low.dtype == np.float32 and low.shape == (12,) and from_low.tobytes() == from_rgb.tobytes()
        if bits == 10:
            assert np.array_equal(low[:9], np.float32(64) * to_rgb[:9]) and np.array_equal(low[9:], to_rgb[9:])
            assert not np.array_equal(low[:9], to_rgb[:9])
        else:
            assert low.tobytes() == to_rgb.tobytes()
    # the default call's numbers, from the formula in the docstring, for one entry: 1 / (219 * 4 * 64) for limited 10 bit
    if not full_range:
        assert yuv.yuv_coefficients(standard, False, 10)[0][0] == np.float32(1.0 / (219.0 * 4.0 * 64.0))
        assert yuv.yuv_coefficients(standard, False, 10, msb_aligned=False)[0][0] == np.float32(1.0 / (219.0 * 4.0))


# ---- the helper's own statement of the rules ---------------------------------------------------------------------------
def test_helper():
    rng = np.random.default_rng(5)
    u = rng.integers(0, 255, (2, 3, 4)).astype(np.uint8)
    v = rng.integers(0, 255, (2, 3, 4)).astype(np.uint8)
    uv = pc.interleave(u, v)
    assert uv.shape == (2, 3, 8) and np.array_equal(uv[:, :, 0::2], u) and np.array_equal(uv[:, :, 1::2], v)
    u2, v2 = pc.split(uv)
    assert np.array_equal(u2, u) and np.array_equal(v2, v) and u2.flags.c_contiguous
    for bits in (8, 10, 16):
        shape = (2, 4, 100)
        (y, u, v), (ys, uvs) = pc.random_planar(np.random.default_rng([7, bits]), shape, bits)
        sh = yc.stored_shift(bits)
        assert y.shape == shape and u.shape == v.shape == (2, 2, 50) and y.dtype == ys.dtype
        assert int(y.max()) == 2 ** bits - 1 and int(y.min()) == 0  # the corners: extreme codes, in the LOW bits
        assert np.array_equal(y.astype(np.uint32) << sh, ys) and np.array_equal(pc.interleave(u, v).astype(np.uint32) << sh, uvs)
        for layout in pc.LAYOUTS:
            bufs, specs = pc.lay_planar(y, u, v, layout)
            assert len(bufs) == (1 if layout == "one_allocation" else 3)
            for spec, t in zip(specs, (y, u, v)):
                assert np.array_equal(pc.plane(bufs, spec), t)
                i, off, _, strides = spec
                size = y.itemsize
                unit = 4 if spec is specs[0] else 2 * size  # the header's alignment rules, in bytes
                assert (off * size) % unit == 0 and (strides[1] * size) % unit == 0 and (strides[0] * size) % unit == 0
            masks = pc.outside_planes(bufs, specs)
            assert sum(int((~m).sum()) for m in masks) == y.size + u.size + v.size  # the planes do not overlap
            for b, m in zip(bufs, masks):
                assert (b[m] == pc.fill_value(y.dtype, pc.POISON)).all() and m[-pc.GUARD_BYTES // y.itemsize:].all()
        if bits == 8:  # tight uint8 chroma rows of W = 100 start 2 bytes past a dword boundary
            _, specs = pc.lay_planar(y, u, v, "tight")
            assert specs[1][3][1] == 50 and specs[1][3][1] % 4 == 2
