"""YUV 4:2:2 / 4:4:4 surfaces without a GPU (include/hdrnet_amd_yuv_chroma.h): the eight entry points are exported and bound
as declared, refuse what the rules exclude with rc = 1 and a text that names the rule before any HIP call -- one case per
rule for each entry point: layout code, H and W, pitch / stride / alignment per layout, output kind against input width,
out_bits, NV24 -- B = 0 is a no-op, the Python layers refuse plane shapes that do not fit the NAMED chroma, the pyramid
model still refuses, and the numpy helpers of tests/yuv_chroma_cases.py say what their comments say."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import u16_out_cases as uc
import yuv_cases as yc
import yuv_chroma_cases as cc
import yuv_planar_cases as pc
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hdrnet_amd_yuv_chroma.h")
A = 0x1000  # a 16-byte aligned non-null "device pointer": never dereferenced, every row below is refused first
NAMES = sorted(["hdrnet_yuv_chroma_to_rgb_f32", "hdrnet_lowres_input_yuv_chroma", "hdrnet_bilateral_slice_apply_io_yuv_chroma",
                "hdrnet_bilateral_slice_apply_io_curves_yuv_chroma", "hdrnet_yuv_planar_chroma_to_rgb_f32",
                "hdrnet_lowres_input_yuv_planar_chroma", "hdrnet_bilateral_slice_apply_io_yuv_planar_chroma",
                "hdrnet_bilateral_slice_apply_io_curves_yuv_planar_chroma"])
C420, C422, C444 = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for name, (res, args) in _lib.YUV_CHROMA_SIGNATURES.items():
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
    assert sorted(decl) == sorted(_lib.YUV_CHROMA_SIGNATURES) == NAMES and len(NAMES) == 8
    for name, params in decl.items():
        res, args = _lib.YUV_CHROMA_SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for ctype, text in zip(args, params):  # pointer / long long / int / unsigned, position by position
            want = (ctypes.c_void_p if "*" in text else ctypes.c_longlong if text.startswith("long long ")
                    else ctypes.c_uint if text.startswith("unsigned") else ctypes.c_int)
            assert ctype is want, (name, text, ctype)
        assert "int chroma" in params and hasattr(lib, name)
    for other in (_lib.SIGNATURES, _lib.YUV_SIGNATURES, _lib.YUV_PLANAR_SIGNATURES, _lib.U16_OUT_SIGNATURES):
        assert not set(decl) & set(other)  # a header and a table of their own
    assert hasattr(_lib.load(), "hdrnet_yuv_planar_chroma_to_rgb_f32")  # ... and the package's handle binds them
    assert lib.hdrnet_version() >= 290
    text = open(HEADER).read()
    for name, code in _lib.CHROMA.items():
        assert re.search(r"#define HDRNET_CHROMA_%s %d\b" % (name, code), text), name
    for name, code in _lib.CHROMA_OUT.items():
        assert re.search(r"#define HDRNET_CHROMA_OUT_%s %d\b" % (name.upper(), code), text), name
    low = text.lower()
    assert "replicated" in low and "out of scope" in low
    for word in ("YUY2", "NV24", "12-bit", "bilinear chroma", "pyramid"):
        assert word in text.split("Out of scope")[-1], word
    # the three headers that called these layouts out of scope point here now
    for h in ("hdrnet_amd_yuv.h", "hdrnet_amd_yuv_planar.h", "hdrnet_amd_u16_out.h"):
        assert "hdrnet_amd_yuv_chroma.h" in open(os.path.join(ROOT, "include", h)).read(), h


# ---- the C ABI: surfaces of H = 3 (odd: no row pair), W = 8 ----------------------------------------------------------------
def _semi(y=A, uv=A, dt=1, py=8, puv=8, sy=24, suv=24):
    return [y, uv, dt, py, puv, sy, suv]


def _planar(chroma, y=A, u=A, v=A, dt=1, py=None, pu=None, pv=None, sy=None, su=None, sv=None):
    cw = (8 if chroma == C444 else 4) * dt
    py, pu, pv = 8 * dt if py is None else py, cw if pu is None else pu, cw if pv is None else pv
    return [y, u, v, dt, py, pu, pv, 3 * py if sy is None else sy, 3 * pu if su is None else su, 3 * pv if sv is None else sv]


def _semi_out(kind=1, out=A, out_uv=None, py=0, puv=0, sy=0, suv=0, k=None, bits=0):
    return [kind, out, out_uv, py, puv, sy, suv, k, bits]


def _planar_out(kind=1, out=A, out_u=None, out_v=None, py=0, pu=0, pv=0, sy=0, su=0, sv=0, k=None, bits=0):
    return [kind, out, out_u, out_v, py, pu, pv, sy, su, sv, k, bits]


NV16_OUT = dict(kind=2, out=A, out_uv=A, py=8, puv=8, sy=24, suv=24, k=A)
P216_OUT = dict(kind=3, out=A, out_uv=A, py=16, puv=16, sy=48, suv=48, k=A, bits=16)
U16_SEMI = dict(dt=2, py=16, puv=16, sy=48, suv=48)


def _call(lib, name, planar, chroma=C422, surf=None, B=1, H=3, W=8, k=A, grid=A, guide=A, GH=2, GW=2, GD=2, Cin=3, Cout=3, off=1,
          flags=0, npts=16, prepared=None, out=None, rgb=A, lowres=A, n=4):
    """One of the eight entry points by its role (``name``: "to_rgb", "lowres", "io", "curves")."""
    surf = surf if surf is not None else (_planar(chroma) if planar else _semi())
    infix = "yuv_planar_chroma" if planar else "yuv_chroma"
    head = [*surf, chroma, B, H, W, k]
    if name == "to_rgb":
        fn, args = f"hdrnet_{infix}_to_rgb_f32", [*head, rgb, None]
    elif name == "lowres":
        fn, args = f"hdrnet_lowres_input_{infix}", [*head, lowres, n, None]
    else:
        out = out if out is not None else (_planar_out() if planar else _semi_out())
        shape = [GH, GW, GD, Cin, Cout, off]
        if name == "io":
            fn, args = f"hdrnet_bilateral_slice_apply_io_{infix}", [grid, guide, *head, *shape, None, None, 0, None, flags, *out, None]
        else:
            fn, args = (f"hdrnet_bilateral_slice_apply_io_curves_{infix}",
                        [grid, *head, *shape, A, A, A, A, npts, prepared, None, *out, None])
    rc = getattr(lib, fn)(*args)
    return rc, lib.hdrnet_last_error().decode(), fn


ROLES = ["to_rgb", "lowres", "io", "curves"]
# rules of the input surface and the layout, the same for all four roles: (planar?, keywords, text)
SURFACE_REFUSALS = [
    # the layout code, and NV24
    (False, dict(chroma=3), "unknown chroma layout code"),
    (True, dict(chroma=-1), "unknown chroma layout code"),
    (False, dict(chroma=C444), "semi-planar 4:4:4 (NV24 / P410) is out of scope"),
    # H and W: any H for 4:2:2 / 4:4:4 (H = 3 passes everywhere below), W % 4 == 0 stays; 4:2:0 keeps H % 2 == 0
    (False, dict(W=6), "W % 4 != 0"),
    (True, dict(chroma=C444, W=10), "W % 4 != 0"),
    (False, dict(chroma=C420, H=3, surf=_semi()), "H % 2 != 0"),
    (True, dict(chroma=C420, H=3, surf=_planar(C420)), "H % 2 != 0"),
    # pitches
    (False, dict(surf=_semi(puv=4)), "below the row"),
    (True, dict(surf=_planar(C422, pu=2)), "below the row"),
    (True, dict(chroma=C444, surf=_planar(C444, pu=4)), "below the row"),  # a 4:4:4 chroma row is W samples
    (False, dict(surf=_semi(puv=10)), "pitches of the input surface must be multiples of 4"),
    (True, dict(surf=_planar(C422, pu=5)), "multiples of 4 (luma) and of 2 (uint8 chroma)"),
    (True, dict(surf=_planar(C422, dt=2, pv=10)), "multiples of 4 (luma) and of 4 (uint16 chroma)"),
    (True, dict(chroma=C444, surf=_planar(C444, pu=10)), "multiples of 4 (luma) and of 4 (4:4:4 chroma)"),
    # image strides: a chroma plane of these layouts has H rows
    (False, dict(surf=_semi(suv=22)), "image strides"),
    (True, dict(chroma=C444, surf=_planar(C444, su=26)), "image strides"),
    (False, dict(B=2, surf=_semi(suv=16)), "below its plane"),          # 16 = pitch * (H / 2 rounded up): 4:2:0's plane
    (True, dict(B=2, surf=_planar(C422, su=8)), "below its plane"),
    # pointers and alignment
    (False, dict(surf=_semi(uv=None)), "null plane"),
    (True, dict(surf=_planar(C422, v=None)), "null plane"),
    (False, dict(k=None), "null constants"),
    (False, dict(surf=_semi(uv=A + 2)), "planes and constants of the input surface must be 4-B aligned"),
    (True, dict(surf=_planar(C422, u=A + 1)), "chroma planes of the input surface must be 2-B aligned"),
    (True, dict(surf=_planar(C422, dt=2, v=A + 2)), "chroma planes of the input surface must be 4-B aligned"),
    (True, dict(chroma=C444, surf=_planar(C444, u=A + 2)), "must be 4-B aligned (4:4:4"),  # a 2-byte offset: refused
    (True, dict(surf=_planar(C422, dt=3)), "unknown sample dtype"),
]
PLANAR_OUT8 = dict(kind=2, out=A, out_u=A, out_v=A, py=8, pu=4, pv=4, sy=24, su=12, sv=12, k=A, bits=8)
PLANAR_OUT16 = dict(kind=3, out=A, out_u=A, out_v=A, py=16, pu=8, pv=8, sy=48, su=24, sv=24, k=A, bits=16)
IO_REFUSALS = SURFACE_REFUSALS + [
    (False, dict(out=_semi_out(kind=4)), "unknown output kind"),
    (True, dict(out=_planar_out(kind=-1)), "unknown output kind"),
    # output kind against input width
    (False, dict(out=_semi_out(**P216_OUT)), "P210 / P216 output needs a uint16 surface in"),
    (True, dict(out=_planar_out(**dict(PLANAR_OUT8, kind=3, bits=16))), "a planar surface output has the input's sample width"),
    (True, dict(surf=_planar(C422, dt=2), out=_planar_out(**dict(PLANAR_OUT16, kind=2, bits=8))),
     "a planar surface output has the input's sample width"),
    (True, dict(chroma=C420, H=4, surf=_planar(C420), out=_planar_out(**dict(PLANAR_OUT8, kind=3))),
     "a planar surface output has the input's sample width"),
    # out_bits
    (False, dict(surf=_semi(**U16_SEMI), out=_semi_out(**dict(P216_OUT, bits=12))), "out_bits must be 10 (P210) or 16 (P216)"),
    (True, dict(out=_planar_out(**dict(PLANAR_OUT8, bits=10))), "out_bits does not fit the sample dtype"),
    (True, dict(surf=_planar(C422, dt=2), out=_planar_out(**dict(PLANAR_OUT16, bits=12))), "out_bits does not fit the sample dtype"),
    # the output surface under the same rules
    (False, dict(out=_semi_out(**dict(NV16_OUT, puv=4))), "below the row"),
    (False, dict(B=2, out=_semi_out(**dict(NV16_OUT, suv=16))), "an image stride of the output surface is below its plane"),
    (True, dict(out=_planar_out(**dict(PLANAR_OUT8, out_v=A + 1))), "chroma planes of the output surface must be 2-B aligned"),
    (True, dict(chroma=C444, surf=_planar(C444), out=_planar_out(**dict(PLANAR_OUT8, pu=8, pv=8, su=24, sv=24, out_u=A + 2))),
     "chroma planes of the output surface must be 4-B aligned (4:4:4"),
    (True, dict(chroma=C444, surf=_planar(C444), out=_planar_out(**PLANAR_OUT8)), "below the row"),  # 4:2:2's pitches
    (False, dict(out=_semi_out(**dict(NV16_OUT, k=None))), "null constants of the output surface"),
    (False, dict(Cout=4), "Cin = Cout = 3 with offset"),
    (True, dict(out=_planar_out(out=None)), "null or misaligned out"),
    (False, dict(grid=None), "null buffer"),
]


@pytest.mark.parametrize("planar,kw,text", IO_REFUSALS)
@pytest.mark.parametrize("role", ["io", "curves"])
def test_fused_forward_refusals(lib, role, planar, kw, text):
    rc, err, fn = _call(lib, role, planar, **kw)
    assert rc == 1 and text in err, (rc, err)
    # with HDRNET_CHROMA_420 the entry point it forwards to answers, in its own name
    assert err.startswith(fn + ": ") or (kw.get("chroma") == C420 and err.startswith(fn.replace("_chroma", "")))


@pytest.mark.parametrize("planar,kw,text", SURFACE_REFUSALS)
@pytest.mark.parametrize("role", ["to_rgb", "lowres"])
def test_conversion_and_gather_refusals(lib, role, planar, kw, text):
    rc, err, fn = _call(lib, role, planar, **kw)
    assert rc == 1 and text in err, (rc, err)
    assert err.startswith(fn + ": ") or (kw.get("chroma") == C420 and err.startswith(fn.replace("_chroma", "")))


def test_other_refusals(lib):
    for planar in (False, True):
        assert "rgb must be" in _call(lib, "to_rgb", planar, rgb=None)[1]
        assert "negative image extent" in _call(lib, "to_rgb", planar, H=-1)[1]
        assert "lowres must be" in _call(lib, "lowres", planar, lowres=A + 4)[1]
        assert "non-positive extent" in _call(lib, "lowres", planar, n=0)[1]
        assert "either a guide map or the guide network" in _call(lib, "io", planar, guide=None)[1]
        assert "unknown flags" in _call(lib, "io", planar, flags=0x40000)[1]
        assert "curve knots" in _call(lib, "curves", planar, npts=0)[1]
        assert "prepared curves tables" in _call(lib, "curves", planar, prepared=A + 4)[1]


def test_tight_planes_pass_the_surface_rules(lib):
    """W = 100, uint8 4:2:2 planar: a tight chroma row is 50 bytes, so odd rows start 2 bytes past a dword boundary --
    admitted, with odd H; the call gets as far as the null grid.  4:4:4 tight planes of W = 100 and NV16 likewise."""
    tight = _planar(C422, u=A + 2, v=A + 6, py=100, pu=50, pv=50, sy=300, su=150, sv=150)
    out = _planar_out(kind=2, out=A, out_u=A + 2, out_v=A + 6, py=100, pu=50, pv=50, sy=300, su=150, sv=150, k=A, bits=8)
    for o in (None, out):
        rc, err, _ = _call(lib, "io", True, surf=tight, W=100, B=2, grid=None, out=o)
        assert rc == 1 and "null buffer (grid)" in err, err
    full = _planar(C444, py=100, pu=100, pv=100)
    rc, err, _ = _call(lib, "curves", True, chroma=C444, surf=full, W=100, B=2, grid=None)
    assert rc == 1 and "null buffer (grid" in err, err
    rc, err, _ = _call(lib, "io", False, surf=_semi(py=100, puv=100, sy=300, suv=300), W=100, B=2, grid=None,
                       out=_semi_out(**dict(NV16_OUT, py=100, puv=100, sy=300, suv=300)))
    assert rc == 1 and "null buffer (grid)" in err, err
    rc, err, _ = _call(lib, "io", False, surf=_semi(**U16_SEMI), grid=None, out=_semi_out(**dict(P216_OUT, bits=10)))
    assert rc == 1 and "null buffer (grid)" in err, err


def test_empty_batch_is_a_noop(lib):
    for planar in (False, True):
        for chroma in (C420, C422) + ((C444,) if planar else ()):
            H = 4 if chroma == C420 else 3
            surf = _planar(chroma, y=None, u=None, v=None) if planar else _semi(y=None, uv=None)
            out = _planar_out(out=None) if planar else _semi_out(out=None)
            for role in ROLES:
                rc, err, fn = _call(lib, role, planar, chroma=chroma, H=H, B=0, surf=surf, k=None, out=out, rgb=None, lowres=None)
                assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop", (fn, chroma, err)


# ---- the Python layers ---------------------------------------------------------------------------------------------------------
def _planes(shape, chroma, dtype=torch.uint8):
    cs = cc.chroma_shape(shape, chroma)
    return torch.zeros(shape, dtype=dtype), torch.zeros(cs, dtype=dtype), torch.zeros(cs, dtype=dtype)


def test_python_refuses_shapes_that_do_not_fit_the_named_chroma():
    from hdrnet_amd import data, hdrnet_ops as ops
    k = torch.zeros(12)
    grid = torch.zeros(1, 2, 2, 2, 12)
    shape = (1, 4, 8)
    y, u0, v0 = _planes(shape, "420")
    _, u2, v2 = _planes(shape, "422")
    _, u4, v4 = _planes(shape, "444")
    uv0, uv2 = torch.zeros(1, 2, 8, dtype=torch.uint8), torch.zeros(1, 4, 8, dtype=torch.uint8)
    planar_calls = [lambda *a, **kw: ops.yuv_planar_to_rgb(*a, k, **kw), lambda *a, **kw: data.lowres_input_yuv_planar(*a, k, **kw),
                    lambda *a, **kw: ops.bilateral_slice_apply_io_yuv_planar(grid, *a, k, guide=torch.zeros(shape), **kw)]
    for f in planar_calls:
        # the layout is named, never guessed: 4:2:0 planes under "422", 4:2:2 planes under "444" and under the default
        with pytest.raises(ValueError, match=r"chroma='422'.*should be \[B, H, W / 2\]"):
            f(y, u0, v0, chroma="422")
        with pytest.raises(ValueError, match=r"chroma='444'.*should be \[B, H, W\]"):
            f(y, u2, v2, chroma="444")
        with pytest.raises(ValueError, match=r"should be \[B, H / 2, W / 2\]"):
            f(y, u2, v2)
        with pytest.raises(ValueError, match=r"should be \[B, H / 2, W / 2\]"):
            f(y, u4, v4, chroma="420")
        with pytest.raises(ValueError, match="unknown chroma"):
            f(y, u2, v2, chroma="440")
        with pytest.raises(RuntimeError):  # the shapes fit: the call gets as far as asking for the device
            f(y, u2, v2, chroma="422")
        with pytest.raises(RuntimeError):
            f(y[:, :3], u4[:, :3], v4[:, :3], chroma="444") if f is not planar_calls[2] else f(y, u4, v4, chroma="444")
    semi_calls = [lambda *a, **kw: ops.yuv_to_rgb(*a, k, **kw), lambda *a, **kw: data.lowres_input_yuv(*a, k, **kw),
                  lambda *a, **kw: ops.bilateral_slice_apply_io_yuv(grid, *a, k, guide=torch.zeros(shape), **kw),
                  lambda *a, **kw: ops.bilateral_slice_apply_io_yuv_deep(grid, *a, k, guide=torch.zeros(shape), from_rgb=k,
                                                                         out_bits=16, **kw)]
    for f in semi_calls:
        with pytest.raises(ValueError, match=r"chroma='422'.*should be \[B, H, W\]"):
            f(y, uv0, chroma="422")
        with pytest.raises(ValueError, match=r"should be \[B, H / 2, W\]"):
            f(y, uv2)
        with pytest.raises(ValueError, match="semi-planar 4:4:4"):
            f(y, uv2, chroma="444")
    with pytest.raises(ValueError, match=r"chroma='422' takes 'rgb', 'nv16'"):
        ops.bilateral_slice_apply_io_yuv(grid, y, uv2, k, guide=torch.zeros(shape), out="nv12", chroma="422")
    with pytest.raises(ValueError, match="takes 'rgb', 'nv12'"):
        ops.bilateral_slice_apply_io_yuv(grid, y, uv0, k, guide=torch.zeros(shape), out="nv16")
    with pytest.raises(TypeError, match="P210 / P216 output needs a uint16 surface"):
        ops.bilateral_slice_apply_io_yuv_deep(grid, y, uv2, k, guide=torch.zeros(shape), from_rgb=k, out_bits=16, chroma="422")
    # W % 4 stays; H may be odd for the new layouts only
    yo, uo, vo = _planes((1, 3, 8), "422")
    with pytest.raises(RuntimeError):
        ops.yuv_planar_to_rgb(yo, uo, vo, k, chroma="422")
    with pytest.raises(ValueError, match="H must be even"):
        ops.yuv_planar_to_rgb(yo, uo[:, :1], vo[:, :1], k)
    with pytest.raises(ValueError, match="W % 4 != 0"):
        ops.yuv_planar_to_rgb(torch.zeros(1, 3, 6, dtype=torch.uint8), uo[:, :, :3], vo[:, :, :3], k, chroma="422")
    # a 4:4:4 chroma plane follows the luma's alignment: a row stride of 10 bytes is refused, a 4:2:2 one of 6 is not
    wide = torch.zeros(1, 3, 10, dtype=torch.uint8)
    with pytest.raises(ValueError, match="multiples of 4 bytes"):
        ops.yuv_planar_to_rgb(torch.zeros(1, 3, 8, dtype=torch.uint8), wide[:, :, :8], wide[:, :, :8], k, chroma="444")
    narrow = torch.zeros(1, 3, 6, dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.yuv_planar_to_rgb(torch.zeros(1, 3, 8, dtype=torch.uint8), narrow[:, :, :4], narrow[:, :, :4], k, chroma="422")


def test_models_and_the_pyramid():
    from hdrnet_amd import models
    torch.manual_seed(0)
    y, u2, v2 = _planes((1, 4, 8), "422")
    uv2 = torch.zeros(1, 4, 8, dtype=torch.uint8)
    m = models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).eval()
    with pytest.raises(ValueError, match=r"chroma='422' takes 'rgb', 'nv16', 'p210', 'p216'"):
        m.process_yuv(y, uv2, out="nv12", chroma="422")
    with pytest.raises(ValueError, match="takes 'rgb', 'nv12', 'p010', 'p016'"):
        m.process_yuv(y, uv2[:, :2], out="nv16")
    with pytest.raises(TypeError, match="needs a uint16 surface in .P210 / P216."):
        m.process_yuv(y, uv2, out="p210", chroma="422")
    with pytest.raises(ValueError, match="semi-planar 4:4:4"):
        m.process_yuv(y, uv2, chroma="444")
    with pytest.raises(ValueError, match=r"chroma='444'.*should be \[B, H, W\]"):
        m.process_yuv_planar(y, u2, v2, chroma="444")
    with pytest.raises(ValueError, match="unknown chroma"):
        m.process_yuv_planar(y, u2, v2, chroma=422)
    with pytest.raises(RuntimeError):  # as far as asking for the device
        m.process_yuv_planar(y, u2, v2, chroma="422", out="planar")
    pyr = models.HDRNetGaussianPyrNN(dict(batch_norm=False)).eval()
    for chroma in ("420", "422", "444"):
        with pytest.raises(ValueError, match="the pyramid model's resize and up-add kernels read RGB frames only"):
            pyr.process_yuv_planar(y, u2, v2, chroma=chroma)
    for chroma in ("420", "422"):
        with pytest.raises(ValueError, match="the pyramid model's resize and up-add kernels read RGB frames only"):
            pyr.process_yuv(y, uv2, chroma=chroma)


# ---- the numpy helpers check themselves ----------------------------------------------------------------------------------------
def test_helpers_shapes_and_layouts():
    shape = (2, 5, 12)
    assert cc.chroma_shape(shape, "422") == (2, 5, 6) and cc.chroma_shape(shape, "444") == shape
    rng = np.random.default_rng(3)
    for chroma in cc.CHROMAS:
        for bits in (8, 10, 16):
            y, u, v = cc.random_planar(rng, shape, bits, chroma)
            assert y.dtype == (np.uint8 if bits == 8 else np.uint16) and u.shape == v.shape == cc.chroma_shape(shape, chroma)
            assert int(max(y.max(), u.max(), v.max())) <= 2 ** bits - 1 and y[0, 0, 0] == 0 and y[0, 0, -1] == 2 ** bits - 1
            # independent chroma: neighbouring rows differ, and for 4:4:4 neighbouring samples of a pair
            assert not np.array_equal(u[:, 1], u[:, 2])
            if chroma == "444":
                assert not np.array_equal(u[:, :, 2::2], u[:, :, 3::2])
            for layout in cc.LAYOUTS:
                for fill in cc.FILLS:
                    bufs, specs = cc.lay((y, u, v), layout, fill)
                    for spec, t in zip(specs, (y, u, v)):
                        assert np.array_equal(pc.plane(bufs, spec), t)
                        assert all(s * y.itemsize % 4 == 0 for s in spec[3][:2]) or (chroma == "422" and t is not y)
                    masks = pc.outside_planes(bufs, specs)
                    assert sum(int(m.sum()) for m in masks) >= len(bufs) * cc.GUARD_BYTES // y.itemsize
                    assert all((b[m] == pc.fill_value(y.dtype, fill)).all() for b, m in zip(bufs, masks))
            sy, suv = cc.semi(y, u, v, bits) if chroma == "422" else (None, None)
            if chroma == "422":
                sh = 0 if bits == 8 else 16 - bits
                assert suv.shape == shape and np.array_equal(suv[:, :, 0::2] >> sh, u) and np.array_equal(sy >> sh, y)
    # tight uint8 4:2:2 chroma rows of W = 100 are 50 bytes
    _, specs = cc.plane_layout([(1, 3, 100), (1, 3, 50), (1, 3, 50)], 1, "tight")
    assert specs[1][3][1] == 50


def test_helpers_replication_and_conversion():
    rng = np.random.default_rng(5)
    shape = (1, 4, 8)
    (y, u, v), (ys, uvs) = pc.random_planar(rng, shape, 8)
    k = rng.standard_normal(12).astype(np.float32) * 0.01
    want = yc.to_rgb64(ys, uvs, k)
    for chroma in cc.CHROMAS:
        y2, u2, v2 = cc.from_420(y, u, v, chroma)
        assert u2.shape == cc.chroma_shape(shape, chroma)
        assert np.array_equal(cc.replicate(u2, chroma), cc.replicate(u, "420"))
        assert np.array_equal(cc.to_rgb64(y2, u2, v2, chroma, k), want)
    # one pixel by hand: 4:4:4 reads (y, x), 4:2:2 reads (y, x >> 1)
    y4, u4, v4 = cc.random_planar(rng, shape, 8, "444", corners=False)
    kk = np.asarray(k, np.float64)
    px = np.clip(kk[0] * y4[0, 3, 5] + kk[1] * u4[0, 3, 5] + kk[2] * v4[0, 3, 5] + kk[9], 0, 1)
    assert cc.to_rgb64(y4, u4, v4, "444", k)[0, 3, 5, 0] == px
    y2, u2, v2 = cc.random_planar(rng, shape, 8, "422", corners=False)
    px = np.clip(kk[0] * y2[0, 3, 5] + kk[1] * u2[0, 3, 2] + kk[2] * v2[0, 3, 2] + kk[9], 0, 1)
    assert cc.to_rgb64(y2, u2, v2, "422", k)[0, 3, 5, 0] == px


def test_helpers_float64_encoder():
    from hdrnet_amd import yuv
    rng = np.random.default_rng(7)
    rgb = rng.random((2, 4, 8, 3)).astype(np.float32) * 1.2 - 0.1  # both clips
    for bits in (8, 10, 16):
        k = yuv.yuv_encode_coefficients("bt709", False, bits)
        # 4:2:0: the existing encoders with the UV plane split
        (y0, u0, v0), pre0 = cc.encode64(rgb, k, bits, "420")
        if bits == 8:
            wy, wuv, wy_pre, wuv_pre = yc.encode_nv12_64(rgb, k)
        else:
            wy, wuv, wy_pre, wuv_pre = uc.encode_p016_64(rgb, k, bits)
        sh = 0 if bits == 8 else 16 - bits
        assert np.array_equal(y0, wy >> sh) and np.array_equal(u0, wuv[:, :, 0::2] >> sh) and np.array_equal(v0, wuv[:, :, 1::2] >> sh)
        assert np.array_equal(pre0[0], wy_pre) and np.allclose(pre0[2], wuv_pre[:, :, 1::2], rtol=0, atol=1e-9)
        # 4:2:2 and 4:4:4 footprints, by hand on one sample each; luma is per pixel whatever the layout
        c = np.clip(rgb.astype(np.float64), 0, 1)
        kk = np.asarray(k, np.float64)
        (y2, u2, v2), pre2 = cc.encode64(rgb, k, bits, "422")
        (y4, u4, v4), pre4 = cc.encode64(rgb, k, bits, "444")
        assert np.array_equal(y2, y0) and np.array_equal(y4, y0)
        assert u2.shape == (2, 4, 4) and u4.shape == (2, 4, 8)
        pair = 0.5 * (c[1, 3, 4] + c[1, 3, 5])
        assert abs(pre2[1][1, 3, 2] - (pair @ kk[3:6] + kk[10])) < 1e-9 and abs(pre2[2][1, 3, 2] - (pair @ kk[6:9] + kk[11])) < 1e-9
        assert abs(pre4[1][1, 3, 5] - (c[1, 3, 5] @ kk[3:6] + kk[10])) < 1e-9
        assert u4[1, 3, 5] == int(np.floor(np.clip(pre4[1][1, 3, 5], 0, 2 ** bits - 1)))
        # a 4:4:4 surface of a frame whose pixels repeat 2 x 2 encodes to the replicated 4:2:0 codes
        flat = rgb[:, ::2, ::2].repeat(2, axis=1).repeat(2, axis=2)
        (_, uf, _), _ = cc.encode64(flat, k, bits, "444")
        (_, ub, _), _ = cc.encode64(flat, k, bits, "420")
        assert np.array_equal(uf, cc.replicate(ub, "420"))


def test_undecided_share_of_random_colours():
    """With colours drawn over the whole range the share of samples within eps of a code boundary is about 2 eps per code
    -- 0.2 % at 8 bits, 0.8 % at 10 -- and below 1 % of a case of some 10^4 samples: the condition of the GPU tests."""
    from hdrnet_amd import yuv
    rng = np.random.default_rng(11)
    rgb = rng.random((2, 5, 1040, 3)).astype(np.float32)
    for bits, expect in ((8, 2e-3), (10, 8e-3)):
        k = yuv.yuv_encode_coefficients("bt709", False, bits)
        for chroma in cc.CHROMAS:
            _, pre = cc.encode64(rgb, k, bits, chroma)
            und = sum(int((~cc.decided(p, bits)).sum()) for p in pre)
            total = sum(p.size for p in pre)
            assert 0.5 * expect < und / total < 0.01, (bits, chroma, und / total)
    assert uc.eps_of(8) == 1e-3 and uc.eps_of(10) == 4e-3
