"""The pyramid model on YUV 4:2:0 surfaces without a GPU (include/hdrnet_amd_pyramid_yuv.h): the five entry points are
exported and bound as declared, refuse what they cannot run with rc = 1 and a text before any HIP call, the model's
process_wire_yuv / process_wire_yuv_planar refuse on CPU tensors before asking for the device, and the caps that
tests/test_gpu_pyramid_yuv.py applies hold for the reference alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import pyramid_io_cases as pio
import pyramid_yuv_cases as pyc
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hdrnet_amd_pyramid_yuv.h")
A = 0x1000  # a 16-byte aligned non-null "device pointer": never dereferenced, every row below is refused first
NAMES = ["hdrnet_bilateral_slice_apply_upadd_io_yuv", "hdrnet_bilateral_slice_apply_upadd_io_yuv_p016",
         "hdrnet_bilateral_slice_apply_upadd_io_yuv_planar", "hdrnet_resize_bilinear_yuv", "hdrnet_resize_bilinear_yuv_planar"]


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for name, (res, args) in _lib.PYRAMID_YUV_SIGNATURES.items():
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


# ---- 1. bindings ---------------------------------------------------------------------------------------------------------
def test_symbols_exported_and_bound_as_declared(lib):
    from hdrnet_amd import _lib
    decl = _declared()
    assert sorted(decl) == sorted(_lib.PYRAMID_YUV_SIGNATURES) == NAMES
    for name, params in decl.items():
        res, args = _lib.PYRAMID_YUV_SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for ctype, text in zip(args, params):  # pointer / long long / unsigned / int, position by position
            want = (ctypes.c_void_p if "*" in text else ctypes.c_longlong if text.startswith("long long")
                    else ctypes.c_uint if text.startswith("unsigned") else ctypes.c_int)
            assert ctype is want, (name, text, ctype)
        assert hasattr(lib, name)
    assert not set(decl) & set(_lib.SIGNATURES)  # a header of their own: the first table still mirrors hdrnet_amd.h
    assert hasattr(_lib.load(), "hdrnet_resize_bilinear_yuv")  # ... and the package's handle binds them
    assert lib.hdrnet_version() >= 291
    # the siblings' argument lists with (coarse, Hc, Wc) added and guide_out dropped
    for name, sibling, table in (("hdrnet_bilateral_slice_apply_upadd_io_yuv", "hdrnet_bilateral_slice_apply_io_yuv", _lib.YUV_SIGNATURES),
                                 ("hdrnet_bilateral_slice_apply_upadd_io_yuv_p016", "hdrnet_bilateral_slice_apply_io_yuv_p016", _lib.U16_OUT_SIGNATURES),
                                 ("hdrnet_bilateral_slice_apply_upadd_io_yuv_planar", "hdrnet_bilateral_slice_apply_io_yuv_planar",
                                  _lib.YUV_PLANAR_SIGNATURES)):
        assert len(_lib.PYRAMID_YUV_SIGNATURES[name][1]) == len(table[sibling][1]) + 3 - 1
        assert "guide_out" not in " ".join(decl[name]) and "const float* coarse" in decl[name]


# ---- 2. validation without a GPU -------------------------------------------------------------------------------------------
# keyword defaults of one valid call per entry point (H = 4, W = 8, uint8 samples unless the entry point needs uint16)
def _semi(dt=1, W=8):
    return dict(y=A, uv=A, dt=dt, py=W * dt, puv=W * dt, sy=0, suv=0, B=1, H=4, W=W)


def _planar(dt=1, W=8):
    return dict(y=A, u=A, v=A, dt=dt, py=W * dt, pu=W * dt // 2, pv=W * dt // 2, sy=0, su=0, sv=0, B=1, H=4, W=W)


def _call(lib, name, **kw):
    if name == "hdrnet_resize_bilinear_yuv":
        d = dict(_semi(), k=A, out=A, Hout=2, Wout=4)
        d.update(kw)
        args = (d["y"], d["uv"], d["dt"], d["py"], d["puv"], d["sy"], d["suv"], d["B"], d["H"], d["W"], d["k"], d["out"],
                d["Hout"], d["Wout"], None)
    elif name == "hdrnet_resize_bilinear_yuv_planar":
        d = dict(_planar(), k=A, out=A, Hout=2, Wout=4)
        d.update(kw)
        args = (d["y"], d["u"], d["v"], d["dt"], d["py"], d["pu"], d["pv"], d["sy"], d["su"], d["sv"], d["B"], d["H"], d["W"],
                d["k"], d["out"], d["Hout"], d["Wout"], None)
    else:
        guide = dict(grid=A, guide=A, k=A, coarse=A, Hc=2, Wc=4, GH=2, GW=2, GD=2, Cin=3, Cout=3, off=1, c1=None, c2=None, n=0,
                     flags=0, kind=0, out=A, from_rgb=A, bits=10)
        if name == "hdrnet_bilateral_slice_apply_upadd_io_yuv":
            d = dict(_semi(), **guide, ouv=A, opy=8, opuv=8)
            d.update(kw)
            tail = (d["kind"], d["out"], d["ouv"], d["opy"], d["opuv"], 0, 0, d["from_rgb"])
            surf = (d["y"], d["uv"], d["dt"], d["py"], d["puv"], d["sy"], d["suv"])
        elif name == "hdrnet_bilateral_slice_apply_upadd_io_yuv_p016":
            d = dict(_semi(dt=2), **guide, ouv=A, opy=16, opuv=16)
            d.update(kw)
            tail = (d["out"], d["ouv"], d["opy"], d["opuv"], 0, 0, d["from_rgb"], d["bits"])
            surf = (d["y"], d["uv"], d["dt"], d["py"], d["puv"], d["sy"], d["suv"])
        else:
            d = dict(_planar(), **guide, ou=A, ov=A, opy=8, opu=4, opv=4)
            d["bits"] = 8
            d.update(kw)
            tail = (d["kind"], d["out"], d["ou"], d["ov"], d["opy"], d["opu"], d["opv"], 0, 0, 0, d["from_rgb"], d["bits"])
            surf = (d["y"], d["u"], d["v"], d["dt"], d["py"], d["pu"], d["pv"], d["sy"], d["su"], d["sv"])
        args = (d["grid"], d["guide"], *surf, d["B"], d["H"], d["W"], d["k"], d["coarse"], d["Hc"], d["Wc"], d["GH"], d["GW"],
                d["GD"], d["Cin"], d["Cout"], d["off"], d["c1"], d["c2"], d["n"], d["flags"], *tail, None)
    rc = getattr(lib, name)(*args)
    return rc, lib.hdrnet_last_error().decode()


COMMON = [  # refused by every entry point
    (dict(y=None), "null plane"),
    (dict(k=None), "null constants"),
    (dict(out=None), "out"),
    (dict(W=6), "W % 4 != 0"),
    (dict(H=3), "H % 2 != 0"),
    (dict(py=4), "pitch"),
    (dict(y=A + 2), "aligned"),
    (dict(dt=3), "unknown sample dtype"),
]
UPADD = [  # ... and by the three up-add entry points
    (dict(grid=None), "null buffer (grid)"),
    (dict(coarse=None), "coarse must be a 4-B aligned buffer"),
    (dict(coarse=A + 2), "coarse must be a 4-B aligned buffer"),
    (dict(Hc=0), "bad coarse extents"),
    (dict(Wc=-1), "bad coarse extents"),
    (dict(flags=0x40000), "unknown flags"),   # no curves (or any other) flag exists: two guide flags, nothing else
    (dict(flags=0x1), "unknown flags"),
    (dict(guide=None), "either a guide map or the guide network"),
    (dict(c1=A, c2=A, n=16), "either a guide map or the guide network"),
    (dict(Cin=4, Cout=4), "Cin = Cout = 3 with offset"),
    (dict(off=0), "Cin = Cout = 3 with offset"),
]
ROWS = [(name, kw, text) for name in NAMES for kw, text in COMMON]
ROWS += [(name, kw, text) for name in NAMES[:3] for kw, text in UPADD]
ROWS += [
    ("hdrnet_resize_bilinear_yuv", dict(uv=None), "null plane"),
    ("hdrnet_resize_bilinear_yuv", dict(Hout=-1), "negative output extent"),
    ("hdrnet_resize_bilinear_yuv", dict(H=0, W=0, py=0, puv=0), "empty surface"),
    ("hdrnet_resize_bilinear_yuv_planar", dict(v=None), "null plane"),
    ("hdrnet_resize_bilinear_yuv_planar", dict(Wout=-2), "negative output extent"),
    ("hdrnet_resize_bilinear_yuv_planar", dict(u=A + 1), "chroma planes"),
    ("hdrnet_bilateral_slice_apply_upadd_io_yuv", dict(kind=3), "unknown output kind"),
    ("hdrnet_bilateral_slice_apply_upadd_io_yuv", dict(kind=-1), "unknown output kind"),
    ("hdrnet_bilateral_slice_apply_upadd_io_yuv", dict(kind=2, opy=4), "pitch"),
    ("hdrnet_bilateral_slice_apply_upadd_io_yuv", dict(kind=2, ouv=None), "null plane of the output"),
    ("hdrnet_bilateral_slice_apply_upadd_io_yuv", dict(kind=2, from_rgb=None), "null constants of the output"),
    ("hdrnet_bilateral_slice_apply_upadd_io_yuv_p016", dict(bits=8), "out_bits must be 10"),
    ("hdrnet_bilateral_slice_apply_upadd_io_yuv_p016", dict(bits=12), "out_bits must be 10"),
    ("hdrnet_bilateral_slice_apply_upadd_io_yuv_p016", dict(dt=1), "needs a uint16 surface in"),
    ("hdrnet_bilateral_slice_apply_upadd_io_yuv_p016", dict(ouv=A + 2), "aligned"),
    ("hdrnet_bilateral_slice_apply_upadd_io_yuv_planar", dict(kind=3), "unknown output kind"),
    ("hdrnet_bilateral_slice_apply_upadd_io_yuv_planar", dict(kind=2, bits=10), "out_bits does not fit"),
    ("hdrnet_bilateral_slice_apply_upadd_io_yuv_planar", dict(kind=2, dt=2, py=16, pu=8, pv=8, opy=16, opu=8, opv=8, bits=12),
     "out_bits does not fit"),
    ("hdrnet_bilateral_slice_apply_upadd_io_yuv_planar", dict(kind=2, ou=A + 1), "chroma planes"),
]


@pytest.mark.parametrize("name,kw,text", ROWS, ids=["%s-%s" % (n.replace("hdrnet_", ""), "-".join("%s=%s" % i for i in kw.items()))
                                                    for n, kw, _ in ROWS])
def test_refusals(lib, name, kw, text):
    rc, err = _call(lib, name, **kw)
    assert rc == 1 and text in err, (rc, err)


@pytest.mark.parametrize("name", NAMES)
def test_valid_defaults_pass_validation_and_empty_is_a_noop(lib, name):
    """B * H * W == 0 (the resize: an empty output) returns 0 with no pointer looked at; so the rows above are refused for
    the rule each names, not for the defaults around it."""
    kw = dict(Hout=0, out=None, y=None) if "resize" in name else dict(B=0, y=None, out=None, grid=None, coarse=None)
    rc, err = _call(lib, name, **kw)
    assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"


# ---- 3. the model refuses on CPU tensors, before asking for the device ------------------------------------------------------
def test_process_wire_yuv_refuses():
    from hdrnet_amd import models
    torch.manual_seed(3)
    m = models.HDRNetGaussianPyrNN(dict(batch_norm=False))
    y, uv = torch.zeros(1, 32, 48, dtype=torch.uint8), torch.zeros(1, 16, 48, dtype=torch.uint8)
    u = v = torch.zeros(1, 16, 24, dtype=torch.uint8)
    m.train()
    with pytest.raises(RuntimeError, match="inference"):
        m.process_wire_yuv(y, uv)
    with pytest.raises(RuntimeError, match="inference"):
        m.process_wire_yuv_planar(y, u, v)
    m.eval()
    with pytest.raises(ValueError, match="W % 16 == 0"):
        m.process_wire_yuv(torch.zeros(1, 32, 40, dtype=torch.uint8), torch.zeros(1, 16, 40, dtype=torch.uint8))
    with pytest.raises(ValueError, match="W % 16 == 0"):
        m.process_wire_yuv_planar(torch.zeros(1, 32, 40, dtype=torch.uint8), *(torch.zeros(1, 16, 20, dtype=torch.uint8),) * 2)
    with pytest.raises(ValueError, match="4:2:0 surfaces only"):
        m.process_wire_yuv(y, torch.zeros(1, 32, 48, dtype=torch.uint8), chroma="422")
    with pytest.raises(ValueError, match="4:2:0 surfaces only"):
        m.process_wire_yuv_planar(y, u, v, chroma="422")
    with pytest.raises(ValueError, match="unknown out"):
        m.process_wire_yuv(y, uv, out="planar")
    with pytest.raises(ValueError, match="unknown out"):
        m.process_wire_yuv_planar(y, u, v, out="nv12")
    with pytest.raises(TypeError, match="needs a uint16 surface in"):
        m.process_wire_yuv(y, uv, out="p010")
    with pytest.raises(ValueError, match="bits"):
        m.process_wire_yuv(y, uv, bits=10)
    with pytest.raises(RuntimeError, match="no CPU path"):  # every rule passed: now the device is required
        m.process_wire_yuv(y, uv, out="nv12")
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.process_wire_yuv_planar(y, u, v, out="planar")
    # process_yuv / process_yuv_planar keep refusing the pyramid model, in their words
    with pytest.raises(ValueError, match="resize and up-add kernels read RGB frames only: there is no YUV surface path"):
        m.process_yuv(y, uv)
    with pytest.raises(ValueError, match="resize and up-add kernels read RGB frames only: there is no YUV surface path"):
        m.process_yuv_planar(y, u, v)
    assert not hasattr(models.HDRNetPointwiseNNGuide, "process_wire_yuv")  # the single-level models' process_yuv takes surfaces


def test_runtime_dispatches_to_process_wire_yuv():
    from hdrnet_amd import models
    from hdrnet_amd.runtime import _ProcessYuv, _ProcessYuvPlanar
    torch.manual_seed(3)
    y = torch.zeros(1, 32, 48, dtype=torch.uint8)
    calls = []
    pyr = models.HDRNetGaussianPyrNN(dict(batch_norm=False)).eval()
    pyr.process_wire_yuv = lambda *a, **k: calls.append(("wire", sorted(k)))
    pyr.process_wire_yuv_planar = lambda *a, **k: calls.append(("wire planar", sorted(k)))
    one = models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).eval()
    one.process_yuv = lambda *a, **k: calls.append(("yuv", sorted(k)))
    one.process_yuv_planar = lambda *a, **k: calls.append(("planar", sorted(k)))
    for m in (pyr, one):
        _ProcessYuv(m, "bt709", False, None, "nv12", None)(y, y)
        _ProcessYuvPlanar(m, "bt709", False, None, "planar", None)(y, y, y)
    keys = ["bits", "full_range", "out", "out_dtype", "standard"]
    assert calls == [("wire", keys), ("wire planar", keys), ("yuv", keys), ("planar", keys)]


def test_ops_wrappers_refuse():
    from hdrnet_amd import hdrnet_ops as ops
    grid, coarse, k = torch.zeros(1, 2, 2, 2, 12), torch.zeros(1, 2, 4, 3), torch.zeros(12)
    y, uv = torch.zeros(1, 4, 8, dtype=torch.uint8), torch.zeros(1, 2, 8, dtype=torch.uint8)
    u = v = torch.zeros(1, 2, 4, dtype=torch.uint8)
    guide, c1, c2 = torch.zeros(1, 4, 8), torch.zeros(16, 4), torch.zeros(17)
    for call in (lambda: ops.resize_bilinear_yuv(y, uv, k, 2, 4), lambda: ops.resize_bilinear_yuv_planar(y, u, v, k, 2, 4),
                 lambda: ops.bilateral_slice_apply_upadd_io_yuv(grid, y, uv, k, coarse, guide=guide),
                 lambda: ops.bilateral_slice_apply_upadd_io_yuv_planar(grid, y, u, v, k, coarse, guide_conv1=c1, guide_conv2=c2)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    with pytest.raises(ValueError, match="bad output extents"):
        ops.resize_bilinear_yuv(y, uv, k, -1, 4)
    with pytest.raises(ValueError, match="H must be even"):
        ops.resize_bilinear_yuv(torch.zeros(1, 3, 8, dtype=torch.uint8), uv, k, 2, 4)
    with pytest.raises(ValueError, match="curves guide"):
        ops.bilateral_slice_apply_upadd_io_yuv(grid, y, uv, k, coarse, guide_curves=(c1, c1, c1, c2))
    with pytest.raises(ValueError, match="curves guide"):
        ops.bilateral_slice_apply_upadd_io_yuv_planar(grid, y, u, v, k, coarse, guide_curves=(c1, c1, c1, c2))
    with pytest.raises(ValueError, match="coarse should be"):
        ops.bilateral_slice_apply_upadd_io_yuv(grid, y, uv, k, torch.zeros(1, 2, 4, 4), guide=guide)
    with pytest.raises(ValueError, match="coarse should be"):
        ops.bilateral_slice_apply_upadd_io_yuv_planar(grid, y, u, v, k, torch.zeros(2, 2, 4, 3), guide=guide)
    with pytest.raises(ValueError, match="unknown out"):
        ops.bilateral_slice_apply_upadd_io_yuv(grid, y, uv, k, coarse, guide=guide, out="planar")
    with pytest.raises(TypeError, match="uint16 surface in"):
        ops.bilateral_slice_apply_upadd_io_yuv(grid, y, uv, k, coarse, guide=guide, out="p010", from_rgb=k)
    with pytest.raises(ValueError, match="exactly one of"):
        ops.bilateral_slice_apply_upadd_io_yuv(grid, y, uv, k, coarse)
    with pytest.raises(ValueError, match="exactly one of"):
        ops.bilateral_slice_apply_upadd_io_yuv_planar(grid, y, u, v, k, coarse, guide=guide, guide_conv1=c1, guide_conv2=c2)


# ---- 4. the caps of the GPU tests, from the reference alone --------------------------------------------------------------
@pytest.mark.parametrize("nn", [False, True], ids=["map", "nnguide"])
@pytest.mark.parametrize("kind", list(pyc.KINDS))
def test_caps_hold_for_the_reference_alone(kind, nn):
    """tests/test_gpu_pyramid_yuv.py lets a surface sample differ by one code where float64 leaves it open (closer than
    eps_of(bits) to a code boundary) and lets fewer than 5e-4 of the uint8 samples differ from the quantised float32
    reference.  Both are caps, not measurements: for every case of that file the expected frame built on the CPU --
    to_rgb64(...).astype(f32) -> port.bilateral_slice_apply with the case's guide map -> + the up-sampled coarse level --
    leaves fewer than 1 % of the surface samples of its kind open (counted over the shapes, as test_nv12_output counts: a
    10-bit code leaves 2 * eps_of(10) = 0.8 % of the unclamped samples open by construction, which 600 samples of the
    smallest shape cannot resolve), and against the float64 evaluation of the same formulas its uint8 image differs on fewer
    than 5e-4 of the samples and reaches 0 and 255 in every case."""
    left_open = total = 0
    for shape in pyc.SHAPES:
        c = pyc.inputs(shape, kind, nn)
        w32 = pyc.want_f32(shape, kind, nn)
        assert w32.min() < -0.05 and w32.max() > 1.05  # the sum leaves [0, 1] on both sides
        _, _, decided, bits = pyc.encode(w32, kind)
        left_open += sum(int((~d).sum()) for d in decided)
        total += sum(d.size for d in decided)
        w64 = pio.slice_apply_upadd_f64(c, shape)
        assert np.abs(w32 - w64).max() < 1e-5, (shape, kind, nn, np.abs(w32 - w64).max())  # the same function
        q32, q64 = pio.quantise(w32), pio.quantise(w64)
        share = float((q32 != q64).mean())
        print(f"{shape} {kind} nn={nn}: uint8 share {share:.2e} (cap 5e-4)")
        assert share < 5e-4, (shape, kind, nn, share)
        assert np.abs(q32.astype(np.int16) - q64.astype(np.int16)).max() <= 1
        assert q32.min() == 0 and q32.max() == 255, (shape, kind, nn)
    print(f"{kind} nn={nn}: {left_open} of {total} surface samples left open = {left_open / total:.2e} (cap 1e-2)")
    assert left_open < 0.01 * total, (kind, nn, left_open, total)
