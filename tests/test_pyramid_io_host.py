"""The pyramid model's wire formats without a GPU (include/hdrnet_amd_pyramid_io.h): the two entry points are exported and
bound as declared, refuse what they cannot run with rc = 1 and a text before any HIP call, and the Python layers above
them (hdrnet_ops.resize_bilinear_io / bilateral_slice_apply_upadd_io, HDRNetGaussianPyrNN.process_wire) raise the
exception types of their siblings."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "hdrnet_amd_pyramid_io.h")
I, P, F, U = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint
A = 0x1000  # a 16-byte aligned non-null "device pointer": never dereferenced, every row below is refused first


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for name, (res, args) in _lib.PYRAMID_IO_SIGNATURES.items():
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
    assert sorted(decl) == sorted(_lib.PYRAMID_IO_SIGNATURES) == ["hdrnet_bilateral_slice_apply_upadd_io_ex",
                                                                  "hdrnet_resize_bilinear_io"]
    for name, params in decl.items():
        res, args = _lib.PYRAMID_IO_SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params), (name, len(args), len(params))
        for ctype, text in zip(args, params):  # pointer / int / float / unsigned, position by position
            want = (ctypes.c_void_p if "*" in text else ctypes.c_float if text.startswith("float ")
                    else ctypes.c_uint if text.startswith("unsigned") else ctypes.c_int)
            assert ctype is want, (name, text, ctype)
        assert hasattr(lib, name)
    assert not set(decl) & set(_lib.SIGNATURES)  # a header of their own: the first table still mirrors hdrnet_amd.h
    assert hasattr(_lib.load(), "hdrnet_resize_bilinear_io")  # ... and the package's handle binds them
    assert lib.hdrnet_version() >= 285


def _resize(lib, inp=A, dtype=1, wl=255.0, out=A, B=1, Hin=4, Win=4, Hout=2, Wout=2, C=3):
    rc = lib.hdrnet_resize_bilinear_io(inp, dtype, wl, out, B, Hin, Win, Hout, Wout, C, None)
    return rc, lib.hdrnet_last_error().decode()


@pytest.mark.parametrize("kw,text", [
    (dict(inp=None), "null buffer"),
    (dict(out=None), "null buffer"),
    (dict(Hin=0), "bad extents"),
    (dict(Win=-1), "bad extents"),
    (dict(Hout=-1), "bad extents"),
    (dict(B=-1), "bad extents"),
    (dict(C=4), "C must be 3"),
    (dict(C=1), "C must be 3"),
    (dict(dtype=3), "unknown dtype code"),
    (dict(dtype=-1), "unknown dtype code"),
    (dict(wl=0.0), "white_level must be positive"),
    (dict(inp=A + 1), "4-B aligned"),
    (dict(inp=A + 2, dtype=2), "4-B aligned"),
    (dict(out=A + 2), "4-B aligned"),
])
def test_resize_refusals(lib, kw, text):
    rc, err = _resize(lib, **kw)
    assert rc == 1 and err.startswith("hdrnet_resize_bilinear_io: ") and text in err, (rc, err)


def test_resize_empty_output_is_a_noop(lib):
    rc, err = _resize(lib, inp=None, out=None, Hout=0)
    assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"


def _upadd(lib, grid=A, guide=A, inp=A, coarse=A, Hc=2, Wc=2, out=A, B=1, H=4, W=4, GH=2, GW=2, GD=2, Cin=3, Cout=3,
           off=1, idt=1, wl=255.0, odt=1, c1=None, c2=None, n=0, flags=0):
    rc = lib.hdrnet_bilateral_slice_apply_upadd_io_ex(grid, guide, inp, coarse, Hc, Wc, out, B, H, W, GH, GW, GD, Cin, Cout,
                                                      off, idt, wl, odt, c1, c2, n, flags, None)
    return rc, lib.hdrnet_last_error().decode()


@pytest.mark.parametrize("kw,text", [
    (dict(GH=0), "grid extents must be positive"),
    (dict(H=-1), "negative image extent"),
    (dict(flags=0x40000), "unknown flags"),
    (dict(Cin=0), "bad channel counts"),
    (dict(idt=3), "unknown dtype code"),
    (dict(odt=2), "unknown dtype code"),
    (dict(wl=0.0), "input_white_level must be positive"),
    (dict(Hc=0), "bad coarse extents"),
    (dict(Wc=-2), "bad coarse extents"),
    (dict(guide=None), "either a guide map or the guide network"),            # neither
    (dict(c1=A, c2=A, n=16), "either a guide map or the guide network"),      # both
    (dict(guide=None, c1=A, c2=None, n=16), "guide network needs conv1, conv2"),
    (dict(guide=None, c1=A, c2=A, n=0), "guide network needs conv1, conv2"),
    (dict(grid=None), "null buffer"),
    (dict(inp=None), "null buffer"),
    (dict(out=None), "null buffer"),
    (dict(coarse=None), "null buffer"),
    (dict(flags=0x20000), "HDRNET_GUIDE_RELU_PRESCALED"),                     # a guide MAP: nothing to prescale
    (dict(Cin=4, Cout=4), "Cin = Cout = 3 with offset"),
    (dict(off=0), "Cin = Cout = 3 with offset"),
    (dict(W=6), "W % 4 == 0"),
    (dict(inp=A + 1), "aligned"),
    (dict(out=A + 2), "aligned"),
    (dict(coarse=A + 2), "aligned"),
    (dict(guide=A + 4), "aligned"),
])
def test_upadd_io_refusals(lib, kw, text):
    rc, err = _upadd(lib, **kw)
    assert rc == 1 and text in err, (rc, err)


def test_upadd_io_empty_image_is_a_noop(lib):
    rc, err = _upadd(lib, B=0, inp=None, out=None)
    assert rc == 0 and err == "" and lib.hdrnet_last_kernel() == b"noop"


def test_upadd_io_f32_to_f32_is_the_float_op(lib):
    """float32 both ways forwards to hdrnet_bilateral_slice_apply_upadd_f32_ex: its refusal text comes back."""
    rc, err = _upadd(lib, idt=0, wl=1.0, odt=0, W=6)
    assert rc == 1 and "slice-apply + up-add needs Cin = Cout = 3" in err


# ---- hdrnet_ops wrappers: shape / dtype rules raise on any device, then the device is required ------------------------
def _cpu_args(dtype=torch.uint8, C=3):
    grid = torch.zeros(1, 2, 2, 2, 3 * (C + 1))
    inp = torch.zeros(1, 4, 8, C, dtype=dtype)
    coarse = torch.zeros(1, 2, 4, 3)
    return grid, inp, coarse


def test_ops_wrappers_refuse(lib):
    from hdrnet_amd import hdrnet_ops as ops
    grid, inp, coarse = _cpu_args()
    guide, c1, c2 = torch.zeros(1, 4, 8), torch.zeros(16, 4), torch.zeros(17)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.resize_bilinear_io(inp, 2, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.bilateral_slice_apply_upadd_io(grid, inp, coarse, guide=guide)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.bilateral_slice_apply_upadd_io(grid, inp, coarse, guide_conv1=c1, guide_conv2=c2, out_dtype=torch.uint8)
    with pytest.raises(TypeError, match="float32, uint8 or uint16"):
        ops.resize_bilinear_io(inp.to(torch.int32), 2, 4)
    with pytest.raises(TypeError, match="float32, uint8 or uint16"):
        ops.bilateral_slice_apply_upadd_io(grid, inp.to(torch.float16), coarse, guide=guide)
    with pytest.raises(TypeError, match="out_dtype must be float32 or uint8"):
        ops.bilateral_slice_apply_upadd_io(grid, inp, coarse, guide=guide, out_dtype=torch.uint16)
    with pytest.raises(ValueError, match="either a guide map or both"):
        ops.bilateral_slice_apply_upadd_io(grid, inp, coarse)
    with pytest.raises(ValueError, match="either a guide map or both"):
        ops.bilateral_slice_apply_upadd_io(grid, inp, coarse, guide=guide, guide_conv1=c1, guide_conv2=c2)
    with pytest.raises(ValueError, match="curves guide"):
        ops.bilateral_slice_apply_upadd_io(grid, inp, coarse, guide_curves=(c1, c1, c1, c2))
    g4, i4, _ = _cpu_args(C=4)
    with pytest.raises(ValueError, match="C = 3"):
        ops.resize_bilinear_io(i4, 2, 4)
    with pytest.raises(ValueError, match="Cin = Cout = 3 with offset"):
        ops.bilateral_slice_apply_upadd_io(torch.zeros(1, 2, 2, 2, 20), i4, coarse, guide=guide)
    with pytest.raises(ValueError, match="coarse should be"):
        ops.bilateral_slice_apply_upadd_io(grid, inp, torch.zeros(1, 2, 4, 4), guide=guide)
    with pytest.raises(ValueError, match="4D"):
        ops.resize_bilinear_io(inp[0], 2, 4)


def test_process_wire_refuses(lib):
    from hdrnet_amd import models
    from hdrnet_amd.runtime import _Process
    torch.manual_seed(3)
    m = models.HDRNetGaussianPyrNN(dict(batch_norm=False))
    frame = torch.zeros(1, 32, 48, 3, dtype=torch.uint8)
    m.train()
    with pytest.raises(RuntimeError, match="inference"):
        m.process_wire(frame, out_dtype=torch.uint8)
    m.eval()
    with pytest.raises(ValueError, match="W % 16 == 0"):
        m.process_wire(torch.zeros(1, 32, 40, 3, dtype=torch.uint8))
    with pytest.raises(TypeError, match="out_dtype"):
        m.process_wire(frame, out_dtype=torch.uint16)
    with pytest.raises(TypeError, match="float32 / uint8 / uint16"):
        m.process_wire(frame.to(torch.int32))
    with pytest.raises(ValueError, match=r"\[B, H, W, 3\]"):
        m.process_wire(frame[0])
    with pytest.raises(TypeError, match="float32"):  # process() keeps its contract
        m.process(frame)
    # the runtime's dispatch: wire formats go to process_wire, float32 -> float32 stays with process
    calls = []
    m.process_wire = lambda f, o, w: calls.append("wire")
    m.process = lambda f, o, w: calls.append("process")
    _Process(m, torch.uint8, None)(frame)
    _Process(m, None, None)(frame)
    _Process(m, torch.uint8, None)(frame.float())
    _Process(m, None, None)(frame.float())
    assert calls == ["wire", "wire", "wire", "process"]
    assert not hasattr(models.HDRNetCurves, "process_wire")  # the single-level models' process() takes the wire formats itself


# ---- the uint8 rule's cap, checked where no GPU is involved -------------------------------------------------------------
def test_u8_rule_cap_holds_for_the_float32_oracle_itself():
    """tests/test_gpu_pyramid_io.py lets fewer than 5e-4 of the uint8 samples differ from the quantised float32 oracle.
    That share is a cap, not a measurement: for the seeds of tests/pyramid_io_cases.py the float32 oracle itself, against
    a float64 evaluation of the same formulas, stays under it in every case -- and its uint8 image reaches 0 and 255, so
    the clip after the up-add is exercised on both sides."""
    import pyramid_io_cases as pc
    worst = 0.0
    for shape in pc.SHAPES:
        for fmt in pc.FORMATS:
            for nn in (False, True):
                c = pc.inputs(shape, fmt, nn)
                w32 = pc.want_f32(shape, fmt, nn)
                w64 = pc.slice_apply_upadd_f64(c, shape)
                assert np.abs(w32 - w64).max() < 1e-5, (shape, fmt, nn, np.abs(w32 - w64).max())  # the same function
                q32, q64 = pc.quantise(w32), pc.quantise(w64)
                share = float((q32 != q64).mean())
                worst = max(worst, share)
                assert share < 5e-4, (shape, fmt, nn, share)
                assert np.abs(q32.astype(np.int16) - q64.astype(np.int16)).max() <= 1
                assert q32.min() == 0 and q32.max() == 255, (shape, fmt, nn)
                assert w32.min() < -0.05 and w32.max() > 1.05  # the sum leaves [0, 1] on both sides
    print(f"float32 oracle vs float64: worst share of differing uint8 samples {worst:.2e} (cap 5e-4)")
