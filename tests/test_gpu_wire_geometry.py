"""The packed (BGR / RGBA / BGRA), YUV-surface and 16-bit-output forwards of csrc/apply_fwd_io.hip.h across row plans, grids
and memory layouts (tests/wire_geometry_cases.py): an interior row segment, the five-segment row of a 4K frame, a row of
more than 8 segments, the vertical clamps and chroma pairs inside and across a grid row, grids of 1 x 1 x 1 to 32 x 32
and 16 planes, surfaces in one allocation per image (image strides beyond the plane), 3-channel frames and planes at the
weakest alignment the argument rules admit.  tests/test_gpu_pixel_formats.py, test_gpu_yuv.py and test_gpu_u16_out.py run
the same instantiations at two toy shapes on one grid; their yardsticks and bars are the ones used here, imported, not
restated:

a. the anchor -- the RGB f32 -> f32 forward against the CPU oracle at tests/test_gpu_fused_fullsize.py's bars and against
   float64 by tests/test_gpu_f64_noise.py's rule; every bit equality below hangs from it;
b. packed frames: bits equal to the RGB path's output, reordered; c. surfaces in: bits equal to the RGB path on
   yuv_to_rgb's frame (itself held against float64); d. surfaces out: the float64 encoders' rule; e. uint16 frames out:
   bits equal to the quantised float32 path; f. every store kind through the C ABI into guarded, twice pre-filled
   buffers; g. every instantiated label ran at every geometry; h. a geometry io_geom refuses is refused by every family
   with its outputs untouched; i. the low-res gathers from the same layouts."""
import os

import numpy as np
import pytest
import torch

import oracle
import pixel_format_cases as px
import test_gpu_pixel_formats as t_px
import test_gpu_u16_out as t_u16
import test_gpu_yuv as t_yuv
import u16_out_cases as uc
import wire_geometry_cases as wg
import yuv_cases as yc
from oracle.f64_ops import f64_slice_apply
from test_gpu_f64_noise import MARGIN, measure, norms
from test_gpu_fused_fullsize import CURVES_GUIDE_TOL, FWD_TOL, NN_GUIDE_TOL, close
from test_sample_prep import reference_lowres

pytestmark = pytest.mark.gpu

GEOS = wg.GEOMETRY_IDS
GUIDE_LABEL = t_yuv.GUIDE_LABEL   # the five guide forms' label suffixes (the packed formats have the first four)
SHORT = {"uint8": "u8", "uint16": "u16", "float32": "f32"}
DTYPE_CODE = {"float32": 0, "uint8": 1, "uint16": 2}
SURFACES = dict(t_yuv.SURFACES)   # kind -> (bits, standard, full range)
LABEL_IN = t_yuv.LABEL_IN

SEEN = {}   # hdrnet_last_kernel() label -> the geometries it ran at (part g)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from hdrnet_amd import hdrnet_ops
    return hdrnet_ops


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def port16(port):
    port.set_threads(min(16, os.cpu_count() or 1))  # the GPU hosts allow 16 CPUs per command
    yield port
    port.set_threads(1)


def T(a, dev):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)
    return torch.from_numpy(a).to(dev)


def N(t):
    if t.dtype == torch.uint16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.detach().cpu().numpy()


def seen(ops, geo, want):
    """Every call's label is asserted exactly and recorded for the coverage test."""
    k = ops.last_kernel()
    assert k == want, (geo, k, want)
    SEEN.setdefault(k, set()).add(geo)


def dview(flat, spec):
    """The device view of a plane in its flat buffer (wire_geometry_cases.plane's twin)."""
    _, off, shape, strides = spec
    return flat.as_strided(shape, strides, off)


_DEV, _REFS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _DEV.clear()
    _REFS.clear()


def on_device(c, dev, ops):
    """The case's grid and guide parameters on the device, uploaded once (the frames and surfaces travel per layout)."""
    if id(c) not in _DEV:
        d = {k: T(c[k], dev) for k in ("grid", "guide", "conv1", "conv2", "ccm", "shifts", "slopes", "shifts20", "slopes20", "mix")}
        d["prepared"] = ops.curves_guide_prepare(d["shifts"], d["slopes"])
        assert d["prepared"] is not None, "the case's knots are apart: the cell tables are usable"
        _DEV[id(c)] = d
    return _DEV[id(c)]


def guide_kw(d, guide):
    if guide == "map":
        return dict(guide=d["guide"])
    if guide == "nn":
        return dict(guide_conv1=d["conv1"], guide_conv2=d["conv2"], return_guide=True)
    names = ("ccm", "shifts20", "slopes20", "mix") if guide == "scan" else ("ccm", "shifts", "slopes", "mix")
    kw = dict(guide_curves=tuple(d[k] for k in names), return_guide=True)
    if guide == "cells":
        kw["curves_prepared"] = d["prepared"]
    return kw


def split(got, guide):
    """(output, guide map or None) of an entry point called with ``guide_kw(d, guide)``."""
    return (got, None) if guide == "map" else got


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def last_error():
    from hdrnet_amd import _lib
    return _lib.last_error()


def differ(tag, got, want):
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), want.view(np.uint32)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{tag}: {len(bad)} of {want.size} samples differ, first at {bad[0]}: got "
                             f"{got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")


# ---- the C ABI with caller-owned buffers: raw addresses, so that an output may sit anywhere --------------------------------
def _p(t):
    return None if t is None else t.data_ptr()


def abi_px(lib, d, guide, inp, out, gout, shape, grid_ext, in_dtype, wl, fmt, dev, out_dtype=None, out_white=None):
    """hdrnet_bilateral_slice_apply_io[_curves]_px, or with ``out_white`` their ..._u16 twins.  ``inp`` / ``out``: addresses."""
    u16 = out_white is not None
    code = px.CODE[fmt]
    frame = (inp, out, *shape, *grid_ext, 3, 3, 1, DTYPE_CODE[in_dtype], float(wl),
             float(out_white) if u16 else DTYPE_CODE[out_dtype])
    codes = (code, code if (u16 or out_dtype == "uint8") else px.CODE["rgb"])
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        if guide in ("map", "nn"):
            fn = lib.hdrnet_bilateral_slice_apply_io_px_u16 if u16 else lib.hdrnet_bilateral_slice_apply_io_px
            net = (None, None, 0) if guide == "map" else (d["conv1"].data_ptr(), d["conv2"].data_ptr(), d["conv1"].shape[0])
            return fn(d["grid"].data_ptr(), d["guide"].data_ptr() if guide == "map" else None, *frame, *net, _p(gout), 0,
                      *codes, stream)
        fn = lib.hdrnet_bilateral_slice_apply_io_curves_px_u16 if u16 else lib.hdrnet_bilateral_slice_apply_io_curves_px
        names = ("ccm", "shifts20", "slopes20", "mix") if guide == "scan" else ("ccm", "shifts", "slopes", "mix")
        return fn(d["grid"].data_ptr(), *frame, *(d[k].data_ptr() for k in names), d[names[1]].shape[0],
                  d["prepared"].data_ptr() if guide == "cells" else None, _p(gout), *codes, stream)


def abi_yuv(lib, d, y, uv, k_in, shape, grid_ext, dev, out_kind=None, out=None, out_uv=None, osurf=(0, 0, 0, 0), k_out=None,
            out_bits=None):
    """hdrnet_bilateral_slice_apply_io_yuv with a guide map, or with ``out_bits`` ..._yuv_p016.  ``y`` / ``uv``: device views;
    ``out`` / ``out_uv``: addresses; ``osurf``: the output's pitches and image strides in bytes."""
    size = y.element_size()
    head = (d["grid"].data_ptr(), d["guide"].data_ptr(), y.data_ptr(), uv.data_ptr(), size, y.stride(1) * size,
            uv.stride(1) * size, y.stride(0) * size, uv.stride(0) * size, *shape, k_in.data_ptr(), *grid_ext, 3, 3, 1,
            None, None, 0, None, 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        if out_bits is not None:
            return lib.hdrnet_bilateral_slice_apply_io_yuv_p016(*head, out, out_uv, *osurf, _p(k_out), out_bits, stream)
        return lib.hdrnet_bilateral_slice_apply_io_yuv(*head, out_kind, out, out_uv, *osurf, _p(k_out), stream)


def guarded(nbytes, fill, dev, guard=256):
    """A byte buffer of ``fill`` with ``guard`` bytes on either side of ``nbytes``: (buffer, address of the body)."""
    buf = torch.full((nbytes + 2 * guard,), fill, dtype=torch.uint8, device=dev)
    assert (buf.data_ptr() + guard) % 16 == 0
    return buf, buf.data_ptr() + guard


def guarded_body(buf, nbytes, fill, dtype, guard=256):
    """The body of a ``guarded`` buffer as ``dtype``, after checking that both guards kept their fill."""
    whole = buf.cpu().numpy()
    assert (whole[:guard] == fill).all() and (whole[guard + nbytes:] == fill).all(), "a store left the output buffer"
    return whole[guard:guard + nbytes].view(dtype)


# ---- a. the anchor ------------------------------------------------------------------------------------------------------------
def oracle_guide(c, guide, x):
    if guide == "map":
        return c["guide"]
    if guide == "nn":
        return oracle.pointwise_nn_guide(x, c["conv1"], c["conv2"])
    return oracle.curves_guide(x, *wg.curves_of(c, guide))


@pytest.mark.parametrize("geo", GEOS)
def test_anchor_rgb_f32_against_the_oracle_and_float64(dev, ops, port16, geo):
    """The RGB f32 -> f32 forward with a guide map, the guide network and the curves guide: against the CPU oracle
    (output rtol = atol = 1e-5 * max(1, GD / 8), as the fuzz of tests/test_gpu_fused_fullsize.py scales it; guides 1e-6 /
    2e-6) and against float64: |HIP - f64| <= 1.5 x |oracle f32 - f64| + 1e-7 in max-norm, 1.5 x in rms, both fed the guide
    the kernel returned (tests/test_gpu_f64_noise.py::fused_case)."""
    shape, grid_ext = wg.GEOMETRIES[geo]
    c = wg.f32_frame_case(geo)
    d = on_device(c, dev, ops)
    x = c["frames"]["rgb"]
    tol = FWD_TOL * max(1.0, grid_ext[2] / 8)
    failures = []
    for guide in ("map", "nn", "curves"):
        out, g = split(ops.bilateral_slice_apply_io(d["grid"], T(x, dev), **guide_kw(d, guide)), guide)
        seen(ops, geo, "apply_fwd_io/f32->f32" + GUIDE_LABEL[guide])
        tag = f"anchor {geo} {guide}"
        want_guide = oracle_guide(c, guide, x)
        if guide != "map":
            close(tag + " guide", N(g), want_guide, rtol=0, atol=NN_GUIDE_TOL if guide == "nn" else CURVES_GUIDE_TOL)
        close(tag + " out", N(out), port16.bilateral_slice_apply(c["grid"], want_guide, x, True), rtol=tol, atol=tol)
        kernel_guide = c["guide"] if guide == "map" else N(g)
        exact = f64_slice_apply(c["grid"], kernel_guide, x, None, True)[0]
        ref = port16.bilateral_slice_apply(c["grid"], kernel_guide, x, True)
        measure(tag, ops.last_kernel(), {"out": N(out)}, {"out": ref}, {"out": exact}, failures)
        (h_max, h_rms, _), (r_max, r_rms, _) = norms(N(out), exact), norms(ref, exact)
        print(f"{tag}: ratio to float64 max {h_max / max(r_max, 1e-300):.3f} rms {h_rms / max(r_rms, 1e-300):.3f}; share of the "
              f"bar used: max {h_max / (MARGIN * r_max + 1e-7):.3f} rms {h_rms / max(MARGIN * r_rms, 1e-300):.3f}")
    assert not failures, "\n".join(failures)


# ---- b. packed formats -------------------------------------------------------------------------------------------------------
def rgb_reference(ops, dev, geo, dtype, wl, out, guide):
    """The RGB path on the case's RGB frame: (output, guide or None) in numpy, once per case, left alone."""
    key = ("px", geo, dtype, wl, out, guide)
    if key not in _REFS:
        c = wg.frame_case(geo, dtype, wl)
        got = ops.bilateral_slice_apply_io(on_device(c, dev, ops)["grid"], T(c["frames"]["rgb"], dev), input_white_level=wl,
                                           out_dtype=getattr(torch, out), **guide_kw(on_device(c, dev, ops), guide))
        seen(ops, geo, f"apply_fwd_io/{SHORT[dtype]}->{SHORT[out]}{GUIDE_LABEL[guide]}")  # RGB: no suffix
        o, g = split(got, guide)
        _REFS[key] = frozen(N(o), None if g is None else N(g))
    return _REFS[key]


@pytest.mark.parametrize("guide", t_px.GUIDES)
@pytest.mark.parametrize("out", ["uint8", "float32"])
@pytest.mark.parametrize("dtype,wl", t_px.WIRE)
@pytest.mark.parametrize("fmt", ["bgr", "rgba", "bgra"])
def test_packed_bits_equal_the_rgb_path(dev, ops, lib, fmt, dtype, wl, out, guide):
    """tests/test_gpu_pixel_formats.py::test_bits_equal_the_rgb_path at every geometry; BGR also from and (uint8 out) into
    storage that starts 4 bytes past a 16-byte boundary, through the C ABI."""
    label = f"apply_fwd_io/{SHORT[dtype]}->{SHORT[out]}{GUIDE_LABEL[guide]}/{fmt}"
    for geo in GEOS:
        shape, grid_ext = wg.GEOMETRIES[geo]
        c = wg.frame_case(geo, dtype, wl)
        d = on_device(c, dev, ops)
        want_rgb, want_guide = rgb_reference(ops, dev, geo, dtype, wl, out, guide)
        frame = c["frames"][fmt]
        want = px.from_rgb(want_rgb, fmt, px.alpha_of(frame, fmt))
        tag = f"{geo} {fmt} {dtype}/{wl} -> {out} {guide}"
        o, g = split(ops.bilateral_slice_apply_io(d["grid"], T(frame, dev), input_white_level=wl, out_dtype=getattr(torch, out),
                                                  pixel_format=fmt, **guide_kw(d, guide)), guide)
        seen(ops, geo, label)
        assert tuple(o.shape) == want.shape and o.dtype == getattr(torch, out), (o.shape, want.shape)
        differ(tag, N(o), want)
        if want_guide is not None:
            differ(tag + " guide", N(g), want_guide)
        if out == "uint8" and geo in ("interior", "uhd_row"):
            assert want[..., :3].min() == 0 and want[..., :3].max() == 255  # the clip is exercised on both sides
            if px.CHANNELS[fmt] == 4:
                assert len(np.unique(want[..., 3])) > 100  # alpha is a plane of its own, not a constant
        if fmt != "bgr":
            continue
        # the same BGR samples 4 bytes off: legal for 3-channel integer frames (check_pixel_buffers)
        host, off = wg.lay_packed(frame, "off4")
        src = T(host, dev)
        inp = src.data_ptr() + off * frame.itemsize
        assert inp % 16 == 4
        gout = torch.empty(shape, dtype=torch.float32, device=dev) if guide != "map" else None
        if out == "float32":   # a float32 output is stored 16 bytes at a time: aligned
            res = torch.full(shape + (3,), float("nan"), dtype=torch.float32, device=dev)
            rc = abi_px(lib, d, guide, inp, res.data_ptr(), gout, shape, grid_ext, dtype, wl, fmt, dev, out_dtype=out)
            assert rc == 0, last_error()
            seen(ops, geo, label)
            differ(tag + " off4", N(res), want)
        else:
            for fill in wg.FILLS:
                dst = torch.full((4 + want.size + wg.GUARD_BYTES,), fill, dtype=torch.uint8, device=dev)
                rc = abi_px(lib, d, guide, inp, dst.data_ptr() + 4, gout, shape, grid_ext, dtype, wl, fmt, dev, out_dtype=out)
                assert rc == 0, last_error()
                seen(ops, geo, label)
                whole = dst.cpu().numpy()
                differ(tag + " off4", whole[4:4 + want.size].reshape(want.shape), want)
                assert (whole[:4] == fill).all() and (whole[4 + want.size:] == fill).all(), "a store left the output frame"
        if want_guide is not None:
            differ(tag + " off4 guide", N(gout), want_guide)
        assert np.array_equal(N(src), host), "the input frame or its guard changed"


# ---- c. surfaces in ----------------------------------------------------------------------------------------------------------
def constants(kind, dev):
    from hdrnet_amd import yuv
    bits, standard, full = SURFACES[kind]
    to_rgb = yuv.yuv_coefficients(standard, full, bits)[0]
    return to_rgb, T(to_rgb, dev)


def surface_in(geo, kind, layout, dev):
    """The case's surface in ``layout`` on the device: (host buffers, device buffers, y view, uv view), uploaded once."""
    key = ("surface", geo, kind, layout)
    if key not in _DEV:
        c = wg.surface_case(geo, SURFACES[kind][0])
        bufs, sy, suv = wg.lay_surface(c["y"], c["uv"], layout)
        flats = [T(b, dev) for b in bufs]
        y, uv = dview(flats[sy[0]], sy), dview(flats[suv[0]], suv)
        if layout == "off4":
            assert y.data_ptr() % 8 == 4 and uv.data_ptr() % 8 == 4
        if layout == "one_allocation":
            assert y.stride(0) == uv.stride(0) > y.stride(1) * y.shape[1]
        _DEV[key] = (bufs, flats, y, uv)
    return _DEV[key]


def inputs_intact(geo, kind):
    """Padding, spare rows, guards -- and the samples -- of every layout of the surface are what was uploaded."""
    for layout in wg.SURFACE_LAYOUTS[geo]:
        key = ("surface", geo, kind, layout)
        if key in _DEV:
            bufs, flats = _DEV[key][:2]
            for b, f in zip(bufs, flats):
                assert np.array_equal(N(f), b), f"{geo} {kind} {layout}: an input buffer changed"


def rgb_frame(ops, dev, geo, kind):
    """``yuv_to_rgb`` of the case's tight surface, float32 on the device: computed once, the input of every reference."""
    key = ("frame", geo, kind)
    if key not in _DEV:
        _, _, y, uv = surface_in(geo, kind, "tight", dev)
        _DEV[key] = ops.yuv_to_rgb(y, uv, constants(kind, dev)[1])
        assert ops.last_kernel() == "yuv_to_rgb"
    return _DEV[key]


def yuv_reference(ops, dev, geo, kind, out, guide):
    """The RGB path on the converted float32 frame: (output, guide or None) in numpy, once per case."""
    key = ("yuv", geo, kind, out, guide)
    if key not in _REFS:
        d = on_device(wg.surface_case(geo, SURFACES[kind][0]), dev, ops)
        got = ops.bilateral_slice_apply_io(d["grid"], rgb_frame(ops, dev, geo, kind), out_dtype=getattr(torch, out),
                                           **guide_kw(d, guide))
        seen(ops, geo, f"apply_fwd_io/f32->{SHORT[out]}{GUIDE_LABEL[guide]}")
        o, g = split(got, guide)
        _REFS[key] = frozen(N(o), None if g is None else N(g))
    return _REFS[key]


@pytest.mark.parametrize("kind", list(SURFACES))
def test_yuv_to_rgb_at_every_geometry_and_layout(dev, ops, kind):
    """tests/test_gpu_yuv.py::test_yuv_to_rgb's bar (atol 2e-6 against the float64 conversion), and the same bits from every
    layout."""
    to_rgb, k = constants(kind, dev)
    for geo in GEOS:
        shape = wg.GEOMETRIES[geo][0]
        c = wg.surface_case(geo, SURFACES[kind][0])
        want = yc.to_rgb64(c["y"], c["uv"], to_rgb)
        assert want.min() == 0.0 and want.max() == 1.0  # both sides of the clamp are reached
        tight = N(rgb_frame(ops, dev, geo, kind))
        for layout in wg.SURFACE_LAYOUTS[geo]:
            _, _, y, uv = surface_in(geo, kind, layout, dev)
            got = ops.yuv_to_rgb(y, uv, k)
            assert ops.last_kernel() == "yuv_to_rgb" and tuple(got.shape) == shape + (3,) and got.dtype == torch.float32
            g = N(got)
            print(f"yuv_to_rgb {kind} {geo} {layout}: max |err| = {np.abs(g - want).max():.3g}")
            np.testing.assert_allclose(g, want, rtol=0, atol=2e-6)
            differ(f"yuv_to_rgb {kind} {geo} {layout} against the tight surface", g, tight)
        inputs_intact(geo, kind)


@pytest.mark.parametrize("guide", t_yuv.GUIDES)
@pytest.mark.parametrize("out", ["uint8", "float32"])
@pytest.mark.parametrize("kind", list(SURFACES))
def test_surfaces_in_bits_equal_convert_then_rgb(dev, ops, kind, out, guide):
    """tests/test_gpu_yuv.py::test_bits_equal_convert_then_rgb at every geometry and layout, with the P010 constants too."""
    k = constants(kind, dev)[1]
    label = f"apply_fwd_io/{LABEL_IN[kind]}->{SHORT[out]}{GUIDE_LABEL[guide]}"
    for geo in GEOS:
        d = on_device(wg.surface_case(geo, SURFACES[kind][0]), dev, ops)
        want, want_guide = yuv_reference(ops, dev, geo, kind, out, guide)
        for layout in wg.SURFACE_LAYOUTS[geo]:
            _, _, y, uv = surface_in(geo, kind, layout, dev)
            o, g = split(ops.bilateral_slice_apply_io_yuv(d["grid"], y, uv, k, out="rgb", out_dtype=getattr(torch, out),
                                                          **guide_kw(d, guide)), guide)
            seen(ops, geo, label)
            assert tuple(o.shape) == want.shape and o.dtype == getattr(torch, out)
            tag = f"{geo} {kind} {layout} -> {out} {guide}"
            differ(tag, N(o), want)
            if want_guide is not None:
                differ(tag + " guide", N(g), want_guide)
        if out == "uint8" and geo in ("interior", "uhd_row"):
            assert want.min() == 0 and want.max() == 255  # the clip is exercised on both sides
        inputs_intact(geo, kind)


# ---- d. surfaces out ---------------------------------------------------------------------------------------------------------
KIND_OF_PAIR = {"nv12->nv12": "nv12", "p016->nv12": "p016", "p010->p010": "p010", "p016->p016": "p016"}


@pytest.mark.parametrize("guide", t_yuv.GUIDES)
@pytest.mark.parametrize("pair", list(wg.SURFACE_OUT))
def test_surfaces_out_against_the_float64_encoders(dev, ops, pair, guide):
    """The rule of test_nv12_output / test_p016_output at every geometry and layout, the output planes laid out as the
    input's: no sample off by more than one code, equal wherever float64 decides by more than eps, low bits zero --
    against the float64 encoder fed with the float32 RGB output of the same path (pinned bit for bit by part c).  The caps
    on undecided samples are conditions on the reference alone.  Everything around the planes keeps both fills."""
    from hdrnet_amd import yuv
    kind = KIND_OF_PAIR[pair]
    bits, standard, full, out_bits = wg.SURFACE_OUT[pair]
    assert SURFACES[kind] == (bits, standard, full)
    from_rgb = yuv.yuv_encode_coefficients(standard, full, out_bits)
    k_in, k_out = constants(kind, dev)[1], T(from_rgb, dev)
    out_dt = np.uint8 if out_bits == 8 else np.uint16
    label = f"apply_fwd_io/{LABEL_IN[kind]}->{'nv12' if out_bits == 8 else 'p016'}{GUIDE_LABEL[guide]}"
    for geo in GEOS:
        shape, _ = wg.GEOMETRIES[geo]
        d = on_device(wg.surface_case(geo, bits), dev, ops)
        rgb, want_guide = yuv_reference(ops, dev, geo, kind, "float32", guide)
        yq, uvq, dy, duv, low_bits = wg.encode64(rgb, from_rgb, out_bits)
        undecided, total = int((~dy).sum() + (~duv).sum()), dy.size + duv.size
        print(f"{pair} {guide} {geo}: {undecided} of the reference's {total} samples undecided ({100.0 * undecided / total:.2f} %)")
        assert wg.within_cap(out_bits, undecided, total), (pair, guide, geo, undecided, total)
        if geo in ("interior", "uhd_row"):
            assert len(np.unique(yq)) > 100 and len(np.unique(uvq)) > 50  # a picture, not a constant
        for layout in wg.SURFACE_LAYOUTS[geo]:
            _, _, y, uv = surface_in(geo, kind, layout, dev)
            lengths, sy, suv = wg.surface_layout(shape, np.dtype(out_dt).itemsize, layout)
            for fill in wg.FILLS:
                flats = [T(np.full(n, wg.fill_value(out_dt, fill), out_dt), dev) for n in lengths]
                oy, ouv = dview(flats[sy[0]], sy), dview(flats[suv[0]], suv)
                if out_bits == 8:
                    got = ops.bilateral_slice_apply_io_yuv(d["grid"], y, uv, k_in, out="nv12", from_rgb=k_out,
                                                           out_planes=(oy, ouv), **guide_kw(d, guide))
                else:
                    got = ops.bilateral_slice_apply_io_yuv_deep(d["grid"], y, uv, k_in, from_rgb=k_out, out_bits=out_bits,
                                                                out_planes=(oy, ouv), **guide_kw(d, guide))
                seen(ops, geo, label)
                (ry, ruv), g = got if want_guide is not None else (got, None)
                assert ry.data_ptr() == oy.data_ptr() and ruv.data_ptr() == ouv.data_ptr()
                host = [N(f) for f in flats]
                for name, spec, want, dec in (("Y", sy, yq, dy), ("UV", suv, uvq, duv)):
                    plane = wg.plane(host, spec)
                    assert not np.any(plane & low_bits), f"{name}: a sample has low bits set"
                    diff = uc.code_diff(plane, want, out_bits) if out_bits != 8 else \
                        np.abs(plane.astype(np.int32) - want.astype(np.int32))
                    tag = f"{pair} {guide} {geo} {layout} {name}"
                    if fill == wg.FILLS[0]:
                        print(f"{tag}: {int((diff > 0).sum())} of {diff.size} differ, max {int(diff.max())}; undecided "
                              f"{int((~dec).sum())}")
                    assert diff.max() <= 1, f"{tag}: off by more than one code"
                    assert np.array_equal(plane[dec], want[dec]), f"{tag}: a sample float64 decides by > eps differs"
                if g is not None:
                    differ(f"{pair} {guide} {geo} {layout} guide", N(g), want_guide)
                for h, m in zip(host, wg.outside_planes(host, (sy, suv))):
                    assert (h[m] == wg.fill_value(out_dt, fill)).all(), \
                        f"{pair} {guide} {geo} {layout}: a store went into padding, a spare row or the guard"
        inputs_intact(geo, kind)


# ---- e. uint16 frames out ----------------------------------------------------------------------------------------------------
def f32_reference(ops, dev, geo, dtype, wl, fmt, guide):
    """The existing entry point on the same inputs, float32 out: (RGB output, guide or None) in numpy, once per case."""
    key = ("u16", geo, dtype, wl, fmt, guide)
    if key not in _REFS:
        c = wg.frame_case(geo, dtype, wl)
        d = on_device(c, dev, ops)
        got = ops.bilateral_slice_apply_io(d["grid"], T(c["frames"][fmt], dev), input_white_level=wl, out_dtype=torch.float32,
                                           pixel_format=fmt, **guide_kw(d, guide))
        seen(ops, geo, f"apply_fwd_io/{SHORT[dtype]}->f32{GUIDE_LABEL[guide]}" + ("" if fmt == "rgb" else "/" + fmt))
        o, g = split(got, guide)
        assert o.dtype == torch.float32 and tuple(o.shape) == wg.GEOMETRIES[geo][0] + (3,)
        _REFS[key] = frozen(N(o), None if g is None else N(g))
    return _REFS[key]


@pytest.mark.parametrize("dtype,wl,fmt,guide", t_u16.INSTANTIATED)
def test_u16_frame_store_equals_the_quantised_f32_path(dev, ops, lib, dtype, wl, fmt, guide):
    """tests/test_gpu_u16_out.py::test_frame_store_equals_the_quantised_f32_path at every geometry; BGR also from and into
    storage 4 bytes off."""
    label = f"apply_fwd_io/{SHORT[dtype]}->u16{GUIDE_LABEL[guide]}" + ("" if fmt == "rgb" else "/" + fmt)
    for geo in GEOS:
        shape, grid_ext = wg.GEOMETRIES[geo]
        c = wg.frame_case(geo, dtype, wl)
        d = on_device(c, dev, ops)
        f, want_guide = f32_reference(ops, dev, geo, dtype, wl, fmt, guide)
        frame = c["frames"][fmt]
        S = px.CHANNELS[fmt]
        if fmt == "bgr":
            host, off = wg.lay_packed(frame, "off4")
            src = T(host, dev)
        for wl_out in t_u16.OUT_WHITE:
            want = uc.quantise_u16(f, wl_out)
            tag = f"{geo} {fmt} {dtype}/{wl} -> u16/{wl_out} {guide}"
            o, g = split(ops.bilateral_slice_apply_io_u16(d["grid"], T(frame, dev), input_white_level=wl,
                                                          output_white_level=wl_out, pixel_format=fmt, **guide_kw(d, guide)), guide)
            seen(ops, geo, label)
            assert o.dtype == torch.uint16 and tuple(o.shape) == shape + (S,), (o.dtype, o.shape)
            o = N(o)
            differ(tag, px.to_rgb(o, fmt), want)   # the output repacked to RGB: the permutation is the input's
            if S == 4:   # alpha: the input's, bit for bit
                assert np.array_equal(px.alpha_of(o, fmt), px.alpha_of(frame, fmt))
            if want_guide is not None:
                differ(tag + " guide", N(g), want_guide)
            if geo in ("interior", "uhd_row"):
                assert want.min() == 0 and want.max() == int(wl_out)  # both clips are hit (from the reference alone)
            if fmt != "bgr":
                continue
            for fill in wg.FILLS:
                dst = torch.full((4 + 2 * want.size + wg.GUARD_BYTES,), fill, dtype=torch.uint8, device=dev)
                gout = torch.empty(shape, dtype=torch.float32, device=dev) if guide != "map" else None
                rc = abi_px(lib, d, guide, src.data_ptr() + 2 * off, dst.data_ptr() + 4, gout, shape, grid_ext, dtype, wl, fmt,
                            dev, out_white=wl_out)
                assert rc == 0, last_error()
                seen(ops, geo, label)
                whole = dst.cpu().numpy()
                body = whole[4:4 + 2 * want.size].view(np.uint16).reshape(shape + (3,))
                differ(tag + " off4", px.to_rgb(body, fmt), want)
                assert (whole[:4] == fill).all() and (whole[4 + 2 * want.size:] == fill).all(), "a store left the output frame"
                if want_guide is not None:
                    differ(tag + " off4 guide", N(gout), want_guide)
        if fmt == "bgr":
            assert np.array_equal(N(src), host), "the input frame or its guard changed"


# ---- f. nothing unwritten, nothing outside -------------------------------------------------------------------------------------
STORE_KINDS = ["f32<-nv12", "u8<-nv12", "u8 bgr", "u8 bgra", "u16 bgr", "u16 bgra", "nv12", "p010"]


@pytest.mark.parametrize("geo", ["uhd_row", "many_seg"])
@pytest.mark.parametrize("kind", STORE_KINDS)
def test_every_store_kind_writes_all_and_only_its_output(dev, ops, lib, kind, geo):
    """One raw C-ABI call per store kind (guide map) into buffers pre-filled twice with different bytes and guarded on both
    sides, in the manner of test_stores_stay_inside_the_buffer: the whole body equals what the Python entry point returns
    for the same inputs under BOTH fills -- so every byte was written -- and the guards keep their fill."""
    from hdrnet_amd import yuv
    shape, grid_ext = wg.GEOMETRIES[geo]
    B, H, W = shape
    if kind in ("f32<-nv12", "u8<-nv12", "nv12", "p010"):
        skind = "p010" if kind == "p010" else "nv12"
        bits, standard, full = SURFACES[skind]
        d = on_device(wg.surface_case(geo, bits), dev, ops)
        _, _, y, uv = surface_in(geo, skind, "tight", dev)
        k_in = constants(skind, dev)[1]
        if kind in ("f32<-nv12", "u8<-nv12"):
            dt = np.float32 if kind[0] == "f" else np.uint8
            out_name = "float32" if kind[0] == "f" else "uint8"
            want = N(ops.bilateral_slice_apply_io_yuv(d["grid"], y, uv, k_in, guide=d["guide"], out_dtype=getattr(torch, out_name)))
            label = f"apply_fwd_io/nv12->{SHORT[out_name]}"
            seen(ops, geo, label)
            for fill in wg.FILLS:
                buf, out = guarded(want.nbytes, fill, dev)
                rc = abi_yuv(lib, d, y, uv, k_in, shape, grid_ext, dev, out_kind=0 if kind[0] == "f" else 1, out=out)
                assert rc == 0, last_error()
                seen(ops, geo, label)
                differ(f"{kind} {geo} fill {fill:#x}", guarded_body(buf, want.nbytes, fill, dt).reshape(want.shape), want)
            return
        out_bits = 8 if kind == "nv12" else 10
        size = 1 if kind == "nv12" else 2
        dt = np.uint8 if kind == "nv12" else np.uint16
        k_out = T(yuv.yuv_encode_coefficients(standard, full, out_bits), dev)
        if kind == "nv12":
            wy, wuv = ops.bilateral_slice_apply_io_yuv(d["grid"], y, uv, k_in, guide=d["guide"], out="nv12", from_rgb=k_out)
        else:
            wy, wuv = ops.bilateral_slice_apply_io_yuv_deep(d["grid"], y, uv, k_in, guide=d["guide"], from_rgb=k_out, out_bits=10)
        label = "apply_fwd_io/nv12->nv12" if kind == "nv12" else "apply_fwd_io/p016->p016"
        seen(ops, geo, label)
        wy, wuv = N(wy), N(wuv)
        osurf = (W * size, W * size, H * W * size, (H // 2) * W * size)
        for fill in wg.FILLS:
            (by, oy), (buv, ouv) = guarded(wy.nbytes, fill, dev), guarded(wuv.nbytes, fill, dev)
            if kind == "nv12":
                rc = abi_yuv(lib, d, y, uv, k_in, shape, grid_ext, dev, out_kind=2, out=oy, out_uv=ouv, osurf=osurf, k_out=k_out)
            else:
                rc = abi_yuv(lib, d, y, uv, k_in, shape, grid_ext, dev, out=oy, out_uv=ouv, osurf=osurf, k_out=k_out, out_bits=10)
            assert rc == 0, last_error()
            seen(ops, geo, label)
            differ(f"{kind} {geo} Y fill {fill:#x}", guarded_body(by, wy.nbytes, fill, dt).reshape(wy.shape), wy)
            differ(f"{kind} {geo} UV fill {fill:#x}", guarded_body(buv, wuv.nbytes, fill, dt).reshape(wuv.shape), wuv)
        return
    depth, fmt = kind.split()
    dtype, wl = ("uint8", 255.0) if depth == "u8" else ("uint16", 65535.0)
    c = wg.frame_case(geo, dtype, wl)
    d = on_device(c, dev, ops)
    frame = T(c["frames"][fmt], dev)
    if depth == "u8":
        want = N(ops.bilateral_slice_apply_io(d["grid"], frame, guide=d["guide"], input_white_level=wl, out_dtype=torch.uint8,
                                              pixel_format=fmt))
        kw = dict(out_dtype="uint8")
    else:
        want = N(ops.bilateral_slice_apply_io_u16(d["grid"], frame, guide=d["guide"], input_white_level=wl,
                                                  output_white_level=32767.0, pixel_format=fmt))
        kw = dict(out_white=32767.0)
    label = f"apply_fwd_io/{depth}->{depth}/{fmt}"
    seen(ops, geo, label)
    assert want.shape == shape + (px.CHANNELS[fmt],)
    for fill in wg.FILLS:
        buf, out = guarded(want.nbytes, fill, dev)
        rc = abi_px(lib, d, "map", frame.data_ptr(), out, None, shape, grid_ext, dtype, wl, fmt, dev, **kw)
        assert rc == 0, last_error()
        seen(ops, geo, label)
        differ(f"{kind} {geo} fill {fill:#x}", guarded_body(buf, want.nbytes, fill, want.dtype).reshape(want.shape), want)


# ---- h. a geometry io_geom refuses ---------------------------------------------------------------------------------------------
WIRE_REFUSAL = "the wire-format forward supports Cin = Cout = 3 with offset"
YUV_REFUSAL = "the YUV forward supports Cin = Cout = 3 with offset"


@pytest.mark.parametrize("family", ["io", "px", "yuv", "u16", "p016"])
def test_a_refused_geometry_leaves_the_outputs_alone(dev, ops, lib, family):
    """(1, 4, 96) on a 16 x 32 x 40 grid: the LDS image does not fit and these families have no other kernel.  The C ABI
    returns HDRNET_INVALID_ARGUMENT before any launch (capi.hip: launch_io asks the predicate first) with the text
    refuse_fused reports for a frame within the extents -- the entry point's own rules --, the poisoned outputs are
    untouched, no kernel is recorded, and the Python entry point raises."""
    from hdrnet_amd import _lib, yuv
    shape, grid_ext = wg.REFUSED
    B, H, W = shape
    fill = wg.FILLS[0]
    if family in ("yuv", "p016"):
        kind = "nv12" if family == "yuv" else "p010"
        bits, standard, full = SURFACES[kind]
        out_bits = 8 if family == "yuv" else 10
        size = 1 if family == "yuv" else 2
        c = wg.surface_case("refused", bits)
        d = on_device(c, dev, ops)
        before = _lib.last_kernel()   # (the case's set-up has prepared its curve tables by now)
        y, uv = T(c["y"], dev), T(c["uv"], dev)
        k_in, k_out = constants(kind, dev)[1], T(yuv.yuv_encode_coefficients(standard, full, out_bits), dev)
        (by, oy), (buv, ouv) = guarded(H * W * size, fill, dev), guarded(H // 2 * W * size, fill, dev)
        osurf = (W * size, W * size, H * W * size, (H // 2) * W * size)
        if family == "yuv":
            rc = abi_yuv(lib, d, y, uv, k_in, shape, grid_ext, dev, out_kind=2, out=oy, out_uv=ouv, osurf=osurf, k_out=k_out)
        else:
            rc = abi_yuv(lib, d, y, uv, k_in, shape, grid_ext, dev, out=oy, out_uv=ouv, osurf=osurf, k_out=k_out, out_bits=10)
        assert rc == _lib.HDRNET_INVALID_ARGUMENT and YUV_REFUSAL in _lib.last_error(), (rc, _lib.last_error())
        torch.cuda.synchronize(dev)
        assert (by.cpu().numpy() == fill).all() and (buv.cpu().numpy() == fill).all(), "a refused call wrote"
        with pytest.raises(_lib.HdrnetInvalidArgument, match="the YUV forward supports"):
            if family == "yuv":
                ops.bilateral_slice_apply_io_yuv(d["grid"], y, uv, k_in, guide=d["guide"], out="nv12", from_rgb=k_out)
            else:
                ops.bilateral_slice_apply_io_yuv_deep(d["grid"], y, uv, k_in, guide=d["guide"], from_rgb=k_out, out_bits=10)
    else:
        dtype, wl, fmt = {"io": ("uint8", 255.0, "rgb"), "px": ("uint8", 255.0, "bgr"), "u16": ("uint16", 65535.0, "bgra")}[family]
        c = wg.frame_case("refused", dtype, wl)
        d = on_device(c, dev, ops)
        before = _lib.last_kernel()
        frame = T(c["frames"][fmt], dev)
        nbytes = frame.numel() * frame.element_size()
        buf, out = guarded(nbytes, fill, dev)
        if family == "io":
            with torch.cuda.device(dev):
                rc = lib.hdrnet_bilateral_slice_apply_io_ex(d["grid"].data_ptr(), d["guide"].data_ptr(), frame.data_ptr(), out,
                                                            *shape, *grid_ext, 3, 3, 1, 1, wl, 1, None, None, 0, None, 0,
                                                            torch.cuda.current_stream(dev).cuda_stream)
        else:
            kw = dict(out_dtype="uint8") if family == "px" else dict(out_white=65535.0)
            rc = abi_px(lib, d, "map", frame.data_ptr(), out, None, shape, grid_ext, dtype, wl, fmt, dev, **kw)
        assert rc == _lib.HDRNET_INVALID_ARGUMENT and WIRE_REFUSAL in _lib.last_error(), (rc, _lib.last_error())
        torch.cuda.synchronize(dev)
        assert (buf.cpu().numpy() == fill).all(), "a refused call wrote"
        with pytest.raises(_lib.HdrnetInvalidArgument, match="the wire-format forward supports"):
            if family == "u16":
                ops.bilateral_slice_apply_io_u16(d["grid"], frame, guide=d["guide"], input_white_level=wl, pixel_format=fmt)
            else:
                ops.bilateral_slice_apply_io(d["grid"], frame, guide=d["guide"], input_white_level=wl, out_dtype=torch.uint8,
                                             pixel_format=fmt)
    assert _lib.last_kernel() == before, "a refused call recorded a kernel"


# ---- i. the low-res gathers from the same layouts ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 5])  # 6: the vector store (n * n % 4 == 0); 5: the scalar tail
def test_lowres_inputs_from_one_allocation_and_four_bytes_off(dev, ops, n):
    """``lowres_input_yuv`` from the one-allocation surface and ``lowres_input`` from the BGR frame 4 bytes off, at the 4K
    row: bit-equal to the numpy nearest-neighbour reference (tests/test_sample_prep.py::reference_lowres) of the frame."""
    from hdrnet_amd import _lib, data
    geo = "uhd_row"
    shape = wg.GEOMETRIES[geo][0]
    for kind in ("nv12", "p010"):
        _, _, y, uv = surface_in(geo, kind, "one_allocation", dev)
        got = data.lowres_input_yuv(y, uv, constants(kind, dev)[1], n)
        assert _lib.last_kernel() == "sample_prep" and tuple(got.shape) == (shape[0], n, n, 3)
        full = N(rgb_frame(ops, dev, geo, kind))   # held against float64 by test_yuv_to_rgb_at_every_geometry_and_layout
        differ(f"lowres_input_yuv {kind} n={n}", N(got), np.stack([reference_lowres(im, n) for im in full]))
        inputs_intact(geo, kind)
    for dtype, wl in (("uint8", 255.0), ("uint16", 65535.0)):
        frame = wg.frame_case(geo, dtype, wl)["frames"]["bgr"]
        host, off = wg.lay_packed(frame, "off4")
        src = T(host, dev)
        view = src[off:off + frame.size].view(frame.shape)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        got = data.lowres_input(view, n, wl, pixel_format="bgr")
        assert _lib.last_kernel() == "sample_prep" and tuple(got.shape) == (shape[0], n, n, 3)
        full = px.to_rgb(frame, "bgr").astype(np.float32) / np.float32(wl)
        differ(f"lowres_input bgr {dtype} n={n}", N(got), np.stack([reference_lowres(im, n) for im in full]))
        assert len(np.unique(N(got))) > 8


# ---- g. coverage: the last test of the module ----------------------------------------------------------------------------------
def instantiated_labels():
    """Every kernel label of the three families, from the existing files' tables."""
    labels = {f"apply_fwd_io/{SHORT[d]}->{SHORT[o]}{t_px.GUIDE_LABEL[g]}/{f}"
              for f in ("bgr", "rgba", "bgra") for d, _ in t_px.WIRE for o in ("uint8", "float32") for g in t_px.GUIDES}
    labels |= {f"apply_fwd_io/{LABEL_IN[k]}->{o}{GUIDE_LABEL[g]}" for k in SURFACES for o in ("f32", "u8", "nv12")
               for g in t_yuv.GUIDES}
    labels |= {f"apply_fwd_io/{SHORT[d]}->u16{GUIDE_LABEL[g]}" + ("" if f == "rgb" else "/" + f) for d, _, f, g in t_u16.INSTANTIATED}
    labels |= {f"apply_fwd_io/p016->p016{GUIDE_LABEL[g]}" for g in t_u16.GUIDES}
    return labels


def in_the_three_families(label):
    return label.endswith(("/bgr", "/rgba", "/bgra")) or "nv12" in label or "p016" in label or "->u16" in label


def test_every_instantiated_label_ran_at_every_geometry():
    """Needs the whole module to have run: a branch of a test above that is quietly skipped fails here."""
    want = instantiated_labels()
    assert len(want) == 48 + 30 + 22 + 5   # packed, surfaces in / NV12 out, uint16 frames, P010 / P016 surfaces
    ran = {k for k in SEEN if in_the_three_families(k)}
    assert ran == want, f"never ran: {sorted(want - ran)}; not in the tables: {sorted(ran - want)}"
    short = {k: sorted(set(GEOS) - SEEN[k]) for k in sorted(want) if SEEN[k] != set(GEOS)}
    assert not short, f"labels that missed a geometry: {short}"
    print(f"{len(want)} labels of the three families at {len(GEOS)} geometries each; {len(SEEN) - len(want)} RGB reference labels")
