"""The pyramid model on YUV 4:2:0 surfaces on the GPU (include/hdrnet_amd_pyramid_yuv.h): the resize that reads a surface, the
finest level's slice-apply + up-add with the surface load and stores, HDRNetGaussianPyrNN.process_wire_yuv[_planar] and their
replay from a hipGraph.

Yardsticks.  The resize: oracle.resize_bilinear_align_corners of the GPU's own yuv_to_rgb output, at the existing resize
bar.  The up-add forward, float32 out: bilateral_slice_apply_upadd on the converted float32 frame at the forward's bar
(pyramid_io_cases.TOL), and for a guide map the composed CPU oracle of tests/pyramid_yuv_cases.py; uint8 out:
pyramid_io_cases.check_u8; a surface out: the rule of test_nv12_output -- equal wherever float64 decides the code by more
than eps_of(bits), one code elsewhere -- against the float64 encoder fed with the kernel's own float32 output.  Inside the
family the results are held bit for bit: planar = semi-planar on the interleaved surface, pitched = tight, prescaled =
exported guide arrays.  ``last_kernel()`` must carry the surface label and ``+upadd``."""
import numpy as np
import pytest
import torch

import pyramid_io_cases as pio
import pyramid_yuv_cases as pyc
import yuv_planar_cases as ypc

pytestmark = pytest.mark.gpu

GUARD = 64  # float32 elements on either side of a resize output


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
    if not a.flags.writeable:  # (the shared references are read-only)
        a = a.copy()
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)
    return torch.from_numpy(a).to(dev)


def N(t):
    if t.dtype == torch.uint16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.detach().cpu().numpy()


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def device_planes(planes, pad, dev):
    """The device views of a surface's planes, each inside rows ``pad`` bytes wider with poisoned padding."""
    return tuple(T(pyc.pitched(p, pad), dev)[:, :, :p.shape[2]] for p in planes)


def surface_bytes(t):
    """(pitch, image stride) of a plane view in bytes."""
    return t.stride(1) * t.element_size(), t.stride(0) * t.element_size()


# ---- 5. the resize -----------------------------------------------------------------------------------------------------
RESIZE_CASES = [
    (2, 38, 52, 19, 26),    # pitched by 64 bytes below, as every case is; two images
    (1, 64, 96, 32, 48),    # the pyramid's 2:1
    (1, 10, 12, 5, 7),      # the scalar store tail
    (1, 10, 12, 1, 1),      # a single output pixel
    (1, 20, 32, 20, 32),    # identity extents
    (1, 6, 3840, 3, 1920),  # wide rows
]
RESIZE_LABEL = {"nv12": "nv12", "p010": "p016", "i420": "i420", "i010": "i016"}


def _resize_capi(lib, kind, planes, k, out, shape, Hout, Wout, dev):
    B, H, W = shape
    dt = planes[0].element_size()
    pitches, strides = zip(*(surface_bytes(p) for p in planes))
    fn = lib.hdrnet_resize_bilinear_yuv_planar if pyc.KINDS[kind][3] else lib.hdrnet_resize_bilinear_yuv
    return fn(*(p.data_ptr() for p in planes), dt, *pitches, *strides, B, H, W, k.data_ptr(), out.data_ptr(), Hout, Wout,
              stream(dev))


@pytest.mark.parametrize("kind", list(RESIZE_LABEL))
@pytest.mark.parametrize("case", RESIZE_CASES, ids=["x".join(map(str, c)) for c in RESIZE_CASES])
def test_resize_yuv_matches_oracle(dev, ops, case, kind):
    import oracle
    from hdrnet_amd import _lib
    B, Hin, Win, Hout, Wout = case
    bits, planar_kind = pyc.bits_of(kind), pyc.KINDS[kind][3]
    rng = np.random.default_rng([51, *case, bits])
    planar, semi = pyc.surface(rng, (B, Hin, Win), bits)
    k = T(pyc.constants(kind)[0], dev)
    k_semi = T(pyc.constants(pyc.TWIN.get(kind, kind))[0], dev)
    ys, uvs = device_planes(semi, 0, dev)
    rgb = ops.yuv_to_rgb(ys, uvs, k_semi)  # the GPU's own conversion: the frame whose resize this is
    want = oracle.resize_bilinear_align_corners(N(rgb), Hout, Wout)
    tight = device_planes(planar if planar_kind else semi, 0, dev)
    n = B * Hout * Wout * 3
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=dev)
    out = buf[GUARD:GUARD + n].view(B, Hout, Wout, 3)
    rc = _resize_capi(_lib.load(), kind, tight, k, out, (B, Hin, Win), Hout, Wout, dev)
    assert rc == 0, _lib.last_error()
    assert ops.last_kernel() == "resize_bilinear_yuv/" + RESIZE_LABEL[kind]
    got = N(out)
    assert np.isfinite(got).all()
    print(f"resize {kind} {case}: max |err| {np.abs(got - want).max():.3e}")
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-7)  # the existing resize bar
    nan = torch.full((GUARD,), float("nan"), device=dev).view(torch.int32)
    assert torch.equal(buf[:GUARD].view(torch.int32), nan) and torch.equal(buf[-GUARD:].view(torch.int32), nan)
    # an output that is only 4-byte aligned: the scalar stores, the same bits
    buf1 = torch.full((n + 2 * GUARD + 1,), float("nan"), device=dev)
    out1 = buf1[GUARD + 1:GUARD + 1 + n].view(B, Hout, Wout, 3)
    assert out1.data_ptr() % 16 == 4
    assert _resize_capi(_lib.load(), kind, tight, k, out1, (B, Hin, Win), Hout, Wout, dev) == 0, _lib.last_error()
    assert bits_equal(out1, out)
    assert torch.equal(buf1[:GUARD + 1].view(torch.int32), torch.full((GUARD + 1,), float("nan"), device=dev).view(torch.int32))
    assert torch.equal(buf1[-GUARD:].view(torch.int32), nan)
    # the op; pitched = tight; planar = semi-planar on the interleaved surface
    op = ops.resize_bilinear_yuv_planar if planar_kind else ops.resize_bilinear_yuv
    assert bits_equal(op(*tight, k, Hout, Wout), out)
    assert bits_equal(op(*device_planes(planar if planar_kind else semi, 64, dev), k, Hout, Wout), out)
    if planar_kind:
        assert bits_equal(ops.resize_bilinear_yuv(ys, uvs, k_semi, Hout, Wout), out)
        assert ops.last_kernel() == "resize_bilinear_yuv/" + RESIZE_LABEL[pyc.TWIN[kind]]
    f32 = ops.resize_bilinear(rgb, Hout, Wout)
    print(f"vs resize_bilinear(yuv_to_rgb(...)): bit-equal {bits_equal(f32, out)}, max |diff| "
          f"{float((f32 - out).abs().max()):.3e}")


def test_resize_yuv_empty_output_is_a_noop(dev, ops):
    planar, semi = pyc.surface(np.random.default_rng(5), (1, 4, 8), 8)
    k = T(pyc.constants("nv12")[0], dev)
    got = ops.resize_bilinear_yuv(*device_planes(semi, 0, dev), k, 0, 5)
    assert tuple(got.shape) == (1, 0, 5, 3) and ops.last_kernel() == "noop"
    got = ops.resize_bilinear_yuv_planar(*device_planes(planar, 0, dev), T(pyc.constants("i420")[0], dev), 3, 0)
    assert tuple(got.shape) == (1, 3, 0, 3) and ops.last_kernel() == "noop"


# ---- 6. the up-add forward ---------------------------------------------------------------------------------------------
def _call(ops, kind, grid, planes, k, coarse, gkw, **kw):
    if pyc.KINDS[kind][3]:
        return ops.bilateral_slice_apply_upadd_io_yuv_planar(grid, *planes, k, coarse, **gkw, **kw)
    return ops.bilateral_slice_apply_upadd_io_yuv(grid, *planes, k, coarse, **gkw, **kw)


def _out_planes(kind, shape, pad, fill, dev):
    """Poisoned output planes of the kind's surface output, rows ``pad`` bytes wider, a guard behind each plane:
    ``(flat buffers, views, (rows, cols, pitch) per plane)`` in samples."""
    B, H, W = shape
    out_bits = pyc.KINDS[kind][5][2]
    dt = np.uint8 if out_bits == 8 else np.uint16
    size = np.dtype(dt).itemsize
    dims = [(H, W), (H // 2, W // 2), (H // 2, W // 2)] if pyc.KINDS[kind][3] else [(H, W), (H // 2, W)]
    flats, views, geo = [], [], []
    for rows, cols in dims:
        pitch = cols + pad // size
        flat = T(np.full(B * rows * pitch + pyc.GUARD_BYTES // size, ypc.fill_value(dt, fill), dt), dev)
        flats.append(flat)
        views.append(flat[:B * rows * pitch].view(B, rows, pitch)[:, :, :cols])
        geo.append((rows, cols, pitch))
    return flats, views, geo


@pytest.mark.parametrize("nn", [False, True], ids=["map", "nnguide"])
@pytest.mark.parametrize("kind", list(pyc.KINDS))
@pytest.mark.parametrize("shape", pyc.SHAPES, ids=["x".join(map(str, s)) for s in pyc.SHAPES])
def test_upadd_io_yuv(dev, ops, shape, kind, nn):
    B, H, W, Hc, Wc = shape
    bits, _, _, planar_kind, label_in, (out_name, label_out, out_bits) = pyc.KINDS[kind]
    c = pyc.inputs(shape, kind, nn)
    to_rgb, from_rgb = pyc.constants(kind)
    k, k_out = T(to_rgb, dev), T(from_rgb, dev)
    grid, coarse = T(c["grid"], dev), T(c["coarse"], dev)
    gkw = dict(guide_conv1=T(c["conv1"], dev), guide_conv2=T(c["conv2"], dev)) if nn else dict(guide=T(c["guide"], dev))
    suffix = ("+nnguide" if nn else "") + "+upadd"
    src = c["planar"] if planar_kind else c["semi"]
    surf_kw = dict(out=out_name, from_rgb=k_out)
    if out_name == "planar":
        surf_kw["out_bits"] = out_bits

    # the float32 reference: the float op on the frame the conversion writes
    tight = device_planes(src, 0, dev)
    frame = ops.yuv_planar_to_rgb(*tight, k) if planar_kind else ops.yuv_to_rgb(*tight, k)
    ref = N(ops.bilateral_slice_apply_upadd(grid, frame, coarse, **gkw))

    results = {}
    for pad in pyc.PADS:
        planes = device_planes(src, pad, dev)
        f32 = _call(ops, kind, grid, planes, k, coarse, gkw)
        assert ops.last_kernel() == f"apply_fwd_io/{label_in}->f32{suffix}"
        assert f32.dtype == torch.float32 and tuple(f32.shape) == (B, H, W, 3)
        u8 = _call(ops, kind, grid, planes, k, coarse, gkw, out_dtype=torch.uint8)
        assert ops.last_kernel() == f"apply_fwd_io/{label_in}->u8{suffix}"
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (B, H, W, 3)
        if pad == 0:
            g = N(f32)
            print(f"{shape} {kind} nn={nn}: f32 out max |err| vs the float op {np.abs(g - ref).max():.3e}")
            np.testing.assert_allclose(g, ref, rtol=pyc.TOL, atol=pyc.TOL)
            if not nn:  # ... and the composed CPU oracle, with the case's guide map
                np.testing.assert_allclose(g, pyc.want_f32(shape, kind, nn), rtol=pyc.TOL, atol=pyc.TOL)
            pio.check_u8(N(u8), ref, f"{shape} {kind} nn={nn} u8")
            codes, _, decided, _ = pyc.encode(g, kind)  # the float64 encoder on the kernel's own float32 output
        for fill in (pyc.FILLS[:1] if pad == 0 else pyc.FILLS):
            flats, views, geo = _out_planes(kind, (B, H, W), pad, fill, dev)
            got = _call(ops, kind, grid, planes, k, coarse, gkw, out_planes=tuple(views), **surf_kw)
            assert ops.last_kernel() == f"apply_fwd_io/{label_in}->{label_out}{suffix}"
            assert len(got) == len(views) and all(r.data_ptr() == v.data_ptr() for r, v in zip(got, views))
            stored = pyc.stored_planes(kind, [N(v) for v in views])
            for name, plane, want, dec in zip("YUV", stored, codes, decided):
                diff = np.abs(plane.astype(np.int64) - want.astype(np.int64))
                print(f"{shape} {kind} nn={nn} pad {pad} {name}: {int((diff > 0).sum())} of {diff.size} differ, max "
                      f"{int(diff.max())}; undecided {int((~dec).sum())}")
                assert np.array_equal(plane[dec], want[dec]), f"{name}: a sample float64 decides by > eps differs"
                assert diff.max() <= 1, f"{name}: off by more than one code"
            value = ypc.fill_value(np.uint8 if out_bits == 8 else np.uint16, fill)
            for flat, (rows, cols, pitch) in zip(flats, geo):  # padding and the guard behind each plane keep their fill
                whole = N(flat)
                body = whole[:B * rows * pitch].reshape(B, rows, pitch)
                assert (body[:, :, cols:] == value).all(), "a store went into the row padding"
                assert (whole[B * rows * pitch:] == value).all(), "a store left the output plane"
        surface = tuple(v.contiguous() for v in views)
        if pad == 0:
            assert len(np.unique(stored[0])) > 50  # a picture, not a constant
            results = dict(f32=f32, u8=u8, surface=surface)
            allocated = _call(ops, kind, grid, planes, k, coarse, gkw, **surf_kw)  # tight planes of its own
            assert all(a.is_contiguous() and bits_equal(a, s) for a, s in zip(allocated, surface))
        else:  # pitched = tight, bit for bit
            assert bits_equal(f32, results["f32"]) and bits_equal(u8, results["u8"])
            assert all(bits_equal(a, b) for a, b in zip(surface, results["surface"]))

    if nn:  # prescaled = exported guide arrays
        p1, p2 = ops.guide_nn_prescale(gkw["guide_conv1"], gkw["guide_conv2"])
        pkw = dict(guide_conv1=p1, guide_conv2=p2, prescaled=True)
        assert bits_equal(_call(ops, kind, grid, tight, k, coarse, pkw), results["f32"])
        assert bits_equal(_call(ops, kind, grid, tight, k, coarse, pkw, out_dtype=torch.uint8), results["u8"])
        pre = _call(ops, kind, grid, tight, k, coarse, pkw, **surf_kw)
        assert all(bits_equal(a, b) for a, b in zip(pre, results["surface"]))
        fast = _call(ops, kind, grid, tight, k, coarse, dict(gkw, fast_sigmoid=True))
        np.testing.assert_allclose(N(fast), N(results["f32"]), rtol=pyc.TOL, atol=pyc.TOL)

    if planar_kind:  # planar = semi-planar on the interleaved surface, for every output kind
        twin = pyc.TWIN[kind]
        k2, k2_out = T(pyc.constants(twin)[0], dev), T(pyc.constants(twin)[1], dev)
        semi = device_planes(c["semi"], 0, dev)
        assert bits_equal(_call(ops, twin, grid, semi, k2, coarse, gkw), results["f32"])
        assert bits_equal(_call(ops, twin, grid, semi, k2, coarse, gkw, out_dtype=torch.uint8), results["u8"])
        other = _call(ops, twin, grid, semi, k2, coarse, gkw, out=pyc.KINDS[twin][5][0], from_rgb=k2_out)
        assert ops.last_kernel() == f"apply_fwd_io/{pyc.KINDS[twin][4]}->{pyc.KINDS[twin][5][1]}{suffix}"
        for a, b in zip(pyc.stored_planes(twin, [N(p) for p in other]), (N(p) for p in results["surface"])):
            assert np.array_equal(a, b)


def test_upadd_io_yuv_refuses_on_the_device(dev, ops):
    from hdrnet_amd import _lib
    grid = torch.rand((1, 4, 4, 4, 12), device=dev)
    y, uv = torch.zeros((1, 4, 16), dtype=torch.uint8, device=dev), torch.zeros((1, 2, 16), dtype=torch.uint8, device=dev)
    k, coarse, guide = torch.zeros(12, device=dev), torch.rand((1, 2, 8, 3), device=dev), torch.rand((1, 4, 16), device=dev)
    with pytest.raises(ValueError, match="exactly one of"):
        ops.bilateral_slice_apply_upadd_io_yuv(grid, y, uv, k, coarse)
    flat = torch.rand(1 * 2 * 8 * 3 + 4, device=dev)  # (a coarse level 2 bytes off a dword: through the C ABI)
    out = torch.zeros((1, 4, 16, 3), device=dev)
    rc = _lib.load().hdrnet_bilateral_slice_apply_upadd_io_yuv(
        grid.data_ptr(), guide.data_ptr(), y.data_ptr(), uv.data_ptr(), 1, 16, 16, 0, 0, 1, 4, 16, k.data_ptr(), flat.data_ptr() + 2,
        2, 8, 4, 4, 4, 3, 3, 1, None, None, 0, 0, 0, out.data_ptr(), None, 0, 0, 0, 0, None, stream(dev))
    assert rc == 1 and "coarse must be a 4-B aligned buffer" in _lib.last_error()


# ---- 7. the model ------------------------------------------------------------------------------------------------------
def _model(dev, cls="HDRNetGaussianPyrNN", seed=7):
    from hdrnet_amd import models
    torch.manual_seed(seed)
    return getattr(models, cls)(dict(batch_norm=False)).to(dev).eval()


def _by_hand(m, planes, k, planar, **fine_kw):
    """process_wire_yuv[_planar]'s launches, spelled out with the ops."""
    from hdrnet_amd import data, hdrnet_ops as ops
    H, W = planes[0].shape[1:3]
    with torch.no_grad():
        if planar:
            low = data.lowres_input_yuv_planar(*planes, k, m.params["net_input_size"])
            l1 = ops.resize_bilinear_yuv_planar(*planes, k, H // 2, W // 2)
        else:
            low = data.lowres_input_yuv(*planes, k, m.params["net_input_size"])
            l1 = ops.resize_bilinear_yuv(*planes, k, H // 2, W // 2)
        grids = m.coefficients.levels(low)
        l2 = ops.resize_bilinear(l1, H // 4, W // 4)
        gp = [g.inference_params(m.prescale_guide) for g in m.guide]
        kw = dict(has_offset=True, fast_sigmoid=m.fast_sigmoid)
        cur = ops.bilateral_slice_apply_nnguide(grids[0], l2, gp[2][0], gp[2][1], prescaled=gp[2][2], **kw)
        cur = ops.bilateral_slice_apply_upadd(grids[1], l1, cur, guide_conv1=gp[1][0], guide_conv2=gp[1][1], prescaled=gp[1][2],
                                              **kw)
        fine = ops.bilateral_slice_apply_upadd_io_yuv_planar if planar else ops.bilateral_slice_apply_upadd_io_yuv
        return fine(grids[2], *planes, k, cur, guide_conv1=gp[0][0], guide_conv2=gp[0][1], fast_sigmoid=m.fast_sigmoid,
                    prescaled=gp[0][2], **fine_kw)


def _check_quantised(got_u8, float_out, what):
    """test_process_wire_matches_the_float_path's rule for a uint8 frame."""
    want = (255 * float_out.clamp(0, 1)).to(torch.uint8)
    diff = (got_u8.to(torch.int16) - want.to(torch.int16)).abs()
    share = float((diff > 0).float().mean())
    print(f"{what}: vs the quantised float path max LSB {int(diff.max())}, share differing {share:.2e}")
    assert int(diff.max()) <= 1 and share < 5e-4
    assert len(torch.unique(got_u8)) > 8  # a picture, not a constant


SHAPE = (1, 272, 480)


def test_process_wire_yuv_matches_the_float_path(dev, ops):
    from hdrnet_amd import yuv
    m = _model(dev)
    _, semi = pyc.picture(np.random.default_rng(61), SHAPE, 8)
    y, uv = device_planes(semi, 0, dev)
    to_rgb, from_rgb = yuv.yuv_coefficients("bt709", False, 8)
    k, k_out = T(to_rgb, dev), T(from_rgb, dev)
    want = m.process(ops.yuv_to_rgb(y, uv, k))
    got = m.process_wire_yuv(y, uv)
    assert ops.last_kernel() == "apply_fwd_io/nv12->f32+nnguide+upadd"
    assert got.dtype == torch.float32 and tuple(got.shape) == SHAPE + (3,)
    assert torch.equal(got, _by_hand(m, (y, uv), k, False))
    np.testing.assert_allclose(N(got), N(want), rtol=5e-5, atol=5e-5)
    got8 = m.process_wire_yuv(y, uv, out_dtype=torch.uint8)
    assert ops.last_kernel() == "apply_fwd_io/nv12->u8+nnguide+upadd"
    assert torch.equal(got8, _by_hand(m, (y, uv), k, False, out_dtype=torch.uint8))
    _check_quantised(got8, want, "nv12 -> u8")
    oy, ouv = m.process_wire_yuv(y, uv, out="nv12")
    assert ops.last_kernel() == "apply_fwd_io/nv12->nv12+nnguide+upadd"
    hy, huv = _by_hand(m, (y, uv), k, False, out="nv12", from_rgb=k_out)
    assert oy.dtype == torch.uint8 and tuple(oy.shape) == SHAPE and tuple(ouv.shape) == (1, 136, 480)
    assert torch.equal(oy, hy) and torch.equal(ouv, huv)
    assert len(torch.unique(oy)) > 8 and len(torch.unique(ouv)) > 8  # pictures
    # the surface out decodes to the float frame within a code of each plane's step (a sanity bound, not a bar: chroma is
    # the mean of a 2 x 2 block): the luma plane alone, against the float64 luma of the float32 frame
    y_want = np.clip(N(want).astype(np.float64), 0, 1) @ from_rgb[0:3].astype(np.float64) + float(from_rgb[9])
    assert np.abs(N(oy).astype(np.float64) - np.floor(np.clip(y_want, 0, 255))).max() <= 1
    # pitched planes in, planes of the caller's out
    py, puv = device_planes(semi, 64, dev)
    qy, quv = torch.zeros_like(oy), torch.zeros_like(ouv)
    ry, ruv = m.process_wire_yuv(py, puv, out="nv12", out_planes=(qy, quv))
    assert ry.data_ptr() == qy.data_ptr() and torch.equal(qy, oy) and torch.equal(quv, ouv)
    with pytest.raises(ValueError, match="there is no YUV surface path"):  # process_yuv keeps its contract
        m.process_yuv(y, uv)


def test_process_wire_yuv_p010_and_planar(dev, ops):
    from hdrnet_amd import yuv
    m = _model(dev)
    planar, semi = pyc.picture(np.random.default_rng(67), SHAPE, 10)
    y, uv = device_planes(semi, 0, dev)
    k = T(yuv.yuv_coefficients("bt2020", True, 10)[0], dev)
    k_out = T(yuv.yuv_encode_coefficients("bt2020", True, 10), dev)
    oy, ouv = m.process_wire_yuv(y, uv, standard="bt2020", full_range=True, bits=10, out="p010")
    assert ops.last_kernel() == "apply_fwd_io/p016->p016+nnguide+upadd"
    hy, huv = _by_hand(m, (y, uv), k, False, out="p010", from_rgb=k_out)
    assert oy.dtype == torch.uint16 and torch.equal(oy.view(torch.int16), hy.view(torch.int16))
    assert torch.equal(ouv.view(torch.int16), huv.view(torch.int16))
    ny, nuv = N(oy), N(ouv)
    assert not (ny & 63).any() and not (nuv & 63).any()  # 10-bit codes in the high bits
    assert len(np.unique(ny)) > 8 and len(np.unique(nuv)) > 8
    want = m.process(ops.yuv_to_rgb(y, uv, k))
    got = m.process_wire_yuv(y, uv, standard="bt2020", full_range=True, bits=10)
    np.testing.assert_allclose(N(got), N(want), rtol=5e-5, atol=5e-5)
    # I420 -> planar
    planar8, semi8 = pyc.picture(np.random.default_rng(71), SHAPE, 8)
    p = device_planes(planar8, 0, dev)
    k8 = T(yuv.yuv_coefficients("bt709", False, 8, msb_aligned=False)[0], dev)
    k8_out = T(yuv.yuv_encode_coefficients("bt709", False, 8), dev)
    out = m.process_wire_yuv_planar(*p, out="planar")
    assert ops.last_kernel() == "apply_fwd_io/i420->i420+nnguide+upadd"
    hand = _by_hand(m, p, k8, True, out="planar", from_rgb=k8_out, out_bits=8)
    assert len(out) == 3 and all(torch.equal(a, b) for a, b in zip(out, hand))
    assert [tuple(t.shape) for t in out] == [SHAPE, (1, 136, 240), (1, 136, 240)]
    assert all(len(torch.unique(t)) > 8 for t in out)
    # ... the planes of process_wire_yuv on the interleaved surface
    sy, suv = m.process_wire_yuv(*device_planes(semi8, 0, dev), out="nv12")
    assert torch.equal(sy, out[0]) and torch.equal(suv[:, :, 0::2], out[1]) and torch.equal(suv[:, :, 1::2], out[2])
    f = m.process_wire_yuv_planar(*p)
    assert ops.last_kernel() == "apply_fwd_io/i420->f32+nnguide+upadd"
    np.testing.assert_allclose(N(f), N(m.process(ops.yuv_planar_to_rgb(*p, k8))), rtol=5e-5, atol=5e-5)
    _check_quantised(m.process_wire_yuv_planar(*p, out_dtype=torch.uint8), f, "i420 -> u8")


# ---- 8. replay ---------------------------------------------------------------------------------------------------------
def test_yuv_frame_inference_replays_the_pyramid(dev, ops):
    from hdrnet_amd.runtime import YuvFrameInference
    m = _model(dev)
    rng = np.random.default_rng(73)
    (y1, uv1), (y2, uv2), (y3, uv3) = (device_planes(pyc.picture(rng, SHAPE, 8)[1], 0, dev) for _ in range(3))
    want1 = m.process_wire_yuv(y1, uv1, out="nv12")
    fi = YuvFrameInference(m, y1, uv1, out="nv12")
    got = fi(y2, uv2)
    assert all(torch.equal(a, b) for a, b in zip(got, m.process_wire_yuv(y2, uv2, out="nv12")))
    assert not torch.equal(got[0], want1[0])  # two pictures
    # the static planes overwritten in place, as a decoder writes into them
    fi.static_inputs[0].copy_(y3)
    fi.static_inputs[1].copy_(uv3)
    got = fi(*fi.static_inputs)
    assert all(torch.equal(a, b) for a, b in zip(got, m.process_wire_yuv(y3, uv3, out="nv12")))
    assert all(torch.equal(a, b) for a, b in zip(fi(y1, uv1), want1))


def test_planar_yuv_frame_inference_replays_the_pyramid(dev, ops):
    from hdrnet_amd.runtime import PlanarYuvFrameInference
    m = _model(dev)
    rng = np.random.default_rng(79)
    p1, p2, p3 = (device_planes(pyc.picture(rng, SHAPE, 8)[0], 0, dev) for _ in range(3))
    fi = PlanarYuvFrameInference(m, *p1, out="planar")
    got = fi(*p2)
    assert all(torch.equal(a, b) for a, b in zip(got, m.process_wire_yuv_planar(*p2, out="planar")))
    for dst, src in zip(fi.static_inputs, p3):
        dst.copy_(src)
    got = fi(*fi.static_inputs)
    assert all(torch.equal(a, b) for a, b in zip(got, m.process_wire_yuv_planar(*p3, out="planar")))
    assert not torch.equal(got[0], m.process_wire_yuv_planar(*p2, out="planar")[0])


def test_yuv_frame_inference_on_a_single_level_model_is_process_yuv(dev, ops):
    """The dispatch did not move the other models: they have no process_wire_yuv."""
    from hdrnet_amd.runtime import YuvFrameInference
    m = _model(dev, "HDRNetPointwiseNNGuide")
    rng = np.random.default_rng(83)
    (y1, uv1), (y2, uv2) = (device_planes(pyc.picture(rng, SHAPE, 8)[1], 0, dev) for _ in range(2))
    fi = YuvFrameInference(m, y1, uv1, out="nv12")
    got = fi(y2, uv2)
    want = m.process_yuv(y2, uv2, out="nv12")
    assert ops.last_kernel() == "apply_fwd_io/nv12->nv12+nnguide"
    assert all(torch.equal(a, b) for a, b in zip(got, want))
