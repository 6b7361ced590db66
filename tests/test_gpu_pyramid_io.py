"""The pyramid model's wire formats on the GPU (include/hdrnet_amd_pyramid_io.h): the resize that reads uint8 / uint16, the
finest level's slice-apply + up-add with both conversions in registers, HDRNetGaussianPyrNN.process_wire and its replay
from a hipGraph.  Oracles: oracle.resize_bilinear_align_corners, oracle.pointwise_nn_guide and port.bilateral_slice_apply
in float32 numpy on ``raw.astype(f32) / f32(white_level)``; tolerances are those of tests/test_gpu_parity.py and
tests/test_models.py.  The C ABI is called directly where the output has to sit inside a poisoned buffer."""
import numpy as np
import pytest
import torch

import pyramid_io_cases as pc

pytestmark = pytest.mark.gpu

GUARD = 64  # elements on either side of an output


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
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)
    return torch.from_numpy(a).to(dev)


def N(t):
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.detach().cpu().numpy()


def poisoned(shape, dtype, dev):
    """(buffer, view of its middle): the output of a direct C-ABI call, NaN (0xA5 for uint8) all around and inside."""
    n = int(np.prod(shape))
    fill = float("nan") if dtype == torch.float32 else 0xA5
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def guards_intact(buf, dtype):
    lo, hi = buf[:GUARD], buf[-GUARD:]
    if dtype == torch.float32:  # bitwise: the NaN that was written
        want = torch.full((GUARD,), float("nan"), dtype=dtype, device=buf.device).view(torch.int32)
        return torch.equal(lo.view(torch.int32), want) and torch.equal(hi.view(torch.int32), want)
    return bool((lo == 0xA5).all()) and bool((hi == 0xA5).all())


def stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


CODE = {"float32": 0, "uint8": 1, "uint16": 2}
SHORT = {"float32": "f32", "uint8": "u8", "uint16": "u16"}


# ---- resize ------------------------------------------------------------------------------------------------------------
RESIZE_CASES = [
    ("uint8", 255.0, (2, 37, 53, 18, 26)),       # a row of 159 bytes: every row-start alignment
    ("uint8", 255.0, (1, 64, 96, 32, 48)),       # the pyramid's 2:1
    ("uint16", 65535.0, (1, 64, 96, 32, 48)),
    ("uint8", 255.0, (1, 9, 13, 1, 1)),          # a single output pixel
    ("uint16", 65535.0, (1, 9, 13, 1, 1)),
    ("uint8", 255.0, (1, 20, 30, 20, 30)),       # identity extents
    ("uint16", 65535.0, (1, 20, 30, 20, 30)),
    ("uint16", 65535.0, (1, 5, 3841, 3, 1920)),  # an odd width: rows start at even bytes that are no dword boundary
    ("uint16", 32767.0, (1, 64, 96, 32, 48)),    # the HDR+ white level
]


@pytest.mark.parametrize("in_dtype,wl,case", RESIZE_CASES,
                         ids=["%s-%g-%s" % (d, w, "x".join(map(str, c))) for d, w, c in RESIZE_CASES])
def test_resize_io_matches_oracle(dev, ops, in_dtype, wl, case):
    import oracle
    from hdrnet_amd import _lib
    B, Hin, Win, Hout, Wout = case
    rng = np.random.default_rng(sum(case) + int(wl))
    hi = 256 if in_dtype == "uint8" else int(wl) + 1
    raw = rng.integers(0, hi, (B, Hin, Win, 3)).astype(in_dtype)
    raw[0, 0, 0, :] = hi - 1  # the white level itself and zero are present
    raw[0, -1, -1, :] = 0
    xf = (raw.astype(np.float32) / np.float32(wl)).astype(np.float32)
    want = oracle.resize_bilinear_align_corners(xf, Hout, Wout)
    t = T(raw, dev)
    buf, out = poisoned((B, Hout, Wout, 3), torch.float32, dev)
    rc = _lib.load().hdrnet_resize_bilinear_io(t.data_ptr(), CODE[in_dtype], wl, out.data_ptr(), B, Hin, Win, Hout, Wout, 3,
                                               stream(dev))
    assert rc == 0, _lib.last_error()
    assert ops.last_kernel() == "resize_bilinear_io/" + SHORT[in_dtype]
    got = N(out)
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-7)  # the existing resize bar
    assert guards_intact(buf, torch.float32)
    via_ops = ops.resize_bilinear_io(t, Hout, Wout, white_level=wl)
    assert torch.equal(via_ops, out)
    f32 = ops.resize_bilinear(T(xf, dev), Hout, Wout)
    print(f"vs resize_bilinear of the float tensor: bit-equal {torch.equal(f32, out)}, "
          f"max |diff| {float((f32 - out).abs().max()):.3e}")


def test_resize_io_f32_is_the_float_kernel(dev, ops):
    x = torch.rand((1, 20, 30, 3), device=dev)
    got = ops.resize_bilinear_io(x, 9, 14)
    assert ops.last_kernel() == "resize_bilinear_io/f32"
    assert torch.equal(got, ops.resize_bilinear(x, 9, 14))
    assert torch.equal(ops.resize_bilinear_io(x, 9, 14, white_level=7.0), got)  # float32 is never scaled


def test_resize_io_refuses_on_the_device(dev, ops):
    from hdrnet_amd import _lib
    with pytest.raises(ValueError, match="C = 3"):
        ops.resize_bilinear_io(torch.zeros((1, 8, 8, 4), dtype=torch.uint8, device=dev), 4, 4)
    t = torch.zeros(1 * 8 * 8 * 3 + 4, dtype=torch.uint8, device=dev)
    out = torch.zeros((1, 4, 4, 3), device=dev)
    rc = _lib.load().hdrnet_resize_bilinear_io(t.data_ptr() + 1, 1, 255.0, out.data_ptr(), 1, 8, 8, 4, 4, 3, stream(dev))
    assert rc == 1 and "4-B aligned" in _lib.last_error()


# ---- slice-apply + up-add ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nn", [False, True], ids=["map", "nnguide"])
@pytest.mark.parametrize("out_dtype", ["float32", "uint8"])
@pytest.mark.parametrize("fmt", pc.FORMATS, ids=["%s-%g" % f for f in pc.FORMATS])
@pytest.mark.parametrize("shape", pc.SHAPES, ids=["x".join(map(str, s)) for s in pc.SHAPES])
def test_upadd_io_matches_composed_oracle(dev, ops, shape, fmt, out_dtype, nn):
    from hdrnet_amd import _lib
    B, H, W, Hc, Wc = shape
    in_dtype, wl = fmt
    c = pc.inputs(shape, fmt, nn)
    want_f = pc.want_f32(shape, fmt, nn)
    grid, t_in, coarse = T(c["grid"], dev), T(c["raw"], dev), T(c["coarse"], dev)
    guide = None if nn else T(c["guide"], dev)
    c1, c2 = (T(c["conv1"], dev), T(c["conv2"], dev)) if nn else (None, None)
    odt = getattr(torch, out_dtype)
    buf, out = poisoned((B, H, W, 3), odt, dev)
    rc = _lib.load().hdrnet_bilateral_slice_apply_upadd_io_ex(
        grid.data_ptr(), None if nn else guide.data_ptr(), t_in.data_ptr(), coarse.data_ptr(), Hc, Wc, out.data_ptr(),
        B, H, W, pc.GH, pc.GW, pc.GD, 3, 3, 1, CODE[in_dtype], wl, 1 if out_dtype == "uint8" else 0,
        c1.data_ptr() if nn else None, c2.data_ptr() if nn else None, 16 if nn else 0, 0, stream(dev))
    assert rc == 0, _lib.last_error()
    kernel = ops.last_kernel()
    kw = dict(guide_conv1=c1, guide_conv2=c2) if nn else dict(guide=guide)
    if in_dtype == "float32" and out_dtype == "float32":
        ref = ops.bilateral_slice_apply_upadd(grid, t_in, coarse, **kw)  # the float op: its kernel, its bits
        assert kernel == ops.last_kernel() == "apply_fwd_seg/vec4" + ("+nnguide" if nn else "") + "+upadd"
        assert torch.equal(out, ref)
    else:
        assert kernel == f"apply_fwd_io/{SHORT[in_dtype]}->{SHORT[out_dtype]}{'+nnguide' if nn else ''}+upadd"
    assert guards_intact(buf, odt)
    via_ops = ops.bilateral_slice_apply_upadd_io(grid, t_in, coarse, input_white_level=wl, out_dtype=odt, **kw)
    assert via_ops.dtype == odt and torch.equal(via_ops, out)
    if out_dtype == "float32":
        np.testing.assert_allclose(N(out), want_f, rtol=pc.TOL, atol=pc.TOL)
    else:
        pc.check_u8(N(out), want_f, f"{shape} {fmt} nn={nn}")


def test_upadd_io_default_white_levels_and_flags(dev, ops):
    """255 / 65535 by default; fast_sigmoid and prescaled reach the kernel as in bilateral_slice_apply_io: the prescaled
    network is the exported one bit for bit, the fast sigmoid stays within the forward's bar of the exact one."""
    shape = pc.SHAPES[0]
    for fmt in pc.FORMATS[:2]:
        c = pc.inputs(shape, fmt, True)
        grid, t_in, coarse = T(c["grid"], dev), T(c["raw"], dev), T(c["coarse"], dev)
        c1, c2 = T(c["conv1"], dev), T(c["conv2"], dev)
        base = ops.bilateral_slice_apply_upadd_io(grid, t_in, coarse, guide_conv1=c1, guide_conv2=c2, input_white_level=fmt[1])
        assert torch.equal(ops.bilateral_slice_apply_upadd_io(grid, t_in, coarse, guide_conv1=c1, guide_conv2=c2), base)
        p1, p2 = ops.guide_nn_prescale(c1, c2)
        pre = ops.bilateral_slice_apply_upadd_io(grid, t_in, coarse, guide_conv1=p1, guide_conv2=p2, prescaled=True)
        assert torch.equal(pre, base)
        fast = ops.bilateral_slice_apply_upadd_io(grid, t_in, coarse, guide_conv1=c1, guide_conv2=c2, fast_sigmoid=True)
        np.testing.assert_allclose(N(fast), N(base), rtol=pc.TOL, atol=pc.TOL)


def test_upadd_io_refuses_on_the_device(dev, ops):
    g = torch.rand((1, 8, 8, 4, 12), device=dev)
    x = torch.zeros((1, 8, 10, 3), dtype=torch.uint8, device=dev)  # W % 4 != 0
    with pytest.raises(ValueError, match="W % 4 == 0"):
        ops.bilateral_slice_apply_upadd_io(g, x, torch.rand((1, 4, 5, 3), device=dev), guide=torch.rand((1, 8, 10), device=dev))


# ---- the model ---------------------------------------------------------------------------------------------------------
def _model(dev, seed=7):
    from hdrnet_amd import models
    torch.manual_seed(seed)
    return models.HDRNetGaussianPyrNN(dict(batch_norm=False)).to(dev).eval()


def _frames(rng, dtype, shape, hi):
    """smooth ramps + noise, so that the low-res input and the guide see a picture rather than white noise"""
    B, H, W, _ = shape
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([xx / W, yy / H, (xx + yy) / (W + H)], -1)[None] * (0.6 + 0.4 * rng.random((B, 1, 1, 3)))
    v = np.clip(base + 0.1 * rng.standard_normal((B, H, W, 3)), 0, 1)
    return np.round(v * hi).astype(dtype)


def _wire_by_hand(m, t, wl, out_dtype):
    """process_wire's launches, spelled out with the ops."""
    from hdrnet_amd import data, hdrnet_ops as ops
    H, W = t.shape[1:3]
    with torch.no_grad():
        low = data.lowres_input(t, m.params["net_input_size"], wl)
        grids = m.coefficients.levels(low)
        l1 = ops.resize_bilinear_io(t, H // 2, W // 2, wl)
        l2 = ops.resize_bilinear(l1, H // 4, W // 4)
        gp = [g.inference_params(m.prescale_guide) for g in m.guide]
        kw = dict(has_offset=True, fast_sigmoid=m.fast_sigmoid)
        cur = ops.bilateral_slice_apply_nnguide(grids[0], l2, gp[2][0], gp[2][1], prescaled=gp[2][2], **kw)
        cur = ops.bilateral_slice_apply_upadd(grids[1], l1, cur, guide_conv1=gp[1][0], guide_conv2=gp[1][1],
                                              prescaled=gp[1][2], **kw)
        return ops.bilateral_slice_apply_upadd_io(grids[2], t, cur, guide_conv1=gp[0][0], guide_conv2=gp[0][1],
                                                  input_white_level=wl, out_dtype=out_dtype, prescaled=gp[0][2], **kw)


def _check_quantised(got_u8, float_out, what):
    want = (255 * float_out.clamp(0, 1)).to(torch.uint8)
    diff = (got_u8.to(torch.int16) - want.to(torch.int16)).abs()
    share = float((diff > 0).float().mean())
    print(f"{what}: vs the quantised float path max LSB {int(diff.max())}, share differing {share:.2e}")
    assert int(diff.max()) <= 1 and share < 5e-4
    assert len(torch.unique(got_u8)) > 8  # a picture, not a constant


@pytest.mark.parametrize("shape", [(1, 272, 480, 3), (2, 144, 256, 3)], ids=["272x480", "2x144x256"])
def test_process_wire_matches_the_float_path(dev, ops, shape):
    m = _model(dev)
    rng = np.random.default_rng(31 + shape[0])
    frame = _frames(rng, np.uint8, shape, 255)
    t = T(frame, dev)
    as_float = T(frame.astype(np.float32) / np.float32(255), dev)
    want = m.process(as_float)
    # uint8 in, float32 out: test_pyramid_model_fused_matches_composed's bar
    got = m.process_wire(t)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    assert ops.last_kernel() == "apply_fwd_io/u8->f32+nnguide+upadd"
    np.testing.assert_allclose(N(got), N(want), rtol=5e-5, atol=5e-5)
    # uint8 out: the io op by hand on the intermediate levels, and the quantised float path
    got8 = m.process_wire(t, out_dtype=torch.uint8)
    assert got8.dtype == torch.uint8 and tuple(got8.shape) == shape
    assert ops.last_kernel() == "apply_fwd_io/u8->u8+nnguide+upadd"
    assert torch.equal(got8, _wire_by_hand(m, t, None, torch.uint8))
    _check_quantised(got8, want, f"{shape} u8 -> u8")
    # uint16 / 32767 in
    f16 = _frames(rng, np.uint16, shape, 32767)
    t16 = T(f16, dev)
    want16 = m.process(T(f16.astype(np.float32) / np.float32(32767), dev))
    got16 = m.process_wire(t16, white_level=32767.0)
    assert ops.last_kernel() == "apply_fwd_io/u16->f32+nnguide+upadd"
    np.testing.assert_allclose(N(got16), N(want16), rtol=5e-5, atol=5e-5)
    assert torch.equal(got16, _wire_by_hand(m, t16, 32767.0, torch.float32))
    _check_quantised(m.process_wire(t16, out_dtype=torch.uint8, white_level=32767.0), want16, f"{shape} u16 -> u8")
    # float32 both ways is process() itself; process() keeps its contract
    assert torch.equal(m.process_wire(as_float), want)
    with pytest.raises(TypeError, match="float32"):
        m.process(t)
    with pytest.raises(TypeError, match="float32 frames only"):
        m.process(as_float, out_dtype=torch.uint8)


def test_frame_inference_replays_process_wire(dev, ops):
    from hdrnet_amd.runtime import FrameInference
    m = _model(dev)
    rng = np.random.default_rng(41)
    shape = (1, 272, 480, 3)
    first, second = (T(_frames(rng, np.uint8, shape, 255), dev) for _ in range(2))
    want_first = m.process_wire(first, out_dtype=torch.uint8)
    fi = FrameInference(m, first, out_dtype=torch.uint8)
    got = fi(second)
    assert got.dtype == torch.uint8
    assert torch.equal(got, m.process_wire(second, out_dtype=torch.uint8))
    assert torch.equal(fi(first), want_first)
    assert not torch.equal(fi(second), want_first)  # two pictures
