"""The ops at the ends of the extents the C ABI admits (tests/extent_cases.py states the shapes and the reason for each;
tests/row_plan.py predicts the kernel each one reaches):

* wide rows, W = 2^23 + 8 and 2^24 + 64: beyond the width at which the four-pixel kernels and the gradient pass form a
  pixel's coordinate exactly (row_geom.h: kMaxFloatX), so the scalar row kernel, the slice row kernel and the generic
  gradients take them and the fused forwards refuse by name;
* tall and deep frames, H or B = 65535 | 65536: the last launch of the segment family's 3-D grid and the first of the row
  family's 1-D grid; the gradient pass at nyg = 65535 | 65536 row groups;
* far offsets: one call per kernel family on a batch whose last image lies wholly beyond byte 2^31 (2^32 for the slice
  forward) of the widest tensor, image b a copy of base image b % 3.

References: oracle.port() and the composed oracles of tests/test_gpu_fused_fullsize.py.  Bars, unchanged: forward 1e-5,
check_pixel_grad / check_dgrid (tests/conftest.py), the uint8 rule of pyramid_io_cases.check_u8; the generic kernels equal
the port bit for bit.  Outputs of the direct C-ABI calls are pre-filled with NaN (float) or 0x00 and 0xFF (uint8): an
element no kernel writes cannot pass.  Every test frees its tensors and empties the allocator's cache before it returns
(the far-offset cases hold up to 7.9 GB)."""
import gc
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
import extent_cases as ec  # noqa: E402
import row_plan as rp  # noqa: E402
from conftest import GRAD_RTOL, check_dgrid, check_pixel_grad  # noqa: E402
from pyramid_io_cases import check_u8  # noqa: E402

FWD_TOL = 1e-5
NN_GUIDE_TOL = 1e-6
GRAD_SUBSETS = ((True, True), (True, False), (False, True), (False, False))  # (dguide, dinput) beside dgrid
_CODE = {torch.float32: 0, torch.uint8: 1, torch.uint16: 2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
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


@pytest.fixture(autouse=True)
def release():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def T16(raw, dev):
    return torch.from_numpy(raw.astype(np.int32)).to(dev).to(torch.uint16)


def _p(t):
    return None if t is None else t.data_ptr()


def _stream(t):
    return torch.cuda.current_stream(t.device).cuda_stream


def nan(shape, dev):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def no_nan(name, *ts):
    """(counted over the leading dimension in chunks: a mask of a far-offset batch would be another 0.5 GB)"""
    n = sum(int(torch.isnan(t[a:a + ec.FAR_CHUNK]).sum()) for t in ts if t is not None
            for a in range(0, t.shape[0], ec.FAR_CHUNK))
    print(f"{name}: NaN left in the poisoned outputs: {n}")
    assert n == 0, name


def close_dev(name, got, want, rtol=FWD_TOL, atol=FWD_TOL):
    """|got - want| <= atol + rtol |want| elementwise, on the device (the arrays are up to 1.6 GB); prints the worst."""
    want = want if isinstance(want, torch.Tensor) else T(want, got.device)
    err = (got - want).abs()
    worst = float((err / (atol + rtol * want.abs())).max())
    print(f"{name}: max|err| = {float(err.max()):.3e}, worst / (atol {atol:g} + rtol {rtol:g} |want|) = {worst:.3f}")
    assert worst <= 1.0 and not bool(torch.isnan(err).any()), name


def last_error():
    from hdrnet_amd import _lib
    return _lib.last_error()


# ---- the C-ABI entry points with caller-owned outputs: the return code, nothing raised --------------------------------
def dims(grid, x):
    B, H, W = x.shape[:3]
    GH, GW, GD, C = grid.shape[1:]
    return B, H, W, GH, GW, GD


def abi_apply(lib, grid, guide, x, out, flags=0):
    with torch.cuda.device(x.device):
        return lib.hdrnet_bilateral_slice_apply_f32_ex(grid.data_ptr(), guide.data_ptr(), x.data_ptr(), out.data_ptr(),
                                                       *dims(grid, x), 3, 3, 1, flags, _stream(x))


def abi_slice(lib, grid, guide, out):
    B, H, W = guide.shape
    GH, GW, GD, C = grid.shape[1:]
    with torch.cuda.device(guide.device):
        return lib.hdrnet_bilateral_slice_f32_ex(grid.data_ptr(), guide.data_ptr(), out.data_ptr(), B, H, W, GH, GW, GD, C, 0,
                                                 _stream(guide))


def abi_grad(lib, grid, guide, x, dout, dgrid, dguide, dinput):
    d = dims(grid, x)
    with torch.cuda.device(x.device):
        wbytes = lib.hdrnet_bilateral_slice_apply_grad_workspace_bytes(*d, 3, 3, 1) if dgrid is not None else 0
        ws = torch.empty((wbytes,), dtype=torch.uint8, device=x.device) if wbytes else None
        rc = lib.hdrnet_bilateral_slice_apply_grad_f32_ex(grid.data_ptr(), guide.data_ptr(), x.data_ptr(), dout.data_ptr(),
                                                          _p(dgrid), _p(dguide), _p(dinput), *d, 3, 3, 1, _p(ws), wbytes, 0,
                                                          _stream(x))
        torch.cuda.synchronize()
    return rc


def abi_nnguide(lib, grid, x, c1, c2, out, gout):
    with torch.cuda.device(x.device):
        return lib.hdrnet_bilateral_slice_apply_nnguide_f32_ex(grid.data_ptr(), x.data_ptr(), c1.data_ptr(), c2.data_ptr(),
                                                               out.data_ptr(), _p(gout), *dims(grid, x), 3, 3, 1, c1.shape[0], 0,
                                                               _stream(x))


def abi_io(lib, grid, x, out, white, guide=None, c1=None, c2=None):
    with torch.cuda.device(x.device):
        return lib.hdrnet_bilateral_slice_apply_io_ex(grid.data_ptr(), _p(guide), x.data_ptr(), out.data_ptr(), *dims(grid, x),
                                                      3, 3, 1, _CODE[x.dtype], float(white), _CODE[out.dtype], _p(c1), _p(c2),
                                                      0 if c1 is None else c1.shape[0], None, 0, _stream(x))


def abi_upadd(lib, grid, x, coarse, out, guide=None, c1=None, c2=None):
    with torch.cuda.device(x.device):
        return lib.hdrnet_bilateral_slice_apply_upadd_f32_ex(grid.data_ptr(), _p(guide), x.data_ptr(), coarse.data_ptr(),
                                                             coarse.shape[1], coarse.shape[2], out.data_ptr(), *dims(grid, x),
                                                             3, 3, 1, _p(c1), _p(c2), 0 if c1 is None else c1.shape[0], 0,
                                                             _stream(x))


def abi_upadd_io(lib, grid, x, coarse, out, white, guide):
    with torch.cuda.device(x.device):
        return lib.hdrnet_bilateral_slice_apply_upadd_io_ex(grid.data_ptr(), _p(guide), x.data_ptr(), coarse.data_ptr(),
                                                            coarse.shape[1], coarse.shape[2], out.data_ptr(), *dims(grid, x),
                                                            3, 3, 1, _CODE[x.dtype], float(white), _CODE[out.dtype], None, None,
                                                            0, 0, _stream(x))


def abi_resize(lib, x, out):
    B, Hin, Win, C = x.shape
    with torch.cuda.device(x.device):
        return lib.hdrnet_resize_bilinear_f32(x.data_ptr(), out.data_ptr(), B, Hin, Win, out.shape[1], out.shape[2], C,
                                              _stream(x))


def ok(rc, what):
    from hdrnet_amd import _lib
    _lib.check(rc, what)
    torch.cuda.synchronize()


def refused(rc, out, fill, B, H, W, word, what):
    """rc = 1, the poisoned output untouched, the text names the limit that binds."""
    torch.cuda.synchronize()
    err = last_error()
    print(f"{what}: rc = {rc}, {err!r}")
    assert rc == 1, (what, rc, err)
    untouched = bool(torch.isnan(out).all()) if out.dtype == torch.float32 else bool((out == fill).all())
    assert untouched, what + ": a refused call wrote to its output"
    assert word in err and f"(B={B}, H={H}, W={W})" in err, (what, err)


# ---- data -------------------------------------------------------------------------------------------------------------
def near_identity_grid(rng, B, GH, GW, GD):
    """An affine close to the identity (test_wire_format_forward): the output spans [0, 1] and beyond."""
    g6 = np.zeros((B, GH, GW, GD, 3, 4), np.float32)
    for i in range(3):
        g6[..., i, i] = 1.0
    return (g6 + 0.15 * rng.standard_normal(g6.shape)).astype(np.float32).reshape(B, GH, GW, GD, 12)


def nn_params(rng, n=16):
    return (rng.standard_normal((n, 4)) * 0.8).astype(np.float32), (rng.standard_normal(n + 1) * 0.5).astype(np.float32)


class Case:
    """The float operands of one shape and, on demand and once, what the oracle makes of them."""

    def __init__(self, port, B, H, W, GH, GW, GD, seed):
        rng = np.random.default_rng(seed)
        self.port, self.shape = port, (B, H, W, GH, GW, GD)
        self.grid = near_identity_grid(rng, B, GH, GW, GD)
        self.guide = (rng.random((B, H, W), dtype=np.float32) * 1.04 - 0.02).astype(np.float32)
        self.x = rng.random((B, H, W, 3), dtype=np.float32)
        self.rng = rng
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    @property
    def dout(self):
        return self.memo("dout", lambda: self.rng.standard_normal(self.x.shape).astype(np.float32))

    def want(self):
        return self.memo("want", lambda: self.port.bilateral_slice_apply(self.grid, self.guide, self.x, True))

    def grads(self):
        return self.memo("grads", lambda: dict(zip(
            ("dgrid", "dguide", "dinput"), self.port.bilateral_slice_apply_grad(self.grid, self.guide, self.x, self.dout, True))))


_CASE = {}


def case_for(port, shape, seed):
    """One shape's data at a time: the wide rows hold up to 2 GB of host arrays each."""
    if _CASE.get("shape") != shape:
        _CASE.clear()
        _CASE.update(shape=shape, case=Case(port, *shape, seed))
    return _CASE["case"]


@pytest.fixture(scope="module", autouse=True)
def drop_cases():
    yield
    _CASE.clear()


def run_forward(ops, lib, dev, c, tag):
    """Auto dispatch into a NaN-filled output against the port at 1e-5 with the predicted kernel; the generic kernel
    bit-equal to the port."""
    B, H, W, GH, GW, GD = c.shape
    grid, guide, x = T(c.grid, dev), T(c.guide, dev), T(c.x, dev)
    want = T(c.want(), dev)
    out = nan((B, H, W, 3), dev)
    ok(abi_apply(lib, grid, guide, x, out), tag)
    assert ops.last_kernel() == rp.forward_kernel(B, H, W, GW, GD), (tag, ops.last_kernel())
    no_nan(tag, out)
    close_dev(f"{tag} forward ({ops.last_kernel()})", out, want)
    out.fill_(float("nan"))
    ok(abi_apply(lib, grid, guide, x, out, flags=1), tag + " generic")  # HDRNET_KERNEL_GENERIC
    assert ops.last_kernel() == "apply_fwd_generic", ops.last_kernel()
    n_diff = int((out != want).sum())
    print(f"{tag} generic kernel: elements that differ from the port: {n_diff}")
    assert n_diff == 0 and torch.equal(out, want), tag + ": the generic kernel is not bit-equal to the port"


def run_slice(ops, lib, dev, port, c, tag, C=ec.WIDE_SLICE_C):
    B, H, W, GH, GW, GD = c.shape
    sgrid = c.grid if C == 12 else c.grid[..., :C]
    want = port.bilateral_slice(np.ascontiguousarray(sgrid), c.guide)
    out = nan((B, H, W, C), dev)
    ok(abi_slice(lib, T(sgrid, dev), T(c.guide, dev), out), tag)
    assert ops.last_kernel() == rp.slice_kernel(B, H, W, GW, GD, C), (tag, ops.last_kernel())
    no_nan(tag, out)
    close_dev(f"{tag} slice C = {C} ({ops.last_kernel()})", out, want)


def run_grads(ops, lib, dev, c, need_guide, need_input, tag):
    B, H, W, GH, GW, GD = c.shape
    want = c.grads()
    grid, guide, x, dout = T(c.grid, dev), T(c.guide, dev), T(c.x, dev), T(c.dout, dev)
    dgrid = nan(tuple(grid.shape), dev)
    dguide = nan(tuple(guide.shape), dev) if need_guide else None
    dinput = nan(tuple(x.shape), dev) if need_input else None
    ok(abi_grad(lib, grid, guide, x, dout, dgrid, dguide, dinput), tag)
    kern = ops.last_kernel()
    assert kern == rp.grad_kernels(B, H, W, GH, GW, GD, need_guide, need_input), (tag, kern)
    tag = f"{tag} (dguide={need_guide}, dinput={need_input}; {kern})"
    no_nan(tag, dgrid, dguide, dinput)
    check_dgrid(N(dgrid), want["dgrid"], tag)
    if need_guide:
        check_pixel_grad(N(dguide), want["dguide"], tag, "dguide")
    if need_input:
        check_pixel_grad(N(dinput), want["dinput"], tag, "dinput")


# ---- 1. wide rows -----------------------------------------------------------------------------------------------------
WIDE_IDS = [f"{H}x{W}" for H, W in ec.WIDE]


def wide_case(port, H, W):
    return case_for(port, (1, H, W) + ec.WIDE_GRID, seed=H * 31 + W % 1000)


@pytest.mark.parametrize("H,W", ec.WIDE + [ec.WIDE_SCALAR_NEIGHBOUR], ids=WIDE_IDS + ["1x(2^23+9)"])
def test_wide_row_forward(dev, ops, lib, port16, H, W):
    """A row wider than 2^23 pixels takes the scalar row kernel, which forms every pixel's centre as the reference does
    ((float)x + 0.5f); the four-pixel kernels' xf0 + k rounds differently from x = 2^23 on."""
    c = wide_case(port16, H, W)
    run_forward(ops, lib, dev, c, f"wide {H} x {W}")


@pytest.mark.parametrize("H,W", ec.WIDE, ids=WIDE_IDS)
def test_wide_row_slice_forward(dev, ops, lib, port16, H, W):
    c = wide_case(port16, H, W)
    run_slice(ops, lib, dev, port16, c, f"wide {H} x {W}")


@pytest.mark.parametrize("need_guide,need_input", GRAD_SUBSETS)
@pytest.mark.parametrize("H,W", ec.WIDE, ids=WIDE_IDS)
def test_wide_row_gradients(dev, ops, lib, port16, H, W, need_guide, need_input):
    """Every gradient subset of test_batched_backward_vs_oracle_every_gradient_subset.  gg_plan refuses a row wider than
    2^23 pixels (its 24-bit multiplies and float column intervals), so do the four-pixel per-pixel kernels: the generic
    kernels take all three gradients."""
    c = wide_case(port16, H, W)
    run_grads(ops, lib, dev, c, need_guide, need_input, f"wide {H} x {W}")


# The last admitted width: one row of exactly 2^23 pixels stays on the four-pixel kernels and the MFMA gradient pass.
LAST_WIDE = (1, 1, ec.WIDE_SIDES[0]) + ec.WIDE_GRID


def test_widest_admitted_row_forwards(dev, ops, lib, port16):
    """W = 2^23 (8192 segments, every lane's xf0 + k still exact): apply_fwd_seg/vec4, its guide-network flavour and
    the wire-format forwards (u16 -> f32 and u8 -> u8 with a guide map), each under its own kernel name at the
    forward's bar; the generic kernel bit-equal to the port."""
    B, H, W, GH, GW, GD = LAST_WIDE
    c = case_for(port16, LAST_WIDE, seed=23)
    assert rp.forward_kernel(B, H, W, GW, GD) == "apply_fwd_seg/vec4" and rp.seg_reaches(B, H, W, GW, GD, io=True)
    run_forward(ops, lib, dev, c, f"widest {H} x {W}")
    grid, x, guide = T(c.grid, dev), T(c.x, dev), T(c.guide, dev)
    c1n, c2n = nn_params(c.rng)
    guide_nn = oracle.pointwise_nn_guide(c.x, c1n, c2n)
    out, gout = nan((B, H, W, 3), dev), nan((B, H, W), dev)
    ok(abi_nnguide(lib, grid, x, T(c1n, dev), T(c2n, dev), out, gout), "nnguide")
    assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide" == rp.fused_forward_kernel(B, H, W, GW, GD, "nnguide")
    no_nan("widest nnguide", out, gout)
    close_dev("widest nnguide guide", gout, guide_nn, rtol=0, atol=NN_GUIDE_TOL)
    close_dev("widest nnguide out", out, port16.bilateral_slice_apply(c.grid, guide_nn, c.x, True))
    raw16 = c.rng.integers(0, 32768, (B, H, W, 3), dtype=np.uint16)
    out.fill_(float("nan"))
    ok(abi_io(lib, grid, T16(raw16, dev), out, 32767.0, guide=guide), "io u16")
    assert ops.last_kernel().startswith("apply_fwd_io/u16->f32"), ops.last_kernel()
    no_nan("widest io u16 -> f32", out)
    x16 = (raw16.astype(np.float32) / np.float32(32767.0)).astype(np.float32)
    close_dev("widest io u16 -> f32", out, port16.bilateral_slice_apply(c.grid, c.guide, x16, True))
    raw8 = c.rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    outs = [torch.full((B, H, W, 3), f, dtype=torch.uint8, device=dev) for f in (0, 255)]
    for o8 in outs:
        ok(abi_io(lib, grid, T(raw8, dev), o8, 255.0, guide=guide), "io u8")
        assert ops.last_kernel().startswith("apply_fwd_io/u8->u8"), ops.last_kernel()
    assert torch.equal(outs[0], outs[1]), "widest io u8 -> u8: a byte no kernel wrote"
    x8 = (raw8.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    check_u8(N(outs[0]), port16.bilateral_slice_apply(c.grid, c.guide, x8, True), "widest io u8 -> u8")


@pytest.mark.parametrize("with_dgrid", [True, False], ids=["apply_bwd_fused", "apply_vjp_seg"])
def test_widest_admitted_row_gradients(dev, ops, lib, port16, with_dgrid):
    """W = 2^23: all three gradients on the MFMA pass (its 24-bit pixel offsets and float column intervals at their
    last admitted width), and dguide + dinput alone on apply_vjp_seg."""
    B, H, W, GH, GW, GD = LAST_WIDE
    c = case_for(port16, LAST_WIDE, seed=23)
    if with_dgrid:
        assert rp.grad_kernels(B, H, W, GH, GW, GD, True, True) == "apply_bwd_fused/mfma"
        run_grads(ops, lib, dev, c, True, True, f"widest {H} x {W}")
        return
    want = c.grads()
    grid, guide, x, dout = T(c.grid, dev), T(c.guide, dev), T(c.x, dev), T(c.dout, dev)
    dguide, dinput = nan(tuple(guide.shape), dev), nan(tuple(x.shape), dev)
    ok(abi_grad(lib, grid, guide, x, dout, None, dguide, dinput), "vjp")
    assert ops.last_kernel() == "apply_vjp_seg/vec4" == rp.vjp_kernel(B, H, W, GW, GD), ops.last_kernel()
    no_nan("widest vjp_seg", dguide, dinput)
    check_pixel_grad(N(dguide), want["dguide"], "widest apply_vjp_seg", "dguide")
    check_pixel_grad(N(dinput), want["dinput"], "widest apply_vjp_seg", "dinput")


@pytest.mark.parametrize("H,W", ec.WIDE, ids=WIDE_IDS)
def test_wide_row_fused_forwards_refuse_by_name(dev, ops, lib, H, W):
    """bilateral_slice_apply_nnguide, _io (u8 -> u8 and u16 -> f32, guide map and guide network) and _upadd have no kernel
    for a row wider than 2^23 pixels: rc = 1, the poisoned output untouched, the limit named."""
    GH, GW, GD = ec.WIDE_GRID
    rng = np.random.default_rng(W % 977)
    grid = T(near_identity_grid(rng, 1, GH, GW, GD), dev)
    c1, c2 = (T(a, dev) for a in nn_params(rng))
    x = torch.rand((1, H, W, 3), device=dev)
    guide = torch.rand((1, H, W), device=dev)
    coarse = torch.rand((1, 1, 8, 3), device=dev)
    for fam in ("nnguide", "upadd", "nnguide+upadd"):
        assert rp.fused_forward_kernel(1, H, W, GW, GD, fam) is None
    assert not rp.seg_reaches(1, H, W, GW, GD, io=True)
    word = rp.extent_limit(1, H, W, "rows4")
    out = nan((1, H, W, 3), dev)
    refused(abi_nnguide(lib, grid, x, c1, c2, out, None), out, None, 1, H, W, word, "nnguide")
    refused(abi_upadd(lib, grid, x, coarse, out, guide=guide), out, None, 1, H, W, word, "upadd (guide map)")
    refused(abi_upadd(lib, grid, x, coarse, out, c1=c1, c2=c2), out, None, 1, H, W, word, "upadd (guide network)")
    word = rp.extent_limit(1, H, W, "seg")
    x16 = torch.zeros((1, H, W, 3), dtype=torch.uint16, device=dev)
    refused(abi_io(lib, grid, x16, out, 32767.0, guide=guide), out, None, 1, H, W, word, "io u16 -> f32 (guide map)")
    refused(abi_io(lib, grid, x16, out, 32767.0, c1=c1, c2=c2), out, None, 1, H, W, word, "io u16 -> f32 (guide network)")
    del out, x16, x
    x8 = torch.zeros((1, H, W, 3), dtype=torch.uint8, device=dev)
    for fill in (0, 255):
        out8 = torch.full((1, H, W, 3), fill, dtype=torch.uint8, device=dev)
        refused(abi_io(lib, grid, x8, out8, 255.0, guide=guide), out8, fill, 1, H, W, word, "io u8 -> u8 (guide map)")
        refused(abi_io(lib, grid, x8, out8, 255.0, c1=c1, c2=c2), out8, fill, 1, H, W, word, "io u8 -> u8 (guide network)")
        refused(abi_upadd_io(lib, grid, x8, coarse, out8, 255.0, guide), out8, fill, 1, H, W, word, "upadd_io u8 -> u8")


@pytest.mark.parametrize("H,W", ec.WIDE, ids=WIDE_IDS)
def test_wide_row_resize_bilinear(dev, lib, H, W):
    """resize_bilinear has no limit on the width: an output row of W pixels from a quarter as many, against the
    float32 restatement of the TensorFlow resize."""
    rng = np.random.default_rng(W % 911)
    x = rng.random((1, H, W // 4 + 3, 3), dtype=np.float32)
    want = oracle.resize_bilinear_align_corners(x, H, W)
    out = nan((1, H, W, 3), dev)
    ok(abi_resize(lib, T(x, dev), out), "resize")
    no_nan(f"resize to {H} x {W}", out)
    close_dev(f"resize_bilinear to {H} x {W}", out, want)


# ---- 2. tall and deep -------------------------------------------------------------------------------------------------
TALL_DEEP = ec.TALL + ec.DEEP
TALL_DEEP_IDS = ["x".join(str(v) for v in s[:3]) for s in TALL_DEEP]


def small_case(port, shape):
    return case_for(port, shape, seed=sum(shape))


@pytest.mark.parametrize("shape", TALL_DEEP, ids=TALL_DEEP_IDS)
def test_tall_and_deep_forwards(dev, ops, lib, port16, shape):
    """Both sides of kLimBH: at 65535 the segment family's 3-D launch grid, at 65536 the row family's 1-D grid (the plain
    forward, the slice forward, the guide-network and up-add forwards) -- each at the forward's bar with the predicted
    kernel."""
    B, H, W, GH, GW, GD = shape
    c = small_case(port16, shape)
    tag = f"{B} x {H} x {W}"
    run_forward(ops, lib, dev, c, tag)
    run_slice(ops, lib, dev, port16, c, tag)
    grid, x = T(c.grid, dev), T(c.x, dev)
    c1n, c2n = nn_params(c.rng)
    guide_nn = oracle.pointwise_nn_guide(c.x, c1n, c2n)
    want_nn = port16.bilateral_slice_apply(c.grid, guide_nn, c.x, True)
    c1, c2 = T(c1n, dev), T(c2n, dev)
    out, gout = nan((B, H, W, 3), dev), nan((B, H, W), dev)
    ok(abi_nnguide(lib, grid, x, c1, c2, out, gout), tag + " nnguide")
    assert ops.last_kernel() == rp.fused_forward_kernel(B, H, W, GW, GD, "nnguide"), ops.last_kernel()
    no_nan(tag + " nnguide", out, gout)
    close_dev(f"{tag} nnguide guide ({ops.last_kernel()})", gout, guide_nn, rtol=0, atol=NN_GUIDE_TOL)
    close_dev(f"{tag} nnguide out", out, want_nn)
    coarse = c.rng.random((B, max(H // 4, 1), max(W // 2, 2), 3), dtype=np.float32)
    up = oracle.resize_bilinear_align_corners(coarse, H, W)
    for fam, kw, want in (("upadd", dict(guide=T(c.guide, dev)), c.want() + up), ("nnguide+upadd", dict(c1=c1, c2=c2), want_nn + up)):
        out.fill_(float("nan"))
        ok(abi_upadd(lib, grid, x, T(coarse, dev), out, **kw), f"{tag} {fam}")
        assert ops.last_kernel() == rp.fused_forward_kernel(B, H, W, GW, GD, fam), ops.last_kernel()
        no_nan(f"{tag} {fam}", out)
        close_dev(f"{tag} {fam} ({ops.last_kernel()})", out, want.astype(np.float32))
    out.fill_(float("nan"))
    ok(abi_resize(lib, T(coarse, dev), out), tag + " resize")
    no_nan(tag + " resize", out)
    close_dev(f"{tag} resize_bilinear", out, up)


@pytest.mark.parametrize("shape", TALL_DEEP, ids=TALL_DEEP_IDS)
def test_tall_and_deep_wire_formats(dev, ops, lib, port16, shape):
    """The wire-format forwards (u8 -> u8 and u16 -> f32, guide map and guide network; the up-add u8 -> u8) exist on the
    segment family alone: parity at 65535, a refusal that names kLimBH at 65536."""
    B, H, W, GH, GW, GD = shape
    c = small_case(port16, shape)
    tag = f"{B} x {H} x {W}"
    inside = rp.seg_reaches(B, H, W, GW, GD, io=True)
    word = rp.extent_limit(B, H, W, "seg")
    assert inside == (word is None)
    grid, guide = T(c.grid, dev), T(c.guide, dev)
    c1n, c2n = nn_params(c.rng)
    c1, c2 = T(c1n, dev), T(c2n, dev)
    raw8 = c.rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    raw16 = c.rng.integers(0, 32768, (B, H, W, 3), dtype=np.uint16)
    coarse = c.rng.random((B, max(H // 4, 1), max(W // 2, 2), 3), dtype=np.float32)
    for kind, raw, white, t_in in (("u8", raw8, 255.0, T(raw8, dev)), ("u16", raw16, 32767.0, T16(raw16, dev))):
        xf = (raw.astype(np.float32) / np.float32(white)).astype(np.float32)
        for gname, kw in (("guide map", dict(guide=guide)), ("guide network", dict(c1=c1, c2=c2))):
            what = f"{tag} io {kind} ({gname})"
            if not inside:
                outs = [torch.full((B, H, W, 3), f, dtype=torch.uint8, device=dev) for f in (0, 255)] if kind == "u8" \
                    else [nan((B, H, W, 3), dev)]
                for out, fill in zip(outs, (0, 255)):
                    refused(abi_io(lib, grid, t_in, out, white, **kw), out, fill, B, H, W, word, what)
                continue
            g = c.guide if "map" in gname else oracle.pointwise_nn_guide(xf, c1n, c2n)
            want = port16.bilateral_slice_apply(c.grid, g, xf, True)
            if kind == "u16":
                out = nan((B, H, W, 3), dev)
                ok(abi_io(lib, grid, t_in, out, white, **kw), what)
                assert ops.last_kernel().startswith("apply_fwd_io/u16->f32"), ops.last_kernel()
                no_nan(what, out)
                close_dev(f"{what} ({ops.last_kernel()})", out, want)
            else:
                outs = [torch.full((B, H, W, 3), f, dtype=torch.uint8, device=dev) for f in (0, 255)]
                for out in outs:
                    ok(abi_io(lib, grid, t_in, out, white, **kw), what)
                    assert ops.last_kernel().startswith("apply_fwd_io/u8->u8"), ops.last_kernel()
                assert torch.equal(outs[0], outs[1]), what + ": a byte no kernel wrote"
                check_u8(N(outs[0]), want, what)
    what = f"{tag} upadd_io u8 -> u8"
    outs = [torch.full((B, H, W, 3), f, dtype=torch.uint8, device=dev) for f in (0, 255)]
    if not inside:
        for out, fill in zip(outs, (0, 255)):
            refused(abi_upadd_io(lib, grid, T(raw8, dev), T(coarse, dev), out, 255.0, guide), out, fill, B, H, W, word, what)
        return
    x8 = (raw8.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    want = port16.bilateral_slice_apply(c.grid, c.guide, x8, True) + oracle.resize_bilinear_align_corners(coarse, H, W)
    for out in outs:
        ok(abi_upadd_io(lib, grid, T(raw8, dev), T(coarse, dev), out, 255.0, guide), what)
    assert torch.equal(outs[0], outs[1]), what + ": a byte no kernel wrote"
    check_u8(N(outs[0]), want.astype(np.float32), what)


@pytest.mark.parametrize("need_guide,need_input", GRAD_SUBSETS)
@pytest.mark.parametrize("shape", TALL_DEEP + ec.NYG, ids=TALL_DEEP_IDS + ["nyg=65535", "nyg=65536"])
def test_tall_and_deep_gradients(dev, ops, lib, port16, shape, need_guide, need_input):
    """The gradient pass has no bound on H (a task takes rg rows) and one on B, the row groups nyg and GH: at H = 65536
    on a 3-row grid it stays on the MFMA pass; at B = 65536, and at nyg = 65536 (H = 65536 on GH = 65535), the row
    family's per-pixel kernel and the generic grid gradient take over."""
    c = small_case(port16, shape)
    run_grads(ops, lib, dev, c, need_guide, need_input, " x ".join(str(v) for v in shape))


def test_per_pixel_gradients_alone_on_both_sides_of_65535(dev, ops, lib, port16):
    """dguide + dinput without dgrid: apply_vjp_seg up to 65535 rows, apply_vjp_rows beyond."""
    for shape in ec.TALL[1:3] + ec.DEEP:  # (65535, 8), (65536, 4) and both batches
        B, H, W, GH, GW, GD = shape
        c = small_case(port16, shape)
        want = c.grads()
        grid, guide, x, dout = T(c.grid, dev), T(c.guide, dev), T(c.x, dev), T(c.dout, dev)
        dguide, dinput = nan(tuple(guide.shape), dev), nan(tuple(x.shape), dev)
        ok(abi_grad(lib, grid, guide, x, dout, None, dguide, dinput), str(shape))
        assert ops.last_kernel() == rp.vjp_kernel(B, H, W, GW, GD), (shape, ops.last_kernel())
        tag = f"{B} x {H} x {W} ({ops.last_kernel()})"
        no_nan(tag, dguide, dinput)
        check_pixel_grad(N(dguide), want["dguide"], tag, "dguide")
        check_pixel_grad(N(dinput), want["dinput"], tag, "dinput")


@pytest.mark.parametrize("shape", ec.LAUNCH, ids=["2^32 - 2^22 threads", "2^32 threads"])
def test_one_dimensional_launch_at_the_runtime_s_thread_bound(dev, ops, lib, port16, shape):
    """kLimBlocks: 1023 x 65536 rows of 4 pixels are the row family's last one-dimensional launch (64 threads per row), at
    1024 x 65536 the runtime would refuse the launch and the generic kernel takes the frame.  The slice forward with one
    channel (guide 1 GB, output 1 GB), image b a copy of base image b % 3, into a NaN-filled output."""
    B, H, W, GH, GW, GD = shape
    rng = np.random.default_rng(B)
    grid = rng.random((3, GH, GW, GD, ec.LAUNCH_SLICE_C), dtype=np.float32)
    guide = (rng.random((3, H, W), dtype=np.float32) * 1.04 - 0.02).astype(np.float32)
    want = port16.bilateral_slice(grid, guide)
    index = torch.arange(B, device=dev) % 3
    out = nan((B, H, W, ec.LAUNCH_SLICE_C), dev)
    ok(abi_slice(lib, T(grid, dev)[index].contiguous(), T(guide, dev)[index].contiguous(), out), "slice")
    assert ops.last_kernel() == rp.slice_kernel(B, H, W, GW, GD, ec.LAUNCH_SLICE_C), ops.last_kernel()
    tag = f"{B} x {H} x {W} slice C = 1 ({ops.last_kernel()})"
    no_nan(tag, out)
    whole = B // 3 * 3
    bad = int((out[:whole].view(whole // 3, 3, -1) != out[:3].reshape(1, 3, -1)).any(dim=2).sum())
    bad += sum(int(not torch.equal(out[b], out[b % 3])) for b in range(whole, B))
    print(f"{tag}: images that differ from the first image of their base: {bad} of {B - 3}")
    assert bad == 0, tag
    for b in (0, 1, 2, B // 2, B - 1):
        np_close(f"{tag} image {b}", N(out[b]), want[b % 3])


# ---- 3. far offsets ---------------------------------------------------------------------------------------------------
class Far:
    """Three base images and a batch of B copies, image b = base b % 3, expanded on the device."""

    def __init__(self, name, dev, seed):
        self.case = ec.FAR[name]
        self.B, self.straddle, self.dev = self.case["B"], self.case["straddle"], dev
        self.H, self.W = ec.FAR_H, ec.FAR_W
        self.GH, self.GW, self.GD = ec.FAR_GRID
        self.rng = np.random.default_rng(seed)
        self.index = torch.arange(self.B, device=dev) % 3
        self.samples = (0, 1, 2, self.straddle, self.B - 1)  # each base once, the straddling image, the last one
        image_bytes, limit = self.H * self.W * self.case["widest"], 1 << self.case["power"]
        assert (self.B - 1) * image_bytes >= limit > self.straddle * image_bytes and limit < (self.straddle + 1) * image_bytes

    def expand(self, base):
        """[3, ...] numpy -> [B, ...] on the device."""
        return T(base, self.dev)[self.index].contiguous()

    def grid(self):
        return near_identity_grid(self.rng, 3, self.GH, self.GW, self.GD)

    def every_image_equals_the_first_of_its_base(self, name, out):
        """Within one launch the arithmetic does not depend on b: bit equality, in chunks of FAR_CHUNK images."""
        first = out[:3]
        bad = 0
        for a in range(3, self.B, ec.FAR_CHUNK):
            chunk = out[a:a + ec.FAR_CHUNK]
            n = chunk.shape[0] // 3
            assert chunk.shape[0] % 3 == 0
            bad += int((chunk.view(n, 3, -1) != first.reshape(1, 3, -1)).any(dim=2).sum())
        print(f"{name}: images that differ from the first image of their base: {bad} of {self.B - 3}")
        assert bad == 0, name

    def sampled(self, name, out, want_base, check):
        """The first images, the one that straddles the power of two and the last one, on the host against the oracle of
        their base image."""
        for b in self.samples:
            check(f"{name} image {b} of {self.B}", N(out[b]), want_base[b % 3])


def np_close(name, got, want, rtol=FWD_TOL, atol=FWD_TOL):
    err = np.abs(got.astype(np.float64) - want)
    print(f"{name}: max|err| = {err.max():.3e}, worst / (atol + rtol |want|) = {(err / (atol + rtol * np.abs(want))).max():.3f}")
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=name)


def test_far_offset_slice_forward_beyond_2_pow_32(dev, ops, lib, port16):
    """519 images of 90 x 1920 x 12 channels: the last starts beyond byte 2^32 of the 4.3 GB output (live: 4.7 GB)."""
    f = Far("slice forward C = 12", dev, 1)
    assert (f.B - 1) * f.H * f.W * 48 >= (1 << 32)
    grid, guide = f.grid(), (f.rng.random((3, f.H, f.W), dtype=np.float32) * 1.04 - 0.02).astype(np.float32)
    want = port16.bilateral_slice(grid, guide)
    out = nan((f.B, f.H, f.W, 12), dev)
    ok(abi_slice(lib, f.expand(grid), f.expand(guide), out), "slice")
    assert ops.last_kernel() == "slice_fwd_rows", ops.last_kernel()
    no_nan("far slice", out)
    f.every_image_equals_the_first_of_its_base("far slice", out)
    f.sampled("far slice", out, want, np_close)


def test_far_offset_apply_forward(dev, ops, lib, port16):
    """1038 images: guide 0.72 + input 2.15 + output 2.15 GB."""
    f = Far("apply forward 3 -> 3", dev, 2)
    grid, guide = f.grid(), (f.rng.random((3, f.H, f.W), dtype=np.float32) * 1.04 - 0.02).astype(np.float32)
    x = f.rng.random((3, f.H, f.W, 3), dtype=np.float32)
    want = port16.bilateral_slice_apply(grid, guide, x, True)
    out = nan((f.B, f.H, f.W, 3), dev)
    ok(abi_apply(lib, f.expand(grid), f.expand(guide), f.expand(x), out), "apply")
    assert ops.last_kernel() == "apply_fwd_seg/vec4", ops.last_kernel()
    no_nan("far apply", out)
    f.every_image_equals_the_first_of_its_base("far apply", out)
    f.sampled("far apply", out, want, np_close)


@pytest.mark.parametrize("with_dgrid", [True, False], ids=["all three gradients", "apply_vjp_seg alone"])
def test_far_offset_gradients(dev, ops, lib, port16, with_dgrid):
    """1038 images, guide + input + dout + dguide + dinput = 44 B/px = 7.9 GB live: the fused gradient pass asked for all
    three gradients, and the per-pixel kernel alone.  dguide / dinput: every image bit-equal to the first of its base;
    dgrid (its sums are ordered by the row groups, which do not depend on b either): check_dgrid's tolerance."""
    f = Far("all three gradients" if with_dgrid else "apply_vjp_seg alone", dev, 3)
    grid, guide = f.grid(), (f.rng.random((3, f.H, f.W), dtype=np.float32) * 1.04 - 0.02).astype(np.float32)
    x = f.rng.random((3, f.H, f.W, 3), dtype=np.float32)
    dout = f.rng.standard_normal((3, f.H, f.W, 3)).astype(np.float32)
    wg, wgu, wi = port16.bilateral_slice_apply_grad(grid, guide, x, dout, True)
    tgrid = f.expand(grid)
    dgrid = nan(tuple(tgrid.shape), dev) if with_dgrid else None
    dguide, dinput = nan((f.B, f.H, f.W), dev), nan((f.B, f.H, f.W, 3), dev)
    ok(abi_grad(lib, tgrid, f.expand(guide), f.expand(x), f.expand(dout), dgrid, dguide, dinput), "grad")
    kern = ops.last_kernel()
    assert kern == ("apply_bwd_fused/mfma" if with_dgrid else "apply_vjp_seg/vec4"), kern
    tag = f"far {kern}"
    no_nan(tag, dgrid, dguide, dinput)
    f.every_image_equals_the_first_of_its_base(tag + " dguide", dguide)
    f.every_image_equals_the_first_of_its_base(tag + " dinput", dinput)
    f.sampled(tag, dguide, wgu, lambda n, g, w: check_pixel_grad(g, w, n, "dguide"))
    f.sampled(tag, dinput, wi, lambda n, g, w: check_pixel_grad(g, w, n, "dinput"))
    if with_dgrid:
        first = dgrid[:3].reshape(1, 3, -1)
        scale = max(1.0, float(first.abs().max()))
        err = (dgrid.view(f.B // 3, 3, -1) - first).abs()
        worst = float((err / (1e-5 * scale + GRAD_RTOL * first.abs())).max())
        print(f"{tag} dgrid: every image against the first of its base: max|err| = {float(err.max()):.3e}, worst / bar = {worst:.3f}")
        assert worst <= 1.0
        f.sampled(tag, dgrid, wg, lambda n, g, w: check_dgrid(g, w, n))


def test_far_offset_guide_network_forward(dev, ops, lib, port16):
    """1038 images: input 2.15 + output 2.15 + guide copy 0.72 GB."""
    f = Far("guide-network forward", dev, 4)
    grid, x = f.grid(), f.rng.random((3, f.H, f.W, 3), dtype=np.float32)
    c1, c2 = nn_params(f.rng)
    guide = oracle.pointwise_nn_guide(x, c1, c2)
    want = port16.bilateral_slice_apply(grid, guide, x, True)
    out, gout = nan((f.B, f.H, f.W, 3), dev), nan((f.B, f.H, f.W), dev)
    ok(abi_nnguide(lib, f.expand(grid), f.expand(x), T(c1, dev), T(c2, dev), out, gout), "nnguide")
    assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide", ops.last_kernel()
    no_nan("far nnguide", out, gout)
    f.every_image_equals_the_first_of_its_base("far nnguide out", out)
    f.every_image_equals_the_first_of_its_base("far nnguide guide", gout)
    f.sampled("far nnguide out", out, want, np_close)
    f.sampled("far nnguide guide", gout, guide, lambda n, g, w: np_close(n, g, w, rtol=0, atol=NN_GUIDE_TOL))


@pytest.mark.parametrize("kind", ["u8", "u16"])
def test_far_offset_wire_format_to_f32(dev, ops, lib, port16, kind):
    """1038 images of uint8 / uint16 samples to float32: the 2.15 GB output is the widest tensor."""
    f = Far(f"{kind} -> f32 wire format", dev, 5)
    white = 255.0 if kind == "u8" else 32767.0
    raw = f.rng.integers(0, 256, (3, f.H, f.W, 3), dtype=np.uint8) if kind == "u8" else \
        f.rng.integers(0, 32768, (3, f.H, f.W, 3), dtype=np.uint16)
    grid, guide = f.grid(), (f.rng.random((3, f.H, f.W), dtype=np.float32) * 1.04 - 0.02).astype(np.float32)
    want = port16.bilateral_slice_apply(grid, guide, (raw.astype(np.float32) / np.float32(white)).astype(np.float32), True)
    # (torch indexes no uint16 tensor: the copies are made on the same bits as int16)
    t_in = T(raw, dev)[f.index].contiguous() if kind == "u8" else \
        T16(raw, dev).view(torch.int16)[f.index].contiguous().view(torch.uint16)
    out = nan((f.B, f.H, f.W, 3), dev)
    ok(abi_io(lib, f.expand(grid), t_in, out, white, guide=f.expand(guide)), "io")
    assert ops.last_kernel().startswith(f"apply_fwd_io/{kind}->f32"), ops.last_kernel()
    no_nan(f"far io {kind}", out)
    f.every_image_equals_the_first_of_its_base(f"far io {kind}", out)
    f.sampled(f"far io {kind} -> f32", out, want, np_close)


def test_far_offset_upadd_and_resize(dev, ops, lib, port16):
    """1038 images: the up-add forward (guide 0.72 + input 2.15 + output 2.15 GB + a 23 x 480 coarse level per image) and,
    into the same output buffer, resize_bilinear on its output side."""
    f = Far("up-add", dev, 6)
    grid, guide = f.grid(), (f.rng.random((3, f.H, f.W), dtype=np.float32) * 1.04 - 0.02).astype(np.float32)
    x = f.rng.random((3, f.H, f.W, 3), dtype=np.float32)
    coarse = f.rng.random((3, ec.COARSE_H, ec.COARSE_W, 3), dtype=np.float32)
    up = oracle.resize_bilinear_align_corners(coarse, f.H, f.W)
    want = (port16.bilateral_slice_apply(grid, guide, x, True) + up).astype(np.float32)
    tcoarse = f.expand(coarse)
    out = nan((f.B, f.H, f.W, 3), dev)
    ok(abi_upadd(lib, f.expand(grid), f.expand(x), tcoarse, out, guide=f.expand(guide)), "upadd")
    assert ops.last_kernel() == "apply_fwd_seg/vec4+upadd", ops.last_kernel()
    no_nan("far upadd", out)
    f.every_image_equals_the_first_of_its_base("far upadd", out)
    f.sampled("far upadd", out, want, np_close)
    out.fill_(float("nan"))
    ok(abi_resize(lib, tcoarse, out), "resize")
    no_nan("far resize", out)
    f.every_image_equals_the_first_of_its_base("far resize", out)
    f.sampled("far resize_bilinear", out, up, np_close)


def test_far_offset_guide_network_vjp(dev, ops, lib):
    """hdrnet_pointwise_guide_grad_f32 (Cin = 3, n = 16) on 1038 images: input 2.15 + guide 0.72 + dguide 0.72 + dinput
    2.15 GB.  dinput into a NaN-filled buffer, every image bit-equal to the first of its base and the sampled images
    against float64 autograd of their base; dconv1 / dconv2 against 346 times the float64 gradients of the three base
    images -- the bars of test_guide_nn_grad_4x1080p_vs_float64 (1e-5 of the sum of |term|)."""
    from test_gpu_guide_grad_fullsize import nn_reference, param_close, pixel_close
    f = Far("guide-network VJP", dev, 9)
    npx_image = f.H * f.W
    x = f.rng.random((3, f.H, f.W, 3), dtype=np.float32)
    dg = f.rng.standard_normal((3, f.H, f.W)).astype(np.float32)
    c1, c2 = (T(a, dev) for a in nn_params(f.rng))
    ref, din64, sin64, guide, kink = nn_reference(T(x, dev).reshape(-1, 3), T(dg, dev).reshape(-1), c1, c2)
    tx, tdg = f.expand(x), f.expand(dg)
    tguide = guide.reshape(3, f.H, f.W)[f.index].contiguous()
    dinput = nan((f.B, f.H, f.W, 3), dev)
    dc1, dc2 = nan(tuple(c1.shape), dev), nan(tuple(c2.shape), dev)
    npx = f.B * npx_image
    with torch.cuda.device(dev):
        wbytes = lib.hdrnet_pointwise_guide_grad_workspace_bytes(npx, 3, 16)
        ws = torch.empty((max(wbytes, 16),), dtype=torch.uint8, device=dev)
        ok(lib.hdrnet_pointwise_guide_grad_f32(tx.data_ptr(), tguide.data_ptr(), tdg.data_ptr(), c1.data_ptr(), c2.data_ptr(),
                                               dinput.data_ptr(), 0, dc1.data_ptr(), dc2.data_ptr(), npx, 3, 16, ws.data_ptr(),
                                               wbytes, _stream(tx)), "guide_nn_grad")
    assert ops.last_kernel() == "guide_nn_grad", ops.last_kernel()
    no_nan("far guide_nn_grad", dinput, dc1, dc2)
    f.every_image_equals_the_first_of_its_base("far guide_nn_grad dinput", dinput)
    n = f.B // 3
    param_close("far guide_nn_grad dconv1", dc1, n * ref["dc1"], n * ref["s1"])
    param_close("far guide_nn_grad dconv2", dc2, n * ref["dc2"], n * ref["s2"])
    for b in f.samples:
        px = slice((b % 3) * npx_image, (b % 3 + 1) * npx_image)
        pixel_close(f"far guide_nn_grad dinput image {b} of {f.B}", dinput[b].reshape(-1, 3), din64[px], sin64[px],
                    kink[px, None].expand(npx_image, 3))


def test_far_offset_input_moments(dev, ops):
    """sum x_j and sum x_i x_j over 1038 images (2.15 GB) against float64 sums of the three base images times 346, at
    test_input_moments_4x1080p_and_fold's bar (1e-6 relative)."""
    f = Far("input_moments", dev, 7)
    x = f.rng.random((3, f.H, f.W, 3), dtype=np.float32)
    sums, mom = ops.input_moments(f.expand(x))
    assert ops.last_kernel() == "input_moments", ops.last_kernel()
    flat = x.reshape(-1, 3).astype(np.float64)
    n = f.B // 3
    for nm, got, want in (("sums", sums, n * flat.sum(0)), ("moments", mom, n * (flat.T @ flat))):
        err = np.abs(N(got).astype(np.float64) - want)
        worst = float((err / (1e-6 * np.abs(want))).max())
        print(f"far input_moments {nm}: max|err| = {err.max():.3e}, worst / (1e-6 |want|) = {worst:.2f}")
        assert worst <= 1.0


def test_far_offset_l2_loss_and_its_gradient(dev, lib):
    """mean((t - p)^2) and (2 / n) g (p - t) over 1038 images (prediction, target, gradient: 6.5 GB) at
    test_l2_loss_config_size_vs_float64's bars: loss 1e-6 relative; gradient rtol 1e-6, every image bit-equal to the first of
    its base."""
    f = Far("l2_loss and its gradient", dev, 8)
    p, t = (f.rng.random((3, f.H, f.W, 3), dtype=np.float32) for _ in range(2))
    tp, tt = f.expand(p), f.expand(t)
    n = tp.numel()
    d64 = p.astype(np.float64) - t
    want = float(np.square(d64).mean())
    loss = nan((1,), dev)
    with torch.cuda.device(dev):
        wbytes = lib.hdrnet_l2_loss_workspace_bytes(n)
        ws = torch.empty((max(wbytes, 16),), dtype=torch.uint8, device=dev)
        ok(lib.hdrnet_l2_loss_f32(tp.data_ptr(), tt.data_ptr(), n, loss.data_ptr(), ws.data_ptr(), wbytes, _stream(tp)), "l2_loss")
        err = abs(float(loss) - want)
        print(f"far l2_loss: |err| = {err:.3e}, worst / (1e-6 want) = {err / (1e-6 * want):.3f}")
        assert err <= 1e-6 * want
        up = torch.tensor(-2.5, device=dev)
        dp = nan(tuple(tp.shape), dev)
        ok(lib.hdrnet_l2_loss_grad_f32(tp.data_ptr(), tt.data_ptr(), up.data_ptr(), n, dp.data_ptr(), _stream(tp)), "l2_loss_grad")
    no_nan("far l2_loss_grad", dp)
    f.every_image_equals_the_first_of_its_base("far l2_loss_grad", dp)
    f.sampled("far l2_loss_grad", dp, -2.5 * (2.0 / n) * d64, lambda nm, g, w: np_close(nm, g, w, rtol=1e-6, atol=1e-14))
