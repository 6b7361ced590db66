"""Parity of the HIP path (through the C-ABI, via hdrnet_amd.hdrnet_ops) with the CPU oracle.

Bars:
* generic kernels (HDRNET_KERNEL_GENERIC, -ffp-contract=off): forward, guide VJP, input VJP
  and the gather-form grid VJP are BIT-EXACT against the oracle / the reference CPU op;
* fast kernels: forward rtol = atol = 1e-5 REQUIRED (the reference's own JAX-vs-CUDA bar of
  1e-6, hdrnet_ops_jax_tf2_test.py:48, is measured and printed); gradients rtol 1e-4 with
  atol scaled to the tensor's magnitude.
"""
import numpy as np
import pytest
import torch

from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu

FWD_RTOL = FWD_ATOL = 1e-5
REF_BAR = 1e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need an MI355X"
    name = torch.cuda.get_device_name(0)
    print("device:", name, torch.version.hip)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from hdrnet_amd import hdrnet_ops
    return hdrnet_ops


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def rand_case(rng, B, H, W, GH, GW, GD, Cin, Cout, ho, lo=0.0, hi=1.0):
    Cj = Cin + int(ho)
    grid = rng.standard_normal((B, GH, GW, GD, Cout * Cj)).astype(np.float32)
    guide = (rng.random((B, H, W)) * (hi - lo) + lo).astype(np.float32)
    inp = rng.random((B, H, W, Cin)).astype(np.float32)
    dout = rng.standard_normal((B, H, W, Cout)).astype(np.float32)
    return grid, guide, inp, dout


def grads_close(got, want, what, rtol=1e-4):
    scale = float(np.abs(want).max()) if want.size else 0.0
    np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-5 * max(scale, 1.0), err_msg=what)


# ---- library really is the thing running ---------------------------------------------------
def test_native_library_loaded(dev, ops):
    from hdrnet_amd import _lib
    lib = _lib.load()
    assert lib.hdrnet_version() >= 100
    maps = open("/proc/self/maps").read()
    assert "libhdrnet_amd.so" in maps
    g = load_golden("apply_forward_default")
    ops.bilateral_slice_apply(T(g["grid"], dev), T(g["guide"], dev), T(g["input"], dev), has_offset=True)
    assert ops.last_kernel().startswith(("apply_fwd_seg", "apply_fwd_rows"))  # AUTO picks an LDS-staged kernel


# ---- golden fixtures (made from the reference's own CPU code) ---------------------------------
@pytest.mark.parametrize("name", golden_names("apply_"))
@pytest.mark.parametrize("which", ["generic", "auto"])
def test_apply_golden(dev, ops, name, which):
    g = load_golden(name)
    ho = bool(g["has_offset"])
    grid = T(g["grid"], dev).requires_grad_(True)
    guide = T(g["guide"], dev).requires_grad_(True)
    inp = T(g["input"], dev).requires_grad_(True)
    with ops.kernel_override(which):
        out = ops.bilateral_slice_apply(grid, guide, inp, has_offset=ho)
        kern_fwd = ops.last_kernel()
        out.backward(T(g["dout"], dev))
    assert list(out.shape) == list(g["out"].shape)
    if which == "generic":
        assert kern_fwd == "apply_fwd_generic"
        assert np.array_equal(N(out), g["out"]), np.abs(N(out) - g["out"]).max()
        assert np.array_equal(N(guide.grad), g["dguide"])
        assert np.array_equal(N(inp.grad), g["dinput"])
        assert np.array_equal(N(grid.grad), g["dgrid"])
    else:
        np.testing.assert_allclose(N(out), g["out"], rtol=FWD_RTOL, atol=FWD_ATOL)
        grads_close(N(guide.grad), g["dguide"], "dguide")
        grads_close(N(inp.grad), g["dinput"], "dinput")
        grads_close(N(grid.grad), g["dgrid"], "dgrid")
    assert list(grid.grad.shape) == list(g["grid"].shape)     # hdrnet_ops_test.py:304-315
    assert list(guide.grad.shape) == list(g["guide"].shape)
    assert list(inp.grad.shape) == list(g["input"].shape)


@pytest.mark.parametrize("name", golden_names("slice_"))
@pytest.mark.parametrize("which", ["generic", "auto"])
def test_slice_golden(dev, ops, name, which):
    g = load_golden(name)
    grid = T(g["grid"], dev).requires_grad_(True)
    guide = T(g["guide"], dev).requires_grad_(True)
    with ops.kernel_override(which):
        out = ops.bilateral_slice(grid, guide)
        out.backward(T(g["dout"], dev))
    assert list(out.shape) == list(g["out"].shape)            # hdrnet_ops_test.py:115-123
    if which == "generic":
        assert np.array_equal(N(out), g["out"])
        assert np.array_equal(N(guide.grad), g["dguide"])
        assert np.array_equal(N(grid.grad), g["dgrid"])
    else:
        np.testing.assert_allclose(N(out), g["out"], rtol=FWD_RTOL, atol=FWD_ATOL)
        grads_close(N(guide.grad), g["dguide"], "dguide")
        grads_close(N(grid.grad), g["dgrid"], "dgrid")


def test_interpolate_known_answer(dev, ops):
    """hdrnet/test/ops_test.py:61-86."""
    k = load_golden("slice_interpolate_kat")
    for val in range(3):
        guide = torch.full((3, 5, 9), (val + 0.5) / 3.0, dtype=torch.float32, device=dev)
        out = N(ops.bilateral_slice(T(k["grid"], dev), guide))
        assert list(out.shape) == [3, 5, 9, 1]
        assert np.amax(np.abs(val - out)) < 5e-4
        np.testing.assert_allclose(out, k["outs"][val], rtol=0, atol=1e-6)


# ---- seeded random shapes against the oracle ---------------------------------------------------
APPLY_SHAPES = [  # B, H, W, GH, GW, GD, Cin, Cout, has_offset, guide range
    (1, 1, 1, 1, 1, 1, 3, 3, True, 0.0, 1.0),        # degenerate extents
    (2, 37, 53, 16, 16, 8, 3, 3, True, 0.0, 1.0),    # ragged W (scalar variant), HDRNet shape
    (1, 64, 256, 16, 16, 8, 3, 3, True, -0.3, 1.3),  # vec4 variant, guide out of range
    (1, 128, 1024, 16, 16, 8, 3, 3, True, 0.0, 1.0),
    (3, 30, 25, 16, 12, 8, 3, 3, False, 0.0, 1.0),   # no offset: C = 9 (non-float4 LDS image)
    (2, 19, 40, 6, 3, 7, 3, 4, True, 0.0, 1.0),      # reference grad-test grid, Cout=4
    (1, 24, 36, 3, 9, 7, 1, 1, True, 0.0, 1.0),      # Cin = Cout = 1
    (1, 24, 36, 3, 9, 7, 1, 1, False, 0.0, 1.0),
    (1, 40, 60, 8, 8, 4, 1, 3, True, 0.0, 1.0),      # grey -> colour
    (1, 20, 28, 4, 4, 4, 4, 4, True, 0.0, 1.0),
    (1, 12, 20, 4, 4, 4, 2, 5, True, 0.0, 1.0),      # no specialisation -> generic
    (1, 6, 4, 32, 32, 8, 3, 3, True, 0.0, 1.0),      # image smaller than the grid
    (1, 48, 2048, 64, 256, 8, 3, 3, True, 0.0, 1.0), # many grid columns per segment
]


@pytest.mark.parametrize("shape", APPLY_SHAPES)
def test_apply_forward_random(dev, ops, port, shape):
    B, H, W, GH, GW, GD, Cin, Cout, ho, lo, hi = shape
    rng = np.random.default_rng(abs(hash(shape)) % (2 ** 31))
    grid, guide, inp, _ = rand_case(rng, B, H, W, GH, GW, GD, Cin, Cout, ho, lo, hi)
    want = port.bilateral_slice_apply(grid, guide, inp, ho)
    tg, tgu, ti = T(grid, dev), T(guide, dev), T(inp, dev)
    with ops.kernel_override("generic"):
        got = N(ops.bilateral_slice_apply(tg, tgu, ti, has_offset=ho))
    assert np.array_equal(got, want), ("generic not bit-exact", np.abs(got - want).max())
    got = N(ops.bilateral_slice_apply(tg, tgu, ti, has_offset=ho))
    kern = ops.last_kernel()
    np.testing.assert_allclose(got, want, rtol=FWD_RTOL, atol=FWD_ATOL, err_msg=kern)
    worst = float(np.max(np.abs(got - want) / (REF_BAR + REF_BAR * np.abs(want))))
    print(f"{shape} kernel={kern} max|err|={np.abs(got - want).max():.3e} "
          f"worst/(1e-6 bar)={worst:.2f}")
    # Regression guard well inside the required 1e-5: every shape here stays within 4x the
    # reference's own JAX-vs-CUDA bar (a contracted coordinate product once cost 10x).
    assert worst < 4.0, (kern, worst)


# The forward kernel that the TOOLS library selects by variant number (19: the round-1 row kernel, the product's own
# fallback; the rejected forwards, variants 2-11, were removed with their kernels) must compute the same op as the
# shipped one, or an A/B timing against it compares nothing.  It is reached through the TOOLS library's C-ABI only.
@pytest.mark.parametrize("variant,expect", [(19, "apply_fwd_rows/vec4")])
@pytest.mark.parametrize("shape", [(2, 48, 2048, 16, 16, 8, 3, 3, True, -0.2, 1.2),
                                   (1, 37, 3076, 16, 16, 8, 3, 3, True, 0.0, 1.0),
                                   (1, 21, 1920, 16, 16, 8, 3, 3, True, -0.1, 1.1)])
def test_apply_forward_benchmark_variants(dev, port, shape, variant, expect):
    import torch
    from hdrnet_amd import _lib
    tools = _lib.load_tools()
    tools.hdrnet_enable_kernel_names(1)
    B, H, W, GH, GW, GD, Cin, Cout, ho, lo, hi = shape
    rng = np.random.default_rng(variant * 1000 + W)
    grid, guide, inp, _ = rand_case(rng, B, H, W, GH, GW, GD, Cin, Cout, ho, lo, hi)
    want = port.bilateral_slice_apply(grid, guide, inp, ho)
    tg, tgu, ti = T(grid, dev), T(guide, dev), T(inp, dev)
    out = torch.full((B, H, W, Cout), float("nan"), device=dev)
    rc = tools.hdrnet_bilateral_slice_apply_f32_ex(
        tg.data_ptr(), tgu.data_ptr(), ti.data_ptr(), out.data_ptr(), B, H, W, GH, GW, GD, Cin, Cout,
        int(ho), _lib.KERNEL_FAST | (variant << 8), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, tools.hdrnet_last_error().decode()
    torch.cuda.synchronize()
    kern = tools.hdrnet_last_kernel().decode()
    assert expect in kern, kern
    np.testing.assert_allclose(N(out), want, rtol=FWD_RTOL, atol=FWD_ATOL, err_msg=kern)


def test_skeleton_variant_without_a_kernel_for_the_shape_is_refused(dev):
    """Variant 106 (a memory skeleton: 3 -> 3 with offset only) on a 1 -> 1 frame is refused by number -- not served by
    the product kernel under the skeleton's number -- and nothing is written."""
    import torch
    from hdrnet_amd import _lib
    tools = _lib.load_tools()
    B, H, W, GH, GW, GD = 1, 4, 16, 2, 2, 2
    grid = torch.rand((B, GH, GW, GD, 2), device=dev)
    guide = torch.rand((B, H, W), device=dev)
    inp = torch.rand((B, H, W, 1), device=dev)
    out = torch.full((B, H, W, 1), float("nan"), device=dev)
    rc = tools.hdrnet_bilateral_slice_apply_f32_ex(
        grid.data_ptr(), guide.data_ptr(), inp.data_ptr(), out.data_ptr(), B, H, W, GH, GW, GD, 1, 1, 1,
        _lib.KERNEL_FAST | (106 << 8), torch.cuda.current_stream(dev).cuda_stream)
    err = tools.hdrnet_last_error().decode()
    assert rc == _lib.HDRNET_INVALID_ARGUMENT, (rc, err)
    assert "variant 106 has no kernel for this shape" in err, err
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_product_library_has_no_benchmark_variants(dev):
    """The product library refuses variant numbers (skeletons that write garbage live only in the
    tools build)."""
    import torch
    from hdrnet_amd import _lib
    lib = _lib.load()
    t = torch.zeros(64, device=dev)
    rc = lib.hdrnet_bilateral_slice_apply_f32_ex(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(),
                                                 1, 1, 4, 1, 1, 1, 3, 3, 1, _lib.KERNEL_FAST | (101 << 8), None)
    assert rc == _lib.HDRNET_INVALID_ARGUMENT
    assert "tools build" in lib.hdrnet_last_error().decode()


@pytest.mark.parametrize("shape", APPLY_SHAPES[:10])
def test_apply_backward_random(dev, ops, port, shape):
    B, H, W, GH, GW, GD, Cin, Cout, ho, lo, hi = shape
    rng = np.random.default_rng(abs(hash(shape)) % (2 ** 31) + 1)
    grid, guide, inp, dout = rand_case(rng, B, H, W, GH, GW, GD, Cin, Cout, ho, lo, hi)
    wg, wgu, wi = port.bilateral_slice_apply_grad(grid, guide, inp, dout, ho)
    for which in ("generic", "auto"):
        tg = T(grid, dev).requires_grad_(True)
        tgu = T(guide, dev).requires_grad_(True)
        ti = T(inp, dev).requires_grad_(True)
        with ops.kernel_override(which):
            ops.bilateral_slice_apply(tg, tgu, ti, has_offset=ho).backward(T(dout, dev))
        if which == "generic":
            assert np.array_equal(N(tg.grad), wg)
            assert np.array_equal(N(tgu.grad), wgu)
            assert np.array_equal(N(ti.grad), wi)
        else:
            grads_close(N(tg.grad), wg, "dgrid")
            grads_close(N(tgu.grad), wgu, "dguide")
            grads_close(N(ti.grad), wi, "dinput")


def test_backward_uses_fast_kernels_and_is_deterministic(dev, ops):
    """HDRNet's shape (Cin 3 -> Cout 3 + offset): all three gradients from the fused backward pass
    (per-pixel VJPs + the two-stage MFMA dgrid reduction); no atomics => bitwise repeatable."""
    gen = torch.Generator(device=dev).manual_seed(77)
    grid = torch.rand((2, 16, 16, 8, 12), device=dev, generator=gen)
    guide = torch.rand((2, 270, 480), device=dev, generator=gen)
    inp = torch.rand((2, 270, 480, 3), device=dev, generator=gen)
    dout = torch.randn((2, 270, 480, 3), device=dev, generator=gen)
    res = []
    for _ in range(2):
        tg, tgu, ti = (t.clone().requires_grad_(True) for t in (grid, guide, inp))
        ops.bilateral_slice_apply(tg, tgu, ti, has_offset=True).backward(dout)
        assert ops.last_kernel() == "apply_bwd_fused/mfma", ops.last_kernel()
        res.append((tg.grad.clone(), tgu.grad.clone(), ti.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("H,W", [(1080, 1920)])
def test_full_frame_backward_fast_equals_generic(dev, ops, H, W):
    """All three VJPs at 1080p: fast kernels vs the generic ones (which are bit-exact to the
    reference CPU code; the gather-form dgrid takes ~0.1 s here, as slow as the reference's)."""
    gen = torch.Generator(device=dev).manual_seed(2024)
    grid = torch.rand((1, 16, 16, 8, 12), device=dev, generator=gen)
    guide = torch.rand((1, H, W), device=dev, generator=gen) * 1.1 - 0.05
    inp = torch.rand((1, H, W, 3), device=dev, generator=gen)
    dout = torch.randn((1, H, W, 3), device=dev, generator=gen)
    out = {}
    for which in ("generic", "auto"):
        tg, tgu, ti = (t.clone().requires_grad_(True) for t in (grid, guide, inp))
        with ops.kernel_override(which):
            ops.bilateral_slice_apply(tg, tgu, ti, has_offset=True).backward(dout)
        out[which] = (tg.grad, tgu.grad, ti.grad)
    for a, b, nm in zip(out["auto"], out["generic"], ("dgrid", "dguide", "dinput")):
        scale = max(1.0, b.abs().max().item())
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5 * scale, msg=lambda m, nm=nm: nm + ": " + m)
        print(f"{nm}: max|fast-generic| = {(a - b).abs().max().item():.3e} (scale {scale:.3g})")


def test_full_frame_adjointness_4k(dev, ops):
    """<dgrid, grid> == <dout, out> (the op is linear in the grid) and
    <dinput, in> + <dout, out(in=0)> == <dout, out> (affine in the input), on a 4K frame."""
    H, W = 2160, 3840
    gen = torch.Generator(device=dev).manual_seed(5)
    grid = torch.rand((1, 16, 16, 8, 12), device=dev, generator=gen).requires_grad_(True)
    guide = torch.rand((1, H, W), device=dev, generator=gen)
    inp = torch.rand((1, H, W, 3), device=dev, generator=gen).requires_grad_(True)
    dout = torch.randn((1, H, W, 3), device=dev, generator=gen)
    out = ops.bilateral_slice_apply(grid, guide, inp, has_offset=True)
    out.backward(dout)
    rhs = (dout.double() * out.detach().double()).sum().item()
    lhs = (grid.grad.double() * grid.detach().double()).sum().item()
    assert abs(lhs - rhs) <= 1e-4 * abs(rhs) + 1e-2, (lhs, rhs)
    off = ops.bilateral_slice_apply(grid.detach(), guide, torch.zeros_like(inp), has_offset=True)
    lhs2 = (inp.grad.double() * inp.detach().double()).sum().item() + (dout.double() * off.double()).sum().item()
    assert abs(lhs2 - rhs) <= 1e-4 * abs(rhs) + 1e-2, (lhs2, rhs)


def test_partial_gradients(dev, ops, port):
    """A NULL output pointer skips that VJP (bilateral_slice_apply.cu.cc:393,401,409)."""
    rng = np.random.default_rng(5)
    grid, guide, inp, dout = rand_case(rng, 1, 16, 24, 4, 4, 4, 3, 3, True)
    _, wgu, _ = port.bilateral_slice_apply_grad(grid, guide, inp, dout, True)
    tg, ti = T(grid, dev), T(inp, dev)
    tgu = T(guide, dev).requires_grad_(True)
    ops.bilateral_slice_apply(tg, tgu, ti, has_offset=True).backward(T(dout, dev))
    assert tg.grad is None and ti.grad is None
    grads_close(N(tgu.grad), wgu, "dguide only")


SLICE_SHAPES = [(2, 37, 53, 16, 12, 8, 12), (1, 64, 256, 16, 16, 8, 2), (1, 9, 7, 3, 4, 5, 1),
                (4, 64, 48, 16, 12, 8, 2)]  # last: hdrnet_ops_jax_tf2_test.py:28-34 at 1/10 size


@pytest.mark.parametrize("shape", SLICE_SHAPES)
def test_slice_random(dev, ops, port, shape):
    B, H, W, GH, GW, GD, C = shape
    rng = np.random.default_rng(abs(hash(shape)) % (2 ** 31))
    grid = rng.random((B, GH, GW, GD, C)).astype(np.float32)
    guide = (rng.random((B, H, W)) * 1.2 - 0.1).astype(np.float32)
    dout = rng.standard_normal((B, H, W, C)).astype(np.float32)
    want = port.bilateral_slice(grid, guide)
    wg, wgu = port.bilateral_slice_grad(grid, guide, dout)
    tg = T(grid, dev).requires_grad_(True)
    tgu = T(guide, dev).requires_grad_(True)
    out = ops.bilateral_slice(tg, tgu)
    out.backward(T(dout, dev))
    np.testing.assert_allclose(N(out), want, rtol=FWD_RTOL, atol=FWD_ATOL)
    grads_close(N(tg.grad), wg, "dgrid")
    grads_close(N(tgu.grad), wgu, "dguide")


# ---- fused point-wise guide network + slice-apply -------------------
@pytest.mark.parametrize("shape", [(2, 36, 64, 16, 16, 8, 3, 16), (1, 128, 1024, 16, 16, 8, 3, 16),
                                   (1, 40, 48, 8, 8, 4, 1, 5)])
def test_nnguide_fused_matches_composed_oracle(dev, ops, port, shape):
    """guide = folded point-wise NN (numpy, oracle.pointwise_nn_guide) -> oracle slice-apply, vs the
    fused kernel.  The guide itself must agree to 1e-6; the output carries the guide's ulp-level
    differences times d out / d guide = GD * (z-difference of the grid); it holds the plain forward's 1e-5
    all the same (round 3 had relaxed this bar to 2e-5)."""
    import oracle
    B, H, W, GH, GW, GD, Cin, n = shape
    rng = np.random.default_rng(sum(shape))
    grid = rng.random((B, GH, GW, GD, Cin * (Cin + 1))).astype(np.float32)
    inp = rng.random((B, H, W, Cin)).astype(np.float32)
    conv1 = (rng.standard_normal((n, Cin + 1)) * 0.8).astype(np.float32)
    conv2 = (rng.standard_normal(n + 1) * 0.5).astype(np.float32)
    guide = oracle.pointwise_nn_guide(inp, conv1, conv2)
    want = port.bilateral_slice_apply(grid, guide, inp, True)
    out, gout = ops.bilateral_slice_apply_nnguide(T(grid, dev), T(inp, dev), T(conv1, dev), T(conv2, dev),
                                                  has_offset=True, return_guide=True)
    assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide"
    np.testing.assert_allclose(N(gout), guide, rtol=0, atol=1e-6)
    np.testing.assert_allclose(N(out), want, rtol=1e-5, atol=1e-5)
    # and against the un-fused HIP path fed with the fused kernel's own guide: same slicing code
    ref = ops.bilateral_slice_apply(T(grid, dev), gout, T(inp, dev), has_offset=True)
    torch.testing.assert_close(out, ref, rtol=1e-6, atol=1e-6)
    # The sigmoid is the CALLER's choice (HDRNET_GUIDE_SIGMOID_FAST), not a side effect of asking for the guide copy
    # (until round 5 `guide_out == NULL` selected the hardware form): without the copy the default call gives the same
    # bits as with it ...
    out_nocopy = ops.bilateral_slice_apply_nnguide(T(grid, dev), T(inp, dev), T(conv1, dev), T(conv2, dev))
    assert torch.equal(out_nocopy, out)
    # ... and with fast_sigmoid=True the kernel takes exp / reciprocal from v_exp_f32 / v_rcp_f32 (<= 2 ulp of the guide):
    # the same bar against the oracle, not bit-equality with `out`; with or without the copy the same bits again
    out2 = ops.bilateral_slice_apply_nnguide(T(grid, dev), T(inp, dev), T(conv1, dev), T(conv2, dev), fast_sigmoid=True)
    np.testing.assert_allclose(N(out2), want, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(out2, out, rtol=1e-5, atol=1e-5)
    out3, gout3 = ops.bilateral_slice_apply_nnguide(T(grid, dev), T(inp, dev), T(conv1, dev), T(conv2, dev),
                                                    return_guide=True, fast_sigmoid=True)
    assert torch.equal(out3, out2)
    np.testing.assert_allclose(N(gout3), guide, rtol=0, atol=1e-6)


def test_inference_sigmoid_moves_the_guide_by_at_most_2_ulp(dev, ops):
    """ADVICE r03 / VERDICT r04: with HDRNET_GUIDE_SIGMOID_FAST (``fast_sigmoid=True``, what the models' inference passes)
    the fused guide network takes its sigmoid from v_exp_f32 + v_rcp_f32 instead of expf + an IEEE divide -- an explicit,
    documented choice of the caller.  This bounds the GUIDE itself,
    not only the output: with a grid whose only non-zero coefficients are the offsets (z + 0.5) / GD the sliced
    output IS the guide up to the smoothed tent (d out / d guide = 1), so the two forms' outputs differ by the two
    sigmoids' difference: <= 2 ulp of a value in (0, 1), i.e. 2.4e-7."""
    B, H, W, GH, GW, GD, n = 1, 64, 512, 16, 16, 8, 16
    rng = np.random.default_rng(77)
    grid6 = np.zeros((B, GH, GW, GD, 3, 4), np.float32)
    grid6[..., :, 3] = ((np.arange(GD, dtype=np.float32) + 0.5) / GD)[None, None, None, :, None]
    grid = grid6.reshape(B, GH, GW, GD, 12)
    inp = rng.random((B, H, W, 3)).astype(np.float32)
    conv1 = (rng.standard_normal((n, 4)) * 0.8).astype(np.float32)
    conv2 = (rng.standard_normal(n + 1) * 0.5).astype(np.float32)
    args = (T(grid, dev), T(inp, dev), T(conv1, dev), T(conv2, dev))
    out_train, gout = ops.bilateral_slice_apply_nnguide(*args, has_offset=True, return_guide=True)
    out_infer = ops.bilateral_slice_apply_nnguide(*args, has_offset=True, fast_sigmoid=True)
    g = N(gout)
    assert g.max() - g.min() > 0.5 and g.std() > 0.05  # the sigmoid is exercised over a wide range
    d = np.abs(N(out_train) - N(out_infer)).max()
    print(f"max|out(train sigmoid) - out(inference sigmoid)| = {d:.3e} (2 ulp of 1.0 = 2.4e-7)")
    assert d <= 2.4e-7
    # and the slice of that grid really is the guide (so that the bound above is a bound on the guide)
    np.testing.assert_allclose(N(out_train)[..., 0], np.clip(g, 0.5 / GD, 1 - 0.5 / GD), rtol=0, atol=2e-4)


@pytest.mark.parametrize("n", [16, 6, 3])
def test_prescaled_guide_network_is_bit_identical(dev, ops, n):
    """HDRNET_GUIDE_RELU_PRESCALED (round 5): the guide network's first layer scaled per feature by 2^-e_k, its mixing
    weight by 2^e_k, relu taken from the CLAMP modifier of the feature's last v_pk_fma_f32.  Powers of two commute with
    every rounding, so for inputs within the prescale's x_max the guide and the output are the plain evaluation's BIT
    FOR BIT -- both sigmoids, the fp32 kernel, the up-add level and the uint8 wire format; n = 6 / 3 run the
    remainder loop (features past a multiple of four)."""
    B, H, W, GH, GW, GD = 2, 40, 256, 16, 16, 8
    rng = np.random.default_rng(500 + n)
    grid = T(rng.random((B, GH, GW, GD, 12)).astype(np.float32), dev)
    inp = T(rng.random((B, H, W, 3)).astype(np.float32), dev)
    conv1 = T((rng.standard_normal((n, 4)) * 0.8).astype(np.float32), dev)
    conv2 = T((rng.standard_normal(n + 1) * 0.5).astype(np.float32), dev)
    p1, p2 = ops.guide_nn_prescale(conv1, conv2, x_max=65536.0)
    # the prescale itself: exact power-of-two scalings of the reordered row {w0, b, w1, w2}, bias copied
    c1, q1 = N(conv1).astype(np.float64), N(p1).astype(np.float64)
    ratio = q1[:, 0] / c1[:, 0]
    e = -np.log2(ratio)
    assert np.array_equal(e, np.round(e))
    np.testing.assert_array_equal(q1, c1[:, [0, 3, 1, 2]] * ratio[:, None])
    np.testing.assert_array_equal(N(p2)[:n].astype(np.float64), N(conv2)[:n].astype(np.float64) / ratio)
    assert N(p2)[n] == N(conv2)[n]
    bound = np.abs(c1[:, 3]) + 65536.0 * np.abs(c1[:, :3]).sum(1)
    assert (2.0 ** e >= 2 * bound * (1 - 1e-6)).all() and (2.0 ** e <= 4 * bound * (1 + 1e-6)).all()
    for fast in (False, True):
        out, g = ops.bilateral_slice_apply_nnguide(grid, inp, conv1, conv2, return_guide=True, fast_sigmoid=fast)
        out_p, g_p = ops.bilateral_slice_apply_nnguide(grid, inp, p1, p2, return_guide=True, fast_sigmoid=fast,
                                                       prescaled=True)
        assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide"
        assert torch.equal(g_p, g) and torch.equal(out_p, out)
    coarse = T(rng.random((B, H // 2, W // 2, 3)).astype(np.float32), dev)
    up = ops.bilateral_slice_apply_upadd(grid, inp, coarse, guide_conv1=conv1, guide_conv2=conv2, fast_sigmoid=True)
    up_p = ops.bilateral_slice_apply_upadd(grid, inp, coarse, guide_conv1=p1, guide_conv2=p2, fast_sigmoid=True,
                                           prescaled=True)
    assert torch.equal(up_p, up)
    raw = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    for od in (torch.uint8, torch.float32):
        o8, g8 = ops.bilateral_slice_apply_io(grid, raw, guide_conv1=conv1, guide_conv2=conv2, out_dtype=od,
                                              return_guide=True, fast_sigmoid=True)
        o8p, g8p = ops.bilateral_slice_apply_io(grid, raw, guide_conv1=p1, guide_conv2=p2, out_dtype=od,
                                                return_guide=True, fast_sigmoid=True, prescaled=True)
        assert torch.equal(g8p, g8) and torch.equal(o8p, o8)
    # inference only: a differentiable call refuses the prescaled layout
    with pytest.raises(ValueError, match="inference-only"):
        ops.bilateral_slice_apply_nnguide(grid.clone().requires_grad_(True), inp, p1, p2, prescaled=True)


def test_prescaled_guide_network_saturates_beyond_x_max(dev, ops):
    """The contract's other half: the clamp bounds a feature at 2^e_k, so an input far beyond the prescale's x_max can
    saturate where the plain evaluation keeps growing -- inside x_max (here 4.0: inputs in [0, 4)) the two agree bit for
    bit, and with the same parameters an input of 1e4 moves the guide."""
    B, H, W, GH, GW, GD, n = 1, 16, 128, 8, 8, 8, 16
    rng = np.random.default_rng(9)
    grid = T(rng.random((B, GH, GW, GD, 12)).astype(np.float32), dev)
    conv1 = T((np.abs(rng.standard_normal((n, 4))) * 0.8).astype(np.float32), dev)  # positive weights: h grows with x
    # (mixing weights small enough that the sigmoid does not saturate on its own at |x| = 1e4: acc ~ +-1 there)
    conv2 = T((rng.standard_normal(n + 1) * 2e-5).astype(np.float32), dev)
    p1, p2 = ops.guide_nn_prescale(conv1, conv2, x_max=4.0)
    inside = T((rng.random((B, H, W, 3)) * 4.0).astype(np.float32), dev)
    _, g = ops.bilateral_slice_apply_nnguide(grid, inside, conv1, conv2, return_guide=True)
    _, gp = ops.bilateral_slice_apply_nnguide(grid, inside, p1, p2, return_guide=True, prescaled=True)
    assert torch.equal(gp, g)
    far = torch.full((B, H, W, 3), 1e4, device=dev)
    _, g = ops.bilateral_slice_apply_nnguide(grid, far, conv1, conv2, return_guide=True)
    _, gp = ops.bilateral_slice_apply_nnguide(grid, far, p1, p2, return_guide=True, prescaled=True)
    assert not torch.equal(gp, g)


# ---- curves guide (the standard model) fused into slice-apply --------------------------------------
@pytest.mark.parametrize("in_dtype,out_dtype", [("float32", "float32"), ("uint8", "uint8"), ("uint16", "float32")])
def test_curves_guide_fused_matches_composed_oracle(dev, ops, port, in_dtype, out_dtype):
    """guide = oracle.curves_guide (numpy restatement of HDRNetCurves._guide) -> oracle slice-apply,
    vs the one fused kernel, fp32 and in the wire formats of the reference's GL renderer."""
    import oracle
    B, H, W = 2, 40, 96
    rng = np.random.default_rng(21)
    grid = rng.random((B, 16, 16, 8, 12)).astype(np.float32)
    ccm = (np.concatenate([np.eye(3), np.zeros((3, 1))], 1) + 0.2 * rng.standard_normal((3, 4))).astype(np.float32)
    shifts = (np.tile(np.linspace(0, 1, 16, endpoint=False)[:, None], (1, 3)) + 0.01 * rng.standard_normal((16, 3))).astype(np.float32)
    slopes = (0.3 * rng.standard_normal((16, 3))).astype(np.float32)
    slopes[0] += 1.0
    mix = np.array([0.4, 0.35, 0.25, 0.02], np.float32)
    if in_dtype == "float32":
        raw = rng.random((B, H, W, 3)).astype(np.float32)
        x, wl = raw, 1.0
    else:
        hi = 255 if in_dtype == "uint8" else 65535
        raw = rng.integers(0, hi + 1, (B, H, W, 3)).astype(in_dtype)
        x, wl = raw.astype(np.float32) / np.float32(hi), float(hi)
    guide = oracle.curves_guide(x, ccm, shifts, slopes, mix)
    want = port.bilateral_slice_apply(grid, guide, x, True)
    traw = torch.from_numpy(raw.astype(np.int32)).to(dev).to(getattr(torch, in_dtype)) if in_dtype != "float32" else T(raw, dev)
    out, gout = ops.bilateral_slice_apply_io(
        T(grid, dev), traw, guide_curves=tuple(T(a, dev) for a in (ccm, shifts, slopes, mix)),
        input_white_level=wl, out_dtype=getattr(torch, out_dtype), return_guide=True)
    assert ops.last_kernel() == f"apply_fwd_io/{ {'float32': 'f32', 'uint8': 'u8', 'uint16': 'u16'}[in_dtype]}->" \
                                f"{ {'float32': 'f32', 'uint8': 'u8'}[out_dtype]}+curvesguide"
    np.testing.assert_allclose(N(gout), guide, rtol=0, atol=2e-6)

    def check(out):
        if out_dtype == "float32":
            np.testing.assert_allclose(N(out), want, rtol=1e-5, atol=1e-5)
        else:
            q = np.clip(want, 0, 1) * np.float32(255)
            got = N(out).astype(np.int32)
            exact = q.astype(np.uint8).astype(np.int32)
            near_edge = np.abs(q - np.round(q)) < 1e-5 * 255
            assert np.all((got == exact) | (near_edge & (np.abs(got - exact) <= 1)))

    check(out)
    # the same with the tables PREPARED once (hdrnet_curves_guide_prepare_f32: uniform cells, one table read per channel
    # and pixel instead of a per-workgroup sort + a 4-level search): the same bars against the oracle, and within 5e-7 of
    # the plain path's guide
    prep = ops.curves_guide_prepare(T(shifts, dev), T(slopes, dev))
    assert prep is not None  # the cells separate these knots
    out_p, gout_p = ops.bilateral_slice_apply_io(
        T(grid, dev), traw, guide_curves=tuple(T(a, dev) for a in (ccm, shifts, slopes, mix)),
        input_white_level=wl, out_dtype=getattr(torch, out_dtype), return_guide=True, curves_prepared=prep)
    assert ops.last_kernel().endswith("+curvesguide/cells")
    np.testing.assert_allclose(N(gout_p), guide, rtol=0, atol=2e-6)
    np.testing.assert_allclose(N(gout_p), N(gout), rtol=0, atol=5e-7)
    check(out_p)


@pytest.mark.parametrize("case", ["shuffled", "five_knots", "one_knot", "wide_range", "tie", "cluster"])
def test_curves_prepared_tables_cases(dev, ops, port, case):
    """The prepared cell tables on knot sets other than the reference's initialisation: knots in any order, fewer than 16
    knots, a single knot, a range far from [0, 1]; and the two cases a cell table cannot hold -- two equal knots, two knots
    closer than a cell -- which the set-up call reports (``curves_guide_prepare`` returns None: the caller stays on the plain
    path).  Otherwise: the oracle's guide to 2e-6, the plain path's to 5e-7 x the curve's scale."""
    import oracle
    B, H, W = 1, 24, 128
    rng = np.random.default_rng(len(case))
    grid = T(rng.random((B, 16, 16, 8, 12)).astype(np.float32), dev)
    x = rng.random((B, H, W, 3)).astype(np.float32)
    ccm = (np.concatenate([np.eye(3), np.zeros((3, 1))], 1) + 0.2 * rng.standard_normal((3, 4))).astype(np.float32)
    mix = np.array([0.4, 0.35, 0.25, 0.02], np.float32)
    npts, scale, want_ok = 16, 1.0, True
    shifts = np.tile(np.linspace(0, 1, 16, endpoint=False)[:, None], (1, 3)) + 0.01 * rng.standard_normal((16, 3))
    if case == "shuffled":
        for c in range(3):
            shifts[:, c] = rng.permutation(shifts[:, c])
    elif case == "five_knots":
        npts = 5
        shifts = np.sort(rng.random((5, 3)) * 0.8 + 0.1, axis=0)
        shifts[:, 1] = shifts[::-1, 1]
    elif case == "one_knot":
        npts = 1
        shifts = np.array([[0.1, 0.3, -0.2]])
    elif case == "wide_range":
        scale = 40.0
        shifts = shifts * 40.0 - 7.0
        x = (x * 40.0 - 7.0).astype(np.float32)
    elif case == "tie":
        shifts[5, 1] = shifts[4, 1]
        want_ok = False
    elif case == "cluster":
        shifts[9, 2] = shifts[8, 2] + 1e-4
        want_ok = False
    shifts = shifts.astype(np.float32)
    slopes = (0.3 * rng.standard_normal((npts, 3))).astype(np.float32)
    slopes[0] += 1.0
    if case == "wide_range":
        slopes /= 40.0
    guide = oracle.curves_guide(x, ccm, shifts, slopes, mix)
    assert guide.std() > 0.02  # the clip does not swallow the test
    curves = tuple(T(a, dev) for a in (ccm, shifts, slopes, mix))
    prep = ops.curves_guide_prepare(curves[1], curves[2])
    assert (prep is not None) == want_ok
    out, g = ops.bilateral_slice_apply_io(grid, T(x, dev), guide_curves=curves, return_guide=True)
    assert ops.last_kernel() == "apply_fwd_io/f32->f32+curvesguide"
    if not want_ok:
        return
    out_p, g_p = ops.bilateral_slice_apply_io(grid, T(x, dev), guide_curves=curves, return_guide=True, curves_prepared=prep)
    assert ops.last_kernel() == "apply_fwd_io/f32->f32+curvesguide/cells"
    np.testing.assert_allclose(N(g_p), guide, rtol=0, atol=2e-6)
    np.testing.assert_allclose(N(g_p), N(g), rtol=0, atol=5e-7)
    want = port.bilateral_slice_apply(N(grid), guide, x, True)
    np.testing.assert_allclose(N(out_p), want, rtol=1e-5, atol=1e-5 * max(1.0, float(np.abs(want).max())))
    # the differentiable op refuses a prepared table
    with pytest.raises(ValueError, match="inference-only"):
        ops.bilateral_slice_apply_curves(grid.clone().requires_grad_(True), T(x, dev), *curves, prepared=prep)


def test_prepared_guide_parameters_fuzz(dev, ops):
    """The shipped models' inference calls the guide forwards with parameters PREPARED once per parameter set (round 5).
    Random parameter sets against the exported-arrays path of the same kernels: the prescaled guide network must give
    the same BITS (any width 1 .. 20, weight scales 1e-3 .. 1e3, inputs up to the prescale's x_max); the curves guide's
    cell tables the same guide to 2e-6 of the curve's scale -- when two knots share a cell the set-up call says so (None)."""
    rng = np.random.default_rng(2025)
    B, H, W = 1, 8, 256
    grid6 = np.zeros((B, 4, 4, 8, 3, 4), np.float32)
    grid6[..., :, 3] = ((np.arange(8, dtype=np.float32) + 0.5) / 8)[None, None, None, :, None]  # out == guide (to the tent)
    grid = T(grid6.reshape(B, 4, 4, 8, 12), dev)
    for trial in range(24):
        n = int(rng.integers(1, 21))
        wscale = float(10.0 ** rng.uniform(-3, 3))
        x_max = float(10.0 ** rng.uniform(0, 4))
        conv1 = T((rng.standard_normal((n, 4)) * wscale).astype(np.float32), dev)
        conv2 = T((rng.standard_normal(n + 1) / (wscale * max(x_max, 1.0) * n)).astype(np.float32), dev)
        inp = T((rng.random((B, H, W, 3)) * x_max).astype(np.float32), dev)
        p1, p2 = ops.guide_nn_prescale(conv1, conv2, x_max=x_max)
        _, g = ops.bilateral_slice_apply_nnguide(grid, inp, conv1, conv2, return_guide=True)
        _, gp = ops.bilateral_slice_apply_nnguide(grid, inp, p1, p2, return_guide=True, prescaled=True)
        assert torch.equal(gp, g), (trial, n, wscale, x_max)
    n_ok = 0
    for trial in range(32):
        npts = int(rng.integers(1, 17))
        lo, span = float(rng.uniform(-5, 5)), float(10.0 ** rng.uniform(-2, 2))
        shifts = (lo + span * rng.random((npts, 3))).astype(np.float32)
        if trial % 4 == 3 and npts > 2:  # a cluster / a tie now and then
            shifts[1, trial % 3] = shifts[0, trial % 3] + (0.0 if trial % 8 == 3 else 1e-4 * span)
        slopes = (rng.standard_normal((npts, 3)) / span).astype(np.float32)
        ccm = (np.concatenate([np.eye(3), np.zeros((3, 1))], 1) + 0.2 * rng.standard_normal((3, 4))).astype(np.float32)
        mix = np.array([0.4, 0.35, 0.25, 0.1], np.float32)
        x = (lo - 0.2 * span + 1.4 * span * rng.random((B, H, W, 3))).astype(np.float32)
        curves = tuple(T(a, dev) for a in (ccm, shifts, slopes, mix))
        prep = ops.curves_guide_prepare(curves[1], curves[2])
        if prep is None:
            continue
        n_ok += 1
        out, g = ops.bilateral_slice_apply_io(grid, T(x, dev), guide_curves=curves, return_guide=True)
        out_p, gp = ops.bilateral_slice_apply_io(grid, T(x, dev), guide_curves=curves, return_guide=True, curves_prepared=prep)
        # the guide is clip(mix . curves): compared at the curve's own scale
        scale = float(np.abs(slopes).sum(0).max() * span) + 1.0
        np.testing.assert_allclose(N(gp), N(g), rtol=0, atol=2e-6 * scale, err_msg=f"trial {trial} npts {npts}")
    # both branches were exercised (knots drawn uniformly at random share a cell more often than not -- 16 of them in 63
    # cells collide with probability ~0.85; the reference's knots start equidistant, hdrnet/models.py:150-154)
    assert 4 <= n_ok <= 31


# ---- pyramid output: resize + slice-apply fused with the up-add -------
@pytest.mark.parametrize("case", [(2, 37, 53, 3, 18, 26), (1, 64, 96, 3, 128, 192), (1, 9, 13, 1, 1, 1),
                                  (1, 20, 30, 5, 20, 30)])
def test_resize_bilinear_matches_oracle(dev, ops, case):
    import oracle
    B, Hin, Win, C, Hout, Wout = case
    x = np.random.default_rng(sum(case)).random((B, Hin, Win, C)).astype(np.float32)
    want = oracle.resize_bilinear_align_corners(x, Hout, Wout)
    got = N(ops.resize_bilinear(T(x, dev), Hout, Wout))
    assert ops.last_kernel() == "resize_bilinear_ac"
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-7)  # fma contraction of the three lerps
    ref = torch.nn.functional.interpolate(T(x, dev).permute(0, 3, 1, 2), size=(Hout, Wout), mode="bilinear",
                                          align_corners=True).permute(0, 2, 3, 1)
    np.testing.assert_allclose(got, N(ref), rtol=0, atol=1e-6)


@pytest.mark.parametrize("fused_guide", [False, True])
@pytest.mark.parametrize("case", [(2, 36, 64, 18, 32), (1, 45, 128, 22, 64), (1, 24, 256, 7, 100),
                                  (1, 6, 3840, 4, 1920), (1, 5, 2048, 3, 1000), (1, 4, 1024, 2, 1), (1, 3, 1536, 3, 1536)])
def test_upadd_matches_composed_oracle(dev, ops, port, case, fused_guide):
    """One pyramid level: oracle slice-apply + oracle resize of the coarse level + add, vs the one
    fused kernel (with the guide given as a map, or evaluated in registers from the folded net).  The wide cases have
    several segments per row, a one-column coarse level, a coarse level as wide as the fine one."""
    import oracle
    B, H, W, Hc, Wc = case
    rng = np.random.default_rng(sum(case) + int(fused_guide))
    grid = rng.random((B, 16, 16, 8, 12)).astype(np.float32)
    inp = rng.random((B, H, W, 3)).astype(np.float32)
    coarse = rng.standard_normal((B, Hc, Wc, 3)).astype(np.float32)
    conv1 = (rng.standard_normal((16, 4)) * 0.8).astype(np.float32)
    conv2 = (rng.standard_normal(17) * 0.5).astype(np.float32)
    guide = oracle.pointwise_nn_guide(inp, conv1, conv2) if fused_guide else rng.random((B, H, W)).astype(np.float32)
    want = port.bilateral_slice_apply(grid, guide, inp, True) + oracle.resize_bilinear_align_corners(coarse, H, W)
    if fused_guide:
        got = ops.bilateral_slice_apply_upadd(T(grid, dev), T(inp, dev), T(coarse, dev), guide_conv1=T(conv1, dev),
                                              guide_conv2=T(conv2, dev))
        assert ops.last_kernel() == "apply_fwd_seg/vec4+nnguide+upadd"
        tol = 1e-5
    else:
        got = ops.bilateral_slice_apply_upadd(T(grid, dev), T(inp, dev), T(coarse, dev), guide=T(guide, dev))
        assert ops.last_kernel() == "apply_fwd_seg/vec4+upadd"
        tol = 1e-5
    np.testing.assert_allclose(N(got), want, rtol=tol, atol=tol)


def test_upadd_rejects_unsupported(dev, ops):
    g = torch.rand((1, 8, 8, 4, 12), device=dev)
    x = torch.rand((1, 8, 10, 3), device=dev)  # W % 4 != 0
    with pytest.raises(ValueError):
        ops.bilateral_slice_apply_upadd(g, x, torch.rand((1, 4, 5, 3), device=dev), guide=torch.rand((1, 8, 10), device=dev))
    with pytest.raises(ValueError):  # neither guide nor guide network
        ops.bilateral_slice_apply_upadd(g, torch.rand((1, 8, 8, 3), device=dev), torch.rand((1, 4, 4, 3), device=dev))


@pytest.mark.parametrize("in_dtype,wl", [("uint8", 255.0), ("uint16", 65535.0), ("uint16", 32767.0), ("float32", 1.0)])
@pytest.mark.parametrize("out_dtype", ["uint8", "float32"])
@pytest.mark.parametrize("nn", [False, True])
def test_wire_format_forward(dev, ops, port, in_dtype, wl, out_dtype, nn):
    """uint8 / uint16 input (value / white level, data_pipeline.py:202-232,
    :267-274) and uint8 output (cast(255 * clip(out, 0, 1)), run.py:95) fused into the kernel, with a
    guide map or the fused guide network.  Oracle = the same conversions in float32 numpy around
    the CPU slice-apply.  The uint8 output is compared exactly except where the float result sits
    within 2e-5 * 255 of an integer boundary (at most 1 LSB, on < 0.05 % of the samples)."""
    import oracle
    B, H, W, GH, GW, GD = 2, 40, 96, 16, 16, 8
    rng = np.random.default_rng(17)
    # an affine close to identity so that the output spans [0, 1] and beyond (clip is exercised)
    grid6 = np.zeros((B, GH, GW, GD, 3, 4), np.float32)
    for i in range(3):
        grid6[..., i, i] = 1.0
    grid = (grid6 + 0.15 * rng.standard_normal(grid6.shape)).astype(np.float32).reshape(B, GH, GW, GD, 12)
    if in_dtype == "float32":
        raw = rng.random((B, H, W, 3)).astype(np.float32)
        inp_f = raw
    else:
        hi = 256 if in_dtype == "uint8" else int(wl) + 1
        raw = rng.integers(0, hi, (B, H, W, 3)).astype(in_dtype)
        inp_f = (raw.astype(np.float32) / np.float32(wl)).astype(np.float32)
    conv1 = (rng.standard_normal((16, 4)) * 0.8).astype(np.float32)
    conv2 = (rng.standard_normal(17) * 0.5).astype(np.float32)
    guide = oracle.pointwise_nn_guide(inp_f, conv1, conv2) if nn else rng.random((B, H, W)).astype(np.float32)
    want_f = port.bilateral_slice_apply(grid, guide, inp_f, True)
    t_in = torch.from_numpy(raw.view(np.uint16) if in_dtype == "uint16" else raw).to(dev)
    if in_dtype == "uint16":
        t_in = t_in.view(torch.uint16)
    kw = dict(guide_conv1=T(conv1, dev), guide_conv2=T(conv2, dev)) if nn else dict(guide=T(guide, dev))
    out = ops.bilateral_slice_apply_io(T(grid, dev), t_in, input_white_level=wl,
                                       out_dtype=getattr(torch, out_dtype), **kw)
    assert ops.last_kernel().startswith("apply_fwd_io/")
    tol = 1e-5  # the plain forward's bar, with or without the fused guide network (round 4: it holds)
    if out_dtype == "float32":
        np.testing.assert_allclose(N(out), want_f, rtol=tol, atol=tol)
    else:
        v = 255.0 * np.clip(want_f.astype(np.float64), 0, 1)
        want_u8 = (np.float32(255.0) * np.clip(want_f, 0, 1)).astype(np.uint8)
        got = N(out)
        diff = np.abs(got.astype(np.int16) - want_u8.astype(np.int16))
        near_edge = np.abs(v - np.round(v)) < 255.0 * 2 * tol
        assert diff.max() <= 1
        assert not np.any((diff > 0) & ~near_edge)
        assert (diff > 0).mean() < 5e-4
        assert got.min() == 0 and got.max() == 255  # the clip is exercised on both sides


@pytest.mark.parametrize("n", [16, 8, 4, 12, 5])
@pytest.mark.parametrize("out_dtype", ["uint8", "float32"])
def test_u8_guide_network_guide_itself(dev, ops, port, n, out_dtype):
    """uint8 input + fused guide network: the GUIDE the kernel computes is held to 1e-6 against the numpy restatement
    of the folded network (the bar of the f32 kernel, test_nnguide_fused_matches_composed_oracle), every byte value
    0..255 in every channel present."""
    import oracle
    from hdrnet_amd import _lib
    B, H, W, GH, GW, GD = 2, 24, 128, 16, 16, 8
    rng = np.random.default_rng(100 + n)
    grid6 = np.zeros((B, GH, GW, GD, 3, 4), np.float32)
    for i in range(3):
        grid6[..., i, i] = 1.0
    grid = (grid6 + 0.15 * rng.standard_normal(grid6.shape)).astype(np.float32).reshape(B, GH, GW, GD, 12)
    raw = rng.integers(0, 256, (B, H, W, 3)).astype(np.uint8)
    raw[0, 0, :, 0] = np.arange(W) * 2 % 256          # ramps: every byte value in every channel
    raw[0, 1, :, 1] = (np.arange(W) * 2 + 1) % 256
    raw[0, 2, :, 2] = np.arange(W) * 2 % 256
    raw[0, 3, :, :] = 255
    raw[0, 4, :, :] = 0
    inp_f = (raw.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    conv1 = (rng.standard_normal((n, 4)) * 0.8).astype(np.float32)
    conv2 = (rng.standard_normal(n + 1) * 0.5).astype(np.float32)
    guide = oracle.pointwise_nn_guide(inp_f, conv1, conv2)
    want_f = port.bilateral_slice_apply(grid, guide, inp_f, True)
    kw = dict(input_white_level=255.0, out_dtype=getattr(torch, out_dtype), guide_conv1=T(conv1, dev),
              guide_conv2=T(conv2, dev))
    out, gout = ops.bilateral_slice_apply_io(T(grid, dev), torch.from_numpy(raw).to(dev), return_guide=True, **kw)
    name = _lib.load().hdrnet_last_kernel().decode()
    assert name == f"apply_fwd_io/u8->{'u8' if out_dtype == 'uint8' else 'f32'}+nnguide"
    np.testing.assert_allclose(N(gout), guide, rtol=0, atol=1e-6)
    # inference form (HDRNET_GUIDE_SIGMOID_FAST: v_exp / v_rcp sigmoid)
    out2 = ops.bilateral_slice_apply_io(T(grid, dev), torch.from_numpy(raw).to(dev), fast_sigmoid=True, **kw)
    if out_dtype == "float32":
        np.testing.assert_allclose(N(out), want_f, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(N(out2), want_f, rtol=1e-5, atol=1e-5)
    else:
        want_u8 = (np.float32(255.0) * np.clip(want_f, 0, 1)).astype(np.uint8)
        for got in (N(out), N(out2)):
            diff = np.abs(got.astype(np.int16) - want_u8.astype(np.int16))
            assert diff.max() <= 1 and (diff > 0).mean() < 5e-4


def test_nnguide_rejects_unsupported(dev, ops):
    from hdrnet_amd import _lib
    g = torch.rand((1, 4, 4, 4, 12), device=dev)
    with pytest.raises(_lib.HdrnetInvalidArgument):   # W % 4 != 0
        ops.bilateral_slice_apply_nnguide(g, torch.rand((1, 8, 10, 3), device=dev), torch.rand((16, 4), device=dev),
                                          torch.rand((17,), device=dev))
    with pytest.raises(ValueError, match="guide_conv1"):
        ops.bilateral_slice_apply_nnguide(g, torch.rand((1, 8, 8, 3), device=dev), torch.rand((16, 3), device=dev),
                                          torch.rand((17,), device=dev))


# ---- layers.py wrappers (6-D grids) -----------------------------------------------------------------
def test_layers_6d(dev, ops, port):
    from hdrnet_amd import layers
    rng = np.random.default_rng(11)
    B, H, W, GH, GW, GD, n_out, n_in = 2, 20, 24, 4, 5, 6, 3, 4
    grid6 = rng.random((B, GH, GW, GD, n_out, n_in)).astype(np.float32)
    guide = rng.random((B, H, W)).astype(np.float32)
    inp = rng.random((B, H, W, n_in - 1)).astype(np.float32)
    want = port.bilateral_slice_apply(grid6.reshape(B, GH, GW, GD, n_out * n_in), guide, inp, True)
    got = N(layers.bilateral_slice_apply(T(grid6, dev), T(guide, dev), T(inp, dev), has_offset=True, name="slice"))
    np.testing.assert_allclose(got, want, rtol=FWD_RTOL, atol=FWD_ATOL)
    # hdrnet/test/ops_test.py:345-365: has_offset True -> 3 channels, False -> 4 from a 12-ch grid
    inp4 = rng.random((B, H, W, 3)).astype(np.float32)
    g12 = T(grid6.reshape(B, GH, GW, GD, 12), dev)
    assert layers.bilateral_slice_apply(g12, T(guide, dev), T(inp4, dev), has_offset=True).shape[-1] == 3
    assert layers.bilateral_slice_apply(g12, T(guide, dev), T(inp4, dev), has_offset=False).shape[-1] == 4
    # layers.bilateral_slice on a 6-D grid: [B,H,W,n_out,n_in] with channel order j*n_out+i inside
    s = N(layers.bilateral_slice(T(grid6, dev), T(guide, dev)))
    assert s.shape == (B, H, W, n_out, n_in)
    flat = np.concatenate([grid6[..., j] for j in range(n_in)], axis=4)
    want_s = port.bilateral_slice(flat, guide).reshape(B, H, W, n_in, n_out).transpose(0, 1, 2, 4, 3)
    np.testing.assert_allclose(s, want_s, rtol=FWD_RTOL, atol=FWD_ATOL)


# ---- full-size frames: size-independent properties (the oracle takes seconds there) ----------------
FULL = [(1080, 1920, 16, 16), (2160, 3840, 16, 16), (3000, 4000, 32, 32)]  # configs #2, #3, #5


@pytest.mark.parametrize("H,W,GH,GW", FULL)
def test_full_frame_identity_grid_returns_input(dev, ops, H, W, GH, GW):
    """A grid holding the identity affine [I | 0] in every cell must return the input for ANY
    guide -- up to the 0.9999 peak of the smoothed tent (numerics.h:108-113): the two z-weights
    sum to 1 - O(1e-8) away from exact cell centres, so out == input to ~1e-6 relative."""
    g = torch.zeros((1, GH, GW, 8, 3, 4), device=dev)
    for i in range(3):
        g[..., i, i] = 1.0
    gen = torch.Generator(device=dev).manual_seed(1234)
    guide = torch.rand((1, H, W), device=dev, generator=gen)
    inp = torch.rand((1, H, W, 3), device=dev, generator=gen)
    out = ops.bilateral_slice_apply(g.reshape(1, GH, GW, 8, 12), guide, inp, has_offset=True)
    assert ops.last_kernel() == "apply_fwd_seg/vec4"
    err = (out - inp).abs().max().item()
    assert err < 2.5e-4, err  # bound: |in| * (1 - (wz0 + wz1)) <= 1e-4-ish at cell centres
    frac = ((out - inp).abs() > 1e-5).float().mean().item()
    assert frac < 2e-3, frac  # only pixels within ~1e-3 of a cell centre in z see the dip


@pytest.mark.parametrize("H,W,GH,GW", FULL)
def test_full_frame_fast_equals_generic(dev, ops, H, W, GH, GW):
    """Fast (LDS-staged) vs generic (bit-exact-to-reference) kernel on the whole frame."""
    gen = torch.Generator(device=dev).manual_seed(4321)
    grid = torch.rand((1, GH, GW, 8, 12), device=dev, generator=gen)
    guide = torch.rand((1, H, W), device=dev, generator=gen) * 1.1 - 0.05
    inp = torch.rand((1, H, W, 3), device=dev, generator=gen)
    with ops.kernel_override("generic"):
        a = ops.bilateral_slice_apply(grid, guide, inp, has_offset=True)
    b = ops.bilateral_slice_apply(grid, guide, inp, has_offset=True)
    assert ops.last_kernel() == "apply_fwd_seg/vec4"
    torch.testing.assert_close(b, a, rtol=FWD_RTOL, atol=FWD_ATOL)
    print(f"{H}x{W}: max|fast-generic| = {(a - b).abs().max().item():.3e}")


def test_full_frame_rows_vs_oracle(dev, ops, port):
    """A horizontal band of a 4K frame against the oracle: the band is computed as a full-height
    problem on the GPU, and on the CPU from the same rows (the op is row-separable given H)."""
    H, W = 2160, 3840
    rng = np.random.default_rng(99)
    grid = rng.random((1, 16, 16, 8, 12)).astype(np.float32)
    guide = rng.random((1, H, W)).astype(np.float32)
    inp = rng.random((1, H, W, 3)).astype(np.float32)
    got = N(ops.bilateral_slice_apply(T(grid, dev), T(guide, dev), T(inp, dev), has_offset=True))
    port.set_threads(0)
    want = port.bilateral_slice_apply(grid, guide, inp, True)
    np.testing.assert_allclose(got, want, rtol=FWD_RTOL, atol=FWD_ATOL)
    worst = float(np.max(np.abs(got - want) / (REF_BAR + REF_BAR * np.abs(want))))
    print(f"4K vs oracle: max|err|={np.abs(got - want).max():.3e}, worst/(1e-6 bar)={worst:.2f}")


def test_linearity_in_grid_full_frame(dev, ops):
    H, W = 1080, 1920
    gen = torch.Generator(device=dev).manual_seed(7)
    g1 = torch.rand((1, 16, 16, 8, 12), device=dev, generator=gen)
    g2 = torch.rand((1, 16, 16, 8, 12), device=dev, generator=gen)
    guide = torch.rand((1, H, W), device=dev, generator=gen)
    inp = torch.rand((1, H, W, 3), device=dev, generator=gen)
    f = lambda g: ops.bilateral_slice_apply(g, guide, inp, has_offset=True)  # noqa: E731
    torch.testing.assert_close(f(g1 + 2 * g2), f(g1) + 2 * f(g2), rtol=1e-5, atol=2e-5)


# ---- streams, batching, error paths ---------------------------------------------------------------
def test_non_default_stream_and_batch(dev, ops, port):
    rng = np.random.default_rng(3)
    grid, guide, inp, _ = rand_case(rng, 4, 32, 64, 8, 8, 8, 3, 3, True)
    want = port.bilateral_slice_apply(grid, guide, inp, True)
    s = torch.cuda.Stream(device=dev)
    tg, tgu, ti = T(grid, dev), T(guide, dev), T(inp, dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        out = ops.bilateral_slice_apply(tg, tgu, ti, has_offset=True)
    s.synchronize()
    np.testing.assert_allclose(N(out), want, rtol=FWD_RTOL, atol=FWD_ATOL)
    # batch elements are independent: per-image calls agree with the batched call
    for b in range(4):
        o = ops.bilateral_slice_apply(tg[b:b + 1], tgu[b:b + 1], ti[b:b + 1], has_offset=True)
        assert torch.equal(o[0], out[b])


def test_empty_batch(dev, ops):
    out = ops.bilateral_slice_apply(torch.rand((0, 4, 4, 4, 12), device=dev), torch.rand((0, 8, 8), device=dev),
                                    torch.rand((0, 8, 8, 3), device=dev), has_offset=True)
    assert tuple(out.shape) == (0, 8, 8, 3)
    out = ops.bilateral_slice(torch.rand((2, 4, 4, 4, 5), device=dev), torch.rand((2, 0, 8), device=dev))
    assert tuple(out.shape) == (2, 0, 8, 5)


def test_non_contiguous_inputs(dev, ops, port):
    rng = np.random.default_rng(8)
    grid, guide, inp, _ = rand_case(rng, 1, 24, 32, 4, 4, 4, 3, 3, True)
    want = port.bilateral_slice_apply(grid, guide, inp, True)
    ti = T(np.ascontiguousarray(inp.transpose(0, 3, 1, 2)), dev).permute(0, 2, 3, 1)  # NCHW storage
    assert not ti.is_contiguous()
    got = N(ops.bilateral_slice_apply(T(grid, dev), T(guide, dev), ti, has_offset=True))
    np.testing.assert_allclose(got, want, rtol=FWD_RTOL, atol=FWD_ATOL)


def test_misaligned_buffers_take_the_scalar_kernels(dev, ops, port):
    """Dense tensors whose storage starts 4 B off a 16-B boundary (a view into a larger buffer):
    the 16-byte-access kernels are not eligible; forward and backward must still be right."""
    rng = np.random.default_rng(9)
    B, H, W = 1, 24, 64
    grid, guide, inp, dout = rand_case(rng, B, H, W, 8, 8, 8, 3, 3, True)
    want = port.bilateral_slice_apply(grid, guide, inp, True)
    wg, wgu, wi = port.bilateral_slice_apply_grad(grid, guide, inp, dout, True)

    def off1(a):  # same values, data pointer = base + 4 bytes
        buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
        v = buf[1:].view(*a.shape)
        v.copy_(torch.from_numpy(a))
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v

    tg = T(grid, dev).requires_grad_(True)
    tgu = off1(guide).requires_grad_(True)
    ti = off1(inp).requires_grad_(True)
    out = ops.bilateral_slice_apply(tg, tgu, ti, has_offset=True)
    assert ops.last_kernel() == "apply_fwd_rows/scalar"
    np.testing.assert_allclose(N(out), want, rtol=FWD_RTOL, atol=FWD_ATOL)
    out.backward(off1(dout))
    grads_close(N(tg.grad), wg, "dgrid")
    grads_close(N(tgu.grad), wgu, "dguide")
    grads_close(N(ti.grad), wi, "dinput")


def test_wild_guide_values_fast_equals_generic(dev, ops):
    """Guides far outside [0, 1] (|guide * GD| beyond 2^23, where f32 rounding makes a corner offset 2):
    the fast kernels keep the reference's max(., 0) on the z tent, so they agree with the generic
    (bit-exact-to-reference) kernels instead of applying a weight of -1."""
    gen = torch.Generator(device=dev).manual_seed(3)
    B, H, W = 1, 16, 256
    grid = torch.rand((B, 16, 16, 8, 12), device=dev, generator=gen)
    inp = torch.rand((B, H, W, 3), device=dev, generator=gen)
    vals = torch.tensor([1e8, -1e8, 3.1e7, -3.1e7, 2.0 ** 21, 2.0 ** 21 + 0.25, 2.0 ** 20 + 0.125, 1.0e6 + 0.3,
                         -5.0, 7.5, 1.0, 0.0, 2097151.9, 1048576.06, 12345678.0, -2.0 ** 22], device=dev)
    guide = vals.repeat(B * H * W // vals.numel()).reshape(B, H, W).contiguous()
    outs = {}
    for which in ("generic", "fast"):
        with ops.kernel_override(which):
            outs[which] = ops.bilateral_slice_apply(grid, guide, inp, has_offset=True)
    assert torch.isfinite(outs["fast"]).all()
    torch.testing.assert_close(outs["fast"], outs["generic"], rtol=1e-5, atol=1e-5)
    with ops.kernel_override("generic"):
        want = ops.bilateral_slice(grid, guide)
    got = ops.bilateral_slice(grid, guide)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("want_dgrid", [True, False])
def test_wild_guide_values_gradients_fast_equal_generic(dev, ops, want_dgrid):
    """The same wild guides through the VJPs: a z tap whose smoothed |dz| exceeds 1 has weight AND derivative 0
    (numerics.h:108-126), far-out guides clamp both taps onto an edge plane.  Both fast per-pixel paths carry their own
    handling of it -- the fused pass (grid_grad_mfma.hip: a wave-uniform branch on a ballot) and apply_vjp_seg (per-lane
    selects, round 6) -- and the dgrid contraction forces the edge half cells to weight 1 (bilateral_slice_apply.cc:121-125);
    all against the generic kernels, which are the reference's arithmetic."""
    gen = torch.Generator(device=dev).manual_seed(5)
    B, H, W, GD = 1, 64, 256, 8
    grid = torch.rand((B, 16, 16, GD, 12), device=dev, generator=gen)
    inp = torch.rand((B, H, W, 3), device=dev, generator=gen)
    dout = torch.randn((B, H, W, 3), device=dev, generator=gen)
    vals = torch.tensor([1e8, -1e8, 3.1e7, -3.1e7, 2.0 ** 21, 2.0 ** 21 + 0.25, 2.0 ** 20 + 0.125, 1.0e6 + 0.3,
                         -5.0, 7.5, 1.0, 0.0, 2097151.9, 1048576.06, 12345678.0, -2.0 ** 22,
                         0.5, 0.0625, 0.9375, 0.31, 0.999999, 1e-7, 0.4375, 0.5625], device=dev)
    guide = vals.repeat(-(-B * H * W // vals.numel()))[:B * H * W].reshape(B, H, W).contiguous()
    res = {}
    for which in ("generic", "fast"):
        tg = grid.clone().requires_grad_(want_dgrid)
        tgu, ti = guide.clone().requires_grad_(True), inp.clone().requires_grad_(True)
        with ops.kernel_override(which):
            ops.bilateral_slice_apply(tg, tgu, ti, has_offset=True).backward(dout)
            res[which] = (tg.grad, tgu.grad, ti.grad, ops.last_kernel())
    assert res["fast"][3] == ("apply_bwd_fused/mfma" if want_dgrid else "apply_vjp_seg/vec4"), res["fast"][3]
    for k, nm, atol in ((1, "dguide", 2e-5), (2, "dinput", 1e-5)):
        a, b = res["fast"][k], res["generic"][k]
        assert torch.isfinite(a).all(), nm
        print(f"wild guides, dgrid {want_dgrid}: {nm} max|fast - generic| = {float((a - b).abs().max()):.3e} on values up to "
              f"{float(b.abs().max()):.3g}")
        torch.testing.assert_close(a, b, rtol=1e-4, atol=atol)
    if want_dgrid:
        a, b = res["fast"][0], res["generic"][0]
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5 * float(b.abs().max()))


def test_fast_flag_rejects_unsupported_shape(dev, ops):
    from hdrnet_amd import _lib
    with ops.kernel_override("fast"):
        with pytest.raises(_lib.HdrnetInvalidArgument):
            ops.bilateral_slice_apply(torch.rand((1, 4, 4, 4, 15), device=dev), torch.rand((1, 8, 8), device=dev),
                                      torch.rand((1, 8, 8, 2), device=dev), has_offset=True)


# ---- the reference's optimisation-convergence test (hdrnet/test/ops_test.py:189-230), shortened ------
def test_grid_optimisation_converges(dev, ops):
    """SGD on the grid only, fitting a sine along a 1 x W strip; the reference runs 10 000 steps to
    SSE < 0.0085 -- here the loss must fall by > 50x in 400 steps (same mechanics, CI-sized)."""
    torch.manual_seed(0)
    W, GD = 100, 8
    x = torch.linspace(0, 1, W, device=dev)
    target = (0.5 + 0.4 * torch.sin(2 * np.pi * x)).reshape(1, 1, W, 1)
    guide = x.reshape(1, 1, W).contiguous()
    grid = (torch.rand((1, 1, 1, GD, 1), device=dev) * 0.1).requires_grad_(True)
    opt = torch.optim.SGD([grid], lr=0.02)
    first = None
    for _ in range(400):
        opt.zero_grad()
        loss = ((ops.bilateral_slice(grid, guide) - target) ** 2).sum()
        loss.backward()
        opt.step()
        first = loss.item() if first is None else first
    assert loss.item() < first / 50, (first, loss.item())
