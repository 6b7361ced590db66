"""Pins the CPU oracle (oracle/) before anything is compared against it.

1. oracle port (C99 restatement)  ==  golden fixtures made from the reference's own
   CPU code (tests/golden/make_golden.py), BIT-EXACT, all seven functions.
2. oracle port == oracle/_ref (the compiled reference) bit-exact on extra random
   shapes, when the compiled reference is present.
3. The reference's known-answer test (hdrnet/test/ops_test.py:61-86).
4. The numpy restatement of jax/bilateral_slice.py == the op at the reference's own
   JAX-vs-op bar (assertAllClose defaults, hdrnet_ops_jax_tf2_test.py:48).
5. The reference's finite-difference gradient checks, with its extents and thresholds
   (hdrnet_ops_test.py:139-210, :319-408), re-hosted on the oracle.
6. Adjointness <GridGrad(u), g> == <u, Apply(g)> (grid-linearity of the op).
"""
import os
import numpy as np
import pytest

from conftest import golden_names, load_golden


# ---- 1. golden fixtures ------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names("apply_"))
def test_port_matches_golden_apply(port, name):
    g = load_golden(name)
    ho = bool(g["has_offset"])
    out = port.bilateral_slice_apply(g["grid"], g["guide"], g["input"], ho)
    assert np.array_equal(out, g["out"])
    dgrid, dguide, dinput = port.bilateral_slice_apply_grad(g["grid"], g["guide"], g["input"], g["dout"], ho)
    assert np.array_equal(dgrid, g["dgrid"])
    assert np.array_equal(dguide, g["dguide"])
    assert np.array_equal(dinput, g["dinput"])


@pytest.mark.parametrize("name", golden_names("slice_"))
def test_port_matches_golden_slice(port, name):
    g = load_golden(name)
    assert np.array_equal(port.bilateral_slice(g["grid"], g["guide"]), g["out"])
    dgrid, dguide = port.bilateral_slice_grad(g["grid"], g["guide"], g["dout"])
    assert np.array_equal(dgrid, g["dgrid"])
    assert np.array_equal(dguide, g["dguide"])


def test_port_threads_do_not_change_results(port):
    g = load_golden("apply_forward_default")
    n = port.set_threads(1)
    a = port.bilateral_slice_apply(g["grid"], g["guide"], g["input"], True)
    port.set_threads(4)
    b = port.bilateral_slice_apply(g["grid"], g["guide"], g["input"], True)
    port.set_threads(n)
    assert np.array_equal(a, b)


# ---- 2. against the compiled reference ------------------------------------------------------
SHAPES = [  # B, H, W, GH, GW, GD, Cin, Cout, has_offset
    (1, 1, 1, 1, 1, 1, 1, 1, True),
    (2, 5, 7, 3, 2, 4, 3, 3, True),
    (1, 33, 65, 16, 16, 8, 3, 3, True),
    (2, 9, 4, 12, 12, 8, 1, 3, True),
    (1, 16, 16, 2, 2, 1, 4, 2, False),
    (1, 40, 24, 5, 3, 2, 2, 5, True),
]


@pytest.mark.parametrize("shape", SHAPES)
def test_port_matches_compiled_reference(port, ref_or_none, shape):
    """Bit-exact against the compiled reference's outputs on these shapes, stored in tests/golden/ref_shapes.npz
    (tests/golden/make_golden.py), everywhere; and against oracle/_ref itself on the same inputs where it is built."""
    ho = shape[-1]
    key = "x".join(str(int(v)) for v in shape) + "/"
    g = {k[len(key):]: v for k, v in load_golden("ref_shapes").items() if k.startswith(key)}
    grid, guide, inp, dout = g["grid"], g["guide"], g["input"], g["dout"]
    out = port.bilateral_slice_apply(grid, guide, inp, ho)
    grads = port.bilateral_slice_apply_grad(grid, guide, inp, dout, ho)
    assert np.array_equal(out, g["out"])
    for a, name in zip(grads, ("dgrid", "dguide", "dinput")):
        assert np.array_equal(a, g[name]), name
    sliced = port.bilateral_slice(grid, guide)
    slice_grads = port.bilateral_slice_grad(grid, guide, g["slice_dout"])
    assert np.array_equal(sliced, g["slice_out"])
    for a, name in zip(slice_grads, ("slice_dgrid", "slice_dguide")):
        assert np.array_equal(a, g[name]), name
    R = ref_or_none
    if R is not None:
        assert np.array_equal(out, R.bilateral_slice_apply(grid, guide, inp, ho))
        for a, b in zip(grads, R.bilateral_slice_apply_grad(grid, guide, inp, dout, ho)):
            assert np.array_equal(a, b)
        assert np.array_equal(sliced, R.bilateral_slice(grid, guide))
        for a, b in zip(slice_grads, R.bilateral_slice_grad(grid, guide, g["slice_dout"])):
            assert np.array_equal(a, b)


def test_apply_equals_slice_plus_matmul(port):
    # bilateral_slice_apply.h:22-29: the fused op == slice -> reshape (Cout x Cj) -> per-pixel multiply
    g = load_golden("apply_forward_default")
    sliced = port.bilateral_slice(g["grid"], g["guide"])  # [B,H,W,12]
    B, H, W, _ = sliced.shape
    m = sliced.reshape(B, H, W, 3, 4)
    ref = np.zeros((B, H, W, 3), np.float32)
    for i in range(3):
        v = np.zeros((B, H, W), np.float32)
        for j in range(4):
            v = v + (m[..., i, j] * g["input"][..., j] if j < 3 else m[..., i, j])
        ref[..., i] = v
    assert np.array_equal(port.bilateral_slice_apply(g["grid"], g["guide"], g["input"], True), ref)


# ---- 3. known-answer test ---------------------------------------------------------------------
def test_interpolate_known_answer(port):
    """hdrnet/test/ops_test.py:61-86: depth planes 0,1,2 sliced at (val+0.5)/d return val +- 5e-4."""
    k = load_golden("slice_interpolate_kat")
    d = 3
    for val in range(d):
        guide = (((val + 0.5) / (1.0 * d)) * np.ones((3, 5, 9))).astype(np.float32)
        out = port.bilateral_slice(k["grid"], guide)
        assert list(out.shape) == [3, 5, 9, 1]
        assert np.amax(np.abs(val - out)) < 5e-4
        assert np.array_equal(out, k["outs"][val])
    # The smoothed tent peaks at 1 - sqrt(1e-8) = 0.9999, not 1 (numerics.h:108-113): the
    # answer for val=2 sits 2e-4 low; a plain-lerp implementation would return exactly 2.
    assert abs(float(k["outs"][2].max()) - (2.0 - 2.0e-4)) < 2e-6


# ---- 4. JAX twin -------------------------------------------------------------------------------
def test_jax_numpy_restatement_matches_op():
    from oracle import jax_np as J
    g = load_golden("slice_jax_shape_small")
    out = J.batched(J.bilateral_slice, g["grid"], g["guide"])
    np.testing.assert_allclose(out, g["out"], rtol=1e-6, atol=1e-6)
    B = g["grid"].shape[0]
    dguide = np.stack([J.bilateral_slice_guide_vjp(g["grid"][b], g["guide"][b], g["dout"][b]) for b in range(B)])
    np.testing.assert_allclose(dguide, g["dguide"], rtol=1e-5, atol=1e-5)
    dgrid = np.stack([J.bilateral_slice_grid_vjp(g["guide"][b], g["dout"][b], g["grid"][b].shape)
                      for b in range(B)])
    np.testing.assert_allclose(dgrid, g["dgrid"], rtol=1e-5, atol=1e-5 * np.abs(g["dgrid"]).max())


def test_jax_config1_plumbing(port):
    """BASELINE.json configs[0]: bilateral_slice 256x256, 16x16x8 grid (unbatched JAX API) on CPU."""
    from oracle import jax_np as J
    rng = np.random.default_rng(1234)
    grid = rng.random((16, 16, 8, 12), dtype=np.float32)
    guide = rng.random((256, 256), dtype=np.float32)
    out = J.bilateral_slice(grid, guide)
    assert out.shape == (256, 256, 12)
    np.testing.assert_allclose(out, port.bilateral_slice(grid[None], guide[None])[0], rtol=1e-6, atol=1e-6)


# ---- 5. the reference's finite-difference gradient checks --------------------------------------
def _max_fd_error(f, x, analytic_vjp_rows, delta):
    """tf.test.compute_gradient_error: max |J_analytic - J_numeric| over the full Jacobian.
    analytic_vjp_rows(k) returns d out_flat[k] / d x (shape of x)."""
    x = x.copy()
    y0 = f(x).ravel()
    num = np.zeros((x.size, y0.size), np.float64)
    flat = x.ravel()
    for i in range(flat.size):
        old = flat[i]
        flat[i] = old + delta
        yp = f(x).ravel().astype(np.float64)
        flat[i] = old - delta
        ym = f(x).ravel().astype(np.float64)
        flat[i] = old
        num[i] = (yp - ym) / (2 * delta)
    ana = np.stack([analytic_vjp_rows(k).ravel() for k in range(y0.size)], axis=1)
    return np.abs(ana - num).max()


def _fd_case(port, B, H, W, Cin, GH, GW, GD, Cout, wrt, apply, delta, thresh):
    rng = np.random.RandomState(7)
    Cj = Cin + 1
    C = Cout * Cj
    grid = rng.rand(B, GH, GW, GD, C).astype(np.float32)
    guide = rng.rand(B, H, W).astype(np.float32)
    # The trilinear tent is not differentiable where guide*GD crosses a half-integer; the
    # reference's (unseeded) random test only passes when no sample lies within `delta` of
    # such a kink.  Make that deterministic: keep every sample >= 0.1 cell away from one.
    t = guide.astype(np.float64) * GD - 0.5
    frac = t - np.floor(t)
    guide = ((np.floor(t) + np.clip(frac, 0.1, 0.9) + 0.5) / GD).astype(np.float32)
    inp = rng.rand(B, H, W, Cin).astype(np.float32)
    oshape = (B, H, W, Cout if apply else C)

    def fwd(g=grid, gu=guide, i=inp):
        return port.bilateral_slice_apply(g, gu, i, True) if apply else port.bilateral_slice(g, gu)

    def rows(k):
        d = np.zeros(oshape, np.float32)
        d.ravel()[k] = 1.0
        if apply:
            gs = port.bilateral_slice_apply_grad(grid, guide, inp, d, True)
            return {"grid": gs[0], "guide": gs[1], "input": gs[2]}[wrt]
        gs = port.bilateral_slice_grad(grid, guide, d)
        return {"grid": gs[0], "guide": gs[1]}[wrt]

    x = {"grid": grid, "guide": guide, "input": inp}[wrt]
    f = {"grid": lambda v: fwd(g=v), "guide": lambda v: fwd(gu=v), "input": lambda v: fwd(i=v)}[wrt]
    err = _max_fd_error(f, x, rows, delta)
    assert err < thresh, err


def test_fd_slice_grid_gradient(port):      # hdrnet_ops_test.py:183-195, delta 1e-4, err < 3e-3
    _fd_case(port, 3, 8, 5, 3, 6, 3, 7, 4, "grid", False, 1e-4, 3e-3)


def test_fd_slice_guide_gradient(port):     # hdrnet_ops_test.py:198-210
    _fd_case(port, 1, 6, 18, 1, 3, 9, 7, 1, "guide", False, 1e-4, 3e-3)


def test_fd_apply_grid_gradient(port):      # hdrnet_ops_test.py:366-378, default delta 1e-3, err < 1e-2
    _fd_case(port, 3, 8, 5, 3, 6, 3, 7, 4, "grid", True, 1e-3, 1e-2)


def test_fd_apply_guide_gradient(port):     # hdrnet_ops_test.py:380-393
    _fd_case(port, 1, 6, 18, 1, 3, 9, 7, 1, "guide", True, 1e-3, 1e-2)


def test_fd_apply_input_gradient(port):     # hdrnet_ops_test.py:396-408
    _fd_case(port, 3, 8, 5, 3, 6, 3, 7, 4, "input", True, 1e-3, 1e-2)


# ---- 6. adjointness ------------------------------------------------------------------------------
def test_grid_grad_is_adjoint_of_apply(port):
    g = load_golden("apply_guide_out_of_range")
    ho = bool(g["has_offset"])
    u = g["dout"].astype(np.float64)
    out = port.bilateral_slice_apply(g["grid"], g["guide"], g["input"], ho).astype(np.float64)
    dgrid, _, dinput = port.bilateral_slice_apply_grad(g["grid"], g["guide"], g["input"], g["dout"], ho)
    lhs = float((dgrid.astype(np.float64) * g["grid"]).sum())   # <A^T u, g>
    rhs = float((u * out).sum())                                 # <u, A g>
    assert abs(lhs - rhs) <= 2e-5 * abs(rhs)
    # input-linearity: <dinput, in> + offset part == <u, out>
    zero_in = np.zeros_like(g["input"])
    off = port.bilateral_slice_apply(g["grid"], g["guide"], zero_in, ho).astype(np.float64)
    lhs2 = float((dinput.astype(np.float64) * g["input"]).sum() + (u * off).sum())
    assert abs(lhs2 - rhs) <= 2e-5 * abs(rhs)


# ---- the TF bilinear resize (align_corners) restatement used by the pyramid tests ------------------
@pytest.mark.parametrize("size", [(18, 26), (74, 106), (37, 53), (1, 1), (5, 200)])
def test_resize_restatement_matches_torch_align_corners(size):
    """tensorflow is not vendored by the reference (requirements.txt pins tensorflow_gpu==2.12.0);
    the restatement of its legacy align_corners bilinear resize is pinned against the one
    independent implementation available here, torch's F.interpolate(align_corners=True), and
    against the closed forms below."""
    import torch
    import torch.nn.functional as F
    import oracle
    x = np.random.default_rng(7).random((2, 37, 53, 3), dtype=np.float32)
    got = oracle.resize_bilinear_align_corners(x, *size)
    want = F.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=size, mode="bilinear",
                         align_corners=True).permute(0, 2, 3, 1).numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-7)


def test_resize_restatement_closed_forms():
    import oracle
    rng = np.random.default_rng(8)
    x = rng.random((1, 9, 13, 2), dtype=np.float32)
    assert np.array_equal(oracle.resize_bilinear_align_corners(x, 9, 13), x)  # identity
    # corners are preserved (align_corners) and a 2x up-sampling of size 2n-1 interleaves exactly
    up = oracle.resize_bilinear_align_corners(x, 17, 25)
    assert np.array_equal(up[:, ::2, ::2], x)
    np.testing.assert_allclose(up[:, 1::2, ::2], 0.5 * (x[:, :-1] + x[:, 1:]), rtol=0, atol=1e-7)
    # a linear ramp is reproduced by bilinear interpolation
    yy, xx = np.meshgrid(np.linspace(0, 1, 9, dtype=np.float32), np.linspace(0, 2, 13, dtype=np.float32), indexing="ij")
    ramp = (0.25 + 0.5 * yy + 0.125 * xx)[None, :, :, None].astype(np.float32)
    y2, x2 = np.meshgrid(np.linspace(0, 1, 20, dtype=np.float32), np.linspace(0, 2, 31, dtype=np.float32), indexing="ij")
    want = (0.25 + 0.5 * y2 + 0.125 * x2)[None, :, :, None]
    np.testing.assert_allclose(oracle.resize_bilinear_align_corners(ramp, 20, 31), want, rtol=0, atol=2e-6)


def test_curves_guide_restatement_closed_forms():
    """oracle.curves_guide (HDRNetCurves._guide, hdrnet/models.py:145-190): with the reference's
    initial parameters (identity ccm, slope 1 on the first knot only, mix = 1/3) the guide is the
    channel mean of the input; and it is piecewise linear with kinks exactly at the shifts."""
    import oracle
    rng = np.random.default_rng(3)
    x = rng.random((2, 6, 7, 3), dtype=np.float32)
    ccm = np.concatenate([np.eye(3, dtype=np.float32), np.zeros((3, 1), np.float32)], axis=1)
    shifts = np.tile(np.linspace(0, 1, 16, endpoint=False, dtype=np.float32)[:, None], (1, 3))
    slopes = np.zeros((16, 3), np.float32)
    slopes[0] = 1.0
    mix = np.array([1 / 3, 1 / 3, 1 / 3, 0.0], np.float32)
    np.testing.assert_allclose(oracle.curves_guide(x, ccm, shifts, slopes, mix), x.mean(-1), rtol=0, atol=1e-6)
    # one active channel, slopes (1, -1 at shift 0.5): a tent rising to 0.5 then flat
    slopes2 = np.zeros((16, 3), np.float32)
    slopes2[0, 0], slopes2[8, 0] = 1.0, -1.0
    mix2 = np.array([1.0, 0.0, 0.0, 0.0], np.float32)
    g = oracle.curves_guide(x, ccm, shifts, slopes2, mix2)
    np.testing.assert_allclose(g, np.minimum(x[..., 0], 0.5), rtol=0, atol=1e-6)
    # clip
    mix3 = np.array([4.0, 0.0, 0.0, -1.0], np.float32)
    g = oracle.curves_guide(x, ccm, shifts, slopes, mix3)
    np.testing.assert_allclose(g, np.clip(4 * x[..., 0] - 1, 0, 1), rtol=0, atol=1e-6)


# ---- the guide restatements vs the reference's OWN second implementation: its GL shaders ------------
def _export_curves(rng):
    """Random curves-guide variables pushed through hdrnet/bin/freeze_graph.py:107-127's export code
    (restated line by line) -> the four flat files the renderer loads."""
    ccm_ = (np.identity(3) + 0.2 * rng.standard_normal((3, 3))).astype(np.float32)     # 'inference/guide/ccm'
    ccm_bias_ = (0.1 * rng.standard_normal(3)).astype(np.float32)
    shifts_ = np.tile(np.linspace(0, 1, 16, endpoint=False, dtype=np.float32)[None, None, None, :], (1, 1, 3, 1))
    shifts_ = (shifts_ + 0.02 * rng.standard_normal(shifts_.shape)).astype(np.float32)  # [1, 1, nchans, npts]
    slopes_ = (0.3 * rng.standard_normal((1, 1, 1, 3, 16))).astype(np.float32)
    mixing_weights_ = rng.standard_normal((1, 1, 3, 1)).astype(np.float32)
    mixing_bias_ = rng.standard_normal(1).astype(np.float32)
    shifts_ = np.squeeze(shifts_).astype(np.float32)                                    # [3, 16]
    slopes_ = np.squeeze(slopes_).astype(np.float32)
    mix_matrix_dump = np.append(np.squeeze(mixing_weights_), mixing_bias_[0]).astype(np.float32)
    ccm34_ = np.vstack((ccm_, ccm_bias_[np.newaxis, :]))                                # [4, 3]
    files = dict(ccm=np.ascontiguousarray(ccm34_.T).ravel(), shifts=np.ascontiguousarray(shifts_.T).ravel(),
                 slopes=np.ascontiguousarray(slopes_.T).ravel(), mix=mix_matrix_dump.ravel())
    return {k: v.astype(np.float32) for k, v in files.items()}


def test_curves_guide_restatement_equals_std_frag():
    """oracle.curves_guide (numpy restatement of hdrnet/models.py:145-190 on the exported layout) ==
    the transliterated benchmark/assets/std.frag:36-45 on the same FILES (renderer.cc:203-223)."""
    import oracle
    from oracle import gl_shaders
    rng = np.random.default_rng(17)
    f = _export_curves(rng)
    px = rng.random((64, 3)).astype(np.float32) * 1.2 - 0.1
    want = np.array([gl_shaders.std_frag_guide(p, f["ccm"], f["shifts"], f["slopes"], f["mix"]) for p in px])
    got = oracle.curves_guide(px[None, None], f["ccm"].reshape(3, 4), f["shifts"].reshape(16, 3),
                              f["slopes"].reshape(16, 3), f["mix"])[0, 0]
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)


def test_pointwise_nn_guide_restatement_equals_gpyrnn_frag():
    """oracle.pointwise_nn_guide (hdrnet/models.py:203-210 folded as freeze_graph.py:129-184) == the
    transliterated benchmark/assets/gpyrnn.frag:49-63 on the same FILES (renderer.cc:274-295), every
    pyramid level; the shader's literal bias index (uGuideConv2[16] at every level) is pinned too."""
    import oracle
    from oracle import gl_shaders
    rng = np.random.default_rng(23)
    conv1_file, conv2_file, per_level = [], [], []
    for lvl in range(3):
        # freeze_graph.py:139-157: fold batch norm (no scale: hdrnet/layers.py:40-58), stack, transpose
        conv1w_ = rng.standard_normal((1, 1, 3, 16)).astype(np.float32)
        conv1b_ = rng.standard_normal(16).astype(np.float32)            # BatchNorm/beta
        mu, sigma, eps = rng.standard_normal(16).astype(np.float32), rng.random(16).astype(np.float32) + 0.5, 1e-3
        conv1b_ = conv1b_ - mu / np.sqrt(sigma + eps)
        conv1w_ = conv1w_ / np.sqrt(sigma + eps)
        conv1w_ = np.squeeze(conv1w_.astype(np.float32))                # [3, 16]
        conv1b_ = np.squeeze(conv1b_.astype(np.float32))[np.newaxis, :]
        conv2w_ = np.squeeze(rng.standard_normal((1, 1, 16, 1)).astype(np.float32))
        conv2b_ = np.squeeze(rng.standard_normal(1).astype(np.float32))
        conv2 = np.append(conv2w_, conv2b_).astype(np.float32)
        conv1 = np.vstack([conv1w_, conv1b_]).astype(np.float32)        # [4, 16]
        conv1_file.append(np.ascontiguousarray(conv1.T).ravel())        # save(conv1.T, ...)
        conv2_file.append(conv2.ravel())
        per_level.append((np.ascontiguousarray(conv1.T), conv2))        # [16, 4], [17]: the C-ABI's layout
    conv1_file, conv2_file = np.concatenate(conv1_file), np.concatenate(conv2_file)
    px = rng.random((48, 3)).astype(np.float32)
    for lvl, (c1, c2) in enumerate(per_level):
        want = np.array([gl_shaders.gpyrnn_frag_guide(p, lvl, conv1_file, conv2_file) for p in px])
        got = oracle.pointwise_nn_guide(px[None, None], c1, c2)[0, 0]
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)
    # the shader as written: level 0's bias everywhere
    lit = gl_shaders.gpyrnn_frag_guide(px[0], 2, conv1_file, conv2_file, literal_bias_index=True)
    c2_lit = per_level[2][1].copy()
    c2_lit[16] = per_level[0][1][16]
    np.testing.assert_allclose(oracle.pointwise_nn_guide(px[:1][None], per_level[2][0], c2_lit)[0, 0], lit, atol=2e-6)


# ---- the row-split restatement (checker of hdrnet_bilateral_slice_apply_rows_f32) ---------------------
@pytest.mark.parametrize("cuts", [(0, 17), (0, 5, 17), (0, 1, 2, 9, 9, 17), (0, 16, 17)])
def test_port_row_bands_concatenate_to_the_pinned_whole_frame(port, cuts):
    """oracle_bilateral_slice_apply_rows keeps the reference's gyf on the FRAME height
    (bilateral_slice_apply.cc:38,42): any partition into bands (1-row and empty ones included),
    concatenated, equals the whole-frame function -- which is pinned to the reference -- bit for bit."""
    rng = np.random.default_rng(5)
    B, H, W = 2, 17, 23
    grid = rng.random((B, 5, 4, 6, 12), dtype=np.float32)
    guide = (rng.random((B, H, W), dtype=np.float32) * 1.1 - 0.05).astype(np.float32)
    inp = rng.random((B, H, W, 3), dtype=np.float32)
    want = port.bilateral_slice_apply(grid, guide, inp, True)
    bands = [port.bilateral_slice_apply_rows(grid, guide[:, a:b], inp[:, a:b], H, a, True)
             for a, b in zip(cuts, cuts[1:])]
    got = np.concatenate(bands, axis=1)
    assert got.shape == want.shape and np.array_equal(got, want)
    with pytest.raises(ValueError):
        port.bilateral_slice_apply_rows(grid, guide[:, :4], inp[:, :4], H, 14, True)


def test_reference_float32_noise_floor_of_the_per_pixel_vjps():
    """Why tests/conftest.py holds dguide to a flat 2e-5 (twice the reference's own noise) and dinput to the flat 1e-5 of SURVEY.md section
    8c: the reference's own float32 evaluation (the oracle) against the float64 value of the same formulas
    (tools/dguide_noise_floor.py) on the suite's data.  dinput's noise is far below 1e-5; dguide's is
    already a good fraction of it on a quarter-megapixel frame (1.1e-5 at 0.5 MP) -- but below the bar the
    HIP kernels are held to."""
    import sys
    from conftest import DGUIDE_ATOL, DINPUT_ATOL, ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dguide_noise_floor
    r = dguide_noise_floor.measure(270, 480)
    print(r)
    assert r["dinput"][0] < 0.2 * DINPUT_ATOL
    assert 0.25e-5 < r["dguide"][0] < DGUIDE_ATOL


# ---- the float64 references of the training step's kernels (oracle/f64_train.py) ---------------------------------------
@pytest.mark.parametrize("dims", [(270, 480, 540, 960), (540, 960, 1080, 1920), (539, 959, 1080, 1920),
                                  (1080, 1920, 270, 480), (1, 2, 1080, 1920)])
def test_f64_upsample_add_equals_the_float32_restatement_at_frame_sizes(dims):
    """Float32 coordinates, float64 sums: within float32 rounding of oracle.resize_bilinear_align_corners, which forms the
    same taps and evaluates three lerps a + (b - a) l in float32 -- five roundings of at most 2^-24 max|x| each per
    lerp, the row lerp on top of the two column lerps: 10 x 2^-24 max|x|."""
    import oracle
    from oracle import f64_train
    h, w, H, W = dims
    rng = np.random.default_rng(sum(dims))
    x = rng.standard_normal((1, h, w, 2)).astype(np.float32)
    fine = rng.standard_normal((1, H, W, 2)).astype(np.float32)
    got = f64_train.upsample_add_f64(x, fine) - fine
    want = oracle.resize_bilinear_align_corners(x, H, W)
    err = np.abs(got - want).max()
    bar = 10 * 2.0 ** -24 * np.abs(x).max()
    print(f"{dims}: max|f64 sums - float32 restatement| = {err:.3e}, bar {bar:.3e}")
    assert err <= bar


@pytest.mark.parametrize("shape", [(2, 17, 23, 34, 46, 3), (1, 5, 7, 11, 13, 3), (2, 8, 8, 16, 16, 1), (1, 1, 4, 3, 9, 3),
                                   (1, 12, 10, 6, 5, 3), (1, 6, 6, 6, 6, 5)])
def test_f64_upsample_add_equals_torch_float64_at_small_extents(shape):
    """At the extents of test_models.py::test_upsample_add_and_its_vjp_vs_torch_float64 the float32 source coordinate
    is within 2^-23 x extent of torch's float64 one (the scale's rounding and the product's), which moves the output
    by at most that times the largest step between neighbours (2 max|x|) per axis; the transpose likewise."""
    import torch
    import torch.nn.functional as F
    from oracle import f64_train
    B, h, w, H, W, C = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal((B, h, w, C)).astype(np.float32)
    fine = rng.standard_normal((B, H, W, C)).astype(np.float32)
    g = rng.standard_normal((B, H, W, C)).astype(np.float32)
    c64 = torch.from_numpy(x).double().requires_grad_(True)
    ref = F.interpolate(c64.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True).permute(0, 2, 3, 1) \
        + torch.from_numpy(fine).double()
    (ref * torch.from_numpy(g).double()).sum().backward()
    bar = 2.0 ** -23 * (h + w) * 2 * np.abs(x).max()
    err = np.abs(f64_train.upsample_add_f64(x, fine) - ref.detach().numpy()).max()
    assert err <= bar, (err, bar)
    # the transpose sums up to (H / h + 2) (W / w + 2) destination pixels per source pixel, each moved as above
    taps = (H / h + 2) * (W / w + 2)
    gbar = 2.0 ** -23 * (h + w) * taps * np.abs(g).max()
    gerr = np.abs(f64_train.upsample_vjp_f64(g, h, w) - c64.grad.numpy()).max()
    print(f"{shape}: forward {err:.3e} (bar {bar:.3e}), transpose {gerr:.3e} (bar {gbar:.3e})")
    assert gerr <= gbar, (gerr, gbar)


@pytest.mark.parametrize("dims", [(5, 7, 11, 13), (270, 480, 1080, 1920), (1080, 1920, 270, 480), (1, 2, 33, 65)])
def test_f64_upsample_vjp_is_the_adjoint(dims):
    """<W x, g> == <x, W^T g> to float64 rounding; every row of a tap matrix sums to one and has at most two entries;
    the float32 matrices (the planted-spike tests' expectation) are the float64 ones rounded."""
    from oracle import f64_train
    h, w, H, W = dims
    rng = np.random.default_rng(sum(dims))
    x = rng.standard_normal((2, h, w, 3)).astype(np.float32)
    g = rng.standard_normal((2, H, W, 3)).astype(np.float32)
    zero = np.zeros((2, H, W, 3), np.float32)
    lhs = float((f64_train.upsample_add_f64(x, zero) * g).sum())
    rhs = float((x * f64_train.upsample_vjp_f64(g, h, w)).sum())
    scale = float(np.abs(x).max() * np.abs(g).sum())
    assert abs(lhs - rhs) <= 1e-13 * scale, (lhs, rhs)
    for n_in, n_out in ((h, H), (w, W)):
        M = f64_train.resize_matrix(n_in, n_out)
        assert np.array_equal(M.sum(1), np.ones(n_out)) and ((M != 0).sum(1) <= 2).all() and (M >= 0).all()
        M32 = f64_train.resize_matrix(n_in, n_out, np.float32)
        assert M32.dtype == np.float32 and np.abs(M32 - M).max() <= 2.0 ** -24
        lo, hi, l = f64_train.resize_taps(n_in, n_out)
        assert lo[0] == 0 and hi.max() == n_in - 1 and (hi - lo <= 1).all() and (0 <= l).all() and (l < 1).all()


@pytest.mark.parametrize("epsilon_hat", [False, True])
def test_f64_adam_restatement_equals_torch_adam_in_float64(epsilon_hat):
    """oracle.f64_train.adam_step in float64 against torch.optim.Adam on float64 tensors with the same (float32-valued)
    hyper-parameters.  TensorFlow's placement of epsilon is torch's with eps / sqrt(1 - b2^t), set per step.  The
    float32 form of the same restatement stays within 1e-5 (relative to the update of an element whose gradients do not
    cancel) of it, and the moving average of |g| equals |exp_avg| for gradients of one sign."""
    import torch
    from oracle import f64_train
    lr, b1, b2, eps = f64_train.adam_hyper(1e-4, 0.9, 0.999, 1e-8)
    assert b2 == float(np.float32(0.999)) and abs((1 - b2) / (1 - 0.999) - 1) > 1e-5   # (not the double's 0.999)
    rng = np.random.default_rng(3)
    n = 1000
    p0 = rng.standard_normal(n)
    w = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([w], lr=float(lr), betas=(float(b1), float(b2)), eps=float(eps))
    p, m, v, s = p0.copy(), np.zeros(n), np.zeros(n), None
    p32, m32, v32 = p0.astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t in range(1, 8):
        g = (rng.standard_normal(n) * 1e-2).astype(np.float32)
        g[:10] = 0
        g[10:20] = 1e-20
        g[20:40] = np.abs(g[20:40])
        if epsilon_hat:
            opt.param_groups[0]["eps"] = float(eps) / (1 - float(b2) ** t) ** 0.5
        w.grad = torch.from_numpy(g).double()
        opt.step()
        p, m, v, upd, s, unit = f64_train.adam_step(p, m, v, g, t, 1e-4, 0.9, 0.999, 1e-8, epsilon_hat, s=s)
        p32, m32, v32, upd32, _, _ = f64_train.adam_step(p32, m32, v32, g, t, 1e-4, 0.9, 0.999, 1e-8, epsilon_hat,
                                                         dtype=np.float32)
        assert p32.dtype == m32.dtype == v32.dtype == upd32.dtype == np.float32
        np.testing.assert_allclose(p, w.detach().numpy(), rtol=1e-13, atol=0)
        assert (np.abs(m - opt.state[w]["exp_avg"].numpy()) <= 1e-13 * s).all()   # (gradients cancel in exp_avg)
        np.testing.assert_allclose(v, opt.state[w]["exp_avg_sq"].numpy(), rtol=1e-13, atol=0)
        assert np.abs(upd32 - upd).max() <= 1e-5 * unit.max()
        np.testing.assert_allclose(s[20:40], np.abs(m[20:40]), rtol=1e-13)
        assert (np.abs(upd) <= unit * (1 + 1e-13)).all()
