"""Every fast kernel flavour of BilateralSliceApply / BilateralSlice against the FLOAT64 value of the reference's formulas
(oracle/f64_ops.py), beside the distance of the reference's own float32 arithmetic (the C oracle) from that value.

The rest of the suite holds the HIP kernels to the C oracle at fixed bars (tests/conftest.py): that a kernel within the
bar is merely ORDERED differently and not noisier than the reference was measured for dguide and dinput of one op only
(tests/test_gpu_fullsize.py::test_dguide_noise_hip_vs_float64_against_the_reference_s_own).  Here it is asked of every
output of every flavour: out, dgrid, dguide, dinput; in max-norm and in rms; no pixel or cell left out.

    required:  |HIP - f64|  <=  1.5 x |reference f32 - f64|        (+ 1e-7 on the max-norm of out and dinput)

-- the margin of that existing test, measured against the reference and not against the kernel.  One line is printed per
case and output: both distances in both norms, the two ratios, the kernel name, and where the worst cell is.

Shapes: 270 x 480 against a 16 x 16 grid (1.3e5 pixels: the max-norms are stable) unless a plan needs another frame.

Measured on an MI355X (the table is in DESIGN.md section 3), ratio HIP / reference in max-norm (rms): dgrid 0.58 - 1.26
(0.13 - 0.48; 1.00 (0.98) on the many-task frame), dguide 0.45 - 0.98 (0.48 - 0.72), dinput 0.85 - 1.20 (0.81 - 0.88), the
forwards 0.66 - 1.11 (0.82 - 0.94) and 1.06 (1.19) for u8 -> f32 with a guide map, which folds the white level into the
coefficients; the generic kernels exactly 1.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle  # noqa: E402
from oracle.f64_ops import f64_slice, f64_slice_apply  # noqa: E402
from oracle.f64_train import upsample_add_f64  # noqa: E402

from grad_plan_cases import FAMILIES as GRAD_FAMILIES, PRODUCT_FRAMES, kernel_name, subsets  # noqa: E402
from row_plan import forward_kernel, row_plan, slice_kernel, vjp_kernel  # noqa: E402

MARGIN = 1.5
SLACK = {"out": 1e-7, "dinput": 1e-7}   # absolute, on the max-norm (test_gpu_fullsize.py: the dinput check's)
MAIN = (1, 270, 480, 16, 16)            # B, H, W, GH, GW
# tests/grad_plan_cases.py's families (op, Cin, Cout, has_offset, ...) and two that only the forward cases use
FAMILIES = dict(GRAD_FAMILIES, apply_3_3_nooff=("apply", 3, 3, 0, (), True), slice_1=("slice", 0, 1, 0, (), True))


def grid_channels(family):
    op, Cin, Cout, off = FAMILIES[family][:4]
    return Cout * (Cin + off) if op == "apply" else Cout


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from hdrnet_amd import hdrnet_ops
    return hdrnet_ops


@pytest.fixture(scope="module")
def mt_port(port):
    port.set_threads(min(os.cpu_count() or 1, 16))
    yield port
    port.set_threads(1)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N(t):
    return t.detach().cpu().numpy()


def misaligned(t, k=1):
    """tests/test_gpu_fuzz.py::misaligned: the same values at a storage offset of k floats -- contiguous, not 16-byte
    aligned."""
    buf = torch.empty(t.numel() + k, dtype=t.dtype, device=t.device)
    v = buf[k:].view(t.shape)
    v.copy_(t)
    return v


def norms(a, exact):
    err = np.abs(a.astype(np.float64) - exact)
    return float(err.max()), float(np.sqrt((err * err).mean())), err


def measure(case, kernel, got, ref, exact, failures, exact_ratio=False):
    """One line per output of `got` ({name: HIP array}) against `exact` (float64) beside `ref` (the C oracle); what breaks
    the 1.5 x rule is appended to `failures` with the worst cell, so that a case prints all its lines before it fails."""
    for o, hip in got.items():
        h_max, h_rms, h_err = norms(hip, exact[o])
        r_max, r_rms, r_err = norms(ref[o], exact[o])
        at = np.unravel_index(int(h_err.argmax()), h_err.shape)
        print(f"{case} [{kernel}] {o}: |HIP - f64| max {h_max:.3e} rms {h_rms:.3e}; |reference f32 - f64| max {r_max:.3e} "
              f"rms {r_rms:.3e}; ratio max {h_max / max(r_max, 1e-300):.2f} rms {h_rms / max(r_rms, 1e-300):.2f}; max|want| = {np.abs(exact[o]).max():.3g}; "
              f"worst at {tuple(int(i) for i in at)}: want {exact[o][at]:.9g}, HIP error {h_err[at]:.3e}, "
              f"reference error {r_err[at]:.3e}")
        if exact_ratio:
            if h_max != r_max or h_rms != r_rms:
                failures.append(f"{case} [{kernel}] {o}: ratio is not exactly 1 ({h_max!r} vs {r_max!r}, {h_rms!r} vs {r_rms!r})")
        elif h_max > MARGIN * r_max + SLACK.get(o, 0.0) or h_rms > MARGIN * r_rms:
            failures.append(f"{case} [{kernel}] {o}: max {h_max:.3e} vs {r_max:.3e} ({h_max / max(r_max, 1e-300):.2f} x), rms {h_rms:.3e} vs "
                            f"{r_rms:.3e} ({h_rms / max(r_rms, 1e-300):.2f} x); worst at {at}: want {exact[o][at]:.9g}")


# ---- the cases' data, float64 and the C oracle: computed once per (frame, family, depth) --------------------------------
_CACHE = {}


def problem(port, frame, family, GD, grads=True):
    """A frame of the suite's data (tests/grad_plan_cases.py::Problem) for `family`, with `exact` (float64) and `ref` (the
    C oracle) of every output the op has."""
    key = (frame, family, GD, grads)
    if key in _CACHE:
        return _CACHE[key]
    op, Cin, Cout, off = FAMILIES[family][:4]
    B, H, W, GH, GW = frame
    rng = np.random.default_rng(sum(frame) * 31 + GD * 7 + len(family))
    grid = rng.random((B, GH, GW, GD, grid_channels(family)), dtype=np.float32)
    g = (rng.random((B, H, W), dtype=np.float32) * 1.04 - 0.02).astype(np.float32)
    x = rng.random((B, H, W, max(Cin, 1)), dtype=np.float32)
    dout = rng.standard_normal((B, H, W, Cout)).astype(np.float32) if grads else None
    P = dict(grid=grid, guide=g, input=x, dout=dout, family=family, GD=GD, frame=frame)
    if op == "apply":
        names = ("out", "dgrid", "dguide", "dinput")
        exact = f64_slice_apply(grid, g, x, dout, bool(off))
        ref = (port.bilateral_slice_apply(grid, g, x, bool(off)),) + \
            (port.bilateral_slice_apply_grad(grid, g, x, dout, bool(off)) if grads else ())
    else:
        names = ("out", "dgrid", "dguide")
        exact = f64_slice(grid, g, dout)
        ref = (port.bilateral_slice(grid, g),) + (port.bilateral_slice_grad(grid, g, dout) if grads else ())
    P["exact"] = {n: e for n, e in zip(names, exact) if e is not None}
    P["ref"] = dict(zip(names, ref))
    _CACHE[key] = P
    return P


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _CACHE.clear()


def run_grads(ops, dev, P, wanted):
    """Forward + backward through the public op asking for `wanted` -> ({output: array}, forward kernel, backward kernel)."""
    op = FAMILIES[P["family"]][0]
    off = bool(FAMILIES[P["family"]][3])
    tg = T(P["grid"], dev).requires_grad_("dgrid" in wanted)
    tgu = T(P["guide"], dev).requires_grad_("dguide" in wanted)
    if op == "apply":
        ti = T(P["input"], dev).requires_grad_("dinput" in wanted)
        out = ops.bilateral_slice_apply(tg, tgu, ti, has_offset=off)
    else:
        ti = None
        out = ops.bilateral_slice(tg, tgu)
    kf = ops.last_kernel()
    out.backward(T(P["dout"], dev))
    kb = ops.last_kernel()
    got = {"out": N(out)}
    for o, t in (("dgrid", tg), ("dguide", tgu), ("dinput", ti)):
        if o in wanted:
            got[o] = N(t.grad)
    return got, kf, kb


# ---- 1. the gradient pass ---------------------------------------------------------------------------------------------------
GRAD_CASES = [(MAIN, fam, GD) for fam, GD in (("apply_3_3_off", 8), ("apply_3_3_off", 16), ("apply_4_4_off", 8),
                                             ("apply_4_4_off", 16), ("slice_12", 8), ("slice_12", 16), ("slice_2", 8))]
# the ragged upper plane tile (9, 12) and a half-empty lower one (4)
GRAD_CASES += [(MAIN, "apply_3_3_off", GD) for GD in (4, 9, 12)] + [(MAIN, "slice_12", 9), (MAIN, "apply_4_4_off", 12)]
# many task columns on few rows: the row plans with rg < cell (tests/test_grad_plan_host.py)
GRAD_CASES += [(PRODUCT_FRAMES[0], "apply_3_3_off", 8), (PRODUCT_FRAMES[0], "slice_12", 16)]


@pytest.mark.parametrize("frame,family,GD", GRAD_CASES, ids=lambda v: "%dx%dx%d-grid%dx%d" % v if isinstance(v, tuple) else str(v))
def test_gradient_pass_against_float64(dev, ops, mt_port, frame, family, GD):
    """grid_grad_mfma (dgrid alone: the f32-MFMA contraction, two plane tiles at GD > 8, two channel windows at 4 -> 4,
    the fixed-order stage 2) and apply_bwd_fused / slice_bwd_fused (dgrid with per-pixel gradients) under every subset of
    the wanted outputs that contains dgrid."""
    P = problem(mt_port, frame, family, GD)
    failures = []
    for wanted in subsets(family):
        got, kf, kb = run_grads(ops, dev, P, wanted)
        assert kb == kernel_name(family, wanted), (wanted, kb)
        case = f"{family} GD={GD} {'x'.join(map(str, frame))} want {'+'.join(wanted)}"
        out = {"out": got.pop("out")}
        if wanted == subsets(family)[0]:
            measure(case, kf, out, P["ref"], P["exact"], failures)
        measure(case, kb, got, P["ref"], P["exact"], failures)
    assert not failures, "\n".join(failures)


# ---- 2. the per-pixel VJPs without dgrid, and the generic kernels as the control -----------------------------------------
@pytest.mark.parametrize("GD", [4, 8, 16])
def test_per_pixel_vjps_against_float64(dev, ops, mt_port, GD):
    """dguide + dinput with the grid frozen: apply_vjp_seg."""
    P = problem(mt_port, MAIN, "apply_3_3_off", GD)
    B, H, W, GH, GW = MAIN
    assert vjp_kernel(B, H, W, GW, GD) == "apply_vjp_seg/vec4"
    failures = []
    for wanted in (("dguide", "dinput"), ("dguide",), ("dinput",)):
        got, _, kb = run_grads(ops, dev, P, wanted)
        assert kb == "apply_vjp_seg/vec4", kb
        got.pop("out")
        measure(f"apply_3_3_off GD={GD} want {'+'.join(wanted)}", kb, got, P["ref"], P["exact"], failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("family,GD", [("apply_3_3_off", 8), ("slice_12", 16)])
def test_generic_kernels_are_the_control(dev, ops, mt_port, family, GD):
    """The generic kernels are bit-exact to the C oracle (tests/test_gpu_parity.py): their distances to float64 are the
    reference's own and every ratio is exactly 1 -- the control of this file's measurement."""
    P = problem(mt_port, MAIN, family, GD)
    failures = []
    with ops.kernel_override("generic"):
        got, kf, kb = run_grads(ops, dev, P, subsets(family)[0])
    op = FAMILIES[family][0]
    assert kf == op + "_fwd_generic" and kb == op + "_grad_generic", (kf, kb)
    measure(f"{family} GD={GD} generic", kf + ", " + kb, got, P["ref"], P["exact"], failures, exact_ratio=True)
    assert not failures, "\n".join(failures)


# ---- 3. the forward's flavours -------------------------------------------------------------------------------------------------
def forward_case(ops, dev, port, frame, family, GD, failures, misalign=False, kernel=None):
    P = problem(port, frame, family, GD, grads=False)
    op, _, _, off = FAMILIES[family][:4]
    tg, tgu, ti = T(P["grid"], dev), T(P["guide"], dev), T(P["input"], dev)
    if misalign:
        tgu, ti = misaligned(tgu), misaligned(ti)
        assert tgu.data_ptr() % 16 and ti.data_ptr() % 16
    with torch.no_grad():
        out = ops.bilateral_slice_apply(tg, tgu, ti, has_offset=bool(off)) if op == "apply" else ops.bilateral_slice(tg, tgu)
    k = ops.last_kernel()
    if kernel is not None:
        assert k == kernel, (k, kernel)
    assert "generic" not in k, k
    measure(f"{family} GD={GD} {'x'.join(map(str, frame))}{' misaligned' if misalign else ''} forward", k, {"out": N(out)},
            P["ref"], P["exact"], failures)
    return k


def test_forward_flavours_against_float64(dev, ops, mt_port):
    """apply_fwd_seg/vec4 (the y-pre-lerped LDS image), the scalar row kernel on a misaligned view, the row-kernel
    fallback where the seg kernel's image does not fit (a FALLBACKS shape of tests/test_gpu_fused_fullsize.py), a width of
    more than one segment per row, has_offset = False, 4 -> 4, and slice_fwd_rows with 12 channels and with 1."""
    failures = []
    B, H, W, GH, GW = MAIN
    for GD in (8, 16):
        assert forward_kernel(B, H, W, GW, GD) == "apply_fwd_seg/vec4"
        forward_case(ops, dev, mt_port, MAIN, "apply_3_3_off", GD, failures, kernel="apply_fwd_seg/vec4")
    k = forward_kernel(B, H, W, GW, 8, aligned=False)
    assert k == "apply_fwd_rows/scalar", k
    forward_case(ops, dev, mt_port, MAIN, "apply_3_3_off", 8, failures, misalign=True, kernel=k)
    odd = (1, 135, 483, 16, 16)    # W % 4 != 0: the scalar kernel by width
    assert forward_kernel(*odd[:3], 16, 8) == "apply_fwd_rows/scalar"
    forward_case(ops, dev, mt_port, odd, "apply_3_3_off", 8, failures, kernel="apply_fwd_rows/scalar")
    fallback = (1, 12, 1024, 8, 64)   # FALLBACKS (1024, 64) at GD 16: (GD + 2) planes of the window exceed 64 KiB
    assert forward_kernel(1, 12, 1024, 64, 16) == "apply_fwd_rows/vec4"
    forward_case(ops, dev, mt_port, fallback, "apply_3_3_off", 16, failures, kernel="apply_fwd_rows/vec4")
    wide = (2, 8, 1920, 4, 16)
    assert row_plan(1920)[1] > 1 and forward_kernel(2, 8, 1920, 16, 8) == "apply_fwd_seg/vec4"
    forward_case(ops, dev, mt_port, wide, "apply_3_3_off", 8, failures, kernel="apply_fwd_seg/vec4")
    for fam in ("apply_3_3_nooff", "apply_4_4_off"):
        forward_case(ops, dev, mt_port, MAIN, fam, 8, failures, kernel="apply_fwd_seg/vec4")
    for fam, C in (("slice_12", 12), ("slice_1", 1)):
        for GD in (8, 16):
            assert slice_kernel(B, H, W, GW, GD, C) == "slice_fwd_rows"
            forward_case(ops, dev, mt_port, MAIN, fam, GD, failures, kernel="slice_fwd_rows")
    assert not failures, "\n".join(failures)


# ---- 4. the fused forwards with float32 output ---------------------------------------------------------------------------------
def nn_params(rng, n, Cin=3):
    return ((rng.standard_normal((n, Cin + 1)) * 0.8).astype(np.float32), (rng.standard_normal(n + 1) * 0.5).astype(np.float32))


def curves_params(rng, npts):
    """tests/test_gpu_fused_fullsize.py::curves_params: ccm near the identity, knots spread over [0, 1)."""
    ccm = (np.concatenate([np.eye(3), np.zeros((3, 1))], 1) + 0.2 * rng.standard_normal((3, 4))).astype(np.float32)
    shifts = (np.tile(np.linspace(0, 1, npts, endpoint=False)[:, None], (1, 3))
              + 0.16 / npts * rng.standard_normal((npts, 3))).astype(np.float32)
    slopes = (0.3 * rng.standard_normal((npts, 3)) * 16 / npts).astype(np.float32)
    slopes[0] += 1.0
    return ccm, shifts, slopes, np.array([0.4, 0.35, 0.25, 0.02], np.float32)


def fused_case(port, case, kernel, grid_P, out, guide, x64, failures, coarse=None):
    """The slice-apply arithmetic of a fused forward: float64 and the C oracle are fed the guide THE KERNEL returned (the
    guides have their own bars in tests/test_gpu_fused_fullsize.py) and the frame / white level (in float64, and rounded
    to float32 for the oracle)."""
    grid = grid_P["grid"]
    x32 = x64.astype(np.float32)
    exact = f64_slice_apply(grid, guide, x64, None, True)[0]
    ref = port.bilateral_slice_apply(grid, guide, x32, True)
    if coarse is not None:
        exact = upsample_add_f64(coarse, exact)
        ref = ref + oracle.resize_bilinear_align_corners(coarse, *ref.shape[1:3])
    measure(case, kernel, {"out": out}, {"out": ref}, {"out": exact}, failures)


@pytest.mark.parametrize("GD", [8, 16])
def test_fused_forwards_against_float64(dev, ops, mt_port, GD):
    """bilateral_slice_apply_nnguide, _curves, _io (u8 -> f32, u16 -> f32 at white level 32767, each with a computed guide
    and with a guide map) and _upadd.  u8 outputs are out of scope: quantisation hides the quantity measured."""
    B, H, W, GH, GW = MAIN
    rng = np.random.default_rng(900 + GD)
    P = dict(grid=rng.random((B, GH, GW, GD, 12), dtype=np.float32))
    x = rng.random((B, H, W, 3), dtype=np.float32)
    raw8 = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    raw16 = rng.integers(0, 32768, (B, H, W, 3), dtype=np.uint16)
    gmap = (rng.random((B, H, W), dtype=np.float32) * 1.04 - 0.02).astype(np.float32)
    c1, c2 = nn_params(rng, 16)
    curves = curves_params(rng, 16)
    coarse = rng.standard_normal((B, H // 2, W // 2, 3)).astype(np.float32)
    tg, tx, tc1, tc2 = T(P["grid"], dev), T(x, dev), T(c1, dev), T(c2, dev)
    tcv = tuple(T(a, dev) for a in curves)
    t8 = T(raw8, dev)
    t16 = torch.from_numpy(raw16.astype(np.int32)).to(dev).to(torch.uint16)
    x8, x16 = raw8.astype(np.float64) / 255.0, raw16.astype(np.float64) / 32767.0
    failures = []
    tag = f"GD={GD} {H}x{W}"

    out, g = ops.bilateral_slice_apply_nnguide(tg, tx, tc1, tc2, return_guide=True)
    k = ops.last_kernel()
    assert k == "apply_fwd_seg/vec4+nnguide", k
    fused_case(mt_port, tag + " nnguide", k, P, N(out), N(g), x, failures)

    with torch.no_grad():
        out = ops.bilateral_slice_apply_curves(tg, tx, *tcv)
    k = ops.last_kernel()
    assert k == "apply_fwd_io/f32->f32+curvesguide", k
    out2, g = ops.bilateral_slice_apply_io(tg, tx, guide_curves=tcv, return_guide=True)
    assert ops.last_kernel() == k and torch.equal(out, out2)   # the same kernel: its guide is the one the first call used
    fused_case(mt_port, tag + " curves", k, P, N(out), N(g), x, failures)

    out, g = ops.bilateral_slice_apply_io(tg, t8, guide_conv1=tc1, guide_conv2=tc2, input_white_level=255.0, return_guide=True)
    k = ops.last_kernel()
    assert k == "apply_fwd_io/u8->f32+nnguide", k
    fused_case(mt_port, tag + " io u8->f32 nnguide", k, P, N(out), N(g), x8, failures)

    out = ops.bilateral_slice_apply_io(tg, t8, guide=T(gmap, dev), input_white_level=255.0)
    k = ops.last_kernel()
    assert k == "apply_fwd_io/u8->f32", k
    fused_case(mt_port, tag + " io u8->f32 guide map", k, P, N(out), gmap, x8, failures)

    out, g = ops.bilateral_slice_apply_io(tg, t16, guide_curves=tcv, input_white_level=32767.0, return_guide=True)
    k = ops.last_kernel()
    assert k == "apply_fwd_io/u16->f32+curvesguide", k
    fused_case(mt_port, tag + " io u16->f32 curves", k, P, N(out), N(g), x16, failures)

    out = ops.bilateral_slice_apply_io(tg, t16, guide=T(gmap, dev), input_white_level=32767.0)
    k = ops.last_kernel()
    assert k.startswith("apply_fwd_io/u16->f32") and "guide" not in k, k
    fused_case(mt_port, tag + " io u16->f32 guide map", k, P, N(out), gmap, x16, failures)

    out = ops.bilateral_slice_apply_upadd(tg, tx, T(coarse, dev), guide=T(gmap, dev))
    k = ops.last_kernel()
    assert k == "apply_fwd_seg/vec4+upadd", k
    fused_case(mt_port, tag + " upadd guide map", k, P, N(out), gmap, x, failures, coarse=coarse)
    assert not failures, "\n".join(failures)
