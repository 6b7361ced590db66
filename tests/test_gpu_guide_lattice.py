"""Every kernel that reads a guide, at the guide values where its address or its branch changes (tests/guide_lattice_cases.py:
tap switches and cell borders to the ulp, exactly 0 and 1, guides far out of range, and wild ones up to |guide * GD| = 2^30)
against the C oracle, which is bit-defined there (tests/test_guide_lattice_host.py holds it to the compiled reference bit for
bit on these very frames).  A float64 twin is no referee at a tap switch: float64 and float32 legitimately fall on different
sides of floor().

Three layouts per depth: "rows" (every 64-pixel chunk uniform: all wild, all on one switch), "mixed" (every chunk mixes
every tier) and "planted" (one lattice value per chunk on a cycling lane over a background inside one plane half: the
ballot branches of the gradient pass with exactly one lane set).

Bars are the suite's (tests/conftest.py, tests/test_gpu_fuzz.py): forward atol = rtol = 1e-5; dinput 1e-5; dguide 2e-5 x
max(1, GD / 8) (x max(1, C / 12) for a slice); dgrid check_dgrid; rtol 1e-4 on the gradients; the generic kernels bit for bit.
No pixel and no cell is left out in any tier.  One line is printed per case and output: the worst error / bar, and the worst
per tier (0 = the planted layout's background)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle  # noqa: E402

from conftest import DGUIDE_ATOL, DINPUT_ATOL, GRAD_RTOL, check_dgrid  # noqa: E402
from grad_plan_cases import FAMILIES as GRAD_FAMILIES, PRODUCT_FRAMES, kernel_name, subsets  # noqa: E402
from guide_lattice_cases import (FALLBACK, LAYOUT_FRAMES, LOWER, MANY_TASKS, ODD, UPPER, guide_frame,  # noqa: E402
                                 problem_arrays)
from row_plan import (forward_kernel, fused_forward_kernel, gg_reaches, grad_kernels, seg_reaches, slice_kernel,  # noqa: E402
                      vjp_kernel)

FWD_TOL = 1e-5
DEPTHS = (4, 7, 8, 12, 16)
LAYOUTS = [("rows", LOWER), ("mixed", LOWER), ("planted", LOWER)]
# tests/grad_plan_cases.py's families (op, Cin, Cout, has_offset, ...) and the forward-only ones
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


def T16(raw16, dev):
    return torch.from_numpy(raw16.astype(np.int32)).to(dev).to(torch.uint16)


def misaligned(t, k=1):
    """The same values at a storage offset of k floats: contiguous, not 16-byte aligned."""
    buf = torch.empty(t.numel() + k, dtype=t.dtype, device=t.device)
    v = buf[k:].view(t.shape)
    v.copy_(t)
    return v


def layouts_for(GD):
    return LAYOUTS + ([("planted", UPPER)] if GD == 16 else [])


def layout_id(layout, background):
    return layout + ("-upper" if background == UPPER else "")


class Tally:
    """Collects what breaks a bar, so that a case prints all its lines before it fails, and the kernels that ran."""

    def __init__(self):
        self.failures, self.kernels = [], set()

    def held(self, case, kernel, name, got, want, atol, rtol, tier=None, guide=None):
        """|got - want| <= atol + rtol |want| everywhere; `tier` [B, H, W] splits the printed worst ratio."""
        self.kernels.add(kernel)
        assert got.shape == want.shape, (case, name, got.shape, want.shape)
        err = np.abs(got.astype(np.float64) - want.astype(np.float64))
        ratio = err / (atol + rtol * np.abs(want.astype(np.float64)))
        ratio = np.where(np.isfinite(got), ratio, np.inf)
        at = np.unravel_index(int(ratio.argmax()), ratio.shape)
        line = f"{case} [{kernel}] {name}: worst |err| / bar = {ratio[at]:.3f} (|err| {err[at]:.3e}, want {want[at]:.6g}) at {tuple(map(int, at))}"
        if tier is not None:
            per_px = ratio.reshape(tier.shape + (-1,)).max(axis=-1)
            line += "; by tier: " + ", ".join(f"{t}: {per_px[tier == t].max():.3f}" for t in sorted(set(tier.ravel().tolist())))
            if guide is not None:
                line += f"; guide there {guide[at[:3]]!r} (tier {int(tier[at[:3]])})"
        print(line)
        if not ratio.max() <= 1.0:
            self.failures.append(line)

    def dgrid(self, case, kernel, got, want):
        scale = max(1.0, float(np.abs(want).max()))
        self.held(case, kernel, "dgrid", got, want, 1e-5 * scale, GRAD_RTOL)
        try:
            check_dgrid(got, want, case)
        except AssertionError as e:
            self.failures.append(f"{case} [{kernel}] check_dgrid: {str(e)[:300]}")

    def equal(self, case, kernel, name, got, want):
        self.kernels.add(kernel)
        same = np.array_equal(got, want)
        print(f"{case} [{kernel}] {name}: {'equal to the oracle' if same else 'DIFFERS'}")
        if not same:
            bad = got != want
            at = np.unravel_index(int(bad.argmax()), bad.shape)
            self.failures.append(f"{case} [{kernel}] {name}: {int(bad.sum())} values differ, first at {tuple(map(int, at))}: "
                                 f"{got[at]!r} vs {want[at]!r}")

    def done(self):
        print("kernels:", sorted(self.kernels))
        assert not self.failures, "\n".join(self.failures)


# ---- the cases' data and the oracle's answers: once per (frame, family, depth, layout) ---------------------------------------
_CACHE = {}


def problem(port, frame, family, GD, layout, background=LOWER, grads=True):
    key = (frame, family, GD, layout, background)
    P = _CACHE.get(key)
    if P is None:
        op, Cin, Cout, off = FAMILIES[family][:4]
        guide, tier = guide_frame(GD, layout, frame[:3], background)
        grid, x, dout = problem_arrays(frame, GD, grid_channels(family), Cin, Cout, sum(frame) * 31 + GD * 7 + len(family))
        P = _CACHE[key] = dict(grid=grid, guide=guide, tier=tier, input=x, dout=dout, family=family, GD=GD, frame=frame, ref={},
                               tag=f"{family} GD={GD} {'x'.join(map(str, frame[:3]))} {layout_id(layout, background)}")
    ref, off = P["ref"], bool(FAMILIES[family][3])
    apply = FAMILIES[family][0] == "apply"
    if "out" not in ref:
        ref["out"] = port.bilateral_slice_apply(P["grid"], P["guide"], P["input"], off) if apply else \
            port.bilateral_slice(P["grid"], P["guide"])
    if grads and "dgrid" not in ref:
        got = port.bilateral_slice_apply_grad(P["grid"], P["guide"], P["input"], P["dout"], off) if apply else \
            port.bilateral_slice_grad(P["grid"], P["guide"], P["dout"])
        ref.update(zip(("dgrid", "dguide", "dinput"), got))
    return P


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    yield
    _CACHE.clear()


def run_grads(ops, dev, P, wanted):
    """Forward + backward through the public op asking for `wanted` -> ({output: array}, forward kernel, backward kernel)."""
    op, off = FAMILIES[P["family"]][0], bool(FAMILIES[P["family"]][3])
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


def dguide_atol(P):
    slice_scale = max(1.0, grid_channels(P["family"]) / 12.0) if FAMILIES[P["family"]][0] == "slice" else 1.0
    return DGUIDE_ATOL * max(1.0, P["GD"] / 8.0) * slice_scale


def hold_grads(tally, P, kb, got, wanted):
    case = f"{P['tag']} want {'+'.join(wanted)}"
    for o in wanted:
        if o == "dgrid":
            tally.dgrid(case, kb, got[o], P["ref"][o])
        else:
            tally.held(case, kb, o, got[o], P["ref"][o], dguide_atol(P) if o == "dguide" else DINPUT_ATOL, GRAD_RTOL, P["tier"],
                       P["guide"])


def hold_forward(tally, P, k, out, what=""):
    tally.held(P["tag"] + what, k, "out", out, P["ref"]["out"], FWD_TOL, FWD_TOL, P["tier"], P["guide"])


# ---- a. the generic kernels: bit for bit on the lattice ------------------------------------------------------------------------
@pytest.mark.parametrize("GD", (1,) + DEPTHS)
@pytest.mark.parametrize("family", ["apply_3_3_off", "slice_12"])
def test_generic_kernels_equal_the_oracle_on_the_lattice(dev, ops, mt_port, family, GD):
    """out, dgrid, dguide and dinput of the generic kernels are the oracle's bit for bit (tests/test_gpu_parity.py) -- also on
    a tap switch, at 0 and 1, out of range and in the wild tier, where the int conversion saturates."""
    tally = Tally()
    op = FAMILIES[family][0]
    wanted = ("dgrid", "dguide") + (("dinput",) if op == "apply" else ())
    for layout, background in layouts_for(GD):
        P = problem(mt_port, LAYOUT_FRAMES[layout], family, GD, layout, background)
        with ops.kernel_override("generic"):
            got, kf, kb = run_grads(ops, dev, P, wanted)
        assert kf == op + "_fwd_generic" and kb == op + "_grad_generic", (kf, kb)
        tally.equal(P["tag"], kf, "out", got["out"], P["ref"]["out"])
        for o in wanted:
            tally.equal(P["tag"], kb, o, got[o], P["ref"][o])
    tally.done()


# ---- b. the forwards with a guide map -----------------------------------------------------------------------------------------
def forward(ops, dev, P, misalign=False):
    op, off = FAMILIES[P["family"]][0], bool(FAMILIES[P["family"]][3])
    tg, tgu, ti = T(P["grid"], dev), T(P["guide"], dev), T(P["input"], dev)
    if misalign:
        tgu, ti = misaligned(tgu), misaligned(ti)
        assert tgu.data_ptr() % 16 and ti.data_ptr() % 16
    with torch.no_grad():
        out = ops.bilateral_slice_apply(tg, tgu, ti, has_offset=off) if op == "apply" else ops.bilateral_slice(tg, tgu)
    return N(out), ops.last_kernel()


@pytest.mark.parametrize("GD", DEPTHS)
def test_forwards_on_the_lattice(dev, ops, mt_port, GD):
    """apply_fwd_seg/vec4 (3 -> 3 with and without offset, 4 -> 4), the scalar row kernel on a misaligned view and at
    W % 4 != 0, slice_fwd_rows with 12 channels and with 1, and two row bands cut inside a grid row."""
    tally = Tally()
    for layout, background in layouts_for(GD):
        frame = LAYOUT_FRAMES[layout]
        B, H, W, GH, GW = frame
        for family in ("apply_3_3_off", "apply_3_3_nooff", "apply_4_4_off"):
            _, Cin, Cout, off = FAMILIES[family][:4]
            want_k = forward_kernel(B, H, W, GW, GD, shape=(Cin, Cout, bool(off)))
            assert want_k == "apply_fwd_seg/vec4", (frame, family, want_k)
            P = problem(mt_port, frame, family, GD, layout, background, grads=False)
            out, k = forward(ops, dev, P)
            assert k == want_k, (P["tag"], k)
            hold_forward(tally, P, k, out)
        for family, C in (("slice_12", 12), ("slice_1", 1)):
            assert slice_kernel(B, H, W, GW, GD, C) == "slice_fwd_rows"
            P = problem(mt_port, frame, family, GD, layout, background, grads=False)
            out, k = forward(ops, dev, P)
            assert k == "slice_fwd_rows", (P["tag"], k)
            hold_forward(tally, P, k, out)
    # the scalar row kernel: by alignment, by width
    frame = LAYOUT_FRAMES["mixed"]
    B, H, W, GH, GW = frame
    assert forward_kernel(B, H, W, GW, GD, aligned=False) == "apply_fwd_rows/scalar"
    P = problem(mt_port, frame, "apply_3_3_off", GD, "mixed", grads=False)
    out, k = forward(ops, dev, P, misalign=True)
    assert k == "apply_fwd_rows/scalar", k
    hold_forward(tally, P, k, out, " misaligned")
    assert forward_kernel(*ODD[:3], ODD[4], GD) == "apply_fwd_rows/scalar"
    P = problem(mt_port, ODD, "apply_3_3_off", GD, "mixed", grads=False)
    out, k = forward(ops, dev, P)
    assert k == "apply_fwd_rows/scalar", k
    hold_forward(tally, P, k, out)
    # two bands of the mixed frame, cut at row 23: inside grid row 1 (16 rows per grid row)
    P = problem(mt_port, frame, "apply_3_3_off", GD, "mixed", grads=False)
    tg, tgu, ti = T(P["grid"], dev), T(P["guide"], dev), T(P["input"], dev)
    bands = []
    for a, b in ((0, 23), (23, H)):
        bands.append(N(ops.bilateral_slice_apply_rows(tg, tgu[:, a:b], ti[:, a:b], H, a, True)))
        assert ops.last_kernel() == "apply_fwd_seg/vec4", ops.last_kernel()
    hold_forward(tally, P, "apply_fwd_seg/vec4", np.concatenate(bands, axis=1), " as row bands 0:23:64")
    tally.done()


@pytest.mark.parametrize("GD", (16, 17))
def test_row_kernel_fallback_on_the_lattice(dev, ops, mt_port, GD):
    """apply_fwd_rows/vec4: 1024 pixels against 64 grid columns, where the segment kernel's (GD + 2)-plane image exceeds the
    LDS at GD >= 16; a row of the mixed layout holds the whole lattice."""
    B, H, W, GH, GW = FALLBACK
    assert forward_kernel(B, H, W, GW, GD) == "apply_fwd_rows/vec4"
    tally = Tally()
    P = problem(mt_port, FALLBACK, "apply_3_3_off", GD, "mixed", grads=False)
    out, k = forward(ops, dev, P)
    assert k == "apply_fwd_rows/vec4", k
    hold_forward(tally, P, k, out)
    tally.done()


@pytest.mark.parametrize("GD", DEPTHS)
def test_fused_forwards_with_a_lattice_guide_map(dev, ops, mt_port, GD):
    """apply_fwd_io u8 -> f32 and u16 -> f32 and apply_fwd_seg/vec4+upadd with the lattice as the guide map; the oracle is
    fed raw / white level rounded to float32."""
    tally = Tally()
    for layout, background in layouts_for(GD):
        frame = LAYOUT_FRAMES[layout]
        B, H, W, GH, GW = frame
        assert seg_reaches(B, H, W, GW, GD, io=True)
        P = problem(mt_port, frame, "apply_3_3_off", GD, layout, background, grads=False)
        rng = np.random.default_rng(40 + GD)
        raw8 = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
        raw16 = rng.integers(0, 32768, (B, H, W, 3), dtype=np.uint16)
        coarse = rng.standard_normal((B, H // 2, W // 2, 3)).astype(np.float32)
        tg, tgu = T(P["grid"], dev), T(P["guide"], dev)

        def hold(k, out, x32, what, add=None):
            want = mt_port.bilateral_slice_apply(P["grid"], P["guide"], x32, True)
            if add is not None:
                want = want + add
            tally.held(P["tag"] + what, k, "out", out, want, FWD_TOL, FWD_TOL, P["tier"], P["guide"])

        out = ops.bilateral_slice_apply_io(tg, T(raw8, dev), guide=tgu, input_white_level=255.0)
        k = ops.last_kernel()
        assert k == "apply_fwd_io/u8->f32", k
        hold(k, N(out), (raw8.astype(np.float64) / 255.0).astype(np.float32), " io u8")
        out = ops.bilateral_slice_apply_io(tg, T16(raw16, dev), guide=tgu, input_white_level=32767.0)
        k = ops.last_kernel()
        assert k.startswith("apply_fwd_io/u16->f32") and "guide" not in k and "generic" not in k, k
        hold(k, N(out), (raw16.astype(np.float64) / 32767.0).astype(np.float32), " io u16")
        assert fused_forward_kernel(B, H, W, GW, GD, "upadd") == "apply_fwd_seg/vec4+upadd"
        out = ops.bilateral_slice_apply_upadd(tg, T(P["input"], dev), T(coarse, dev), guide=tgu)
        k = ops.last_kernel()
        assert k == "apply_fwd_seg/vec4+upadd", k
        hold(k, N(out), P["input"], " upadd", add=oracle.resize_bilinear_align_corners(coarse, H, W))
    tally.done()


# ---- c. the gradient pass ----------------------------------------------------------------------------------------------------------
GRAD_CASES = [("apply_3_3_off", GD) for GD in DEPTHS] + [(f, GD) for f in ("apply_4_4_off", "slice_12") for GD in (8, 16)] + \
    [("slice_2", 8)]
GRAD_PARAMS = [(fam, GD, layout, bg) for fam, GD in GRAD_CASES for layout, bg in layouts_for(GD)]


def gradient_pass_case(ops, dev, port, frame, family, GD, layout, background):
    B, H, W, GH, GW = frame
    assert gg_reaches(B, H, W, GH, GW, GD, grid_channels(family)), (frame, family, GD)
    P = problem(port, frame, family, GD, layout, background)
    tally = Tally()
    for wanted in subsets(family):
        got, kf, kb = run_grads(ops, dev, P, wanted)
        assert kb == kernel_name(family, wanted), (wanted, kb)
        assert "generic" not in kf, kf
        if wanted == subsets(family)[0]:
            hold_forward(tally, P, kf, got["out"])
        hold_grads(tally, P, kb, got, wanted)
    tally.done()


@pytest.mark.parametrize("family,GD,layout,background", GRAD_PARAMS,
                         ids=[f"{f}-GD{GD}-{layout_id(la, bg)}" for f, GD, la, bg in GRAD_PARAMS])
def test_gradient_pass_on_the_lattice(dev, ops, mt_port, family, GD, layout, background):
    """grid_grad_mfma alone and apply_bwd_fused / slice_bwd_fused under every subset of the wanted outputs: the clamped z
    taps, the cancellation-free dw0 + dw1 at a tap offset of exactly 0, the wave-uniform branch for taps past their cell
    (one lane of a chunk in "planted", all of them in "rows"), P and Q on one slot at the last plane, and at GD = 16 a plane
    half that exactly one lane of a chunk reaches."""
    gradient_pass_case(ops, dev, mt_port, LAYOUT_FRAMES[layout], family, GD, layout, background)


@pytest.mark.parametrize("family,GD", [("apply_3_3_off", 8), ("slice_12", 16)])
def test_gradient_pass_on_the_lattice_many_tasks(dev, ops, mt_port, family, GD):
    """A PRODUCT_FRAMES entry: many task columns on few rows (rows per task below the cell height); 32-pixel rows, so every
    chunk is half dead lanes."""
    assert MANY_TASKS in PRODUCT_FRAMES
    gradient_pass_case(ops, dev, mt_port, MANY_TASKS, family, GD, "mixed", LOWER)


# ---- d. the per-pixel VJPs with the grid frozen ---------------------------------------------------------------------------------
@pytest.mark.parametrize("GD", DEPTHS)
def test_per_pixel_vjps_on_the_lattice(dev, ops, mt_port, GD):
    """apply_vjp_seg/vec4 for (dguide, dinput), (dguide,) and (dinput,): its derivative's zero branch is taken per lane."""
    tally = Tally()
    for layout, background in layouts_for(GD):
        frame = LAYOUT_FRAMES[layout]
        B, H, W, GH, GW = frame
        assert vjp_kernel(B, H, W, GW, GD) == "apply_vjp_seg/vec4"
        P = problem(mt_port, frame, "apply_3_3_off", GD, layout, background)
        for wanted in (("dguide", "dinput"), ("dguide",), ("dinput",)):
            got, _, kb = run_grads(ops, dev, P, wanted)
            assert kb == "apply_vjp_seg/vec4", kb
            hold_grads(tally, P, kb, got, wanted)
    tally.done()


def test_row_family_vjp_on_the_lattice(dev, ops, mt_port):
    """apply_vjp_rows/vec4: alone at GD = 16 on the fallback frame, where the segment kernel's image does not fit, and with
    apply_grad_generic for dgrid at GD = 17, which puts the MFMA pass out of reach."""
    B, H, W, GH, GW = FALLBACK
    tally = Tally()
    assert vjp_kernel(B, H, W, GW, 16) == "apply_vjp_rows/vec4"
    P = problem(mt_port, FALLBACK, "apply_3_3_off", 16, "mixed")
    got, _, kb = run_grads(ops, dev, P, ("dguide", "dinput"))
    assert kb == "apply_vjp_rows/vec4", kb
    hold_grads(tally, P, kb, got, ("dguide", "dinput"))
    want_k = grad_kernels(B, H, W, GH, GW, 17, True, True)
    assert want_k == "apply_vjp_rows/vec4+apply_grad_generic", want_k
    P = problem(mt_port, FALLBACK, "apply_3_3_off", 17, "mixed")
    got, _, kb = run_grads(ops, dev, P, ("dgrid", "dguide", "dinput"))
    assert kb == want_k, kb
    hold_grads(tally, P, kb, got, ("dgrid", "dguide", "dinput"))
    tally.done()


# ---- e. computed guides that saturate ------------------------------------------------------------------------------------------
def nn_params(rng, n, Cin=3):
    """tests/test_gpu_f64_noise.py::nn_params."""
    return ((rng.standard_normal((n, Cin + 1)) * 0.8).astype(np.float32), (rng.standard_normal(n + 1) * 0.5).astype(np.float32))


def curves_params(rng, npts, scale):
    """tests/test_gpu_f64_noise.py::curves_params with the colour matrix scaled by `scale`."""
    ccm = (scale * (np.concatenate([np.eye(3), np.zeros((3, 1))], 1) + 0.2 * rng.standard_normal((3, 4)))).astype(np.float32)
    shifts = (np.tile(np.linspace(0, 1, npts, endpoint=False)[:, None], (1, 3))
              + 0.16 / npts * rng.standard_normal((npts, 3))).astype(np.float32)
    slopes = (0.3 * rng.standard_normal((npts, 3)) * 16 / npts).astype(np.float32)
    slopes[0] += 1.0
    return ccm, shifts, slopes, np.array([0.4, 0.35, 0.25, 0.02], np.float32)


def hold_against_returned_guide(tally, port, case, k, grid, out, guide, x):
    """The slice-apply of a fused forward against the oracle fed the guide THE KERNEL returned."""
    want = port.bilateral_slice_apply(grid, guide, x, True)
    tally.held(case, k, "out", out, want, FWD_TOL, FWD_TOL)


@pytest.mark.parametrize("GD", [8, 16])
def test_guide_network_saturates_to_exact_ends(dev, ops, mt_port, GD):
    """An input scaled to [0, 1e3] drives the guide network's logit to thousands: the sigmoid must land on exactly 1.0 where
    the float64 logit is >= 20 (1 - sigmoid(20) = 2e-9 is below half an ulp of 1), within [0, 2 sigmoid(-20) = 4.2e-9]
    where it is <= -20, and on no NaN anywhere (exp of +-1e4 overflows in float32) -- exact sigmoid, fast sigmoid and the
    prescaled layout, which is the plain one bit for bit."""
    frame = LAYOUT_FRAMES["mixed"]
    B, H, W, GH, GW = frame
    rng = np.random.default_rng(600 + GD)
    grid = rng.random((B, GH, GW, GD, 12), dtype=np.float32)
    unit = rng.random((B, H, W, 3), dtype=np.float32)
    c1, c2 = nn_params(rng, 16)
    tg, tc1, tc2 = T(grid, dev), T(c1, dev), T(c2, dev)
    p1, p2 = ops.guide_nn_prescale(tc1, tc2)
    want_k = fused_forward_kernel(B, H, W, GW, GD, "nnguide")
    assert want_k == "apply_fwd_seg/vec4+nnguide"
    tally = Tally()
    for scale in (1e3, 1.2e4):   # the second one carries the logits past +-1e4
        x = (unit * np.float32(scale)).astype(np.float32)
        h = np.maximum(x.astype(np.float64) @ c1[:, :3].astype(np.float64).T + c1[:, 3].astype(np.float64), 0.0)
        logit = h @ c2[:16].astype(np.float64) + float(c2[16])
        hi, lo = logit >= 20.0, logit <= -20.0
        print(f"GD={GD} input in [0, {scale:g}]: float64 logits in [{logit.min():.4g}, {logit.max():.4g}]; >= 20 on {hi.mean():.1%}, "
              f"<= -20 on {lo.mean():.1%}")
        assert hi.mean() >= 0.01 and lo.mean() >= 0.01 and np.abs(logit).max() >= (1e4 if scale > 1e3 else 5e2)
        tx = T(x, dev)
        plain = {}
        for fast in (False, True):
            for prescaled in (False, True):
                a1, a2 = (p1, p2) if prescaled else (tc1, tc2)
                out, g = ops.bilateral_slice_apply_nnguide(tg, tx, a1, a2, return_guide=True, fast_sigmoid=fast,
                                                           prescaled=prescaled)
                k = ops.last_kernel()
                assert k == want_k, k
                out, g = N(out), N(g)
                case = f"nnguide GD={GD} x{scale:g}{' fast' if fast else ''}{' prescaled' if prescaled else ''}"
                assert not np.isnan(g).any() and not np.isnan(out).any(), case
                assert (g[hi] == 1.0).all(), (case, float(g[hi].min()))
                assert (g[lo] >= 0.0).all() and (g[lo] <= 4.2e-9).all(), (case, float(g[lo].min()), float(g[lo].max()))
                assert g.min() >= 0.0 and g.max() <= 1.0, case
                if prescaled:
                    assert np.array_equal(g, plain[fast][1]) and np.array_equal(out, plain[fast][0]), case
                else:
                    plain[fast] = (out, g)
                hold_against_returned_guide(tally, mt_port, case, k, grid, out, g, x)
    tally.done()


@pytest.mark.parametrize("GD", [8, 16])
def test_curves_guide_clips_to_exact_ends(dev, ops, mt_port, GD):
    """The curves guide of an input scaled to [0, 1e3]: inside [0, 1] everywhere, exactly 0 where the float64 value before
    the clip is < -1e-3 and exactly 1 where it is > 1 + 1e-3; each side on at least 1 % of the pixels (seed and colour-matrix
    scale are chosen so that the float64 evaluation alone says so)."""
    frame = LAYOUT_FRAMES["mixed"]
    B, H, W, GH, GW = frame
    rng = np.random.default_rng(701)
    x = (rng.random((B, H, W, 3), dtype=np.float32) * np.float32(1e3)).astype(np.float32)
    curves = curves_params(rng, 16, 0.01)
    grid = np.random.default_rng(610 + GD).random((B, GH, GW, GD, 12), dtype=np.float32)
    ccm, shifts, slopes, mix = (a.astype(np.float64) for a in curves)
    t = x.astype(np.float64) @ ccm[:, :3].T + ccm[:, 3]
    pre = (slopes * np.maximum(t[..., None, :] - shifts, 0.0)).sum(-2) @ mix[:3] + mix[3]
    lo, hi = pre < -1e-3, pre > 1.0 + 1e-3
    print(f"GD={GD}: float64 guide before the clip in [{pre.min():.4g}, {pre.max():.4g}]; < 0 on {lo.mean():.1%}, > 1 on {hi.mean():.1%}")
    assert lo.mean() >= 0.01 and hi.mean() >= 0.01
    assert seg_reaches(B, H, W, GW, GD, io=True)
    tg, tx = T(grid, dev), T(x, dev)
    tcv = tuple(T(a, dev) for a in curves)
    with torch.no_grad():
        out = ops.bilateral_slice_apply_curves(tg, tx, *tcv)
    k = ops.last_kernel()
    assert k == "apply_fwd_io/f32->f32+curvesguide", k
    out2, g = ops.bilateral_slice_apply_io(tg, tx, guide_curves=tcv, return_guide=True)
    assert ops.last_kernel() == k and torch.equal(out, out2)   # the same kernel: its guide is the one the first call used
    out, g = N(out), N(g)
    assert not np.isnan(g).any() and g.min() >= 0.0 and g.max() <= 1.0
    assert (g[lo] == 0.0).all(), float(g[lo].max())
    assert (g[hi] == 1.0).all(), float(g[hi].min())
    tally = Tally()
    hold_against_returned_guide(tally, mt_port, f"curves GD={GD}", k, grid, out, g, x)
    tally.done()


# ---- non-finite guides: they stay in their own pixel ---------------------------------------------------------------------------
NON_FINITE = (np.nan, np.inf, -np.inf, 3e38, -3e38)   # +-3e38 * GD overflows to +-Inf in the kernels' first multiply


@pytest.mark.parametrize("GD", [8, 16])
def test_non_finite_guides_do_not_leak_into_other_pixels(dev, ops, GD):
    """Forward only.  Every kernel clamps the z index it converts from the guide (v_med3_f32 before the conversion in the
    segment and row kernels, whose NaN result is the lower bound; a saturating conversion and clamp_index after it in the
    generic ones), so a NaN, an infinity or an overflowing guide reads inside the grid and spoils its own pixel only: every
    other pixel is bit for bit what the same call gives with 0.5 in the planted places.  The planted pixels themselves are
    not asserted (the reference's int conversion is undefined there), and no gradient is: 0 * NaN inside a matrix-core
    tile legitimately spreads further than the reference's eight corners."""
    kernels = set()

    def pair(frame, family, call, want_k):
        guide, tier = guide_frame(GD, "planted", frame[:3])
        planted = tier != 0
        n = int(planted.sum())
        bad, clean = guide.copy(), guide.copy()
        bad[planted] = np.resize(np.array(NON_FINITE, np.float32), n)
        clean[planted] = 0.5
        op, Cin, Cout, off = FAMILIES[family][:4]
        grid, x, _ = problem_arrays(frame, GD, grid_channels(family), Cin, Cout, 5 * GD)
        outs = []
        for g in (bad, clean):
            outs.append(N(call(T(grid, dev), T(g, dev), T(x, dev), x)))
            k = ops.last_kernel()
            assert k == want_k, (k, want_k)
        kernels.add(k)
        got, want = (o[~planted].view(np.uint32) for o in outs)
        assert np.isfinite(outs[1]).all()
        print(f"GD={GD} [{k}] {family} {frame[:3]}: {n} non-finite guides, {int((got != want).sum())} other values changed")
        assert np.array_equal(got, want), (k, family)

    def plain(tg, tgu, tx, x):
        with torch.no_grad():
            return ops.bilateral_slice_apply(tg, tgu, tx, has_offset=True)

    def sliced(tg, tgu, tx, x):
        with torch.no_grad():
            return ops.bilateral_slice(tg, tgu)

    def scalar(tg, tgu, tx, x):
        with torch.no_grad():
            return ops.bilateral_slice_apply(tg, misaligned(tgu), misaligned(tx), has_offset=True)

    def io_u8(tg, tgu, tx, x):
        raw = torch.from_numpy((x * 255.0).astype(np.uint8)).to(tg.device)
        return ops.bilateral_slice_apply_io(tg, raw, guide=tgu, input_white_level=255.0)

    def generic(fn):
        def call(*a):
            with ops.kernel_override("generic"):
                return fn(*a)
        return call

    frame = LAYOUT_FRAMES["planted"]
    pair(frame, "apply_3_3_off", plain, "apply_fwd_seg/vec4")
    pair(frame, "apply_3_3_off", scalar, "apply_fwd_rows/scalar")
    pair(frame, "apply_3_3_off", io_u8, "apply_fwd_io/u8->f32")
    pair(frame, "slice_12", sliced, "slice_fwd_rows")
    pair(frame, "apply_3_3_off", generic(plain), "apply_fwd_generic")
    pair(frame, "slice_12", generic(sliced), "slice_fwd_generic")
    if GD == 16:
        pair(FALLBACK, "apply_3_3_off", plain, "apply_fwd_rows/vec4")
    print("kernels:", sorted(kernels))
