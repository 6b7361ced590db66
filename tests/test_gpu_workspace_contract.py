"""The workspace contract of include/hdrnet_amd.h -- a buffer of the queried size, "contents undefined on entry and
exit" -- for every entry point that reduces through one: the two slice ops' gradients, the guide networks' VJPs, the input
moments and the l2 loss.

The older tests allocate the workspace with torch.empty and mostly reuse it across calls on the SAME inputs: a kernel
that skipped a partial tile or a partial sum (a task with no pixels, a block past the end of n, a plane half no tap falls
into) while the second stage read it would find the previous call's correct value there.  Here every call runs three
times on a workspace of EXACTLY the queried size between guard bands, holding beforehand

1. 0xFF in every byte (every float a NaN),
2. 0x00 in every byte,
3. what a call on DIFFERENT data of the same shape left behind,

with the outputs prefilled with NaNs between guard bands of their own (an accumulated dinput holds its prior share
instead).  Required: the three results are the same bits; no NaN is left in an output; all guards are intact; the inputs
are unchanged; the first result lies within the suite's existing bars of its reference -- the CPU oracle for the slice
ops (tests/conftest.py, tests/test_gpu_luma_bins.py), float64 for the others (tests/test_gpu_guide_grad_fullsize.py:
1e-5 x the sum of the terms' magnitudes; input moments and the loss: 1e-6 relative) --; the kernel is the fast one.
dconv*, the curve parameters' gradients, sums, moments and the loss are written by a second stage into buffers the
entry point does not expect cleared: their NaN prefill must be harmless too.

Sizes: the slice ops on the frames of tests/test_gpu_grad_plans.py whose tasks end inside cells, and on a frame of 4
columns under a grid of 8, where every other task holds no pixel; the per-pixel ops at
5 004 pixels -- five persistent workgroups, the last one partly filled -- and 1 024, one; the loss at n = 5 000 and n = 4,
where most or nearly all of its 2 048 workgroups see no element.
"""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from conftest import check_dgrid  # noqa: E402
from grad_plan_cases import NAN_BYTE, PRODUCT_FRAMES, Guarded, Problem, frame_id, kernel_name, prepare  # noqa: E402
from test_gpu_guide_grad_fullsize import (NAMES, curves_case, curves_reference, nn_case, nn_reference,  # noqa: E402
                                          param_close, pixel_close)
from test_gpu_luma_bins import check_pix  # noqa: E402

STATES = ("nan", "zero", "other data")
NPX = (5004, 1024)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib
    return prepare(_lib.load())


def three_states(dev, what, nbytes, run, run_other):
    """run(ws) -> {name: Guarded}; run_other(ws): the same call on other data.  -> the first run's outputs, after the
    checks that need no reference: same bits from all three prior states, nothing non-finite, guards intact."""
    assert nbytes > 0, what
    ws = Guarded(nbytes, dev)
    results = []
    for state in STATES:
        if state == "other data":
            for g in run_other(ws).values():
                assert g.intact(), f"{what}: guard band overwritten by the call on other data"
        else:
            ws.body.fill_(NAN_BYTE if state == "nan" else 0)
        outs = run(ws)
        assert ws.intact(), f"{what} [{state}]: guard band of the workspace overwritten"
        for name, g in outs.items():
            assert g.intact(), f"{what} [{state}]: guard band of {name} overwritten"
            assert bool(torch.isfinite(g.t).all()), f"{what} [{state}]: non-finite values left in {name}"
        results.append(outs)
    for state, outs in zip(STATES[1:], results[1:]):
        for name, g in outs.items():
            assert torch.equal(g.t, results[0][name].t), f"{what}: {name} after a workspace of [{state}] differs in bits " \
                                                         f"from [{STATES[0]}]"
    return results[0]


# ---- the slice ops' gradients ----------------------------------------------------------------------------------------
# (family, wanted outputs): the fused pass, the contraction alone, the two channel windows; each at 8 and 16 planes
# ... and one frame narrower than its grid, B, H, W = 2, 24, 4 on 3 x 8: every other x-interval (gx0 = -1, 1, 3, 5, 7) holds
# no pixel, so half of the tasks have nothing to contract and stage 2 still reads their tiles
NO_PIXEL_TASKS_FRAME = (2, 24, 4, 3, 8)
SLICE_CELLS = [("apply_3_3_off", ("dgrid", "dguide", "dinput")), ("apply_3_3_off", ("dgrid",)),
               ("apply_4_4_off", ("dgrid",)), ("slice_12", ("dgrid", "dguide")), ("slice_2", ("dgrid",))]


@pytest.mark.parametrize("GD", [8, 16])
@pytest.mark.parametrize("family,wanted", SLICE_CELLS, ids=lambda v: v if isinstance(v, str) else "+".join(v))
@pytest.mark.parametrize("frame", PRODUCT_FRAMES + [NO_PIXEL_TASKS_FRAME], ids=frame_id)
def test_slice_gradients_ignore_what_the_workspace_held(dev, lib, port, frame, family, wanted, GD):
    p = Problem(port, dev, frame, family, GD, seed=sum(frame) + GD + len(family))
    other = Problem(None, dev, frame, family, GD, seed=977 + GD, oracle=False)
    what = f"{frame_id(frame)} {family} gd{GD} [{','.join(wanted)}]"

    def run(prob):
        def go(ws):
            name, outs = prob.call(lib, wanted, ws)
            assert name == kernel_name(family, wanted), (what, name)
            return outs
        return go

    first = three_states(dev, what, p.query(lib), run(p), run(other))
    p.check(first, what, check_dgrid, check_pix)
    assert p.inputs_unchanged() and other.inputs_unchanged()


# ---- the guide networks' VJPs, the input moments, the loss -----------------------------------------------------------
def stream():
    return torch.cuda.current_stream().cuda_stream


def last_kernel(lib):
    return lib.hdrnet_last_kernel().decode()


def unchanged(tensors, copies):
    return all(torch.equal(a, b) for a, b in zip(tensors, copies))


@pytest.mark.parametrize("accumulate", [False, True], ids=["stored", "accumulated"])
@pytest.mark.parametrize("Cin,n", [(3, 16), (3, 4), (1, 16), (1, 4)])
@pytest.mark.parametrize("npx", NPX)
def test_pointwise_guide_grad_ignores_what_the_workspace_held(dev, lib, npx, Cin, n, accumulate):
    x, c1, c2, dguide = nn_case(dev, Cin, n, npx, seed=Cin * 100 + n + npx)
    # a pixel within rounding of the ReLU's kink carries a term float32 and float64 may count differently: its dguide is
    # zero on both sides (as tests/test_gpu_guide_grad_fullsize.py does for the curves)
    kink = nn_reference(x, dguide, c1, c2)[4]
    dguide = torch.where(kink, torch.zeros_like(dguide), dguide)
    ref, din64, sin64, guide, _ = nn_reference(x, dguide, c1, c2)
    prefill = torch.randn((npx, Cin), device=dev)
    x2, _, _, dguide2 = nn_case(dev, Cin, n, npx, seed=7)
    guide2 = nn_reference(x2, dguide2, c1, c2)[3]
    inputs = (x, guide, dguide, c1, c2)
    copies = [t.clone() for t in inputs]
    nbytes = lib.hdrnet_pointwise_guide_grad_workspace_bytes(npx, Cin, n)
    what = f"guide_nn_grad npx={npx} Cin={Cin} n={n} dinput {'accumulated' if accumulate else 'stored'}"

    def run(xx, gg, dg):
        def go(ws):
            outs = dict(dinput=Guarded.floats((npx, Cin), dev, prefill if accumulate else None),
                        dconv1=Guarded.floats(c1.shape, dev), dconv2=Guarded.floats(c2.shape, dev))
            rc = lib.hdrnet_pointwise_guide_grad_f32(xx.data_ptr(), gg.data_ptr(), dg.data_ptr(), c1.data_ptr(), c2.data_ptr(),
                                                     outs["dinput"].ptr(), int(accumulate), outs["dconv1"].ptr(),
                                                     outs["dconv2"].ptr(), npx, Cin, n, ws.ptr(), ws.nbytes, stream())
            assert rc == 0, lib.hdrnet_last_error().decode()
            torch.cuda.synchronize()
            assert last_kernel(lib) == "guide_nn_grad", last_kernel(lib)
            return outs
        return go

    first = three_states(dev, what, nbytes, run(x, guide, dguide), run(x2, guide2, dguide2))
    param_close(what + " dconv1", first["dconv1"].t, ref["dc1"], ref["s1"])
    param_close(what + " dconv2", first["dconv2"].t, ref["dc2"], ref["s2"])
    got = first["dinput"].t.double() - prefill.double() if accumulate else first["dinput"].t
    scale = sin64 + (prefill.double().abs() * 2 ** -23 / 1e-5 if accumulate else 0)   # + the float32 add's rounding
    pixel_close(what + " dinput", got, din64, scale, torch.zeros_like(din64, dtype=torch.bool))
    assert unchanged(inputs, copies)


@pytest.mark.parametrize("accumulate", [False, True], ids=["stored", "accumulated"])
@pytest.mark.parametrize("npx", NPX)
def test_curves_guide_grad_ignores_what_the_workspace_held(dev, lib, npx, accumulate):
    x, params, dguide = curves_case(dev, npx, seed=npx % 7 + 40)
    kink = curves_reference(x, params, dguide)[4]
    dguide = torch.where(kink, torch.zeros_like(dguide), dguide)
    grads, sums, din64, sin64, _, _ = curves_reference(x, params, dguide)
    prefill = torch.randn((npx, 3), device=dev)
    x2, _, dguide2 = curves_case(dev, npx, seed=3)
    inputs = (x, dguide) + tuple(params)
    copies = [t.clone() for t in inputs]
    nbytes = lib.hdrnet_curves_guide_grad_workspace_bytes(npx, 3, 16)
    what = f"curves_guide_grad npx={npx} dinput {'accumulated' if accumulate else 'stored'}"

    def run(xx, dg):
        def go(ws):
            outs = dict(dinput=Guarded.floats((npx, 3), dev, prefill if accumulate else None))
            outs.update({nm: Guarded.floats(p.shape, dev) for nm, p in zip(NAMES, params)})
            rc = lib.hdrnet_curves_guide_grad_f32(xx.data_ptr(), dg.data_ptr(), *[p.data_ptr() for p in params],
                                                  outs["dinput"].ptr(), int(accumulate), *[outs[nm].ptr() for nm in NAMES],
                                                  npx, 3, 16, ws.ptr(), ws.nbytes, stream())
            assert rc == 0, lib.hdrnet_last_error().decode()
            torch.cuda.synchronize()
            assert last_kernel(lib) == "curves_guide_grad", last_kernel(lib)
            return outs
        return go

    first = three_states(dev, what, nbytes, run(x, dguide), run(x2, dguide2))
    for nm, w, s in zip(NAMES, grads, sums):
        param_close(f"{what} {nm}", first[nm].t, w, s)
    got = first["dinput"].t.double() - prefill.double() if accumulate else first["dinput"].t
    scale = sin64 + (prefill.double().abs() * 2 ** -23 / 1e-5 if accumulate else 0)
    pixel_close(what + " dinput", got, din64, scale, torch.zeros_like(din64, dtype=torch.bool))
    assert unchanged(inputs, copies)


@pytest.mark.parametrize("Cin", [3, 1])
@pytest.mark.parametrize("npx", NPX)
def test_input_moments_ignore_what_the_workspace_held(dev, lib, npx, Cin):
    gen = torch.Generator(device=dev).manual_seed(npx + Cin)
    x = torch.rand((npx, Cin), device=dev, generator=gen)
    x2 = 0.3 + 0.5 * torch.rand((npx, Cin), device=dev, generator=gen)
    copy = x.clone()
    nbytes = lib.hdrnet_input_moments_workspace_bytes(npx, Cin)
    what = f"input_moments npx={npx} Cin={Cin}"

    def run(xx):
        def go(ws):
            outs = dict(sums=Guarded.floats((Cin,), dev), moments=Guarded.floats((Cin, Cin), dev))
            rc = lib.hdrnet_input_moments_f32(xx.data_ptr(), npx, Cin, outs["sums"].ptr(), outs["moments"].ptr(), ws.ptr(),
                                              ws.nbytes, stream())
            assert rc == 0, lib.hdrnet_last_error().decode()
            torch.cuda.synchronize()
            assert last_kernel(lib) == "input_moments", last_kernel(lib)
            return outs
        return go

    first = three_states(dev, what, nbytes, run(x), run(x2))
    flat = x.double()
    for nm, want in (("sums", flat.sum(0)), ("moments", flat.t() @ flat)):
        err = (first[nm].t.double() - want).abs()
        worst = float((err / (1e-6 * want.abs())).max())
        print(f"{what} {nm}: max|err| = {float(err.max()):.3e}, worst / (1e-6 |want|) = {worst:.2f}")
        assert worst <= 1.0
    assert torch.equal(x, copy)


@pytest.mark.parametrize("n", [5000, 4])
def test_l2_loss_ignores_what_the_workspace_held(dev, lib, n):
    gen = torch.Generator(device=dev).manual_seed(n)
    t, p = torch.rand((n,), device=dev, generator=gen), torch.rand((n,), device=dev, generator=gen)
    t2, p2 = torch.rand((n,), device=dev, generator=gen), 3.0 * torch.rand((n,), device=dev, generator=gen)
    copies = (t.clone(), p.clone())
    nbytes = lib.hdrnet_l2_loss_workspace_bytes(n)
    what = f"l2_loss n={n}"

    def run(pp, tt):
        def go(ws):
            outs = dict(loss=Guarded.floats((1,), dev))
            rc = lib.hdrnet_l2_loss_f32(pp.data_ptr(), tt.data_ptr(), n, outs["loss"].ptr(), ws.ptr(), ws.nbytes, stream())
            assert rc == 0, lib.hdrnet_last_error().decode()
            torch.cuda.synchronize()
            assert last_kernel(lib) == "l2_loss", last_kernel(lib)
            return outs
        return go

    first = three_states(dev, what, nbytes, run(p, t), run(p2, t2))
    want = float((p.double() - t.double()).square().mean())
    err = abs(float(first["loss"].t[0]) - want)
    print(f"{what}: loss |err| = {err:.3e}, worst / (1e-6 want) = {err / (1e-6 * want):.3f}")
    assert err <= 1e-6 * want
    assert unchanged((t, p), copies)
