"""Sample preparation on the GPU (csrc/sample_prep.hip through hdrnet_amd/data.py) against the numpy reference of
tests/test_sample_prep.py.  The operation is a permutation plus one correctly rounded division, so EVERY comparison is
bit-exact (np.array_equal on the fp32 bits); there is no tolerance.  Outputs are pre-filled with NaN and sit between
guard bands whose bytes are checked after each launch.

The 64 x 40 source of the alignment sweep is 64 rows of 40 pixels: with W = 36 an even turn leaves crop_x only 0 .. 4
(an odd turn 0 .. 28), so the sweep 0 .. 7 is taken modulo the room of each record; with W = 4 it is complete."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_sample_prep import reference_lowres, reference_sample  # noqa: E402

GUARD = 64  # floats on either side of every output
SENTINEL = 0x5A5A5A5A
GEOMETRIES = list(itertools.product((0, 1), (0, 1), (0, 1, 2, 3)))  # (flip_lr, flip_ud, rot90)
FORMATS = {"u8": (np.uint8, 255.0), "u16": (np.uint16, 65535.0), "u16_hdrp": (np.uint16, 32767.0), "f32": (np.float32, 1.0)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    return torch.device("cuda:0")


def make_sources(rng, dtype, shape):
    if dtype == np.float32:
        return rng.standard_normal(shape).astype(np.float32)
    return rng.integers(0, np.iinfo(dtype).max + 1, shape, dtype=np.int64).astype(dtype)


def to_dev(a, dev):
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)
    return torch.from_numpy(a).to(dev)


class Guarded:
    """A NaN-filled float32 tensor of `shape` between two guard bands of SENTINEL words."""

    def __init__(self, shape, dev):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
        words = self.buf.view(torch.int32)
        words[:GUARD] = SENTINEL
        words[GUARD + n:] = SENTINEL
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        assert self.t.data_ptr() % 16 == 0

    def result(self):
        w = self.buf.view(torch.int32).cpu().numpy()
        n = w.size - 2 * GUARD
        assert (w[:GUARD] == SENTINEL).all() and (w[GUARD + n:] == SENTINEL).all(), "guard band overwritten"
        return self.t.cpu().numpy()


def bits_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    same = got.view(np.uint32) == want.view(np.uint32)
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} words differ, first at {np.argwhere(~same)[0]}"


def run_and_check(dev, src_in, wl_in, src_tg, wl_tg, ops, H, W, n, even=False, want=(True, True, True), device_table=False,
                  expect_ops=None, what=""):
    """prepare_batch into guarded buffers; every requested output bit-equal to the numpy reference of `expect_ops`."""
    from hdrnet_amd import data
    B = src_in.shape[0] if ops is None else ops.shape[0]
    t_in, t_tg = to_dev(src_in, dev), (None if src_tg is None else to_dev(src_tg, dev))
    shapes = ((B, n, n, 3), (B, H, W, 3), (B, H, W, 3))
    g = [Guarded(s, dev) if w else None for s, w in zip(shapes, want)]
    table = None
    if ops is not None:
        table = torch.from_numpy(np.ascontiguousarray(ops, dtype=np.int32))
        if device_table:
            table = table.to(dev)
    res = data.prepare_batch(t_in, t_tg, table, (H, W), n, wl_in, wl_tg, out=[None if x is None else x.t for x in g],
                             even_turns_only=even)
    torch.cuda.synchronize(dev)
    assert [r is None for r in res] == [x is None for x in g]
    got = [None if x is None else x.result() for x in g]
    ref_ops = expect_ops if expect_ops is not None else (
        ops if ops is not None else np.array([[b, 0, 0, 0, 0, 0, 0, 0] for b in range(B)]))
    for b in range(B):
        full, low = reference_sample(src_in, ref_ops[b], H, W, wl_in, n)
        if got[0] is not None:
            bits_equal(got[0][b], low, f"{what} lowres_input[{b}] op {list(ref_ops[b][:6])}")
        if got[1] is not None:
            bits_equal(got[1][b], full, f"{what} image_input[{b}] op {list(ref_ops[b][:6])}")
        if got[2] is not None:
            tg, _ = reference_sample(src_tg, ref_ops[b], H, W, wl_tg, n)
            bits_equal(got[2][b], tg, f"{what} image_target[{b}] op {list(ref_ops[b][:6])}")
    return got


def geometry_table(rng, N, Hs, Ws, H, W, crop_x=None, extremes=True):
    """One record per geometry, random source and crop offsets (the first records take the extreme offsets)."""
    rows = []
    for k, (flr, fud, rot) in enumerate(GEOMETRIES):
        Hr, Wr = (Ws, Hs) if rot & 1 else (Hs, Ws)
        cy, cx = int(rng.integers(0, Hr - H + 1)), int(rng.integers(0, Wr - W + 1))
        if extremes and k % 4 == 0:
            cy, cx = Hr - H, Wr - W
        if extremes and k % 4 == 1:
            cy, cx = 0, 0
        if crop_x is not None:
            cx = crop_x % (Wr - W + 1)
        rows.append([int(rng.integers(0, N)), flr, fud, rot, cy, cx, 0, 0])
    return np.array(rows, dtype=np.int32)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_all_geometries_on_an_odd_pitch_source(dev, fmt):
    dtype, wl = FORMATS[fmt]
    rng = np.random.default_rng(11)
    N, Hs, Ws, H, W, n = 3, 37, 53, 24, 28, 16
    src = make_sources(rng, dtype, (N, Hs, Ws, 3))
    tgt = make_sources(rng, dtype, (N, Hs, Ws, 3))
    for rep in range(2):
        ops = geometry_table(rng, N, Hs, Ws, H, W, extremes=rep == 0)
        run_and_check(dev, src, wl, tgt, wl, ops, H, W, n, what=fmt)
    # nearly the whole source: one pixel of room in one direction of either orientation
    ops = geometry_table(rng, N, Hs, Ws, 36, 36)
    run_and_check(dev, src, wl, tgt, wl, ops, 36, 36, 20, what=fmt + " 36x36")


@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("W", [4, 36])
def test_every_byte_alignment_of_a_row_start(dev, fmt, W):
    dtype, wl = FORMATS[fmt]
    rng = np.random.default_rng(12)
    N, Hs, Ws, H, n = 2, 64, 40, 30, 12
    src = make_sources(rng, dtype, (N, Hs, Ws, 3))
    tgt = make_sources(rng, dtype, (N, Hs, Ws, 3))
    ops = np.concatenate([geometry_table(rng, N, Hs, Ws, H, W, crop_x=cx, extremes=False) for cx in range(8)])
    assert ops.shape[0] == 128
    if W == 4:
        assert sorted(set(ops[:, 5])) == list(range(8))
    run_and_check(dev, src, wl, tgt, wl, ops, H, W, n, what=f"{fmt} W={W}")


def test_target_dtype_differs_from_input_dtype(dev):
    """HDR+: u16 / 32767 in, u8 / 255 out -- one table, two dtypes, two white levels."""
    rng = np.random.default_rng(13)
    N, Hs, Ws, H, W, n = 3, 37, 53, 24, 28, 16
    src = make_sources(rng, np.uint16, (N, Hs, Ws, 3))
    tgt = make_sources(rng, np.uint8, (N, Hs, Ws, 3))
    run_and_check(dev, src, 32767.0, tgt, 255.0, geometry_table(rng, N, Hs, Ws, H, W), H, W, n, what="u16 -> u8")
    run_and_check(dev, tgt, 255.0, make_sources(rng, np.float32, (N, Hs, Ws, 3)), 1.0,
                  geometry_table(rng, N, Hs, Ws, H, W), H, W, n, what="u8 -> f32")


@pytest.mark.parametrize("want", [(False, True, True), (True, False, True), (True, True, False), (True, False, False),
                                  (False, False, True)])
def test_each_output_is_optional(dev, want):
    rng = np.random.default_rng(14)
    N, Hs, Ws, H, W, n = 3, 37, 53, 24, 28, 16
    src, tgt = make_sources(rng, np.uint8, (N, Hs, Ws, 3)), make_sources(rng, np.uint16, (N, Hs, Ws, 3))
    run_and_check(dev, src, 255.0, tgt, 65535.0, geometry_table(rng, N, Hs, Ws, H, W), H, W, n, want=want, what=str(want))
    if not want[2]:
        run_and_check(dev, src, 255.0, None, None, geometry_table(rng, N, Hs, Ws, H, W), H, W, n, want=want, what="no target")


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_null_table_is_the_identity(dev, fmt):
    dtype, wl = FORMATS[fmt]
    rng = np.random.default_rng(15)
    src, tgt = make_sources(rng, dtype, (3, 64, 40, 3)), make_sources(rng, dtype, (3, 64, 40, 3))
    run_and_check(dev, src, wl, tgt, wl, None, 64, 40, 24, what=fmt)


def test_out_of_range_records_give_the_clamped_sample(dev):
    """A DEVICE table is not validated: index and crop offsets are clamped, turns and flips masked (documented in
    include/hdrnet_amd_train.h) -- a caller error with a defined result and no out-of-bounds access."""
    rng = np.random.default_rng(16)
    N, Hs, Ws, H, W, n = 3, 37, 53, 24, 28, 16
    src, tgt = make_sources(rng, np.uint8, (N, Hs, Ws, 3)), make_sources(rng, np.uint16, (N, Hs, Ws, 3))
    big = 2 ** 31 - 1
    bad = np.array([[-3, 0, 0, 0, 2, 3, 0, 0], [99, 0, 0, 0, 2, 3, 5, 5], [big, 1, 1, 1, big, big, 0, 0],
                    [-big - 1, 0, 0, 2, -big - 1, -big - 1, 0, 0], [1, 3, 2, 7, 1000, -5, 0, 0], [1, -1, -2, -1, -7, 1000, 0, 0],
                    [2, 0, 0, 5, 30, 10, 0, 0], [0, 0, 0, 4, 14, 26, -1, -1]], dtype=np.int64)
    good = np.array([[0, 0, 0, 0, 2, 3, 0, 0], [2, 0, 0, 0, 2, 3, 0, 0], [2, 1, 1, 1, Ws - H, Hs - W, 0, 0],
                     [0, 0, 0, 2, 0, 0, 0, 0], [1, 1, 0, 3, Ws - H, 0, 0, 0], [1, 1, 0, 3, 0, Hs - W, 0, 0],
                     [2, 0, 0, 1, Ws - H, Hs - W, 0, 0], [0, 0, 0, 0, Hs - H, Ws - W, 0, 0]], dtype=np.int64)
    run_and_check(dev, src, 255.0, tgt, 65535.0, bad.astype(np.int32), H, W, n, device_table=True, expect_ops=good,
                  what="clamped")
    # even_turns_only reads rot90 & 2
    bad = np.array([[0, 0, 0, 1, 5, 5, 0, 0], [1, 1, 0, 3, 5, 5, 0, 0], [1, 0, 1, 7, 500, 500, 0, 0]], dtype=np.int32)
    good = np.array([[0, 0, 0, 0, 5, 5, 0, 0], [1, 1, 0, 2, 5, 5, 0, 0], [1, 0, 1, 2, Hs - H, Ws - W, 0, 0]])
    run_and_check(dev, src, 255.0, tgt, 65535.0, bad, H, W, n, even=True, device_table=True, expect_ops=good, what="even only")
    # a CPU table is validated instead
    from hdrnet_amd import data
    with pytest.raises(ValueError, match="source index"):
        data.prepare_batch(to_dev(src, dev), None, torch.tensor([[5, 0, 0, 0, 0, 0, 0, 0]], dtype=torch.int32), (H, W), n)


@pytest.mark.parametrize("n", [256, 200])
def test_frame_size_even_turns(dev, n):
    """N = 6 u8 pairs of 1200 x 2000 -> 4 crops of 1080 x 1920: odd turns cannot fit, HDRNET_SAMPLE_EVEN_TURNS_ONLY."""
    from hdrnet_amd import data
    rng = np.random.default_rng(17)
    N, Hs, Ws, H, W = 6, 1200, 2000, 1080, 1920
    src, tgt = make_sources(rng, np.uint8, (N, Hs, Ws, 3)), make_sources(rng, np.uint8, (N, Hs, Ws, 3))
    with pytest.raises(ValueError, match="turned by 90 degrees"):
        data.draw_ops(4, N, (Hs, Ws), (H, W))
    ops = data.draw_ops(4, N, (Hs, Ws), (H, W), rotate="even", generator=torch.Generator().manual_seed(n)).numpy()
    ops[:, 3] = [0, 2, 2, 0]
    ops[:, 1] = [1, 0, 1, 0]
    run_and_check(dev, src, 255.0, tgt, 255.0, ops, H, W, n, even=True, device_table=True, what=f"1080p even n={n}")
    with pytest.raises(Exception, match="turned by 90 degrees"):
        data.prepare_batch(to_dev(src, dev), None, to_dev(ops, dev), (H, W), n)  # without the flag: refused


@pytest.mark.parametrize("fmt,n", [("u8", 256), ("u16_hdrp", 200)])
def test_frame_size_all_turns_from_square_sources(dev, fmt, n):
    dtype, wl = FORMATS[fmt]
    rng = np.random.default_rng(18)
    N, Hs, Ws, H, W = 2, 2048, 2048, 1080, 1920
    src = make_sources(rng, dtype, (N, Hs, Ws, 3))
    tgt = make_sources(rng, np.uint8, (N, Hs, Ws, 3))
    ops = np.array([[0, 0, 0, 0, 7, 13, 0, 0], [1, 1, 0, 1, 968, 1, 0, 0], [0, 0, 1, 2, 500, 128, 0, 0],
                    [1, 1, 1, 3, 3, 127, 0, 0]], dtype=np.int32)
    run_and_check(dev, src, wl, tgt, 255.0, ops, H, W, n, what=f"1080p all turns {fmt}")


@pytest.mark.parametrize("fmt,B,H,W", [("u8", 1, 2160, 3840), ("u16_hdrp", 1, 3000, 4000), ("f32", 4, 1080, 1920)])
@pytest.mark.parametrize("n", [256, 200])
def test_lowres_input_of_whole_frames(dev, fmt, B, H, W, n):
    from hdrnet_amd import data
    dtype, wl = FORMATS[fmt]
    rng = np.random.default_rng(19)
    frames = make_sources(rng, dtype, (B, H, W, 3))
    t = to_dev(frames, dev)
    g = Guarded((B, n, n, 3), dev)
    assert data.lowres_input(t, n, wl, out=g.t) is g.t
    got = g.result()
    for b in range(B):
        full = frames[b] if dtype == np.float32 else frames[b].astype(np.float32) / np.float32(wl)
        bits_equal(got[b], reference_lowres(full, n), f"lowres_input {fmt} [{b}]")
    low2 = torch.full((B, n, n, 3), float("nan"), device=dev)
    data.prepare_batch(t, None, None, (H, W), n, wl, out=(low2, None, None))
    bits_equal(low2.cpu().numpy(), got, "lowres_input == prepare_batch(identity)")
    if wl in (255.0, 65535.0, 1.0):  # the default white level is the dtype's
        bits_equal(data.lowres_input(t, n).cpu().numpy(), got, "default white level")


def test_capture_and_replay_with_a_new_table(dev):
    from hdrnet_amd import data
    rng = np.random.default_rng(20)
    N, Hs, Ws, H, W, n, B = 5, 64, 72, 40, 48, 32, 4
    src, tgt = make_sources(rng, np.uint8, (N, Hs, Ws, 3)), make_sources(rng, np.uint16, (N, Hs, Ws, 3))
    t_in, t_tg = to_dev(src, dev), to_dev(tgt, dev)
    gen = torch.Generator().manual_seed(2)
    draws = [data.draw_ops(B, N, (Hs, Ws), (H, W), generator=gen) for _ in range(3)]
    assert not torch.equal(draws[0], draws[1])
    table = draws[0].to(dev)
    outs = [Guarded(s, dev) for s in ((B, n, n, 3), (B, H, W, 3), (B, H, W, 3))]
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        data.prepare_batch(t_in, t_tg, table, (H, W), n, out=[o.t for o in outs])
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        data.prepare_batch(t_in, t_tg, table, (H, W), n, out=[o.t for o in outs])

    def replay_and_check(ops):
        for o in outs:
            o.t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize(dev)
        got = [o.result() for o in outs]
        for b in range(B):
            full, low = reference_sample(src, ops[b], H, W, 255.0, n)
            tg, _ = reference_sample(tgt, ops[b], H, W, 65535.0, n)
            bits_equal(got[0][b], low, "replay lowres")
            bits_equal(got[1][b], full, "replay input")
            bits_equal(got[2][b], tg, "replay target")
        return got

    replay_and_check(draws[0].numpy())
    table.copy_(draws[1])  # the 128-byte copy: the graph holds the table's address, not its contents
    second = replay_and_check(draws[1].numpy())
    again = replay_and_check(draws[1].numpy())
    for a, b in zip(second, again):
        bits_equal(a, b, "two replays of one table")


def test_training_step_fed_by_the_device_dataset(dev):
    """Config #4's step (GraphedTrainStep, HDRNetPointwiseNNGuide, flat Adam) at 4 x 270 x 480 fed through
    DeviceDataset.feed, and the same module state fed the numpy-prepared batches: the inputs are bit-equal, so the losses
    of three steps must be too; feed() stages nothing."""
    from hdrnet_amd import data, metrics, models, optim
    from hdrnet_amd.runtime import GraphedTrainStep
    rng = np.random.default_rng(21)
    N, Hs, Ws, B, H, W, n = 6, 520, 500, 4, 270, 480, 256
    src, tgt = make_sources(rng, np.uint16, (N, Hs, Ws, 3)), make_sources(rng, np.uint8, (N, Hs, Ws, 3))
    wl_in, wl_tg = 32767.0, 255.0
    ds = data.DeviceDataset(to_dev(src, dev), to_dev(tgt, dev), wl_in, wl_tg, output_resolution=(H, W), net_input_size=n,
                            generator=torch.Generator().manual_seed(4))
    tables = [ds.draw(B) for _ in range(3)]
    assert {int(v) for t in tables for v in t[:, 3]} == {0, 1, 2, 3}

    def numpy_batch(ops):
        parts = [reference_sample(src, op, H, W, wl_in, n) for op in ops.numpy()]
        tg = [reference_sample(tgt, op, H, W, wl_tg, n)[0] for op in ops.numpy()]
        return [torch.from_numpy(np.stack(x)).to(dev) for x in ([p[1] for p in parts], [p[0] for p in parts], tg)]

    torch.manual_seed(3)
    state = {k: v.clone() for k, v in models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).to(dev).state_dict().items()}
    losses = []
    for fed in ("numpy", "dataset"):
        m = models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).to(dev).train()
        m.load_state_dict(state)
        opt = optim.FlatAdam([p for p in m.parameters() if p.requires_grad], lr=1e-4, epsilon_hat=True)
        low0, full0, tgt0 = numpy_batch(tables[0])
        step = GraphedTrainStep(m, lambda out, t: metrics.l2_loss(t, out), opt, [low0, full0], [tgt0], warmup=2,
                                flat_bucket=True)
        got = []
        for ops in tables:
            if fed == "numpy":
                low, full, target = numpy_batch(ops)
                loss = step([low, full], [target])
            else:
                inputs, targets = ds.feed(step, ops=ops)
                assert [t.data_ptr() for t in inputs + targets] == [t.data_ptr() for t in step.static_inputs + step.static_targets]
                low, full, target = numpy_batch(ops)
                assert torch.equal(inputs[0], low) and torch.equal(inputs[1], full) and torch.equal(targets[0], target)
                loss = step(inputs, targets)
            got.append(float(loss.detach()))
        assert all(np.isfinite(got)) and len(set(got)) == 3, got
        losses.append(got)
    print("losses", losses)
    assert losses[0] == losses[1], losses


def _model(cls, dev, seed=7):
    from hdrnet_amd import models
    torch.manual_seed(seed)
    return getattr(models, cls)(dict(batch_norm=False)).to(dev).eval()


@pytest.mark.parametrize("cls", ["HDRNetCurves", "HDRNetPointwiseNNGuide"])
def test_process_of_a_float_frame_is_forward(dev, cls):
    from hdrnet_amd.runtime import FrameInference
    m = _model(cls, dev)
    rng = np.random.default_rng(22)
    frame = rng.random((1, 1080, 1920, 3), dtype=np.float32)
    low = torch.from_numpy(reference_lowres(frame[0], 256)[None]).to(dev)
    t = torch.from_numpy(frame).to(dev)
    with torch.no_grad():
        want = m(low, t)
    got = m.process(t)
    assert got.dtype == torch.float32 and torch.isfinite(got).all()
    bits_equal(got.cpu().numpy(), want.cpu().numpy(), f"{cls}.process(f32)")
    fi = FrameInference(m, t)
    other = torch.from_numpy(rng.random((1, 1080, 1920, 3), dtype=np.float32)).to(dev)
    bits_equal(fi(other).cpu().numpy(), m.process(other).cpu().numpy(), f"{cls} FrameInference replay")
    bits_equal(fi(t).cpu().numpy(), want.cpu().numpy(), f"{cls} FrameInference replay, first frame")


@pytest.mark.parametrize("cls", ["HDRNetCurves", "HDRNetPointwiseNNGuide"])
@pytest.mark.parametrize("H,W", [(1080, 1920), (2160, 3840)])
def test_process_of_a_u8_frame_is_the_io_op_by_hand(dev, cls, H, W):
    from hdrnet_amd import hdrnet_ops
    from hdrnet_amd.runtime import FrameInference
    m = _model(cls, dev)
    rng = np.random.default_rng(23)
    frame = make_sources(rng, np.uint8, (1, H, W, 3))
    t = to_dev(frame, dev)
    low = torch.from_numpy(reference_lowres(frame[0].astype(np.float32) / np.float32(255), 256)[None]).to(dev)
    with torch.no_grad():
        coeffs = m.coefficients(low)
        gs = coeffs.shape
        grid = coeffs.reshape(gs[0], gs[1], gs[2], gs[3], gs[4] * gs[5])
        if cls == "HDRNetCurves":
            kw = dict(guide_curves=m.guide.exported(), curves_prepared=m.guide.prepared() if m.prepare_curves else None)
        else:
            c1, c2, pre = m.guide.inference_params(m.prescale_guide)
            kw = dict(guide_conv1=c1, guide_conv2=c2, prescaled=pre, fast_sigmoid=m.fast_sigmoid)
        want = hdrnet_ops.bilateral_slice_apply_io(grid, t, out_dtype=torch.uint8, **kw)
    got = m.process(t, out_dtype=torch.uint8)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, H, W, 3)
    assert torch.equal(got, want)
    assert len(torch.unique(got)) > 8  # a picture, not a constant
    fi = FrameInference(m, t, out_dtype=torch.uint8)
    other = to_dev(make_sources(rng, np.uint8, (1, H, W, 3)), dev)
    assert torch.equal(fi(other), m.process(other, out_dtype=torch.uint8))
    # u16 / 32767 in, f32 out: the same op with the other wire format
    f16 = make_sources(rng, np.uint16, (1, H, W, 3))
    t16 = to_dev(f16, dev)
    low16 = torch.from_numpy(reference_lowres(f16[0].astype(np.float32) / np.float32(32767), 256)[None]).to(dev)
    with torch.no_grad():
        c = m.coefficients(low16)
        want16 = hdrnet_ops.bilateral_slice_apply_io(c.reshape(gs[0], gs[1], gs[2], gs[3], gs[4] * gs[5]), t16,
                                                     input_white_level=32767.0, **kw)
    bits_equal(m.process(t16, white_level=32767.0).cpu().numpy(), want16.cpu().numpy(), f"{cls}.process(u16)")


def test_pyramid_process_takes_float_frames_only(dev):
    m = _model("HDRNetGaussianPyrNN", dev)
    rng = np.random.default_rng(24)
    with pytest.raises(TypeError, match="float32"):
        m.process(torch.zeros(1, 272, 480, 3, dtype=torch.uint8, device=dev))
    with pytest.raises(TypeError, match="float32"):
        m.process(torch.zeros(1, 272, 480, 3, dtype=torch.uint16, device=dev))
    frame = rng.random((1, 272, 480, 3), dtype=np.float32)
    t = torch.from_numpy(frame).to(dev)
    low = torch.from_numpy(reference_lowres(frame[0], 256)[None]).to(dev)
    with torch.no_grad():
        want = m(low, t)
    bits_equal(m.process(t).cpu().numpy(), want.cpu().numpy(), "pyramid process(f32)")
    with pytest.raises(TypeError, match="float32 frames only"):
        m.process(t, out_dtype=torch.uint8)
