"""Sample preparation from a packed set of images of mixed extents on the GPU (the RAGGED flavour of
csrc/sample_prep.hip through data.prepare_batch_ragged / data.RaggedDeviceDataset) against the numpy reference of
tests/test_sample_prep.py.  As in tests/test_gpu_sample_prep.py EVERY comparison of pixel data is bit-exact, outputs are
pre-filled with NaN and sit between guard bands.

The flat source buffers are carved out of a larger allocation filled with a marker byte: the data ends on its last
dword, there is no slack behind it, and whatever a wrong index reads next to an image -- a neighbour or the marker --
shows in the comparison.

The geometry cases run on the base set (portrait, landscape, square and exactly crop-sized images) and on the base set
plus two images: packed as u8 the base set alone starts its images at bytes = 0, 3, 3, 2, 2, 2 (mod 4), the longer set
adds a start = 1 (asserted in `packed`)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_sample_prep import FORMATS, GEOMETRIES, Guarded, bits_equal, make_sources, to_dev  # noqa: E402
from test_sample_prep import reference_sample  # noqa: E402
from test_sample_prep_ragged import EXTENDED, SIZES  # noqa: E402

SETS = {"base": SIZES, "extended": EXTENDED}
MARKER = 0xA5
H0 = W0 = 32  # the crop of the geometry cases


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need an MI355X"
    return torch.device("cuda:0")


def embed(flat, dev):
    """The CPU buffer `flat` on the device, inside a marker-filled allocation: 16 marker bytes before it, and after its
    last dword markers again."""
    nbytes = flat.numel() * flat.element_size()
    big = torch.full((16 + (nbytes + 3) // 4 * 4 + 64,), MARKER, dtype=torch.uint8, device=dev)
    big[16:16 + nbytes] = flat.view(torch.uint8).to(dev)
    view = big[16:16 + nbytes].view(flat.dtype)
    assert view.data_ptr() % 4 == 0 and view.numel() == flat.numel()
    return view


class Packed:
    """Arrays of the given extents, packed with data.pack_images and embedded on the device."""

    def __init__(self, dev, sizes, dtype_in, dtype_tg, seed, arrays_in=None):
        from hdrnet_amd import data
        rng = np.random.default_rng(seed)
        self.sizes = list(sizes)
        self.arrays_in = arrays_in or [make_sources(rng, dtype_in, (h, w, 3)) for h, w in sizes]
        self.arrays_tg = None if dtype_tg is None else [make_sources(rng, dtype_tg, (h, w, 3)) for h, w in sizes]
        flat, self.table = data.pack_images([to_dev(a, "cpu") for a in self.arrays_in])
        self.flat_in = embed(flat, dev)
        self.flat_tg = None
        if self.arrays_tg is not None:
            flat, table = data.pack_images([to_dev(a, "cpu") for a in self.arrays_tg])
            assert torch.equal(table, self.table)  # one table for both buffers
            self.flat_tg = embed(flat, dev)


def packed(dev, set_name, fmt_in, fmt_tg, seed):
    from hdrnet_amd import data
    p = Packed(dev, SETS[set_name], FORMATS[fmt_in][0], None if fmt_tg is None else FORMATS[fmt_tg][0], seed)
    if set_name == "extended" and fmt_in == "u8":
        assert {int(o) % 4 for o in data.image_offsets(p.table)} == {0, 1, 2, 3}
    return p


def reference(arrays, op, H, W, wl, n):
    """reference_sample of the record's own image (the reference indexes a dense [N, Hs, Ws, 3] array)."""
    return reference_sample(arrays[int(op[0])][None], [0] + [int(v) for v in op[1:6]], H, W, wl, n)


def run_and_check(dev, p, ops, H, W, n, wl_in, wl_tg, want=(True, True, True), device_tables=True, expect_ops=None,
                  even=False, what=""):
    """prepare_batch_ragged into guarded buffers; every requested output bit-equal to the numpy reference."""
    from hdrnet_amd import data
    ops = np.ascontiguousarray(ops, dtype=np.int32)
    B = ops.shape[0]
    g = [Guarded(s, dev) if w else None for s, w in zip(((B, n, n, 3), (B, H, W, 3), (B, H, W, 3)), want)]
    table, images = torch.from_numpy(ops), p.table
    if device_tables:
        table, images = table.to(dev), images.to(dev)
    res = data.prepare_batch_ragged(p.flat_in, p.flat_tg, images, table, (H, W), n, wl_in, wl_tg,
                                    out=[None if x is None else x.t for x in g], even_turns_only=even)
    torch.cuda.synchronize(dev)
    assert [r is None for r in res] == [x is None for x in g]
    got = [None if x is None else x.result() for x in g]
    ref_ops = ops if expect_ops is None else expect_ops
    for b in range(B):
        full, low = reference(p.arrays_in, ref_ops[b], H, W, wl_in, n)
        tag = f"{what} [{b}] op {list(ref_ops[b][:6])}"
        if got[0] is not None:
            bits_equal(got[0][b], low, "lowres_input " + tag)
        if got[1] is not None:
            bits_equal(got[1][b], full, "image_input " + tag)
        if got[2] is not None:
            bits_equal(got[2][b], reference(p.arrays_tg, ref_ops[b], H, W, wl_tg, n)[0], "image_target " + tag)
    return got


def room(sizes, i, rot, H, W):
    """(room_y, room_x) of an H x W crop in image i after `rot` quarter turns."""
    Hr, Wr = sizes[i][::-1] if rot & 1 else sizes[i]
    return Hr - H, Wr - W


def corner(sizes, i, rot, H, W, c):
    ry, rx = room(sizes, i, rot, H, W)
    return (ry if c & 2 else 0), (rx if c & 1 else 0)


def geometry_table(rng, sizes, H, W):
    """Every image under every flip and turn: image i with geometry k takes corner (i + k) % 5 of its room, a random
    offset where that is 4 -- so every geometry meets all four corners and a random crop, every image too."""
    rows = []
    for i in range(len(sizes)):
        for k, (flr, fud, rot) in enumerate(GEOMETRIES):
            c = (i + k) % 5
            if c < 4:
                cy, cx = corner(sizes, i, rot, H, W, c)
            else:
                ry, rx = room(sizes, i, rot, H, W)
                cy, cx = int(rng.integers(0, ry + 1)), int(rng.integers(0, rx + 1))
            rows.append([i, flr, fud, rot, cy, cx, 0, 0])
    return np.array(rows, dtype=np.int32)


def corner_table(sizes, images, H, W):
    return np.array([[i, flr, fud, rot, *corner(sizes, i, rot, H, W, c), 0, 0]
                     for i in images for (flr, fud, rot) in GEOMETRIES for c in range(4)], dtype=np.int32)


# ---- 1. every geometry x format ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 10])  # 64 pixels: the 16-byte low-res stores; 100: the scalar ones
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("set_name", list(SETS))
def test_all_geometries_over_the_mixed_set(dev, set_name, fmt, n):
    wl = FORMATS[fmt][1]
    p = packed(dev, set_name, fmt, fmt, 31)
    ops = geometry_table(np.random.default_rng(32), p.sizes, H0, W0)
    crop_sized = ops[ops[:, 0] == 3]
    assert p.sizes[3] == (H0, W0) and len(crop_sized) == 16 and not crop_sized[:, 4:6].any()  # room 0
    run_and_check(dev, p, ops, H0, W0, n, wl, wl, what=f"{set_name} {fmt}")
    # CPU tables: validated, copied, the same launch
    run_and_check(dev, p, ops[::7], H0, W0, n, wl, wl, device_tables=False, what=f"{set_name} {fmt} cpu tables")


# ---- 2. the edges of the flat buffer ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("set_name", list(SETS))
def test_corner_crops_of_the_first_and_the_last_image(dev, set_name, fmt):
    wl = FORMATS[fmt][1]
    p = packed(dev, set_name, fmt, fmt, 33)
    ops = corner_table(p.sizes, (0, len(p.sizes) - 1), H0, W0)
    assert ops.shape[0] == 2 * 16 * 4
    run_and_check(dev, p, ops, H0, W0, 10, wl, wl, what=f"edges {set_name} {fmt}")
    run_and_check(dev, p, ops, H0, W0, 8, wl, wl, what=f"edges {set_name} {fmt}")


# ---- 3. neighbour isolation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["u8", "u16", "f32"])
@pytest.mark.parametrize("set_name", list(SETS))
def test_a_sample_holds_nothing_of_a_neighbouring_image(dev, set_name, fmt):
    dtype, wl = FORMATS[fmt]
    sizes = SETS[set_name]
    arrays = [np.full((h, w, 3), i + 1, dtype=dtype) for i, (h, w) in enumerate(sizes)]
    p = Packed(dev, sizes, dtype, None, 0, arrays_in=arrays)
    ops = corner_table(sizes, range(len(sizes)), H0, W0)
    for n in (8, 10):
        low, full, _ = run_and_check(dev, p, ops, H0, W0, n, wl, None, want=(True, True, False), what=f"constants {fmt}")
        for b, op in enumerate(ops):
            value = np.float32(op[0] + 1) if dtype == np.float32 else np.float32(op[0] + 1) / np.float32(wl)
            assert (full[b] == value).all() and (low[b] == value).all(), (b, list(op))


# ---- 4. two dtypes, optional outputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want", [(True, True, True), (False, True, True), (True, False, True), (True, True, False),
                                  (True, False, False), (False, False, True), (False, True, False)])
def test_u16_input_u8_target_and_each_output_is_optional(dev, want):
    p = packed(dev, "extended", "u16_hdrp", "u8", 34)
    ops = geometry_table(np.random.default_rng(35), p.sizes, H0, W0)[::3]
    run_and_check(dev, p, ops, H0, W0, 10, 32767.0, 255.0, want=want, what=f"u16 -> u8 {want}")
    if not want[2]:
        q = Packed(dev, p.sizes, np.uint16, None, 34)
        run_and_check(dev, q, ops, H0, W0, 8, 32767.0, None, want=want, what="no target")


# ---- 5. a set of equal extents is the uniform call ----------------------------------------------------------------------------------
def test_equal_sized_images_give_what_prepare_batch_gives(dev):
    from hdrnet_amd import data
    N, Hs, Ws, H, W, n = 5, 37, 53, 24, 28, 10
    p = Packed(dev, [(Hs, Ws)] * N, np.uint8, np.uint16, 36)
    ops = data.draw_ops(48, N, (Hs, Ws), (H, W), generator=torch.Generator().manual_seed(1))
    assert torch.equal(ops, data.draw_ops(48, N, p.table[:, 2:], (H, W), generator=torch.Generator().manual_seed(1)))
    uniform = data.prepare_batch(to_dev(np.stack(p.arrays_in), dev), to_dev(np.stack(p.arrays_tg), dev), ops.to(dev), (H, W), n)
    ragged = run_and_check(dev, p, ops.numpy(), H, W, n, 255.0, 65535.0, what="equal extents")
    for u, r, name in zip(uniform, ragged, ("lowres_input", "image_input", "image_target")):
        bits_equal(r, u.cpu().numpy(), f"ragged == uniform, {name}")


# ---- 6. out-of-range records -----------------------------------------------------------------------------------------------------------
def test_out_of_range_records_give_the_clamped_sample_of_their_own_source(dev):
    """A DEVICE ops table is not validated: index and crop offsets are clamped -- the offsets to the room of the record's
    OWN image -- turns and flips masked.  (The descriptor table is the library's: it is not corrupted here.)"""
    from hdrnet_amd import data
    p = packed(dev, "extended", "u8", "u16", 37)
    S, N, H, W = p.sizes, len(p.sizes), H0, W0
    big = 2 ** 31 - 1

    def rm(i, rot):
        return room(S, i, rot, H, W)

    bad = np.array([[-3, 0, 0, 0, 2, 3, 0, 0], [99, 0, 0, 0, 2, 3, 5, 5], [big, 1, 1, 1, big, big, 0, 0],
                    [-big - 1, 0, 0, 2, -big - 1, -big - 1, 0, 0], [1, 3, 2, 7, 1000, -5, 0, 0], [4, -1, -2, -1, -7, 1000, 0, 0],
                    [5, 0, 0, 5, 30, 10, 0, 0], [4, 0, 0, 4, 70, 2, -1, -1], [3, 0, 1, 1, 1, 1, 0, 0], [2, 0, 0, 3, 2, 0, 0, 0]],
                   dtype=np.int64)
    good = np.array([[0, 0, 0, 0, 2, 3, 0, 0], [N - 1, 0, 0, 0, 2, 3, 0, 0], [N - 1, 1, 1, 1, *rm(N - 1, 1), 0, 0],
                     [0, 0, 0, 2, 0, 0, 0, 0], [1, 1, 0, 3, rm(1, 3)[0], 0, 0, 0], [4, 1, 0, 3, 0, rm(4, 3)[1], 0, 0],
                     [5, 0, 0, 1, 30, 3, 0, 0], [4, 0, 0, 0, 64, 2, 0, 0], [3, 0, 1, 1, 0, 0, 0, 0], [2, 0, 0, 3, 1, 0, 0, 0]],
                    dtype=np.int64)
    assert rm(5, 1) == (64, 3) and rm(4, 0) == (64, 3) and rm(2, 3) == (1, 1)
    for n in (8, 10):
        run_and_check(dev, p, bad.astype(np.int32), H, W, n, 255.0, 65535.0, expect_ops=good, what="clamped")
    # even_turns_only reads rot90 & 2
    bad = np.array([[0, 0, 0, 1, 5, 5, 0, 0], [1, 1, 0, 3, 5, 5, 0, 0], [4, 0, 1, 7, 500, 500, 0, 0]], dtype=np.int32)
    good = np.array([[0, 0, 0, 0, 5, 5, 0, 0], [1, 1, 0, 2, 5, 5, 0, 0], [4, 0, 1, 2, 64, 3, 0, 0]])
    run_and_check(dev, p, bad, H, W, 8, 255.0, 65535.0, even=True, expect_ops=good, what="even only")
    # CPU tables are validated instead: the record against its own source, the descriptors against the buffer
    ok = torch.tensor([[4, 0, 0, 0, 64, 3, 0, 0]], dtype=torch.int32)
    data.prepare_batch_ragged(p.flat_in, None, p.table, ok, (H, W), 8)
    for rec, text in (([3, 0, 0, 0, 1, 0, 0, 0], "record 0"), ([4, 0, 0, 1, 64, 3, 0, 0], "record 0"), ([N, 0, 0, 0, 0, 0, 0, 0], "source index")):
        with pytest.raises(ValueError, match=text):
            data.prepare_batch_ragged(p.flat_in, None, p.table, torch.tensor([rec], dtype=torch.int32), (H, W), 8)
        with pytest.raises(ValueError, match=text):  # a device descriptor table is read back for the check
            data.prepare_batch_ragged(p.flat_in, None, p.table.to(dev), torch.tensor([rec], dtype=torch.int32), (H, W), 8)
    shifted = p.table.clone()
    shifted[N - 1, 0] += 1
    with pytest.raises(ValueError, match=f"image {N - 1} ends outside the buffer"):
        data.prepare_batch_ragged(p.flat_in, None, shifted, ok, (H, W), 8)
    with pytest.raises(ValueError, match="does not fit image 3"):
        data.prepare_batch_ragged(p.flat_in, None, p.table, ok, (33, 32), 8)
    with pytest.raises(ValueError, match="ops is required"):
        data.prepare_batch_ragged(p.flat_in, None, p.table, None, (H, W), 8)


# ---- 7. capture and replay -------------------------------------------------------------------------------------------------------------
def test_capture_and_replay_with_a_table_that_selects_other_sizes(dev):
    from hdrnet_amd import data
    p = packed(dev, "extended", "u8", "u16", 38)
    S, N, H, W, n, B = p.sizes, len(p.sizes), H0, W0, 10, 4
    gen = torch.Generator().manual_seed(2)
    draws = [data.draw_ops(B, N, S, (H, W), generator=gen, indices=idx) for idx in ([0, 1, 2, 3], [4, 5, 7, 6], [6, 0, 4, 1])]
    images = p.table.to(dev)
    table = draws[0].to(dev)
    outs = [Guarded(s, dev) for s in ((B, n, n, 3), (B, H, W, 3), (B, H, W, 3))]

    def launch():
        data.prepare_batch_ragged(p.flat_in, p.flat_tg, images, table, (H, W), n, out=[o.t for o in outs])

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        launch()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()

    def fill_nan():
        for o in outs:
            o.t.fill_(float("nan"))

    for ops in (draws[0], draws[1], draws[2], draws[1]):
        table.copy_(ops)  # the graph holds the table's address, not its contents
        fill_nan()
        graph.replay()
        torch.cuda.synchronize(dev)
        replayed = [o.result().copy() for o in outs]
        fill_nan()
        launch()
        torch.cuda.synchronize(dev)
        eager = [o.result() for o in outs]
        for r, e, name in zip(replayed, eager, ("lowres_input", "image_input", "image_target")):
            bits_equal(r, e, f"replay == eager, {name}")
        for b, op in enumerate(ops.numpy()):
            full, low = reference(p.arrays_in, op, H, W, 255.0, n)
            bits_equal(replayed[0][b], low, "replay lowres")
            bits_equal(replayed[1][b], full, "replay input")
            bits_equal(replayed[2][b], reference(p.arrays_tg, op, H, W, 65535.0, n)[0], "replay target")


# ---- 8. the dataset class ----------------------------------------------------------------------------------------------------------------
def test_training_step_fed_by_the_ragged_dataset(dev):
    """RaggedDeviceDataset.feed into a GraphedTrainStep (batch 2, crop 64 x 64) and the same module state fed the
    batches prepared by hand with numpy: the inputs are bit-equal, so the losses must be too."""
    from hdrnet_amd import data, metrics, models, optim
    from hdrnet_amd.runtime import GraphedTrainStep
    rng = np.random.default_rng(39)
    sizes = [(70, 90), (64, 64), (100, 66), (66, 128), (81, 77)]
    N, B, H, W, n = len(sizes), 2, 64, 64, 256
    src = [make_sources(rng, np.uint16, (h, w, 3)) for h, w in sizes]
    tgt = [make_sources(rng, np.uint8, (h, w, 3)) for h, w in sizes]
    wl_in, wl_tg = 32767.0, 255.0
    ds = data.DeviceDataset.from_images([to_dev(a, "cpu") for a in src], [to_dev(a, "cpu") for a in tgt], device=dev,
                                        input_white_level=wl_in, target_white_level=wl_tg, output_resolution=(H, W),
                                        net_input_size=n, generator=torch.Generator().manual_seed(4), order="epoch")
    assert isinstance(ds, data.RaggedDeviceDataset) and len(ds) == N and ds.order == "epoch"
    assert ds.sizes.tolist() == [list(s) for s in sizes] and not ds.sizes.is_cuda
    assert ds.images.is_cuda and torch.equal(ds.images.cpu()[:, 2:].long(), ds.sizes) and ds.images.dtype == torch.int32
    assert ds.flat_inputs.dtype == torch.uint16 and ds.flat_targets.dtype == torch.uint8
    assert ds.flat_inputs.numel() == ds.flat_targets.numel() == sum(h * w * 3 for h, w in sizes)
    for name in ("sizes", "images", "flat_inputs", "flat_targets"):
        with pytest.raises(AttributeError):
            setattr(ds, name, None)
    tables = [ds.draw(B) for _ in range(5)]  # 10 samples = two epochs of 5, the first one ending inside a batch
    seq = [int(v) for t in tables for v in t[:, 0]]
    assert sorted(seq[:N]) == list(range(N)) and sorted(seq[N:]) == list(range(N))
    for t in tables:
        data.check_ops(t, N, ds.sizes, (H, W))
    tables = tables[:3]

    def numpy_batch(ops):
        parts = [reference(src, op, H, W, wl_in, n) for op in ops.numpy()]
        tg = [reference(tgt, op, H, W, wl_tg, n)[0] for op in ops.numpy()]
        return [torch.from_numpy(np.stack(x)).to(dev) for x in ([p[1] for p in parts], [p[0] for p in parts], tg)]

    # next_batch allocates when no `out` is given
    low, full, target = ds.next_batch(B, ops=tables[0])
    want = numpy_batch(tables[0])
    assert torch.equal(low, want[0]) and torch.equal(full, want[1]) and torch.equal(target, want[2])

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


def test_order_of_both_dataset_classes(dev):
    from hdrnet_amd import data
    images = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in SIZES]
    seqd = data.DeviceDataset.from_images(images, device=dev, output_resolution=(32, 32), order="sequential", fliplr=False,
                                          flipud=False, rotate=False, random_crop=False)
    t = torch.cat([seqd.draw(4) for _ in range(3)]).numpy()  # the reference's evaluation pipeline, wrapping
    assert t[:, 0].tolist() == [0, 1, 2, 3, 4, 5] * 2 and not t[:, 1:4].any()
    assert [(r[4], r[5]) for r in t[:6]] == [(int((h - 32) / 2), int((w - 32) / 2)) for h, w in SIZES]
    uni = torch.zeros(7, 40, 48, 3, dtype=torch.uint8, device=dev)
    ep = data.DeviceDataset(uni, output_resolution=(32, 32), generator=torch.Generator().manual_seed(1), order="epoch")
    seq = [int(v) for _ in range(7) for v in ep.draw(3)[:, 0]]  # 21 = 3 epochs of 7 in batches of 3
    assert ep.order == "epoch" and all(sorted(seq[7 * k:7 * k + 7]) == list(range(7)) for k in range(3))
    sq = data.DeviceDataset(uni, output_resolution=(32, 32), order="sequential")
    assert [int(v) for _ in range(3) for v in sq.draw(5)[:, 0]] == [0, 1, 2, 3, 4, 5, 6] * 2 + [0]
    # "random" is the default and draws what it drew before there was an order
    a = data.DeviceDataset(uni, output_resolution=(32, 32), generator=torch.Generator().manual_seed(5))
    assert a.order == "random"
    assert torch.equal(a.draw(16), data.draw_ops(16, 7, (40, 48), (32, 32), generator=torch.Generator().manual_seed(5)))
    low, full, target = seqd.next_batch(3)
    assert target is None and tuple(full.shape) == (3, 32, 32, 3) and not full.any() and not low.any()


# ---- 9. frame size -----------------------------------------------------------------------------------------------------------------------
def test_frame_size_all_turns_from_three_orientations(dev):
    sizes = [(1080, 1920), (1200, 1600), (1920, 1080)]
    H = W = 1024
    p = Packed(dev, sizes, np.uint8, np.uint8, 40)
    ops = np.array([[0, 0, 0, 0, 56, 896, 0, 0], [1, 1, 0, 1, room(sizes, 1, 1, H, W)[0], 3, 0, 0],
                    [2, 0, 1, 2, 451, 55, 0, 0], [1, 1, 1, 3, 0, room(sizes, 1, 3, H, W)[1], 0, 0]], dtype=np.int32)
    assert room(sizes, 0, 0, H, W) == (56, 896) and sorted(ops[:, 3]) == [0, 1, 2, 3]
    run_and_check(dev, p, ops, H, W, 256, 255.0, 255.0, what="1024 x 1024 from frames")
