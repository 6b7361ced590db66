"""Sample preparation from a set of images of mixed extents (hdrnet_prepare_batch_ragged, data.pack_images,
draw_ops / check_ops with per-source extents, order= of the dataset classes), the part that needs no GPU: the argument
validation runs before any HIP call, the tables are built on the host.  tests/test_gpu_sample_prep_ragged.py compares
the kernel with the numpy reference of tests/test_sample_prep.py bit for bit."""
import ctypes
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import ROOT  # noqa: E402
from test_sample_prep import reference_full  # noqa: E402

SIZES = [(37, 53), (64, 41), (33, 33), (32, 32), (96, 35), (35, 96)]  # the base set of the GPU suite
# Packed as u8 the base set's images start at bytes = 0, 3, 3, 2, 2, 2 (mod 4): two more images, so that a start = 1 exists
# as well (the sample counts of the base set are = 3 or 0 mod 4 and only two are = 3, so no order of it reaches 1).
EXTENDED = SIZES + [(33, 37), (40, 36)]
NAME = "hdrnet_prepare_batch_ragged"


# ---- C-ABI validation -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    lib.hdrnet_last_error.restype = ctypes.c_char_p
    lib.hdrnet_version.restype = ctypes.c_int
    getattr(lib, NAME).argtypes = _lib.TRAIN_SIGNATURES[NAME][1]
    getattr(lib, NAME).restype = ctypes.c_int
    return lib


P = 0x10000  # a well aligned non-null "pointer": validation fails before anything dereferences it
ORDER = ("src_input", "input_dtype", "input_white_level", "src_target", "target_dtype", "target_white_level", "n_samples",
         "images", "N", "ops", "B", "image_input", "image_target", "H", "W", "lowres_input", "net_input_size", "flags", "stream")


def call(lib, **kw):
    a = dict(src_input=P, input_dtype=1, input_white_level=255.0, src_target=P, target_dtype=1, target_white_level=255.0,
             n_samples=40 * 64 * 3 * 4, images=P, N=4, ops=P, B=2, image_input=P, image_target=P, H=32, W=36, lowres_input=P,
             net_input_size=16, flags=0, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    rc = getattr(lib, NAME)(*[a[k] for k in ORDER])
    return rc, lib.hdrnet_last_error().decode()


BAD = [
    (dict(images=None), "null image table"),
    (dict(ops=None), "null ops"),
    (dict(N=0), "the image table is empty"),
    (dict(N=-3), "the image table is empty"),
    (dict(n_samples=0), "the source buffers are empty"),
    (dict(n_samples=-1), "the source buffers are empty"),
    (dict(input_dtype=3), "unknown dtype"),
    (dict(input_dtype=-1), "unknown dtype"),
    (dict(target_dtype=7), "unknown dtype"),
    (dict(input_white_level=0.0), "white levels must be positive and finite"),
    (dict(input_white_level=-1.0), "white levels must be positive and finite"),
    (dict(target_white_level=0.0), "white levels must be positive and finite"),
    (dict(target_white_level=float("inf")), "white levels must be positive and finite"),
    (dict(input_white_level=float("nan")), "white levels must be positive and finite"),
    (dict(W=34), "W % 4 != 0"),
    (dict(flags=2), "unknown flags"),
    (dict(flags=0x10001), "unknown flags"),
    (dict(image_input=P + 4), "16-B aligned"),
    (dict(image_target=P + 8), "16-B aligned"),
    (dict(lowres_input=P + 8), "16-B aligned"),
    # the rest of hdrnet_prepare_batch's rules
    (dict(src_input=None), "null buffer"),
    (dict(image_input=None, image_target=None, lowres_input=None), "null buffer"),
    (dict(src_target=None), "image_target given without src_target"),
    (dict(H=0), "non-positive extent"),
    (dict(B=-1), "non-positive extent"),
    (dict(net_input_size=0), "non-positive extent"),
    (dict(src_input=P + 2), "4-B aligned"),
    (dict(ops=P + 2), "4-B aligned"),
    (dict(images=P + 4), "image table must be 16-B aligned"),
]


@pytest.mark.parametrize("kw,text", BAD, ids=[f"{i}-{t[:14]}" for i, (_, t) in enumerate(BAD)])
def test_prepare_batch_ragged_validates_before_any_hip_call(lib, kw, text):
    rc, msg = call(lib, **kw)
    assert rc == 1, msg
    assert text in msg and msg.startswith(NAME + ":"), msg


def test_each_refusal_the_issue_lists_has_its_own_message(lib):
    cases = [dict(images=None), dict(ops=None), dict(N=0), dict(n_samples=0), dict(input_dtype=3), dict(input_white_level=0.0),
             dict(W=34), dict(flags=2), dict(image_input=P + 4)]
    texts = []
    for kw in cases:
        rc, msg = call(lib, **kw)
        assert rc == 1
        texts.append(re.sub(r"[-0-9x]+", "#", msg))
    assert len(set(texts)) == len(cases), texts


def test_prepare_batch_ragged_noop_and_flag(lib):
    assert call(lib, B=0) == (0, "")
    assert call(lib, B=0, src_input=None, images=None, ops=None, image_input=None, image_target=None, lowres_input=None) == (0, "")
    # no extents to check a crop against: any crop, with either flag value, gets as far as the alignment checks
    for flags in (0, 1):
        rc, msg = call(lib, H=4000, W=4000, flags=flags, image_input=P + 4)
        assert rc == 1 and "16-B aligned" in msg
    # lowres only: W need not be a multiple of 4
    rc, msg = call(lib, W=34, image_input=None, image_target=None, lowres_input=P + 4)
    assert rc == 1 and "16-B aligned" in msg


def test_header_exports_and_binding_table_agree(lib):
    from hdrnet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/hdrnet_amd_train.h").read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(hdrnet_[a-z0-9_]+)\s*\(", src)))
    assert NAME in declared and sorted(_lib.TRAIN_SIGNATURES) == declared
    for name, (_, args) in _lib.TRAIN_SIGNATURES.items():
        assert hasattr(lib, name), name
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(params.split(",")) == len(args), name
    params = [p.strip() for p in re.search(NAME + r"\s*\(([^)]*)\)", src).group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == list(ORDER)
    assert params[6] == "long long n_samples" and params[7] == "const int* images"
    assert lib.hdrnet_version() >= 270
    main = open(ROOT + "/include/hdrnet_amd.h").read()
    assert re.search(r"\b270\b.*" + NAME, main)


# ---- pack_images ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.uint8, torch.uint16, torch.float32])
def test_pack_images_offsets_are_running_sums_in_samples(dtype):
    from hdrnet_amd import data
    rng = np.random.default_rng(1)
    np_dtype = {torch.uint8: np.uint8, torch.uint16: np.uint16, torch.float32: np.float32}[dtype]
    arrays = [(rng.random((h, w, 3)) * 200).astype(np_dtype) for h, w in SIZES]
    if dtype == torch.uint16:
        images = [torch.from_numpy(a.view(np.int16)).view(torch.uint16) for a in arrays]
    else:
        images = [torch.from_numpy(a) for a in arrays]
    images[1] = images[1].transpose(0, 1).contiguous().transpose(0, 1)  # not contiguous: packed in index order all the same
    flat, table = data.pack_images(images)
    assert flat.dtype == dtype and flat.dim() == 1 and flat.numel() == sum(h * w * 3 for h, w in SIZES)
    assert table.dtype == torch.int32 and tuple(table.shape) == (len(SIZES), 4) and not table.is_cuda
    t = table.numpy().astype(np.int64)
    sums = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in SIZES])[:-1]])
    assert (t[:, 0] == sums).all() and (t[:, 1] == 0).all()
    assert [tuple(r) for r in t[:, 2:]] == SIZES
    _, ext = data.pack_images([torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in EXTENDED])
    assert {int(o) % 4 for o in data.image_offsets(ext)} == {0, 1, 2, 3}  # u8: every byte alignment of an image start
    got = flat.view(torch.int16).numpy().view(np.uint16) if dtype == torch.uint16 else flat.numpy()
    for a, o in zip(arrays, sums):
        assert np.array_equal(got[o:o + a.size].reshape(a.shape), a)
    assert torch.equal(data.image_offsets(table), torch.from_numpy(sums))


def test_pack_images_offsets_past_2_to_the_31_and_32():
    """Descriptors only (nothing this large is allocated): the 64-bit offset splits into two int32 words."""
    from hdrnet_amd import data
    for off in (0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 3, 2 ** 32, 5 * 2 ** 32 + 2 ** 31 + 7):
        lo = off & 0xFFFFFFFF
        row = torch.tensor([[lo - 2 ** 32 if lo >= 2 ** 31 else lo, off >> 32, 8, 8]], dtype=torch.int32)
        assert int(data.image_offsets(row)[0]) == off
    with pytest.raises(ValueError, match="negative offset"):
        data.check_images(torch.tensor([[0, -1, 8, 8]], dtype=torch.int32), 10 ** 12, (4, 4))


def test_pack_images_refuses():
    from hdrnet_amd import data
    ok = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="empty list"):
        data.pack_images([])
    for bad in (torch.zeros(8, 8, dtype=torch.uint8), torch.zeros(8, 8, 4, dtype=torch.uint8),
                torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(0, 8, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"image 1 should be \[H, W, 3\]"):
            data.pack_images([ok, bad])
    with pytest.raises(ValueError, match="mixed dtypes"):
        data.pack_images([ok, torch.zeros(8, 8, 3, dtype=torch.float32)])
    with pytest.raises(TypeError, match="float32, uint8 or uint16"):
        data.pack_images([torch.zeros(8, 8, 3, dtype=torch.int16)])


def test_check_images():
    from hdrnet_amd import data
    _, table = data.pack_images([torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in SIZES])
    n = sum(h * w * 3 for h, w in SIZES)
    data.check_images(table, n, (32, 32))
    with pytest.raises(ValueError, match="image 5 ends outside the buffer"):
        data.check_images(table, n - 1, (32, 32))
    with pytest.raises(ValueError, match=r"does not fit image 3 \(32 x 32\)"):
        data.check_images(table, n, (33, 32))
    _, wide = data.pack_images([torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in ((40, 64), (36, 50))])
    with pytest.raises(ValueError, match="does not fit image 1 turned by 90 degrees"):
        data.check_images(wide, 10 ** 6, (32, 40))  # 36 x 50 holds 32 x 40, 50 x 36 does not
    data.check_images(wide, 10 ** 6, (32, 40), even_turns_only=True)
    bad = table.clone()
    bad[2, 2] = 0
    with pytest.raises(ValueError, match="non-positive extents"):
        data.check_images(bad, n, (32, 32))
    with pytest.raises(ValueError, match="int32"):
        data.check_images(table.long(), n, (32, 32))


# ---- draw_ops / check_ops with per-source extents ------------------------------------------------------------------------------------
def test_draw_ops_per_source_is_reproducible_and_fits_each_record_to_its_own_source():
    from hdrnet_amd import data
    H, W, N = 32, 32, len(SIZES)
    a = data.draw_ops(8192, N, SIZES, (H, W), generator=torch.Generator().manual_seed(5))
    b = data.draw_ops(8192, N, np.array(SIZES), (H, W), generator=torch.Generator().manual_seed(5))
    c = data.draw_ops(8192, N, torch.tensor(SIZES, dtype=torch.int32), (H, W), generator=torch.Generator().manual_seed(6))
    assert a.dtype == torch.int32 and tuple(a.shape) == (8192, 8)
    assert torch.equal(a, b) and not torch.equal(a, c)
    o = a.numpy().astype(np.int64)
    assert set(np.unique(o[:, 0])) == set(range(N)) and set(np.unique(o[:, 3])) == {0, 1, 2, 3} and not o[:, 6:].any()
    sources = [np.zeros((1, h, w, 3), np.uint8) for h, w in SIZES]
    seen = {}
    for k, op in enumerate(o):
        Hs, Ws = SIZES[op[0]]
        Hr, Wr = (Ws, Hs) if op[3] & 1 else (Hs, Ws)
        assert 0 <= op[4] <= Hr - H and 0 <= op[5] <= Wr - W, op
        if k < 512:
            reference_full(sources[op[0]], [0] + list(op[1:]), H, W, 255.0)  # asserts the crop's shape
        seen.setdefault((op[0], op[3] & 1), set()).add((op[4], op[5]))
    assert seen[(3, 0)] == {(0, 0)} and seen[(3, 1)] == {(0, 0)}  # the crop-sized image has no room
    # every offset the room of a source allows turns up, the last one included
    assert {y for y, _ in seen[(4, 0)]} == set(range(96 - 32 + 1)) and {x for _, x in seen[(4, 0)]} == set(range(35 - 32 + 1))
    assert {y for y, _ in seen[(4, 1)]} == set(range(35 - 32 + 1)) and {x for _, x in seen[(4, 1)]} == set(range(96 - 32 + 1))
    data.check_ops(a, N, SIZES, (H, W))
    data.check_ops(a, N, torch.tensor(SIZES), (H, W))


def test_draw_ops_per_source_centre_crop_is_the_reference_expression():
    from hdrnet_amd import data
    H, W = 20, 24
    o = data.draw_ops(512, len(SIZES), SIZES, (H, W), random_crop=False, generator=torch.Generator().manual_seed(3)).numpy()
    assert set(np.unique(o[:, 3])) == {0, 1, 2, 3} and set(np.unique(o[:, 0])) == set(range(len(SIZES)))
    for op in o:
        Hs, Ws = SIZES[op[0]]
        shape = (Ws, Hs) if op[3] & 1 else (Hs, Ws)  # tf.shape(inout) after the rotation
        assert op[4] == int((shape[0] - H) / 2) and op[5] == int((shape[1] - W) / 2)  # data_pipeline.py:154-155


def test_draw_ops_honours_indices():
    from hdrnet_amd import data
    idx = [5, 0, 3, 3, 1, 4, 2]
    a = data.draw_ops(7, len(SIZES), SIZES, (32, 32), generator=torch.Generator().manual_seed(2), indices=idx)
    assert a[:, 0].tolist() == idx
    data.check_ops(a, len(SIZES), SIZES, (32, 32))
    # nothing is drawn for column 0: the other columns are those of a draw that starts at the flips
    g = torch.Generator().manual_seed(2)
    flr = torch.randint(0, 2, (7,), generator=g, dtype=torch.int64)
    assert a[:, 1].tolist() == flr.tolist()
    # with a plain pair too, tensors too
    b = data.draw_ops(3, 4, (40, 48), (32, 32), generator=torch.Generator().manual_seed(2), indices=torch.tensor([3, 3, 0]))
    assert b[:, 0].tolist() == [3, 3, 0]
    with pytest.raises(ValueError, match="2 indices for a batch of 3"):
        data.draw_ops(3, 4, (40, 48), (32, 32), indices=[0, 1])
    with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
        data.draw_ops(3, 4, (40, 48), (32, 32), indices=[0, 1, 4])


def test_draw_ops_names_the_offending_source():
    from hdrnet_amd import data
    with pytest.raises(ValueError, match=r"does not fit source 3 \(32 x 32\)"):
        data.draw_ops(4, len(SIZES), SIZES, (33, 32))
    with pytest.raises(ValueError, match=r"does not fit source 2 \(33 x 33\)"):
        data.draw_ops(4, len(SIZES), SIZES, (34, 32), rotate=False)
    sizes = [(40, 64), (64, 40), (36, 50), (64, 64)]
    with pytest.raises(ValueError, match=r"does not fit source 2 turned by 90 degrees \(50 x 36\)"):
        data.draw_ops(4, 4, sizes, (32, 40))  # 36 x 50 holds 32 x 40; turned, 50 x 36 does not
    for rotate in ("even", False):
        t = data.draw_ops(64, 4, sizes, (32, 40), rotate=rotate, generator=torch.Generator().manual_seed(1))
        data.check_ops(t, 4, sizes, (32, 40), even_turns_only=True)
    with pytest.raises(ValueError, match="lists 4 sources, n_sources is 5"):
        data.draw_ops(4, 5, sizes, (32, 32))
    with pytest.raises(ValueError, match="integer"):
        data.draw_ops(4, 4, np.array(sizes, dtype=np.float32), (32, 32))
    # check_ops: the record's own source
    t = data.draw_ops(6, len(SIZES), SIZES, (32, 32), rotate=False, fliplr=False, flipud=False, random_crop=False,
                      indices=range(6))
    data.check_ops(t, len(SIZES), SIZES, (32, 32))
    bad = t.clone()
    bad[3, 4] = 1  # image 3 is crop-sized
    with pytest.raises(ValueError, match=r"record 3: .* 32 x 32 source 3"):
        data.check_ops(bad, len(SIZES), SIZES, (32, 32))
    bad = t.clone()
    bad[4, 3], bad[4, 4] = 1, 4  # image 4 is 96 x 35: turned, crop_y has room 3
    with pytest.raises(ValueError, match="record 4"):
        data.check_ops(bad, len(SIZES), SIZES, (32, 32))
    bad[4, 4], bad[4, 5] = 3, 64
    data.check_ops(bad, len(SIZES), SIZES, (32, 32))
    bad = t.clone()
    bad[0, 0] = 6
    with pytest.raises(ValueError, match="source index"):
        data.check_ops(bad, len(SIZES), SIZES, (32, 32))


def documented_draw(batch, n_sources, Hs, Ws, H, W, fliplr, flipud, mode, random_crop, g):
    """The draw order hdrnet_amd/data.py documents and the parent commit implements, restated: one int64 randint vector
    per enabled column (index, flip_lr, flip_ud, turns), then two float64 rand vectors scaled to the record's room."""
    def rnd(high):
        return torch.randint(0, high, (batch,), generator=g, dtype=torch.int64).numpy()
    o = np.zeros((batch, 8), np.int64)
    o[:, 0] = rnd(n_sources)
    if fliplr:
        o[:, 1] = rnd(2)
    if flipud:
        o[:, 2] = rnd(2)
    if mode == "all":
        o[:, 3] = rnd(4)
    elif mode == "even":
        o[:, 3] = 2 * rnd(2)
    odd = (o[:, 3] & 1).astype(bool)
    room_y, room_x = np.where(odd, Ws - H, Hs - H), np.where(odd, Hs - W, Ws - W)
    if random_crop:
        uy = torch.rand((batch,), generator=g, dtype=torch.float64).numpy()
        ux = torch.rand((batch,), generator=g, dtype=torch.float64).numpy()
        o[:, 4] = np.minimum(np.floor(uy * (room_y + 1)).astype(np.int64), room_y)
        o[:, 5] = np.minimum(np.floor(ux * (room_x + 1)).astype(np.int64), room_x)
    else:
        o[:, 4], o[:, 5] = room_y // 2, room_x // 2
    return o.astype(np.int32)


@pytest.mark.parametrize("fliplr,flipud,rotate,random_crop", [(True, True, True, True), (False, True, "even", True),
                                                              (True, False, False, False), (False, False, True, False)])
def test_draw_ops_of_a_pair_consumes_the_generator_as_before(fliplr, flipud, rotate, random_crop):
    from hdrnet_amd import data
    Hs, Ws, H, W, N, B = 48, 40, 32, 36, 7, 65
    mode = "even" if rotate == "even" else ("all" if rotate else "none")
    g1, g2 = torch.Generator().manual_seed(9), torch.Generator().manual_seed(9)
    for _ in range(2):  # the second table starts where the first draw left the generator
        got = data.draw_ops(B, N, (Hs, Ws), (H, W), fliplr, flipud, rotate, random_crop, g1)
        want = documented_draw(B, N, Hs, Ws, H, W, fliplr, flipud, mode, random_crop, g2)
        assert np.array_equal(got.numpy(), want)
    assert torch.equal(g1.get_state(), g2.get_state())
    # a table of equal extents draws what the pair draws
    g3 = torch.Generator().manual_seed(9)
    same = data.draw_ops(B, N, [(Hs, Ws)] * N, (H, W), fliplr, flipud, rotate, random_crop, g3)
    assert np.array_equal(same.numpy(), documented_draw(B, N, Hs, Ws, H, W, fliplr, flipud, mode, random_crop,
                                                         torch.Generator().manual_seed(9)))


# ---- order= -----------------------------------------------------------------------------------------------------------------------------
def test_order_epoch_visits_every_index_once_per_epoch():
    from hdrnet_amd import data
    N, batch = 10, 4  # 4 does not divide 10: an epoch ends inside a batch
    walk = data._Walk("epoch", N, torch.Generator().manual_seed(1))
    seq = []
    while len(seq) < 3 * N:
        got = walk.take(batch)
        assert len(got) == batch
        seq += got
    epochs = [seq[k * N:(k + 1) * N] for k in range(3)]
    for e in epochs:
        assert sorted(e) == list(range(N))
    assert np.bincount(seq[:3 * N], minlength=N).tolist() == [3] * N
    assert epochs[0] != epochs[1] and epochs[0] != list(range(N))  # shuffled, and anew per epoch
    again = data._Walk("epoch", N, torch.Generator().manual_seed(1))
    assert [again.take(batch) for _ in range(3)] == [seq[0:4], seq[4:8], seq[8:12]]
    # through draw_ops: the walk's indices are column 0
    walk = data._Walk("epoch", len(SIZES), torch.Generator().manual_seed(2))
    col = []
    for _ in range(9):  # 9 batches of 4 = 6 epochs of 6
        col += data.draw_ops(4, len(SIZES), SIZES, (32, 32), generator=walk.generator, indices=walk.take(4))[:, 0].tolist()
    for k in range(6):
        assert sorted(col[6 * k:6 * k + 6]) == list(range(6))


def test_order_sequential_wraps_and_random_leaves_the_draw_alone():
    from hdrnet_amd import data
    walk = data._Walk("sequential", 5, None)
    assert walk.take(3) == [0, 1, 2] and walk.take(4) == [3, 4, 0, 1] and walk.take(7) == [2, 3, 4, 0, 1, 2, 3]
    assert walk.take(0) == []
    assert data._Walk("random", 5, None).take(3) is None
    with pytest.raises(ValueError, match="order should be one of"):
        data._Walk("shuffled", 5, None)
    # the reference's evaluation pipeline: in order, centre crop, no flips or turns
    t = data.draw_ops(6, len(SIZES), SIZES, (32, 32), fliplr=False, flipud=False, rotate=False, random_crop=False,
                      indices=data._Walk("sequential", len(SIZES), None).take(6)).numpy()
    assert t[:, 0].tolist() == list(range(6)) and not t[:, 1:4].any()
    assert [(r[4], r[5]) for r in t] == [(int((h - 32) / 2), int((w - 32) / 2)) for h, w in SIZES]


def test_python_entry_points_exist_and_refuse_cpu_tensors():
    import hdrnet_amd
    from hdrnet_amd import data
    assert hdrnet_amd.prepare_batch_ragged is data.prepare_batch_ragged and hdrnet_amd.pack_images is data.pack_images
    assert hdrnet_amd.RaggedDeviceDataset is data.RaggedDeviceDataset
    images = [torch.zeros(h, w, 3, dtype=torch.uint8) for h, w in SIZES]
    flat, table = data.pack_images(images)
    ops = data.draw_ops(2, len(SIZES), table[:, 2:], (32, 32))
    with pytest.raises(RuntimeError, match="device only"):
        data.prepare_batch_ragged(flat, None, table, ops, (32, 32), 8)
    with pytest.raises(RuntimeError, match="device only"):
        data.DeviceDataset.from_images(images, output_resolution=(32, 32), device="cpu")
    with pytest.raises(ValueError, match=r"does not fit source 3 \(32 x 32\)"):
        data.DeviceDataset.from_images(images, output_resolution=(33, 32), device="cuda")
    with pytest.raises(ValueError, match="pair 1"):
        data.DeviceDataset.from_images(images, [images[0], images[0]] + images[2:], output_resolution=(32, 32), device="cuda")
    with pytest.raises(ValueError, match="order should be one of"):
        data.DeviceDataset.from_images(images, output_resolution=(32, 32), device="cuda", order="bogus")
