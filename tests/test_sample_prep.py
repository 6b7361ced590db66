"""Sample preparation (csrc/sample_prep.hip, hdrnet_amd/data.py), the part that needs no GPU: the argument validation of
hdrnet_prepare_batch / hdrnet_lowres_input (it runs before any HIP call), draw_ops, and this file's own numpy
reference -- the four lines of hdrnet/data_pipeline.py's `_augment_data` -- against the integer index map the kernel
uses.  tests/test_gpu_sample_prep.py compares the kernel with `reference_sample` bit for bit."""
import ctypes
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")


# ---- the numpy reference (imports nothing from the product or from oracle/) -----------------------------------------------
def reference_full(source, op, H, W, white_level):
    """s = source[index]; flips; rot90; crop; / white_level -- fp32, IEEE division (float sources are copied)."""
    index, flr, fud, rot, cy, cx = (int(v) for v in op[:6])
    s = source[index]
    if flr:
        s = s[:, ::-1]
    if fud:
        s = s[::-1]
    s = np.rot90(s, rot)  # counter-clockwise in the (row, col) plane, as tf.image.rot90
    s = s[cy:cy + H, cx:cx + W]
    assert s.shape[:2] == (H, W), (s.shape, H, W)
    if source.dtype == np.float32:
        return np.ascontiguousarray(s)
    return s.astype(np.float32) / np.float32(white_level)


def reference_lowres(full, n):
    """TF1 ResizeNearestNeighbor(align_corners=False) = cv::INTER_NEAREST: fp32 scale, fp32 product, floor, clamp."""
    H, W = full.shape[:2]
    sy, sx = np.float32(H) / np.float32(n), np.float32(W) / np.float32(n)
    ys = np.minimum(np.floor(np.arange(n, dtype=np.float32) * sy).astype(np.int64), H - 1)
    xs = np.minimum(np.floor(np.arange(n, dtype=np.float32) * sx).astype(np.int64), W - 1)
    return np.ascontiguousarray(full[ys][:, xs])


def reference_sample(source, op, H, W, white_level, n):
    full = reference_full(source, op, H, W, white_level)
    return full, reference_lowres(full, n)


def index_table(Hs, Ws, flr, fud, rot, Y, X):
    """The issue's table: output pixel (Y, X) of the turned, flipped image -> source (row, col)."""
    row, col = [(Y, X), (X, Ws - 1 - Y), (Hs - 1 - Y, Ws - 1 - X), (Hs - 1 - X, Y)][rot]
    if fud:
        row = Hs - 1 - row
    if flr:
        col = Ws - 1 - col
    return row, col


@pytest.mark.parametrize("flr,fud,rot", list(itertools.product((0, 1), (0, 1), (0, 1, 2, 3))))
def test_reference_matches_the_index_table(flr, fud, rot):
    Hs, Ws = 7, 11
    src = np.arange(Hs * Ws * 3, dtype=np.float32).reshape(1, Hs, Ws, 3)
    Hr, Wr = (Ws, Hs) if rot & 1 else (Hs, Ws)
    full = reference_full(src, (0, flr, fud, rot, 0, 0), Hr, Wr, 1.0)
    for Y in range(Hr):
        for X in range(Wr):
            r, c = index_table(Hs, Ws, flr, fud, rot, Y, X)
            assert np.array_equal(full[Y, X], src[0, r, c]), (Y, X)
    # a crop is an offset into that image
    H, W, cy, cx = 3, 4, 2, 1
    crop = reference_full(src, (0, flr, fud, rot, cy, cx), H, W, 1.0)
    assert np.array_equal(crop, full[cy:cy + H, cx:cx + W])


def test_reference_lowres_is_the_tf1_rule():
    full = np.arange(5 * 7 * 3, dtype=np.float32).reshape(5, 7, 3)
    low = reference_lowres(full, 4)
    # rows floor(y * 1.25) = 0 1 2 3, columns floor(x * 1.75) = 0 1 3 5
    assert np.array_equal(low, full[[0, 1, 2, 3]][:, [0, 1, 3, 5]])
    up = reference_lowres(full, 9)  # upsampling clamps nothing here: floor(8 * 5 / 9) = 4
    assert up.shape == (9, 9, 3) and np.array_equal(up[8, 8], full[4, 6])
    assert np.array_equal(reference_full(np.full((1, 2, 4, 3), 200, np.uint8), (0, 0, 0, 0, 0, 0), 2, 4, 255.0),
                          np.full((2, 4, 3), np.float32(200) / np.float32(255)))


# ---- C-ABI validation -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    lib.hdrnet_last_error.restype = ctypes.c_char_p
    lib.hdrnet_prepare_batch.argtypes = _lib.TRAIN_SIGNATURES["hdrnet_prepare_batch"][1]
    lib.hdrnet_lowres_input.argtypes = _lib.SIGNATURES["hdrnet_lowres_input"][1]
    return lib


P = 0x10000  # a well aligned non-null "pointer": validation fails before anything dereferences it


def call(lib, **kw):
    a = dict(src_input=P, input_dtype=1, input_white_level=255.0, src_target=P, target_dtype=1, target_white_level=255.0,
             N=4, Hs=40, Ws=64, ops=P, B=2, image_input=P, image_target=P, H=32, W=36, lowres_input=P, net_input_size=16,
             flags=0, stream=None)
    a.update(kw)
    rc = lib.hdrnet_prepare_batch(a["src_input"], a["input_dtype"], a["input_white_level"], a["src_target"],
                                  a["target_dtype"], a["target_white_level"], a["N"], a["Hs"], a["Ws"], a["ops"], a["B"],
                                  a["image_input"], a["image_target"], a["H"], a["W"], a["lowres_input"],
                                  a["net_input_size"], a["flags"], a["stream"])
    return rc, lib.hdrnet_last_error().decode()


BAD = [
    (dict(src_input=None), "null buffer"),
    (dict(image_input=None, image_target=None, lowres_input=None), "null buffer"),
    (dict(src_target=None), "image_target given without src_target"),
    (dict(input_dtype=3), "unknown dtype"),
    (dict(input_dtype=-1), "unknown dtype"),
    (dict(target_dtype=7), "unknown dtype"),
    (dict(input_white_level=0.0), "white levels must be positive and finite"),
    (dict(input_white_level=-1.0), "white levels must be positive and finite"),
    (dict(target_white_level=float("inf")), "white levels must be positive and finite"),
    (dict(input_white_level=float("nan")), "white levels must be positive and finite"),
    (dict(N=0), "non-positive extent"),
    (dict(H=0), "non-positive extent"),
    (dict(W=-4), "non-positive extent"),
    (dict(Hs=0), "non-positive extent"),
    (dict(B=-1), "non-positive extent"),
    (dict(net_input_size=0), "non-positive extent"),
    (dict(H=41), "does not fit the 40 x 64 source"),
    (dict(W=68), "does not fit the 40 x 64 source"),
    (dict(W=44), "turned by 90 degrees"),           # W > Hs: an odd turn would not fit
    (dict(Hs=80, Ws=36, H=40, W=36), "turned by 90 degrees"),  # H > Ws
    (dict(ops=None), "ops == NULL"),                # (H, W) != (Hs, Ws)
    (dict(ops=None, H=40, W=64, B=5), "ops == NULL"),  # B > N
    (dict(W=34), "W % 4 != 0"),
    (dict(image_input=P + 4), "16-B aligned"),
    (dict(lowres_input=P + 8), "16-B aligned"),
    (dict(src_input=P + 2), "4-B aligned"),
    (dict(src_target=P + 1), "4-B aligned"),
    (dict(flags=2), "unknown flags"),
    (dict(flags=0x10001), "unknown flags"),
]


@pytest.mark.parametrize("kw,text", BAD, ids=[f"{i}-{t[:14]}" for i, (_, t) in enumerate(BAD)])
def test_prepare_batch_validates_before_any_hip_call(lib, kw, text):
    rc, msg = call(lib, **kw)
    assert rc == 1, msg
    assert text in msg and msg.startswith("hdrnet_prepare_batch"), msg


def test_prepare_batch_noop_and_flag(lib):
    assert call(lib, B=0) == (0, "")
    assert call(lib, B=0, src_input=None, image_input=None, image_target=None, lowres_input=None) == (0, "")
    # the flag lifts the odd-turn rule only: the message of the NEXT check shows the call got past it
    rc, msg = call(lib, W=44, flags=1, image_input=P + 4)
    assert rc == 1 and "16-B aligned" in msg
    rc, msg = call(lib, W=68, flags=1)
    assert rc == 1 and "does not fit the 40 x 64 source" in msg


def test_lowres_input_validates_before_any_hip_call(lib):
    def low(frames=P, dtype=1, wl=255.0, B=1, H=30, W=50, lowres=P, n=16):
        rc = lib.hdrnet_lowres_input(frames, dtype, wl, B, H, W, lowres, n, None)
        return rc, lib.hdrnet_last_error().decode()

    for kw, text in ((dict(frames=None), "null buffer"), (dict(lowres=None), "null buffer"), (dict(dtype=4), "unknown dtype"),
                     (dict(wl=0.0), "white levels"), (dict(H=0), "non-positive extent"), (dict(n=-1), "non-positive extent"),
                     (dict(lowres=P + 4), "16-B aligned"), (dict(frames=P + 1), "4-B aligned"), (dict(B=-1), "non-positive extent")):
        rc, msg = low(**kw)
        assert rc == 1 and text in msg and msg.startswith("hdrnet_lowres_input"), (kw, msg)
    assert low(B=0) == (0, "")
    assert low(B=0, lowres=None, frames=None) == (0, "")


# ---- draw_ops -----------------------------------------------------------------------------------------------------------------------
def test_draw_ops_is_reproducible_in_range_and_fits():
    from hdrnet_amd import data
    Hs, Ws, H, W = 48, 40, 32, 36
    a = data.draw_ops(512, 7, (Hs, Ws), (H, W), generator=torch.Generator().manual_seed(5))
    b = data.draw_ops(512, 7, (Hs, Ws), (H, W), generator=torch.Generator().manual_seed(5))
    c = data.draw_ops(512, 7, (Hs, Ws), (H, W), generator=torch.Generator().manual_seed(6))
    assert a.dtype == torch.int32 and tuple(a.shape) == (512, 8) and not a.is_cuda
    assert torch.equal(a, b) and not torch.equal(a, c)
    o = a.numpy().astype(np.int64)
    assert o[:, 0].min() == 0 and o[:, 0].max() == 6
    assert set(np.unique(o[:, 1])) == {0, 1} and set(np.unique(o[:, 2])) == {0, 1} and set(np.unique(o[:, 3])) == {0, 1, 2, 3}
    assert not o[:, 6:].any()
    src = np.zeros((7, Hs, Ws, 3), np.uint8)
    for op in o:
        odd = op[3] & 1
        Hr, Wr = (Ws, Hs) if odd else (Hs, Ws)
        assert 0 <= op[4] <= Hr - H and 0 <= op[5] <= Wr - W
        reference_full(src, op, H, W, 255.0)  # asserts the crop's shape
    # every offset the room allows turns up, the last one included
    even = o[(o[:, 3] & 1) == 0]
    assert set(np.unique(even[:, 4])) == set(range(Hs - H + 1)) and set(np.unique(even[:, 5])) == set(range(Ws - W + 1))
    data.check_ops(a, 7, (Hs, Ws), (H, W))
    # switches
    off = data.draw_ops(64, 3, (Hs, Ws), (H, W), fliplr=False, flipud=False, rotate=False,
                        generator=torch.Generator().manual_seed(1)).numpy()
    assert not off[:, 1:4].any()
    ev = data.draw_ops(256, 3, (Hs, Ws), (H, W), rotate="even", generator=torch.Generator().manual_seed(1)).numpy()
    assert set(np.unique(ev[:, 3])) == {0, 2}


def test_draw_ops_centre_crop_is_the_reference_expression():
    from hdrnet_amd import data
    Hs, Ws, H, W = 37, 53, 20, 24
    o = data.draw_ops(256, 2, (Hs, Ws), (H, W), random_crop=False, generator=torch.Generator().manual_seed(3)).numpy()
    assert set(np.unique(o[:, 3])) == {0, 1, 2, 3}
    for op in o:
        shape = (Ws, Hs) if op[3] & 1 else (Hs, Ws)  # tf.shape(inout) after the rotation
        assert op[4] == int((shape[0] - H) / 2) and op[5] == int((shape[1] - W) / 2)  # data_pipeline.py:154-155


def test_draw_ops_refuses_what_cannot_fit():
    from hdrnet_amd import data
    with pytest.raises(ValueError, match="does not fit the 30 x 50 source"):
        data.draw_ops(4, 2, (30, 50), (32, 40))
    with pytest.raises(ValueError, match="turned by 90 degrees"):
        data.draw_ops(4, 2, (30, 50), (24, 40))  # W = 40 > Hs = 30
    data.draw_ops(4, 2, (30, 50), (24, 40), rotate="even")
    data.draw_ops(4, 2, (30, 50), (24, 40), rotate=False)
    t = data.draw_ops(4, 2, (30, 50), (24, 28), generator=torch.Generator().manual_seed(0))
    bad = t.clone()
    bad[1, 0] = 2
    with pytest.raises(ValueError, match="source index"):
        data.check_ops(bad, 2, (30, 50), (24, 28))
    bad = t.clone()
    bad[2, 3], bad[2, 4] = 0, 7
    with pytest.raises(ValueError, match="does not fit"):
        data.check_ops(bad, 2, (30, 50), (24, 28))
    bad = t.clone()
    bad[0, 3] = 1
    with pytest.raises(ValueError, match="even_turns_only"):
        data.check_ops(bad, 2, (30, 50), (24, 28), even_turns_only=True)


def test_python_entry_points_refuse_cpu_tensors():
    import hdrnet_amd
    from hdrnet_amd import data
    assert hdrnet_amd.prepare_batch is data.prepare_batch and hdrnet_amd.lowres_input is data.lowres_input
    assert hdrnet_amd.draw_ops is data.draw_ops and hdrnet_amd.DeviceDataset is data.DeviceDataset
    with pytest.raises(RuntimeError, match="device only"):
        data.lowres_input(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(TypeError):
        data.lowres_input(torch.zeros(1, 8, 8, 3, dtype=torch.int16))
    with pytest.raises(ValueError):
        data.lowres_input(torch.zeros(8, 8, 3, dtype=torch.uint8))
