"""tests/wire_geometry_cases.py is what its comments say (no GPU): the row plans, that every geometry fits the wire-format
kernel and the refused one does not, which rows reach the vertical clamp and which chroma pairs share their grid rows,
what the layouts promise -- and that the contents chosen for the surface-output tests stay within those tests' caps on
undecided samples, with the CPU oracle's float32 output in place of the kernel's."""
import os

import numpy as np
import pytest

import oracle
import wire_geometry_cases as wg
import yuv_cases as yc
from row_plan import io_fits, row_plan


def test_the_row_plans():
    assert row_plan(2052) == (192, 3, 684)    # the narrowest row with an interior segment ...
    assert row_plan(2048)[1] == 2             # ... one lane group narrower has two
    assert row_plan(3840) == (192, 5, 768)
    assert row_plan(8196) == (192, 11, 748) and row_plan(8196)[1] > 8   # past the host's column table
    assert row_plan(260) == (128, 1, 260) and 260 // 4 == 65            # 65 of 128 lanes active
    assert row_plan(96) == (64, 1, 96)
    for shape, _ in wg.GEOMETRIES.values():
        assert shape[0] * shape[1] * shape[2] < 100_000 and shape[1] % 2 == 0 and shape[2] % 4 == 0


def test_every_geometry_fits_and_the_refused_one_does_not():
    for geo, ((B, H, W), (GH, GW, GD)) in wg.GEOMETRIES.items():
        assert io_fits(W, GW, GD), geo
    (B, H, W), (GH, GW, GD) = wg.REFUSED
    assert not io_fits(W, GW, GD) and H % 2 == 0 and W % 4 == 0   # refused for its LDS image, nothing else


def test_the_vertical_regime():
    clamps = {geo: wg.clamped_rows(shape[1], grid[0]) for geo, (shape, grid) in wg.GEOMETRIES.items()}
    assert clamps["interior"] == ([0], [39])
    assert clamps["uhd_row"] == ([0], [11])
    assert clamps["many_seg"] == ([0], [3])
    assert clamps["one_cell"] == ([0, 1, 2], [3, 4, 5])   # every row: one grid row
    assert clamps["tall"] == ([0], [65])
    gy = wg.gy_of_rows(40, 16)
    assert np.isclose(gy[0], -0.3) and np.isclose(gy[39], 15.3)
    shared = wg.pair_floors(40, 16)
    assert len(shared) == 20 and any(shared) and not all(shared)
    assert shared[1] and shared[2] and not shared[4]   # rows (2, 3), (4, 5) inside a grid row; rows (8, 9) straddle
    # the existing tests' H = 6 on GH = 16: no clamp, no pair inside a grid row
    assert wg.clamped_rows(6, 16) == ([], []) and not any(wg.pair_floors(6, 16))


@pytest.mark.parametrize("size", [1, 2])
def test_the_surface_layouts(size):
    for geo, layouts in wg.SURFACE_LAYOUTS.items():
        shape = wg.GEOMETRIES[geo][0]
        B, H, W = shape
        assert ("one_allocation" in layouts) == (B >= 2), geo
        for layout in layouts:
            lengths, sy, suv = wg.surface_layout(shape, size, layout)
            dt = np.uint8 if size == 1 else np.uint16
            rng = np.random.default_rng(3)
            y, uv = yc.random_surface(rng, shape, 8 * size)
            bufs, sy, suv = wg.lay_surface(y, uv, layout)
            assert np.array_equal(wg.plane(bufs, sy), y) and np.array_equal(wg.plane(bufs, suv), uv)
            outside = wg.outside_planes(bufs, (sy, suv))
            assert sum(int((~m).sum()) for m in outside) == y.size + uv.size   # the planes do not overlap
            for b, m in zip(bufs, outside):
                assert (b[m] == wg.fill_value(dt, yc.POISON)).all()
                assert m[-wg.GUARD_BYTES // size:].all()                      # a guard behind every buffer
            for spec in (sy, suv):
                assert spec[3][2] == 1 and (spec[3][1] * size) % 4 == 0 and (spec[3][0] * size) % 4 == 0
            if layout == "one_allocation":
                pitch = sy[3][1]
                assert sy[0] == suv[0] and sy[3][0] == suv[3][0] == pitch * (3 * H // 2 + 2) > pitch * H
                assert suv[1] == H * pitch and pitch * size == W * size + 64
            if layout == "pitch64":
                assert sy[3][1] * size == W * size + 64 and sy[3][0] == H * sy[3][1]
            if layout == "off4":
                assert sy[1] * size == 4 and suv[1] * size == 4   # buffers are at least 16-byte aligned: 4 past 8


def test_the_packed_layouts():
    frame = np.arange(2 * 3 * 4 * 3, dtype=np.uint16).reshape(2, 3, 4, 3)
    buf, off = wg.lay_packed(frame, "off4")
    assert off * 2 == 4 and np.array_equal(buf[off:off + frame.size].reshape(frame.shape), frame)
    assert (buf[:off] == 0xA5A5).all() and (buf[off + frame.size:] == 0xA5A5).all()
    with pytest.raises(AssertionError):
        wg.lay_packed(np.zeros((1, 2, 4, 4), np.uint8), "off4")   # RGBA / BGRA stay 16-byte aligned


# ---- the surface-output contents against the caps, before any GPU run -------------------------------------------------------
def oracle_guide(c, guide, x):
    if guide == "map":
        return c["guide"]
    if guide == "nn":
        return oracle.pointwise_nn_guide(x, c["conv1"], c["conv2"])
    return oracle.curves_guide(x, *wg.curves_of(c, guide))


@pytest.fixture(scope="module")
def port16(port):
    port.set_threads(min(16, os.cpu_count() or 1))
    yield port
    port.set_threads(1)


@pytest.mark.parametrize("geo", wg.GEOMETRY_IDS)
def test_surface_output_contents_stay_within_the_caps(port16, geo):
    """Per (pair, guide form): the share of samples the float64 encoder leaves undecided, computed from the CPU oracle's
    float32 output -- under 1 % at 8 bits, under 2 % at 10, at least 40 % decided at 16.  A content that did not would get
    another seed (wire_geometry_cases.surface_case), never another cap."""
    from hdrnet_amd import yuv
    rgb = {}
    for pair, (bits, standard, full, out_bits) in wg.SURFACE_OUT.items():
        c = wg.surface_case(geo, bits)
        to_rgb = yuv.yuv_coefficients(standard, full, bits)[0]
        from_rgb = yuv.yuv_encode_coefficients(standard, full, out_bits)
        x = yc.to_rgb64(c["y"], c["uv"], to_rgb).astype(np.float32)
        for guide in ("map", "nn", "curves", "scan"):   # "cells" is the curves guide through other tables
            if (bits, guide) not in rgb:
                rgb[bits, guide] = port16.bilateral_slice_apply(c["grid"], oracle_guide(c, guide, x), x, True)
            _, _, dy, duv, _ = wg.encode64(rgb[bits, guide], from_rgb, out_bits)
            undecided, total = int((~dy).sum() + (~duv).sum()), dy.size + duv.size
            print(f"{geo} {pair} {guide}: {undecided} of {total} undecided ({100.0 * undecided / total:.2f} %)")
            assert wg.within_cap(out_bits, undecided, total), (geo, pair, guide, undecided, total)
