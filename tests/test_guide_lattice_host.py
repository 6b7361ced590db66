"""The guide lattice on the CPU (tests/guide_lattice_cases.py): that the frames tests/test_gpu_guide_lattice.py runs hold
what they promise, that the two C oracles agree bit for bit on them, and a closed form that uses neither oracle."""
import numpy as np
import pytest

from guide_lattice_cases import (CHUNK, DEPTHS, EDGE_LANES, FALLBACK, LAYOUT_FRAMES, LOWER, MANY_TASKS, ODD, TIERS, UPPER,
                                 gz_product, guide_frame, lattice, plant_plan, problem_arrays, taps)

LAYOUTS = [("rows", LOWER), ("mixed", LOWER), ("planted", LOWER), ("planted", UPPER)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- 1. coverage ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("GD", DEPTHS)
def test_lattice_holds_its_tiers(GD):
    L, T = lattice(GD)
    assert len(set(bits(L).tolist())) == len(L)
    gz = np.abs(gz_product(L, GD).astype(np.float64))
    assert (gz[T <= 2] < 2.0 ** 22).all() and ((gz[T == 3] >= 2.0 ** 22) & (gz[T == 3] <= 2.0 ** 30)).all()
    for t in TIERS:
        assert (T == t).any(), t
    have = set(bits(L).tolist())
    for v in (0.0, -0.0, 1.0, 1e-45, -1e-45, 1.1754944e-38, -1.1754944e-38, 2.0, -2.0, 37.5, -1e3, 2.0 ** 22 / GD):
        assert int(bits(np.float32(v))[0]) in have, v
    # every tap switch and every cell border is there AS A PRODUCT: some value's float32 guide * GD is exactly k + 0.5 / k
    prod = set(gz_product(L, GD).tolist())
    for k in range(-1, GD + 1):
        assert k + 0.5 in prod and float(k) in prod, k
    # ... and both sides of it: floor(gz - 0.5) takes k - 1 and k among the values within 64 ulps of the switch
    gz1 = gz_product(L[T == 1], GD)
    fz = np.floor(gz1 - np.float32(0.5))
    assert set(range(-2, GD + 1)) <= set(fz.astype(int).tolist())
    # ... and the ulp below a switch where gz - 0.5f rounds UP onto the integer: floor() lands one plane high and the lower
    # tap's offset (gz0 + 0.5f) - gz is POSITIVE -- the reference's arithmetic, which a closed form taking dz0 <= 0 misses
    dz0 = (fz + np.float32(0.5)) - gz1
    assert (dz0 > 0).any() and dz0.max() <= 2e-6 * max(GD, 1)


@pytest.mark.parametrize("GD", DEPTHS)
@pytest.mark.parametrize("layout,background", LAYOUTS)
def test_every_lattice_value_occurs_in_every_layout(GD, layout, background):
    L, T = lattice(GD)
    g, t = guide_frame(GD, layout, LAYOUT_FRAMES[layout][:3], background)
    assert set(bits(L).tolist()) <= set(bits(g).ravel().tolist())
    for tier in TIERS:   # the tier map marks exactly the lattice values of the tier
        assert set(bits(g[t == tier]).ravel().tolist()) == set(bits(L[T == tier]).tolist())
    gc, tc = g.reshape(-1, CHUNK), t.reshape(-1, CHUNK)
    if layout == "rows":      # every chunk is uniform
        assert (bits(gc) == bits(gc[:, :1])).all()
    elif layout == "mixed":   # every chunk mixes every tier
        assert all(((tc == tier).any(axis=1)).all() for tier in TIERS)
    else:
        assert ((tc != 0).sum(axis=1) == 1).all() and gc.shape[0] >= len(plant_plan(GD))
        bg = gc[tc == 0]
        assert background[0] <= bg.min() and bg.max() <= background[1]
        assert set(np.argmax(tc != 0, axis=1).tolist()) == set(range(CHUNK))   # the planted lane cycles through all 64
        for lane in EDGE_LANES:
            assert set(tc[:, lane].tolist()) >= set(TIERS), (lane, sorted(set(tc[:, lane].tolist())))


@pytest.mark.parametrize("GD,frame", [(GD, f) for GD in DEPTHS[1:] for f in (ODD, MANY_TASKS)] + [(16, FALLBACK), (17, FALLBACK)])
def test_every_lattice_value_occurs_in_the_other_mixed_frames(GD, frame):
    L, T = lattice(GD)
    g, t = guide_frame(GD, "mixed", frame[:3])
    assert set(bits(L).tolist()) == set(bits(g).ravel().tolist())
    if frame[2] % CHUNK == 0:
        tc = t.reshape(-1, CHUNK)
        assert all(((tc == tier).any(axis=1)).all() for tier in TIERS)


def test_planted_frames_split_the_plane_halves_by_one_lane():
    """GD = 16: the gradient pass contracts planes 0 .. 7 and 8 .. 15 separately and skips a half no lane of the chunk
    touches.  Over the lower background some chunk has exactly ONE lane whose upper tap reaches plane 8, over the upper
    background some chunk has exactly one lane whose lower tap lies below it -- at each of EDGE_LANES."""
    for background, one_lane in ((LOWER, lambda zP, zQ: zQ >= 8), (UPPER, lambda zP, zQ: zP < 8)):
        g, t = guide_frame(16, "planted", LAYOUT_FRAMES["planted"][:3], background)
        hit = one_lane(*taps(g, 16)).reshape(-1, CHUNK)
        tc = t.reshape(-1, CHUNK)
        single = hit.sum(axis=1) == 1
        assert single.any()
        assert (tc[hit & single[:, None]] != 0).all()       # the one lane is the planted one
        lanes = set(np.argmax(hit[single], axis=1).tolist())
        assert lanes >= set(EDGE_LANES), sorted(lanes)


# ---- 2. the two oracles agree bit for bit on the lattice ---------------------------------------------------------------------
def oracle_outputs(O, op, grid, g, x, dout):
    if op == "apply":
        return (O.bilateral_slice_apply(grid, g, x, True),) + tuple(O.bilateral_slice_apply_grad(grid, g, x, dout, True))
    return (O.bilateral_slice(grid, g),) + tuple(O.bilateral_slice_grad(grid, g, dout))


@pytest.mark.parametrize("GD", DEPTHS)
@pytest.mark.parametrize("op", ["apply", "slice"])
def test_port_equals_compiled_reference_on_the_lattice(port, ref_or_none, op, GD):
    """out, dgrid, dguide (and dinput) of the C restatement against the reference's own code compiled unchanged, bit for
    bit, on every layout; every value finite, the wild tier included: the comparison on the GPU has a definite answer."""
    if ref_or_none is None:
        pytest.skip("the compiled reference is not built here")
    for layout, background in LAYOUTS:
        frame = LAYOUT_FRAMES[layout]
        g, _ = guide_frame(GD, layout, frame[:3], background)
        grid, x, dout = problem_arrays(frame, GD, 12, 3 if op == "apply" else 0, 3 if op == "apply" else 12, 77 + GD)
        got = oracle_outputs(port, op, grid, g, x, dout)
        want = oracle_outputs(ref_or_none, op, grid, g, x, dout)
        for name, a, b in zip(("out", "dgrid", "dguide", "dinput"), got, want):
            assert np.isfinite(b).all(), (layout, name)
            assert np.array_equal(bits(a), bits(b)), (layout, background, name, int((bits(a) != bits(b)).sum()))


# ---- 3. a closed form that uses neither oracle ---------------------------------------------------------------------------------
TOL = 4.09e-7   # 2 x 2.043e-7, see test_out_of_range_guides_clamp_closed_form


def closed_form(G, g, GD):
    """sum over the taps floor(gz - 0.5), + 1 of max(1 - sqrt(d^2 + 1e-8), 0) * G[clamp(tap, 0, GD - 1)], d = tap + 0.5 -
    gz, with gz the float32 product and everything after it in float64."""
    gz = gz_product(g, GD).astype(np.float64)
    t0 = np.floor(gz - 0.5)
    out = 0.0
    for tap in (t0, t0 + 1.0):
        d = tap + 0.5 - gz
        w = np.maximum(1.0 - np.sqrt(d * d + 1e-8), 0.0)
        out = out + w[..., None] * G[np.clip(tap, 0, GD - 1).astype(np.int64)]
    return out


@pytest.mark.parametrize("GD", DEPTHS)
def test_out_of_range_guides_clamp_closed_form(port, ref_or_none, GD):
    """A grid that varies in z only: the slice is the two-tap z blend alone, whatever x and y.  On tiers 1 and 2 this pins
    that a guide outside [0, 1] CLAMPS -- both taps fold onto the border plane, whose weight sums to 1 - 2e-8 far out and
    to the peak 1 - 1e-4 at the border's own half cell; it neither mirrors nor fades to zero -- and that guide == 1.0f
    reads plane GD - 1 alone.  Tier 3 is left to the bit equality above: no closed form of an artefact is asserted.

    Tolerance: the largest distance of the compiled reference from the closed form over the six depths, measured on the
    development machine, is 2.043e-7 (at GD = 7; 1.30e-7 .. 1.96e-7 at the other depths: a few float32 roundings of weights
    that sum to 1 on values in [0, 1)); twice that, 4.09e-7, is allowed."""
    O = ref_or_none if ref_or_none is not None else port
    frame = LAYOUT_FRAMES["mixed"]
    B, H, W, GH, GW = frame
    g, t = guide_frame(GD, "mixed", frame[:3])
    G = np.random.default_rng(5 + GD).random((GD, 4))
    grid = np.ascontiguousarray(np.broadcast_to(G.astype(np.float32), (B, GH, GW, GD, 4)))
    G = G.astype(np.float32).astype(np.float64)
    out = O.bilateral_slice(grid, g).astype(np.float64)
    keep = t != 3
    assert (t[keep] >= 1).all() and set(t[keep].tolist()) == {1, 2}
    want = closed_form(G, g, GD)
    dist = np.abs(out - want)[keep].max()
    print(f"GD={GD}: max|{O.kind} - closed form| on tiers 1, 2 = {dist:.3e}")
    assert dist <= TOL
    # far out, both taps ARE the border plane: its weight is between the peak (on a switch) and 1 - 2e-8 (between two)
    gz = gz_product(g, GD).astype(np.float64)
    d0 = np.floor(gz - 0.5) + 0.5 - gz
    wsum = sum(np.maximum(1.0 - np.sqrt(d * d + 1e-8), 0.0) for d in (d0, d0 + 1.0))[..., None]
    far_lo, far_hi = keep & (gz <= -1.0), keep & (gz >= GD + 1.0)
    assert far_lo.any() and far_hi.any() and wsum[far_lo | far_hi].min() >= 1.0 - 1.0001e-4
    assert np.abs(out - wsum * G[0])[far_lo].max() <= TOL and np.abs(out - wsum * G[GD - 1])[far_hi].max() <= TOL
    one = bits(g) == bits(np.float32(1.0))
    assert one.any() and np.abs(out[one] - G[GD - 1]).max() <= TOL
