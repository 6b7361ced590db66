"""The guide lattice: the guide values at which a kernel's address or branch changes, and frames that carry them.

The guide is the one operand whose VALUE decides an address (the two z taps) and a branch (the outermost half cells, the
derivative's zero branch, the plane halves of the gradient pass) in every kernel.  The rest of the suite draws it from
continuous distributions over at most [-0.2, 1.2]; a float32 draw does not land on a tap switch guide * GD = k + 0.5, on
exactly 0 or 1, or far outside the grid.  `lattice(GD)` lists those values in three tiers:

  1  switches and borders: k / GD (k = -1 .. GD + 1) and (k + 0.5) / GD (k = -1 .. GD), each also 1, 4 and 64 float32
     ulps to either side; 0.0, -0.0, 1.0, the smallest denormals and the smallest normals of both signs;
  2  out of range but tame (|guide * GD| < 2^22: guide * GD - 0.5 is still exact to a quarter): +-(1 + 0.5 / GD), +-2,
     +-37.5, +-1e3, and +-3e5 where it fits;
  3  wild (2^22 <= |guide * GD| <= 2^30): +-(2^m + j) / GD for m = 22, 23, 24, 25, 30 and j = 0 .. 3.  The reference's tap
     offsets round to 0 or +-2 there and two taps can both carry the peak weight; its int conversion is still defined
     C++, so its outputs -- artefacts as they are -- are definite, and the kernels are held to them.

numpy only: tests/test_guide_lattice_host.py asserts the coverage this file promises for the frames
tests/test_gpu_guide_lattice.py runs."""
import functools

import numpy as np

DEPTHS = (1, 4, 7, 8, 12, 16)
TIERS = (1, 2, 3)
ULP_STEPS = (1, 4, 64)
EDGE_LANES = (0, 31, 32, 63)     # first and last lane of a 64-pixel chunk and the two around its middle
CHUNK = 64                       # the gradient pass works on 64-pixel chunks
LOWER, UPPER = (0.30, 0.40), (0.55, 0.65)   # "planted" backgrounds: at GD = 16 planes 4 .. 6 and 8 .. 10

# B, H, W, GH, GW of the frame a layout is laid into: B * H >= len(lattice) for "rows", B * H * W / 64 >= len(plant_plan)
# for "planted" (held by the host test for every depth)
LAYOUT_FRAMES = {"rows": (1, 352, 128, 4, 8), "mixed": (1, 64, 256, 4, 8), "planted": (1, 96, 256, 4, 8)}
# further frames of the "mixed" layout, which takes any width
FALLBACK = (1, 12, 1024, 8, 64)   # the segment forward's image does not fit at GD >= 16: the row kernels; W >= len(lattice)
ODD = (1, 64, 250, 4, 8)          # W % 4 != 0: the scalar row kernel by width
MANY_TASKS = (8, 96, 32, 3, 8)    # tests/grad_plan_cases.py::PRODUCT_FRAMES[0]: the gradient pass's many-task row plan


def _step(v, n):
    """`v` moved by n float32 ulps (n < 0: downwards)."""
    to = np.float32(np.inf if n > 0 else -np.inf)
    for _ in range(abs(n)):
        v = np.nextafter(v, to, dtype=np.float32)
    return v


def gz_product(g, GD):
    """guide * GD as every implementation forms it: one float32 multiply."""
    return (np.asarray(g, np.float32) * np.float32(GD)).astype(np.float32)


def lattice(GD):
    """-> (values float32 [n], tiers int [n]); every float32 bit pattern once (0.0 and -0.0 are two values)."""
    vals, tiers = _lattice(GD)
    return vals.copy(), tiers.copy()


@functools.lru_cache(maxsize=None)
def _lattice(GD):
    vals, tiers, seen = [], [], set()

    def add(v, tier):
        v = np.float32(v)
        bits = int(v.view(np.uint32))
        if bits not in seen:
            seen.add(bits)
            vals.append(v)
            tiers.append(tier)

    centres = [np.float32(k / GD) for k in range(-1, GD + 2)] + [np.float32((k + 0.5) / GD) for k in range(-1, GD + 1)]
    for c in centres:
        add(c, 1)
        for n in ULP_STEPS:
            add(_step(c, n), 1)
            add(_step(c, -n), 1)
    for v in (0.0, -0.0, 1.0, 1e-45, -1e-45, 1.1754944e-38, -1.1754944e-38):
        add(v, 1)
    for v in (1.0 + 0.5 / GD, 2.0, 37.5, 1e3, 3e5):
        for s in (1.0, -1.0):
            g = np.float32(s * v)
            if abs(float(gz_product(g, GD))) < 2.0 ** 22:
                add(g, 2)
    for m in (22, 23, 24, 25, 30):
        for j in range(4):
            for s in (1.0, -1.0):
                g = np.float32(s * (2.0 ** m + j) / GD)
                if 2.0 ** 22 <= abs(float(gz_product(g, GD))) <= 2.0 ** 30:
                    add(g, 3)
    # the tiers interleaved, each spread evenly over the list: any 64 consecutive values (cyclically) hold all three
    tiers = np.array(tiers, np.int64)
    pos = np.empty(len(vals))
    for t in TIERS:
        idx = np.flatnonzero(tiers == t)
        pos[idx] = (np.arange(len(idx)) + 0.5) / len(idx)
    order = np.argsort(pos, kind="stable")
    return np.array(vals, np.float32)[order], tiers[order]


def plant_plan(GD):
    """The (lattice index, lane) pairs "planted" cycles through, one per chunk: every value once with the lane cycling
    through 0 .. 63, then every tier once more on each of EDGE_LANES (a different value of the tier per lane)."""
    _, tiers = lattice(GD)
    plan = [(i, i % CHUNK) for i in range(len(tiers))]
    for li, lane in enumerate(EDGE_LANES):
        for t in TIERS:
            idx = np.flatnonzero(tiers == t)
            if len(idx):
                plan.append((int(idx[(li * 5 + 1) % len(idx)]), lane))
    return plan


def guide_frame(GD, layout, shape, background=LOWER, seed=0):
    """-> (guide float32 [B, H, W], tier int [B, H, W]; 0 = background) of `layout` in a frame of `shape` = (B, H, W):

      "rows"     row r (counted through the batch) is the constant L[r % n]: every chunk is uniform;
      "mixed"    pixel (r, x) is L[(x + 7 r) % n]: every chunk mixes every tier;
      "planted"  a background drawn uniformly from `background`, one lattice value per 64-pixel chunk (plant_plan)."""
    B, H, W = shape
    L, T = lattice(GD)
    n = len(L)
    r = np.arange(B * H)[:, None]
    x = np.arange(W)[None, :]
    if layout == "rows":
        idx = np.broadcast_to(r % n, (B * H, W))
        g, t = L[idx], T[idx]
    elif layout == "mixed":
        idx = (x + 7 * r) % n
        g, t = L[idx], T[idx]
    elif layout == "planted":
        assert W % CHUNK == 0, W
        rng = np.random.default_rng(1000 * GD + seed)
        lo, hi = background
        g = (lo + (hi - lo) * rng.random((B * H, W), dtype=np.float32)).astype(np.float32)
        t = np.zeros((B * H, W), np.int64)
        plan = plant_plan(GD)
        gc, tc = g.reshape(-1, CHUNK), t.reshape(-1, CHUNK)   # views: chunk c of the frame, rows then batch
        for c in range(gc.shape[0]):
            i, lane = plan[c % len(plan)]
            gc[c, lane], tc[c, lane] = L[i], T[i]
    else:
        raise ValueError(layout)
    return np.ascontiguousarray(g.reshape(B, H, W)), np.ascontiguousarray(t.reshape(B, H, W))


def taps(g, GD):
    """(zP, zQ): the clamped planes of the two z taps of guide values `g`, as the gradient pass forms them
    (floor(guide * GD - 0.5) clamped in float, then + 1 clamped)."""
    fz = np.floor(gz_product(g, GD) - np.float32(0.5))
    zP = np.clip(fz, 0, GD - 1).astype(np.int64)
    return zP, np.minimum(zP + 1, GD - 1)


def problem_arrays(frame, GD, C, Cin, Cout, seed):
    """grid, input and dout as tests/test_gpu_f64_noise.py::problem draws them (rng.random; standard_normal for dout)."""
    B, H, W, GH, GW = frame
    rng = np.random.default_rng(seed)
    grid = rng.random((B, GH, GW, GD, C), dtype=np.float32)
    x = rng.random((B, H, W, max(Cin, 1)), dtype=np.float32)
    dout = rng.standard_normal((B, H, W, Cout)).astype(np.float32)
    return grid, x, dout
