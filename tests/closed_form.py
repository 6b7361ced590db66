"""Expected values of BilateralSliceApply / BilateralSlice that a reader can check by hand (numpy, float64).

Written from the reference's own text and from nothing in this repository (it imports nothing from oracle/ or
hdrnet_amd/), so that an oracle and a kernel that share one misreading of the layout cannot pass together:

* layout -- hdrnet/ops/bilateral_slice_apply_op.cc:201-227: the grid is [B, GH, GW, GD, C] with c changing fastest, and
  c is read as (i, j) with j (the input channel, the offset last) changing fastest, then i (the output channel); guide
  [B, H, W]; input [B, H, W, Cin]; output [B, H, W, Cout].  Here that order is stated ONLY as numpy shapes: np.arange
  reshaped to [B, GH, GW, GD, C], and the same array viewed as [B, GH, GW, GD, Cout, Cj].
* weights -- hdrnet/ops/numerics.h:53-126: the tent max(1 - |d|, 0) in x and y; in z the smoothed tent
  max(1 - sqrt(d * d + 1e-8f), 0), whose derivative d / sqrt(d * d + 1e-8f) is cut to 0 where the smoothed |d| exceeds 1.
* coordinates -- hdrnet/ops/bilateral_slice_apply.cc:37-48, :121-125, :186-187: pixel p sits at (p + 0.5) * gn / n, the
  guide at guide * GD (no half-cell shift in z), the two taps are floor(c - 0.5) and the next cell, each CLAMPED into the
  grid (not mirrored), and the guide derivative carries a factor GD.

Nothing below walks the eight corners of a cell or forms a linear offset: x and y are matrices [pixels, cells]
(`axis_matrix`), z is a pair of taps per pixel (`z_taps`), and an expected value is a product of those.

Three families:

(i)   ADDRESS CODES.  grid = 1 + its own linear index (`address_codes`), frames whose height and width are odd multiples
      of the grid's, so that pixel (my * gy + (my - 1) / 2, mx * gx + (mx - 1) / 2) is the centre of cell (gy, gx)
      (`centre_pixels`), a constant guide at the centre of plane gz (`plane_guide`, exact for GD a power of two).  There
      the x and y tents are exactly 1 and 0, the far z tap has weight exactly 0 and the near one PEAK, so
      out / PEAK reads one grid entry back: `decode`.
(ii)  ONE AXIS AT A TIME.  grid = Y[gy] * X[gx] * Z[gz] * K[c] with all but one factor constant (`separable_grid`):
      out = (Wy Y)[y] (Wx X)[x] S_Z(guide) . affine_K(input) -- `separable_forward`, `separable_dguide`.
(iii) ONE PLANE.  A constant guide at a plane centre with a random grid: out = PEAK Wy grid[:, :, gz] Wx^T, dgrid lives
      in that plane alone, dinput = PEAK sum_i dout_i (Wy grid_ij Wx^T) -- `plane_forward`, `plane_dgrid`, `plane_dinput`.
"""
import numpy as np

F32 = np.float32
EPS = np.float64(np.float32(1e-8))      # numerics.h:83: the eps of SmoothedAbs, a float
PEAK = 1.0 - np.sqrt(EPS)               # the smoothed tent at distance 0: 1 - sqrt(1e-8f) = 0.9999
DECODE_BAR = 0.25                       # |out / PEAK - code|: a wrong cell, plane or channel is off by at least 1


# ---- x and y: one matrix per axis --------------------------------------------------------------------------------------
def axis_matrix(n, gn):
    """[n, gn]: row p holds the weights with which pixel p of an n-pixel axis reads the gn cells.  c = (p + 0.5) * gn / n
    (formed in float32 as bilateral_slice_apply.cc:37-42 forms it: it decides which cells are read), g0 = floor(c - 0.5),
    the taps g0 and g0 + 1 weigh max(1 - |g + 0.5 - c|, 0) and land on the clamped cell."""
    p = np.arange(n)
    c = (p.astype(F32) + F32(0.5)) * (F32(gn) / F32(n))
    g0 = np.floor(c - F32(0.5)).astype(np.int64)
    M = np.zeros((n, gn))
    for g in (g0, g0 + 1):
        w = np.maximum(1.0 - np.abs((g + 0.5) - c.astype(np.float64)), 0.0)
        np.add.at(M, (p, np.clip(g, 0, gn - 1)), w)
    return M


def centre_pixels(n, gn):
    """The pixels that sit on cell centres of an axis with n = gn * m pixels, m odd: m * g + (m - 1) / 2."""
    m = n // gn
    assert m * gn == n and m % 2 == 1, (n, gn)
    return m * np.arange(gn) + (m - 1) // 2


# ---- z: two taps per pixel ---------------------------------------------------------------------------------------------
def z_taps(guide, GD):
    """For a float32 guide [..]: (cell [2, ..] clamped, w [2, ..], dw [2, ..]) of the taps gz0 and gz0 + 1, gz0 =
    floor(guide * GD - 0.5) with guide * GD rounded to float32 (bilateral_slice_apply.cc:44-48).  w = max(1 - s, 0) and
    dw = (s > 1 ? 0 : dz / s) with dz = gz + 0.5 - guide * GD and s = sqrt(dz * dz + eps); whether s exceeds 1 is asked
    of the float32 value, as numerics.h:116-126 asks it (a tap exactly one cell away is NOT cut there)."""
    guide = np.asarray(guide)
    assert guide.dtype == np.float32
    gzf = guide * F32(GD)
    gz0 = np.floor(gzf - F32(0.5)).astype(np.int64)
    gz = np.stack([gz0, gz0 + 1])
    dz32 = (gz.astype(F32) + F32(0.5)) - gzf
    dz = dz32.astype(np.float64)
    s = np.sqrt(dz * dz + EPS)
    cut = np.sqrt(dz32 * dz32 + F32(1e-8), dtype=F32) > F32(1.0)
    return np.clip(gz, 0, GD - 1), np.maximum(1.0 - s, 0.0), np.where(cut, 0.0, dz / s)


def z_sample(guide, Z):
    """(S, dS/dguide) of a profile Z[gz] under the guide: S = sum_d w_d Z[cell_d], dS = GD sum_d dw_d Z[cell_d]
    (the factor GD: bilateral_slice_apply.cc:186-187)."""
    Z = np.asarray(Z, np.float64)
    cell, w, dw = z_taps(guide, len(Z))
    return (w * Z[cell]).sum(0), len(Z) * (dw * Z[cell]).sum(0)


def plane_guide(B, H, W, gz, GD):
    """The constant guide at the centre of plane gz; exact in float32, and guide * GD = gz + 0.5 exactly, for GD a power
    of two."""
    assert GD & (GD - 1) == 0, GD
    return np.full((B, H, W), (gz + 0.5) / GD, np.float32)


# ---- the per-pixel affine map ------------------------------------------------------------------------------------------
def with_one(inp, has_offset):
    """[.., Cin] -> [.., Cj] float64: the input with the constant 1 of the offset column behind it."""
    inp = np.asarray(inp, np.float64)
    return np.concatenate([inp, np.ones(inp.shape[:-1] + (1,))], -1) if has_offset else inp


def affine(A, inp, has_offset):
    """out_i = sum_j A[.., i, j] in_j (+ A[.., i, Cin]): the coefficients A [.., Cout, Cj] on the input [.., Cin]."""
    return np.einsum("...ij,...j->...i", A, with_one(inp, has_offset))


def as_matrix(a, Cj):
    """[.., C] -> [.., Cout, Cj]: channel c is (i, j) with j changing fastest (bilateral_slice_apply_op.cc:203)."""
    assert a.shape[-1] % Cj == 0
    return a.reshape(a.shape[:-1] + (a.shape[-1] // Cj, Cj))


# ---- (i) address codes ---------------------------------------------------------------------------------------------------
def address_codes(B, GH, GW, GD, C):
    """grid[b, gy, gx, gz, c] = 1 + its position in memory; every code is an integer below 2^24, exact in float32."""
    n = B * GH * GW * GD * C
    assert n < (1 << 24)
    return np.arange(1, n + 1, dtype=np.float32).reshape(B, GH, GW, GD, C)


def decode(run, grid_shape, H, W, Cin, has_offset):
    """Read a grid back through an implementation.  `run(guide, j)` -> [B, H, W, Cout]: the forward on the guide map with
    the one-hot input e_j in every pixel (the zero input for j None).  For every plane gz: the zero input reads the offset
    column (with an offset), e_j reads column j on top of it.  Returns (got, dev): got [B, GH, GW, GD, Cout, Cj] =
    round(out / PEAK), the zero-input launch subtracted from the one-hot ones; dev: the same array before rounding minus
    its rounding, i.e. how far each launch's out / PEAK was from an integer, summed over the two launches it came from."""
    B, GH, GW, GD, C = grid_shape
    Cj = Cin + (1 if has_offset else 0)
    ys, xs = centre_pixels(H, GH), centre_pixels(W, GW)
    got = np.zeros((B, GH, GW, GD, C // Cj, Cj))
    dev = np.zeros_like(got)
    for gz in range(GD):
        guide = plane_guide(B, H, W, gz, GD)

        def centres(j):
            out = np.asarray(run(guide, j), np.float64)
            assert out.shape == (B, H, W, C // Cj), out.shape
            v = out[:, ys][:, :, xs] / PEAK
            return np.rint(v), np.abs(v - np.rint(v))

        base, base_dev = centres(None) if has_offset else (0.0, 0.0)
        if has_offset:
            got[:, :, :, gz, :, Cin], dev[:, :, :, gz, :, Cin] = base, base_dev
        for j in range(Cin):
            v, d = centres(j)
            got[:, :, :, gz, :, j], dev[:, :, :, gz, :, j] = v - base, d + base_dev
    return got, dev


def check_decode(got, dev, codes, Cj, name):
    """Every cell, plane, i and j: the decoded integer equals the code and each launch was within DECODE_BAR of an
    integer.  Prints the worst deviation; returns the number of wrong decodes (asserting is the caller's)."""
    want = as_matrix(codes.astype(np.float64), Cj)
    wrong = int((got != want).sum())
    print(f"{name}: {got.size} codes up to {int(want.max())}, {wrong} wrong, max |out / PEAK - integer| = {dev.max():.4f}")
    return wrong, float(dev.max())


# ---- (ii) one axis at a time -------------------------------------------------------------------------------------------
def separable_grid(B, Y, X, Z, K):
    """grid[b, gy, gx, gz, c] = Y[gy] X[gx] Z[gz] K[c] in float32.  The callers pick factors of few bits (dyadic
    rationals), so that the product is exact and the float32 grid IS the product."""
    g = np.einsum("y,x,z,c->yxzc", *(np.asarray(a, np.float64) for a in (Y, X, Z, K)))
    g32 = g.astype(np.float32)
    assert np.array_equal(g32.astype(np.float64), g), "factors too fine: the float32 grid is not their product"
    return np.ascontiguousarray(np.broadcast_to(g32, (B,) + g32.shape))


def _plane_factor(H, W, Y, X):
    return (axis_matrix(H, len(Y)) @ np.asarray(Y, np.float64))[:, None] * (axis_matrix(W, len(X)) @ np.asarray(X, np.float64))[None, :]


def separable_forward(guide, inp, Y, X, Z, K, has_offset):
    """out = (Wy Y)[y] (Wx X)[x] S_Z(guide) affine_K(input).  With Y = X = 1 the first two factors are the row sums of
    the axis matrices, 1; with Z = 1 the third is w_0 + w_1."""
    B, H, W = guide.shape
    Cj = inp.shape[-1] + (1 if has_offset else 0)
    S, _ = z_sample(guide, Z)
    return (_plane_factor(H, W, Y, X) * S)[..., None] * affine(as_matrix(np.asarray(K, np.float64), Cj), inp, has_offset)


def separable_dguide(guide, inp, dout, Y, X, Z, K, has_offset):
    """dguide = (Wy Y)[y] (Wx X)[x] dS_Z/dguide sum_i dout_i affine_K(input)_i."""
    B, H, W = guide.shape
    Cj = inp.shape[-1] + (1 if has_offset else 0)
    _, dS = z_sample(guide, Z)
    a = affine(as_matrix(np.asarray(K, np.float64), Cj), inp, has_offset)
    return _plane_factor(H, W, Y, X) * dS * (np.asarray(dout, np.float64) * a).sum(-1)


def separable_dinput(guide, inp, dout, Y, X, Z, K, has_offset):
    """dinput_j = (Wy Y)[y] (Wx X)[x] S_Z(guide) sum_i dout_i K[i, j]."""
    B, H, W = guide.shape
    Cin = inp.shape[-1]
    S, _ = z_sample(guide, Z)
    A = as_matrix(np.asarray(K, np.float64), Cin + (1 if has_offset else 0))[:, :Cin]
    return (_plane_factor(H, W, Y, X) * S)[..., None] * (np.asarray(dout, np.float64) @ A)


def axis_case(axis, B, H, W, GH, GW, GD, Cin, Cout, has_offset, seed):
    """The data of one case of (ii): the grid varies along `axis` ("z", "x" or "y") only -- or, for "xyz", along all
    three as a product, which is what holds the x and y weights of the guide derivative (under a grid constant in z the
    two taps' derivatives cancel).  Z is not symmetric about the middle plane, X and Y are random; every factor is a
    dyadic rational of few bits.  Cin = 0 with an offset is the slice op (C = Cout).  The guide is random in
    [-0.1, 1.1]: both z borders are crossed."""
    assert axis in ("z", "x", "y", "xyz"), axis
    rng = np.random.default_rng(seed)
    C = Cout * (Cin + (1 if has_offset else 0))
    Y, X, Z = np.ones(GH), np.ones(GW), np.ones(GD)
    fine = 8.0 if axis == "xyz" else 32.0     # coarser factors where three of them multiply
    if "z" in axis:
        Z = 0.25 + 0.5 * (np.arange(GD) + 0.5) / GD
    if "x" in axis:
        X = rng.integers(-fine, fine + 1, GW) / fine
    if "y" in axis:
        Y = rng.integers(-fine, fine + 1, GH) / fine
    K = rng.integers(-8, 9, C) / 4.0 if axis == "xyz" else rng.integers(-16, 17, C) / 8.0
    return dict(Y=Y, X=X, Z=Z, K=K, has_offset=has_offset, grid=separable_grid(B, Y, X, Z, K),
                guide=rng.uniform(-0.1, 1.1, (B, H, W)).astype(np.float32),
                inp=rng.random((B, H, W, Cin), dtype=np.float32),
                dout=rng.standard_normal((B, H, W, Cout)).astype(np.float32))


def plane_case(gz, B, H, W, GH, GW, GD, Cin, Cout, has_offset, seed):
    """The data of one case of (iii): a random grid, input and dout under the constant guide of plane gz."""
    rng = np.random.default_rng(seed)
    C = Cout * (Cin + (1 if has_offset else 0))
    return dict(gz=gz, has_offset=has_offset, grid=rng.standard_normal((B, GH, GW, GD, C)).astype(np.float32),
                guide=plane_guide(B, H, W, gz, GD), inp=rng.random((B, H, W, Cin), dtype=np.float32),
                dout=rng.standard_normal((B, H, W, Cout)).astype(np.float32))


# ---- (iii) one plane -----------------------------------------------------------------------------------------------------
def plane_coefficients(grid, gz, H, W):
    """PEAK Wy grid[:, :, :, gz] Wx^T -> [B, H, W, C]: what every pixel reads under plane_guide(gz)."""
    B, GH, GW, GD, C = grid.shape
    return PEAK * np.einsum("yg,bghc,xh->byxc", axis_matrix(H, GH), grid[:, :, :, gz].astype(np.float64),
                            axis_matrix(W, GW))


def plane_forward(grid, gz, inp, has_offset):
    B, H, W, Cin = inp.shape
    Cj = Cin + (1 if has_offset else 0)
    return affine(as_matrix(plane_coefficients(grid, gz, H, W), Cj), inp, has_offset)


def plane_dgrid(grid_shape, gz, inp, dout, has_offset):
    """dgrid[:, :, :, gz, (i, j)] = PEAK Wy^T (dout_i in_j) Wx; every other plane is exactly zero."""
    B, GH, GW, GD, C = grid_shape
    _, H, W, Cout = dout.shape
    outer = np.einsum("byxi,byxj->byxij", np.asarray(dout, np.float64), with_one(inp, has_offset)).reshape(B, H, W, C)
    dgrid = np.zeros(grid_shape)
    dgrid[:, :, :, gz] = PEAK * np.einsum("yg,byxc,xh->bghc", axis_matrix(H, GH), outer, axis_matrix(W, GW))
    return dgrid


def plane_dinput(grid, gz, inp, dout, has_offset):
    """dinput_j = PEAK sum_i dout_i (Wy grid_ij Wx^T)."""
    B, H, W, Cin = inp.shape
    A = as_matrix(plane_coefficients(grid, gz, H, W), Cin + (1 if has_offset else 0))
    return np.einsum("byxi,byxij->byxj", np.asarray(dout, np.float64), A[..., :Cin])


# ---- what a case expects -------------------------------------------------------------------------------------------------
def axis_expected(case):
    """(ii): out, dguide and dinput of an axis_case."""
    a = (case["guide"], case["inp"])
    f = (case["Y"], case["X"], case["Z"], case["K"], case["has_offset"])
    return dict(out=separable_forward(*a, *f), dguide=separable_dguide(*a, case["dout"], *f),
                dinput=separable_dinput(*a, case["dout"], *f))


def plane_expected(case):
    """(iii): out, dgrid and dinput of a plane_case."""
    g, gz, inp, dout, off = (case[k] for k in ("grid", "gz", "inp", "dout", "has_offset"))
    return dict(out=plane_forward(g, gz, inp, off), dgrid=plane_dgrid(g.shape, gz, inp, dout, off),
                dinput=plane_dinput(g, gz, inp, dout, off))
