"""The row plan of the row-segment kernels, restated (hdrnet_amd/csrc/row_geom.h: make_row_plan, seg_fwd_geom,
rows_fwd_geom, io_fwd_geom) for Cin = Cout = 3 with offset (C = 12): the GPU tests predict from it which kernel a shape
reaches (tests/test_gpu_fused_fullsize.py), and tests/test_row_geom.py holds the header to it cell by cell."""


def _rup(v, m):
    return (v + m - 1) // m * m


def row_plan(W):
    best = None
    for threads in (256, 192, 128):
        nseg = -(-W // (4 * threads))
        waste = nseg * 4 * threads - W
        if best is None or waste < best[0]:
            best = (waste, nseg)
    nseg = best[1]
    seg = _rup(-(-W // nseg), 4)
    return min(_rup(-(-seg // 4), 64), 256), nseg, seg


def seg_fits(W, GW, GD, guide_map):
    """seg_fwd_geom(dma = true, guide_map).ok: (GD + 2) planes of the window's columns + the slabs in 64 KiB."""
    threads, _, seg = row_plan(W)
    cols = (seg - 1) * GW // W + 4
    slabw = 256 * 3 + (256 if guide_map else 0)
    return (_rup(cols * (GD + 2) * 12, 4) + threads // 64 * slabw) * 4 <= 65536


def rows_fits(W, GW, GD):
    """rows_fwd_geom(...).ok: GD planes of at most GW columns + the per-wave slabs in 64 KiB."""
    threads, _, seg = row_plan(W)
    cols = min((seg - 1) * GW // W + 4, GW)
    return (cols * GD * 12 + 4 + threads // 64 * 256 * 3) * 4 <= 65536


def io_fits(W, GW, GD):
    """io_fwd_geom(...).ok: the curves kernel's static tables (768 floats) + (GD + 2) planes + the slabs in 64 KiB."""
    threads, _, seg = row_plan(W)
    cols = (seg - 1) * GW // W + 4
    return (768 + _rup(cols * (GD + 2) * 12, 4) + threads // 64 * 256 * 3) * 4 <= 65536
