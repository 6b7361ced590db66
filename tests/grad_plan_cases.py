"""Shared by tests/test_gpu_grad_plans.py and tests/test_gpu_workspace_contract.py: device buffers between guard bands,
the frames and variants of the gradient pass the two files run, and the two gradient entry points through ctypes on such
buffers with the CPU oracle's result beside them."""
import itertools

import numpy as np
import torch

GUARD_BYTES = 8192   # wider than a task's partial tile (3 x 16 x 16 floats): a tile written one task too far lands in it
GUARD_BYTE = 0xA5
NAN_BYTE = 0xFF      # 0xFFFFFFFF is a NaN: a word read before it was written poisons what is computed from it


class Guarded:
    """`nbytes` of device memory between two guard bands; the body starts out as NaNs."""

    def __init__(self, nbytes, dev, fill=NAN_BYTE):
        self.nbytes = int(nbytes)
        self.buf = torch.empty((self.nbytes + 2 * GUARD_BYTES,), dtype=torch.uint8, device=dev)
        self.buf[:GUARD_BYTES] = GUARD_BYTE
        self.buf[GUARD_BYTES + self.nbytes:] = GUARD_BYTE
        self.body = self.buf[GUARD_BYTES:GUARD_BYTES + self.nbytes]
        self.body.fill_(fill)
        assert self.body.data_ptr() % 16 == 0
        self.t = None

    @classmethod
    def floats(cls, shape, dev, values=None):
        """A float32 tensor of `shape` (`.t`) between guards: NaNs, or a copy of `values`."""
        g = cls(4 * int(np.prod(shape)), dev)
        g.t = g.body.view(torch.float32).view(shape)
        if values is not None:
            g.t.copy_(values)
        return g

    def ptr(self):
        return self.body.data_ptr()

    def intact(self):
        return bool((self.buf[:GUARD_BYTES] == GUARD_BYTE).all()) and \
            bool((self.buf[GUARD_BYTES + self.nbytes:] == GUARD_BYTE).all())


# B, H, W, GH, GW.  PRODUCT_FRAMES: many task columns on few rows, so that gg_plan gives rg < cell at every occupancy
# (tests/test_grad_plan_host.py); FORCED_FRAMES: run on the tools library at every rg listed (None: min(cell, 4) .. cell).
PRODUCT_FRAMES = [(8, 96, 32, 3, 8), (8, 96, 32, 4, 8), (8, 128, 32, 3, 8)]
FORCED_FRAMES = [((2, 37, 52, 3, 5), None),                        # cell 12, a ragged last group at most rg
                 ((2, 45, 64, 4, 4), None),                        # cell 11
                 ((1, 200, 32, 2, 4), (4, 5, 7, 33, 50, 99, 100)),  # cell 100
                 ((2, 12, 32, 4, 4), None),                        # cell 3: rg = 3 only
                 ((1, 5, 32, 8, 4), None)]                         # H < GH: rg = 1 only

# family -> (op, Cin, Cout, has_offset, the per-pixel gradients that can be wanted beside dgrid on the fast pass, whether
# the op has a fast gradient at all for these channels)
FAMILIES = {
    "apply_3_3_off": ("apply", 3, 3, 1, ("dguide", "dinput"), True),
    "apply_4_4_off": ("apply", 4, 4, 1, (), True),       # 20 grid channels: dgrid alone, as two channel windows
    "slice_12": ("slice", 0, 12, 0, ("dguide",), True),
    "slice_2": ("slice", 0, 2, 0, (), True),             # 2 channels are no float4: dgrid alone on the contraction
    # 3 channels are not among the slice op's fast channel counts (HDRNET_SLICE_FAST_CHANNELS: 1, 2, 4, 8, 12, 16): the
    # workspace query answers 0 and the generic kernel runs, under every plan -- held to exactly that
    "slice_3": ("slice", 0, 3, 0, (), False),
}
VARIANTS = [("apply_3_3_off", 8), ("apply_3_3_off", 16), ("apply_4_4_off", 8), ("apply_4_4_off", 16), ("slice_12", 8),
            ("slice_12", 16), ("slice_2", 8), ("slice_3", 8)]


def frame_id(frame):
    return "%dx%dx%d-grid%dx%d" % frame


def subsets(family):
    """Every subset of the wanted outputs that contains dgrid."""
    extra = FAMILIES[family][4]
    return [("dgrid",) + tuple(o for o, on in zip(extra, mask) if on)
            for mask in itertools.product((1, 0), repeat=len(extra))]


def kernel_name(family, wanted):
    if not FAMILIES[family][5]:
        return FAMILIES[family][0] + "_grad_generic"
    if wanted == ("dgrid",):
        return "grid_grad_mfma"
    return "apply_bwd_fused/mfma" if FAMILIES[family][0] == "apply" else "slice_bwd_fused/mfma"


def grid_channels(family):
    op, Cin, Cout, off = FAMILIES[family][:4]
    return Cout * (Cin + off) if op == "apply" else Cout


def prepare(lib):
    lib.hdrnet_enable_kernel_names(1)
    return lib


class Problem:
    """One frame and variant: inputs on the device, the oracle's gradients of them (computed once), and the call."""

    def __init__(self, port, dev, frame, family, GD, seed, oracle=True):
        self.dev, self.frame, self.family, self.GD = dev, frame, family, GD
        self.op, self.Cin, self.Cout, self.off, _, self.fast = FAMILIES[family]
        B, H, W, GH, GW = frame
        self.C = grid_channels(family)
        rng = np.random.default_rng(seed)
        grid = rng.random((B, GH, GW, GD, self.C), dtype=np.float32)
        # a little past [0, 1]: the forced-1 half cells at both ends of z and the clamp beyond them
        guide = (rng.random((B, H, W), dtype=np.float32) * 1.04 - 0.02).astype(np.float32)
        inp = rng.random((B, H, W, max(self.Cin, 1)), dtype=np.float32)
        dout = rng.standard_normal((B, H, W, self.Cout)).astype(np.float32)
        self.host = dict(grid=grid, guide=guide, input=inp, dout=dout)
        self.want = {}
        if oracle:
            if self.op == "apply":
                got = port.bilateral_slice_apply_grad(grid, guide, inp, dout, bool(self.off))
            else:
                got = port.bilateral_slice_grad(grid, guide, dout)
            self.want = dict(zip(("dgrid", "dguide", "dinput"), got))
        self.dev_in = {k: torch.from_numpy(v).to(dev) for k, v in self.host.items()}
        self.out_shapes = {"dgrid": grid.shape, "dguide": guide.shape, "dinput": (B, H, W, self.Cin)}

    def query(self, lib):
        B, H, W, GH, GW = self.frame
        if self.op == "apply":
            return lib.hdrnet_bilateral_slice_apply_grad_workspace_bytes(B, H, W, GH, GW, self.GD, self.Cin, self.Cout,
                                                                         self.off)
        return lib.hdrnet_bilateral_slice_grad_workspace_bytes(B, H, W, GH, GW, self.GD, self.Cout)

    def call(self, lib, wanted, ws):
        """The ..._ex entry point (flags 0) with the guarded workspace `ws`, exactly its size -> (kernel name,
        {output: Guarded}); the outputs start as NaNs."""
        d = self.dev_in
        outs = {o: Guarded.floats(self.out_shapes[o], self.dev) for o in wanted}
        ptr = lambda o: outs[o].ptr() if o in outs else None  # noqa: E731
        stream = torch.cuda.current_stream().cuda_stream
        dims = self.frame + (self.GD,)
        if self.op == "apply":
            rc = lib.hdrnet_bilateral_slice_apply_grad_f32_ex(
                d["grid"].data_ptr(), d["guide"].data_ptr(), d["input"].data_ptr(), d["dout"].data_ptr(), ptr("dgrid"),
                ptr("dguide"), ptr("dinput"), *dims, self.Cin, self.Cout, self.off, ws.ptr(), ws.nbytes, 0, stream)
        else:
            rc = lib.hdrnet_bilateral_slice_grad_f32_ex(
                d["grid"].data_ptr(), d["guide"].data_ptr(), d["dout"].data_ptr(), ptr("dgrid"), ptr("dguide"), *dims,
                self.Cout, ws.ptr(), ws.nbytes, 0, stream)
        assert rc == 0, lib.hdrnet_last_error().decode()
        torch.cuda.synchronize()
        return lib.hdrnet_last_kernel().decode(), outs

    def check(self, outs, what, check_dgrid, check_pix):
        """Guards, no NaN left, and every output against the oracle at the suite's bars."""
        for o, g in outs.items():
            assert g.intact(), f"{what}: guard band of {o} overwritten"
            got = g.t.cpu().numpy()
            assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} non-finite values left in {o}"
            if o == "dgrid":
                check_dgrid(got, self.want[o], what)
            else:
                check_pix(got, self.want[o], what, o, self.GD)

    def inputs_unchanged(self):
        return all(np.array_equal(t.cpu().numpy(), self.host[k]) for k, t in self.dev_in.items())
