"""Which kernels the two gradient entry points pick, cell by cell.

hdrnet_bilateral_slice_apply_grad_f32_ex and hdrnet_bilateral_slice_grad_f32_ex share one ladder (capi.hip,
grad_dispatch: fused pass, per-pixel fast kernel, MFMA dgrid, the op's generic kernel).  This calls both through
ctypes on torch buffers -- the workspace has to be controlled -- and crosses

* op and shape class: apply (3,3,offset), (1,1,offset), (4,4,offset), (2,2,offset) and Cin = 0 with offset; slice
  C = 12, 2, 3.  Cin = 0 with offset has Cout = 12: the numbers of the slice op's C = 12, so a lost op tag would
  show as a slice kernel's name;
* family: auto, generic, fast;
* wanted outputs: every subset, the empty one included (Cin = 0 has no dinput to want);
* workspace: as queried, null, one byte short;
* B = 0 once per op.

B = 2, 12 x 32 pixels, grid 3 x 4 x 8: batch 2 and unequal grid extents are the smallest sizes at which a swapped
stride or extent shows.  One more geometry with GD = 16 (two plane tiles in the fused pass) and one with W = 30
(no whole float4 rows) for apply (3,3,offset) and slice C = 12.  No cell needed a larger frame to reach its fast
kernel.

For every cell: the exact hdrnet_last_kernel() string, or the return code and message, as recorded in
tests/golden/grad_dispatch.json from the library BEFORE the two ladders became one (recorded by running cells()
below against that library on an MI355X; read against the ladder by eye).  Where a non-generic kernel ran, each
gradient it produced agrees with the generic family's on the same inputs within the suite's gradient tolerances
(tests/conftest.py: dgrid rtol 1e-4 and 1e-5 x max, dguide and dinput at their flat atols).  All shapes are far
below the frame size at which a generic dgrid draws its stderr line, which the test asserts through capfd.
"""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from conftest import GOLDEN, check_dgrid, check_pixel_grad  # noqa: E402

B, H, W, GH, GW, GD = 2, 12, 32, 3, 4, 8
FAMILIES = {"auto": 0, "generic": 1, "fast": 2}
WORKSPACES = ("queried", "null", "short")

# shape class -> (op, Cin, Cout, has_offset); for the slice op Cout is its C
SHAPES = {
    "apply_3_3_off": ("apply", 3, 3, 1),
    "apply_1_1_off": ("apply", 1, 1, 1),
    "apply_4_4_off": ("apply", 4, 4, 1),
    "apply_2_2_off": ("apply", 2, 2, 1),
    "apply_0_12_off": ("apply", 0, 12, 1),
    "slice_12": ("slice", 0, 12, 1),
    "slice_2": ("slice", 0, 2, 1),
    "slice_3": ("slice", 0, 3, 1),
}
# (shape class, H, W, GD) of every group of cells: the full cross at the base geometry, then the two extra geometries
GROUPS = [(s, H, W, GD) for s in SHAPES] + [(s, h, w, gd) for s in ("apply_3_3_off", "slice_12")
                                            for h, w, gd in ((H, W, 16), (H, 30, GD))]


def outputs_of(shape):
    op, Cin, _, _ = SHAPES[shape]
    return ("dgrid", "dguide", "dinput") if op == "apply" and Cin > 0 else ("dgrid", "dguide")


def cells(shape, full):
    """(family, wanted outputs, workspace) of one group: the whole cross, or for the extra geometries every family
    with all outputs and the queried workspace."""
    outs = outputs_of(shape)
    if not full:
        return [(f, outs, "queried") for f in FAMILIES]
    subsets = [tuple(o for o, on in zip(outs, mask) if on) for mask in itertools.product((1, 0), repeat=len(outs))]
    return list(itertools.product(FAMILIES, subsets, WORKSPACES))


def cell_id(shape, h, w, gd, family, wanted, ws):
    return "%s %dx%d gd%d %s [%s] ws=%s" % (shape, h, w, gd, family, ",".join(wanted), ws)


def bind(lib):
    from hdrnet_amd import _lib
    for name in ("hdrnet_bilateral_slice_apply_grad_f32_ex", "hdrnet_bilateral_slice_grad_f32_ex",
                 "hdrnet_bilateral_slice_apply_grad_workspace_bytes", "hdrnet_bilateral_slice_grad_workspace_bytes"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    lib.hdrnet_last_error.restype = ctypes.c_char_p
    lib.hdrnet_last_kernel.restype = ctypes.c_char_p
    lib.hdrnet_enable_kernel_names(1)
    return lib


class Problem:
    """The inputs of one group on the device, and the generic family's gradients of them (computed once)."""

    def __init__(self, lib, dev, shape, b, h, w, gd):
        self.lib, self.dev, self.shape = lib, dev, shape
        self.op, self.Cin, self.Cout, self.off = SHAPES[shape]
        self.b, self.h, self.w, self.gd = b, h, w, gd
        Cj = 1 if self.op == "slice" else self.Cin + self.off
        rng = np.random.default_rng(len(shape) * 1000 + h * w + gd)
        up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        self.grid = up(rng.random((b, GH, GW, gd, self.Cout * Cj), dtype=np.float32))
        self.guide = up(rng.random((b, h, w), dtype=np.float32))
        self.input = up(rng.random((b, h, w, max(self.Cin, 1)), dtype=np.float32))
        self.dout = up(rng.standard_normal((b, h, w, self.Cout)).astype(np.float32))
        self.out_shapes = {"dgrid": tuple(self.grid.shape), "dguide": (b, h, w), "dinput": (b, h, w, self.Cin)}
        if self.op == "apply":
            self.ws_bytes = lib.hdrnet_bilateral_slice_apply_grad_workspace_bytes(b, h, w, GH, GW, gd, self.Cin, self.Cout,
                                                                                  self.off)
        else:
            self.ws_bytes = lib.hdrnet_bilateral_slice_grad_workspace_bytes(b, h, w, GH, GW, gd, self.Cout)
        self.ws = torch.empty(max(self.ws_bytes, 16), dtype=torch.uint8, device=dev)
        self.generic = None

    def call(self, family, wanted, ws):
        """-> (outcome, {output: array}).  The outcome is the kernel name, or "rc=N: message"."""
        outs = {o: torch.full(self.out_shapes[o] if self.b else (1,), float("nan"), device=self.dev) for o in wanted}
        ptr = lambda o: outs[o].data_ptr() if o in outs else None  # noqa: E731
        ws_ptr, ws_bytes = {"queried": (self.ws.data_ptr() if self.ws_bytes else None, self.ws_bytes),
                            "null": (None, 0),
                            "short": (self.ws.data_ptr(), max(self.ws_bytes, 1) - 1)}[ws]
        stream = torch.cuda.current_stream().cuda_stream
        dims = (self.b, self.h, self.w, GH, GW, self.gd)
        if self.op == "apply":
            rc = self.lib.hdrnet_bilateral_slice_apply_grad_f32_ex(
                self.grid.data_ptr(), self.guide.data_ptr(), self.input.data_ptr() if self.Cin else None,
                self.dout.data_ptr(), ptr("dgrid"), ptr("dguide"), ptr("dinput"), *dims, self.Cin, self.Cout, self.off,
                ws_ptr, ws_bytes, FAMILIES[family], stream)
        else:
            rc = self.lib.hdrnet_bilateral_slice_grad_f32_ex(
                self.grid.data_ptr(), self.guide.data_ptr(), self.dout.data_ptr(), ptr("dgrid"), ptr("dguide"), *dims,
                self.Cout, ws_ptr, ws_bytes, FAMILIES[family], stream)
        if rc != 0:
            return "rc=%d: %s" % (rc, self.lib.hdrnet_last_error().decode()), {}
        assert self.lib.hdrnet_last_error() == b""
        return self.lib.hdrnet_last_kernel().decode(), {o: t.cpu().numpy() for o, t in outs.items()}

    def check_against_generic(self, what, got):
        """Every gradient a non-generic kernel produced against the generic family's (conftest's checks: they print
        the figures and assert)."""
        if self.generic is None:
            name, self.generic = self.call("generic", outputs_of(self.shape), "null")
            assert name == self.op + "_grad_generic", name
        for o, g in got.items():
            if o == "dgrid":
                check_dgrid(g, self.generic[o], what)
            else:
                check_pixel_grad(g, self.generic[o], what, o)


def run_group(lib, dev, shape, h, w, gd):
    """{cell id: outcome} of one group; the numeric check of every cell that ran a non-generic kernel."""
    p = Problem(lib, dev, shape, B, h, w, gd)
    seen = {}
    for family, wanted, ws in cells(shape, full=(h, w, gd) == (H, W, GD)):
        cid = cell_id(shape, h, w, gd, family, wanted, ws)
        outcome, got = p.call(family, wanted, ws)
        seen[cid] = outcome
        if got and outcome != p.op + "_grad_generic":
            assert outcome != "noop", cid
            p.check_against_generic(cid, got)
    return seen


def run_noop(lib, dev, shape):
    p = Problem(lib, dev, shape, 0, H, W, GD)
    return {cell_id(shape, H, W, GD, "auto", outputs_of(shape), "queried") + " B=0":
            p.call("auto", outputs_of(shape), "queried")[0]}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run with -m gpu on the MI355X box"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import build
    return bind(ctypes.CDLL(build.build()))


@pytest.fixture(scope="module")
def expected():
    with open(os.path.join(GOLDEN, "grad_dispatch.json")) as fh:
        return json.load(fh)


def compare(seen, expected, capfd):
    wrong = {cid: (got, expected.get(cid)) for cid, got in seen.items() if got != expected.get(cid)}
    assert not wrong, "\n".join("%s: %r, recorded %r" % (cid, g, e) for cid, (g, e) in wrong.items())
    assert "takes the generic grid-gradient kernel" not in capfd.readouterr().err


@pytest.mark.parametrize("group", GROUPS, ids=["%s-%dx%d-gd%d" % g for g in GROUPS])
def test_dispatch_picks_what_it_picked(lib, dev, expected, capfd, group):
    compare(run_group(lib, dev, *group), expected, capfd)


@pytest.mark.parametrize("shape", ["apply_3_3_off", "slice_12"])
def test_empty_batch_is_a_noop(lib, dev, expected, capfd, shape):
    seen = run_noop(lib, dev, shape)
    assert list(seen.values()) == ["noop"]
    compare(seen, expected, capfd)


def test_the_table_is_the_cross(expected):
    """The fixture holds exactly the cells above: none recorded and dropped, none run and unrecorded."""
    ids = [cell_id(s, h, w, gd, *c) for s, h, w, gd in GROUPS for c in cells(s, full=(h, w, gd) == (H, W, GD))]
    ids += [cell_id(s, H, W, GD, "auto", outputs_of(s), "queried") + " B=0" for s in ("apply_3_3_off", "slice_12")]
    assert sorted(ids) == sorted(expected) and len(set(ids)) == len(ids)
    assert len(ids) == 5 * 72 - 36 + 3 * 36 + 4 * 3 + 2   # Cin = 0 has 4 subsets, not 8
