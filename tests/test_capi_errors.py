"""Argument validation of the C-ABI, row by row: every entry point that returns a status answers a table of
deliberately wrong and deliberately empty calls with the return code and the complete hdrnet_last_error() text
recorded in tests/golden/capi_errors.json (tests/golden/make_capi_errors.py: recorded from the library before the
front-end's tails, and later the wire-format forwards' argument rules, were folded into shared helpers), and a legal
no-op names the kernel "noop".

Validation happens before any HIP call, so this runs without a GPU; no row validates fully (the generator refuses
to record one that does), so none reaches one where there is a GPU."""
import ctypes
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

_spec = importlib.util.spec_from_file_location("make_capi_errors", os.path.join(GOLDEN, "make_capi_errors.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

ROWS = json.load(open(os.path.join(GOLDEN, "capi_errors.json")))


@pytest.fixture(scope="module")
def lib():
    from hdrnet_amd import build
    lib = ctypes.CDLL(build.build())
    lib.hdrnet_enable_kernel_names(1)
    return lib


def test_table_covers_every_status_entry_point():
    """>= 3 rows per function of the five binding tables (the coefficient network's training tables have tests of their
    own) that returns a status: wrong extents, a null buffer and a case of its own; the fixture is the generator's
    table, row for row."""
    from hdrnet_amd import _lib
    table = dict(_lib.SIGNATURES)
    for more in (_lib.TRAIN_SIGNATURES, _lib.PIXEL_FORMAT_SIGNATURES, _lib.YUV_SIGNATURES, _lib.PYRAMID_IO_SIGNATURES):
        table.update(more)
    status = sorted(n for n, (res, _) in table.items() if res is ctypes.c_int and n != "hdrnet_version")
    assert sorted(gen.TABLE) == status
    assert [(r["fn"], r["case"]) for r in ROWS] == [(fn, case) for fn, (_, cases) in gen.TABLE.items() for case, _ in cases]
    for fn in status:
        cases = [r["case"] for r in ROWS if r["fn"] == fn]
        assert len(cases) >= 3 and len(set(cases)) == len(cases), (fn, cases)
        assert "wrong extents" in cases and "null buffer" in cases, (fn, cases)
    for r in ROWS:
        assert len(r["args"]) == len(table[r["fn"]][1]), r
        assert r["rc"] == 1 or (r["rc"] == 0 and r["kernel"] == "noop"), r  # nothing here may validate and launch


@pytest.mark.parametrize("row", ROWS, ids=["%s-%s" % (r["fn"][len("hdrnet_"):], r["case"].replace(" ", "_")) for r in ROWS])
def test_wrong_and_empty_calls(lib, row):
    rc, err, kern = gen.call(lib, row["fn"], row["args"])
    assert rc == row["rc"], (rc, err)
    if row["error"] is not None:
        assert err == row["error"]
    else:  # the training-loop helpers had no text when the fixture was recorded: they must have one, and it names them
        assert err.startswith(row["fn"] + ": ") and len(err) > len(row["fn"]) + 2, err
    if row["kernel"] is not None:
        assert kern == row["kernel"] == "noop"
