#!/usr/bin/env python3
"""In-process interleaved A/B timing of BilateralSliceApply forward kernel variants.

    python tools/ab_bench.py [--workload 4k] [--variants 0,19,106,108] [--rounds 5] [--steps 100]
                             [--settle 80] [--yardstick] [--out ab.json]

Variants (include/hdrnet_amd_tools.h): 0 the product kernel, 19 the round-1 row kernel, 106 / 108 the memory skeletons.
(The rejected forwards and the product kernel's own flavours were removed with their kernels; the library refuses their
numbers, and the refusal is reported here.  Their records are DESIGN.md section 4, docs/EXPERIMENTS.md and profiles/.)

Uses the TOOLS build of the library (libhdrnet_amd_tools.so, include/hdrnet_amd_tools.h): variant 0
is the product kernel, the others are documented in that header.  Every round times each variant
once (HIP events around `steps` back-to-back launches over rotating buffer sets larger than the
Infinity Cache), variants interleaved, and the table reports median / min of the per-launch time.
Each variant is first checked against the generic (bit-exact-to-reference) kernel; a variant that the
library refuses, or that fails the check, is reported and dropped, the others still run.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import CACHE_BYTES, WORKLOADS, algorithmic_bytes, make_sets  # noqa: E402
from hdrnet_amd import _lib  # noqa: E402


def time_launches(fn, steps):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for k in range(steps):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / steps  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="4k")
    ap.add_argument("--variants", default="0,19,106,108")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--yardstick", action="store_true")
    ap.add_argument("--settle", type=int, default=80, help="untimed launches of a variant before its timed window")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load_tools()
    lib.hdrnet_enable_kernel_names(1)
    B, H, W, GH, GW, GD, desc = WORKLOADS[args.workload]
    abytes = algorithmic_bytes(B, H, W, GH, GW, GD)
    nsets = max(3, -(-int(CACHE_BYTES * 1.5) // abytes))
    sets = make_sets(dev, nsets, B, H, W, GH, GW, GD, 1234)
    stream = torch.cuda.current_stream(dev).cuda_stream
    variants = [int(v) for v in args.variants.split(",") if v != ""]

    class Refused(RuntimeError):
        """A non-zero return code of the library: its own text."""

    def launcher(flags):
        def fn(k):
            grid, guide, inp, out = sets[k % nsets]
            rc = lib.hdrnet_bilateral_slice_apply_f32_ex(
                grid.data_ptr(), guide.data_ptr(), inp.data_ptr(), out.data_ptr(),
                B, H, W, GH, GW, GD, 3, 3, 1, flags, stream)
            if rc:
                raise Refused(lib.hdrnet_last_error().decode())
        return fn

    # correctness of every variant against the generic kernel (same inputs)
    grid, guide, inp, out = sets[0]
    launcher(_lib.KERNEL_GENERIC)(0)
    ref = out.clone()
    names = {}
    errs = {}
    good = []
    for v in variants:
        try:
            out.fill_(float("nan"))
            launcher(_lib.KERNEL_FAST | (v << 8))(0)
            launcher(_lib.KERNEL_FAST | (v << 8))(0)  # twice: a variant with launch-to-launch state must leave it clean
            torch.cuda.synchronize()
        except Refused as e:
            print(f"variant {v}: refused by the library ({e}), dropped", flush=True)
            continue
        names[v] = lib.hdrnet_last_kernel().decode()
        err = (out - ref).abs().max().item()
        err = float("inf") if err != err else err  # NaN left in the output: pixels nobody wrote
        errs[v] = err
        ok = (err < 1e-5) or names[v].startswith("ABLATION")
        print(f"variant {v} [{names[v]}]: max|fast - generic| = {err:.3e}{'' if ok else '   <-- WRONG, dropped'}",
              flush=True)
        if ok:
            good.append(v)
    variants = good

    results = {v: [] for v in variants}
    yard = {"copy(out<-in, 2x100MB)": [], "elementwise(out=in*a+b, in 133MB out 100MB)": []}
    for r in range(args.rounds):
        for v in variants:
            fn = launcher(_lib.KERNEL_FAST | (v << 8))
            # settle: cache-policy stores run ~15 % slower for the first ~50 launches after a kernel that left
            # plain-store dirty lines behind (profiles/r02/exp25); a timed window must not start inside that
            time_launches(fn, args.settle)
            results[v].append(time_launches(fn, args.steps))
        if args.yardstick:
            def cp(k):
                sets[k % nsets][3].copy_(sets[k % nsets][2])
            time_launches(cp, 5)
            yard["copy(out<-in, 2x100MB)"].append(time_launches(cp, args.steps))

            def ew(k):
                g, gu, i, o = sets[k % nsets]
                torch.addcmul(i, i, gu.unsqueeze(-1), out=o)
            time_launches(ew, 5)
            yard["elementwise(out=in*a+b, in 133MB out 100MB)"].append(time_launches(ew, args.steps))

    print(f"\n{desc}; {nsets} rotating sets; algorithmic {abytes / 1e6:.1f} MB/launch")
    table = []
    for v in variants:
        t = results[v]
        med = statistics.median(t)
        print(f"variant {v:>4d} {names[v]:42s} median {med:7.2f} us  min {min(t):7.2f} us  "
              f"-> {abytes / med / 1e3:7.1f} GB/s ({abytes / med / 1e3 / 8000 * 100:4.1f}% of 8 TB/s)  "
              f"{B * H * W / med:9.0f} MP/s   all: {[round(x, 1) for x in t]}")
        table.append({"variant": v, "name": names[v], "median_us": med, "min_us": min(t), "all_us": t,
                      "max_abs_err_vs_generic": errs[v]})
    if args.yardstick:
        vol = {"copy(out<-in, 2x100MB)": 2 * 4 * B * H * W * 3,
               "elementwise(out=in*a+b, in 133MB out 100MB)": 4 * B * H * W * 7}
        for k, t in yard.items():
            med = statistics.median(t)
            print(f"yardstick {k}: median {med:7.2f} us -> {vol[k] / med / 1e3:7.1f} GB/s")

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"workload": desc, "algorithmic_bytes": abytes, "table": table}, f)


if __name__ == "__main__":
    main()
