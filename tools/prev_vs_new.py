#!/usr/bin/env python3
"""Interleaved timing of the gradient (and forward) entry points of TWO builds of the library in one process:
the tree's libhdrnet_amd.so against a previous build given with --prev (e.g. built from the last commit in a
scratch worktree and copied to tools/exp/prev/libhdrnet_amd_prev.so -- *.so files are git-ignored but travel
to the GPU box).  Box-to-box spread is ~5 %, run-to-run drift 1-2 %: a kernel change smaller than that can
only be measured like this.

    python tools/prev_vs_new.py --prev tools/exp/prev/libhdrnet_amd_prev.so [--workload 4k] [--rounds 7]
                                [--cases fwd,nn,u8nn,u16nn] [--order new,prev]

Per case: each build's median and min - max over the rounds, and whether the new median lies inside the previous build's
range.  --order says which build runs first in every round; a difference that changes sign with it is the run order's.

--coeff: the coefficient network's training step (forward + gradient through the C ABI, with and without batch norm,
through the first entry points and their ..._wide twins) instead of the slice-apply entry points:

    --coeff bits     both builds on the same seeded network, input and cotangent: the output, every gradient and, with
                     batch norm, the running statistics after three steps, compared byte for byte (exit status 1 on a
                     difference)
    --coeff times    alternating windows of steps on the default network; per case the medians and whether the new one
                     exceeds the previous build's by more than that build's own spread over its rounds
    --coeff trace --only new|prev
                     the same cases, COEFF_TRACE_STEPS steps each, for one build: to be run under
                     rocprofv3 --kernel-trace --stats --output-format csv
    --coeff report --traces PREV_kernel_trace.csv NEW_kernel_trace.csv
                     from two such traces: per case the mean time per launch of the fully connected layers' training
                     kernels, and whether a step's ordered (kernel, grid) list is the same (needs no GPU)
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import CACHE_BYTES, WORKLOADS  # noqa: E402
from hdrnet_amd import _lib  # noqa: E402


def bind(path):
    lib = ctypes.CDLL(path)
    tables = (_lib.SIGNATURES, _lib.TRAIN_SIGNATURES, _lib.COEFF_BN_SIGNATURES, _lib.COEFF_WIDE_SIGNATURES,
              _lib.PYRAMID_IO_SIGNATURES)
    for name, (res, args) in ((n, sig) for table in tables for n, sig in table.items()):
        try:
            fn = getattr(lib, name)
        except AttributeError:
            continue  # an older build may lack newer entry points
        fn.restype, fn.argtypes = res, args
    return lib


COEFF_TINY = dict(net_input_size=64, spatial_bin=8)
# (hyper-parameters, batches): the smallest shapes at which each piece of the training step can differ between two builds
COEFF_BITS = [
    (COEFF_TINY, (1, 2, 8, 9, 16, 17, 32)),                # either side of every image-count instance of the fc kernels
    (dict(COEFF_TINY, channel_multiplier=2), (8, 16)),     # fc1 has 512 outputs: two 256-output chunks
    (dict(COEFF_TINY, luma_bins=4), (3, 12)),              # fc3 with 32 outputs: partial workgroups
    ({}, (4, 16)),                                         # the default network
]
COEFF_TIMES = [(4, False), (8, False), (16, True)]         # default network: (batch, through the ..._wide entry points)
COEFF_TRACE_STEPS = 40
COEFF_FC_KERNELS = ("coeff_fc_bwd", "coeff_bn_fc_bwd", "coeff_bn_fc")


def coeff_net(params, bn):
    """The coefficient network of a seeded model, every bias, beta and running statistic off its initial value."""
    from hdrnet_amd import models
    torch.manual_seed(21)
    net = models.HDRNetPointwiseNNGuide(dict(batch_norm=bn, **params)).coefficients
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if p.dim() == 1 and "bn.weight" not in name:
                p.copy_(0.2 * torch.randn(p.shape, generator=g))
        for name, b in net.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(0.3 * torch.randn(b.shape, generator=g))
            elif name.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=g))
    return net.to("cuda:0").train()


def coeff_step(libs, net, bn, wide, low, dc):
    """({build: a function that runs one forward + gradient of `net` through that build's C ABI}, the tensors they write:
    the output, every gradient, the running statistics).  The builds share every buffer: where an allocation lies moves a
    step's time by more than the builds differ."""
    from hdrnet_amd import hdrnet_ops as ops
    B, w = low.shape[0], "_wide" if wide else ""
    ps, stats = net._train_params_bn() if bn else (net._train_params(), None)
    n_splat = len(net.splat)
    desc = ops._live_net_bn(net.hyper, net.n_out, net.n_in, ps, n_splat, stats, 1e-3, 1e-3)
    grads = [torch.full_like(p, float("nan")) for p in ps]
    gr = ops._coeff_fill(_lib.CoeffNetBnGrads() if bn else _lib.CoeffNetGrads(), n_splat, grads, bn)
    if bn:
        names = (f"hdrnet_coefficients_bn{w}_workspace_bytes", f"hdrnet_coefficients_bn_train{w}_f32",
                 f"hdrnet_coefficients_bn_grad{w}_workspace_bytes", f"hdrnet_coefficients_bn_grad{w}_f32")
    else:
        names = ("hdrnet_coefficients_workspace_bytes", "hdrnet_coefficients_f32",
                 f"hdrnet_coefficients_grad{w}_workspace_bytes", f"hdrnet_coefficients_grad{w}_f32")
    sizes = {(getattr(lib, names[0])(ctypes.byref(desc), B), getattr(lib, names[2])(ctypes.byref(desc), B))
             for lib in libs.values()}
    assert len(sizes) == 1, ("the builds' workspaces differ", sizes)
    (fbytes, bbytes), = sizes
    assert fbytes > 0 and bbytes > 0, (names, B)
    fws = torch.full((fbytes,), 0xA5, dtype=torch.uint8, device=low.device)
    bws = torch.full((bbytes,), 0xA5, dtype=torch.uint8, device=low.device)
    sb = net.hyper["spatial_bin"]
    out = torch.full((B, sb, sb, net.gd, net.n_out, net.n_in), float("nan"), device=low.device)
    stream = torch.cuda.current_stream(low.device).cuda_stream

    def bound(lib):
        fwd, bwd = getattr(lib, names[1]), getattr(lib, names[3])

        def step():
            if fwd(low.data_ptr(), ctypes.byref(desc), out.data_ptr(), B, fws.data_ptr(), fbytes, stream):
                raise RuntimeError(lib.hdrnet_last_error().decode())
            if bwd(low.data_ptr(), ctypes.byref(desc), fws.data_ptr(), dc.data_ptr(), ctypes.byref(gr), B, bws.data_ptr(),
                   bbytes, stream):
                raise RuntimeError(lib.hdrnet_last_error().decode())

        step.keep = (desc, gr, ps, stats)  # the structs hold raw addresses
        return step

    return {which: bound(lib) for which, lib in libs.items()}, [out, *grads, *(t for st in stats or () for t in st)]


def coeff_data(net, B):
    g = torch.Generator(device="cuda:0").manual_seed(5)
    N, sb = net.hyper["net_input_size"], net.hyper["spatial_bin"]
    low = torch.rand((B, N, N, 3), device="cuda:0", generator=g)
    dc = torch.randn((B, sb, sb, net.gd, net.n_out, net.n_in), device="cuda:0", generator=g)
    return low, dc


def coeff_bits(libs):
    bad = 0
    for params, batches in COEFF_BITS:
        for B in batches:
            for bn in (False, True):
                for wide in (False, True):
                    if (bn and B < 2) or (not wide and B > 8):
                        continue
                    got = {}
                    for which, lib in libs.items():
                        net = coeff_net(params, bn)
                        low, dc = coeff_data(net, B)
                        steps, results = coeff_step({which: lib}, net, bn, wide, low, dc)
                        for _ in range(3):
                            steps[which]()
                        torch.cuda.synchronize()
                        assert not any(bool(torch.isnan(t).any()) for t in results), "an element was not written"
                        got[which] = [t.cpu().view(torch.int32) for t in results]  # bits: the sign of a zero counts
                    diff = [i for i, (a, b) in enumerate(zip(got["prev"], got["new"])) if not torch.equal(a, b)]
                    bad += bool(diff)
                    print(f"{params or 'default'} B={B} {'bn' if bn else 'plain'} {'wide' if wide else 'first'}: "
                          f"{len(got['new'])} tensors, " + (f"DIFFERENT: results {diff}" if diff else "equal"), flush=True)
    print("coefficient training, bits:", "ALL EQUAL" if not bad else f"{bad} CASES DIFFER")
    return 1 if bad else 0


def coeff_cases(libs):
    """The timed cases on the default network: (label, {build: step function})."""
    for B, wide in COEFF_TIMES:
        for bn in (False, True):
            net = coeff_net({}, bn)
            steps, _ = coeff_step(libs, net, bn, wide, *coeff_data(net, B))
            yield f"B={B} {'bn' if bn else 'plain'} {'wide' if wide else 'first'}", steps


def coeff_window(step, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def coeff_times(libs, rounds):
    worse = 0
    print("case                 prev median (min .. max) us    new median (min .. max) us   new - prev   prev spread")
    for label, steps in coeff_cases(libs):
        n = max(50, int(0.3e6 / coeff_window(steps["prev"], 50)))  # a window of ~0.3 s
        res = {"prev": [], "new": []}
        for r in range(rounds):
            for w in (("prev", "new"), ("new", "prev"))[r % 2]:  # the second of a pair measured 0.3-0.5 us slower: take turns
                coeff_window(steps[w], 20)
                res[w].append(coeff_window(steps[w], n))
        mp, mn = statistics.median(res["prev"]), statistics.median(res["new"])
        spread = max(res["prev"]) - min(res["prev"])
        ok = mn - mp <= spread
        worse += not ok
        print(f"{label:20s} {mp:8.1f} ({min(res['prev']):7.1f} .. {max(res['prev']):7.1f})   {mn:8.1f} "
              f"({min(res['new']):7.1f} .. {max(res['new']):7.1f})   {mn - mp:+8.1f}   {spread:8.1f}   "
              f"{'ok' if ok else 'SLOWER'}   ({n} steps a window, {rounds} rounds)", flush=True)
    return 1 if worse else 0


def coeff_trace(libs, which):
    for _, steps in coeff_cases({which: libs[which]}):
        for _ in range(COEFF_TRACE_STEPS):
            steps[which]()
        torch.cuda.synchronize()


def coeff_report(prev_csv, new_csv):
    import csv
    import re

    def short(n):
        n = re.sub(r"void |\(anonymous namespace\)::|hdrnet_amd::|\(.*$", "", n)
        # one name for a fully connected kernel whether the build calls it coeff_fc_bwd / coeff_fc_bwd_wide<16> or
        # coeff_fc_bwd<8> / coeff_fc_bwd<16>
        return re.sub(r"^(coeff_(?:bn_)?fc(?:_bwd)?)<8>$", r"\1", n.replace("_wide<", "<"))

    def cases(path):
        rows = [r for r in csv.DictReader(open(path)) if "coeff_" in r["Kernel_Name"]]
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        starts = [i for i, r in enumerate(rows) if "coeff_conv_first" in r["Kernel_Name"]]  # the first launch of a step
        assert len(starts) == 2 * len(COEFF_TIMES) * COEFF_TRACE_STEPS, len(starts)
        starts.append(len(rows))
        out = []
        for c in range(2 * len(COEFF_TIMES)):
            lo, hi = starts[c * COEFF_TRACE_STEPS], starts[(c + 1) * COEFF_TRACE_STEPS]
            mean = {}
            for k in COEFF_FC_KERNELS:
                d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[lo:hi]
                     if re.sub(r"[<(].*$", "", short(r["Kernel_Name"])).replace("_wide", "") == k]
                mean[k] = (sum(d) / len(d), len(d) // COEFF_TRACE_STEPS) if d else None
            last = rows[starts[(c + 1) * COEFF_TRACE_STEPS - 1]:hi]
            out.append((mean, [(short(r["Kernel_Name"]), r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"]) for r in last]))
        return out

    prev, new = cases(prev_csv), cases(new_csv)
    labels = [f"B={B} {'bn' if bn else 'plain'}" for B, _ in COEFF_TIMES for bn in (False, True)]
    for label, (mp, lp), (mn, ln) in zip(labels, prev, new):
        same = lp == ln
        print(f"{label:12s} {len(ln)} launches a step, ordered (kernel, grid) list {'the same' if same else 'DIFFERENT'}")
        if not same:
            for a, b in zip(lp, ln):
                if a != b:
                    print("     ", a, "->", b)
        for k in COEFF_FC_KERNELS:
            if mn[k]:
                print(f"    {k:16s} {mn[k][1]} launches a step: prev {mp[k][0]:6.2f} us   new {mn[k][0]:6.2f} us per launch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prev")
    ap.add_argument("--workload", default="4k", choices=sorted(WORKLOADS))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--cases", default="fwd,all,gg,g,v,slice_fwd,slice_bwd")
    ap.add_argument("--order", default="prev,new", choices=["prev,new", "new,prev"], help="which build runs first in a round")
    ap.add_argument("--nsets", type=int, default=0, help="buffer sets to rotate over (default: enough to exceed the "
                    "Infinity Cache; 1 = cache-resident, for telling memory time from issue time)")
    ap.add_argument("--coeff", choices=["bits", "times", "trace", "report"],
                    help="the coefficient network's training step (see the top of the file)")
    ap.add_argument("--only", choices=["new", "prev"], help="--coeff trace: the build to run")
    ap.add_argument("--traces", nargs=2, metavar="CSV", help="--coeff report: the previous and the new build's kernel traces")
    args = ap.parse_args()
    if args.coeff == "report":
        return coeff_report(*args.traces)
    if not args.prev:
        ap.error("--prev is required")
    dev = torch.device("cuda:0")
    libs = {"new": _lib.load(), "prev": bind(os.path.abspath(args.prev))}
    if args.coeff == "bits":
        return coeff_bits(libs)
    if args.coeff == "times":
        return coeff_times(libs, args.rounds)
    if args.coeff == "trace":
        return coeff_trace(libs, args.only)
    B, H, W, GH, GW, GD, desc = WORKLOADS[args.workload]
    Cin, Cout, C = 3, 3, 12
    npx = B * H * W
    nsets = args.nsets or max(3, -(-int(CACHE_BYTES * 1.5) // (4 * npx * 11)))
    gen = torch.Generator(device=dev).manual_seed(1)
    S = [dict(grid=torch.rand((B, GH, GW, GD, C), device=dev, generator=gen),
              guide=torch.rand((B, H, W), device=dev, generator=gen),
              inp=torch.rand((B, H, W, Cin), device=dev, generator=gen),
              dout=torch.randn((B, H, W, Cout), device=dev, generator=gen),
              out=torch.empty((B, H, W, Cout), device=dev),
              dgrid=torch.empty((B, GH, GW, GD, C), device=dev),
              dguide=torch.empty((B, H, W), device=dev),
              dinput=torch.empty((B, H, W, Cin), device=dev)) for _ in range(nsets)]
    sl = [dict(dout=torch.randn((B, H, W, C), device=dev, generator=gen),
               out=torch.empty((B, H, W, C), device=dev)) for _ in range(2)]
    conv1 = (torch.randn((16, Cin + 1), device=dev, generator=gen) * 0.8).contiguous()
    conv2 = (torch.randn((17,), device=dev, generator=gen) * 0.5).contiguous()
    ccm = (torch.eye(3, 4, device=dev) + 0.2 * torch.randn((3, 4), device=dev, generator=gen)).contiguous()
    shifts = (torch.linspace(0, 1, 17, device=dev)[:16, None].repeat(1, 3)
              + 0.01 * torch.randn((16, 3), device=dev, generator=gen)).contiguous()
    slopes = (0.3 * torch.randn((16, 3), device=dev, generator=gen)).contiguous()
    slopes[0] += 1.0
    mix = torch.tensor([0.4, 0.35, 0.25, 0.02], device=dev)
    u8 = [dict(inp=torch.randint(0, 256, (B, H, W, 3), device=dev, dtype=torch.uint8),
               out=torch.empty((B, H, W, 3), device=dev, dtype=torch.uint8)) for _ in range(nsets)]
    u16 = [torch.randint(0, 65536, (B, H, W, 3), device=dev, dtype=torch.int32).to(torch.uint16) for _ in range(nsets)]
    coarse = [torch.randn((B, H // 2, W // 2, 3), device=dev, generator=gen) for _ in range(nsets)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    # The guide-network / curves-guide cases call each build the way its round's models did: a build with the round-5
    # prepare-once helpers gets the guide network's PRESCALED parameters (HDRNET_GUIDE_RELU_PRESCALED: the same bits) and
    # the curves guide's PREPARED tables (the same guide to 1e-6); older builds the exported arrays.
    prepared = {}
    for k, lib in libs.items():
        if hasattr(lib, "hdrnet_guide_nn_prescale_f32") and hasattr(lib, "hdrnet_curves_guide_prepare_f32"):
            p1, p2 = torch.empty_like(conv1), torch.empty_like(conv2)
            assert lib.hdrnet_guide_nn_prescale_f32(conv1.data_ptr(), conv2.data_ptr(), 16, 3, 65536.0, p1.data_ptr(),
                                                    p2.data_ptr(), stream) == 0
            nb = lib.hdrnet_curves_guide_prepared_bytes(3)
            cp = torch.empty((nb // 4,), device=dev)
            if lib.hdrnet_version() >= 241:
                usable = ctypes.c_int(0)
                assert lib.hdrnet_curves_guide_prepare_f32(shifts.data_ptr(), slopes.data_ptr(), 16, 3, cp.data_ptr(), nb,
                                                           ctypes.byref(usable), stream) == 0 and usable.value == 1
            else:  # a mid-round build: the set-up call did not report usability yet (the kernels read the ok word themselves)
                fn = lib.hdrnet_curves_guide_prepare_f32
                fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                               ctypes.c_void_p]
                assert fn(shifts.data_ptr(), slopes.data_ptr(), 16, 3, cp.data_ptr(), nb, stream) == 0
            prepared[k] = (p1, p2, cp)
    ws, ws2 = {}, {}
    for k, lib in libs.items():
        n = lib.hdrnet_bilateral_slice_apply_grad_workspace_bytes(B, H, W, GH, GW, GD, Cin, Cout, 1)
        ws[k] = torch.empty((max(n, 16),), dtype=torch.uint8, device=dev)
        n2 = lib.hdrnet_bilateral_slice_grad_workspace_bytes(B, H, W, GH, GW, GD, C)
        ws2[k] = torch.empty((max(n2, 16),), dtype=torch.uint8, device=dev)

    def make(case, which):
        lib = libs[which]
        prep = prepared.get(which)
        nn1, nn2 = (prep[0], prep[1]) if prep else (conv1, conv2)
        nnflags = _lib.GUIDE_SIGMOID_FAST | (_lib.GUIDE_RELU_PRESCALED if prep else 0)

        def chk(rc):
            if rc:
                raise RuntimeError(lib.hdrnet_last_error().decode())

        if case == "fwd":
            def fn(k):
                s = S[k % nsets]
                chk(lib.hdrnet_bilateral_slice_apply_f32(s["grid"].data_ptr(), s["guide"].data_ptr(), s["inp"].data_ptr(),
                                                         s["out"].data_ptr(), B, H, W, GH, GW, GD, Cin, Cout, 1, stream))
            return fn
        if case == "slice_fwd":
            def fn(k):
                s, t = S[k % nsets], sl[k % 2]
                chk(lib.hdrnet_bilateral_slice_f32(s["grid"].data_ptr(), s["guide"].data_ptr(), t["out"].data_ptr(),
                                                   B, H, W, GH, GW, GD, C, stream))
            return fn
        if case == "slice_bwd":
            def fn(k):
                s, t = S[k % nsets], sl[k % 2]
                chk(lib.hdrnet_bilateral_slice_grad_f32(s["grid"].data_ptr(), s["guide"].data_ptr(), t["dout"].data_ptr(),
                                                        s["dgrid"].data_ptr(), s["dguide"].data_ptr(), B, H, W, GH, GW, GD,
                                                        C, ws2[which].data_ptr(), ws2[which].numel(), stream))
            return fn
        if case == "nn":  # guide network fused into the forward
            def fn(k):
                s = S[k % nsets]
                # (a build with the ..._ex twin chooses its sigmoid by flag; older builds: fast when guide_out is NULL)
                if hasattr(lib, "hdrnet_bilateral_slice_apply_nnguide_f32_ex"):
                    chk(lib.hdrnet_bilateral_slice_apply_nnguide_f32_ex(
                        s["grid"].data_ptr(), s["inp"].data_ptr(), nn1.data_ptr(), nn2.data_ptr(), s["out"].data_ptr(),
                        None, B, H, W, GH, GW, GD, Cin, Cout, 1, 16, nnflags, stream))
                    return
                chk(lib.hdrnet_bilateral_slice_apply_nnguide_f32(
                    s["grid"].data_ptr(), s["inp"].data_ptr(), conv1.data_ptr(), conv2.data_ptr(), s["out"].data_ptr(),
                    None, B, H, W, GH, GW, GD, Cin, Cout, 1, 16, stream))
            return fn
        if case in ("u8", "u8nn"):  # u8 in -> (guide map | guide network) -> u8 out
            nn = case == "u8nn"

            def fn(k):
                s, t = S[k % nsets], u8[k % nsets]
                if hasattr(lib, "hdrnet_bilateral_slice_apply_io_ex"):
                    chk(lib.hdrnet_bilateral_slice_apply_io_ex(
                        s["grid"].data_ptr(), None if nn else s["guide"].data_ptr(), t["inp"].data_ptr(), t["out"].data_ptr(),
                        B, H, W, GH, GW, GD, 3, 3, 1, 1, 255.0, 1, nn1.data_ptr() if nn else None,
                        nn2.data_ptr() if nn else None, 16 if nn else 0, None, nnflags if nn else 0, stream))
                    return
                chk(lib.hdrnet_bilateral_slice_apply_io(
                    s["grid"].data_ptr(), None if nn else s["guide"].data_ptr(), t["inp"].data_ptr(), t["out"].data_ptr(),
                    B, H, W, GH, GW, GD, 3, 3, 1, 1, 255.0, 1, conv1.data_ptr() if nn else None,
                    conv2.data_ptr() if nn else None, 16 if nn else 0, None, stream))
            return fn
        if case == "u16nn":  # u16 in -> guide network -> f32 out
            def fn(k):
                s = S[k % nsets]
                chk(lib.hdrnet_bilateral_slice_apply_io_ex(
                    s["grid"].data_ptr(), None, u16[k % nsets].data_ptr(), s["out"].data_ptr(), B, H, W, GH, GW, GD, 3, 3, 1,
                    2, 65535.0, 0, nn1.data_ptr(), nn2.data_ptr(), 16, None, nnflags, stream))
            return fn
        if case in ("curves", "u8curves"):  # curves guide fused: f32 -> f32, u8 -> u8
            u = case == "u8curves"

            def fn(k):
                s, t = S[k % nsets], u8[k % nsets]
                if prep:
                    chk(lib.hdrnet_bilateral_slice_apply_io_curves_prepared(
                        s["grid"].data_ptr(), (t if u else s)["inp"].data_ptr(), (t if u else s)["out"].data_ptr(),
                        B, H, W, GH, GW, GD, 3, 3, 1, 1 if u else 0, 255.0 if u else 1.0, 1 if u else 0,
                        ccm.data_ptr(), shifts.data_ptr(), slopes.data_ptr(), mix.data_ptr(), 16, prep[2].data_ptr(), None, stream))
                    return
                chk(lib.hdrnet_bilateral_slice_apply_io_curves(
                    s["grid"].data_ptr(), (t if u else s)["inp"].data_ptr(), (t if u else s)["out"].data_ptr(),
                    B, H, W, GH, GW, GD, 3, 3, 1, 1 if u else 0, 255.0 if u else 1.0, 1 if u else 0,
                    ccm.data_ptr(), shifts.data_ptr(), slopes.data_ptr(), mix.data_ptr(), 16, None, stream))
            return fn
        if case in ("upadd", "nnupadd"):  # one pyramid level: (guide map | guide network) + apply + up-add of the coarser level
            nn = case == "nnupadd"

            def fn(k):
                s = S[k % nsets]
                if hasattr(lib, "hdrnet_bilateral_slice_apply_upadd_f32_ex"):
                    chk(lib.hdrnet_bilateral_slice_apply_upadd_f32_ex(
                        s["grid"].data_ptr(), None if nn else s["guide"].data_ptr(), s["inp"].data_ptr(),
                        coarse[k % nsets].data_ptr(), H // 2, W // 2, s["out"].data_ptr(), B, H, W, GH, GW, GD, 3, 3, 1,
                        nn1.data_ptr() if nn else None, nn2.data_ptr() if nn else None, 16 if nn else 0, nnflags if nn else 0,
                        stream))
                    return
                chk(lib.hdrnet_bilateral_slice_apply_upadd_f32(
                    s["grid"].data_ptr(), None if nn else s["guide"].data_ptr(), s["inp"].data_ptr(), coarse[k % nsets].data_ptr(),
                    H // 2, W // 2, s["out"].data_ptr(), B, H, W, GH, GW, GD, 3, 3, 1, conv1.data_ptr() if nn else None,
                    conv2.data_ptr() if nn else None, 16 if nn else 0, stream))
            return fn
        dg, dgu, di = {"all": (1, 1, 1), "gg": (1, 1, 0), "g": (1, 0, 0), "v": (0, 1, 1)}[case]

        def fn(k):
            s = S[k % nsets]
            chk(lib.hdrnet_bilateral_slice_apply_grad_f32(
                s["grid"].data_ptr(), s["guide"].data_ptr(), s["inp"].data_ptr(), s["dout"].data_ptr(),
                s["dgrid"].data_ptr() if dg else None, s["dguide"].data_ptr() if dgu else None,
                s["dinput"].data_ptr() if di else None, B, H, W, GH, GW, GD, Cin, Cout, 1,
                ws[which].data_ptr(), ws[which].numel(), stream))
        return fn

    def time_launches(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(n):
            fn(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n

    print(f"{desc}; prev = {args.prev}")
    for case in args.cases.split(","):
        fns = {w: make(case, w) for w in ("prev", "new")}
        # same results?  (the new build against the previous one; gradients are deterministic in both)
        outs = {}
        for w in ("prev", "new"):
            for t in ("out", "dgrid", "dguide", "dinput"):
                S[0][t].fill_(0)
            fns[w](0)
            torch.cuda.synchronize()
            outs[w] = [S[0][t].clone() for t in ("out", "dgrid", "dguide", "dinput")]
        diff = max(float((a - b).abs().max()) for a, b in zip(outs["prev"], outs["new"]))
        res = {"prev": [], "new": []}
        for _ in range(args.rounds):
            for w in args.order.split(","):
                time_launches(fns[w], 20)
                res[w].append(time_launches(fns[w], args.steps))
        mp, mn = statistics.median(res["prev"]), statistics.median(res["new"])
        lo, hi = min(res["prev"]), max(res["prev"])
        where = "inside prev's range" if lo <= mn <= hi else f"{mn - hi:+.2f} us beyond prev's max" if mn > hi else f"{mn - lo:+.2f} us below prev's min"
        print(f"{case:10s} prev {mp:7.2f} us ({lo:7.2f} - {hi:7.2f})   new {mn:7.2f} us ({min(res['new']):7.2f} - {max(res['new']):7.2f})   "
              f"new / prev = {mn / mp:.3f}   new median {where}   max|new - prev| = {diff:.2e}")


if __name__ == "__main__":
    sys.exit(main())
