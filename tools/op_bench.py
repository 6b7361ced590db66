#!/usr/bin/env python3
"""Times every entry point of the C-ABI on one MI355X (HIP events, rotating buffer sets).

    python tools/op_bench.py [--workload 4k|1080p|hdrp|refbench|prep|metrics|pyramid_io|pixel_formats|yuv|yuv_planar|yuv_chroma|u16_out|pyramid_yuv|yuv_packed] [--steps 50] [--json out.json] [--tools] [--ragged]

`hdrp` = BASELINE config #5 per GPU (4000x3000, grid 32x32x8x12; also the uint16 / 32767 -> f32 wire
format of hdrnet/data_pipeline.py:267-274); `refbench` = the reference's own micro-benchmark shape
(hdrnet/hdrnet_ops_jax_tf2_test.py:56-65: batch 4, guide 4 x 1024 x 768 (h x w), grid 16 x 12 x 8 (gh x gw x gd), 2 channels, BilateralSlice,
10 burn-in + 100 timed iterations there); `prep` = sample preparation (hdrnet_prepare_batch at 4 x 1080p from u8 and from
u16 / 32767 + u8, hdrnet_lowres_input of a 4K u8 frame), each interleaved round by round with the stock-torch chain
index -> flip -> rot90 -> crop -> .float() / wl -> nearest resize; `prep --ragged` instead times the same u8 batch from a
packed set of images of mixed extents (hdrnet_prepare_batch_ragged) against the uniform call, interleaved; `metrics` =
the training step's loss at 4 x 1080p three ways, interleaved: l2_loss with its gradient, l2_loss + metrics.psnr, and
metrics.Monitor (loss, PSNR and both moving averages from csrc/loss_psnr.hip); `pyramid_io` = the pyramid model frame in,
frame out at 4K and 1080p, u8 -> u8 and u16 / 32767 -> f32: FrameInference over process_wire against the chain a caller had
before it (frame.float() / wl -> FrameInference over process -> quantise), alternating in one process; `pixel_formats` =
HDRNetPointwiseNNGuide on BGRA u8 frames at 4K and 1080p: a hipGraph of process(..., pixel_format="bgra") against a hipGraph
of the chain a caller wrote before it (index-select to RGB -> process -> flip + cat alpha), alternating, and beside it the
fused kernel alone, BGRA u8 -> u8 against RGB u8 -> u8; `yuv` = HDRNetPointwiseNNGuide on NV12 surfaces at 4K and 1080p: a
hipGraph of process_yuv(..., out="nv12") against a hipGraph of the stock chain (planes -> repeat_interleave -> affine + clamp
-> process -> affine -> 2 x 2 mean -> quantise), alternating, and beside it the fused kernel alone, NV12 -> NV12 and NV12 ->
u8 RGB against RGB u8 -> u8; `u16_out` = 16-bit output (include/hdrnet_amd_u16_out.h): a hipGraph of process(u16 -> u16 at
32767) against a hipGraph of the chain a caller had before it (process -> float32, clamp * wl, .to(uint16)) at 4000x3000,
4K and 1080p, process_yuv(P010 -> P010) against the stock encode chain at 4K, and the kernel alone, u16 -> u16 against
u16 -> f32 at 4000x3000, all alternating; `yuv_planar` = planar surfaces (include/hdrnet_amd_yuv_planar.h):
HDRNetPointwiseNNGuide on I420 uint8 planes at 4K and 1080p, a hipGraph of process_yuv_planar(..., out="planar") against a
hipGraph of the chain a caller had before it (interleave U, V -> process_yuv(out="nv12") -> split the chroma), the same
pair for yuv420p10le (the chain shifts by 6 each way around P010), and the fused kernel alone at 4K, I420 -> I420 against
NV12 -> NV12, all alternating; `yuv_chroma` = 4:2:2 / 4:4:4 surfaces (include/hdrnet_amd_yuv_chroma.h): a hipGraph of
process_yuv_planar(..., chroma=..., out="planar") against a hipGraph of the stock chain (replicate chroma -> affine + clamp
-> process -> affine -> footprint mean -> quantise) for yuv422p10le and yuv444p at 4K and 1080p, and the fused kernel alone at
4K, yuv422p -> yuv422p and yuv444p -> yuv444p against NV12 -> NV12, all alternating; `pyramid_yuv` = HDRNetGaussianPyrNN on
decoder surfaces (include/hdrnet_amd_pyramid_yuv.h): a hipGraph of process_wire_yuv, NV12 -> NV12 and P010 -> P010 at 4K and
1080p, against a hipGraph of yuv_to_rgb -> process -> stock encode, and the finest level's kernel alone at 4K against its RGB
sibling, all alternating; `yuv_packed` = packed 4:2:2 surfaces (include/hdrnet_amd_yuv_packed.h): a hipGraph of
process_yuv_packed(..., out="packed"), yuy2 -> yuy2 and y210 -> y210 at 4K and 1080p, against a hipGraph of the chain a caller
had before it (strided de-interleave -> process_yuv(chroma="422") -> re-interleave), and the fused kernel alone at 4K against
its NV16 / P210 sibling, all alternating.  --tools loads the tools build and adds the un-fused
gradient kernels (variant 3 of the gradient entry points) for A/B.

Reports per-launch microseconds and algorithmic GB/s (SURVEY.md section 8d byte counts):
  apply fwd   4*[HW(1+Cin+Cout) + grid]
  apply bwd   reads grid, guide, input, dout; writes dgrid, dguide, dinput
  slice fwd   4*[HW(1+C) + grid]
  slice bwd   reads grid, guide, dout (C ch); writes dgrid, dguide
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import CACHE_BYTES, WORKLOADS  # noqa: E402
from hdrnet_amd import _lib  # noqa: E402


def timeit(fn, steps, rounds=5):
    out = []
    for _ in range(rounds):
        for k in range(3):
            fn(k)
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(steps):
            fn(k)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / steps)
    return statistics.median(out), min(out)


def smooth_guide(dev, gen, B, H, W):
    """Luminance-like guide: a low-pass ramp + 2 % noise (the form of bench.make_sets(smooth_guide=True))."""
    yy = torch.linspace(0, 1, H, device=dev)[:, None]
    xx = torch.linspace(0, 1, W, device=dev)[None, :]
    base = 0.5 + 0.25 * torch.sin(6.28318 * (xx * 1.5 + yy)) + 0.2 * (xx - 0.5)
    return (base[None] + 0.02 * torch.rand((B, H, W), device=dev, generator=gen)).clamp(0, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="4k")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--json", default=None)
    ap.add_argument("--tools", action="store_true")
    ap.add_argument("--luma-bins", type=int, default=None, help="override the grid depth GD (hdrnet/bin/train.py:235)")
    ap.add_argument("--smooth-guide", action="store_true",
                    help="an image-like guide (bench.make_sets' low-pass ramp + 2 %% noise) instead of U[0, 1)")
    ap.add_argument("--ragged", action="store_true",
                    help="with --workload prep: hdrnet_prepare_batch_ragged against hdrnet_prepare_batch, interleaved")
    ap.add_argument("--only", default=None, help="comma-separated substrings: run only the ops whose name contains one")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load_tools() if args.tools else _lib.load()
    lib.hdrnet_enable_kernel_names(1)
    if args.workload == "refbench":
        return refbench(lib, dev, args)
    if args.workload == "prep":
        return prep_ragged(dev, args) if args.ragged else prep(dev, args)
    if args.workload == "metrics":
        return metrics_monitor(dev, args)
    if args.workload == "pyramid_io":
        return pyramid_io(dev, args)
    if args.workload == "pixel_formats":
        return pixel_formats(lib, dev, args)
    if args.workload == "yuv":
        return yuv_surfaces(lib, dev, args)
    if args.workload == "u16_out":
        return u16_out(lib, dev, args)
    if args.workload == "yuv_planar":
        return yuv_planar(lib, dev, args)
    if args.workload == "yuv_chroma":
        return yuv_chroma(lib, dev, args)
    if args.workload == "pyramid_yuv":
        return pyramid_yuv(lib, dev, args)
    if args.workload == "yuv_packed":
        return yuv_packed(lib, dev, args)
    B, H, W, GH, GW, GD, desc = WORKLOADS[args.workload]
    if args.luma_bins:
        desc = desc.replace(f"x{GD}x12", f"x{args.luma_bins}x12")
        GD = args.luma_bins
    if args.smooth_guide:
        desc += ", smooth (image-like) guide"
    Cin, Cout, C = 3, 3, 12
    npx = B * H * W
    gridb = 4 * B * GH * GW * GD * C
    # enough buffer sets that even the op with the smallest footprint per set -- the forward, 28 B/px -- cycles through
    # 1.5 x the Infinity Cache (bench.py's rule; until round 6 the count was taken from the backward's 44 B/px, which at
    # 1080p left the forward 290 MB for a 256-MB cache and read 10.9 us where bench.py's seven sets read 11.6-12.0)
    nsets = max(3, -(-int(CACHE_BYTES * 1.5) // (4 * npx * 7)))
    gen = torch.Generator(device=dev).manual_seed(1)
    S = []
    for _ in range(nsets):
        S.append(dict(
            grid=torch.rand((B, GH, GW, GD, C), device=dev, generator=gen),
            guide=smooth_guide(dev, gen, B, H, W) if args.smooth_guide else torch.rand((B, H, W), device=dev, generator=gen),
            inp=torch.rand((B, H, W, Cin), device=dev, generator=gen),
            dout=torch.randn((B, H, W, Cout), device=dev, generator=gen),
            out=torch.empty((B, H, W, Cout), device=dev),
            dgrid=torch.empty((B, GH, GW, GD, C), device=dev),
            dguide=torch.empty((B, H, W), device=dev),
            dinput=torch.empty((B, H, W, Cin), device=dev)))
    # the un-fused slice moves 4*C B/px: two sets suffice to exceed the cache
    sl = [dict(dout=torch.randn((B, H, W, C), device=dev, generator=gen),
               out=torch.empty((B, H, W, C), device=dev)) for _ in range(2)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    wsb = lib.hdrnet_bilateral_slice_apply_grad_workspace_bytes(B, H, W, GH, GW, GD, Cin, Cout, 1)
    ws = torch.empty((max(wsb, 16),), dtype=torch.uint8, device=dev)
    wsb2 = lib.hdrnet_bilateral_slice_grad_workspace_bytes(B, H, W, GH, GW, GD, C)
    ws2 = torch.empty((max(wsb2, 16),), dtype=torch.uint8, device=dev)

    def chk(rc):
        if rc:
            raise RuntimeError(lib.hdrnet_last_error().decode())

    def apply_fwd(k):
        s = S[k % nsets]
        chk(lib.hdrnet_bilateral_slice_apply_f32(s["grid"].data_ptr(), s["guide"].data_ptr(), s["inp"].data_ptr(),
                                                 s["out"].data_ptr(), B, H, W, GH, GW, GD, Cin, Cout, 1, stream))

    conv1 = (torch.randn((16, Cin + 1), device=dev, generator=gen) * 0.8).contiguous()
    conv2 = (torch.randn((17,), device=dev, generator=gen) * 0.5).contiguous()

    FAST = _lib.GUIDE_SIGMOID_FAST  # the inference lines: the models' explicit choice (HDRNET_GUIDE_SIGMOID_FAST)
    # ... and the guide network's parameters in their PRESCALED form (HDRNET_GUIDE_RELU_PRESCALED, what the models' inference
    # passes since round 5: the same guide bit for bit); `pre=False` lines time the exported layout
    PRE = _lib.GUIDE_RELU_PRESCALED
    pconv1, pconv2 = torch.empty_like(conv1), torch.empty_like(conv2)
    chk(lib.hdrnet_guide_nn_prescale_f32(conv1.data_ptr(), conv2.data_ptr(), 16, 3, 65536.0, pconv1.data_ptr(),
                                         pconv2.data_ptr(), stream))

    def nnp(pre):
        return (pconv1.data_ptr(), pconv2.data_ptr(), FAST | PRE) if pre else (conv1.data_ptr(), conv2.data_ptr(), FAST)

    def apply_fwd_nnguide(k, pre=True):
        s = S[k % nsets]
        c1, c2, fl = nnp(pre)
        chk(lib.hdrnet_bilateral_slice_apply_nnguide_f32_ex(
            s["grid"].data_ptr(), s["inp"].data_ptr(), c1, c2, s["out"].data_ptr(),
            None, B, H, W, GH, GW, GD, Cin, Cout, 1, 16, fl, stream))

    u8 = [dict(inp=torch.randint(0, 256, (B, H, W, 3), device=dev, dtype=torch.uint8),
               out=torch.empty((B, H, W, 3), device=dev, dtype=torch.uint8)) for _ in range(nsets)]

    def apply_io_u8(k, nn=True, pre=True):
        s, t = S[k % nsets], u8[k % nsets]
        c1, c2, fl = nnp(pre)
        chk(lib.hdrnet_bilateral_slice_apply_io_ex(
            s["grid"].data_ptr(), None if nn else s["guide"].data_ptr(), t["inp"].data_ptr(), t["out"].data_ptr(),
            B, H, W, GH, GW, GD, 3, 3, 1, 1, 255.0, 1, c1 if nn else None,
            c2 if nn else None, 16 if nn else 0, None, fl if nn else 0, stream))

    ccm = torch.cat([torch.eye(3, device=dev), torch.zeros((3, 1), device=dev)], 1) + 0.1 * torch.randn((3, 4), device=dev, generator=gen)
    shifts = torch.linspace(0, 1, 17, device=dev)[:-1, None].repeat(1, 3).contiguous()
    slopes = (0.2 * torch.randn((16, 3), device=dev, generator=gen)).contiguous()
    mixv = torch.tensor([0.4, 0.35, 0.25, 0.0], device=dev)

    # the curves' lookup tables prepared once per parameter set (hdrnet_curves_guide_prepare_f32; what the models' inference
    # passes since round 5); `pre=False` lines time the exported arrays alone (every workgroup sorts the knots itself)
    nprep = lib.hdrnet_curves_guide_prepared_bytes(3)
    cprep = torch.empty((nprep // 4,), device=dev)
    import ctypes
    usable = ctypes.c_int(0)
    chk(lib.hdrnet_curves_guide_prepare_f32(shifts.data_ptr(), slopes.data_ptr(), 16, 3, cprep.data_ptr(), nprep,
                                            ctypes.byref(usable), stream))
    assert usable.value == 1, "the bench's equidistant knots fit the cell tables"

    def apply_io_curves(k, u8io=True, pre=True):
        s, t = S[k % nsets], u8[k % nsets]
        chk(lib.hdrnet_bilateral_slice_apply_io_curves_prepared(
            s["grid"].data_ptr(), (t["inp"] if u8io else s["inp"]).data_ptr(), (t["out"] if u8io else s["out"]).data_ptr(),
            B, H, W, GH, GW, GD, 3, 3, 1, 1 if u8io else 0, 255.0 if u8io else 1.0, 1 if u8io else 0,
            ccm.data_ptr(), shifts.data_ptr(), slopes.data_ptr(), mixv.data_ptr(), 16, cprep.data_ptr() if pre else None,
            None, stream))

    coarse = [torch.randn((B, H // 2, W // 2, 3), device=dev, generator=gen) for _ in range(nsets)]
    half = [torch.empty((B, H // 2, W // 2, 3), device=dev) for _ in range(nsets)]

    def apply_upadd(k, nn=True, pre=True):
        s = S[k % nsets]
        c1, c2, fl = nnp(pre)
        chk(lib.hdrnet_bilateral_slice_apply_upadd_f32_ex(
            s["grid"].data_ptr(), None if nn else s["guide"].data_ptr(), s["inp"].data_ptr(),
            coarse[k % nsets].data_ptr(), H // 2, W // 2, s["out"].data_ptr(), B, H, W, GH, GW, GD, 3, 3, 1,
            c1 if nn else None, c2 if nn else None, 16 if nn else 0, fl if nn else 0,
            stream))

    def resize_half(k):
        chk(lib.hdrnet_resize_bilinear_f32(S[k % nsets]["inp"].data_ptr(), half[k % nsets].data_ptr(),
                                           B, H, W, H // 2, W // 2, 3, stream))

    def apply_bwd(k, dg=True, dgu=True, di=True, variant=0):
        s = S[k % nsets]
        chk(lib.hdrnet_bilateral_slice_apply_grad_f32_ex(
            s["grid"].data_ptr(), s["guide"].data_ptr(), s["inp"].data_ptr(), s["dout"].data_ptr(),
            s["dgrid"].data_ptr() if dg else None, s["dguide"].data_ptr() if dgu else None,
            s["dinput"].data_ptr() if di else None, B, H, W, GH, GW, GD, Cin, Cout, 1,
            ws.data_ptr(), wsb, _lib.KERNEL_AUTO | (variant << 8), stream))

    u16 = None
    if args.workload == "hdrp":
        u16 = [torch.randint(0, 32768, (B, H, W, 3), device=dev, dtype=torch.int32).to(torch.uint16)
               for _ in range(nsets)]

    def apply_io_u16(k):
        s = S[k % nsets]
        chk(lib.hdrnet_bilateral_slice_apply_io(
            s["grid"].data_ptr(), s["guide"].data_ptr(), u16[k % nsets].data_ptr(), s["out"].data_ptr(),
            B, H, W, GH, GW, GD, 3, 3, 1, 2, 32767.0, 0, None, None, 0, None, stream))

    def slice_fwd(k):
        s, t = S[k % nsets], sl[k % 2]
        chk(lib.hdrnet_bilateral_slice_f32(s["grid"].data_ptr(), s["guide"].data_ptr(), t["out"].data_ptr(),
                                           B, H, W, GH, GW, GD, C, stream))

    def slice_bwd(k):
        s, t = S[k % nsets], sl[k % 2]
        chk(lib.hdrnet_bilateral_slice_grad_f32(s["grid"].data_ptr(), s["guide"].data_ptr(), t["dout"].data_ptr(),
                                                s["dgrid"].data_ptr(), s["dguide"].data_ptr(),
                                                B, H, W, GH, GW, GD, C, ws2.data_ptr(), wsb2, stream))

    rows = []

    only = [t.strip() for t in args.only.split(",")] if args.only else None

    def run(name, fn, nbytes):
        if only and not any(t in name for t in only):
            return
        fn(0)
        torch.cuda.synchronize()
        kern = lib.hdrnet_last_kernel().decode()
        med, mn = timeit(fn, args.steps)
        rows.append(dict(op=name, kernel=kern, us=round(med, 2), us_min=round(mn, 2),
                         algorithmic_MB=round(nbytes / 1e6, 1), GBps=round(nbytes / med / 1e3, 1),
                         hbm_frac=round(nbytes / med / 1e3 / 8000, 4), MPps=round(npx / med, 0)))
        print(f"{name:28s} {kern:40s} {med:8.2f} us (min {mn:7.2f})  {nbytes / 1e6:7.1f} MB  "
              f"{nbytes / med / 1e3:7.1f} GB/s  {nbytes / med / 1e3 / 80:5.1f}% of 8 TB/s")

    print(f"{desc}; {nsets} rotating sets; workspace apply-grad {wsb / 1e6:.1f} MB")
    for k in range(1500):  # pre-roll: ~60 ms of launches take the device out of the idle power state
        apply_fwd(k)
    torch.cuda.synchronize()
    run("apply fwd", apply_fwd, 4 * npx * (1 + Cin + Cout) + gridb)
    if u16 is not None:
        run("u16 / 32767 + guide map -> apply -> f32", apply_io_u16, npx * (4 + 6 + 12) + gridb)
    run("guide-NN(16) + apply fwd fused", apply_fwd_nnguide, 4 * npx * (Cin + Cout) + gridb)
    run("... exported layout (no prescale)", lambda k: apply_fwd_nnguide(k, pre=False), 4 * npx * (Cin + Cout) + gridb)
    run("u8 -> guide-NN + apply -> u8", apply_io_u8, npx * 6 + gridb)
    run("... exported layout (no prescale)", lambda k: apply_io_u8(k, pre=False), npx * 6 + gridb)
    run("u8 + guide map -> apply -> u8", lambda k: apply_io_u8(k, nn=False), npx * 10 + gridb)
    run("curves guide + apply fwd fused", lambda k: apply_io_curves(k, u8io=False), 4 * npx * (Cin + Cout) + gridb)
    run("... exported arrays only (no prepared tables)", lambda k: apply_io_curves(k, u8io=False, pre=False),
        4 * npx * (Cin + Cout) + gridb)
    run("u8 -> curves guide + apply -> u8", apply_io_curves, npx * 6 + gridb)
    run("... exported arrays only (no prepared tables)", lambda k: apply_io_curves(k, pre=False), npx * 6 + gridb)
    run("apply + up-add of coarse level", lambda k: apply_upadd(k, nn=False),
        4 * npx * (1 + Cin + Cout) + gridb + 4 * npx * 3 // 4)
    run("guide-NN + apply + up-add", apply_upadd, 4 * npx * (Cin + Cout) + gridb + 4 * npx * 3 // 4)
    run("... exported layout (no prescale)", lambda k: apply_upadd(k, pre=False),
        4 * npx * (Cin + Cout) + gridb + 4 * npx * 3 // 4)
    run("resize bilinear 4K -> 1080p", resize_half, 4 * npx * 3 + 4 * npx * 3 // 4)
    run("apply bwd (all three)", apply_bwd, 4 * npx * (1 + Cin + Cout) + 4 * npx * (1 + Cin) + 2 * gridb)
    run("apply bwd dguide+dinput", lambda k: apply_bwd(k, dg=False), 4 * npx * (1 + Cin + Cout) + 4 * npx * (1 + Cin) + gridb)
    run("apply bwd dgrid only", lambda k: apply_bwd(k, dgu=False, di=False), 4 * npx * (1 + Cin + Cout) + gridb)
    run("apply bwd dgrid+dguide", lambda k: apply_bwd(k, di=False), 4 * npx * (1 + Cin + Cout) + 4 * npx + 2 * gridb)
    if args.tools:
        run("apply bwd (all three), un-fused kernels", lambda k: apply_bwd(k, variant=3),
            4 * npx * (1 + Cin + Cout) + 4 * npx * (1 + Cin) + 2 * gridb)
    run("slice fwd", slice_fwd, 4 * npx * (1 + C) + gridb)
    run("slice bwd (both)", slice_bwd, 4 * npx * (1 + C) + 4 * npx + 2 * gridb)
    if args.json:
        json.dump(dict(workload=desc, rows=rows), open(args.json, "w"), indent=1)


def refbench(lib, dev, args):
    """BilateralSlice at the reference's micro-benchmark shape, its iteration counts."""
    B, H, W, GH, GW, GD, C = 4, 1024, 768, 16, 12, 8, 2  # guide (4, 1024, 768), grid (4, 16, 12, 8, 2)
    gen = torch.Generator(device=dev).manual_seed(1)
    nsets = 16  # 4 * 768 * 1024 * (1 + 2) * 4 B = 37.7 MB per set
    S = [dict(grid=torch.rand((B, GH, GW, GD, C), device=dev, generator=gen),
              guide=torch.rand((B, H, W), device=dev, generator=gen),
              out=torch.empty((B, H, W, C), device=dev)) for _ in range(nsets)]
    stream = torch.cuda.current_stream(dev).cuda_stream

    def slice_fwd(k):
        s = S[k % nsets]
        rc = lib.hdrnet_bilateral_slice_f32(s["grid"].data_ptr(), s["guide"].data_ptr(), s["out"].data_ptr(),
                                            B, H, W, GH, GW, GD, C, stream)
        if rc:
            raise RuntimeError(lib.hdrnet_last_error().decode())

    slice_fwd(0)
    torch.cuda.synchronize()
    kern = lib.hdrnet_last_kernel().decode()
    for k in range(10):  # the reference's burn-in
        slice_fwd(k)
    med, mn = timeit(slice_fwd, 100, rounds=5)
    nbytes = 4 * B * (H * W * (1 + C) + GH * GW * GD * C)
    print(f"BilateralSlice fwd, reference micro-benchmark shape (batch {B}, {W}x{H}, grid {GW}x{GH}x{GD}x{C}); "
          f"{nsets} rotating sets\n{'slice fwd':28s} {kern:40s} {med:8.2f} us (min {mn:7.2f})  {nbytes / 1e6:7.1f} MB  "
          f"{nbytes / med / 1e3:7.1f} GB/s  {nbytes / med / 1e3 / 80:5.1f}% of 8 TB/s   {B * H * W / med:9.0f} MP/s")
    if args.json:
        json.dump(dict(workload="refbench", rows=[dict(op="slice fwd", kernel=kern, us=round(med, 2), us_min=round(mn, 2),
                                                       GBps=round(nbytes / med / 1e3, 1))]), open(args.json, "w"), indent=1)


def prep(dev, args):
    """hdrnet_prepare_batch / hdrnet_lowres_input against the stock-torch chain a user would write today, interleaved
    (kernel round, torch round, kernel round, ...) after a pre-roll, medians of 5 rounds each."""
    from hdrnet_amd import data
    B, H, W, n, N, S = 4, 1080, 1920, 256, 8, 2048
    gen = torch.Generator(device=dev).manual_seed(1)
    src8 = torch.randint(0, 256, (N, S, S, 3), device=dev, dtype=torch.uint8, generator=gen)
    tgt8 = torch.randint(0, 256, (N, S, S, 3), device=dev, dtype=torch.uint8, generator=gen)
    src16 = torch.randint(0, 32768, (N, S, S, 3), device=dev, dtype=torch.int32, generator=gen).to(torch.uint16)
    outs = [(torch.empty((B, n, n, 3), device=dev), torch.empty((B, H, W, 3), device=dev), torch.empty((B, H, W, 3), device=dev))
            for _ in range(2)]
    ry, rx = S - H, S - W  # square sources: the same room after an odd turn

    def table(geos):  # one record per sample: (flip_lr, flip_ud, rot90), different sources, offsets off every alignment
        return torch.tensor([[(3 * b + 1) % N, flr, fud, rot, (37 * b + 5) % (ry + 1), (11 * b + 3) % (rx + 1), 0, 0]
                             for b, (flr, fud, rot) in enumerate(geos)], dtype=torch.int32)

    cases = {"identity geometry": table([(0, 0, 0)] * 4), "flips + even turns": table([(1, 0, 0), (0, 1, 2), (1, 1, 0), (0, 0, 2)]),
             "mixed, odd turns included": table([(0, 0, 1), (1, 0, 3), (0, 1, 2), (1, 1, 1)]), "odd turns only": table([(0, 0, 1), (1, 0, 3), (0, 1, 3), (1, 1, 1)])}
    sy = torch.tensor(H, dtype=torch.float32) / torch.tensor(n, dtype=torch.float32)
    sx = torch.tensor(W, dtype=torch.float32) / torch.tensor(n, dtype=torch.float32)
    ar = torch.arange(n, dtype=torch.float32)
    ys = torch.clamp((ar * sy).floor().long(), max=H - 1).to(dev)
    xs = torch.clamp((ar * sx).floor().long(), max=W - 1).to(dev)

    def as_float(t):
        return t.view(torch.uint16).float() if t.dtype == torch.int16 else t.float()

    def chain(src, tgt, wl_in, wl_tg, ops, out):
        low, full, target = out
        for b, (idx, flr, fud, rot, cy, cx, _, _) in enumerate(ops):
            for s_all, wl, dst in ((src, wl_in, full), (tgt, wl_tg, target)):
                s = s_all[idx]
                if s.dtype == torch.uint16:
                    s = s.view(torch.int16)  # flips / rot90 of the same bits where uint16 has no kernel
                if flr:
                    s = s.flip(1)
                if fud:
                    s = s.flip(0)
                if rot:
                    s = torch.rot90(s, rot, (0, 1))
                torch.div(as_float(s[cy:cy + H, cx:cx + W]), wl, out=dst[b])
            low[b] = full[b].index_select(0, ys).index_select(1, xs)

    rows = []

    def ab(name, kernel, torch_chain, nbytes):
        for k in range(400):  # pre-roll (~60 ms of launches)
            kernel(k)
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(5):
            a.append(timeit(kernel, args.steps, rounds=1)[0])
            b.append(timeit(torch_chain, max(3, args.steps // 5), rounds=1)[0])
        ka, tb = statistics.median(a), statistics.median(b)
        rows.append(dict(op=name, us=round(ka, 2), us_torch_chain=round(tb, 2), algorithmic_MB=round(nbytes / 1e6, 1),
                         GBps=round(nbytes / ka / 1e3, 1), hbm_frac=round(nbytes / ka / 1e3 / 8000, 4)))
        print(f"{name:46s} kernel {ka:8.2f} us = {nbytes / ka / 1e3:7.1f} GB/s ({nbytes / ka / 1e3 / 80:5.1f}% of 8 TB/s)   "
              f"torch chain {tb:9.2f} us ({nbytes / tb / 1e3 / 80:5.1f}%)   x{tb / ka:6.1f}   {nbytes / 1e6:6.1f} MB")

    print(f"sample preparation: {B} x {H} x {W} crops of {N} sources of {S} x {S}, net_input_size {n}")
    for fmt, (src, tgt, wl_in, wl_tg) in {"u8 / 255 + u8 / 255": (src8, tgt8, 255.0, 255.0),
                                          "u16 / 32767 + u8 / 255": (src16, tgt8, 32767.0, 255.0)}.items():
        nbytes = B * H * W * 3 * (src.element_size() + tgt.element_size() + 8) + B * n * n * 3 * (4 + src.element_size())
        for cname, ops in cases.items():
            dtab, ltab = ops.to(dev), ops.tolist()
            ab(f"prepare_batch {fmt}, {cname}",
               lambda k: data.prepare_batch(src, tgt, dtab, (H, W), n, wl_in, wl_tg, out=outs[k % 2]),
               lambda k: chain(src, tgt, wl_in, wl_tg, ltab, outs[k % 2]), nbytes)
    FH, FW = 2160, 3840
    frames = [torch.randint(0, 256, (1, FH, FW, 3), device=dev, dtype=torch.uint8, generator=gen) for _ in range(12)]
    lows = [torch.empty((1, n, n, 3), device=dev) for _ in range(2)]
    ar = torch.arange(n, dtype=torch.float32)
    fy = torch.clamp((ar * (torch.tensor(FH, dtype=torch.float32) / n)).floor().long(), max=FH - 1).to(dev)
    fx = torch.clamp((ar * (torch.tensor(FW, dtype=torch.float32) / n)).floor().long(), max=FW - 1).to(dev)

    def low_chain(k):
        torch.div(frames[k % 12][0].index_select(0, fy).index_select(1, fx).float(), 255.0, out=lows[k % 2][0])

    ab("lowres_input 4K u8", lambda k: data.lowres_input(frames[k % 12], n, out=lows[k % 2]), low_chain, n * n * 3 * (4 + 1))
    if args.json:
        json.dump(dict(workload="prep", rows=rows), open(args.json, "w"), indent=1)


def prep_ragged(dev, args):
    """hdrnet_prepare_batch_ragged from a packed set of u8 photographs of mixed extents against hdrnet_prepare_batch from
    8 sources of 2048 x 2048: the same batch (4 crops of 1080 x 1920, the same records, u8 / 255 in and out, n = 256),
    interleaved (uniform round, ragged round, ...) after a pre-roll; per case the median of the rounds and their spread.
    A third column runs the ragged entry point on the UNIFORM call's own 8 x 2048 x 2048 sources, packed: same bytes at the
    same pitch, so it separates the cost of the descriptor read from the effect of other images and row pitches."""
    from hdrnet_amd import data
    B, H, W, n, N, S, rounds = 4, 1080, 1920, 256, 8, 2048, 7
    sizes = [(2048, 2048), (2160, 3840), (3840, 2160), (2048, 2731), (2731, 2049), (2049, 2051), (3000, 2000), (2000, 3000)]
    gen = torch.Generator(device=dev).manual_seed(1)
    src8 = torch.randint(0, 256, (N, S, S, 3), device=dev, dtype=torch.uint8, generator=gen)
    tgt8 = torch.randint(0, 256, (N, S, S, 3), device=dev, dtype=torch.uint8, generator=gen)
    flat_in, images = data.pack_images([torch.randint(0, 256, (h, w, 3), device=dev, dtype=torch.uint8, generator=gen)
                                        for h, w in sizes])
    flat_tg, _ = data.pack_images([torch.randint(0, 256, (h, w, 3), device=dev, dtype=torch.uint8, generator=gen)
                                   for h, w in sizes])
    outs = [(torch.empty((B, n, n, 3), device=dev), torch.empty((B, H, W, 3), device=dev), torch.empty((B, H, W, 3), device=dev))
            for _ in range(2)]

    def table(geos):  # prep()'s records: they fit every image of `sizes` under every turn as well
        return torch.tensor([[(3 * b + 1) % N, flr, fud, rot, 37 * b + 5, 11 * b + 3, 0, 0]
                             for b, (flr, fud, rot) in enumerate(geos)], dtype=torch.int32)

    cases = {"identity geometry": table([(0, 0, 0)] * 4), "flips + even turns": table([(1, 0, 0), (0, 1, 2), (1, 1, 0), (0, 0, 2)]),
             "mixed, odd turns included": table([(0, 0, 1), (1, 0, 3), (0, 1, 2), (1, 1, 1)]), "odd turns only": table([(0, 0, 1), (1, 0, 3), (0, 1, 3), (1, 1, 1)])}
    nbytes = B * H * W * 3 * (1 + 1 + 8) + B * n * n * 3 * (4 + 1)
    dimages = images.to(dev)
    same_images = data.pack_images([src8[0]] * N)[1].to(dev)  # src8 / tgt8 flattened ARE the packed 2048 x 2048 set
    rows = []
    print(f"sample preparation, u8 / 255 + u8 / 255: {B} x {H} x {W} crops of {N} sources of {S} x {S} (uniform) and of a packed "
          f"set of {N} images of {min(sizes)} .. {max(sizes)} (ragged), net_input_size {n}; {rounds} interleaved rounds of {args.steps}")
    for cname, ops in cases.items():
        data.check_ops(ops, N, (S, S), (H, W))
        data.check_ops(ops, N, images[:, 2:], (H, W))
        dtab = ops.to(dev)

        def uniform(k):
            data.prepare_batch(src8, tgt8, dtab, (H, W), n, 255.0, 255.0, out=outs[k % 2])

        def ragged(k):
            data.prepare_batch_ragged(flat_in, flat_tg, dimages, dtab, (H, W), n, 255.0, 255.0, out=outs[k % 2])

        def ragged_same(k):
            data.prepare_batch_ragged(src8.view(-1), tgt8.view(-1), same_images, dtab, (H, W), n, 255.0, 255.0, out=outs[k % 2])

        for k in range(200):  # pre-roll
            uniform(k)
            ragged(k)
            ragged_same(k)
        torch.cuda.synchronize()
        u, r, q = [], [], []
        for _ in range(rounds):
            u.append(timeit(uniform, args.steps, rounds=1)[0])
            r.append(timeit(ragged, args.steps, rounds=1)[0])
            q.append(timeit(ragged_same, args.steps, rounds=1)[0])
        mu, mr, mq = statistics.median(u), statistics.median(r), statistics.median(q)
        rows.append(dict(op=cname, us_uniform=round(mu, 2), us_uniform_min=round(min(u), 2), us_uniform_max=round(max(u), 2),
                         us_ragged=round(mr, 2), us_ragged_min=round(min(r), 2), us_ragged_max=round(max(r), 2),
                         us_ragged_same_set=round(mq, 2), us_ragged_same_set_min=round(min(q), 2), us_ragged_same_set_max=round(max(q), 2),
                         algorithmic_MB=round(nbytes / 1e6, 1), ragged_inside_uniform_spread=bool(min(u) <= mr <= max(u))))
        print(f"{cname:28s} uniform {mu:8.2f} us ({min(u):8.2f} .. {max(u):8.2f}) = {nbytes / mu / 1e3:7.1f} GB/s   "
              f"ragged {mr:8.2f} us ({min(r):8.2f} .. {max(r):8.2f}) = {nbytes / mr / 1e3:7.1f} GB/s   ragged / uniform {mr / mu:6.3f}   "
              f"ragged on the uniform set {mq:8.2f} us ({min(q):8.2f} .. {max(q):8.2f}), / uniform {mq / mu:6.3f}")
    if args.json:
        json.dump(dict(workload="prep --ragged", rows=rows), open(args.json, "w"), indent=1)


def pyramid_io(dev, args):
    """HDRNetGaussianPyrNN frame in, frame out with the wire formats: FrameInference over process_wire (the resize reads the
    wire format, the finest level converts in registers) against the chain a caller had until now -- frame.float() / wl ->
    FrameInference over process -> (255 * out.clamp(0, 1)).to(uint8) for uint8 out -- built from stock ops and the float32
    kernels only.  Per case both are warmed, then run ALTERNATING three times each in one process (baseline, new, baseline,
    ...); reported: the mean of the three and their spread.  The new path counts as faster where its mean is below the
    baseline's by more than the baseline's own spread."""
    from hdrnet_amd import models
    from hdrnet_amd.runtime import FrameInference
    torch.manual_seed(7)
    m = models.HDRNetGaussianPyrNN(dict(batch_norm=False)).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    rows = []
    for H, W in ((2160, 3840), (1080, 1920)):
        for in_dtype, wl, out_dtype in ((torch.uint8, 255.0, torch.uint8), (torch.uint16, 32767.0, torch.float32)):
            hi = 256 if in_dtype == torch.uint8 else 32768
            frames = [torch.randint(0, hi, (1, H, W, 3), device=dev, dtype=torch.int32, generator=gen).to(in_dtype)
                      for _ in range(3)]
            new = FrameInference(m, frames[0], out_dtype=out_dtype, white_level=wl)
            base = FrameInference(m, frames[0].float() / wl)

            def run_new(k):
                return new(frames[k % 3])

            def run_base(k):
                out = base(frames[k % 3].float() / wl)
                return (255 * out.clamp(0, 1)).to(torch.uint8) if out_dtype == torch.uint8 else out

            for k in range(30):  # both warmed with their shapes
                run_base(k)
                run_new(k)
            torch.cuda.synchronize()
            b, n = [], []
            for _ in range(3):
                b.append(timeit(run_base, args.steps, rounds=1)[0])
                n.append(timeit(run_new, args.steps, rounds=1)[0])
            mb, mn = statistics.mean(b), statistics.mean(n)
            spread = max(b) - min(b)
            name = f"{H}x{W} {str(in_dtype)[6:]}/{wl:g} -> {str(out_dtype)[6:]}"
            rows.append(dict(op=name, us_baseline=round(mb, 2), us_baseline_min=round(min(b), 2), us_baseline_max=round(max(b), 2),
                             us_wire=round(mn, 2), us_wire_min=round(min(n), 2), us_wire_max=round(max(n), 2),
                             faster_beyond_baseline_spread=bool(mb - mn > spread)))
            print(f"{name:36s} baseline chain {mb:8.2f} us ({min(b):8.2f} .. {max(b):8.2f})   process_wire {mn:8.2f} us "
                  f"({min(n):8.2f} .. {max(n):8.2f})   wire / baseline {mn / mb:6.3f}   "
                  f"faster by more than the baseline's spread: {mb - mn > spread}")
    if args.json:
        json.dump(dict(workload="pyramid_io", rows=rows), open(args.json, "w"), indent=1)


class _RepackChain(torch.nn.Module):
    """What a caller with a BGRA frame wrote before process() took the format: index-select to RGB (drops alpha), process,
    flip the result and put the frame's alpha back -- two stock-op passes around the fused kernels."""

    def __init__(self, model, dev):
        super().__init__()
        self.model = model
        self.register_buffer("bgr", torch.tensor([2, 1, 0], device=dev), persistent=False)

    def forward(self, frame):
        out = self.model.process(frame.index_select(3, self.bgr), out_dtype=torch.uint8)
        return torch.cat([out.index_select(3, self.bgr), frame[..., 3:]], -1)


def pixel_formats(lib, dev, args):
    """BGRA uint8 frames in, BGRA uint8 frames out through HDRNetPointwiseNNGuide at 4K and 1080p: one hipGraph of
    process(frame, uint8, pixel_format="bgra") -- the permutation in the kernels' loads and stores -- against one hipGraph of
    _RepackChain.  Both are warmed, then run ALTERNATING three times each in one process; reported: the mean of the three
    and their range.  The new path counts as faster where its mean is below the chain's by more than the chain's own
    spread.  Beside it, without a bar: the fused guide-network kernel alone, BGRA u8 -> u8 (8 bytes per pixel) against RGB
    u8 -> u8 (6), over buffer sets that together exceed the Infinity Cache, alternating the same way."""
    from hdrnet_amd import models
    from hdrnet_amd.runtime import FrameInference, GraphedInference
    torch.manual_seed(7)
    m = models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rows = []

    def alternate(run_a, run_b):
        for k in range(30):  # both warmed with their shapes
            run_a(k)
            run_b(k)
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(3):
            a.append(timeit(run_a, args.steps, rounds=1)[0])
            b.append(timeit(run_b, args.steps, rounds=1)[0])
        return a, b

    for H, W in ((2160, 3840), (1080, 1920)):
        frames = [torch.randint(0, 256, (1, H, W, 4), device=dev, dtype=torch.int32, generator=gen).to(torch.uint8)
                  for _ in range(3)]
        new = FrameInference(m, frames[0], out_dtype=torch.uint8, pixel_format="bgra")
        chain_module = _RepackChain(m, dev)
        base = GraphedInference(chain_module, [frames[0]])
        assert torch.equal(new(frames[1]), base(frames[1])), "the two paths return the same frame"
        b, n = alternate(lambda k: base(frames[k % 3]), lambda k: new(frames[k % 3]))
        mb, mn = statistics.mean(b), statistics.mean(n)
        spread = max(b) - min(b)
        name = f"{H}x{W} model, bgra u8 -> bgra u8"
        rows.append(dict(op=name, us_chain=round(mb, 2), us_chain_min=round(min(b), 2), us_chain_max=round(max(b), 2),
                         us_fused=round(mn, 2), us_fused_min=round(min(n), 2), us_fused_max=round(max(n), 2),
                         faster_beyond_chain_spread=bool(mb - mn > spread)))
        print(f"{name:40s} repack chain {mb:8.2f} us ({min(b):8.2f} .. {max(b):8.2f})   pixel_format='bgra' {mn:8.2f} us "
              f"({min(n):8.2f} .. {max(n):8.2f})   fused / chain {mn / mb:6.3f}   "
              f"faster by more than the chain's spread: {mb - mn > spread}")
        del new, base

        # the kernel alone: the same grid and guide network, frames of 4 against 3 bytes per pixel
        GH, GW, GD = 16, 16, 8
        nsets = max(3, -(-int(CACHE_BYTES * 1.5) // (H * W * 6)))
        grid = torch.rand((1, GH, GW, GD, 12), device=dev, generator=gen)
        conv1 = (torch.randn((16, 4), device=dev, generator=gen) * 0.8).contiguous()
        conv2 = (torch.randn((17,), device=dev, generator=gen) * 0.5).contiguous()
        sets = [dict(rgb=torch.randint(0, 256, (1, H, W, 3), device=dev, dtype=torch.int32, generator=gen).to(torch.uint8),
                     bgra=torch.randint(0, 256, (1, H, W, 4), device=dev, dtype=torch.int32, generator=gen).to(torch.uint8),
                     out3=torch.empty((1, H, W, 3), device=dev, dtype=torch.uint8),
                     out4=torch.empty((1, H, W, 4), device=dev, dtype=torch.uint8)) for _ in range(nsets)]

        def kernel(k, fmt):
            t = sets[k % nsets]
            src, dst = (t["bgra"], t["out4"]) if fmt else (t["rgb"], t["out3"])
            rc = lib.hdrnet_bilateral_slice_apply_io_px(grid.data_ptr(), None, src.data_ptr(), dst.data_ptr(), 1, H, W, GH, GW,
                                                        GD, 3, 3, 1, 1, 255.0, 1, conv1.data_ptr(), conv2.data_ptr(), 16, None,
                                                        _lib.GUIDE_SIGMOID_FAST, fmt, fmt, stream)
            if rc:
                raise RuntimeError(lib.hdrnet_last_error().decode())

        r, q = alternate(lambda k: kernel(k, 0), lambda k: kernel(k, 3))
        mr, mq = statistics.mean(r), statistics.mean(q)
        name = f"{H}x{W} kernel, u8 -> u8 +nnguide"
        rows.append(dict(op=name, us_rgb=round(mr, 2), us_rgb_min=round(min(r), 2), us_rgb_max=round(max(r), 2),
                         us_bgra=round(mq, 2), us_bgra_min=round(min(q), 2), us_bgra_max=round(max(q), 2)))
        print(f"{name:40s} rgb (6 B/px) {mr:8.2f} us ({min(r):8.2f} .. {max(r):8.2f})   bgra (8 B/px) {mq:8.2f} us "
              f"({min(q):8.2f} .. {max(q):8.2f})   bgra / rgb {mq / mr:6.3f}")
        del sets
    if args.json:
        json.dump(dict(workload="pixel_formats", rows=rows), open(args.json, "w"), indent=1)


class _YuvStockChain(torch.nn.Module):
    """What a caller with a decoded NV12 surface writes around process(): slice the chroma, repeat_interleave it, three
    affine ops and a clamp into a float32 RGB frame, process, and for the encoder the mirror image -- an affine to Y, U, V,
    the 2 x 2 mean of the chroma, quantise, interleave."""

    def __init__(self, model, to_rgb, from_rgb):
        super().__init__()
        self.model = model
        self.register_buffer("m_in", to_rgb[:9].reshape(3, 3).t().contiguous(), persistent=False)   # [Y U V] @ m_in -> RGB
        self.register_buffer("b_in", to_rgb[9:].contiguous(), persistent=False)
        self.register_buffer("m_out", from_rgb[:9].reshape(3, 3).t().contiguous(), persistent=False)
        self.register_buffer("b_out", from_rgb[9:].contiguous(), persistent=False)

    def forward(self, y, uv):
        B, H, W = y.shape
        c = uv.view(B, H // 2, W // 2, 2).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        yuv = torch.cat([y.unsqueeze(-1), c], -1).float()
        rgb = (yuv @ self.m_in + self.b_in).clamp_(0.0, 1.0)
        out = self.model.process(rgb).clamp_(0.0, 1.0)
        enc = out @ self.m_out
        yq = (enc[..., 0] + self.b_out[0]).clamp_(0.0, 255.0).to(torch.uint8)
        cm = enc[..., 1:].reshape(B, H // 2, 2, W // 2, 2, 2).mean(dim=(2, 4)) + self.b_out[1:]
        return yq, cm.clamp_(0.0, 255.0).to(torch.uint8).reshape(B, H // 2, W)


def yuv_surfaces(lib, dev, args):
    """NV12 uint8 surfaces in, NV12 uint8 surfaces out through HDRNetPointwiseNNGuide at 4K and 1080p: one hipGraph of
    process_yuv(y, uv, out="nv12") -- the conversions in the kernels' loads and stores -- against one hipGraph of
    _YuvStockChain.  Both are warmed, then run ALTERNATING three times each in one process; reported: the mean of the three
    and their range (device events around `steps` replays).  Beside it, without a bar: the fused guide-network kernel alone,
    NV12 -> NV12 (3 bytes per pixel) and NV12 -> u8 RGB (4.5) against RGB u8 -> u8 (6), over buffer sets that together exceed
    the Infinity Cache, alternating the same way."""
    from hdrnet_amd import models, yuv
    from hdrnet_amd.runtime import GraphedInference, YuvFrameInference
    torch.manual_seed(7)
    m = models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    to_rgb, from_rgb = (torch.from_numpy(a).to(dev) for a in yuv.yuv_coefficients("bt709", False, 8))
    rows = []

    def alternate(*runs):
        for k in range(30):  # all warmed with their shapes
            for run in runs:
                run(k)
        torch.cuda.synchronize()
        out = [[] for _ in runs]
        for _ in range(3):
            for o, run in zip(out, runs):
                o.append(timeit(run, args.steps, rounds=1)[0])
        return out

    def u8(*shape):
        return torch.randint(0, 256, shape, device=dev, dtype=torch.int32, generator=gen).to(torch.uint8)

    for H, W in ((2160, 3840), (1080, 1920)):
        surfaces = [(u8(1, H, W), u8(1, H // 2, W)) for _ in range(3)]
        new = YuvFrameInference(m, *surfaces[0], out="nv12")
        base = GraphedInference(_YuvStockChain(m, to_rgb, from_rgb), list(surfaces[0]))
        (ny, nuv), (by, buv) = new(*surfaces[1]), base(*surfaces[1])
        dy = (ny.int() - by.int()).abs()
        duv = (nuv.int() - buv.int()).abs()
        # (the chain rounds its affine ops in another order: it is a timing opponent, not the reference of the tests)
        print(f"{H}x{W}: fused vs chain, codes that differ: Y {int((dy > 0).sum())} (max {int(dy.max())}), "
              f"UV {int((duv > 0).sum())} (max {int(duv.max())}) of {dy.numel()} + {duv.numel()}")
        assert int(dy.max()) <= 1 and int(duv.max()) <= 1, "the two paths encode the same surface to within a code"
        b, n = alternate(lambda k: base(*surfaces[k % 3]), lambda k: new(*surfaces[k % 3]))
        mb, mn = statistics.mean(b), statistics.mean(n)
        spread = max(b) - min(b)
        name = f"{H}x{W} model, nv12 -> nv12"
        rows.append(dict(op=name, us_chain=round(mb, 2), us_chain_min=round(min(b), 2), us_chain_max=round(max(b), 2),
                         us_fused=round(mn, 2), us_fused_min=round(min(n), 2), us_fused_max=round(max(n), 2),
                         faster_beyond_chain_spread=bool(mb - mn > spread)))
        print(f"{name:40s} stock chain {mb:8.2f} us ({min(b):8.2f} .. {max(b):8.2f})   process_yuv {mn:8.2f} us "
              f"({min(n):8.2f} .. {max(n):8.2f})   fused / chain {mn / mb:6.3f}   "
              f"faster by more than the chain's spread: {mb - mn > spread}")
        del new, base

        # the kernel alone: the same grid and guide network over three frame layouts
        GH, GW, GD = 16, 16, 8
        nsets = max(3, -(-int(CACHE_BYTES * 1.5) // (H * W * 3)))
        grid = torch.rand((1, GH, GW, GD, 12), device=dev, generator=gen)
        conv1 = (torch.randn((16, 4), device=dev, generator=gen) * 0.8).contiguous()
        conv2 = (torch.randn((17,), device=dev, generator=gen) * 0.5).contiguous()
        sets = [dict(rgb=u8(1, H, W, 3), y=u8(1, H, W), uv=u8(1, H // 2, W),
                     out3=torch.empty((1, H, W, 3), device=dev, dtype=torch.uint8),
                     oy=torch.empty((1, H, W), device=dev, dtype=torch.uint8),
                     ouv=torch.empty((1, H // 2, W), device=dev, dtype=torch.uint8)) for _ in range(nsets)]

        def check(rc):
            if rc:
                raise RuntimeError(lib.hdrnet_last_error().decode())

        def rgb_kernel(k):
            t = sets[k % nsets]
            check(lib.hdrnet_bilateral_slice_apply_io_ex(grid.data_ptr(), None, t["rgb"].data_ptr(), t["out3"].data_ptr(), 1, H, W,
                                                         GH, GW, GD, 3, 3, 1, 1, 255.0, 1, conv1.data_ptr(), conv2.data_ptr(), 16,
                                                         None, _lib.GUIDE_SIGMOID_FAST, stream))

        def yuv_kernel(k, nv12_out):
            t = sets[k % nsets]
            out = ((2, t["oy"].data_ptr(), t["ouv"].data_ptr(), W, W, H * W, H // 2 * W, from_rgb.data_ptr()) if nv12_out
                   else (1, t["out3"].data_ptr(), None, 0, 0, 0, 0, None))
            check(lib.hdrnet_bilateral_slice_apply_io_yuv(grid.data_ptr(), None, t["y"].data_ptr(), t["uv"].data_ptr(), 1, W, W,
                                                          H * W, H // 2 * W, 1, H, W, to_rgb.data_ptr(), GH, GW, GD, 3, 3, 1,
                                                          conv1.data_ptr(), conv2.data_ptr(), 16, None,
                                                          _lib.GUIDE_SIGMOID_FAST, *out, stream))

        r, q, v = alternate(rgb_kernel, lambda k: yuv_kernel(k, True), lambda k: yuv_kernel(k, False))
        name = f"{H}x{W} kernel, +nnguide"
        row = dict(op=name)
        text = []
        for key, label, t in (("rgb_u8_u8", "rgb u8 -> u8 (6 B/px)", r), ("nv12_nv12", "nv12 -> nv12 (3 B/px)", q),
                              ("nv12_rgb_u8", "nv12 -> u8 rgb (4.5 B/px)", v)):
            row.update({f"us_{key}": round(statistics.mean(t), 2), f"us_{key}_min": round(min(t), 2),
                        f"us_{key}_max": round(max(t), 2)})
            text.append(f"{label} {statistics.mean(t):8.2f} us ({min(t):8.2f} .. {max(t):8.2f})")
        rows.append(row)
        print(f"{name:28s} " + "   ".join(text))
        del sets
    if args.json:
        json.dump(dict(workload="yuv", rows=rows), open(args.json, "w"), indent=1)


class _PyramidYuvChain(torch.nn.Module):
    """What a caller with a decoder surface and the pyramid model wrote before process_wire_yuv: hdrnet_ops.yuv_to_rgb into a
    float32 RGB frame, process (the float32 pyramid), and the stock encode half of _YuvStockChain -- an affine to Y, U, V, the
    2 x 2 mean of the chroma, quantise to ``bits`` bits (codes in the high bits of a uint16 sample), interleave."""

    def __init__(self, model, to_rgb, from_rgb, bits):
        super().__init__()
        self.model, self.bits = model, bits
        self.register_buffer("to_rgb", to_rgb, persistent=False)
        self.register_buffer("m_out", from_rgb[:9].reshape(3, 3).t().contiguous(), persistent=False)
        self.register_buffer("b_out", from_rgb[9:].contiguous(), persistent=False)

    def forward(self, y, uv):
        from hdrnet_amd import hdrnet_ops
        B, H, W = y.shape
        top = float(2 ** self.bits - 1)
        out = self.model.process(hdrnet_ops.yuv_to_rgb(y, uv, self.to_rgb)).clamp_(0.0, 1.0)
        enc = out @ self.m_out
        yq = (enc[..., 0] + self.b_out[0]).clamp_(0.0, top)
        cm = (enc[..., 1:].reshape(B, H // 2, 2, W // 2, 2, 2).mean(dim=(2, 4)) + self.b_out[1:]).clamp_(0.0, top).reshape(B, H // 2, W)
        if self.bits == 8:
            return yq.to(torch.uint8), cm.to(torch.uint8)
        sh = 16 - self.bits
        return (yq.to(torch.int32) << sh).to(torch.uint16), (cm.to(torch.int32) << sh).to(torch.uint16)


def pyramid_yuv(lib, dev, args):
    """HDRNetGaussianPyrNN on decoder surfaces at 4K and 1080p, NV12 -> NV12 and P010 -> P010: one hipGraph of
    process_wire_yuv (YuvFrameInference: the resize and the finest level read the surface, the finest level stores one)
    against one hipGraph of _PyramidYuvChain, the chain a caller had.  Both are warmed, then run ALTERNATING three times each
    in one process; reported: the mean of the three and their range (device events around `steps` replays).  Beside it,
    without a bar, at 4K: the finest level's kernel alone, nv12 -> nv12 + nnguide + upadd (3 bytes per pixel) against
    u8 -> u8 + nnguide + upadd on an RGB frame (6), over buffer sets that together exceed the Infinity Cache, alternating the
    same way."""
    from hdrnet_amd import models, yuv
    from hdrnet_amd.runtime import GraphedInference, YuvFrameInference
    torch.manual_seed(7)
    m = models.HDRNetGaussianPyrNN(dict(batch_norm=False)).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rows = []

    def alternate(*runs):
        for k in range(30):  # all warmed with their shapes
            for run in runs:
                run(k)
        torch.cuda.synchronize()
        out = [[] for _ in runs]
        for _ in range(3):
            for o, run in zip(out, runs):
                o.append(timeit(run, args.steps, rounds=1)[0])
        return out

    def samples(bits, *shape):
        t = torch.randint(0, 2 ** bits, shape, device=dev, dtype=torch.int32, generator=gen)
        return t.to(torch.uint8) if bits == 8 else (t << (16 - bits)).to(torch.uint16)

    for H, W in ((2160, 3840), (1080, 1920)):
        for bits, out in ((8, "nv12"), (10, "p010")):
            to_rgb = torch.from_numpy(yuv.yuv_coefficients("bt709", False, bits)[0]).to(dev)
            from_rgb = torch.from_numpy(yuv.yuv_encode_coefficients("bt709", False, bits)).to(dev)
            surfaces = [(samples(bits, 1, H, W), samples(bits, 1, H // 2, W)) for _ in range(3)]
            new = YuvFrameInference(m, *surfaces[0], bits=bits, out=out)
            base = GraphedInference(_PyramidYuvChain(m, to_rgb, from_rgb, bits), list(surfaces[0]))
            (ny, nuv), (by, buv) = new(*surfaces[1]), base(*surfaces[1])
            sh = 16 - bits if bits > 8 else 0
            dy = ((ny.int() >> sh) - (by.int() >> sh)).abs()
            duv = ((nuv.int() >> sh) - (buv.int() >> sh)).abs()
            # (the chain rounds its affine ops in another order: it is a timing opponent, not the reference of the tests)
            print(f"{H}x{W} {out}: fused vs chain, codes that differ: Y {int((dy > 0).sum())} (max {int(dy.max())}), "
                  f"UV {int((duv > 0).sum())} (max {int(duv.max())}) of {dy.numel()} + {duv.numel()}")
            assert int(dy.max()) <= 1 and int(duv.max()) <= 1, "the two paths encode the same surface to within a code"
            b, n = alternate(lambda k: base(*surfaces[k % 3]), lambda k: new(*surfaces[k % 3]))
            mb, mn = statistics.mean(b), statistics.mean(n)
            spread = max(b) - min(b)
            name = f"{H}x{W} pyramid model, {out} -> {out}"
            rows.append(dict(op=name, us_chain=round(mb, 2), us_chain_min=round(min(b), 2), us_chain_max=round(max(b), 2),
                             us_fused=round(mn, 2), us_fused_min=round(min(n), 2), us_fused_max=round(max(n), 2),
                             below_chain_beyond_its_spread=bool(mb - mn > spread)))
            print(f"{name:44s} chain {mb:8.2f} us ({min(b):8.2f} .. {max(b):8.2f})   process_wire_yuv {mn:8.2f} us "
                  f"({min(n):8.2f} .. {max(n):8.2f})   fused / chain {mn / mb:6.3f}   "
                  f"below the chain by more than its spread: {mb - mn > spread}")
            del new, base, surfaces

    # the finest level's kernel alone at 4K: the same grid, guide network and coarse level over two frame layouts
    H, W = 2160, 3840
    GH, GW, GD = 16, 16, 8
    nsets = max(3, -(-int(CACHE_BYTES * 1.5) // (H * W * 3)))
    to_rgb, from_rgb = (torch.from_numpy(a).to(dev) for a in yuv.yuv_coefficients("bt709", False, 8))
    grid = torch.rand((1, GH, GW, GD, 12), device=dev, generator=gen)
    conv1 = (torch.randn((16, 4), device=dev, generator=gen) * 0.8).contiguous()
    conv2 = (torch.randn((17,), device=dev, generator=gen) * 0.5).contiguous()
    coarse = (0.3 * torch.randn((1, H // 2, W // 2, 3), device=dev, generator=gen)).contiguous()
    sets = [dict(rgb=samples(8, 1, H, W, 3), y=samples(8, 1, H, W), uv=samples(8, 1, H // 2, W),
                 out3=torch.empty((1, H, W, 3), device=dev, dtype=torch.uint8),
                 oy=torch.empty((1, H, W), device=dev, dtype=torch.uint8),
                 ouv=torch.empty((1, H // 2, W), device=dev, dtype=torch.uint8)) for _ in range(nsets)]

    def check(rc):
        if rc:
            raise RuntimeError(lib.hdrnet_last_error().decode())

    def rgb_kernel(k):
        t = sets[k % nsets]
        check(lib.hdrnet_bilateral_slice_apply_upadd_io_ex(grid.data_ptr(), None, t["rgb"].data_ptr(), coarse.data_ptr(), H // 2,
                                                           W // 2, t["out3"].data_ptr(), 1, H, W, GH, GW, GD, 3, 3, 1, 1, 255.0, 1,
                                                           conv1.data_ptr(), conv2.data_ptr(), 16, _lib.GUIDE_SIGMOID_FAST, stream))

    def yuv_kernel(k):
        t = sets[k % nsets]
        check(lib.hdrnet_bilateral_slice_apply_upadd_io_yuv(grid.data_ptr(), None, t["y"].data_ptr(), t["uv"].data_ptr(), 1, W, W,
                                                            H * W, H // 2 * W, 1, H, W, to_rgb.data_ptr(), coarse.data_ptr(),
                                                            H // 2, W // 2, GH, GW, GD, 3, 3, 1, conv1.data_ptr(),
                                                            conv2.data_ptr(), 16, _lib.GUIDE_SIGMOID_FAST, 2, t["oy"].data_ptr(),
                                                            t["ouv"].data_ptr(), W, W, H * W, H // 2 * W, from_rgb.data_ptr(),
                                                            stream))

    rgb_kernel(0)
    k_rgb = lib.hdrnet_last_kernel().decode()
    yuv_kernel(0)
    k_yuv = lib.hdrnet_last_kernel().decode()
    r, q = alternate(rgb_kernel, yuv_kernel)
    name = f"{H}x{W} kernel, +nnguide+upadd"
    row = dict(op=name, kernels=[k_rgb, k_yuv])
    text = []
    for key, label, t in (("rgb_u8_u8", f"{k_rgb} (6 B/px)", r), ("nv12_nv12", f"{k_yuv} (3 B/px)", q)):
        row.update({f"us_{key}": round(statistics.mean(t), 2), f"us_{key}_min": round(min(t), 2), f"us_{key}_max": round(max(t), 2)})
        text.append(f"{label} {statistics.mean(t):8.2f} us ({min(t):8.2f} .. {max(t):8.2f})")
    rows.append(row)
    print(f"{name:36s} " + "   ".join(text))
    if args.json:
        json.dump(dict(workload="pyramid_yuv", rows=rows), open(args.json, "w"), indent=1)


class _PlanarChain(torch.nn.Module):
    """What a caller with a planar surface wrote before process_yuv_planar: interleave U and V into a new plane (10-bit:
    shift every sample up by 6 as well), process_yuv to a semi-planar surface, split the chroma again (and shift back)."""

    def __init__(self, model, bits):
        super().__init__()
        self.model, self.bits = model, bits

    def forward(self, y, u, v):
        if self.bits == 8:
            oy, ouv = self.model.process_yuv(y, torch.stack((u, v), dim=-1).flatten(2), out="nv12")
            return oy, ouv[:, :, 0::2].contiguous(), ouv[:, :, 1::2].contiguous()
        # (stock torch has neither shifts nor stack for uint16: through int32, the shift fused into the conversion's pass)
        up = lambda t: (t << 6).to(torch.uint16)  # noqa: E731
        down = lambda t: (t.int() >> 6).to(torch.uint16)  # noqa: E731
        oy, ouv = self.model.process_yuv(up(y.int()), up(torch.stack((u.int(), v.int()), dim=-1).flatten(2)), bits=10, out="p010")
        return down(oy), down(ouv[:, :, 0::2]), down(ouv[:, :, 1::2])


def yuv_planar(lib, dev, args):
    """Planar 4:2:0 surfaces through HDRNetPointwiseNNGuide at 4K and 1080p: one hipGraph of process_yuv_planar(y, u, v,
    out="planar") against one hipGraph of _PlanarChain, I420 uint8 and yuv420p10le; both warmed, then run ALTERNATING three
    times each in one process; reported: the mean of the three and their range.  Beside it, at 4K: the fused guide-network
    kernel alone, I420 -> I420 against NV12 -> NV12 (the same bytes, two narrower chroma accesses per lane each way), over
    buffer sets that together exceed the Infinity Cache, alternating the same way."""
    from hdrnet_amd import models, yuv
    from hdrnet_amd.runtime import GraphedInference, PlanarYuvFrameInference
    torch.manual_seed(7)
    m = models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rows = []

    def alternate(*runs):
        for k in range(30):  # all warmed with their shapes
            for run in runs:
                run(k)
        torch.cuda.synchronize()
        out = [[] for _ in runs]
        for _ in range(3):
            for o, run in zip(out, runs):
                o.append(timeit(run, args.steps, rounds=1)[0])
        return out

    def samples(bits, *shape):
        t = torch.randint(0, 2 ** bits, shape, device=dev, dtype=torch.int32, generator=gen)
        return t.to(torch.uint8 if bits == 8 else torch.uint16)

    for H, W in ((2160, 3840), (1080, 1920)):
        for bits, fmt in ((8, "i420"), (10, "yuv420p10le")):
            surfaces = [(samples(bits, 1, H, W), samples(bits, 1, H // 2, W // 2), samples(bits, 1, H // 2, W // 2))
                        for _ in range(3)]
            new = PlanarYuvFrameInference(m, *surfaces[0], bits=bits, out="planar")
            base = GraphedInference(_PlanarChain(m, bits), list(surfaces[0]))
            for a, b in zip(new(*surfaces[1]), base(*surfaces[1])):
                assert torch.equal(a, b), "the fused path and the chain around process_yuv give the same planes"
            b, n = alternate(lambda k: base(*surfaces[k % 3]), lambda k: new(*surfaces[k % 3]))
            mb, mn = statistics.mean(b), statistics.mean(n)
            spread = max(b) - min(b)
            name = f"{H}x{W} model, {fmt} -> {fmt}"
            rows.append(dict(op=name, us_chain=round(mb, 2), us_chain_min=round(min(b), 2), us_chain_max=round(max(b), 2),
                             us_fused=round(mn, 2), us_fused_min=round(min(n), 2), us_fused_max=round(max(n), 2),
                             faster_beyond_chain_spread=bool(mb - mn > spread)))
            print(f"{name:46s} chain {mb:8.2f} us ({min(b):8.2f} .. {max(b):8.2f})   process_yuv_planar {mn:8.2f} us "
                  f"({min(n):8.2f} .. {max(n):8.2f})   fused / chain {mn / mb:6.3f}   "
                  f"faster by more than the chain's spread: {mb - mn > spread}")
            del new, base, surfaces

    # the kernel alone at 4K: the same grid and guide network, the same samples in two surface layouts
    H, W = 2160, 3840
    GH, GW, GD = 16, 16, 8
    to_rgb, from_rgb = (torch.from_numpy(a).to(dev) for a in yuv.yuv_coefficients("bt709", False, 8))
    nsets = max(3, -(-int(CACHE_BYTES * 1.5) // (H * W * 3)))
    grid = torch.rand((1, GH, GW, GD, 12), device=dev, generator=gen)
    conv1 = (torch.randn((16, 4), device=dev, generator=gen) * 0.8).contiguous()
    conv2 = (torch.randn((17,), device=dev, generator=gen) * 0.5).contiguous()
    Hc, Wc = H // 2, W // 2
    e = lambda *shape: torch.empty(shape, device=dev, dtype=torch.uint8)  # noqa: E731
    sets = [dict(y=samples(8, 1, H, W), uv=samples(8, 1, Hc, W), u=samples(8, 1, Hc, Wc), v=samples(8, 1, Hc, Wc),
                 oy=e(1, H, W), ouv=e(1, Hc, W), ou=e(1, Hc, Wc), ov=e(1, Hc, Wc)) for _ in range(nsets)]

    def check(rc):
        if rc:
            raise RuntimeError(lib.hdrnet_last_error().decode())

    def nv12_kernel(k):
        t = sets[k % nsets]
        check(lib.hdrnet_bilateral_slice_apply_io_yuv(grid.data_ptr(), None, t["y"].data_ptr(), t["uv"].data_ptr(), 1, W, W, H * W,
                                                      Hc * W, 1, H, W, to_rgb.data_ptr(), GH, GW, GD, 3, 3, 1, conv1.data_ptr(),
                                                      conv2.data_ptr(), 16, None, _lib.GUIDE_SIGMOID_FAST, 2, t["oy"].data_ptr(),
                                                      t["ouv"].data_ptr(), W, W, H * W, Hc * W, from_rgb.data_ptr(), stream))

    def i420_kernel(k):
        t = sets[k % nsets]
        check(lib.hdrnet_bilateral_slice_apply_io_yuv_planar(
            grid.data_ptr(), None, t["y"].data_ptr(), t["u"].data_ptr(), t["v"].data_ptr(), 1, W, Wc, Wc, H * W, Hc * Wc, Hc * Wc,
            1, H, W, to_rgb.data_ptr(), GH, GW, GD, 3, 3, 1, conv1.data_ptr(), conv2.data_ptr(), 16, None,
            _lib.GUIDE_SIGMOID_FAST, 2, t["oy"].data_ptr(), t["ou"].data_ptr(), t["ov"].data_ptr(), W, Wc, Wc, H * W, Hc * Wc,
            Hc * Wc, from_rgb.data_ptr(), 8, stream))

    q, p = alternate(nv12_kernel, i420_kernel)
    name = f"{H}x{W} kernel, +nnguide"
    row = dict(op=name)
    text = []
    for key, label, t in (("nv12_nv12", "nv12 -> nv12 (3 B/px)", q), ("i420_i420", "i420 -> i420 (3 B/px)", p)):
        row.update({f"us_{key}": round(statistics.mean(t), 2), f"us_{key}_min": round(min(t), 2), f"us_{key}_max": round(max(t), 2)})
        text.append(f"{label} {statistics.mean(t):8.2f} us ({min(t):8.2f} .. {max(t):8.2f})")
    rows.append(row)
    print(f"{name:28s} " + "   ".join(text))
    if args.json:
        json.dump(dict(workload="yuv_planar", rows=rows), open(args.json, "w"), indent=1)


class _ChromaStockChain(torch.nn.Module):
    """What a caller with a planar 4:2:2 / 4:4:4 surface writes around process() today: replicate the chroma over its
    footprint, an affine and a clamp into a float32 RGB frame, process, and for the encoder the mirror image -- an affine to Y,
    U, V, the mean of the chroma over the footprint, quantise."""

    def __init__(self, model, to_rgb, from_rgb, chroma, bits):
        super().__init__()
        self.model, self.fx, self.top = model, (1 if chroma == "444" else 2), float(2 ** bits - 1)
        self.dtype = torch.uint8 if bits == 8 else torch.uint16
        self.register_buffer("m_in", to_rgb[:9].reshape(3, 3).t().contiguous(), persistent=False)   # [Y U V] @ m_in -> RGB
        self.register_buffer("b_in", to_rgb[9:].contiguous(), persistent=False)
        self.register_buffer("m_out", from_rgb[:9].reshape(3, 3).t().contiguous(), persistent=False)
        self.register_buffer("b_out", from_rgb[9:].contiguous(), persistent=False)

    def forward(self, y, u, v):
        B, H, W = y.shape
        wide = (lambda t: t.float().repeat_interleave(2, dim=2)) if self.fx == 2 else (lambda t: t.float())
        yuv = torch.stack([y.float(), wide(u), wide(v)], -1)
        rgb = (yuv @ self.m_in + self.b_in).clamp_(0.0, 1.0)
        out = self.model.process(rgb).clamp_(0.0, 1.0)
        enc = out @ self.m_out
        yq = (enc[..., 0] + self.b_out[0]).clamp_(0.0, self.top).to(self.dtype)
        cm = enc[..., 1:].reshape(B, H, W // self.fx, self.fx, 2).mean(dim=3) + self.b_out[1:]
        cq = cm.clamp_(0.0, self.top).to(self.dtype)
        return yq, cq[..., 0].contiguous(), cq[..., 1].contiguous()


def yuv_chroma(lib, dev, args):
    """4:2:2 / 4:4:4 planar surfaces (include/hdrnet_amd_yuv_chroma.h) through HDRNetPointwiseNNGuide at 4K and 1080p,
    yuv422p10le -> yuv422p10le and yuv444p -> yuv444p: one hipGraph of process_yuv_planar(y, u, v, chroma=..., out="planar")
    against one hipGraph of _ChromaStockChain; both warmed, then run ALTERNATING three times each in one process; reported:
    the mean of the three and their range.  Beside it, at 4K: the fused guide-network kernel alone, yuv422p -> yuv422p (2 + 2
    B/px) and yuv444p -> yuv444p (3 + 3 B/px) against NV12 -> NV12 (1.5 + 1.5 B/px), over buffer sets that together exceed the
    Infinity Cache, alternating the same way."""
    from hdrnet_amd import models, yuv
    from hdrnet_amd.runtime import GraphedInference, PlanarYuvFrameInference
    torch.manual_seed(7)
    m = models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rows = []

    def alternate(*runs):
        for k in range(30):  # all warmed with their shapes
            for run in runs:
                run(k)
        torch.cuda.synchronize()
        out = [[] for _ in runs]
        for _ in range(3):
            for o, run in zip(out, runs):
                o.append(timeit(run, args.steps, rounds=1)[0])
        return out

    def samples(bits, *shape):
        t = torch.randint(0, 2 ** bits, shape, device=dev, dtype=torch.int32, generator=gen)
        return t.to(torch.uint8 if bits == 8 else torch.uint16)

    for H, W in ((2160, 3840), (1080, 1920)):
        for chroma, bits, fmt in (("422", 10, "yuv422p10le"), ("444", 8, "yuv444p")):
            Wc = W if chroma == "444" else W // 2
            surfaces = [(samples(bits, 1, H, W), samples(bits, 1, H, Wc), samples(bits, 1, H, Wc)) for _ in range(3)]
            to_rgb = torch.from_numpy(yuv.yuv_coefficients("bt709", False, bits, msb_aligned=False)[0]).to(dev)
            from_rgb = torch.from_numpy(yuv.yuv_encode_coefficients("bt709", False, bits)).to(dev)
            new = PlanarYuvFrameInference(m, *surfaces[0], bits=bits, out="planar", chroma=chroma)
            base = GraphedInference(_ChromaStockChain(m, to_rgb, from_rgb, chroma, bits), list(surfaces[0]))
            worst = 0
            for a, b in zip(new(*surfaces[1]), base(*surfaces[1])):
                worst = max(worst, int((a.int() - b.int()).abs().max()))
            # (the chain rounds its affine ops in another order: it is a timing opponent, not the reference of the tests)
            print(f"{H}x{W} {fmt}: fused vs chain, largest code difference {worst}")
            assert worst <= 1, "the two paths encode the same surface to within a code"
            b, n = alternate(lambda k: base(*surfaces[k % 3]), lambda k: new(*surfaces[k % 3]))
            mb, mn = statistics.mean(b), statistics.mean(n)
            spread = max(b) - min(b)
            name = f"{H}x{W} model, {fmt} -> {fmt}"
            rows.append(dict(op=name, us_chain=round(mb, 2), us_chain_min=round(min(b), 2), us_chain_max=round(max(b), 2),
                             us_fused=round(mn, 2), us_fused_min=round(min(n), 2), us_fused_max=round(max(n), 2),
                             faster_beyond_chain_spread=bool(mb - mn > spread)))
            print(f"{name:46s} stock chain {mb:8.2f} us ({min(b):8.2f} .. {max(b):8.2f})   process_yuv_planar {mn:8.2f} us "
                  f"({min(n):8.2f} .. {max(n):8.2f})   fused / chain {mn / mb:6.3f}   "
                  f"faster by more than the chain's spread: {mb - mn > spread}")
            del new, base, surfaces

    # the kernel alone at 4K: the same grid and guide network over three surface layouts
    H, W = 2160, 3840
    GH, GW, GD = 16, 16, 8
    to_rgb, from_rgb = (torch.from_numpy(a).to(dev) for a in yuv.yuv_coefficients("bt709", False, 8))
    nsets = max(3, -(-int(CACHE_BYTES * 1.5) // (H * W * 3)))
    grid = torch.rand((1, GH, GW, GD, 12), device=dev, generator=gen)
    conv1 = (torch.randn((16, 4), device=dev, generator=gen) * 0.8).contiguous()
    conv2 = (torch.randn((17,), device=dev, generator=gen) * 0.5).contiguous()
    e = lambda *shape: torch.empty(shape, device=dev, dtype=torch.uint8)  # noqa: E731
    sets = [dict(y=samples(8, 1, H, W), uv=samples(8, 1, H // 2, W), u2=samples(8, 1, H, W // 2), v2=samples(8, 1, H, W // 2),
                 u4=samples(8, 1, H, W), v4=samples(8, 1, H, W), oy=e(1, H, W), ouv=e(1, H // 2, W), ou2=e(1, H, W // 2),
                 ov2=e(1, H, W // 2), ou4=e(1, H, W), ov4=e(1, H, W)) for _ in range(nsets)]

    def check(rc):
        if rc:
            raise RuntimeError(lib.hdrnet_last_error().decode())

    def nv12_kernel(k):
        t = sets[k % nsets]
        check(lib.hdrnet_bilateral_slice_apply_io_yuv(grid.data_ptr(), None, t["y"].data_ptr(), t["uv"].data_ptr(), 1, W, W, H * W,
                                                      H // 2 * W, 1, H, W, to_rgb.data_ptr(), GH, GW, GD, 3, 3, 1, conv1.data_ptr(),
                                                      conv2.data_ptr(), 16, None, _lib.GUIDE_SIGMOID_FAST, 2, t["oy"].data_ptr(),
                                                      t["ouv"].data_ptr(), W, W, H * W, H // 2 * W, from_rgb.data_ptr(), stream))

    def planar_kernel(k, chroma):
        t = sets[k % nsets]
        s, Wc = ("4", W) if chroma == 2 else ("2", W // 2)
        check(lib.hdrnet_bilateral_slice_apply_io_yuv_planar_chroma(
            grid.data_ptr(), None, t["y"].data_ptr(), t["u" + s].data_ptr(), t["v" + s].data_ptr(), 1, W, Wc, Wc, H * W, H * Wc,
            H * Wc, chroma, 1, H, W, to_rgb.data_ptr(), GH, GW, GD, 3, 3, 1, conv1.data_ptr(), conv2.data_ptr(), 16, None,
            _lib.GUIDE_SIGMOID_FAST, 2, t["oy"].data_ptr(), t["ou" + s].data_ptr(), t["ov" + s].data_ptr(), W, Wc, Wc, H * W,
            H * Wc, H * Wc, from_rgb.data_ptr(), 8, stream))

    q, p2, p4 = alternate(nv12_kernel, lambda k: planar_kernel(k, 1), lambda k: planar_kernel(k, 2))
    name = f"{H}x{W} kernel, +nnguide"
    row = dict(op=name)
    text = []
    for key, label, t in (("nv12_nv12", "nv12 -> nv12 (3 B/px)", q), ("i422_i422", "yuv422p -> yuv422p (4 B/px)", p2),
                          ("i444_i444", "yuv444p -> yuv444p (6 B/px)", p4)):
        row.update({f"us_{key}": round(statistics.mean(t), 2), f"us_{key}_min": round(min(t), 2), f"us_{key}_max": round(max(t), 2)})
        text.append(f"{label} {statistics.mean(t):8.2f} us ({min(t):8.2f} .. {max(t):8.2f})")
    row["i422_over_nv12"] = round(statistics.mean(p2) / statistics.mean(q), 3)
    row["i444_over_nv12"] = round(statistics.mean(p4) / statistics.mean(q), 3)
    rows.append(row)
    print(f"{name:28s} " + "   ".join(text))
    if args.json:
        json.dump(dict(workload="yuv_chroma", rows=rows), open(args.json, "w"), indent=1)


class _PackedDeinterleaveChain(torch.nn.Module):
    """What a caller with a packed 4:2:2 surface (YUY2, Y210) writes around process_yuv today: a strided de-interleave into the
    NV16 / P210 pair, process_yuv(chroma="422") with a surface out, and the strided re-interleave."""

    def __init__(self, model, bits):
        super().__init__()
        self.model, self.bits, self.out = model, bits, ("nv16" if bits == 8 else "p210")

    def forward(self, surface):
        B, H, W2 = surface.shape
        y = surface[:, :, 0::2].contiguous()
        uv = surface[:, :, 1::2].contiguous()
        oy, ouv = self.model.process_yuv(y, uv, bits=self.bits, out=self.out, chroma="422")
        out = torch.empty_like(surface)
        out[:, :, 0::2] = oy
        out[:, :, 1::2] = ouv
        return out


def yuv_packed(lib, dev, args):
    """Packed 4:2:2 surfaces (include/hdrnet_amd_yuv_packed.h) through HDRNetPointwiseNNGuide at 4K and 1080p, yuy2 -> yuy2 and
    y210 -> y210: one hipGraph of process_yuv_packed(..., out="packed") against one hipGraph of _PackedDeinterleaveChain; both
    warmed, then run ALTERNATING three times each in one process; reported: the mean of the three and their range.  Beside it,
    at 4K: the fused guide-network kernel alone, yuy2 -> yuy2 against nv16 -> nv16 and y210 -> y210 against p210 -> p210 (the
    same bytes per pixel, one plane against two), over buffer sets that together exceed the Infinity Cache, alternating the
    same way."""
    from hdrnet_amd import models, yuv
    from hdrnet_amd.runtime import GraphedInference, PackedYuvFrameInference
    torch.manual_seed(7)
    m = models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    rows = []

    def alternate(*runs):
        for k in range(30):  # all warmed with their shapes
            for run in runs:
                run(k)
        torch.cuda.synchronize()
        out = [[] for _ in runs]
        for _ in range(3):
            for o, run in zip(out, runs):
                o.append(timeit(run, args.steps, rounds=1)[0])
        return out

    def samples(bits, *shape):
        t = torch.randint(0, 2 ** bits, shape, device=dev, dtype=torch.int32, generator=gen)
        return t.to(torch.uint8) if bits == 8 else (t << (16 - bits)).to(torch.uint16)

    for H, W in ((2160, 3840), (1080, 1920)):
        for fmt, bits in (("yuy2", 8), ("y210", 10)):
            surfaces = [samples(bits, 1, H, 2 * W) for _ in range(3)]
            new = PackedYuvFrameInference(m, surfaces[0], fmt, out="packed")
            base = GraphedInference(_PackedDeinterleaveChain(m, bits), [surfaces[0]])
            assert torch.equal(new(surfaces[1]), base(surfaces[1])), "the two paths write the same surface, bit for bit"
            b, n = alternate(lambda k: base(surfaces[k % 3]), lambda k: new(surfaces[k % 3]))
            mb, mn = statistics.mean(b), statistics.mean(n)
            spread = max(b) - min(b)
            name = f"{H}x{W} model, {fmt} -> {fmt}"
            rows.append(dict(op=name, us_chain=round(mb, 2), us_chain_min=round(min(b), 2), us_chain_max=round(max(b), 2),
                             us_fused=round(mn, 2), us_fused_min=round(min(n), 2), us_fused_max=round(max(n), 2),
                             faster_beyond_chain_spread=bool(mb - mn > spread)))
            print(f"{name:40s} de-interleave chain {mb:8.2f} us ({min(b):8.2f} .. {max(b):8.2f})   process_yuv_packed {mn:8.2f} us "
                  f"({min(n):8.2f} .. {max(n):8.2f})   fused / chain {mn / mb:6.3f}   "
                  f"faster by more than the chain's spread: {mb - mn > spread}")
            del new, base, surfaces

    # the kernel alone at 4K: the same grid and guide network, one plane against the plane pair
    H, W = 2160, 3840
    GH, GW, GD = 16, 16, 8
    grid = torch.rand((1, GH, GW, GD, 12), device=dev, generator=gen)
    conv1 = (torch.randn((16, 4), device=dev, generator=gen) * 0.8).contiguous()
    conv2 = (torch.randn((17,), device=dev, generator=gen) * 0.5).contiguous()

    def check(rc):
        if rc:
            raise RuntimeError(lib.hdrnet_last_error().decode())

    for fmt, bits, semi in (("yuy2", 8, "nv16"), ("y210", 10, "p210")):
        S = 1 if bits == 8 else 2
        dt = torch.uint8 if bits == 8 else torch.uint16
        to_rgb = torch.from_numpy(yuv.yuv_coefficients("bt709", False, bits)[0]).to(dev)
        from_rgb = torch.from_numpy(yuv.yuv_encode_coefficients("bt709", False, bits)).to(dev)
        nsets = max(3, -(-int(CACHE_BYTES * 1.5) // (H * W * 4 * S)))
        e = lambda *shape: torch.empty(shape, device=dev, dtype=dt)  # noqa: E731
        sets = [dict(s=samples(bits, 1, H, 2 * W), y=samples(bits, 1, H, W), uv=samples(bits, 1, H, W), os=e(1, H, 2 * W),
                     oy=e(1, H, W), ouv=e(1, H, W)) for _ in range(nsets)]
        kind, out_bits = (2, 0) if bits == 8 else (3, bits)

        def packed_kernel(k):
            t = sets[k % nsets]
            check(lib.hdrnet_bilateral_slice_apply_io_yuv_packed(
                grid.data_ptr(), None, t["s"].data_ptr(), S, 2 * W * S, H * 2 * W * S, 0, 1, H, W, to_rgb.data_ptr(), GH, GW, GD, 3,
                3, 1, conv1.data_ptr(), conv2.data_ptr(), 16, None, _lib.GUIDE_SIGMOID_FAST, kind, t["os"].data_ptr(), 2 * W * S,
                H * 2 * W * S, from_rgb.data_ptr(), out_bits, stream))

        def semi_kernel(k):
            t = sets[k % nsets]
            check(lib.hdrnet_bilateral_slice_apply_io_yuv_chroma(
                grid.data_ptr(), None, t["y"].data_ptr(), t["uv"].data_ptr(), S, W * S, W * S, H * W * S, H * W * S, 1, 1, H, W,
                to_rgb.data_ptr(), GH, GW, GD, 3, 3, 1, conv1.data_ptr(), conv2.data_ptr(), 16, None, _lib.GUIDE_SIGMOID_FAST, kind,
                t["oy"].data_ptr(), t["ouv"].data_ptr(), W * S, W * S, H * W * S, H * W * S, from_rgb.data_ptr(), out_bits, stream))

        q, p = alternate(semi_kernel, packed_kernel)
        name = f"{H}x{W} kernel, +nnguide, {fmt} -> {fmt} against {semi} -> {semi}"
        rows.append({"op": name, "us_semi": round(statistics.mean(q), 2), "us_semi_min": round(min(q), 2),
                     "us_semi_max": round(max(q), 2), "us_packed": round(statistics.mean(p), 2), "us_packed_min": round(min(p), 2),
                     "us_packed_max": round(max(p), 2), "packed_over_semi": round(statistics.mean(p) / statistics.mean(q), 3)})
        print(f"{name:60s} {semi} {statistics.mean(q):8.2f} us ({min(q):8.2f} .. {max(q):8.2f})   {fmt} {statistics.mean(p):8.2f} us "
              f"({min(p):8.2f} .. {max(p):8.2f})   packed / semi-planar {statistics.mean(p) / statistics.mean(q):6.3f}")
        del sets
    if args.json:
        json.dump(dict(workload="yuv_packed", rows=rows), open(args.json, "w"), indent=1)


class _QuantiseChain(torch.nn.Module):
    """What a caller with a 16-bit pipeline wrote before process() stored uint16: take the float32 frame and quantise it
    with stock ops -- clamp, scale, convert: three more full-frame launches around the fused kernels."""

    def __init__(self, model, white_level):
        super().__init__()
        self.model, self.white_level = model, white_level

    def forward(self, frame):
        out = self.model.process(frame, out_dtype=torch.float32, white_level=self.white_level)
        return (out.clamp(0.0, 1.0) * self.white_level).to(torch.uint16)


class _P010StockChain(torch.nn.Module):
    """process_yuv(out="rgb") of a P010 surface, then _YuvStockChain's encode chain with 10-bit constants: an affine to
    Y, U, V, the 2 x 2 mean of the chroma, quantise to 10-bit codes, shift into the high bits, interleave."""

    def __init__(self, model, from_rgb):
        super().__init__()
        self.model = model
        self.register_buffer("m_out", from_rgb[:9].reshape(3, 3).t().contiguous(), persistent=False)
        self.register_buffer("b_out", from_rgb[9:].contiguous(), persistent=False)

    def forward(self, y, uv):
        B, H, W = y.shape
        out = self.model.process_yuv(y, uv, bits=10, out="rgb").clamp_(0.0, 1.0)
        enc = out @ self.m_out
        yq = (enc[..., 0] + self.b_out[0]).clamp_(0.0, 1023.0).to(torch.int32) << 6
        cm = enc[..., 1:].reshape(B, H // 2, 2, W // 2, 2, 2).mean(dim=(2, 4)) + self.b_out[1:]
        cq = cm.clamp_(0.0, 1023.0).to(torch.int32) << 6
        return yq.to(torch.uint16), cq.to(torch.uint16).reshape(B, H // 2, W)


def u16_out(lib, dev, args):
    """16-bit output (include/hdrnet_amd_u16_out.h) through HDRNetPointwiseNNGuide, one hipGraph each, ALTERNATING three
    times each in one process, reported as mean and range (device events around `steps` replays):
      model    4000x3000 (BASELINE config #5's frame, 32x32 grid), 4K, 1080p: process(u16 -> u16 at 32767) against
               _QuantiseChain (process -> float32, clamp * wl, .to(uint16));
      surface  4K: process_yuv(P010 -> P010) against _P010StockChain;
      kernel   4000x3000, guide map, grid 32x32x8: u16 -> u16 against its float32-store sibling u16 -> f32, over buffer sets
               that together exceed the Infinity Cache.
    The new path counts as faster where its mean is below the chain's by more than the chain's own spread."""
    from hdrnet_amd import models, yuv
    from hdrnet_amd.runtime import FrameInference, GraphedInference, YuvFrameInference
    torch.manual_seed(7)
    gen = torch.Generator(device=dev).manual_seed(1)
    stream = torch.cuda.current_stream(dev).cuda_stream
    WL = 32767.0
    rows = []

    def alternate(*runs):
        for k in range(30):  # all warmed with their shapes
            for run in runs:
                run(k)
        torch.cuda.synchronize()
        out = [[] for _ in runs]
        for _ in range(3):
            for o, run in zip(out, runs):
                o.append(timeit(run, args.steps, rounds=1)[0])
        return out

    def u16(hi, *shape):
        return torch.randint(0, hi, shape, device=dev, dtype=torch.int32, generator=gen).to(torch.uint16)

    def report(name, b, n, chain_label, new_label):
        mb, mn = statistics.mean(b), statistics.mean(n)
        spread = max(b) - min(b)
        rows.append(dict(op=name, us_chain=round(mb, 2), us_chain_min=round(min(b), 2), us_chain_max=round(max(b), 2),
                         us_fused=round(mn, 2), us_fused_min=round(min(n), 2), us_fused_max=round(max(n), 2),
                         faster_beyond_chain_spread=bool(mb - mn > spread)))
        print(f"{name:40s} {chain_label} {mb:8.2f} us ({min(b):8.2f} .. {max(b):8.2f})   {new_label} {mn:8.2f} us "
              f"({min(n):8.2f} .. {max(n):8.2f})   fused / chain {mn / mb:6.3f}   "
              f"faster by more than the chain's spread: {mb - mn > spread}")

    for H, W, spatial_bin in ((3000, 4000, 32), (2160, 3840, 16), (1080, 1920, 16)):
        torch.manual_seed(7)
        m = models.HDRNetPointwiseNNGuide(dict(batch_norm=False, spatial_bin=spatial_bin)).to(dev).eval()
        frames = [u16(int(WL) + 1, 1, H, W, 3) for _ in range(3)]
        new = FrameInference(m, frames[0], out_dtype=torch.uint16, white_level=WL)
        base = GraphedInference(_QuantiseChain(m, WL), [frames[0]])
        d = (new(frames[1]).int() - base(frames[1]).int()).abs()
        # (the chain multiplies the same float32 values by the same white level: it returns the same frame)
        assert int(d.max()) == 0, "the two paths return the same frame"
        b, n = alternate(lambda k: base(frames[k % 3]), lambda k: new(frames[k % 3]))
        report(f"{H}x{W} model, u16 -> u16 / 32767", b, n, "quantise chain", "out_dtype=uint16")
        del new, base, frames

    # the surface: P010 in, P010 out at 4K
    H, W = 2160, 3840
    torch.manual_seed(7)
    m = models.HDRNetPointwiseNNGuide(dict(batch_norm=False)).to(dev).eval()
    from_rgb = torch.from_numpy(yuv.yuv_encode_coefficients("bt709", False, 10)).to(dev)
    def p010(*shape):  # 10-bit codes in the high bits
        return (torch.randint(0, 1024, shape, device=dev, dtype=torch.int32, generator=gen) << 6).to(torch.uint16)

    surfaces = [(p010(1, H, W), p010(1, H // 2, W)) for _ in range(3)]
    new = YuvFrameInference(m, *surfaces[0], bits=10, out="p010")
    base = GraphedInference(_P010StockChain(m, from_rgb), list(surfaces[0]))
    (ny, nuv), (by, buv) = new(*surfaces[1]), base(*surfaces[1])
    dy, duv = ((ny.int() - by.int()).abs() >> 6), ((nuv.int() - buv.int()).abs() >> 6)
    # (the chain rounds its affine ops in another order: it is a timing opponent, not the reference of the tests)
    print(f"{H}x{W}: fused vs chain, codes that differ: Y {int((dy > 0).sum())} (max {int(dy.max())}), "
          f"UV {int((duv > 0).sum())} (max {int(duv.max())}) of {dy.numel()} + {duv.numel()}")
    assert int(dy.max()) <= 1 and int(duv.max()) <= 1, "the two paths encode the same surface to within a code"
    b, n = alternate(lambda k: base(*surfaces[k % 3]), lambda k: new(*surfaces[k % 3]))
    report(f"{H}x{W} model, p010 -> p010", b, n, "stock chain", "process_yuv")
    del new, base, surfaces

    # the kernel alone: config #5's frame and grid with a guide map, 6 against 12 bytes per pixel stored
    H, W, GH, GW, GD = 3000, 4000, 32, 32, 8
    nsets = max(3, -(-int(CACHE_BYTES * 1.5) // (H * W * 22)))
    grid = torch.rand((1, GH, GW, GD, 12), device=dev, generator=gen)
    sets = [dict(inp=u16(int(WL) + 1, 1, H, W, 3), guide=torch.rand((1, H, W), device=dev, generator=gen),
                 out16=torch.empty((1, H, W, 3), device=dev, dtype=torch.uint16),
                 out32=torch.empty((1, H, W, 3), device=dev, dtype=torch.float32)) for _ in range(nsets)]

    def check(rc):
        if rc:
            raise RuntimeError(lib.hdrnet_last_error().decode())

    def to_f32(k):
        t = sets[k % nsets]
        check(lib.hdrnet_bilateral_slice_apply_io_ex(grid.data_ptr(), t["guide"].data_ptr(), t["inp"].data_ptr(),
                                                     t["out32"].data_ptr(), 1, H, W, GH, GW, GD, 3, 3, 1, 2, WL, 0, None, None,
                                                     0, None, 0, stream))

    def to_u16(k):
        t = sets[k % nsets]
        check(lib.hdrnet_bilateral_slice_apply_io_px_u16(grid.data_ptr(), t["guide"].data_ptr(), t["inp"].data_ptr(),
                                                         t["out16"].data_ptr(), 1, H, W, GH, GW, GD, 3, 3, 1, 2, WL, WL, None,
                                                         None, 0, None, 0, 0, 0, stream))

    f, q = alternate(to_f32, to_u16)
    name = f"{H}x{W} kernel, u16 / 32767 in, guide map"
    rows.append(dict(op=name, us_u16_f32=round(statistics.mean(f), 2), us_u16_f32_min=round(min(f), 2),
                     us_u16_f32_max=round(max(f), 2), us_u16_u16=round(statistics.mean(q), 2), us_u16_u16_min=round(min(q), 2),
                     us_u16_u16_max=round(max(q), 2)))
    print(f"{name:40s} u16 -> f32 (12 B/px stored) {statistics.mean(f):8.2f} us ({min(f):8.2f} .. {max(f):8.2f})   "
          f"u16 -> u16 (6 B/px stored) {statistics.mean(q):8.2f} us ({min(q):8.2f} .. {max(q):8.2f})   "
          f"u16 / f32 {statistics.mean(q) / statistics.mean(f):6.3f}")
    if args.json:
        json.dump(dict(workload="u16_out", rows=rows), open(args.json, "w"), indent=1)


def metrics_monitor(dev, args):
    """What monitoring a training step costs at 4 x 1080p (config #4's batch): forward + backward of
    (a) metrics.l2_loss with its gradient, (b) the same plus metrics.psnr as a torch chain under no_grad -- the reference's
    train_op fetches both (hdrnet/bin/train.py:95-96) -- and (c) metrics.Monitor: loss, PSNR, the moving averages of both
    and the unit gradient from the two launches of csrc/loss_psnr.hip.  Interleaved (a round of each in turn) after a
    pre-roll, over three rotating pairs of tensors (600 MB: nothing is served from the cache); per case the median of
    the rounds and their spread -- once as eager calls (host work included) and once as hipGraph replays (what a
    GraphedTrainStep runs: device time alone)."""
    from hdrnet_amd import metrics
    B, H, W, rounds, sets = 4, 1080, 1920, 7, 3
    gen = torch.Generator(device=dev).manual_seed(1)
    tg = [torch.rand((B, H, W, 3), device=dev, generator=gen) for _ in range(sets)]
    pr = [torch.rand((B, H, W, 3), device=dev, generator=gen).requires_grad_(True) for _ in range(sets)]
    assert 2 * sets * tg[0].numel() * 4 > 2 * CACHE_BYTES
    one = torch.ones((), device=dev)
    monitor = metrics.Monitor()

    def a(k):
        torch.autograd.grad(metrics.l2_loss(tg[k % sets], pr[k % sets]), pr[k % sets], one)

    def b(k):
        torch.autograd.grad(metrics.l2_loss(tg[k % sets], pr[k % sets]), pr[k % sets], one)
        with torch.no_grad():
            metrics.psnr(tg[k % sets], pr[k % sets])

    def c(k):
        torch.autograd.grad(monitor(pr[k % sets], tg[k % sets]), pr[k % sets], one)

    def replayed(fn):
        """fn over each tensor pair captured into a hipGraph of its own: what a GraphedTrainStep replays, no host work."""
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for k in range(sets):
                fn(k)
        torch.cuda.current_stream().wait_stream(side)
        graphs = []
        for k in range(sets):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                fn(k)
            graphs.append(g)
        return lambda k: graphs[k % sets].replay()

    names = ("l2_loss + gradient", "l2_loss + gradient, metrics.psnr", "Monitor + gradient")
    nbytes = tg[0].numel() * 4 * 3  # two reads and the gradient's write
    rows = []
    print(f"loss of a training step at {B} x {H} x {W} x 3 fp32, forward + backward; {rounds} interleaved rounds of {args.steps}")
    for mode, fns in (("eager", (a, b, c)), ("hipGraph replay", tuple(replayed(fn) for fn in (a, b, c)))):
        for k in range(60):  # pre-roll
            for fn in fns:
                fn(k)
        torch.cuda.synchronize()
        times = {name: [] for name in names}
        for _ in range(rounds):
            for name, fn in zip(names, fns):
                times[name].append(timeit(fn, args.steps, rounds=1)[0])
        lo, hi = min(times[names[0]]), max(times[names[0]])
        for name in names:
            t = times[name]
            med = statistics.median(t)
            rows.append(dict(op=name, mode=mode, us=round(med, 2), us_min=round(min(t), 2), us_max=round(max(t), 2),
                             algorithmic_MB=round(nbytes / 1e6, 1), inside_l2_loss_spread=bool(lo <= med <= hi)))
            print(f"{mode:16s} {name:34s} {med:8.2f} us ({min(t):8.2f} .. {max(t):8.2f})   {nbytes / med / 1e3:7.1f} GB/s of "
                  f"the loss's own bytes   / l2_loss {med / statistics.median(times[names[0]]):6.3f}")
    print("Monitor.read():", monitor.read())
    if args.json:
        json.dump(dict(workload="metrics", rows=rows), open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
