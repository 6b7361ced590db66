#!/usr/bin/env python
"""Records what the C-ABI library answers to deliberately wrong and deliberately empty calls.

    python tests/golden/make_capi_errors.py [path/to/libhdrnet_amd.so]      # writes tests/golden/capi_errors.json

Run it against the library whose argument validation is the one to keep (default: the tree's own build); the
fixture then pins the return code, the complete hdrnet_last_error() text and, for the legal no-ops, the kernel
name "noop" of every row for the libraries that follow (tests/test_capi_errors.py).

Every row fails validation, or is a no-op that touches nothing: validation happens before any HIP call, so the
rows run on a machine without a GPU, and with one they never reach it.  Pointers are small fake addresses
(tests/test_capi_symbols.py does the same); no row may hold a combination that validates fully, and none goes as
far as a `*_supported` query or a zero-fill of an output (both may ask the HIP runtime something).  The generator
refuses to write a row whose answer is neither HDRNET_INVALID_ARGUMENT nor a "noop".

A row is {"fn", "case", "args", "rc", "error", "kernel"}: `args` positional, a pointer as an integer or null, the
network descriptions as {"CoeffNet": {...}} / {"CoeffNetGrads": {...}} (fields not given: every pointer P), an
`int*` result as {"int": start value}; `error` null = the entry point left the text alone (the training-loop
helpers before 0.2.8.1), `kernel` null = not a no-op.
"""
import ctypes
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "capi_errors.json")

P, Q, ODD = 0x1000, 0x1004, 0x1001  # aligned, 4-byte aligned only, unaligned
INF = 1e39  # +inf as a float

NET = dict(net_input_size=256, spatial_bin=16, luma_bins=8, channel_multiplier=1, n_out=3, n_in=4, n_levels=1, fc_layout=1)


def net(**kw):
    return {"CoeffNet": dict(NET, **kw)}


def grads(**kw):
    return {"CoeffNetGrads": kw}


APPLY = dict(grid=P, guide=P, input=P, out=P, B=1, H=4, W=4, GH=2, GW=2, GD=2, Cin=3, Cout=3, has_offset=1, flags=0)
ROWS_ = dict(APPLY, H_total=8, y0=0, rows=4)
NNG = dict(APPLY, guide_conv1=P, guide_conv2=P, guide_out=None, n_feats=16)
CURVES = dict(APPLY, input_dtype=0, input_white_level=1.0, output_dtype=0, guide_ccm=P, guide_shifts=P, guide_slopes=P,
              guide_mix=P, npts=16, guide_out=None, prepared=P)
UPADD = dict(APPLY, coarse=P, Hc=2, Wc=2, guide_conv1=None, guide_conv2=None, n_feats=0)
IO = dict(APPLY, input_dtype=1, input_white_level=255.0, output_dtype=1, guide_conv1=None, guide_conv2=None, n_feats=0,
          guide_out=None)
GRAD = dict(APPLY, dout=P, dgrid=P, dguide=P, dinput=P, workspace=None, workspace_bytes=0)
SLICE = dict(grid=P, guide=P, out=P, dout=P, dgrid=P, dguide=P, B=1, H=4, W=4, GH=2, GW=2, GD=2, C=12, flags=0,
             workspace=None, workspace_bytes=0)
PREP = dict(src_input=P, input_dtype=1, input_white_level=255.0, src_target=P, target_dtype=1, target_white_level=255.0,
            N=2, Hs=8, Ws=8, ops=P, B=2, image_input=P, image_target=P, H=4, W=4, lowres_input=None, net_input_size=0,
            flags=0, n_samples=1000, images=P)
ADAM = dict(param=P, grad=P, exp_avg=P, exp_avg_sq=P, n=16, step=P, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
RESIZE_T = dict(coarse=P, fine=P, output=P, doutput=P, dinput=P, batch=1, in_height=2, in_width=2, out_height=4,
                out_width=4, channels=3)
FLAG_ROWS = [("unknown flags", dict(flags=0x7)), ("variant in the product build", dict(flags=0x200)),
             ("bits above 15", dict(flags=0x10000))]
GUIDE_FLAG_ROWS = [("unknown flags", dict(flags=0x40000)), ("kernel-family bit", dict(flags=0x1))]
APPLY_ROWS = [("wrong extents", dict(GH=0)), ("negative extent", dict(B=-1)), ("image too large", dict(B=65536, H=65536, W=65536)),
              ("null buffer", dict(out=None)), ("null input", dict(input=None)), ("channel counts", dict(Cin=0, has_offset=0)),
              ("zero size", dict(B=0))]
BAND_ROWS = [("wrong extents", dict(W=-1)), ("null buffer", dict(grid=None)), ("band outside the frame", dict(y0=6)),
             ("negative y0", dict(y0=-1)), ("zero size", dict(rows=0))]
NNG_ROWS = [("wrong extents", dict(GD=0)), ("null buffer", dict(guide_conv2=None)), ("feature count", dict(n_feats=5000)),
            ("zero size", dict(H=0))]
CURVES_ROWS = [("wrong extents", dict(H=-1)), ("null buffer", dict(guide_mix=None)), ("dtype code", dict(input_dtype=5)),
               ("output dtype code", dict(output_dtype=2)), ("white level", dict(input_white_level=0.0)),
               ("knots", dict(npts=0)), ("channel counts", dict(Cout=0)), ("zero size", dict(W=0))]
UPADD_ROWS = [("wrong extents", dict(B=-1)), ("null buffer", dict(coarse=None)), ("guide and network both", dict(guide_conv1=P)),
              ("guide and network neither", dict(guide=None)), ("coarse extents", dict(Hc=0)),
              ("network without conv2", dict(guide=None, guide_conv1=P)), ("zero size", dict(H=0))]
IO_ROWS = [("wrong extents", dict(GW=-2)), ("null buffer", dict(out=None)), ("dtype code", dict(input_dtype=3)),
           ("white level", dict(input_white_level=-1.0)), ("neither guide nor network", dict(guide=None)),
           ("network without features", dict(guide=None, guide_conv1=P, guide_conv2=P)), ("zero size", dict(B=0))]
GRAD_ROWS = [("wrong extents", dict(GD=0)), ("null buffer", dict(dout=None)), ("null grid for dguide", dict(grid=None)),
             ("channel counts", dict(Cin=0, has_offset=0)), ("no gradient wanted", dict(dgrid=None, dguide=None, dinput=None)),
             ("zero size", dict(B=0))]
SLICE_ROWS = [("wrong extents", dict(GH=-1)), ("null buffer", dict(guide=None)), ("channel count", dict(C=0)),
              ("zero size", dict(H=0))]
SLICE_GRAD_ROWS = [("wrong extents", dict(W=-1)), ("null buffer", dict(dout=None)), ("null grid for dguide", dict(grid=None)),
                   ("channel count", dict(C=-3)), ("no gradient wanted", dict(dgrid=None, dguide=None)),
                   ("zero size", dict(B=0))]
PREP_COMMON = [("unknown flags", dict(flags=2)), ("dtype code", dict(target_dtype=3)), ("white level", dict(input_white_level=INF)),
               ("wrong extents", dict(H=0)), ("batch too large", dict(B=65536)), ("zero size", dict(B=0)),
               ("null buffer", dict(src_input=None)), ("target without source", dict(src_target=None)),
               ("no output", dict(image_input=None, image_target=None)), ("W not a multiple of 4", dict(W=6)),
               ("misaligned output", dict(image_input=Q)), ("misaligned source", dict(src_input=ODD))]
# the first extents beyond a limit of the launch geometry (hdrnet_amd/csrc/row_geom.h): an entry point without another
# kernel to fall back to names the limit (tests/extent_cases.py derives the extents, tests/test_extent_edges_host.py
# calls every such entry point with them)
WIDE = (1 << 23) + 4                 # the first W % 4 == 0 beyond kMaxFloatX
ROW_2G = -(-(1 << 31) // 48) * 4     # the first W % 4 == 0 whose 3-channel float row reaches 2^31 bytes
ROWS_EXTENT_ROWS = [("W beyond 2^23", dict(H=1, W=WIDE)), ("launch beyond 2^32 - 1 threads", dict(B=1024, H=65536))]
GENERIC_EXTENT_ROWS = [("no kernel beyond 2^32 - 256 pixels", dict(B=65536, H=65536, W=1))]
SEG_EXTENT_ROWS = [("H beyond 65535", dict(H=65536)), ("B beyond 65535", dict(B=65536, H=1)),
                   ("W beyond 2^23", dict(H=1, W=WIDE)), ("row beyond 2^31 bytes", dict(H=1, W=ROW_2G))]
PREP_EXTENT_ROWS = [("image too large", dict(Hs=16384, Ws=16384, H=16384, W=16384))]
ADAM_ROWS = [("wrong extents", dict(n=0)), ("null buffer", dict(step=None)), ("misaligned pointer", dict(grad=Q))]

# ---- the wire formats' other front ends: pixel formats, YUV surfaces, the pyramid model (their own headers)
IO_PX = dict(IO, flags=0, input_format=1, output_format=1)          # uint8 BGR both ways
CURVES_PX = dict(CURVES, input_dtype=1, input_white_level=255.0, output_dtype=1, input_format=3, output_format=3)  # BGRA
LOWRES_PX = dict(frames=P, dtype=1, white_level=255.0, B=1, H=64, W=64, lowres=P, net_input_size=16, pixel_format=3)
UPADD_IO = dict(UPADD, input_dtype=1, white_level=255.0, output_dtype=1, flags=0)
RESIZE_IO = dict(input=P, input_dtype=1, white_level=255.0, out=P, B=1, Hin=2, Win=2, Hout=4, Wout=4, C=3)
SURFACE = dict(y=P, uv=P, sample_dtype=1, pitch_y=8, pitch_uv=8, image_stride_y=32, image_stride_uv=16, B=1, H=4, W=8, to_rgb=P)
RGB_OUT = dict(output_kind=1, out=P, out_uv=None, out_pitch_y=0, out_pitch_uv=0, out_image_stride_y=0, out_image_stride_uv=0,
               from_rgb=None)
NV12_OUT = dict(output_kind=2, out=P, out_uv=P, out_pitch_y=8, out_pitch_uv=8, out_image_stride_y=32, out_image_stride_uv=16,
                from_rgb=P)
IO_YUV = dict(SURFACE, grid=P, guide=P, GH=2, GW=2, GD=2, Cin=3, Cout=3, has_offset=1, guide_conv1=None, guide_conv2=None,
              n_feats=0, guide_out=None, flags=0, **RGB_OUT)
CURVES_YUV = dict(SURFACE, grid=P, GH=2, GW=2, GD=2, Cin=3, Cout=3, has_offset=1, guide_ccm=P, guide_shifts=P, guide_slopes=P,
                  guide_mix=P, npts=16, prepared=None, guide_out=None, **RGB_OUT)
NETWORK = dict(guide=None, guide_conv1=P, guide_conv2=P, n_feats=16)
PRESCALED_ROWS = [("prescaled with a guide map", dict(flags=0x20000)),
                  ("prescaled misaligned", dict(NETWORK, guide_conv1=Q, flags=0x30000))]
# rows that break two rules which live in different steps of the front end: the text pins which one answers
IO_TWO_RULES = [("unknown flags and dtype code", dict(flags=0x40000, input_dtype=3)),
                ("null grid and missing guide", dict(grid=None, guide=None)),
                ("channel counts and white level", dict(Cin=0, input_white_level=0.0)),
                ("zero size with null buffers", dict(B=0, grid=None, guide=None, input=None, out=None)),
                ("zero size and unknown flags", dict(B=0, flags=0x40000))]
CURVES_TWO_RULES = [("knots and dtype code", dict(npts=0, input_dtype=5)), ("null buffer and misaligned tables", dict(grid=None, prepared=Q)),
                    ("tables need Cin = 3", dict(Cin=1, Cout=1, input_format=0, output_format=0)),
                    ("zero size and knots", dict(W=0, npts=0))]
PX_FORMAT_ROWS = [("unknown pixel format", dict(input_format=4, output_format=4)), ("negative pixel format", dict(input_format=-1, output_format=-1)),
                  ("unknown output format", dict(input_format=0, output_format=7, output_dtype=0)),
                  ("float32 with BGR", dict(input_dtype=0, input_white_level=1.0)),
                  ("float32 both ways with BGRA", dict(input_dtype=0, input_white_level=1.0, output_dtype=0, input_format=3, output_format=0)),
                  ("u8 output format differs", dict(output_format=0)), ("u8 output format differs from RGB", dict(input_format=0)),
                  ("f32 output not RGB", dict(output_dtype=0)),
                  ("unknown pixel format and wrong extents", dict(input_format=4, GH=0)),
                  ("unknown pixel format and W % 4", dict(input_format=4, W=6)),
                  ("unknown pixel format and dtype code", dict(input_format=4, input_dtype=3)),
                  ("zero size and unknown pixel format", dict(B=0, output_format=9))]
PX_BUFFER_ROWS = [("W not a multiple of 4", dict(W=6)), ("W % 4 with RGB passes the format step", dict(W=6, H=65536, input_format=0, output_format=0)),
                  ("4-channel alignment", dict(input_format=3, output_format=3, input=Q)),
                  ("4-channel alignment of out", dict(input_format=2, output_format=2, out=0x1008)),
                  ("4-channel u16 alignment", dict(input_format=3, output_format=3, input_dtype=2, input_white_level=65535.0, input=Q)),
                  ("3-channel alignment", dict(input_format=1, output_format=1, input=0x1002)),
                  ("not 3 -> 3", dict(Cin=4, Cout=4)), ("no offset", dict(has_offset=0)),
                  ("null input and W % 4", dict(input=None, W=6))]
SURFACE_ROWS = [("wrong extents", dict(B=-1)), ("null buffer", dict(y=None)), ("null uv plane", dict(uv=None)),
                ("null constants", dict(to_rgb=None)), ("misaligned plane", dict(y=0x1002)), ("odd H", dict(H=5)),
                ("W not a multiple of 4", dict(W=6)), ("pitch below row", dict(pitch_y=4)), ("uv pitch below row", dict(pitch_uv=4)),
                ("u16 pitch below row", dict(sample_dtype=2, image_stride_y=64, image_stride_uv=32)),
                ("pitch not a multiple of 4", dict(pitch_y=10)), ("uv pitch not a multiple of 4", dict(pitch_uv=14)),
                ("image stride", dict(image_stride_y=30)), ("image stride below plane", dict(B=2, image_stride_y=16)),
                ("sample dtype", dict(sample_dtype=0)), ("sample dtype 3", dict(sample_dtype=3)),
                ("H beyond 65535", dict(H=65536)), ("B beyond 65535", dict(B=65536, H=2)), ("row beyond 2^31 bytes", dict(H=2, W=ROW_2G)),
                ("odd H and sample dtype", dict(H=5, sample_dtype=0)), ("zero size", dict(B=0)),
                ("zero size with null buffers", dict(B=0, y=None, uv=None, to_rgb=None))]
YUV_IO_ROWS = SURFACE_ROWS + [
    ("output kind", dict(output_kind=3)), ("negative output kind", dict(output_kind=-1)), ("channel counts", dict(Cin=4, Cout=4)),
    ("output channel count", dict(Cout=4)), ("no offset", dict(has_offset=0)), ("null out", dict(out=None)),
    ("misaligned f32 out", dict(output_kind=0, out=Q)), ("output pitch below row", dict(NV12_OUT, out_pitch_y=4)),
    ("output pitch not a multiple of 4", dict(NV12_OUT, out_pitch_uv=10)), ("null output plane", dict(NV12_OUT, out_uv=None)),
    ("null output constants", dict(NV12_OUT, from_rgb=None)), ("null grid", dict(grid=None)),
    ("grid extents and odd H", dict(GH=0, H=5)), ("output kind and pitch", dict(output_kind=3, pitch_y=10)),
    ("output kind and channel counts", dict(output_kind=3, Cin=4, Cout=4)), ("null out and null grid", dict(out=None, grid=None)),
    ("zero size with a null NV12 output", dict(NV12_OUT, B=0, out=None, out_uv=None, from_rgb=None)),
    ("W beyond 2^23", dict(H=2, W=WIDE, pitch_y=WIDE, pitch_uv=WIDE))]

# function -> (base arguments by name, [(case, overrides)])
TABLE = {
    "hdrnet_bilateral_slice_apply_f32": (APPLY, APPLY_ROWS + GENERIC_EXTENT_ROWS),
    "hdrnet_bilateral_slice_apply_f32_ex": (APPLY, APPLY_ROWS + FLAG_ROWS + GENERIC_EXTENT_ROWS),
    "hdrnet_bilateral_slice_apply_rows_f32": (ROWS_, BAND_ROWS),
    "hdrnet_bilateral_slice_apply_rows_f32_ex": (ROWS_, BAND_ROWS + FLAG_ROWS),
    "hdrnet_bilateral_slice_apply_nnguide_f32": (NNG, NNG_ROWS + ROWS_EXTENT_ROWS),
    "hdrnet_bilateral_slice_apply_nnguide_f32_ex": (NNG, NNG_ROWS + GUIDE_FLAG_ROWS + [
        ("prescaled needs Cin = 3", dict(flags=0x20000, Cin=1, Cout=1)), ("prescaled misaligned", dict(flags=0x30000, guide_conv1=Q))]
        + ROWS_EXTENT_ROWS + [("unknown flags and feature count", dict(flags=0x40000, n_feats=0)),
                              ("null buffer and prescaled misaligned", dict(grid=None, flags=0x20000, guide_conv2=Q))]),
    "hdrnet_bilateral_slice_apply_io_curves": (CURVES, CURVES_ROWS + SEG_EXTENT_ROWS),
    "hdrnet_curves_guide_prepare_f32": (
        dict(guide_shifts=P, guide_slopes=P, npts=16, Cin=3, prepared=P, prepared_bytes=1 << 20, usable={"int": 7}),
        [("wrong extents", dict(npts=17)), ("channel count", dict(Cin=1)), ("null buffer", dict(guide_slopes=None)),
         ("buffer too small", dict(prepared_bytes=64)), ("misaligned pointer", dict(prepared=Q)), ("nowhere to report", dict(usable=None))]),
    "hdrnet_bilateral_slice_apply_io_curves_prepared": (CURVES, CURVES_ROWS + [
        ("misaligned tables", dict(prepared=Q)), ("too many knots for tables", dict(npts=20))] + SEG_EXTENT_ROWS + [
        ("knots and dtype code", dict(npts=0, input_dtype=5)), ("null buffer and misaligned tables", dict(grid=None, prepared=Q)),
        ("tables need Cin = 3", dict(Cin=1, Cout=1)), ("zero size and knots", dict(W=0, npts=0))]),
    "hdrnet_bilateral_slice_apply_upadd_f32": (UPADD, UPADD_ROWS + ROWS_EXTENT_ROWS),
    "hdrnet_bilateral_slice_apply_upadd_f32_ex": (UPADD, UPADD_ROWS + GUIDE_FLAG_ROWS + [
        ("prescaled with a guide map", dict(flags=0x20000))] + ROWS_EXTENT_ROWS + [
        ("prescaled misaligned", dict(NETWORK, guide_conv1=Q, flags=0x30000)),
        ("network without features", dict(NETWORK, n_feats=0)), ("unknown flags and coarse extents", dict(flags=0x40000, Hc=0)),
        ("coarse extents and guide and network both", dict(Hc=0, guide_conv1=P)),
        ("null buffer and prescaled with a guide map", dict(coarse=None, flags=0x20000)),
        ("zero size and guide and network neither", dict(H=0, guide=None))]),
    "hdrnet_resize_bilinear_f32": (dict({"in": P}, out=P, B=1, Hin=4, Win=4, Hout=8, Wout=8, C=3),
                                   [("wrong extents", dict(Hin=0)), ("null buffer", dict(out=None)), ("channel count", dict(C=0)),
                                    ("zero size", dict(Hout=0))]),
    # the two guide-network gradients: a too small workspace and a misaligned pointer are refused only after the
    # *_supported query, which asks the device for its compute-unit count (a HIP call), so their own row is a second
    # null buffer
    "hdrnet_pointwise_guide_grad_f32": (
        dict(input=P, guide=P, dguide=P, guide_conv1=P, guide_conv2=P, dinput=None, accumulate_dinput=0, dconv1=P, dconv2=P,
             npx=16, Cin=3, n_feats=16, workspace=P, workspace_bytes=1 << 20),
        [("wrong extents", dict(npx=-1)), ("null buffer", dict(dconv1=None)), ("null pixels", dict(input=None)),
         ("channel count", dict(Cin=0))]),
    "hdrnet_curves_guide_grad_f32": (
        dict(input=P, dguide=P, guide_ccm=P, guide_shifts=P, guide_slopes=P, guide_mix=P, dinput=None, accumulate_dinput=0,
             dccm=P, dshifts=P, dslopes=P, dmix=P, npx=16, Cin=3, npts=16, workspace=P, workspace_bytes=1 << 20),
        [("wrong extents", dict(npts=0)), ("null buffer", dict(dmix=None)), ("null pixels", dict(dguide=None))]),
    "hdrnet_input_moments_f32": (dict(input=P, npx=16, Cin=3, sums=P, moments=P, workspace=P, workspace_bytes=1 << 20),
                                 [("wrong extents", dict(npx=-1)), ("null buffer", dict(sums=None)), ("channel count", dict(Cin=2))]),
    "hdrnet_l2_loss_f32": (dict(prediction=P, target=P, n=16, loss=P, workspace=P, workspace_bytes=1 << 20),
                           [("wrong extents", dict(n=0)), ("null buffer", dict(loss=None)), ("misaligned pointer", dict(prediction=Q)),
                            ("workspace too small", dict(workspace_bytes=8)), ("no workspace", dict(workspace=None))]),
    "hdrnet_l2_loss_grad_f32": (dict(prediction=P, target=P, grad_output=P, n=16, dprediction=P),
                                [("wrong extents", dict(n=-1)), ("null buffer", dict(grad_output=None)),
                                 ("misaligned pointer", dict(dprediction=Q))]),
    "hdrnet_guide_nn_prescale_f32": (
        dict(guide_conv1=P, guide_conv2=P, n_feats=16, Cin=3, x_max=1.0, conv1_out=P, conv2_out=P),
        [("wrong extents", dict(n_feats=0)), ("channel count", dict(Cin=1)), ("x_max", dict(x_max=0.0)),
         ("x_max not finite", dict(x_max=INF)), ("null buffer", dict(guide_conv1=None)), ("misaligned pointer", dict(conv1_out=Q))]),
    "hdrnet_guide_fold_batch_f32": (
        dict(sums=P, moments=P, npx=16, w1=P, gamma=P, beta=P, w2=P, b2=P, eps=1e-5, momentum=0.1, Cin=3, n_feats=16, conv1=P,
             conv2=P, running_mean=None, running_var=None, num_batches_tracked=None),
        [("wrong extents", dict(npx=0)), ("null buffer", dict(gamma=None)), ("one running statistic", dict(running_mean=P))]),
    "hdrnet_guide_fold_batch_grad_f32": (
        dict(sums=P, moments=P, npx=16, w1=P, gamma=P, beta=P, eps=1e-5, Cin=3, n_feats=16, dconv1=P, dconv2=P, dw1=P,
             dbeta=P, dw2=P, db2=P),
        [("wrong extents", dict(n_feats=0)), ("channel count", dict(Cin=2)), ("null buffer", dict(db2=None))]),
    "hdrnet_coefficients_f32": (
        dict(lowres=P, net=net(), coeffs=P, B=1, workspace=P, workspace_bytes=1 << 30),
        [("wrong extents", dict(B=-1)), ("batch too large", dict(B=65536)), ("null description", dict(net=None)),
         ("hyper-parameters", dict(net=net(net_input_size=100))), ("null parameter", dict(net=net(pred_w=None))),
         ("null splat parameter", dict(net=net(splat_b=[P, P, P, None]))), ("null buffer", dict(coeffs=None)),
         ("workspace too small", dict(workspace_bytes=16)), ("misaligned workspace", dict(workspace=Q)), ("zero size", dict(B=0))]),
    "hdrnet_coefficients_grad_f32": (
        dict(lowres=P, net=net(), forward_workspace=P, dcoeffs=P, grads=grads(), B=1, workspace=P, workspace_bytes=1 << 30),
        [("wrong extents", dict(B=0)), ("batch too large", dict(B=9)), ("null description", dict(grads=None)),
         ("null parameter", dict(net=net(fc_w=[P, None, P]))), ("null gradient", dict(grads=grads(local_w=[P, None]))),
         ("null buffer", dict(forward_workspace=None)), ("workspace too small", dict(workspace_bytes=16)),
         ("misaligned workspace", dict(workspace=Q))]),
    "hdrnet_bilateral_slice_apply_io": (IO, IO_ROWS + SEG_EXTENT_ROWS),
    "hdrnet_bilateral_slice_apply_io_ex": (IO, IO_ROWS + GUIDE_FLAG_ROWS + [("prescaled with a guide map", dict(flags=0x20000))]
                                           + SEG_EXTENT_ROWS + [("prescaled misaligned", dict(NETWORK, guide_conv1=Q, flags=0x30000)),
                                                                ("guide map and network both", dict(guide_conv1=P, guide_conv2=P, n_feats=16, H=65536))]
                                           + IO_TWO_RULES),
    "hdrnet_bilateral_slice_apply_grad_f32": (GRAD, GRAD_ROWS),
    "hdrnet_bilateral_slice_apply_grad_f32_ex": (GRAD, GRAD_ROWS + FLAG_ROWS),
    "hdrnet_bilateral_slice_f32": (SLICE, SLICE_ROWS + GENERIC_EXTENT_ROWS),
    "hdrnet_bilateral_slice_f32_ex": (SLICE, SLICE_ROWS + FLAG_ROWS + GENERIC_EXTENT_ROWS),
    "hdrnet_bilateral_slice_grad_f32": (SLICE, SLICE_GRAD_ROWS),
    "hdrnet_bilateral_slice_grad_f32_ex": (SLICE, SLICE_GRAD_ROWS + FLAG_ROWS),
    "hdrnet_lowres_input": (dict(frames=P, dtype=1, white_level=255.0, B=1, H=64, W=64, lowres=P, net_input_size=16),
                            [("wrong extents", dict(H=0)), ("null buffer", dict(lowres=None)), ("null frames", dict(frames=None)),
                             ("dtype code", dict(dtype=7)), ("white level", dict(white_level=0.0)),
                             ("misaligned pointer", dict(lowres=Q)), ("zero size", dict(B=0)),
                             ("batch too large", dict(B=65536)), ("image too large", dict(H=16384, W=16384))]),
    "hdrnet_l2_loss_with_grad_f32": (
        dict(prediction=P, target=P, n=16, loss=P, dprediction_unit=P, workspace=P, workspace_bytes=1 << 20),
        [("wrong extents", dict(n=0)), ("null buffer", dict(loss=None)), ("workspace too small", dict(workspace_bytes=8)),
         ("misaligned pointer", dict(prediction=Q))]),
    "hdrnet_l2_loss_grad_scale_f32": (dict(dprediction=P, grad_output=P, n=16),
                                      [("wrong extents", dict(n=0)), ("null buffer", dict(grad_output=None)),
                                       ("misaligned pointer", dict(dprediction=Q))]),
    "hdrnet_loss_psnr_f32": (
        dict(prediction=P, target=P, n=48, batch=2, loss=P, psnr=P, image_mse=None, dprediction_unit=None, ema=None, decay=0.9,
             totals=None, workspace=P, workspace_bytes=1 << 20),
        [("wrong extents", dict(n=49)), ("null buffer", dict(psnr=None)), ("workspace too small", dict(workspace_bytes=8)),
         ("misaligned pointer", dict(target=Q)), ("misaligned scalar", dict(loss=0x1002)), ("misaligned totals", dict(totals=Q)),
         ("decay out of range", dict(ema=P, decay=1.5))]),
    "hdrnet_resize_add_f32": (RESIZE_T, [("wrong extents", dict(in_height=0)), ("null buffer", dict(fine=None)),
                                         ("output too large", dict(batch=65535, out_height=65535, out_width=65535))]),
    "hdrnet_resize_bilinear_grad_f32": (RESIZE_T, [("wrong extents", dict(channels=0)), ("null buffer", dict(dinput=None)),
                                                   ("input too large", dict(batch=65535, in_height=65535, in_width=65535))]),
    "hdrnet_adam_step_f32": (ADAM, ADAM_ROWS),
    "hdrnet_adam_step_tf_f32": (ADAM, ADAM_ROWS),
    # include/hdrnet_amd_pixel_formats.h
    "hdrnet_bilateral_slice_apply_io_px": (IO_PX, IO_ROWS + GUIDE_FLAG_ROWS + PRESCALED_ROWS + PX_FORMAT_ROWS + PX_BUFFER_ROWS + [
        ("missing guide and W % 4", dict(guide=None, W=6)),
        ("W % 4 and prescaled misaligned", dict(NETWORK, W=6, guide_conv1=Q, flags=0x30000))] + IO_TWO_RULES + SEG_EXTENT_ROWS),
    "hdrnet_bilateral_slice_apply_io_curves_px": (CURVES_PX, CURVES_ROWS + [
        ("misaligned tables", dict(prepared=Q)), ("too many knots for tables", dict(npts=20))] + PX_FORMAT_ROWS + PX_BUFFER_ROWS + [
        ("knots and unknown pixel format", dict(npts=0, input_format=4)), ("W % 4 and misaligned tables", dict(W=6, prepared=Q))]
        + CURVES_TWO_RULES + SEG_EXTENT_ROWS),
    "hdrnet_lowres_input_px": (LOWRES_PX, [
        ("wrong extents", dict(H=0)), ("null buffer", dict(lowres=None)), ("null frames", dict(frames=None)),
        ("dtype code", dict(dtype=7)), ("white level", dict(white_level=0.0)), ("misaligned pointer", dict(lowres=Q)),
        ("zero size", dict(B=0)), ("batch too large", dict(B=65536)), ("image too large", dict(H=16384, W=16384)),
        ("net input size", dict(net_input_size=0)), ("unknown pixel format", dict(pixel_format=4)),
        ("negative pixel format", dict(pixel_format=-2)), ("float32 with BGR", dict(dtype=0, white_level=1.0, pixel_format=1)),
        ("4-channel alignment", dict(frames=Q)), ("3-channel alignment", dict(frames=0x1002, pixel_format=1)),
        ("RGB is hdrnet_lowres_input", dict(pixel_format=0, lowres=None)),
        ("unknown pixel format and dtype code", dict(pixel_format=4, dtype=7)),
        ("unknown pixel format and null buffer", dict(pixel_format=4, lowres=None)),
        ("null buffer and white level", dict(lowres=None, white_level=0.0)),
        ("zero size with null buffers", dict(B=0, frames=None, lowres=None))]),
    # include/hdrnet_amd_yuv.h
    "hdrnet_yuv_to_rgb_f32": (dict(SURFACE, rgb=P), SURFACE_ROWS + [("null rgb", dict(rgb=None)), ("misaligned rgb", dict(rgb=Q)),
                                                                   ("null plane and null rgb", dict(uv=None, rgb=None))]),
    "hdrnet_lowres_input_yuv": (dict(SURFACE, lowres=P, net_input_size=4), SURFACE_ROWS + [
        ("null lowres", dict(lowres=None)), ("misaligned lowres", dict(lowres=Q)), ("net input size", dict(net_input_size=0)),
        ("empty frame", dict(H=0)), ("net input size and null plane", dict(net_input_size=0, y=None))]),
    "hdrnet_bilateral_slice_apply_io_yuv": (IO_YUV, YUV_IO_ROWS + GUIDE_FLAG_ROWS + PRESCALED_ROWS + [
        ("neither guide nor network", dict(guide=None)), ("network without features", dict(NETWORK, n_feats=0)),
        ("unknown flags and odd H", dict(flags=0x40000, H=5)), ("unknown flags and sample dtype", dict(flags=0x40000, sample_dtype=0)),
        ("null grid and missing guide", dict(grid=None, guide=None)), ("missing guide and null out", dict(guide=None, out=None)),
        ("zero size and unknown flags", dict(B=0, flags=0x40000))]),
    "hdrnet_bilateral_slice_apply_io_curves_yuv": (CURVES_YUV, YUV_IO_ROWS + [
        ("knots", dict(npts=0)), ("knots and odd H", dict(npts=0, H=5)), ("knots and wrong extents", dict(npts=0, GD=0)),
        ("null curves parameter", dict(guide_mix=None)), ("misaligned tables", dict(prepared=Q)),
        ("too many knots for tables", dict(prepared=P, npts=20)), ("null grid and misaligned tables", dict(grid=None, prepared=Q)),
        ("null out and misaligned tables", dict(out=None, prepared=Q)), ("zero size and knots", dict(B=0, npts=0))]),
    # include/hdrnet_amd_pyramid_io.h
    "hdrnet_resize_bilinear_io": (RESIZE_IO, [
        ("wrong extents", dict(Hin=0)), ("null buffer", dict(out=None)), ("null input", dict(input=None)), ("channel count", dict(C=4)),
        ("dtype code", dict(input_dtype=3)), ("white level", dict(white_level=0.0)), ("white level not finite", dict(white_level=INF)),
        ("input too large", dict(B=65535, Hin=65535, Win=65535)), ("misaligned input", dict(input=ODD)),
        ("misaligned out", dict(out=0x1002)), ("zero size", dict(Hout=0)), ("channel count and dtype code", dict(C=1, input_dtype=-1))]),
    "hdrnet_bilateral_slice_apply_upadd_io_ex": (UPADD_IO, UPADD_ROWS + GUIDE_FLAG_ROWS + PRESCALED_ROWS + [
        ("dtype code", dict(input_dtype=3)), ("output dtype code", dict(output_dtype=2)), ("white level", dict(white_level=0.0)),
        ("channel counts", dict(Cin=0)), ("network without features", dict(NETWORK, n_feats=0)),
        ("unknown flags and dtype code", dict(flags=0x40000, input_dtype=3)), ("dtype code and coarse extents", dict(output_dtype=2, Wc=-2)),
        ("coarse extents and guide and network both", dict(Hc=0, guide_conv1=P)),
        ("null buffer and prescaled with a guide map", dict(coarse=None, flags=0x20000)),
        ("zero size and guide and network neither", dict(H=0, guide=None)),
        ("float32 both ways is the float op", dict(input_dtype=0, white_level=1.0, output_dtype=0, H=1, W=WIDE))] + SEG_EXTENT_ROWS),
    "hdrnet_prepare_batch": (PREP, PREP_COMMON + [
        ("crop does not fit", dict(H=16)), ("crop does not fit turned", dict(Ws=16, W=12)),
        ("identity needs the whole image", dict(ops=None)), ("misaligned ops", dict(ops=ODD))] + PREP_EXTENT_ROWS),
    "hdrnet_prepare_batch_ragged": (PREP, PREP_COMMON + [
        ("empty table", dict(N=0)), ("empty sources", dict(n_samples=0)), ("null table", dict(images=None)),
        ("null ops", dict(ops=None)), ("image too large", dict(H=16384, W=16384)), ("misaligned table", dict(images=Q))]),
}
# the training-loop helpers that kept no error text before 0.2.8.1: the fixture holds their return codes only
NO_TEXT = ("hdrnet_l2_loss_with_grad_f32", "hdrnet_l2_loss_grad_scale_f32", "hdrnet_loss_psnr_f32", "hdrnet_resize_add_f32",
           "hdrnet_resize_bilinear_grad_f32", "hdrnet_adam_step_f32", "hdrnet_adam_step_tf_f32")


def parameter_names():
    src = ""
    for h in ("hdrnet_amd.h", "hdrnet_amd_train.h", "hdrnet_amd_pixel_formats.h", "hdrnet_amd_yuv.h", "hdrnet_amd_pyramid_io.h"):
        src += re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = {}
    for name in TABLE:
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        out[name] = [re.findall(r"[A-Za-z_0-9]+", p)[-1] for p in params.split(",")]
    return out


def decode(value, keep):
    """A fixture argument as a ctypes argument; `keep` holds what must outlive the call."""
    from hdrnet_amd import _lib
    if isinstance(value, dict):
        (kind, fields), = value.items()
        if kind == "int":
            keep.append(ctypes.c_int(fields))
            return ctypes.byref(keep[-1])
        obj = getattr(_lib, kind)()
        for fname, ftype in obj._fields_:
            if fname in fields:
                v = fields[fname]
                setattr(obj, fname, ftype(*v) if isinstance(v, list) else v)
            elif ftype is not ctypes.c_int:
                setattr(obj, fname, ftype(*([P] * ftype._length_)) if hasattr(ftype, "_length_") else P)
        keep.append(obj)
        return ctypes.addressof(obj)
    return value


def call(lib, fn, args):
    """(rc, error text, kernel name) of one fixture row on `lib` (argtypes as hdrnet_amd._lib declares them)."""
    from hdrnet_amd import _lib
    table = dict(_lib.SIGNATURES)
    for more in (_lib.TRAIN_SIGNATURES, _lib.PIXEL_FORMAT_SIGNATURES, _lib.YUV_SIGNATURES, _lib.PYRAMID_IO_SIGNATURES):
        table.update(more)
    f = getattr(lib, fn)
    f.restype, f.argtypes = table[fn]
    lib.hdrnet_last_error.restype = lib.hdrnet_last_kernel.restype = ctypes.c_char_p
    keep = []
    lib.hdrnet_bilateral_slice_f32(None, None, None, 1, 1, 1, 0, 0, 0, 0, None)  # a known text, not the last row's
    rc = f(*[decode(a, keep) for a in args])
    return rc, lib.hdrnet_last_error().decode(), lib.hdrnet_last_kernel().decode()


def main():
    if len(sys.argv) > 1:
        path = sys.argv[1]
    else:
        from hdrnet_amd import build
        path = build.build()
    lib = ctypes.CDLL(path)
    lib.hdrnet_enable_kernel_names(1)
    names = parameter_names()
    rows = []
    for fn, (base, cases) in TABLE.items():
        for case, over in cases:
            unknown = set(over) - set(names[fn])
            assert not unknown, (fn, case, unknown)
            a = dict(base, stream=None)
            a.update(over)
            args = [a[p] for p in names[fn]]
            rc, err, kern = call(lib, fn, args)
            assert rc == 1 or (rc == 0 and kern == "noop" and err == ""), (fn, case, rc, err, kern)
            rows.append({"fn": fn, "case": case, "args": args, "rc": rc, "error": None if fn in NO_TEXT else err,
                         "kernel": kern if rc == 0 else None})
    with open(OUT, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("%d rows of %d functions -> %s" % (len(rows), len(TABLE), OUT))


if __name__ == "__main__":
    main()
