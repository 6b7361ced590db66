/* Tools build of the C-ABI library: libhdrnet_amd_tools.so.
 *
 * Same sources and the same entry points as libhdrnet_amd.so (include/hdrnet_amd.h), compiled with
 * -DHDRNET_TOOLS_BUILD, plus what only benchmarks and experiments need:
 *
 *   - kernel VARIANTS of BilateralSliceApply forward, selected with HDRNET_VARIANT(n) in the
 *     `flags` of hdrnet_bilateral_slice_apply_f32_ex (tools/ab_bench.py times them interleaved
 *     with the product kernel).  Variants 106 and 108 are memory skeletons that do NOT compute the op
 *     (their kernel name starts with "ABLATION"); they are the reason this is a separate library.
 *       19    the round-1 product kernel (apply_fwd_rows), which the product keeps as its fallback
 *       106   memory skeleton: the shipped kernel's accesses (nontemporal lane-contiguous loads, lane-contiguous
 *             stores) on its row segments, no slicing -- the calibration of tools/make_traffic.py, power_probe.py
 *       108   skeleton 106 on flat 1024-pixel tasks
 *       The skeletons exist for 3 -> 3 with offset, W % 4 == 0 and 16-byte aligned buffers, whatever the kernel
 *       family; any other shape is refused ("variant N has no kernel for this shape"), not served by the product kernel.
 *       (2 one wavefront per tile, 3..6 the persistent stream, 7 per-lane stores, 8 nontemporal lane-contiguous loads,
 *                9..11 two to four quads per thread, 101 and 103..105 the other memory skeletons, 107 the empty launch;
 *                20..72, through round 4, the product kernel's own flavours.  Removed -- the forward's files hold the
 *                product's configurations only; measurements in DESIGN.md section 4, docs/EXPERIMENTS.md and
 *                profiles/, code in the history, last at 0006d48.)
 *       Any other number is refused with HDRNET_INVALID_ARGUMENT before a pointer is looked at: no variant runs the
 *       product kernel under its name.
 *   - kernel variants of the GRADIENT entry points (HDRNET_VARIANT(n) in the flags of
 *     hdrnet_bilateral_slice{,_apply}_grad_f32_ex; tools/bwd_ab.py times them interleaved):
 *       3     un-fused kernels (per-pixel VJPs and the dgrid contraction as separate launches)
 *       11    (dgrid == NULL) the round-1 per-pixel VJP kernel (apply_vjp_rows) instead of apply_vjp_seg
 *       (2 and 4..10: the bf16-split and f16 hi/lo' contractions, the timing ablations of the fused pass and its
 *                phase trace.  Removed -- grid_grad_mfma.hip holds the product's configurations only; measurements in
 *                DESIGN.md section 4.2, docs/EXPERIMENTS.md and profiles/, code in the history, last at 6d87df0.)
 *       Any other number is refused with HDRNET_INVALID_ARGUMENT: no variant runs the product pass under its name.
 *       knob 3 (hdrnet_tools_set_knob): rows per workgroup task of the fast gradient pass, forced
 *   - hdrnet_tools_set_trace: device buffer for the coefficient network's per-workgroup timeline (tools/coeff_trace.py).
 *
 * Nothing in the product path links or loads this library.
 */
#ifndef HDRNET_AMD_TOOLS_H_
#define HDRNET_AMD_TOOLS_H_

#include "hdrnet_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* device_buf: sized by the tracing tool (tools/coeff_trace.py); NULL disables. */
void hdrnet_tools_set_trace(void* device_buf);

/* Experiment knobs read at launch (knobs 0, 2 and 7 drove the product kernel's removed flavours, knob 1 padded the
 * gradient pass's LDS to lower its occupancy, knob 5 put the wire-format forward's guide network on the bf16 matrix
 * cores: removed with them, nothing reads those numbers):
 *   3  gradient pass: rg, the rows per workgroup task, FORCED instead of fitted to the device (gg_plan); 0 = fitted.
 *      Accepted: 1 .. cell, cell = max(H / GH, 1) -- a task's rows may span at most three clamped grid rows.  With any
 *      other value the pass refuses the shape: hdrnet_bilateral_slice{,_apply}_grad_workspace_bytes returns 0 and the
 *      gradient entry points take their other kernels.  While it is set the workspace query answers with exactly the
 *      forced plan's size, B * (GW + 1) * ceil(H / rg) tasks x (GD > 8 ? 2 : 1) x (C > 16 ? 2 : 1) tiles of
 *      3 x 16 x 16 floats: query after setting it.  Process-wide, like every knob: set it back to 0.  The planner
 *      itself returns min(cell, 4) .. cell; tests/test_gpu_grad_plans.py runs every such plan on small frames. */
void hdrnet_tools_set_knob(int idx, int value);

#ifdef __cplusplus
}
#endif

#endif /* HDRNET_AMD_TOOLS_H_ */
