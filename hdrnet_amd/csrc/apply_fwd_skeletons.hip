// TOOLS BUILD ONLY: the memory skeletons of the forward -- its loads, stores and launch shape with no slicing.  They
// do NOT compute the op (their kernel name says ABLATION): tools/make_traffic.py, tools/power_probe.py and
// tools/collect_profiles.sh run them as the calibration of what the memory system gives this access pattern.
//
//   106      the shipped kernel's accesses on its row segments: nontemporal lane-contiguous loads, lane-contiguous stores
//   108      the same accesses on flat 1024-pixel tasks (row boundaries ignored)
//
// Nothing here is reachable with flags == 0: the C-ABI's *_ex entry points of the tools library route these two variant
// numbers (flags bits 8..15) here, for 3 -> 3 with offset on a vec4-able frame, and refuse them for any other shape.
// The forwards that were measured and rejected (one wave per tile, the persistent stream, multi-quad, the other
// skeletons, the empty launch) are not kept: DESIGN.md section 4 and docs/EXPERIMENTS.md hold their figures.
#include <hip/hip_runtime.h>

#include "launch.hip.h"
#include "rows_common.hip.h"

namespace hdrnet_amd {
namespace {

using namespace rows;

// Variant 108: skeleton 106's accesses on FLAT tasks -- workgroup b moves pixels [1024 b, 1024 b + 1024) of the
// image taken as one run of B * H * W pixels, whatever rows they fall in: 1920 x 1080 = 2025 four-wave workgroups
// against the chip's 2048 slots, where row segments need 2160.  What a flattened decomposition of a one-round frame
// could gain, measured before building it.
__global__ __launch_bounds__(256) void apply_fwd_skeleton_flat(const float* __restrict__ guide,
                                                               const float* __restrict__ input,
                                                               float* __restrict__ out, long long npx) {
  const long long p0 = (long long)blockIdx.x * 1024;
  const int n = (int)min((long long)1024, npx - p0);  // pixels of this task (multiple of 4)
  const int t = threadIdx.x;
  float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (4 * t < n) g4 = load_stream4(guide + p0 + 4 * t);
  const float4* ip = reinterpret_cast<const float4*>(input + p0 * 3);
  float4* op = reinterpret_cast<float4*>(out + p0 * 3);
  const int nq = n * 3 / 4;
  float4 v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int e = t + 256 * k;
    if (e < nq) v[k] = load_stream4(reinterpret_cast<const float*>(ip + e));
  }
  const float gq = g4.x + g4.y + g4.z + g4.w;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int e = t + 256 * k;
    if (e < nq) {
      v[k].x *= gq; v[k].y *= gq; v[k].z *= gq; v[k].w *= gq;
      op[e] = v[k];
    }
  }
}

// Variant 106: a workgroup owns a row segment as in the product kernel; thread t touches float4 number t + k * blockDim
// of the segment's input / output (lane-contiguous), nontemporal loads.  The guide is read as in the product kernel.
__global__ __launch_bounds__(256) void apply_fwd_skeleton(
    const float* __restrict__ guide, const float* __restrict__ input, float* __restrict__ out,
    int H, int W, int nseg, int seg) {
  constexpr int CIN = 3, COUT = 3;
  const int bid = blockIdx.x;
  const int segi = bid % nseg;
  const int row = bid / nseg;
  const int xs = segi * seg;
  const int xe = min(xs + seg, W);
  const int x = xs + kPxPerThread * threadIdx.x;
  const bool active = x < xe;
  const size_t p = (size_t)row * W + x;
  float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (active) g4 = load_stream4(guide + p);
  const int nthreads = blockDim.x;
  const size_t seg_p = (size_t)row * W + xs;
  const int nq = (xe - xs) * CIN / 4;  // float4 count of the segment's input
  const float4* ip = reinterpret_cast<const float4*>(input + seg_p * CIN);
  float4* op = reinterpret_cast<float4*>(out + seg_p * COUT);
  float4 v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int e = (int)threadIdx.x + k * nthreads;
    if (e < nq) v[k] = load_stream4(reinterpret_cast<const float*>(ip + e));
  }
  const float gq = g4.x + g4.y + g4.z + g4.w;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int e = (int)threadIdx.x + k * nthreads;
    if (e < nq) {
      v[k].x *= gq; v[k].y *= gq; v[k].z *= gq; v[k].w *= gq;
      op[e] = v[k];
    }
  }
}

Plan skeleton_plan(const ApplyArgs& a) {
  return make_row_plan(a.W, a.GW, (ptr_bits(a.guide, a.input, a.out, a.grid) & 15u) == 0);
}

}  // namespace

// 3 -> 3 with offset, W % 4 == 0, 16-B aligned buffers, a launch grid of less than 2^31 workgroups.
bool apply_fwd_skeleton_supported(const ApplyArgs& a) {
  if (!(a.variant == 106 || a.variant == 108) || !(a.Cin == 3 && a.Cout == 3 && a.has_offset)) return false;
  const Plan pl = skeleton_plan(a);
  return pl.vec4 && (long long)a.B * a.H * pl.nseg <= 0x7fffffffLL;
}

hipError_t launch_apply_fwd_skeleton(const ApplyArgs& a, hipStream_t s, const char** name) {
  if (!apply_fwd_skeleton_supported(a)) return hipErrorInvalidValue;
  const Plan pl = skeleton_plan(a);
  if (a.variant == 106) {
    const unsigned nblocks = (unsigned)((long long)a.B * a.H * pl.nseg);
    apply_fwd_skeleton<<<nblocks, pl.threads, 0, s>>>(a.guide, a.input, a.out, a.H, a.W, pl.nseg, pl.seg);
    *name = "ABLATION/skeleton nt-ld-contig st-contig";
  } else {
    const long long npx = (long long)a.B * a.H * a.W;
    apply_fwd_skeleton_flat<<<(unsigned)((npx + 1023) / 1024), 256, 0, s>>>(a.guide, a.input, a.out, npx);
    *name = "ABLATION/skeleton flat 1024-px tasks";
  }
  return hipGetLastError();
}

}  // namespace hdrnet_amd
