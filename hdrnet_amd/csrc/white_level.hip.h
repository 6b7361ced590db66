// tf.to_float(im) / white_level for integer samples, shared by the wire-format forward (apply_fwd_io.hip) and the
// sample preparation (sample_prep.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>

namespace hdrnet_amd {

// v / wl for an integer sample v, correctly rounded like the IEEE division TF performs
// (tf.to_float(im) / white_level), in three instructions instead of the ~11 of a general IEEE divide:
//   q = v * r;  e = fma(-q, wl, v);  q' = fma(e, r, q)      with r = RN(1 / wl) from the host.
// With a correctly rounded reciprocal, one exact-remainder correction yields RN(v / wl) for every v
// unless wl's significand is all ones (Markstein, "Computation of elementary functions on the IBM RISC
// System/6000 processor", 1990, theorem on division by a correctly rounded reciprocal); v <= 65535 and
// wl in [2^-40, 2^40] keep every intermediate normal.  The host (io_white_level) checks those conditions and
// otherwise selects the plain divide; tests/test_gpu_parity.py compares both forms exhaustively over
// all 65536 sample values for the white levels of hdrnet/data_pipeline.py:202-232,267-274.
struct WhiteLevel {
  float wl, rcp;  // rcp = 0: use the IEEE divide
  float inv;      // RN(1 / wl), always: the factor folded into the coefficient image where the input feeds the affine only
};

__device__ __forceinline__ float div_white(float v, const WhiteLevel& w) {
  if (w.rcp == 0.0f) return v / w.wl;  // uniform
  const float q = v * w.rcp;
  const float e = __builtin_fmaf(-q, w.wl, v);
  return __builtin_fmaf(e, w.rcp, q);
}

// Host side of div_white: the reciprocal if the three-instruction form is exact for this white level.
inline WhiteLevel io_white_level(float wl) {
  unsigned bits;
  memcpy(&bits, &wl, sizeof bits);
  const bool all_ones = (bits & 0x7fffffu) == 0x7fffffu;
  const bool in_range = wl >= 0x1p-40f && wl <= 0x1p40f;
  volatile float r = 1.0f / wl;  // IEEE, correctly rounded
  return WhiteLevel{wl, (all_ones || !in_range) ? 0.0f : (float)r, (float)r};
}

}  // namespace hdrnet_amd
