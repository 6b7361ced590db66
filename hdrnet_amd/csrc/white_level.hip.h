// tf.to_float(im) / white_level for integer samples, shared by the wire-format forwards (apply_fwd_io.hip,
// apply_fwd_io_upadd.hip), the wire-format resize (resize_bilinear.hip) and the sample preparation (sample_prep.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

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

// Load 4 pixels x CIN channels of TI starting at element index e0, as floats / white level.
// UNSCALED: the samples as they are, (float)v -- the white level then sits in the coefficient image (stage_image IN_SCALE).
template <typename TI, int N, bool UNSCALED = false>
__device__ __forceinline__ void load_pixels(const TI* __restrict__ src, size_t e0, const WhiteLevel& wl,
                                            float (&dst)[N], uint32_t* raw = nullptr) {
  if constexpr (sizeof(TI) == 4) {
#pragma unroll
    for (int q = 0; q < N; ++q) dst[q] = reinterpret_cast<const float*>(src)[e0 + q];
  } else {
    static_assert((N * sizeof(TI)) % 4 == 0, "whole dwords per thread");
    constexpr int ND = N * sizeof(TI) / 4;
    uint32_t w[ND];
    const uint32_t* p = reinterpret_cast<const uint32_t*>(src + e0);
#pragma unroll
    for (int q = 0; q < ND; ++q) w[q] = p[q];
    if (raw) {
#pragma unroll
      for (int q = 0; q < ND; ++q) raw[q] = w[q];
    }
#pragma unroll
    for (int q = 0; q < N; ++q) {
      uint32_t v;
      if constexpr (sizeof(TI) == 1) v = (w[q >> 2] >> (8 * (q & 3))) & 0xffu;
      else v = (w[q >> 1] >> (16 * (q & 1))) & 0xffffu;
      if constexpr (UNSCALED) dst[q] = (float)v;
      else dst[q] = div_white((float)v, wl);  // tf.to_float(im) / white_level, rounded as TF's IEEE division
    }
  }
}

}  // namespace hdrnet_amd
