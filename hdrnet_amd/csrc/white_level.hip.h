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
// otherwise selects the plain divide; tests/test_host_logic.py steps through the three instructions in exact rational
// arithmetic for every sample value of the white levels of hdrnet/data_pipeline.py:202-232,267-274 (255, 65535, 32767)
// and compares with the IEEE division.
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

// How a wire-format frame stores a pixel (include/hdrnet_amd_pixel_formats.h: HDRNET_PX_*).  The model always sees
// R, G, B: the permutation is a matter of which bytes a load picks and a store fills, nowhere else.
constexpr int kPxRGB = 0, kPxBGR = 1, kPxRGBA = 2, kPxBGRA = 3;
constexpr int px_stored(int px) { return px >= kPxRGBA ? 4 : 3; }   // samples per stored pixel
constexpr bool px_b_first(int px) { return (px & 1) != 0; }        // B, G, R instead of R, G, B
// stored sample index of colour channel c (0 R, 1 G, 2 B) of a lane's pixel q
constexpr int px_sample(int px, int q, int c) { return q * px_stored(px) + (px_b_first(px) ? 2 - c : c); }

// Load 4 pixels x CIN channels of TI starting at element index e0, as floats / white level.
// UNSCALED: the samples as they are, (float)v -- the white level then sits in the coefficient image (stage_image IN_SCALE).
// PX (integer samples, N = 12): the frame's pixel format.  dst is R, G, B per pixel whatever the format; e0 counts STORED
// samples (4 per pixel with alpha: one 16-byte load per lane for uint8, two for uint16, from a 16-byte aligned frame);
// `alpha` receives the 4 pixels' alpha samples as stored -- never divided by the white level.
template <typename TI, int N, bool UNSCALED = false, int PX = kPxRGB>
__device__ __forceinline__ void load_pixels(const TI* __restrict__ src, size_t e0, const WhiteLevel& wl,
                                            float (&dst)[N], uint32_t* raw = nullptr, uint32_t* alpha = nullptr) {
  if constexpr (sizeof(TI) == 4) {
    static_assert(PX == kPxRGB, "float32 frames are RGB");
#pragma unroll
    for (int q = 0; q < N; ++q) dst[q] = reinterpret_cast<const float*>(src)[e0 + q];
  } else if constexpr (PX == kPxRGB) {
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
  } else {
    static_assert(N == 12, "4 pixels of 3 colour channels");
    constexpr int S = px_stored(PX);
    constexpr int ND = 4 * S * sizeof(TI) / 4;
    uint32_t w[ND];
    if constexpr (S == 4) {
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      const u32x4* p = reinterpret_cast<const u32x4*>(src + e0);
#pragma unroll
      for (int k = 0; k < ND / 4; ++k) {
        const u32x4 v = p[k];
        w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
      }
    } else {
      const uint32_t* p = reinterpret_cast<const uint32_t*>(src + e0);
#pragma unroll
      for (int q = 0; q < ND; ++q) w[q] = p[q];
    }
    const auto sample = [&w](int i) -> uint32_t {
      if constexpr (sizeof(TI) == 1) return (w[i >> 2] >> (8 * (i & 3))) & 0xffu;
      else return (w[i >> 1] >> (16 * (i & 1))) & 0xffffu;
    };
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint32_t v = sample(px_sample(PX, q, c));
        if constexpr (UNSCALED) dst[3 * q + c] = (float)v;
        else dst[3 * q + c] = div_white((float)v, wl);
      }
      if constexpr (S == 4) {
        if (alpha) alpha[q] = sample(4 * q + 3);
      }
    }
  }
}

}  // namespace hdrnet_amd
