// Semi-planar YUV 4:2:0 surfaces (include/hdrnet_amd_yuv.h): NV12 (uint8) and P010 / P016 (uint16) in, NV12 out -- and
// P010 / P016 out (include/hdrnet_amd_u16_out.h) -- and planar surfaces, I420 / yuv420p10le / yuv420p16le, in and out
// (include/hdrnet_amd_yuv_planar.h): the same functions with the chroma in two planes -- and 4:2:2 / 4:4:4 surfaces
// (include/hdrnet_amd_yuv_chroma.h): the same functions with a compile-time chroma layout, 4:2:0 by default -- and packed
// 4:2:2 surfaces (include/hdrnet_amd_yuv_packed.h): YUY2 / UYVY / YVYU / Y210 / Y216, the 4:2:2 pair woven into one plane.
//
// Every kernel that reads a surface -- hdrnet_yuv_to_rgb_f32 (apply_fwd_io_yuv.hip), the low-res gather
// (sample_prep.hip) and the fused forward (apply_fwd_io.hip.h) -- converts a pixel with the ONE function below, and the
// NV12 store of the fused forward encodes with the other two.  The kernels know nothing of colour standards or ranges:
// they apply 12 floats (hdrnet_amd/yuv.py: yuv_coefficients) to the samples as stored.  The chains are written with
// explicit fmaf / fmed3 so that no instantiation contracts them differently: the fused paths are held bit for bit
// against hdrnet_yuv_to_rgb_f32 followed by the RGB forward.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace hdrnet_amd {

// One plane pair of a batch: bytes per row, bytes between images (hdrnet_amd_yuv.h).  Padding beyond a row's samples is
// never read and never written.
struct YuvSurface {
  const void* y;
  const void* uv;
  int pitch_y, pitch_uv;
  long long image_y, image_uv;
};

// Chroma layout of a surface (include/hdrnet_amd_yuv_chroma.h), a compile-time axis of every load and store below: which
// chroma sample serves pixel (y, x).  4:2:0 (y >> 1, x >> 1), the default and the only one the headers above know; 4:2:2
// (y, x >> 1); 4:4:4 (y, x), planar surfaces only.  Chroma is replicated in all three.
constexpr int kChroma420 = 0, kChroma422 = 1, kChroma444 = 2;
__host__ __device__ constexpr int yuv_chroma_row(int chroma, int row) { return chroma == kChroma420 ? row >> 1 : row; }

typedef __attribute__((address_space(4))) const float yuv_cfloat;  // the 12 constants: wave-uniform, s_load

// m = [row 0: m00 m01 m02][row 1][row 2][bias0 bias1 bias2]
struct YuvMatrix {
  float m[9], bias[3];
};

__device__ __forceinline__ YuvMatrix yuv_load_matrix(const float* coef) {
  yuv_cfloat* c = (yuv_cfloat*)coef;
  YuvMatrix k;
#pragma unroll
  for (int i = 0; i < 9; ++i) k.m[i] = c[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) k.bias[i] = c[9 + i];
  return k;
}

// c_i = fmed3(fmaf(m_i2, V, fmaf(m_i1, U, fmaf(m_i0, Y, bias_i))), 0, 1) on the raw stored samples as floats.
__device__ __forceinline__ void yuv_to_rgb_px(const YuvMatrix& k, float Y, float U, float V, float* __restrict__ rgb) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float t = __builtin_fmaf(k.m[3 * i + 2], V, __builtin_fmaf(k.m[3 * i + 1], U, __builtin_fmaf(k.m[3 * i], Y, k.bias[i])));
    rgb[i] = __builtin_amdgcn_fmed3f(t, 0.0f, 1.0f);
  }
}

// A lane's 4 pixels x .. x + 3 of image row `row` (x % 4 == 0): one dword of Y and one of UV for uint8 samples, two of
// each for uint16 -- the chroma pairs (x >> 1) and (x >> 1) + 1 of chroma row (row >> 1) start at the same sample offset x
// of their row as the luma does in its own.  rgb[3 q + c]: pixel q, channel c (R, G, B).  Chroma is replicated.
// (CH == kChroma422, NV16 / P210 / P216: the same access into chroma row `row`.)
template <typename TI, int CH = kChroma420>
__device__ __forceinline__ void yuv_load_quad(const YuvSurface& s, const YuvMatrix& k, int b, int row, int x,
                                              float* __restrict__ rgb) {
  static_assert(sizeof(TI) == 1 || sizeof(TI) == 2, "uint8 or uint16 samples");
  static_assert(CH == kChroma420 || CH == kChroma422, "semi-planar 4:4:4 (NV24, P410) is out of scope");
  const char* yp = static_cast<const char*>(s.y) + (long long)b * s.image_y + (long long)row * s.pitch_y + (size_t)x * sizeof(TI);
  const char* cp = static_cast<const char*>(s.uv) + (long long)b * s.image_uv + (long long)yuv_chroma_row(CH, row) * s.pitch_uv + (size_t)x * sizeof(TI);
  float Y[4], U[2], V[2];
  if constexpr (sizeof(TI) == 1) {
    const uint32_t wy = *reinterpret_cast<const uint32_t*>(yp);
    const uint32_t wc = *reinterpret_cast<const uint32_t*>(cp);
#pragma unroll
    for (int q = 0; q < 4; ++q) Y[q] = (float)((wy >> (8 * q)) & 0xffu);
    U[0] = (float)(wc & 0xffu); V[0] = (float)((wc >> 8) & 0xffu);
    U[1] = (float)((wc >> 16) & 0xffu); V[1] = (float)(wc >> 24);
  } else {
    // (two dwords each: the planes promise 4-byte alignment, not 8)
    const uint2 wy = make_uint2(reinterpret_cast<const uint32_t*>(yp)[0], reinterpret_cast<const uint32_t*>(yp)[1]);
    const uint2 wc = make_uint2(reinterpret_cast<const uint32_t*>(cp)[0], reinterpret_cast<const uint32_t*>(cp)[1]);
    Y[0] = (float)(wy.x & 0xffffu); Y[1] = (float)(wy.x >> 16);
    Y[2] = (float)(wy.y & 0xffffu); Y[3] = (float)(wy.y >> 16);
    U[0] = (float)(wc.x & 0xffffu); V[0] = (float)(wc.x >> 16);
    U[1] = (float)(wc.y & 0xffffu); V[1] = (float)(wc.y >> 16);
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) yuv_to_rgb_px(k, Y[q], U[q >> 1], V[q >> 1], rgb + 3 * q);
}

// One pixel (row, x) of a surface, any x: scalar sample loads (the low-res gather).
template <typename TI, int CH = kChroma420>
__device__ __forceinline__ void yuv_load_px(const YuvSurface& s, const YuvMatrix& k, int b, int row, int x,
                                            float* __restrict__ rgb) {
  static_assert(CH == kChroma420 || CH == kChroma422, "semi-planar 4:4:4 (NV24, P410) is out of scope");
  const TI* yp = reinterpret_cast<const TI*>(static_cast<const char*>(s.y) + (long long)b * s.image_y + (long long)row * s.pitch_y);
  const TI* cp = reinterpret_cast<const TI*>(static_cast<const char*>(s.uv) + (long long)b * s.image_uv +
                                             (long long)yuv_chroma_row(CH, row) * s.pitch_uv);
  const int xc = (x >> 1) * 2;
  yuv_to_rgb_px(k, (float)yp[x], (float)cp[xc], (float)cp[xc + 1], rgb);
}

// ---- planar 4:2:0 surfaces (include/hdrnet_amd_yuv_planar.h): I420 (uint8) and yuv420p10le / yuv420p16le (uint16) -----------
// Three planes of a batch, each with its own bytes per row and bytes between images: y [B][H][W], u and v [B][H/2][W/2].
// (YV12: the caller passes the planes in the other order.)  Padding is never read and never written.
struct YuvPlanarSurface {
  const void* y;
  const void* u;
  const void* v;
  int pitch_y, pitch_u, pitch_v;
  long long image_y, image_u, image_v;
};

// The planar counterpart of yuv_load_quad: the lane's two chroma samples (x >> 1) and (x >> 1) + 1 of chroma row
// (row >> 1) are one 16-bit load from each of U and V for uint8 samples (the chroma planes promise 2-byte alignment, and
// x / 2 is even), one dword from each for uint16 (4-byte alignment); the luma is yuv_load_quad's.  The same
// yuv_to_rgb_px on the same samples: the bits of yuv_load_quad on the interleaved surface.
// (CH == kChroma422, yuv422p...: the same accesses into chroma row `row`.  CH == kChroma444, yuv444p...: the lane's four U and
// four V samples x .. x + 3 of chroma row `row` -- one dword from each plane for uint8 samples, two from each for uint16:
// a 4:4:4 chroma plane promises the luma's alignment.)
template <typename TI, int CH = kChroma420>
__device__ __forceinline__ void yuv_load_quad(const YuvPlanarSurface& s, const YuvMatrix& k, int b, int row, int x,
                                              float* __restrict__ rgb) {
  static_assert(sizeof(TI) == 1 || sizeof(TI) == 2, "uint8 or uint16 samples");
  constexpr bool FULL = CH == kChroma444;  // one chroma sample per pixel
  constexpr int NC = FULL ? 4 : 2;         // chroma samples of each plane per lane
  const char* yp = static_cast<const char*>(s.y) + (long long)b * s.image_y + (long long)row * s.pitch_y + (size_t)x * sizeof(TI);
  const size_t xc = (size_t)(FULL ? x : x >> 1) * sizeof(TI);
  const char* up = static_cast<const char*>(s.u) + (long long)b * s.image_u + (long long)yuv_chroma_row(CH, row) * s.pitch_u + xc;
  const char* vp = static_cast<const char*>(s.v) + (long long)b * s.image_v + (long long)yuv_chroma_row(CH, row) * s.pitch_v + xc;
  float Y[4], U[NC], V[NC];
  if constexpr (sizeof(TI) == 1) {
    const uint32_t wy = *reinterpret_cast<const uint32_t*>(yp);
#pragma unroll
    for (int q = 0; q < 4; ++q) Y[q] = (float)((wy >> (8 * q)) & 0xffu);
    if constexpr (FULL) {
      const uint32_t wu = *reinterpret_cast<const uint32_t*>(up);
      const uint32_t wv = *reinterpret_cast<const uint32_t*>(vp);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        U[q] = (float)((wu >> (8 * q)) & 0xffu);
        V[q] = (float)((wv >> (8 * q)) & 0xffu);
      }
    } else {
      const uint32_t wu = *reinterpret_cast<const uint16_t*>(up);
      const uint32_t wv = *reinterpret_cast<const uint16_t*>(vp);
      U[0] = (float)(wu & 0xffu); U[1] = (float)(wu >> 8);
      V[0] = (float)(wv & 0xffu); V[1] = (float)(wv >> 8);
    }
  } else {
    const uint2 wy = make_uint2(reinterpret_cast<const uint32_t*>(yp)[0], reinterpret_cast<const uint32_t*>(yp)[1]);
    Y[0] = (float)(wy.x & 0xffffu); Y[1] = (float)(wy.x >> 16);
    Y[2] = (float)(wy.y & 0xffffu); Y[3] = (float)(wy.y >> 16);
#pragma unroll
    for (int d = 0; d < NC / 2; ++d) {  // (dwords: the planes promise 4-byte alignment, not 8)
      const uint32_t wu = reinterpret_cast<const uint32_t*>(up)[d];
      const uint32_t wv = reinterpret_cast<const uint32_t*>(vp)[d];
      U[2 * d] = (float)(wu & 0xffffu); U[2 * d + 1] = (float)(wu >> 16);
      V[2 * d] = (float)(wv & 0xffffu); V[2 * d + 1] = (float)(wv >> 16);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) yuv_to_rgb_px(k, Y[q], U[FULL ? q : q >> 1], V[FULL ? q : q >> 1], rgb + 3 * q);
}

// One pixel (row, x) of a planar surface, any x: scalar sample loads (the low-res gather).
template <typename TI, int CH = kChroma420>
__device__ __forceinline__ void yuv_load_px(const YuvPlanarSurface& s, const YuvMatrix& k, int b, int row, int x,
                                            float* __restrict__ rgb) {
  const TI* yp = reinterpret_cast<const TI*>(static_cast<const char*>(s.y) + (long long)b * s.image_y + (long long)row * s.pitch_y);
  const TI* up = reinterpret_cast<const TI*>(static_cast<const char*>(s.u) + (long long)b * s.image_u +
                                             (long long)yuv_chroma_row(CH, row) * s.pitch_u);
  const TI* vp = reinterpret_cast<const TI*>(static_cast<const char*>(s.v) + (long long)b * s.image_v +
                                             (long long)yuv_chroma_row(CH, row) * s.pitch_v);
  const int xc = CH == kChroma444 ? x : x >> 1;
  yuv_to_rgb_px(k, (float)yp[x], (float)up[xc], (float)vp[xc], rgb);
}

// ---- packed 4:2:2 surfaces (include/hdrnet_amd_yuv_packed.h): YUY2 / UYVY / YVYU (uint8) and Y210 / Y216 (uint16) ------------
// ONE plane [B][H][2 W] samples: the NV16 / P210 surface with its two planes woven into one, a group of four samples
// (Y0 U Y1 V in HDRNET_PACKED_YUYV order) per horizontal pixel pair.  Padding is never read and never written.
struct YuvPackedSurface {
  const void* p;
  int pitch;   // bytes per row
  int order;   // HDRNET_PACKED_*: uint8 samples take all three, uint16 samples YUYV only
  long long image;  // bytes between images
};
constexpr int kPackedYUYV = 0, kPackedUYVY = 1, kPackedYVYU = 2;

// The byte order costs no instantiation: a uint8 group's dword is normalised to Y0 U Y1 V by one v_perm_b32 whose selector
// is wave-uniform (result byte i = source byte sel[i]).  UYVY swaps bytes 0 <-> 1 and 2 <-> 3, YVYU bytes 1 <-> 3: both are
// their own inverse, so the store applies the SAME selector to the Y0 U Y1 V dword it has built.
__device__ __forceinline__ uint32_t yuv_packed_selector(int order) {
  return order == kPackedUYVY ? 0x02030001u : order == kPackedYVYU ? 0x01020300u : 0x03020100u;
}
__device__ __forceinline__ uint32_t yuv_packed_perm(uint32_t w, uint32_t sel) { return __builtin_amdgcn_perm(w, w, sel); }

// yuv_load_quad of a packed surface: a lane's 4 pixels x .. x + 3 (x % 4 == 0) are two groups, 8 contiguous bytes of uint8
// samples (two dwords) or 16 of uint16 (four: [Y0 U][Y1 V][Y2 U'][Y3 V'], the code in the high bits as P210 / P216).  The
// same yuv_to_rgb_px on the same samples: the bits of yuv_load_quad<TI, kChroma422> on the unwoven (y, uv) pair.
template <typename TI>
__device__ __forceinline__ void yuv_load_quad(const YuvPackedSurface& s, const YuvMatrix& k, int b, int row, int x,
                                              float* __restrict__ rgb) {
  static_assert(sizeof(TI) == 1 || sizeof(TI) == 2, "uint8 or uint16 samples");
  const uint32_t* wp = reinterpret_cast<const uint32_t*>(static_cast<const char*>(s.p) + (long long)b * s.image +
                                                         (long long)row * s.pitch + (size_t)x * 2 * sizeof(TI));
  float Y[4], U[2], V[2];
  if constexpr (sizeof(TI) == 1) {
    const uint32_t sel = yuv_packed_selector(s.order);
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // (dwords: the surface promises 4-byte alignment, not 8)
      const uint32_t w = yuv_packed_perm(wp[h], sel);
      Y[2 * h] = (float)(w & 0xffu); U[h] = (float)((w >> 8) & 0xffu);
      Y[2 * h + 1] = (float)((w >> 16) & 0xffu); V[h] = (float)(w >> 24);
    }
  } else {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t w0 = wp[2 * h], w1 = wp[2 * h + 1];
      Y[2 * h] = (float)(w0 & 0xffffu); U[h] = (float)(w0 >> 16);
      Y[2 * h + 1] = (float)(w1 & 0xffffu); V[h] = (float)(w1 >> 16);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) yuv_to_rgb_px(k, Y[q], U[q >> 1], V[q >> 1], rgb + 3 * q);
}

// One pixel (row, x) of a packed surface, any x (the low-res gather): the pixel's group is samples 4 (x >> 1) .. + 3 of its
// row -- one aligned dword for uint8 samples, normalised as above; three scalar sample loads for uint16.  (CH: for callers
// written on the chroma layout; a packed surface is 4:2:2.)
template <typename TI, int CH = kChroma422>
__device__ __forceinline__ void yuv_load_px(const YuvPackedSurface& s, const YuvMatrix& k, int b, int row, int x,
                                            float* __restrict__ rgb) {
  static_assert(CH == kChroma422, "a packed surface is 4:2:2");
  const char* rp = static_cast<const char*>(s.p) + (long long)b * s.image + (long long)row * s.pitch;
  const int g = x >> 1;
  if constexpr (sizeof(TI) == 1) {
    const uint32_t w = yuv_packed_perm(reinterpret_cast<const uint32_t*>(rp)[g], yuv_packed_selector(s.order));
    yuv_to_rgb_px(k, (float)((w >> (16 * (x & 1))) & 0xffu), (float)((w >> 8) & 0xffu), (float)(w >> 24), rgb);
  } else {
    const TI* sp = reinterpret_cast<const TI*>(rp) + 4 * (size_t)g;
    yuv_to_rgb_px(k, (float)sp[2 * (x & 1)], (float)sp[1], (float)sp[3], rgb);
  }
}

// Surface output: code values clamped to code_max and truncated (the + 0.5 of the rounding is in the bias of from_rgb),
// placed `shift` bits up in the sample.  NV12 (uint8): code_max = 255, shift = 0, as compile-time constants.  P010 / P016
// (include/hdrnet_amd_u16_out.h): from_rgb is in code values of out_bits bits (hdrnet_amd/yuv.py:
// yuv_encode_coefficients), code_max = 2^out_bits - 1, and the code sits in the HIGH bits of the uint16 sample (shift = 16
// - out_bits).  c: R, G, B already clipped to [0, 1].  Luma per pixel; the LINEAR part of chroma row i per pixel, summed
// over the 2 x 2 block by the caller -- horizontal pair first, even row then odd row -- and finished by yuv_chroma_code
// (x 0.25, + bias, clamp).
__device__ __forceinline__ uint32_t yuv_luma_code(const YuvMatrix& k, const float* c, float code_max, int shift) {
  const float t = __builtin_fmaf(k.m[2], c[2], __builtin_fmaf(k.m[1], c[1], __builtin_fmaf(k.m[0], c[0], k.bias[0])));
  return ((uint32_t)__builtin_amdgcn_fmed3f(t, 0.0f, code_max)) << shift;
}
__device__ __forceinline__ float yuv_chroma_linear(const YuvMatrix& k, int i, const float* c) {
  return __builtin_fmaf(k.m[3 * i + 2], c[2], __builtin_fmaf(k.m[3 * i + 1], c[1], k.m[3 * i] * c[0]));
}
// (`weight`: the reciprocal of the chroma sample's footprint -- 0.25 for the 2 x 2 block of 4:2:0, 0.5 for the horizontal pair
// of 4:2:2, 1 for the single pixel of 4:4:4 -- applied in the fmaf that adds the bias.)
__device__ __forceinline__ uint32_t yuv_chroma_code(const YuvMatrix& k, int i, float sum, float code_max, int shift,
                                                    float weight = 0.25f) {
  return ((uint32_t)__builtin_amdgcn_fmed3f(__builtin_fmaf(sum, weight, k.bias[i]), 0.0f, code_max)) << shift;
}

}  // namespace hdrnet_amd
