// NHWC bilinear resize with align_corners = True: the `tf.image.resize_images(level, sz,
// BILINEAR, align_corners=True)` that builds HDRNetGaussianPyrNN's multi-scale input
// (hdrnet/models.py:253-266) and up-samples its coarse outputs (:283-286).
//
// TensorFlow is a dependency of the reference that is not vendored (hdrnet/requirements.txt:
// tensorflow_gpu==2.12.0); its published algorithm (tensorflow/core/kernels/image/
// resize_bilinear_op.cc, legacy path used when half_pixel_centers = false) is restated here:
//   scale = (in - 1) / float(out - 1)  (in / float(out) when out == 1)
//   src = i * scale;  lower = floor(src);  upper = min(ceil(src), in - 1);  lerp = src - lower
//   out = top + (bottom - top) * y_lerp,  top = tl + (tr - tl) * x_lerp
// One thread per output pixel; a pure gather, HBM-bound (reads every source pixel once when
// down-sampling by two: 4 * C * (Hin*Win + Hout*Wout) bytes).
//
// Training the pyramid model also needs the up-ADD of hdrnet/models.py:283-287 (`current = resize(current) + out_lvl`) and
// its VJP; as torch ops they were 0.46 ms of a 1.32-ms graph-captured step (upsample 78 us, its backward 149 us + fills,
// adds, permute copies).  resize_add: the resize above plus the fine level in the same pass.  resize_bilinear_grad: the
// transpose as a GATHER -- thread = source pixel, which walks the destination pixels whose two taps per axis can touch it
// (the same float arithmetic as the forward decides the taps and weights) and sums in a fixed order: no atomics, so the
// gradient is bit-reproducible.  Entry points in include/hdrnet_amd_train.h.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "../../include/hdrnet_amd_train.h"
#include "launch.hip.h"
#include "numerics.hip.h"
#include "white_level.hip.h"

namespace hdrnet_amd {
namespace {

template <int C>
__global__ __launch_bounds__(256) void resize_bilinear_ac(const float* __restrict__ in,
                                                          float* __restrict__ out, int Hin, int Win,
                                                          int Hout, int Wout, int Cdyn, float sh,
                                                          float sw, long long npx) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npx) return;
  const int x = (int)(p % Wout);
  const int y = (int)((p / Wout) % Hout);
  const long long b = p / ((long long)Wout * Hout);
  const int nc = C > 0 ? C : Cdyn;
  const float sy = mul_rn((float)y, sh), sx = mul_rn((float)x, sw);
  const float fy = floorf(sy), fx = floorf(sx);
  const float ly = sy - fy, lx = sx - fx;
  const int y0 = (int)fy, y1 = min((int)ceilf(sy), Hin - 1);
  const int x0 = (int)fx, x1 = min((int)ceilf(sx), Win - 1);
  const float* r0 = in + ((size_t)b * Hin + y0) * Win * nc;
  const float* r1 = in + ((size_t)b * Hin + y1) * Win * nc;
  float* o = out + (size_t)p * nc;
#pragma unroll
  for (int c = 0; c < nc; ++c) {
    const float tl = r0[x0 * nc + c], tr = r0[x1 * nc + c];
    const float bl = r1[x0 * nc + c], br = r1[x1 * nc + c];
    const float top = tl + (tr - tl) * lx;
    const float bot = bl + (br - bl) * lx;
    o[c] = top + (bot - top) * ly;
  }
}

// out[b, y, x, :] = resize(coarse)[b, y, x, :] + fine[b, y, x, :]
template <int C>
__global__ __launch_bounds__(256) void resize_add_ac(const float* __restrict__ in, const float* __restrict__ fine,
                                                     float* __restrict__ out, int Hin, int Win, int Hout, int Wout,
                                                     int Cdyn, float sh, float sw, long long npx) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npx) return;
  const int x = (int)(p % Wout);
  const int y = (int)((p / Wout) % Hout);
  const long long b = p / ((long long)Wout * Hout);
  const int nc = C > 0 ? C : Cdyn;
  const float sy = mul_rn((float)y, sh), sx = mul_rn((float)x, sw);
  const float fy = floorf(sy), fx = floorf(sx);
  const float ly = sy - fy, lx = sx - fx;
  const int y0 = (int)fy, y1 = min((int)ceilf(sy), Hin - 1);
  const int x0 = (int)fx, x1 = min((int)ceilf(sx), Win - 1);
  const float* r0 = in + ((size_t)b * Hin + y0) * Win * nc;
  const float* r1 = in + ((size_t)b * Hin + y1) * Win * nc;
  const float* f = fine + (size_t)p * nc;
  float* o = out + (size_t)p * nc;
#pragma unroll
  for (int c = 0; c < nc; ++c) {
    const float tl = r0[x0 * nc + c], tr = r0[x1 * nc + c];
    const float bl = r1[x0 * nc + c], br = r1[x1 * nc + c];
    const float top = tl + (tr - tl) * lx;
    const float bot = bl + (br - bl) * lx;
    o[c] = (top + (bot - top) * ly) + f[c];
  }
}

// The weight with which destination index i reads source index k along one axis of extent `nin`: the forward's
// out = a + (b - a) * l = a * (1 - l) + b * l up to rounding, a = in[floor(s)], b = in[min(ceil(s), nin - 1)].
__device__ __forceinline__ float tap_weight(int i, int k, float scale, int nin) {
  const float s = mul_rn((float)i, scale);
  const float f = floorf(s);
  const float l = s - f;
  const int k0 = (int)f, k1 = min((int)ceilf(s), nin - 1);
  return (k0 == k ? 1.0f - l : 0.0f) + (k1 == k ? l : 0.0f);
}

// din[b, ys, xs, :] = sum over destination pixels (y, x) of wy(y, ys) * wx(x, xs) * dout[b, y, x, :]
// (Hin x Win = the SOURCE of the forward, Hout x Wout its destination; rows then columns, ascending: a fixed order).
template <int C>
__global__ __launch_bounds__(256) void resize_bilinear_grad_ac(const float* __restrict__ dout, float* __restrict__ din,
                                                               int Hin, int Win, int Hout, int Wout, int Cdyn, float sh,
                                                               float sw, float inv_sh, float inv_sw, long long npx) {
  constexpr int kMaxC = C > 0 ? C : 4;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npx) return;
  const int xs = (int)(p % Win);
  const int ys = (int)((p / Win) % Hin);
  const long long b = p / ((long long)Win * Hin);
  const int nc = C > 0 ? C : Cdyn;
  // destination indices whose taps can be ys: floor(s) or ceil(s) == ys  =>  s in (ys - 1, ys + 1); one more on each side
  // for the rounding of the reciprocal
  // (clamped as floats: the reciprocal of a zero scale is huge)
  const int ylo = (int)fmaxf(floorf((float)(ys - 1) * inv_sh) - 1.0f, 0.0f);
  const int yhi = (int)fminf(ceilf((float)(ys + 1) * inv_sh) + 1.0f, (float)(Hout - 1));
  const int xlo = (int)fmaxf(floorf((float)(xs - 1) * inv_sw) - 1.0f, 0.0f);
  const int xhi = (int)fminf(ceilf((float)(xs + 1) * inv_sw) + 1.0f, (float)(Wout - 1));
  // the column weights do not depend on the row: kept for windows of <= 8 columns (up-sampling n -> 2 n: 8 -- the scale
  // is just under 1 / 2, (xs - 1, xs + 1) / scale just over 4 wide: 6 columns after floor / ceil, 8 with the slack)
  constexpr int kW = 8;
  float wxs[kW];
  const bool cached = xhi - xlo + 1 <= kW;
#pragma unroll
  for (int i = 0; i < kW; ++i) wxs[i] = (cached && xlo + i <= xhi) ? tap_weight(xlo + i, xs, sw, Win) : 0.0f;
  for (int c0 = 0; c0 < nc; c0 += kMaxC) {  // (one round unless C is dynamic and > 4)
    float acc[kMaxC], comp[kMaxC];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c) acc[c] = comp[c] = 0.0f;
    for (int y = ylo; y <= yhi; ++y) {
      const float wy = tap_weight(y, ys, sh, Hin);
      if (wy == 0.0f) continue;
      const float* row = dout + ((size_t)b * Hout + y) * Wout * nc;
      if (cached) {
#pragma unroll
        for (int i = 0; i < kW; ++i) {
          const float w = wy * wxs[i];
          if (w != 0.0f) {  // (wxs[i] == 0 beyond the window)
#pragma unroll
            for (int c = 0; c < kMaxC; ++c)
              if (c0 + c < nc) acc[c] = __builtin_fmaf(w, row[(size_t)(xlo + i) * nc + c0 + c], acc[c]);
          }
        }
      } else {
        // a window this wide can hold up to the whole destination per source pixel (one source row -> 1080 x 1920: 2 M terms,
        // beyond what a plain float32 running sum keeps to 2e-6 of the result): compensated, still in a fixed order
        for (int x = xlo; x <= xhi; ++x) {
          const float w = wy * tap_weight(x, xs, sw, Win);
          if (w == 0.0f) continue;
#pragma unroll
          for (int c = 0; c < kMaxC; ++c)
            if (c0 + c < nc) {
              const float t = __builtin_fmaf(w, row[(size_t)x * nc + c0 + c], -comp[c]);
              const float sum = acc[c] + t;
              comp[c] = (sum - acc[c]) - t;
              acc[c] = sum;
            }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
      if (c0 + c < nc) din[(size_t)p * nc + c0 + c] = acc[c];
  }
}

// ---- the forward resize reading the WIRE FORMAT (hdrnet_resize_bilinear_io, include/hdrnet_amd_pyramid_io.h) ----------
// out = resize_bilinear_ac(in / white_level) for uint8 / uint16 RGB: level 1 of the pyramid model built from the frame as it
// arrives (a 2:1 reduction of a uint8 4K frame reads 25 MB where the float32 frame is 100 MB).  Taps, scales and lerp are
// resize_bilinear_ac's, expression for expression; value / white_level is div_white (white_level.hip.h).
// A pixel's two taps of a source row are ADJACENT pixels (x1 = min(ceil(sx), Win - 1) <= floor(sx) + 1): 6 bytes of uint8
// or 12 of uint16 that start at any byte / even byte (a uint8 row is 3 * Win bytes), i.e. inside 3 / 4 aligned dwords.
// Those come with ONE load per source row and are realigned in registers (v_alignbyte, as sample_prep.hip does) -- two
// loads per output pixel instead of twelve single-byte ones.  A thread owns kIoRun consecutive output pixels: 2 * kIoRun
// independent loads in flight (the kernel is a gather bound by load latency) and 48 contiguous output bytes.  (At the
// pyramid's 2:1 the taps of neighbouring output pixels are disjoint source pixels, so a run shares no bytes; lanes next to
// each other read next to each other.)  Every load is of aligned dwords that hold at least one byte of the frame: where
// the span would pass the frame's last dword the lane loads dword by dword with each index clamped to it, and what a
// clamped dword returns is only ever the unused right tap of the frame's last pixel.
constexpr int kIoRun = 4;

struct u32x3a { uint32_t x, y, z; };  // 12 bytes exactly, 4-byte aligned
typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));

// l = pixel at sample index e (3 samples), r = the pixel after it, as floats / white level.  `last`: index of the frame
// buffer's last dword.
template <typename T>
__device__ __forceinline__ void load_tap_pair(const uint32_t* __restrict__ base, long long e, long long last,
                                              const WhiteLevel& wl, float (&l)[3], float (&r)[3]) {
  constexpr int ND = sizeof(T) == 1 ? 3 : 4;
  const long long o = e * (long long)sizeof(T);  // byte offset
  const long long d = o >> 2;
  const uint32_t shift = (uint32_t)o & 3u;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (d + ND - 1 <= last) {
    if constexpr (sizeof(T) == 1) {
      const u32x3a a = *reinterpret_cast<const u32x3a*>(base + d);
      w[0] = a.x; w[1] = a.y; w[2] = a.z;
    } else {
      const u32x4a a = *reinterpret_cast<const u32x4a*>(base + d);
      w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < ND; ++k) w[k] = base[d + k < last ? d + k : last];
  }
  uint32_t v[6];
  if constexpr (sizeof(T) == 1) {
    const uint32_t a = __builtin_amdgcn_alignbyte(w[1], w[0], shift), b = __builtin_amdgcn_alignbyte(w[2], w[1], shift);
    v[0] = a & 0xffu; v[1] = (a >> 8) & 0xffu; v[2] = (a >> 16) & 0xffu; v[3] = a >> 24; v[4] = b & 0xffu; v[5] = (b >> 8) & 0xffu;
  } else {
    const uint32_t a = __builtin_amdgcn_alignbyte(w[1], w[0], shift), b = __builtin_amdgcn_alignbyte(w[2], w[1], shift),
                   c = __builtin_amdgcn_alignbyte(w[3], w[2], shift);
    v[0] = a & 0xffffu; v[1] = a >> 16; v[2] = b & 0xffffu; v[3] = b >> 16; v[4] = c & 0xffffu; v[5] = c >> 16;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    l[c] = div_white((float)v[c], wl);
    r[c] = div_white((float)v[3 + c], wl);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void resize_bilinear_io_ac(const uint32_t* __restrict__ in, float* __restrict__ out,
                                                             const WhiteLevel wl, int Hin, int Win, int Hout, int Wout,
                                                             int nrun, float sh, float sw, long long nruns,
                                                             long long last, int vec) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= nruns) return;
  const int x = (int)(p % nrun) * kIoRun;
  const int y = (int)((p / nrun) % Hout);
  const long long b = p / ((long long)nrun * Hout);
  const float sy = mul_rn((float)y, sh);
  const float fy = floorf(sy);
  const float ly = sy - fy;
  const int y0 = min((int)fy, Hin - 1), y1 = min((int)ceilf(sy), Hin - 1);
  const long long r0 = (b * Hin + y0) * Win, r1 = (b * Hin + y1) * Win;  // first pixel of the two source rows
  float tl[kIoRun][3], tr[kIoRun][3], bl[kIoRun][3], br[kIoRun][3], lx[kIoRun];
  bool same[kIoRun];
#pragma unroll
  for (int k = 0; k < kIoRun; ++k) {
    const int xk = min(x + k, Wout - 1);  // a run's pixels past the row repeat its last one and are not stored
    const float sx = mul_rn((float)xk, sw);
    const float fx = floorf(sx);
    lx[k] = sx - fx;
    const int x0 = min((int)fx, Win - 1), x1 = min((int)ceilf(sx), Win - 1);
    same[k] = x1 <= x0;
    load_tap_pair<T>(in, (r0 + x0) * 3, last, wl, tl[k], tr[k]);
    load_tap_pair<T>(in, (r1 + x0) * 3, last, wl, bl[k], br[k]);
  }
  float o[kIoRun * 3];
#pragma unroll
  for (int k = 0; k < kIoRun; ++k) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float l0 = tl[k][c], l1 = bl[k][c];
      const float t1 = same[k] ? l0 : tr[k][c], b1 = same[k] ? l1 : br[k][c];
      const float top = l0 + (t1 - l0) * lx[k];
      const float bot = l1 + (b1 - l1) * lx[k];
      o[k * 3 + c] = top + (bot - top) * ly;
    }
  }
  float* op = out + ((b * Hout + y) * Wout + x) * 3;
  if (vec) {  // uniform: Wout % kIoRun == 0 and a 16-byte aligned output
#pragma unroll
    for (int q = 0; q < 3; ++q) reinterpret_cast<float4*>(op)[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < kIoRun; ++k) {
      if (x + k < Wout) {
#pragma unroll
        for (int c = 0; c < 3; ++c) op[k * 3 + c] = o[k * 3 + c];
      }
    }
  }
}

}  // namespace

hipError_t launch_resize_bilinear(const float* in, float* out, int B, int Hin, int Win, int Hout,
                                  int Wout, int C, hipStream_t s, const char** name) {
  const long long npx = (long long)B * Hout * Wout;
  const long long nblocks = (npx + 255) / 256;
  if (nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const float sh = Hout > 1 ? (float)(Hin - 1) / (float)(Hout - 1) : (float)Hin / (float)Hout;
  const float sw = Wout > 1 ? (float)(Win - 1) / (float)(Wout - 1) : (float)Win / (float)Wout;
  *name = "resize_bilinear_ac";
  if (C == 3)
    resize_bilinear_ac<3><<<(unsigned)nblocks, 256, 0, s>>>(in, out, Hin, Win, Hout, Wout, C, sh, sw, npx);
  else if (C == 1)
    resize_bilinear_ac<1><<<(unsigned)nblocks, 256, 0, s>>>(in, out, Hin, Win, Hout, Wout, C, sh, sw, npx);
  else
    resize_bilinear_ac<0><<<(unsigned)nblocks, 256, 0, s>>>(in, out, Hin, Win, Hout, Wout, C, sh, sw, npx);
  return hipGetLastError();
}

// input_dtype 1 uint8 / 2 uint16 (0 float32 forwards to launch_resize_bilinear: float32 is never scaled); three channels.
hipError_t launch_resize_bilinear_io(const void* in, int input_dtype, float white_level, float* out, int B, int Hin, int Win,
                                     int Hout, int Wout, hipStream_t s, const char** name) {
  if (input_dtype == 0) {
    const hipError_t e = launch_resize_bilinear(static_cast<const float*>(in), out, B, Hin, Win, Hout, Wout, 3, s, name);
    *name = "resize_bilinear_io/f32";
    return e;
  }
  if (input_dtype != 1 && input_dtype != 2) return hipErrorInvalidValue;
  const int nrun = (Wout + kIoRun - 1) / kIoRun;
  const long long nruns = (long long)B * Hout * nrun;
  const long long nblocks = (nruns + 255) / 256;
  if (nblocks > 0x7fffffffLL) return hipErrorInvalidValue;
  const float sh = Hout > 1 ? (float)(Hin - 1) / (float)(Hout - 1) : (float)Hin / (float)Hout;
  const float sw = Wout > 1 ? (float)(Win - 1) / (float)(Wout - 1) : (float)Win / (float)Wout;
  const long long bytes = (long long)B * Hin * Win * 3 * (input_dtype == 1 ? 1 : 2);
  const long long last = (bytes - 1) >> 2;
  const int vec = (Wout % kIoRun == 0 && ((uintptr_t)out & 15u) == 0) ? 1 : 0;
  const WhiteLevel wl = io_white_level(white_level);
  const uint32_t* src = static_cast<const uint32_t*>(in);
  if (input_dtype == 1) {
    *name = "resize_bilinear_io/u8";
    resize_bilinear_io_ac<uint8_t><<<(unsigned)nblocks, 256, 0, s>>>(src, out, wl, Hin, Win, Hout, Wout, nrun, sh, sw, nruns,
                                                                    last, vec);
  } else {
    *name = "resize_bilinear_io/u16";
    resize_bilinear_io_ac<uint16_t><<<(unsigned)nblocks, 256, 0, s>>>(src, out, wl, Hin, Win, Hout, Wout, nrun, sh, sw,
                                                                     nruns, last, vec);
  }
  return hipGetLastError();
}

}  // namespace hdrnet_amd

extern "C" int hdrnet_resize_add_f32(const float* coarse, const float* fine, float* output, int batch, int in_height,
                                     int in_width, int out_height, int out_width, int channels, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_resize_add_f32";
  if (!coarse || !fine || !output || batch <= 0 || in_height <= 0 || in_width <= 0 || out_height <= 0 || out_width <= 0 ||
      channels <= 0)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer or non-positive extent (B=%d, in %dx%d, out %dx%d, C=%d)", what,
                batch, in_height, in_width, out_height, out_width, channels);
  const long long npx = (long long)batch * out_height * out_width;
  const long long nblocks = (npx + 255) / 256;
  if (nblocks > 0x7fffffffLL) return fail(HDRNET_INVALID_ARGUMENT, "%s: output too large (%lld pixels)", what, npx);
  const float sh = out_height > 1 ? (float)(in_height - 1) / (float)(out_height - 1) : (float)in_height / (float)out_height;
  const float sw = out_width > 1 ? (float)(in_width - 1) / (float)(out_width - 1) : (float)in_width / (float)out_width;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (channels == 3)
    resize_add_ac<3><<<(unsigned)nblocks, 256, 0, s>>>(coarse, fine, output, in_height, in_width, out_height, out_width,
                                                       channels, sh, sw, npx);
  else
    resize_add_ac<0><<<(unsigned)nblocks, 256, 0, s>>>(coarse, fine, output, in_height, in_width, out_height, out_width,
                                                       channels, sh, sw, npx);
  return finish_launch(hipGetLastError(), what, nullptr);
}

extern "C" int hdrnet_resize_bilinear_grad_f32(const float* doutput, float* dinput, int batch, int in_height, int in_width,
                                               int out_height, int out_width, int channels, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_resize_bilinear_grad_f32";
  if (!doutput || !dinput || batch <= 0 || in_height <= 0 || in_width <= 0 || out_height <= 0 || out_width <= 0 ||
      channels <= 0)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer or non-positive extent (B=%d, in %dx%d, out %dx%d, C=%d)", what,
                batch, in_height, in_width, out_height, out_width, channels);
  const long long npx = (long long)batch * in_height * in_width;
  const long long nblocks = (npx + 255) / 256;
  if (nblocks > 0x7fffffffLL) return fail(HDRNET_INVALID_ARGUMENT, "%s: input too large (%lld pixels)", what, npx);
  const float sh = out_height > 1 ? (float)(in_height - 1) / (float)(out_height - 1) : (float)in_height / (float)out_height;
  const float sw = out_width > 1 ? (float)(in_width - 1) / (float)(out_width - 1) : (float)in_width / (float)out_width;
  // a source index k is touched by destination indices within (k - 1, k + 1) / scale; scale 0 (one source row): all of them
  const float inv_sh = sh > 0.0f ? 1.0f / sh : 3.0e38f, inv_sw = sw > 0.0f ? 1.0f / sw : 3.0e38f;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (channels == 3)
    resize_bilinear_grad_ac<3><<<(unsigned)nblocks, 256, 0, s>>>(doutput, dinput, in_height, in_width, out_height, out_width,
                                                                 channels, sh, sw, inv_sh, inv_sw, npx);
  else
    resize_bilinear_grad_ac<0><<<(unsigned)nblocks, 256, 0, s>>>(doutput, dinput, in_height, in_width, out_height, out_width,
                                                                 channels, sh, sw, inv_sh, inv_sw, npx);
  return finish_launch(hipGetLastError(), what, nullptr);
}
