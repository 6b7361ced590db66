// Sample preparation in one pass: wire-format source images in, the fp32 tensors the models and the training step
// consume out (hdrnet_prepare_batch, include/hdrnet_amd_train.h; hdrnet_lowres_input, include/hdrnet_amd.h).
//
// The reference does this on the host / in a chain of TF ops (hdrnet/data_pipeline.py:126-171 `_augment_data`,
// :228-241, :267-287; per inference frame hdrnet/bin/run.py:166-169 and benchmark/src/processor.cc:109-122):
//   s   = source[index]                                 [Hs][Ws][3], u8 / u16 / f32
//   s   = s[:, ::-1] if flip_lr;  s = s[::-1] if flip_ud;  s = rot90(s, k)      (counter-clockwise, tf.image.rot90)
//   out = s[crop_y : crop_y + H, crop_x : crop_x + W] / white_level             (tf.to_float(im) / wl, IEEE-rounded)
//   low[y, x] = out[min(floor(y * (H / (float)n)), H - 1), min(floor(x * (W / (float)n)), W - 1)]
// The last line is TF1's ResizeNearestNeighbor with align_corners=False (data_pipeline.py:165-169) and OpenCV's
// INTER_NEAREST (processor.cc:112); scale and product in fp32.  run.py's `skimage.transform.resize(order=0)` is
// centre-aligned, differs from it by one source pixel, and is NOT followed here.
//
// Everything is a map from an output pixel (y, x) of sample b back to a source pixel.  With Y = crop_y + y,
// X = crop_x + x the pixel before the flips is
//   rot90 0: (Y, X)   1: (X, Ws-1-Y)   2: (Hs-1-Y, Ws-1-X)   3: (Hs-1-X, Y)
// and then row -> Hs-1-row if flip_ud, col -> Ws-1-col if flip_lr: an affine map with unit steps (struct Geom).
//
// One launch, no workspace, no atomics.  A workgroup of a full-resolution job owns a tile of 32 rows x 64 pixels of the
// output:
//   1. it reads the source pixels of the tile along SOURCE rows, 4 pixels per lane as the aligned dwords that cover
//      them (a row start sits at any byte: crop_x, an odd Ws, flip_lr), realigns them in registers (v_alignbyte),
//      divides by the white level and writes them to LDS at their OUTPUT position -- the flips and quarter turns
//      happen in that LDS write, so odd turns read memory row-wise too (never 64 loads one source row apart);
//   2. after a barrier it walks the tile row by row and stores whole 16-byte vectors, lanes contiguous.
// The LDS tile is [32][192] floats with the float4 column XOR-ed by (row / 4) & 7: the transposed dword writes of an
// odd turn (a lane's 4 pixels are 4 tile rows) and the float4 accesses are then both free of bank conflicts.
// The low-res gather (B x n x n pixels, latency-bound) reads the SOURCE through the same map, so it has no ordering
// dependency on the full-res output and runs as extra workgroups of the same launch.
//
// Memory safety does not depend on the table: `index` is clamped to [0, N), the crop offsets to [0, dim - size],
// rot90 is masked with 3 (2 with HDRNET_SAMPLE_EVEN_TURNS_ONLY) and the flips with 1.  Such a record is a caller error
// whose result is the clamped sample.  Every load is of an aligned dword that contains at least one byte of the
// source buffer (dword indices are clamped to the buffer's last dword).
//
// The RAGGED flavour (hdrnet_prepare_batch_ragged) reads a set of images of mixed extents: the sources are two flat
// buffers, images back to back without padding, and a device table images[N][4] = {offset_lo, offset_hi, Hs, Ws} (the
// offset in samples, the same for both buffers) takes the place of the uniform (Hs, Ws).  A workgroup reads its record's
// descriptor with one wave-uniform 16-byte load through the constant address space; everything after make_geom is the
// same code with the image's own pitch.  An image then starts at any byte (u8) or even byte (u16), which the unaligned
// row machinery covers already.  Safety does not depend on the descriptors either: EVERY dword index of this flavour
// is clamped to the flat buffer, so a bad descriptor gives a wrong sample, never an access outside the buffer.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "launch.hip.h"
#include "white_level.hip.h"

namespace hdrnet_amd {
namespace {

constexpr int kTileH = 32, kTileW = 64, kThreads = 256;
constexpr int kRowVec = kTileW * 3 / 4;  // float4 per tile row
constexpr int kPitch = kTileW * 3;       // floats per tile row
static_assert(kRowVec % 8 == 0, "the XOR swizzle permutes aligned blocks of 8 float4");

struct PrepJob {
  const void* src;
  float* dst;
  WhiteLevel white;
  int dtype;   // 0 f32 (copied unscaled), 1 u8, 2 u16
  int lowres;  // 0: [B][H][W][3];  1: [B][n][n][3];  2: [B][n][n][3] gathered from a YUV surface (PrepParams::yuv);
               // 3: ... from a planar YUV surface (PrepParams::yuv_planar);  4: ... from a packed 4:2:2 one (::yuv_packed)
};

struct PrepParams {
  PrepJob job[3];
  const int* ops;  // device [B][8], or null: identity, index = b
  int N, Hs, Ws, B, H, W, n;
  float scale_y, scale_x;  // H / (float)n, W / (float)n
  int tiles_x, tiles;      // full-res tiles per sample
  int even_only;
  const int* images;    // RAGGED: device [N][4] = {offset_lo, offset_hi, Hs, Ws}, the offset in samples
  long long n_samples;  // RAGGED: samples of each flat source buffer
  // the low-res gather of a frame in another pixel format (hdrnet_lowres_input_px; the full-resolution jobs and the ragged
  // flavour are RGB): samples per stored pixel, and whether B comes first
  int px_stride, px_b_first;
  // the low-res gather of a semi-planar YUV surface (hdrnet_lowres_input_yuv, job kind 2): the planes and the 12 constants
  // of yuv_convert.hip.h; the job's dtype is the sample dtype
  // (... or of a packed 4:2:2 one, hdrnet_lowres_input_yuv_packed, job kind 4: one plane of the pair, in the pair's bytes --
  // the parameter block of every other job stays what it was)
  union {
    YuvSurface yuv;
    YuvPackedSurface yuv_packed;
  };
  const float* yuv_to_rgb;
  // ... of a planar one (hdrnet_lowres_input_yuv_planar, job kind 3): three planes, the same constants
  YuvPlanarSurface yuv_planar;
  int yuv_chroma;  // the surface's chroma layout (yuv_convert.hip.h: kChroma420 / 422 / 444; include/hdrnet_amd_yuv_chroma.h)
};

typedef uint32_t u32x2a __attribute__((ext_vector_type(2), aligned(4)));
struct u32x3a { uint32_t x, y, z; };  // 12 bytes exactly (a 3-vector type may be loaded as 4 dwords)
typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(4))) const i32x4 ci32x4;  // wave-uniform descriptor: s_load_dwordx4

// source (row, col) of output pixel (y, x):  even turns  row = r0 + rs * y, col = c0 + cs * x
//                                            odd turns   row = r0 + rs * x, col = c0 + cs * y
struct Geom {
  long long image;  // first sample of source image `index`
  int odd, r0, rs, c0, cs;
  int Ws;  // pixels per source row of that image
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool RAGGED>
__device__ __forceinline__ Geom make_geom(const PrepParams& p, int b) {
  int index = b, flr = 0, fud = 0, rot = 0, cy = 0, cx = 0;
  if (p.ops) {
    const int4 lo = *reinterpret_cast<const int4*>(p.ops + 8 * b);
    const int2 hi = *reinterpret_cast<const int2*>(p.ops + 8 * b + 4);
    index = lo.x; flr = lo.y & 1; fud = lo.z & 1; rot = lo.w & (p.even_only ? 2 : 3);
    cy = hi.x; cx = hi.y;
  }
  index = clampi(index, 0, p.N - 1);
  Geom g;
  int Hs = p.Hs, Ws = p.Ws;
  if constexpr (RAGGED) {
    // the record is the same for the whole workgroup: the descriptor is one scalar 16-byte load
    const i32x4 d = *((ci32x4*)p.images + __builtin_amdgcn_readfirstlane(index));
    g.image = (long long)(((unsigned long long)(uint32_t)d.y << 32) | (uint32_t)d.x);
    Hs = d.z; Ws = d.w;
  } else {
    g.image = (long long)index * p.Hs * p.Ws * p.px_stride;
  }
  g.Ws = Ws;
  g.odd = rot & 1;
  cy = clampi(cy, 0, (g.odd ? Ws : Hs) - p.H);
  cx = clampi(cx, 0, (g.odd ? Hs : Ws) - p.W);
  // the turn, in terms of (Y, X) = (cy + y, cx + x)
  const bool r_down = rot == 2 || rot == 3;  // row = Hs-1 - (Y or X)
  const bool c_down = rot == 1 || rot == 2;  // col = Ws-1 - (Y or X)
  g.rs = r_down ? -1 : 1;
  g.r0 = r_down ? Hs - 1 : 0;
  g.cs = c_down ? -1 : 1;
  g.c0 = c_down ? Ws - 1 : 0;
  g.r0 += g.rs * (g.odd ? cx : cy);
  g.c0 += g.cs * (g.odd ? cy : cx);
  if (fud) { g.r0 = Hs - 1 - g.r0; g.rs = -g.rs; }
  if (flr) { g.c0 = Ws - 1 - g.c0; g.cs = -g.cs; }
  return g;
}

__device__ __forceinline__ long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// index of the last dword of a source buffer of element type T
template <typename T, bool RAGGED>
__device__ __forceinline__ long long last_dword(const PrepParams& p) {
  const long long samples = RAGGED ? p.n_samples : (long long)p.N * p.Hs * p.Ws * p.px_stride;
  return ((samples * (long long)sizeof(T)) - 1) >> 2;
}

// 12 consecutive samples (4 pixels) starting at sample index e of the source, as floats / white level.  `last` is the
// index of the source buffer's last dword.  A group at a tile's edge may be valid in part only, and its span may then
// leave the buffer (before the first row of the first image, past the last row of the last one): such a lane loads dword
// by dword with each index clamped, so that the bytes of its valid pixels stay where they belong; the rest is discarded
// by the caller.
template <typename T>
__device__ __forceinline__ void load_4px(const void* src, long long e, long long last, const WhiteLevel& wl, float (&v)[12]) {
  const uint32_t* base = static_cast<const uint32_t*>(src);
  constexpr int ND = 3 * sizeof(T);              // dwords of 12 samples
  const long long o = e * (long long)sizeof(T);  // byte offset
  const long long d = o >> 2;
  uint32_t w[ND + 1];
  if (d >= 0 && d + ND - 1 <= last) {
    if constexpr (sizeof(T) == 1) {
      const u32x3a a = *reinterpret_cast<const u32x3a*>(base + d);
      w[0] = a.x; w[1] = a.y; w[2] = a.z;
    } else if constexpr (sizeof(T) == 2) {
      const u32x4a a = *reinterpret_cast<const u32x4a*>(base + d);
      const u32x2a c = *reinterpret_cast<const u32x2a*>(base + d + 4);
      w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = c.x; w[5] = c.y;
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const u32x4a a = reinterpret_cast<const u32x4a*>(base + d)[k];
        w[4 * k] = a.x; w[4 * k + 1] = a.y; w[4 * k + 2] = a.z; w[4 * k + 3] = a.w;
      }
    }
    w[ND] = sizeof(T) == 4 ? 0u : base[d + ND < last ? d + ND : last];  // needed only when the span starts inside a dword
  } else {
#pragma unroll
    for (int k = 0; k <= ND; ++k) w[k] = base[clampll(d + k, 0, last)];
  }
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int q = 0; q < 12; ++q) v[q] = __uint_as_float(w[q]);
  } else {
    const uint32_t shift = (uint32_t)o & 3u;
#pragma unroll
    for (int k = 0; k < ND; ++k) w[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], shift);
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      uint32_t s;
      if constexpr (sizeof(T) == 1) s = (w[q >> 2] >> (8 * (q & 3))) & 0xffu;
      else s = (w[q >> 1] >> (16 * (q & 1))) & 0xffffu;
      v[q] = div_white((float)s, wl);
    }
  }
}

// one pixel (3 samples) at sample index e -- of a pixel with alpha too: its colour samples are the first three of its
// 4 (uint8: one aligned dword; uint16: two), and alpha is never read into v.  CLAMP: the pixel's position comes from a descriptor table that is not
// trusted, so every dword index is clamped (the uniform flavour's positions are inside the buffer by construction).
template <typename T, bool CLAMP>
__device__ __forceinline__ void load_1px(const void* src, long long e, long long last, const WhiteLevel& wl, float (&v)[3]) {
  const uint32_t* base = static_cast<const uint32_t*>(src);
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = __uint_as_float(base[CLAMP ? clampll(e + c, 0, last) : e + c]);
  } else {
    const long long o = e * (long long)sizeof(T);
    const long long d = o >> 2;
    const uint32_t shift = (uint32_t)o & 3u;
    // u8: 3 bytes, inside one dword unless shift >= 2;  u16: 6 bytes, always exactly two dwords
    const uint32_t w0 = base[CLAMP ? clampll(d, 0, last) : d];
    const uint32_t w1 = base[CLAMP ? clampll(d + 1, 0, last) : (d + 1 < last ? d + 1 : last)];
    if constexpr (sizeof(T) == 1) {
      const uint32_t a = __builtin_amdgcn_alignbyte(w1, w0, shift);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = div_white((float)((a >> (8 * c)) & 0xffu), wl);
    } else {
      const uint32_t a = __builtin_amdgcn_alignbyte(w1, w0, shift);
      const uint32_t b = shift ? (w1 >> 16) : (w1 & 0xffffu);
      v[0] = div_white((float)(a & 0xffffu), wl);
      v[1] = div_white((float)(a >> 16), wl);
      v[2] = div_white((float)b, wl);
    }
  }
}

__device__ __forceinline__ int tile_addr(int ty, int e) {  // float index of element e (= 3 * px + c) of tile row ty
  return ty * kPitch + ((((e >> 2) ^ ((ty >> 2) & 7)) << 2) | (e & 3));
}

template <typename T, bool RAGGED>
__device__ __forceinline__ void full_tile(const PrepParams& p, const PrepJob& job, const Geom& g, int b, int tile_id,
                                          float* __restrict__ tile) {
  const int ty0 = (tile_id / p.tiles_x) * kTileH, tx0 = (tile_id % p.tiles_x) * kTileW;
  const int tid = threadIdx.x;
  const long long last = last_dword<T, RAGGED>(p);
  const bool rev = g.cs < 0;  // the 4 pixels of a group run against the source columns
  constexpr int kGroups = kTileH * kTileW / 4 / kThreads;
  float v[kGroups][12];
  if (!g.odd) {
    // a group = 4 pixels of one output row = 4 pixels of one source row
#pragma unroll
    for (int it = 0; it < kGroups; ++it) {
      const int grp = tid + kThreads * it, ty = grp / (kTileW / 4), x = tx0 + 4 * (grp % (kTileW / 4));
      const int row = g.r0 + g.rs * (ty0 + ty), col = g.c0 + g.cs * x - (rev ? 3 : 0);
      load_4px<T>(job.src, g.image + ((long long)row * g.Ws + col) * 3, last, job.white, v[it]);
    }
#pragma unroll
    for (int it = 0; it < kGroups; ++it) {
      const int grp = tid + kThreads * it, ty = grp / (kTileW / 4), gx = grp % (kTileW / 4);
      if (ty0 + ty < p.H && tx0 + 4 * gx < p.W) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          float4 o;
          float* of = reinterpret_cast<float*>(&o);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int q = 4 * k + j, px = q / 3, c = q % 3;
            of[j] = rev ? v[it][3 * (3 - px) + c] : v[it][q];
          }
          *reinterpret_cast<float4*>(tile + tile_addr(ty, 12 * gx + 4 * k)) = o;
        }
      }
    }
  } else {
    // a group = 4 pixels of one source row = one pixel of each of 4 output rows
#pragma unroll
    for (int it = 0; it < kGroups; ++it) {
      const int grp = tid + kThreads * it, tx = grp / (kTileH / 4), y = ty0 + 4 * (grp % (kTileH / 4));
      const int row = g.r0 + g.rs * (tx0 + tx), col = g.c0 + g.cs * y - (rev ? 3 : 0);
      load_4px<T>(job.src, g.image + ((long long)row * g.Ws + col) * 3, last, job.white, v[it]);
    }
#pragma unroll
    for (int it = 0; it < kGroups; ++it) {
      const int grp = tid + kThreads * it, tx = grp / (kTileH / 4), gy = grp % (kTileH / 4);
      if (tx0 + tx < p.W) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (ty0 + 4 * gy + j < p.H) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
              tile[tile_addr(4 * gy + j, 3 * tx + c)] = rev ? v[it][3 * (3 - j) + c] : v[it][3 * j + c];
          }
        }
      }
    }
  }
  __syncthreads();
  const int nvec = ((p.W - tx0 < kTileW ? p.W - tx0 : kTileW) * 3) >> 2;  // W % 4 == 0: whole float4
  float* out = job.dst + (((long long)b * p.H + ty0) * p.W + tx0) * 3;
#pragma unroll
  for (int k = 0; k < kTileH * kRowVec / kThreads; ++k) {
    const int f = tid + kThreads * k, ty = f / kRowVec, q = f % kRowVec;
    if (ty0 + ty < p.H && q < nvec)
      *reinterpret_cast<float4*>(out + (long long)ty * p.W * 3 + 4 * q) =
          *reinterpret_cast<const float4*>(tile + tile_addr(ty, 4 * q));
  }
}

// 4 consecutive samples of a low-res image of npx samples, starting at sample px0 (a multiple of 4)
__device__ __forceinline__ void store_lowres_4px(float* __restrict__ out, int px0, int npx, bool vec, const float (&v)[4][3]) {
  if (vec) {
    const float* f = &v[0][0];
#pragma unroll
    for (int k = 0; k < 3; ++k)
      *reinterpret_cast<float4*>(out + (long long)px0 * 3 + 4 * k) = make_float4(f[4 * k], f[4 * k + 1], f[4 * k + 2], f[4 * k + 3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (px0 + j < npx) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[(long long)(px0 + j) * 3 + c] = v[j][c];
      }
    }
  }
}

template <typename T, bool RAGGED>
__device__ __forceinline__ void lowres_job(const PrepParams& p, const PrepJob& job, const Geom& g, int b) {
  const long long last = last_dword<T, RAGGED>(p);
  const int npx = p.n * p.n;
  float* out = job.dst + (long long)b * npx * 3;
  const bool vec = (npx & 3) == 0;  // then every sample starts on a 16-byte boundary
  for (int px0 = 4 * (blockIdx.x * kThreads + threadIdx.x); px0 < npx; px0 += 4 * gridDim.x * kThreads) {
    float v[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int px = px0 + j < npx ? px0 + j : npx - 1;
      const int yl = px / p.n, xl = px % p.n;
      int y = (int)__builtin_floorf((float)yl * p.scale_y), x = (int)__builtin_floorf((float)xl * p.scale_x);
      y = y < p.H - 1 ? y : p.H - 1;
      x = x < p.W - 1 ? x : p.W - 1;
      const int row = g.r0 + g.rs * (g.odd ? x : y), col = g.c0 + g.cs * (g.odd ? y : x);
      load_1px<T, RAGGED>(job.src, g.image + ((long long)row * g.Ws + col) * p.px_stride, last, job.white, v[j]);
      if (p.px_b_first) {  // uniform: B, G, R as stored -> R, G, B
        const float t = v[j][0];
        v[j][0] = v[j][2];
        v[j][2] = t;
      }
    }
    store_lowres_4px(out, px0, npx, vec, v);
  }
}

// The same gather from a YUV surface: output sample (yl, xl) takes the source pixel lowres_job takes (identity geometry:
// hdrnet_lowres_input's), its luma from (y, x) and its chroma from (y >> 1, x >> 1), converted by yuv_to_rgb_px -- the
// bits of lowres_job on the float32 frame hdrnet_yuv_to_rgb_f32 writes.
// (`surf`: p.yuv, or p.yuv_planar for a planar surface -- the chroma then comes from two planes)
// (CH: the surface's chroma layout -- 4:2:2 takes the chroma from (y, x >> 1), 4:4:4 from (y, x))
// (a packed 4:2:2 surface, p.yuv_packed: luma and chroma from the pixel's group of ONE plane)
template <typename T, int CH, typename SURF>
__device__ __forceinline__ void lowres_job_yuv(const PrepParams& p, const SURF& surf, const PrepJob& job, int b) {
  const int npx = p.n * p.n;
  float* out = job.dst + (long long)b * npx * 3;
  const bool vec = (npx & 3) == 0;
  const YuvMatrix k = yuv_load_matrix(p.yuv_to_rgb);
  for (int px0 = 4 * (blockIdx.x * kThreads + threadIdx.x); px0 < npx; px0 += 4 * gridDim.x * kThreads) {
    float v[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int px = px0 + j < npx ? px0 + j : npx - 1;
      const int yl = px / p.n, xl = px % p.n;
      int y = (int)__builtin_floorf((float)yl * p.scale_y), x = (int)__builtin_floorf((float)xl * p.scale_x);
      y = y < p.H - 1 ? y : p.H - 1;
      x = x < p.W - 1 ? x : p.W - 1;
      yuv_load_px<T, CH>(surf, k, b, y, x, v[j]);
    }
    store_lowres_4px(out, px0, npx, vec, v);
  }
}

template <bool RAGGED>
__global__ __launch_bounds__(kThreads) void sample_prep_kernel(const PrepParams p) {
  __shared__ __attribute__((aligned(16))) float tile[kTileH * kPitch];
  const PrepJob& job = p.job[blockIdx.z];
  const int b = blockIdx.y;
  if (job.lowres >= 2) {  // a YUV surface, semi-planar (2) or planar (3): no geometry record, no packed source
    if constexpr (!RAGGED) {
      if (job.lowres == 4) {
        if (job.dtype == 1) lowres_job_yuv<uint8_t, kChroma422>(p, p.yuv_packed, job, b);
        else lowres_job_yuv<uint16_t, kChroma422>(p, p.yuv_packed, job, b);
      } else if (job.lowres == 2) {
        if (p.yuv_chroma == kChroma422) {
          if (job.dtype == 1) lowres_job_yuv<uint8_t, kChroma422>(p, p.yuv, job, b);
          else lowres_job_yuv<uint16_t, kChroma422>(p, p.yuv, job, b);
        } else if (job.dtype == 1) lowres_job_yuv<uint8_t, kChroma420>(p, p.yuv, job, b);
        else lowres_job_yuv<uint16_t, kChroma420>(p, p.yuv, job, b);
      } else {
        if (p.yuv_chroma == kChroma422) {
          if (job.dtype == 1) lowres_job_yuv<uint8_t, kChroma422>(p, p.yuv_planar, job, b);
          else lowres_job_yuv<uint16_t, kChroma422>(p, p.yuv_planar, job, b);
        } else if (p.yuv_chroma == kChroma444) {
          if (job.dtype == 1) lowres_job_yuv<uint8_t, kChroma444>(p, p.yuv_planar, job, b);
          else lowres_job_yuv<uint16_t, kChroma444>(p, p.yuv_planar, job, b);
        } else if (job.dtype == 1) lowres_job_yuv<uint8_t, kChroma420>(p, p.yuv_planar, job, b);
        else lowres_job_yuv<uint16_t, kChroma420>(p, p.yuv_planar, job, b);
      }
    }
    return;
  }
  const Geom g = make_geom<RAGGED>(p, b);
  if (job.lowres) {
    if (job.dtype == 1) lowres_job<uint8_t, RAGGED>(p, job, g, b);
    else if (job.dtype == 2) lowres_job<uint16_t, RAGGED>(p, job, g, b);
    else lowres_job<float, RAGGED>(p, job, g, b);
    return;
  }
  if ((int)blockIdx.x >= p.tiles) return;
  if (job.dtype == 1) full_tile<uint8_t, RAGGED>(p, job, g, b, blockIdx.x, tile);
  else if (job.dtype == 2) full_tile<uint16_t, RAGGED>(p, job, g, b, blockIdx.x, tile);
  else full_tile<float, RAGGED>(p, job, g, b, blockIdx.x, tile);
}

}  // namespace

hipError_t launch_sample_prep(const SamplePrepArgs& a, hipStream_t s) {
  PrepParams p{};
  int nj = 0;
  bool full = false;
  if (a.image_input) { p.job[nj++] = PrepJob{a.src_input, a.image_input, io_white_level(a.input_white_level), a.input_dtype, 0}; full = true; }
  if (a.image_target) { p.job[nj++] = PrepJob{a.src_target, a.image_target, io_white_level(a.target_white_level), a.target_dtype, 0}; full = true; }
  if (a.lowres_input)
    p.job[nj++] = PrepJob{a.src_input, a.lowres_input, io_white_level(a.input_white_level), a.input_dtype,
                           a.yuv_packed ? 4 : a.yuv_planar ? 3 : a.yuv ? 2 : 1};
  if (nj == 0 || a.B == 0) return hipSuccess;
  p.ops = a.ops;
  p.N = a.N; p.Hs = a.Hs; p.Ws = a.Ws; p.B = a.B; p.H = a.H; p.W = a.W; p.n = a.n;
  p.scale_y = a.n > 0 ? (float)a.H / (float)a.n : 0.0f;
  p.scale_x = a.n > 0 ? (float)a.W / (float)a.n : 0.0f;
  p.tiles_x = (a.W + kTileW - 1) / kTileW;
  p.tiles = p.tiles_x * ((a.H + kTileH - 1) / kTileH);
  p.even_only = a.even_turns_only ? 1 : 0;
  p.images = a.images;
  p.n_samples = a.n_samples;
  p.px_stride = px_stored(a.pixel_format);
  p.px_b_first = px_b_first(a.pixel_format) ? 1 : 0;
  p.yuv_chroma = a.yuv_chroma;
  if (a.yuv) {
    p.yuv = *a.yuv;
    p.yuv_to_rgb = a.yuv_to_rgb;
  }
  if (a.yuv_packed) {
    p.yuv_packed = *a.yuv_packed;
    p.yuv_to_rgb = a.yuv_to_rgb;
  }
  if (a.yuv_planar) {
    p.yuv_planar = *a.yuv_planar;
    p.yuv_to_rgb = a.yuv_to_rgb;
  }
  const long long low_blocks = ((long long)a.n * a.n + 4 * kThreads - 1) / (4 * kThreads);
  const long long gx = full ? p.tiles : low_blocks;
  const dim3 grid((unsigned)gx, (unsigned)a.B, (unsigned)nj);
  if (a.images) sample_prep_kernel<true><<<grid, kThreads, 0, s>>>(p);
  else sample_prep_kernel<false><<<grid, kThreads, 0, s>>>(p);
  return hipGetLastError();
}

}  // namespace hdrnet_amd
