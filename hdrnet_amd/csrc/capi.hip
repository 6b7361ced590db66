// C-ABI front-end of libhdrnet_amd.so: argument validation (the OP_REQUIRES checks
// of hdrnet/ops/bilateral_slice_apply_op.cc:147-193 and bilateral_slice_op.cc:129-147
// re-expressed as return codes), kernel selection, asynchronous launch on the
// caller's stream.  See include/hdrnet_amd.h for the contract.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "../../include/hdrnet_amd.h"
#include "../../include/hdrnet_amd_pixel_formats.h"
#include "../../include/hdrnet_amd_yuv.h"
#include "../../include/hdrnet_amd_yuv_planar.h"
#include "../../include/hdrnet_amd_yuv_chroma.h"
#include "../../include/hdrnet_amd_yuv_packed.h"
#include "../../include/hdrnet_amd_u16_out.h"
#include "../../include/hdrnet_amd_pyramid_io.h"
#include "../../include/hdrnet_amd_pyramid_yuv.h"
#include "../../include/hdrnet_amd_train.h"
#include "launch.hip.h"

namespace {

thread_local char g_error[512] = "";

// Introspection only (tests / benchmarks): name of the kernel(s) the most recent successful
// call launched.  OFF by default -- a launch then does no bookkeeping at all (no lock, no
// formatting); hdrnet_enable_kernel_names(1), or HDRNET_AMD_KERNEL_NAMES=1 in the environment at
// load time, switches it on.  Process-wide rather than thread-local because autograd runs
// backward on a thread of its own.  Not used for any decision.
std::atomic<int> g_kernel_names{-1};  // -1: consult the environment on first use
std::mutex g_kernel_mu;
char g_kernel_buf[128] = "";

bool kernel_names_on() {
  int v = g_kernel_names.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("HDRNET_AMD_KERNEL_NAMES");
    v = (e && *e && *e != '0') ? 1 : 0;
    g_kernel_names.store(v, std::memory_order_relaxed);
  }
  return v != 0;
}

void set_kernel(const char* a, const char* b = "", const char* c = "") {
  if (!kernel_names_on()) return;
  std::lock_guard<std::mutex> lock(g_kernel_mu);
  snprintf(g_kernel_buf, sizeof(g_kernel_buf), "%s%s%s%s%s", a, (*a && *b) ? "+" : "", b,
           ((*a || *b) && *c) ? "+" : "", c);
}

}  // namespace

// The tail of every entry point, here and beside the kernels (declared in launch.hip.h).
namespace hdrnet_amd {

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
  return code;
}

int finish_launch(hipError_t e, const char* what, const char* name) {
  if (e != hipSuccess) {
    // TF: errors::Internal("BilateralSliceApply kernel failed.")
    return fail(HDRNET_RUNTIME_FAILURE, "%s kernel failed: %s", what, hipGetErrorString(e));
  }
  g_error[0] = '\0';
  if (name) set_kernel(name);
  return HDRNET_OK;
}

int finish_noop() { return finish_launch(hipSuccess, "", "noop"); }

}  // namespace hdrnet_amd

namespace {

using hdrnet_amd::fail;
using hdrnet_amd::finish_launch;
using hdrnet_amd::finish_noop;

bool positive(int v) { return v > 0; }

// A grid gradient on the generic gather kernel (the reference's own design, bilateral_slice_apply.cc:84-138: every grid
// element loops over its +-1-cell pixel window) is ~100x slower than the contraction pass.  HDRNET_KERNEL_AUTO falls
// back to it for shapes the pass has no specialisation for (GD > 16, C > 32, an unlisted channel combination) or
// without a large enough workspace; on a frame-sized call (grad_dispatch asks only above kWarnGenericPixels, and works
// out the reason only then) that is a performance cliff worth one line on stderr per process and reason.
constexpr long long kWarnGenericPixels = 65536;
void warn_generic_grid_grad(const char* op, long long npix, int GD, int C, bool no_fast_shape) {
  static std::atomic<bool> said[2];
  if (said[no_fast_shape].exchange(true)) return;
  fprintf(stderr, "hdrnet_amd: %s on %lld pixels (GD=%d, C=%d) takes the generic grid-gradient kernel, ~100x slower "
          "than the fast pass (%s)\n", op, npix, GD, C,
          no_fast_shape ? "no fast specialisation for this shape: needs GD <= 16, C <= 32 and a listed channel combination"
                        : "no workspace passed: see hdrnet_bilateral_slice*_grad_workspace_bytes");
}

// Extents >= 0; a zero-sized batch / image is a legal no-op, a zero-sized grid is not.
int check_common(int B, int H, int W, int GH, int GW, int GD) {
  if (B < 0 || H < 0 || W < 0)
    return fail(HDRNET_INVALID_ARGUMENT, "negative image extent (B=%d, H=%d, W=%d)", B, H, W);
  if (!positive(GH) || !positive(GW) || !positive(GD))
    return fail(HDRNET_INVALID_ARGUMENT, "grid extents must be positive (GH=%d, GW=%d, GD=%d)",
                GH, GW, GD);
  if ((long long)B * H * W > 0x7fffffffLL * 64)
    return fail(HDRNET_INVALID_ARGUMENT, "image too large");
  if ((long long)GH * GW * GD > 0x7fffffffLL / 4096)
    return fail(HDRNET_INVALID_ARGUMENT, "grid too large");
  return HDRNET_OK;
}

// The generic kernels launch one thread per pixel on a one-dimensional grid, and the HIP runtime refuses a launch of 2^32
// threads or more: a frame that no LDS-staged kernel takes and that is this large has no kernel at all.
constexpr long long kGenericMaxPixels = 0xffffffffLL - 255;
int refuse_generic(const char* what, long long npix) {
  return fail(HDRNET_INVALID_ARGUMENT, "%s: no kernel for this frame: the generic kernels take at most 2^32 - 256 pixels "
              "(B * H * W = %lld)", what, npix);
}

// The refusal of a fused forward, which has no other kernel to fall back to: where the frame's EXTENTS break a limit of
// the last kernel family the entry point could take (`limits`: row_geom.h; `row_channels`: floats per pixel of its
// widest pixel stream), the text names that limit; else it is `otherwise`, the entry point's shape and alignment rules.
int refuse_fused(int B, int H, int W, int GW, int GD, int row_channels, unsigned limits, const char* otherwise) {
  using namespace hdrnet_amd::rows;
  if (const char* limit = extent_refusal(Frame{B, H, W, GW, GD}, row_channels, limits))
    return fail(HDRNET_INVALID_ARGUMENT, "frame beyond the fused kernels' extents (B=%d, H=%d, W=%d): %s", B, H, W, limit);
  return fail(HDRNET_INVALID_ARGUMENT, "%s", otherwise);
}

// flags: bits 0..7 kernel family (HDRNET_KERNEL_*), bits 8..15 variant inside the family
// (0 = the library's default; used by benchmarks for A/B runs), rest must be zero.
// flags of the guide-network entry points (..._nnguide_f32_ex, ..._upadd_f32_ex, ..._io_ex): the sigmoid choice and
// whether conv1 / conv2 are the prescaled arrays of hdrnet_guide_nn_prescale_f32
int check_guide_flags(unsigned flags) {
  if ((flags & ~(HDRNET_GUIDE_SIGMOID_FAST | HDRNET_GUIDE_RELU_PRESCALED)) != 0)
    return fail(HDRNET_INVALID_ARGUMENT,
                "unknown flags 0x%x (guide-network entry points take HDRNET_GUIDE_SIGMOID_FAST, HDRNET_GUIDE_RELU_PRESCALED)",
                flags);
  return HDRNET_OK;
}

// ... and what the flags ask of the launch (`a`: ApplyArgs or ApplyIoArgs), once the pointers count.
// HDRNET_GUIDE_RELU_PRESCALED: a guide NETWORK of three input channels whose arrays are 16-B aligned ([n][4] rows, s_load_dwordx4)
template <class Args>
int set_guide_flags(Args& a, unsigned flags, int Cin, const float* conv1, const float* conv2) {
  if (flags & HDRNET_GUIDE_RELU_PRESCALED) {
    if (!conv1 || !conv2 || Cin != 3)
      return fail(HDRNET_INVALID_ARGUMENT, "HDRNET_GUIDE_RELU_PRESCALED needs a guide network with Cin = 3 (Cin=%d)", Cin);
    if (((uintptr_t)conv1 | (uintptr_t)conv2) & 15u)
      return fail(HDRNET_INVALID_ARGUMENT, "HDRNET_GUIDE_RELU_PRESCALED needs 16-B aligned guide_conv1 / guide_conv2 "
                                           "(the arrays hdrnet_guide_nn_prescale_f32 wrote)");
  }
  a.fast_sigmoid = (flags & HDRNET_GUIDE_SIGMOID_FAST) != 0;
  a.guide_prescaled = (flags & HDRNET_GUIDE_RELU_PRESCALED) != 0;
  return HDRNET_OK;
}

// The up-add entry points name their guide source before the no-op: a map or the network, never both, and a network whole.
int check_upadd_values(int Hc, int Wc, const float* guide, const float* conv1, const float* conv2, int n_feats) {
  if (Hc <= 0 || Wc <= 0) return fail(HDRNET_INVALID_ARGUMENT, "bad coarse extents (%d x %d)", Hc, Wc);
  if ((guide != nullptr) == (conv1 != nullptr))
    return fail(HDRNET_INVALID_ARGUMENT, "give either a guide map or the guide network, not both / neither");
  if (conv1 && (!conv2 || n_feats <= 0 || n_feats > 4096))
    return fail(HDRNET_INVALID_ARGUMENT, "guide network needs conv1, conv2 and 0 < n_feats <= 4096");
  return HDRNET_OK;
}

// ... and on a YUV surface (include/hdrnet_amd_pyramid_yuv.h): the coarse level as the surface entry points' bodies take it,
// and the one rule of its pointer (the float ops' coarse level sits in 16-B aligned tensors; here it is read dword by dword)
struct IoCoarse {
  const float* coarse;
  int Hc, Wc;
};

int check_coarse_pointer(const char* what, const float* coarse) {
  if (!coarse || ((uintptr_t)coarse & 3u))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: coarse must be a 4-B aligned buffer ([B][Hc][Wc][3] float32)", what);
  return HDRNET_OK;
}

// ---- The wire-format forwards (..._io_ex / _px, ..._io_curves_prepared / _px, ..._upadd_io_ex, ..._io_yuv, ..._io_curves_yuv,
// and their 16-bit-output twins ..._px_u16 / ..._yuv_p016 of include/hdrnet_amd_u16_out.h)
// fill one ApplyIoArgs from a pixel source, a guide source and a launch.  Each side checks values before the zero-size
// no-op and pointers after it, as two functions: a frame's are check_frame_values / check_pixel_buffers, a YUV surface's
// check_yuv_io_values / check_yuv_io_pointers; a guide map or network's check_guide_flags / check_guide_given /
// set_io_guide_flags, the curves guide's check_curves_knots / set_curves_prepared; launch_io is the tail of all five.
// `prefix`: "" for the entry points of include/hdrnet_amd.h, whose texts predate naming the function, else "<function>: ".

// Pixel side, a frame: channel counts and the wire formats (0 f32, 1 u8, 2 u16 in; 0 f32, 1 u8 out)
int check_io_format(int input_dtype, float input_white_level, int output_dtype) {
  if (input_dtype < 0 || input_dtype > 2 || output_dtype < 0 || output_dtype > 1)
    return fail(HDRNET_INVALID_ARGUMENT, "unknown dtype code (input %d, output %d)", input_dtype, output_dtype);
  if (!(input_white_level > 0.0f)) return fail(HDRNET_INVALID_ARGUMENT, "input_white_level must be positive");
  return HDRNET_OK;
}

// ... of the entry points with a uint16 frame out (include/hdrnet_amd_u16_out.h: `output_dtype` is not an argument there):
// uint16 or float32 in, and the white level the output is scaled to
struct U16Out {
  const char* what;  // the entry point
  float white_level;
};

int check_u16_format(const U16Out& u, int input_dtype, float input_white_level) {
  if (input_dtype < 0 || input_dtype > 2)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: unknown dtype code (input %d; 0 f32, 1 u8, 2 u16)", u.what, input_dtype);
  if (input_dtype == 1)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: a uint16 output needs a uint16 or float32 frame (input_dtype 1, uint8: no "
                "kernel goes from 8 to 16 bits)", u.what);
  if (!(input_white_level > 0.0f)) return fail(HDRNET_INVALID_ARGUMENT, "%s: input_white_level must be positive", u.what);
  if (!(u.white_level > 0.0f && u.white_level <= 65535.0f))  // (false for NaN; +inf fails the upper bound)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: output_white_level must be finite with 0 < output_white_level <= 65535 (got %g)",
                u.what, (double)u.white_level);
  return HDRNET_OK;
}

// (`u16`: the call is one of those entry points; output_dtype is then the 2 they pass)
int check_frame_values(int Cin, int Cout, int input_dtype, float input_white_level, int output_dtype,
                       const U16Out* u16 = nullptr) {
  if (Cin <= 0 || Cout <= 0) return fail(HDRNET_INVALID_ARGUMENT, "bad channel counts");
  if (u16) return check_u16_format(*u16, input_dtype, input_white_level);
  return check_io_format(input_dtype, input_white_level, output_dtype);
}

// the one integer frame in, float32 out that the pyramid's resize and the low-res gather read
int check_input_dtype(const char* what, int dtype) {
  if (dtype < 0 || dtype > 2)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: unknown dtype code (input %d; 0 f32, 1 u8, 2 u16)", what, dtype);
  return HDRNET_OK;
}

// the pixel formats of include/hdrnet_amd_pixel_formats.h: integer frames take all four, float32 frames RGB only; a
// uint8 output (and a uint16 one, output_dtype 2: hdrnet_amd_u16_out.h) has the input's format, a float32 output is RGB
int check_pixel_formats(const char* what, int input_dtype, int output_dtype, int input_format, int output_format) {
  if (input_format < HDRNET_PX_RGB || input_format > HDRNET_PX_BGRA || output_format < HDRNET_PX_RGB ||
      output_format > HDRNET_PX_BGRA)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: unknown pixel format code (input %d, output %d; 0 RGB, 1 BGR, 2 RGBA, 3 BGRA)",
                what, input_format, output_format);
  if (input_dtype == 0 && input_format != HDRNET_PX_RGB)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: float32 frames take HDRNET_PX_RGB only (input_format %d); the other pixel "
                "formats are those of uint8 / uint16 frames", what, input_format);
  if (output_dtype != 0 && output_format != input_format)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: a %s output has the input's pixel format (input_format %d, output_format %d)",
                what, output_dtype == 1 ? "uint8" : "uint16", input_format, output_format);
  if (output_dtype == 0 && output_format != HDRNET_PX_RGB)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: a float32 output is [B][H][W][3] in RGB order: output_format must be "
                "HDRNET_PX_RGB (got %d)", what, output_format);
  return HDRNET_OK;
}

// ... and what a frame in another format than RGB needs of the call: the 3 -> 3 op with offset, W % 4 == 0, 4-byte
// aligned 3-channel and 16-byte aligned 4-channel integer buffers (`out`: the uint8 / uint16 output, or null)
int check_pixel_buffers(const char* what, int pixel_format, int Cin, int Cout, int has_offset, int W, const void* input,
                        const void* out) {
  if (pixel_format == HDRNET_PX_RGB) return HDRNET_OK;
  if (Cin != 3 || Cout != 3 || !has_offset)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: pixel formats other than HDRNET_PX_RGB need Cin = Cout = 3 with offset (the "
                "format says how the frame stores a pixel, not how many channels the op sees)", what);
  if (W % 4 != 0)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: W %% 4 != 0 (W=%d): a lane owns 4 pixels", what, W);
  const unsigned mask = pixel_format >= HDRNET_PX_RGBA ? 15u : 3u;
  if (((uintptr_t)input | (uintptr_t)out) & mask)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: %s", what,
                mask == 15u ? "4-channel frames (RGBA / BGRA) must be 16-B aligned (one 16-byte access per lane)"
                            : "3-channel integer frames must be 4-B aligned");
  return HDRNET_OK;
}

// Pixel side, a semi-planar YUV 4:2:0 surface (include/hdrnet_amd_yuv.h).  The rules of one surface (`which`: "input" /
// "output"), checked before any HIP call:
// (`chroma`, here and below: the surface's chroma layout, include/hdrnet_amd_yuv_chroma.h -- 4:2:2 and 4:4:4 have a chroma row
// per image row: any H, and H rows in a chroma plane)
int check_yuv_extents(const char* what, int B, int H, int W, int chroma = HDRNET_CHROMA_420) {
  if (B < 0 || H < 0 || W < 0) return fail(HDRNET_INVALID_ARGUMENT, "%s: negative image extent (B=%d, H=%d, W=%d)", what, B, H, W);
  if (chroma == HDRNET_CHROMA_420 && H % 2 != 0) return fail(HDRNET_INVALID_ARGUMENT, "%s: H %% 2 != 0 (H=%d): a chroma row serves two image rows", what, H);
  if (W % 4 != 0) return fail(HDRNET_INVALID_ARGUMENT, "%s: W %% 4 != 0 (W=%d): a lane owns 4 pixels", what, W);
  if (B > 65535 || H > 65535 || (long long)W * 12 >= (1LL << 31))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: image or batch too large (B, H <= 65535)", what);
  return HDRNET_OK;
}

int check_yuv_surface(const char* what, const char* which, int sample_dtype, const hdrnet_amd::YuvSurface& s, int B, int H,
                      int W, int chroma = HDRNET_CHROMA_420) {
  if (sample_dtype != 1 && sample_dtype != 2)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: unknown sample dtype code of the %s surface (%d; 1 u8, 2 u16)", what, which,
                sample_dtype);
  const long long row = (long long)W * sample_dtype;
  if (s.pitch_y < row || s.pitch_uv < row)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: a pitch of the %s surface is below the row's %lld bytes (pitch_y=%d, "
                "pitch_uv=%d)", what, which, row, s.pitch_y, s.pitch_uv);
  if ((s.pitch_y | s.pitch_uv) & 3)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the pitches of the %s surface must be multiples of 4 (pitch_y=%d, pitch_uv=%d)",
                what, which, s.pitch_y, s.pitch_uv);
  if (s.image_y < 0 || s.image_uv < 0 || ((s.image_y | s.image_uv) & 3))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the image strides of the %s surface must be non-negative multiples of 4", what,
                which);
  if (B > 1 && (s.image_y < (long long)s.pitch_y * H || s.image_uv < (long long)s.pitch_uv * hdrnet_amd::yuv_chroma_row(chroma, H)))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: an image stride of the %s surface is below its plane (pitch * rows)", what, which);
  return HDRNET_OK;
}

int check_yuv_pointers(const char* what, const char* which, const hdrnet_amd::YuvSurface& s, const float* coef) {
  if (!s.y || !s.uv) return fail(HDRNET_INVALID_ARGUMENT, "%s: null plane of the %s surface", what, which);
  if (!coef) return fail(HDRNET_INVALID_ARGUMENT, "%s: null constants of the %s surface (the 12 floats)", what, which);
  if (((uintptr_t)s.y | (uintptr_t)s.uv | (uintptr_t)coef) & 3u)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the planes and constants of the %s surface must be 4-B aligned", what, which);
  return HDRNET_OK;
}

// ... and of a fused forward's surfaces and output.  `io`: the call's arguments as given; io.out.y is `out` whatever the
// output kind.  `p016`: the call is an entry point of hdrnet_amd_u16_out.h, which has no output kind argument: io.out_kind
// is then kYuvOutP016 and the output a uint16 surface of io.out_bits bits.
int check_yuv_io_values(const char* what, const hdrnet_amd::YuvIo& io, int sample_dtype, int B, int H, int W, int Cin, int Cout,
                        int has_offset, bool p016 = false) {
  const bool c422 = io.chroma == HDRNET_CHROMA_422;
  if (int rc = check_yuv_extents(what, B, H, W, io.chroma)) return rc;
  if (int rc = check_yuv_surface(what, "input", sample_dtype, io.in, B, H, W, io.chroma)) return rc;
  if (p016) {
    if (sample_dtype != 2)
      return fail(HDRNET_INVALID_ARGUMENT, "%s: a %s output needs a uint16 surface in (sample_dtype 2, got %d: no "
                  "kernel goes from 8 to 16 bits)", what, c422 ? "P210 / P216" : "P010 / P016", sample_dtype);
    if (io.out_bits != 10 && io.out_bits != 16)
      return fail(HDRNET_INVALID_ARGUMENT, "%s: out_bits must be 10 (%s) or 16 (%s), got %d", what, c422 ? "P210" : "P010",
                  c422 ? "P216" : "P016", io.out_bits);
  } else if (io.out_kind < HDRNET_YUV_OUT_RGB_F32 || io.out_kind > HDRNET_YUV_OUT_NV12) {
    return fail(HDRNET_INVALID_ARGUMENT, "%s: unknown output kind %d (0 float32 RGB, 1 uint8 RGB, 2 NV12)", what, io.out_kind);
  }
  if (Cin != 3 || Cout != 3 || !has_offset)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: a YUV surface needs Cin = Cout = 3 with offset (the op sees R, G, B)", what);
  if (p016) return check_yuv_surface(what, "output", 2, io.out, B, H, W, io.chroma);
  if (io.out_kind == HDRNET_YUV_OUT_NV12) return check_yuv_surface(what, "output", 1, io.out, B, H, W, io.chroma);
  return HDRNET_OK;
}

int check_yuv_io_pointers(const char* what, const hdrnet_amd::YuvIo& io) {
  if (int rc = check_yuv_pointers(what, "input", io.in, io.to_rgb)) return rc;
  if (io.out_kind == HDRNET_YUV_OUT_NV12 || io.out_kind == hdrnet_amd::kYuvOutP016)
    return check_yuv_pointers(what, "output", io.out, io.from_rgb);
  if (!io.out.y || ((uintptr_t)io.out.y & (io.out_kind == HDRNET_YUV_OUT_RGB_F32 ? 15u : 3u)))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: null or misaligned out (float32 frames 16-B, uint8 frames 4-B aligned)", what);
  return HDRNET_OK;
}

// Pixel side, a PLANAR YUV 4:2:0 surface (include/hdrnet_amd_yuv_planar.h): the extents are check_yuv_extents'; each rule of
// a surface is stated once below and shared by the four entry points (`which`: "input" / "output").
int check_yuv_planar_surface(const char* what, const char* which, int sample_dtype, const hdrnet_amd::YuvPlanarSurface& s, int B,
                             int H, int W, int chroma = HDRNET_CHROMA_420) {
  if (sample_dtype != 1 && sample_dtype != 2)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: unknown sample dtype code of the %s surface (%d; 1 u8, 2 u16)", what, which,
                sample_dtype);
  const bool c444 = chroma == HDRNET_CHROMA_444;  // a chroma plane as wide as the luma: the luma's rules
  const long long row = (long long)W * sample_dtype, crow = c444 ? row : row / 2;
  if (s.pitch_y < row || s.pitch_u < crow || s.pitch_v < crow)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: a pitch of the %s surface is below the row's bytes (%lld luma, %lld chroma; "
                "pitch_y=%d, pitch_u=%d, pitch_v=%d)", what, which, row, crow, s.pitch_y, s.pitch_u, s.pitch_v);
  // a lane touches 4 luma samples (dwords) and 2 samples of each chroma plane: 2 bytes of uint8, 4 of uint16
  // (4:4:4: 4 samples of each chroma plane, whole dwords)
  const int cmask = sample_dtype == 1 && !c444 ? 1 : 3;
  const char* const ckind = c444 ? "4:4:4" : sample_dtype == 1 ? "uint8" : "uint16";
  if ((s.pitch_y & 3) || ((s.pitch_u | s.pitch_v) & cmask))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the pitches of the %s surface must be multiples of 4 (luma) and of %d (%s chroma) "
                "(pitch_y=%d, pitch_u=%d, pitch_v=%d)", what, which, cmask + 1, ckind, s.pitch_y, s.pitch_u, s.pitch_v);
  if (s.image_y < 0 || s.image_u < 0 || s.image_v < 0 || (s.image_y & 3) || ((s.image_u | s.image_v) & cmask))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the image strides of the %s surface must be non-negative multiples of 4 (luma) and "
                "of %d (%s chroma)", what, which, cmask + 1, ckind);
  const int crows = hdrnet_amd::yuv_chroma_row(chroma, H);
  if (B > 1 && (s.image_y < (long long)s.pitch_y * H || s.image_u < (long long)s.pitch_u * crows ||
                s.image_v < (long long)s.pitch_v * crows))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: an image stride of the %s surface is below its plane (pitch * rows)", what, which);
  return HDRNET_OK;
}

int check_yuv_planar_pointers(const char* what, const char* which, int sample_dtype, const hdrnet_amd::YuvPlanarSurface& s,
                              const float* coef, int chroma = HDRNET_CHROMA_420) {
  if (!s.y || !s.u || !s.v) return fail(HDRNET_INVALID_ARGUMENT, "%s: null plane of the %s surface", what, which);
  if (!coef) return fail(HDRNET_INVALID_ARGUMENT, "%s: null constants of the %s surface (the 12 floats)", what, which);
  if (((uintptr_t)s.y | (uintptr_t)coef) & 3u)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the Y plane and constants of the %s surface must be 4-B aligned", what, which);
  if (chroma == HDRNET_CHROMA_444 && (((uintptr_t)s.u | (uintptr_t)s.v) & 3u))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the chroma planes of the %s surface must be 4-B aligned (4:4:4: a lane touches 4 "
                "samples of each, as of the luma)", what, which);
  if (((uintptr_t)s.u | (uintptr_t)s.v) & (sample_dtype == 1 ? 1u : 3u))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the chroma planes of the %s surface must be %d-B aligned (%s samples: a lane "
                "touches 2 of them)", what, which, sample_dtype == 1 ? 2 : 4, sample_dtype == 1 ? "uint8" : "uint16");
  return HDRNET_OK;
}

// ... and of a fused forward's surfaces and output.  io.out.y is `out` whatever the output kind.
int check_yuv_planar_io_values(const char* what, const hdrnet_amd::YuvPlanarIo& io, int sample_dtype, int B, int H, int W,
                               int Cin, int Cout, int has_offset) {
  if (int rc = check_yuv_extents(what, B, H, W, io.chroma)) return rc;
  if (int rc = check_yuv_planar_surface(what, "input", sample_dtype, io.in, B, H, W, io.chroma)) return rc;
  if (io.out_kind < HDRNET_YUV_PLANAR_OUT_RGB_F32 || io.out_kind > HDRNET_YUV_PLANAR_OUT_PLANAR)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: unknown output kind %d (0 float32 RGB, 1 uint8 RGB, 2 a planar surface of the "
                "input's sample dtype)", what, io.out_kind);
  if (Cin != 3 || Cout != 3 || !has_offset)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: a YUV surface needs Cin = Cout = 3 with offset (the op sees R, G, B)", what);
  if (io.out_kind != HDRNET_YUV_PLANAR_OUT_PLANAR) return HDRNET_OK;
  if (sample_dtype == 1 ? io.out_bits != 8 : (io.out_bits != 10 && io.out_bits != 16))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: out_bits does not fit the sample dtype: a planar output has the input's (uint8 "
                "samples: 8; uint16 samples: 10 or 16; got out_bits = %d for sample_dtype %d)", what, io.out_bits, sample_dtype);
  return check_yuv_planar_surface(what, "output", sample_dtype, io.out, B, H, W, io.chroma);
}

int check_yuv_planar_io_pointers(const char* what, const hdrnet_amd::YuvPlanarIo& io, int sample_dtype) {
  if (int rc = check_yuv_planar_pointers(what, "input", sample_dtype, io.in, io.to_rgb, io.chroma)) return rc;
  if (io.out_kind == HDRNET_YUV_PLANAR_OUT_PLANAR)
    return check_yuv_planar_pointers(what, "output", sample_dtype, io.out, io.from_rgb, io.chroma);
  if (!io.out.y || ((uintptr_t)io.out.y & (io.out_kind == HDRNET_YUV_PLANAR_OUT_RGB_F32 ? 15u : 3u)))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: null or misaligned out (float32 frames 16-B, uint8 frames 4-B aligned)", what);
  return HDRNET_OK;
}

// Guide side, a map or the network.  Here the map wins over a network given beside it (the up-add entry points refuse
// that: check_upadd_values), so with a map there is nothing to prescale: the refusal's Cin is then 0.
int check_guide_given(const char* prefix, const float* guide, const float* conv1, const float* conv2, int n_feats) {
  if (!guide && (!conv1 || !conv2 || n_feats <= 0 || n_feats > 4096))
    return fail(HDRNET_INVALID_ARGUMENT, "%seither a guide map or the guide network must be given", prefix);
  return HDRNET_OK;
}

int set_io_guide_flags(hdrnet_amd::ApplyIoArgs& a, unsigned flags) {
  const bool network = !a.guide;
  return set_guide_flags(a, flags, network ? a.Cin : 0, network ? a.guide_conv1 : nullptr, network ? a.guide_conv2 : nullptr);
}

// Guide side, the curves: the knots, and the cell tables of hdrnet_curves_guide_prepare_f32 where given.  One rule with
// two texts: a YUV surface has refused Cin != 3 by then, so its text does not name it.
int check_curves_knots(const char* prefix, int npts) {
  if (npts <= 0 || npts > 4096) return fail(HDRNET_INVALID_ARGUMENT, "%sbad number of curve knots (%d)", prefix, npts);
  return HDRNET_OK;
}

int set_curves_prepared(hdrnet_amd::ApplyIoArgs& a, const void* prepared, const char* prefix, const char* needs) {
  if (!prepared) return HDRNET_OK;
  if (((uintptr_t)prepared & 15u) || a.Cin != 3 || a.n_feats > 16)
    return fail(HDRNET_INVALID_ARGUMENT, "%sprepared curves tables need %s and the 16-B aligned buffer "
                                         "hdrnet_curves_guide_prepare_f32 wrote (and reported usable)", prefix, needs);
  a.guide_prepared = static_cast<const float*>(prepared);
  return HDRNET_OK;
}

// The tail: the call's kernel family (apply_fwd_io.hip chooses it; `coarse`: the pyramid's up-add), `otherwise` what the
// entry point supports, `op` its name in a runtime failure.
int launch_io(const hdrnet_amd::ApplyIoArgs& a, const float* coarse, int Hc, int Wc, const char* op, const char* otherwise,
              void* stream) {
  using namespace hdrnet_amd;
  if (!apply_fwd_io_family_supported(a, coarse))
    return refuse_fused(a.B, a.H, a.W, a.GW, a.GD, a.Cout, rows::kSegLimits, otherwise);
  const char* name = "";
  const hipError_t e = launch_apply_fwd_io_family(a, coarse, Hc, Wc, static_cast<hipStream_t>(stream), &name);
  return finish_launch(e, op, name);
}

// any parameter the coefficient network reads (and, for the gradient, any it writes) missing?
bool coeff_net_null_param(const hdrnet_coeff_net& net, const hdrnet_coeff_net_grads* grads) {
  int n_ds = 0;
  for (int v = net.net_input_size / net.spatial_bin; v > 1; v >>= 1) ++n_ds;
  const auto scan = [n_ds](const auto& p) {
    bool null_param = !p.pred_w || !p.pred_b || !p.local_w[0] || !p.local_w[1] || !p.local_b[0];
    for (int i = 0; i < n_ds; ++i) null_param = null_param || !p.splat_w[i] || !p.splat_b[i];
    for (int i = 0; i < 2; ++i) null_param = null_param || !p.global_conv_w[i] || !p.global_conv_b[i];
    for (int i = 0; i < 3; ++i) null_param = null_param || !p.fc_w[i] || !p.fc_b[i];
    return null_param;
  };
  return scan(net) || (grads && scan(*grads));
}

// the batch-norm description: why a call cannot run (null: it can).  `grads`: also check where the gradients go.
// `max_b`: the entry point's largest batch (8, or 32 for the ..._wide ones).
const char* coeff_net_bn_refusal(const hdrnet_coeff_net_bn& bn, const hdrnet_coeff_net_bn_grads* grads, int B, int max_b) {
  using namespace hdrnet_amd;
  const hdrnet_coeff_net& net = bn.net;
  if (coefficients_bn_workspace_bytes(net, B, max_b) == 0 || coefficients_bn_grad_workspace_bytes(net, B, max_b) == 0)
    return max_b > kCoeffNarrowMaxB
               ? "unsupported (needs what hdrnet_coefficients_grad_wide_f32 supports, 2 <= B <= 32, n_levels = 1, fc_layout = 1)"
               : "unsupported (needs what hdrnet_coefficients_grad_f32 supports, 2 <= B <= 8, n_levels = 1, fc_layout = 1)";
  int n_ds = 0;
  for (int v = net.net_input_size / net.spatial_bin; v > 1; v >>= 1) ++n_ds;
  bool null_param = !net.pred_w || !net.pred_b || !net.local_w[0] || !net.local_w[1] || !net.splat_b[0] || !net.fc_b[2];
  for (int i = 0; i < n_ds; ++i) null_param = null_param || !net.splat_w[i];
  for (int i = 0; i < 2; ++i) null_param = null_param || !net.global_conv_w[i];
  for (int i = 0; i < 3; ++i) null_param = null_param || !net.fc_w[i];
  if (null_param) return "null parameter";
  bool null_bn = !bn.local_beta || !bn.local_running_mean || !bn.local_running_var;
  for (int i = 1; i < n_ds; ++i)
    null_bn = null_bn || !bn.splat_beta[i] || !bn.splat_running_mean[i] || !bn.splat_running_var[i];
  for (int i = 0; i < 2; ++i)
    null_bn = null_bn || !bn.global_conv_beta[i] || !bn.global_conv_running_mean[i] || !bn.global_conv_running_var[i] ||
              !bn.fc_beta[i] || !bn.fc_running_mean[i] || !bn.fc_running_var[i];
  if (null_bn) return "null beta, running_mean or running_var of a normalised layer";
  if (!(bn.eps > 0.0f) || !(bn.momentum >= 0.0f && bn.momentum <= 1.0f)) return "eps must be positive and momentum in [0, 1]";
  if (grads) {
    const hdrnet_coeff_net_grads& g = grads->net;
    bool null_grad = !g.pred_w || !g.pred_b || !g.local_w[0] || !g.local_w[1] || !g.splat_b[0] || !g.fc_b[2] || !grads->local_beta;
    for (int i = 0; i < n_ds; ++i) null_grad = null_grad || !g.splat_w[i] || (i > 0 && !grads->splat_beta[i]);
    for (int i = 0; i < 2; ++i) null_grad = null_grad || !g.global_conv_w[i] || !grads->global_conv_beta[i] || !grads->fc_beta[i];
    for (int i = 0; i < 3; ++i) null_grad = null_grad || !g.fc_w[i];
    if (null_grad) return "null gradient";
  }
  return nullptr;
}

int check_flags(unsigned flags) {
  if ((flags & 0xffu) > HDRNET_KERNEL_FAST || (flags >> 16) != 0)
    return fail(HDRNET_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
#ifndef HDRNET_TOOLS_BUILD
  if ((flags >> 8) != 0)
    return fail(HDRNET_INVALID_ARGUMENT,
                "kernel variants (flags bits 8..15) exist only in the tools build "
                "(libhdrnet_amd_tools.so), flags 0x%x", flags);
#endif
  return HDRNET_OK;
}
unsigned family(unsigned flags) { return flags & 0xffu; }
int variant(unsigned flags) { return (int)((flags >> 8) & 0xffu); }

// Both gradient entry points, once their own arguments are checked: the legal no-ops, then the ladder -- all gradients
// from ONE pass over the pixels (fused), else dguide / dinput on the per-pixel fast kernel and dgrid on the MFMA
// contraction, and what neither took on the op's generic kernel.  `family`: HDRNET_KERNEL_*.
int grad_dispatch(const hdrnet_amd::ApplyGradArgs& a, unsigned family, hipStream_t s) {
  using namespace hdrnet_amd;
  const char* what = a.slice ? "BilateralSliceGrad" : "BilateralSliceApplyGrad";
#ifdef HDRNET_TOOLS_BUILD
  // an A/B script must not time the product pass against itself under a number whose kernel is gone
  if (a.variant != 0 && a.variant != 3 && a.variant != 11)
    return fail(HDRNET_INVALID_ARGUMENT,
                "gradient kernel variant %d is not in this library: variants 2 and 4..10 were retired with their "
                "kernels, 0, 3 and 11 remain (include/hdrnet_amd_tools.h)", a.variant);
#endif
  if (!a.dgrid && !a.dguide && !a.dinput) return finish_noop();
  const long long npix = (long long)a.B * a.H * a.W;
  if (npix == 0) {
    // Gradients of an empty image: dgrid is all zeros, the others are empty.
    if (a.dgrid && a.B > 0) {
      const hipError_t e =
          hipMemsetAsync(a.dgrid, 0, sizeof(float) * (size_t)a.B * a.GH * a.GW * a.GD * a.Cout * a.Cj, s);
      if (e != hipSuccess) return finish_launch(e, what, nullptr);
    }
    return finish_noop();
  }
  if (!a.guide || !a.dout || (a.Cin > 0 && !a.input) || ((a.dguide || a.dinput) && !a.grid))
    return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  // (tools variant 3: the un-fused kernels)
  if (family != HDRNET_KERNEL_GENERIC && a.variant != 3 && bwd_fused_supported(a)) {
    const char* name = "";
    const hipError_t e = launch_bwd_fused(a, s, &name);
    return finish_launch(e, what, name);
  }
  const bool pix_fast = family != HDRNET_KERNEL_GENERIC && (a.dguide || a.dinput) && vjp_rows_supported(a);
  if (family == HDRNET_KERNEL_FAST && (a.dguide || a.dinput) && !pix_fast)
    return fail(HDRNET_INVALID_ARGUMENT, "no fast %s variant for this shape", what);
  const char *pix_name = "", *gg_name = "", *rest_name = "";
  ApplyGradArgs rest = a;
  if (pix_fast) {
    if (int rc = finish_launch(launch_vjp_rows(a, s, &pix_name), what, nullptr)) return rc;
    rest.dguide = nullptr;
    rest.dinput = nullptr;
  }
  if (a.dgrid && family != HDRNET_KERNEL_GENERIC) {
    if (grid_grad_mfma_supported(a)) {
      if (int rc = finish_launch(launch_grid_grad_mfma(a, s, &gg_name), what, nullptr)) return rc;
      rest.dgrid = nullptr;
    } else if (family == HDRNET_KERNEL_FAST) {
      return fail(HDRNET_INVALID_ARGUMENT,
                  "no fast grid-gradient variant for this shape (or workspace missing / too small)");
    }
  }
  if (rest.dgrid || rest.dguide || rest.dinput) {
    if (npix > kGenericMaxPixels) return refuse_generic(what, npix);
    if (rest.dgrid && family == HDRNET_KERNEL_AUTO && npix > kWarnGenericPixels)
      warn_generic_grid_grad(what, npix, a.GD, a.Cout * a.Cj, /*no_fast_shape=*/!grad_fast_shape(a) ||
                             grid_grad_mfma_workspace(a.B, a.H, a.W, a.GH, a.GW, a.GD, a.Cout * a.Cj) == 0);
    const hipError_t e = a.slice ? launch_slice_grad_generic(rest, s) : launch_apply_grad_generic(rest, s);
    if (int rc = finish_launch(e, what, nullptr)) return rc;
    rest_name = a.slice ? "slice_grad_generic" : "apply_grad_generic";
  }
  set_kernel(pix_name, gg_name, rest_name);
  return HDRNET_OK;
}

}  // namespace

extern "C" {

// 0.2.4.1: + hdrnet_guide_nn_prescale_f32 / HDRNET_GUIDE_RELU_PRESCALED, hdrnet_curves_guide_prepare_f32 (with `usable`) /
//          ..._io_curves_prepared; the non-_ex guide-network entry points use the exact sigmoid (flags = 0)
// 0.2.5.0: the gradient entry points take grids of up to 16 planes on the fast pass (the workspace bound grows with it:
//          query ..._grad_workspace_bytes again); one stderr line when a frame-sized dgrid falls back to the generic kernel
// 0.2.5.1: 4 -> 4 with offset (C = 20): dgrid on the contraction pass as two channel windows (the workspace bound doubles
//          for that shape: query again); apply_vjp_seg's dguide in the z-difference form (bits change; closer to float64)
// 0.2.6.0: + hdrnet_prepare_batch (include/hdrnet_amd_train.h), hdrnet_lowres_input: sample preparation from u8 / u16 / f32
// 0.2.7.0: + hdrnet_prepare_batch_ragged (include/hdrnet_amd_train.h): sample preparation from a packed set of images of
//          mixed extents
// 0.2.8.1: the training-loop entry points of include/hdrnet_amd_train.h set / clear hdrnet_last_error() like the rest
// 0.2.8.2: the coefficient network's entry points refuse widths their kernels cannot run (workspace queries return 0
//          where 281 returned a size: include/hdrnet_amd.h)
// 0.2.8.5: + include/hdrnet_amd_pyramid_io.h: hdrnet_resize_bilinear_io, hdrnet_bilateral_slice_apply_upadd_io_ex (the
//          pyramid model's wire formats)
// 0.2.8.6: + include/hdrnet_amd_pixel_formats.h: hdrnet_lowres_input_px, hdrnet_bilateral_slice_apply_io_px,
//          hdrnet_bilateral_slice_apply_io_curves_px (uint8 / uint16 frames in BGR, RGBA and BGRA order)
// 0.2.8.7: + include/hdrnet_amd_yuv.h: hdrnet_yuv_to_rgb_f32, hdrnet_lowres_input_yuv, hdrnet_bilateral_slice_apply_io_yuv,
//          hdrnet_bilateral_slice_apply_io_curves_yuv (NV12 / P010 / P016 surfaces in, RGB or NV12 out)
// 0.2.8.9: + include/hdrnet_amd_yuv_planar.h: hdrnet_yuv_planar_to_rgb_f32, hdrnet_lowres_input_yuv_planar,
//          hdrnet_bilateral_slice_apply_io_yuv_planar, hdrnet_bilateral_slice_apply_io_curves_yuv_planar (I420 / yuv420p10le /
//          yuv420p16le surfaces in, RGB or a planar surface out)
// 0.2.9.0: + include/hdrnet_amd_yuv_chroma.h: the eight entry points of the three headers above with a `chroma` argument (4:2:2
//          NV16 / P210 / P216 / yuv422p..., 4:4:4 yuv444p... surfaces in, RGB or a surface of the input's container and layout out)
// 0.2.9.2: + include/hdrnet_amd_yuv_packed.h: hdrnet_yuv_packed_to_rgb_f32, hdrnet_lowres_input_yuv_packed,
//          hdrnet_bilateral_slice_apply_io_yuv_packed, hdrnet_bilateral_slice_apply_io_curves_yuv_packed (YUY2 / UYVY / YVYU /
//          Y210 / Y216 surfaces in, RGB or a packed surface of the input's width and order out)
int hdrnet_version(void) { return 292; }

const char* hdrnet_last_error(void) { return g_error; }

const char* hdrnet_last_kernel(void) { return g_kernel_buf; }

void hdrnet_enable_kernel_names(int on) { g_kernel_names.store(on ? 1 : 0, std::memory_order_relaxed); }

#ifdef HDRNET_TOOLS_BUILD
// tools build only (include/hdrnet_amd_tools.h)
void hdrnet_tools_set_knob(int idx, int value) { hdrnet_amd::tools_set_knob(idx, value); }

void hdrnet_tools_set_trace(void* device_buf) { hdrnet_amd::coeff_net_set_trace(static_cast<long long*>(device_buf)); }
#endif

// Forward, whole frames (H_total = rows, y0 = 0) or one row band of every frame.
static int apply_fwd_impl(const float* grid, const float* guide, const float* input, float* out, int B,
                          int H_total, int y0, int H, int W, int GH, int GW, int GD, int Cin, int Cout,
                          int has_offset, unsigned flags, void* stream) {
  using namespace hdrnet_amd;
  if (int rc = check_common(B, H, W, GH, GW, GD)) return rc;
  if (int rc = check_flags(flags)) return rc;
#ifdef HDRNET_TOOLS_BUILD
  // an A/B script must not time the product kernel against itself under a number whose kernel is gone
  const int v = variant(flags);
  if (v != 0 && v != 19 && v != 106 && v != 108)
    return fail(HDRNET_INVALID_ARGUMENT,
                "forward kernel variant %d is not in this library: variants 2..11, 101, 103..105 and 107 were retired "
                "with their kernels, 0, 19, 106 and 108 remain (include/hdrnet_amd_tools.h)", v);
#endif
  if (H_total < 0 || y0 < 0 || (long long)y0 + H > H_total)
    return fail(HDRNET_INVALID_ARGUMENT, "row band [%d, %d + %d) outside the frame's %d rows", y0, y0, H, H_total);
  const bool band = y0 != 0 || H != H_total;
  if (band && variant(flags) != 0)
    return fail(HDRNET_INVALID_ARGUMENT, "kernel variants take whole frames");
  if (Cin < 0 || Cout <= 0 || Cin + (has_offset ? 1 : 0) <= 0)
    return fail(HDRNET_INVALID_ARGUMENT,
                "grid should have output_channels * (input_channels%s) channels "
                "(Cin=%d, Cout=%d)", has_offset ? " + 1" : "", Cin, Cout);
  const long long npix = (long long)B * H * W;
  if (npix == 0) return finish_noop();
  if (!grid || !guide || !out || (Cin > 0 && !input))
    return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  ApplyArgs a{grid, guide, input, out, B, H, W, GH, GW, GD, Cin, Cout,
              Cin + (has_offset ? 1 : 0), has_offset != 0, variant(flags)};
  a.y0 = y0;
  a.H_total = H_total;
  hipStream_t s = static_cast<hipStream_t>(stream);
#ifdef HDRNET_TOOLS_BUILD
  // the memory skeletons (whatever the family): their own kernel or a refusal, never the product under their number
  if (v == 106 || v == 108) {
    if (!apply_fwd_skeleton_supported(a))
      return fail(HDRNET_INVALID_ARGUMENT,
                  "forward kernel variant %d has no kernel for this shape: the memory skeletons take 3 -> 3 with offset, "
                  "W %% 4 == 0 and 16-byte aligned buffers (include/hdrnet_amd_tools.h)", v);
    const char* name = "";
    const hipError_t e = launch_apply_fwd_skeleton(a, s, &name);
    return finish_launch(e, "BilateralSliceApply", name);
  }
#endif
  // a row band runs on the row-segment kernel (apply_fwd_seg.hip) or the generic one; whole frames may
  // also take the scalar row kernel (unaligned buffers, W % 4 != 0)
  const bool fast_ok = band ? apply_fwd_seg_supported(a) : apply_fwd_rows_supported(a);
  if (family(flags) == HDRNET_KERNEL_FAST && !fast_ok)
    return fail(HDRNET_INVALID_ARGUMENT, "no fast BilateralSliceApply variant for this shape");
  if (family(flags) != HDRNET_KERNEL_GENERIC && fast_ok) {
    const char* name = "";
    const hipError_t e = band ? launch_apply_fwd_seg(a, s, &name) : launch_apply_fwd_rows(a, s, &name);
    return finish_launch(e, "BilateralSliceApply", name);
  }
  if (npix > kGenericMaxPixels) return refuse_generic("BilateralSliceApply", npix);
  return finish_launch(launch_apply_fwd_generic(a, s), "BilateralSliceApply", "apply_fwd_generic");
}

int hdrnet_bilateral_slice_apply_f32_ex(const float* grid, const float* guide,
                                        const float* input, float* out, int B, int H, int W,
                                        int GH, int GW, int GD, int Cin, int Cout,
                                        int has_offset, unsigned flags, void* stream) {
  return apply_fwd_impl(grid, guide, input, out, B, H, 0, H, W, GH, GW, GD, Cin, Cout, has_offset, flags,
                        stream);
}

int hdrnet_bilateral_slice_apply_rows_f32_ex(const float* grid, const float* guide, const float* input,
                                             float* out, int B, int H_total, int y0, int rows, int W,
                                             int GH, int GW, int GD, int Cin, int Cout, int has_offset,
                                             unsigned flags, void* stream) {
  return apply_fwd_impl(grid, guide, input, out, B, H_total, y0, rows, W, GH, GW, GD, Cin, Cout, has_offset,
                        flags, stream);
}

int hdrnet_bilateral_slice_apply_rows_f32(const float* grid, const float* guide, const float* input,
                                          float* out, int B, int H_total, int y0, int rows, int W, int GH,
                                          int GW, int GD, int Cin, int Cout, int has_offset, void* stream) {
  return apply_fwd_impl(grid, guide, input, out, B, H_total, y0, rows, W, GH, GW, GD, Cin, Cout, has_offset,
                        HDRNET_KERNEL_AUTO, stream);
}

int hdrnet_bilateral_slice_apply_f32(const float* grid, const float* guide, const float* input,
                                     float* out, int B, int H, int W, int GH, int GW, int GD,
                                     int Cin, int Cout, int has_offset, void* stream) {
  return hdrnet_bilateral_slice_apply_f32_ex(grid, guide, input, out, B, H, W, GH, GW, GD, Cin,
                                             Cout, has_offset, HDRNET_KERNEL_AUTO, stream);
}

int hdrnet_bilateral_slice_apply_nnguide_f32(const float* grid, const float* input,
                                             const float* guide_conv1, const float* guide_conv2,
                                             float* out, float* guide_out, int B, int H, int W,
                                             int GH, int GW, int GD, int Cin, int Cout,
                                             int has_offset, int n_feats, void* stream) {
  return hdrnet_bilateral_slice_apply_nnguide_f32_ex(grid, input, guide_conv1, guide_conv2, out, guide_out, B, H, W,
                                                     GH, GW, GD, Cin, Cout, has_offset, n_feats, 0u, stream);
}

int hdrnet_bilateral_slice_apply_nnguide_f32_ex(const float* grid, const float* input,
                                                const float* guide_conv1, const float* guide_conv2,
                                                float* out, float* guide_out, int B, int H, int W,
                                                int GH, int GW, int GD, int Cin, int Cout,
                                                int has_offset, int n_feats, unsigned flags, void* stream) {
  using namespace hdrnet_amd;
  if (int rc = check_common(B, H, W, GH, GW, GD)) return rc;
  if (int rc = check_guide_flags(flags)) return rc;
  if (Cin <= 0 || Cout <= 0 || n_feats <= 0 || n_feats > 4096)
    return fail(HDRNET_INVALID_ARGUMENT, "bad channel / feature counts (Cin=%d, Cout=%d, n=%d)", Cin,
                Cout, n_feats);
  if ((long long)B * H * W == 0) return finish_noop();
  if (!grid || !input || !out || !guide_conv1 || !guide_conv2)
    return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  ApplyArgs a{grid, nullptr, input, out, B, H, W, GH, GW, GD, Cin, Cout,
              Cin + (has_offset ? 1 : 0), has_offset != 0, 0};
  if (int rc = set_guide_flags(a, flags, Cin, guide_conv1, guide_conv2)) return rc;
  if (!apply_fwd_nnguide_supported(a, guide_out))
    return refuse_fused(B, H, W, GW, GD, Cin > Cout ? Cin : Cout, rows::kNeedVec4 | rows::kRowsLimits,
                        "fused guide + slice-apply needs (Cin, Cout) in {(3,3), (1,1)}, W % 4 == 0 and 16-B "
                        "aligned buffers; run the guide network and hdrnet_bilateral_slice_apply_f32 instead");
  const char* name = "";
  const hipError_t e = launch_apply_fwd_nnguide(a, guide_conv1, guide_conv2, n_feats, guide_out,
                                                static_cast<hipStream_t>(stream), &name);
  return finish_launch(e, "BilateralSliceApplyNNGuide", name);
}

int hdrnet_bilateral_slice_apply_upadd_f32(const float* grid, const float* guide, const float* input,
                                           const float* coarse, int Hc, int Wc, float* out, int B,
                                           int H, int W, int GH, int GW, int GD, int Cin, int Cout,
                                           int has_offset, const float* guide_conv1,
                                           const float* guide_conv2, int n_feats, void* stream) {
  return hdrnet_bilateral_slice_apply_upadd_f32_ex(grid, guide, input, coarse, Hc, Wc, out, B, H, W, GH, GW, GD, Cin,
                                                   Cout, has_offset, guide_conv1, guide_conv2, n_feats, 0u, stream);
}

int hdrnet_bilateral_slice_apply_upadd_f32_ex(const float* grid, const float* guide, const float* input,
                                              const float* coarse, int Hc, int Wc, float* out, int B,
                                              int H, int W, int GH, int GW, int GD, int Cin, int Cout,
                                              int has_offset, const float* guide_conv1,
                                              const float* guide_conv2, int n_feats, unsigned flags,
                                              void* stream) {
  using namespace hdrnet_amd;
  if (int rc = check_common(B, H, W, GH, GW, GD)) return rc;
  if (int rc = check_guide_flags(flags)) return rc;
  if (Cin <= 0 || Cout <= 0) return fail(HDRNET_INVALID_ARGUMENT, "bad channel counts");
  if (int rc = check_upadd_values(Hc, Wc, guide, guide_conv1, guide_conv2, n_feats)) return rc;
  if ((long long)B * H * W == 0) return finish_noop();
  if (!grid || !input || !out || !coarse) return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  ApplyArgs a{grid, guide, input, out, B, H, W, GH, GW, GD, Cin, Cout,
              Cin + (has_offset ? 1 : 0), has_offset != 0, 0};
  if (int rc = set_guide_flags(a, flags, Cin, guide_conv1, guide_conv2)) return rc;
  if (!apply_fwd_upadd_supported(a, coarse, guide_conv1 != nullptr))
    return refuse_fused(B, H, W, GW, GD, Cin > Cout ? Cin : Cout, rows::kNeedVec4 | rows::kRowsLimits,
                        "slice-apply + up-add needs Cin = Cout = 3 with offset, W % 4 == 0 and 16-B aligned "
                        "buffers; compose hdrnet_bilateral_slice_apply_f32 and hdrnet_resize_bilinear_f32 instead");
  const char* name = "";
  const hipError_t e = launch_apply_fwd_upadd(a, coarse, Hc, Wc, guide_conv1, guide_conv2, n_feats,
                                              static_cast<hipStream_t>(stream), &name);
  return finish_launch(e, "BilateralSliceApplyUpAdd", name);
}

int hdrnet_resize_bilinear_f32(const float* in, float* out, int B, int Hin, int Win, int Hout, int Wout,
                               int C, void* stream) {
  using namespace hdrnet_amd;
  if (B < 0 || Hin <= 0 || Win <= 0 || Hout < 0 || Wout < 0 || C <= 0)
    return fail(HDRNET_INVALID_ARGUMENT, "bad extents (B=%d, in %dx%d, out %dx%d, C=%d)", B, Hin, Win, Hout,
                Wout, C);
  if ((long long)B * Hout * Wout == 0) return finish_noop();
  if (!in || !out) return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  const char* name = "";
  const hipError_t e = launch_resize_bilinear(in, out, B, Hin, Win, Hout, Wout, C, static_cast<hipStream_t>(stream),
                                              &name);
  return finish_launch(e, "ResizeBilinear", name);
}

size_t hdrnet_pointwise_guide_grad_workspace_bytes(long long npx, int Cin, int n_feats) {
  if (npx <= 0) return 0;
  return hdrnet_amd::guide_grad_workspace_bytes(npx, Cin, n_feats);
}

int hdrnet_pointwise_guide_grad_f32(const float* input, const float* guide, const float* dguide,
                                    const float* guide_conv1, const float* guide_conv2,
                                    float* dinput, int accumulate_dinput, float* dconv1,
                                    float* dconv2, long long npx, int Cin, int n_feats,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  using namespace hdrnet_amd;
  if (npx < 0 || Cin <= 0 || n_feats <= 0)
    return fail(HDRNET_INVALID_ARGUMENT, "bad sizes (npx=%lld, Cin=%d, n=%d)", npx, Cin, n_feats);
  if (!dconv1 || !dconv2 || !guide_conv1 || !guide_conv2)
    return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (npx == 0) {  // no pixels: zero parameter gradients
    hipError_t e = hipMemsetAsync(dconv1, 0, sizeof(float) * (size_t)n_feats * (Cin + 1), s);
    if (e == hipSuccess) e = hipMemsetAsync(dconv2, 0, sizeof(float) * (size_t)(n_feats + 1), s);
    return finish_launch(e, "PointwiseGuideGrad", "noop");
  }
  if (!input || !guide || !dguide) return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  GuideGradArgs a{input, guide, dguide, guide_conv1, guide_conv2, dinput, accumulate_dinput != 0,
                  dconv1, dconv2, npx, Cin, n_feats, workspace, workspace_bytes};
  if (!guide_grad_supported(a))
    return fail(HDRNET_INVALID_ARGUMENT,
                "guide-network gradient needs Cin in {1,3}, n_feats in {4,8,16}, 16-B aligned buffers "
                "and a workspace of hdrnet_pointwise_guide_grad_workspace_bytes()");
  const char* name = "";
  const hipError_t e = launch_guide_grad(a, s, &name);
  return finish_launch(e, "PointwiseGuideGrad", name);
}

size_t hdrnet_curves_guide_grad_workspace_bytes(long long npx, int Cin, int npts) {
  if (npx <= 0) return 0;
  return hdrnet_amd::curves_grad_workspace_bytes(npx, Cin, npts);
}

int hdrnet_curves_guide_grad_f32(const float* input, const float* dguide, const float* guide_ccm,
                                 const float* guide_shifts, const float* guide_slopes,
                                 const float* guide_mix, float* dinput, int accumulate_dinput,
                                 float* dccm, float* dshifts, float* dslopes, float* dmix, long long npx,
                                 int Cin, int npts, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  using namespace hdrnet_amd;
  if (npx < 0 || Cin <= 0 || npts <= 0)
    return fail(HDRNET_INVALID_ARGUMENT, "bad sizes (npx=%lld, Cin=%d, npts=%d)", npx, Cin, npts);
  if (!dccm || !dshifts || !dslopes || !dmix || !guide_ccm || !guide_shifts || !guide_slopes || !guide_mix)
    return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (npx == 0) {  // no pixels: zero parameter gradients
    hipError_t e = hipMemsetAsync(dccm, 0, sizeof(float) * (size_t)Cin * (Cin + 1), s);
    if (e == hipSuccess) e = hipMemsetAsync(dshifts, 0, sizeof(float) * (size_t)npts * Cin, s);
    if (e == hipSuccess) e = hipMemsetAsync(dslopes, 0, sizeof(float) * (size_t)npts * Cin, s);
    if (e == hipSuccess) e = hipMemsetAsync(dmix, 0, sizeof(float) * (size_t)(Cin + 1), s);
    return finish_launch(e, "CurvesGuideGrad", "noop");
  }
  if (!input || !dguide) return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  CurvesGradArgs a{input, dguide, guide_ccm, guide_shifts, guide_slopes, guide_mix, dinput,
                   accumulate_dinput != 0, dccm, dshifts, dslopes, dmix, npx, Cin, npts, workspace,
                   workspace_bytes};
  if (!curves_grad_supported(a))
    return fail(HDRNET_INVALID_ARGUMENT,
                "curves-guide gradient needs Cin = 3, npts = 16 and a workspace of "
                "hdrnet_curves_guide_grad_workspace_bytes()");
  const char* name = "";
  const hipError_t e = launch_curves_grad(a, s, &name);
  return finish_launch(e, "CurvesGuideGrad", name);
}

size_t hdrnet_input_moments_workspace_bytes(long long npx, int Cin) {
  if (npx <= 0) return 0;
  return hdrnet_amd::input_moments_workspace_bytes(npx, Cin);
}

int hdrnet_input_moments_f32(const float* input, long long npx, int Cin, float* sums,
                             float* moments, void* workspace, size_t workspace_bytes,
                             void* stream) {
  using namespace hdrnet_amd;
  if (npx < 0 || (Cin != 1 && Cin != 3))
    return fail(HDRNET_INVALID_ARGUMENT, "input moments need npx >= 0 and Cin in {1,3} (npx=%lld, Cin=%d)",
                npx, Cin);
  if (!sums || !moments) return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (npx == 0) {
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(float) * Cin, s);
    if (e == hipSuccess) e = hipMemsetAsync(moments, 0, sizeof(float) * Cin * Cin, s);
    return finish_launch(e, "InputMoments", "noop");
  }
  const size_t need = input_moments_workspace_bytes(npx, Cin);
  if (!input || ((uintptr_t)input & 15u) || !workspace || workspace_bytes < need)
    return fail(HDRNET_INVALID_ARGUMENT, "input moments need a 16-B aligned input and a workspace of "
                                         "hdrnet_input_moments_workspace_bytes()");
  const char* name = "";
  const hipError_t e = launch_input_moments(input, npx, Cin, sums, moments, workspace, s, &name);
  return finish_launch(e, "InputMoments", name);
}

int hdrnet_guide_nn_prescale_f32(const float* guide_conv1, const float* guide_conv2, int n_feats, int Cin, float x_max,
                                 float* conv1_out, float* conv2_out, void* stream) {
  using namespace hdrnet_amd;
  if (Cin != 3 || n_feats <= 0 || n_feats > 4096)
    return fail(HDRNET_INVALID_ARGUMENT, "guide prescale needs Cin = 3 and 0 < n_feats <= 4096 (Cin=%d, n=%d)", Cin, n_feats);
  if (!(x_max > 0.0f) || !(x_max < 1e30f))
    return fail(HDRNET_INVALID_ARGUMENT, "guide prescale needs a finite positive x_max");
  if (!guide_conv1 || !guide_conv2 || !conv1_out || !conv2_out) return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  if (((uintptr_t)conv1_out | (uintptr_t)conv2_out) & 15u)
    return fail(HDRNET_INVALID_ARGUMENT, "guide prescale needs 16-B aligned output arrays");
  return finish_launch(launch_guide_nn_prescale(guide_conv1, guide_conv2, n_feats, x_max, conv1_out, conv2_out,
                                                static_cast<hipStream_t>(stream)), "GuideNNPrescale",
                       "guide_nn_prescale");
}

int hdrnet_guide_fold_batch_f32(const float* sums, const float* moments, long long npx, const float* w1,
                                const float* gamma, const float* beta, const float* w2, const float* b2, double eps,
                                double momentum, int Cin, int n_feats, float* conv1, float* conv2,
                                float* running_mean, float* running_var, long long* num_batches_tracked,
                                void* stream) {
  using namespace hdrnet_amd;
  if (npx <= 0 || (Cin != 1 && Cin != 3) || n_feats <= 0)
    return fail(HDRNET_INVALID_ARGUMENT, "guide fold needs npx > 0, Cin in {1,3}, n_feats > 0 (npx=%lld, Cin=%d, n=%d)",
                npx, Cin, n_feats);
  if (!sums || !moments || !w1 || !gamma || !beta || !w2 || !b2 || !conv1 || !conv2 || (!running_mean != !running_var))
    return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  return finish_launch(launch_guide_fold_batch(sums, moments, npx, w1, gamma, beta, w2, b2, eps, momentum, Cin, n_feats,
                                               conv1, conv2, running_mean, running_var, num_batches_tracked,
                                               static_cast<hipStream_t>(stream)), "GuideFoldBatch", "guide_fold_batch");
}

int hdrnet_guide_fold_batch_grad_f32(const float* sums, const float* moments, long long npx, const float* w1,
                                     const float* gamma, const float* beta, double eps, int Cin, int n_feats,
                                     const float* dconv1, const float* dconv2, float* dw1, float* dbeta, float* dw2,
                                     float* db2, void* stream) {
  using namespace hdrnet_amd;
  if (npx <= 0 || (Cin != 1 && Cin != 3) || n_feats <= 0)
    return fail(HDRNET_INVALID_ARGUMENT, "guide fold needs npx > 0, Cin in {1,3}, n_feats > 0 (npx=%lld, Cin=%d, n=%d)",
                npx, Cin, n_feats);
  if (!sums || !moments || !w1 || !gamma || !beta || !dconv1 || !dconv2 || !dw1 || !dbeta || !dw2 || !db2)
    return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  return finish_launch(launch_guide_fold_batch_grad(sums, moments, npx, w1, gamma, beta, eps, Cin, n_feats, dconv1,
                                                    dconv2, dw1, dbeta, dw2, db2, static_cast<hipStream_t>(stream)),
                       "GuideFoldBatchGrad", "guide_fold_batch_grad");
}

size_t hdrnet_l2_loss_workspace_bytes(long long n) { return hdrnet_amd::l2_loss_workspace_bytes(n); }

int hdrnet_l2_loss_f32(const float* prediction, const float* target, long long n, float* loss, void* workspace,
                       size_t workspace_bytes, void* stream) {
  using namespace hdrnet_amd;
  if (n <= 0) return fail(HDRNET_INVALID_ARGUMENT, "l2 loss of an empty tensor (n=%lld)", n);
  if (!prediction || !target || !loss) return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  if ((((uintptr_t)prediction | (uintptr_t)target) & 15u) || !workspace || workspace_bytes < l2_loss_workspace_bytes(n))
    return fail(HDRNET_INVALID_ARGUMENT, "l2 loss needs 16-B aligned tensors and a workspace of "
                                         "hdrnet_l2_loss_workspace_bytes()");
  return finish_launch(launch_l2_loss(prediction, target, n, loss, workspace, static_cast<hipStream_t>(stream)),
                       "L2Loss", "l2_loss");
}

int hdrnet_l2_loss_grad_f32(const float* prediction, const float* target, const float* grad_output, long long n,
                            float* dprediction, void* stream) {
  using namespace hdrnet_amd;
  if (n <= 0) return fail(HDRNET_INVALID_ARGUMENT, "l2 loss of an empty tensor (n=%lld)", n);
  if (!prediction || !target || !grad_output || !dprediction) return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  if (((uintptr_t)prediction | (uintptr_t)target | (uintptr_t)dprediction) & 15u)
    return fail(HDRNET_INVALID_ARGUMENT, "l2 loss needs 16-B aligned tensors");
  return finish_launch(launch_l2_loss_grad(prediction, target, grad_output, n, dprediction,
                                           static_cast<hipStream_t>(stream)), "L2LossGrad", "l2_loss_grad");
}

size_t hdrnet_coefficients_workspace_bytes(const hdrnet_coeff_net* net, int B) {
  if (!net || B <= 0) return 0;
  return hdrnet_amd::coefficients_workspace_bytes(*net, B);
}

int hdrnet_coefficients_f32(const float* lowres, const hdrnet_coeff_net* net, float* coeffs, int B,
                            void* workspace, size_t workspace_bytes, void* stream) {
  using namespace hdrnet_amd;
  if (!net) return fail(HDRNET_INVALID_ARGUMENT, "null network description");
  if (B < 0 || B > 65535) return fail(HDRNET_INVALID_ARGUMENT, "batch out of range (B=%d, at most 65535 per call)", B);
  if (const char* limit = coefficients_limit(*net))
    return fail(HDRNET_INVALID_ARGUMENT,
                "coefficient network: %s (net_input_size=%d, spatial_bin=%d, luma_bins=%d, channel_multiplier=%d)", limit,
                net->net_input_size, net->spatial_bin, net->luma_bins, net->channel_multiplier);
  if (!coefficients_supported(*net))
    return fail(HDRNET_INVALID_ARGUMENT,
                "coefficient network: unsupported hyper-parameters (net_input_size=%d, spatial_bin=%d, luma_bins=%d, "
                "channel_multiplier=%d, n_out=%d, n_in=%d, n_levels=%d): sizes must be powers of two and "
                "channel_multiplier * luma_bins / 4 a power of two",
                net->net_input_size, net->spatial_bin, net->luma_bins, net->channel_multiplier, net->n_out,
                net->n_in, net->n_levels);
  if (B == 0) return finish_noop();
  if (coeff_net_null_param(*net, nullptr)) return fail(HDRNET_INVALID_ARGUMENT, "coefficient network: null parameter");
  if (!lowres || !coeffs) return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  const size_t need = coefficients_workspace_bytes(*net, B);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15u))
    return fail(HDRNET_INVALID_ARGUMENT, "coefficient network needs a 16-B aligned workspace of "
                                         "hdrnet_coefficients_workspace_bytes() = %zu bytes", need);
  const char* name = "";
  const hipError_t e = launch_coefficients(lowres, *net, coeffs, B, workspace, static_cast<hipStream_t>(stream), &name);
  return finish_launch(e, "Coefficients", name);
}

// The training entry points of the coefficient network exist twice: the first ones for batches up to 8 and their ..._wide
// twins (include/hdrnet_amd_coeff_wide.h) up to 32.  One body each: `prefix` goes in front of every refusal ("" for
// hdrnet_coefficients_grad_f32, which predates the convention), `query` names the workspace query in the text.
namespace {

int coefficients_grad_entry(const char* prefix, const char* query, int max_b, const float* lowres,
                            const hdrnet_coeff_net* net, const void* forward_workspace, const float* dcoeffs,
                            const hdrnet_coeff_net_grads* grads, int B, void* workspace, size_t workspace_bytes,
                            void* stream) {
  using namespace hdrnet_amd;
  if (!net || !grads) return fail(HDRNET_INVALID_ARGUMENT, "%snull network description", prefix);
  const size_t need = B > 0 ? coefficients_grad_workspace_bytes(*net, B, max_b) : 0;
  if (const char* limit = B > 0 ? coefficients_grad_limit(*net, B, max_b) : nullptr) {
    char batch[24] = "";  // the wide entry point's refusals all carry the batch; the first one's text stays as it was
    if (prefix[0]) snprintf(batch, sizeof batch, "; B=%d", B);
    return fail(HDRNET_INVALID_ARGUMENT,
                "%scoefficient network gradient: %s (spatial_bin=%d, luma_bins=%d, n_out=%d, n_in=%d); the forward has no "
                "such limit%s", prefix, limit, net->spatial_bin, net->luma_bins, net->n_out, net->n_in, batch);
  }
  if (need == 0)
    return fail(HDRNET_INVALID_ARGUMENT,
                "%scoefficient network gradient: unsupported (needs the forward's support, n_levels = 1, fc_layout = 1, "
                "1 <= B <= %d, 8 * cm * gd <= 256; got B=%d, n_levels=%d, fc_layout=%d)", prefix, max_b, B, net->n_levels,
                net->fc_layout);
  if (coeff_net_null_param(*net, grads))
    return fail(HDRNET_INVALID_ARGUMENT, "%scoefficient network gradient: null parameter", prefix);
  if (!lowres || !forward_workspace || !dcoeffs) return fail(HDRNET_INVALID_ARGUMENT, "%snull buffer", prefix);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15u))
    return fail(HDRNET_INVALID_ARGUMENT, "%scoefficient network gradient needs a 16-B aligned workspace of "
                                         "%s() = %zu bytes", prefix, query, need);
  const char* name = "";
  const hipError_t e = launch_coefficients_grad(lowres, *net, *grads, dcoeffs, B, forward_workspace, workspace,
                                                static_cast<hipStream_t>(stream), &name, max_b);
  return finish_launch(e, "CoefficientsGrad", name);
}

int coefficients_bn_train_entry(const char* kFn, const char* query, int max_b, const float* lowres,
                                const hdrnet_coeff_net_bn* net, float* coeffs, int B, void* workspace,
                                size_t workspace_bytes, void* stream) {
  using namespace hdrnet_amd;
  if (!net) return fail(HDRNET_INVALID_ARGUMENT, "%s: null network description", kFn);
  if (const char* why = coeff_net_bn_refusal(*net, nullptr, B, max_b))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: %s (B=%d, n_levels=%d, fc_layout=%d)", kFn, why, B, net->net.n_levels,
                net->net.fc_layout);
  if (!lowres || !coeffs) return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer", kFn);
  const size_t need = coefficients_bn_workspace_bytes(net->net, B, max_b);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15u))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: needs a 16-B aligned workspace of %s() = %zu bytes", kFn, query, need);
  // (no kernel name recorded: the training-loop helpers leave hdrnet_last_kernel() alone)
  return finish_launch(launch_coefficients_bn(lowres, *net, coeffs, B, workspace, static_cast<hipStream_t>(stream), max_b),
                       kFn, nullptr);
}

int coefficients_bn_grad_entry(const char* kFn, const char* query, int max_b, const float* lowres,
                               const hdrnet_coeff_net_bn* net, const void* forward_workspace, const float* dcoeffs,
                               const hdrnet_coeff_net_bn_grads* grads, int B, void* workspace, size_t workspace_bytes,
                               void* stream) {
  using namespace hdrnet_amd;
  if (!net || !grads) return fail(HDRNET_INVALID_ARGUMENT, "%s: null network description", kFn);
  if (const char* why = coeff_net_bn_refusal(*net, grads, B, max_b))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: %s (B=%d, n_levels=%d, fc_layout=%d)", kFn, why, B, net->net.n_levels,
                net->net.fc_layout);
  if (!lowres || !forward_workspace || !dcoeffs) return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer", kFn);
  const size_t need = coefficients_bn_grad_workspace_bytes(net->net, B, max_b);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15u))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: needs a 16-B aligned workspace of %s() = %zu bytes", kFn, query, need);
  return finish_launch(launch_coefficients_bn_grad(lowres, *net, *grads, dcoeffs, B, forward_workspace, workspace,
                                                   static_cast<hipStream_t>(stream), max_b), kFn, nullptr);
}

}  // namespace

size_t hdrnet_coefficients_grad_workspace_bytes(const hdrnet_coeff_net* net, int B) {
  if (!net || B <= 0) return 0;
  return hdrnet_amd::coefficients_grad_workspace_bytes(*net, B);
}

int hdrnet_coefficients_grad_f32(const float* lowres, const hdrnet_coeff_net* net, const void* forward_workspace,
                                 const float* dcoeffs, const hdrnet_coeff_net_grads* grads, int B, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return coefficients_grad_entry("", "hdrnet_coefficients_grad_workspace_bytes", hdrnet_amd::kCoeffNarrowMaxB, lowres, net,
                                 forward_workspace, dcoeffs, grads, B, workspace, workspace_bytes, stream);
}

size_t hdrnet_coefficients_bn_workspace_bytes(const hdrnet_coeff_net_bn* net, int B) {
  if (!net || B <= 0) return 0;
  return hdrnet_amd::coefficients_bn_workspace_bytes(net->net, B);
}

int hdrnet_coefficients_bn_train_f32(const float* lowres, const hdrnet_coeff_net_bn* net, float* coeffs, int B,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  return coefficients_bn_train_entry("hdrnet_coefficients_bn_train_f32", "hdrnet_coefficients_bn_workspace_bytes",
                                     hdrnet_amd::kCoeffNarrowMaxB, lowres, net, coeffs, B, workspace, workspace_bytes, stream);
}

size_t hdrnet_coefficients_bn_grad_workspace_bytes(const hdrnet_coeff_net_bn* net, int B) {
  if (!net || B <= 0) return 0;
  return hdrnet_amd::coefficients_bn_grad_workspace_bytes(net->net, B);
}

int hdrnet_coefficients_bn_grad_f32(const float* lowres, const hdrnet_coeff_net_bn* net, const void* forward_workspace,
                                    const float* dcoeffs, const hdrnet_coeff_net_bn_grads* grads, int B, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return coefficients_bn_grad_entry("hdrnet_coefficients_bn_grad_f32", "hdrnet_coefficients_bn_grad_workspace_bytes",
                                    hdrnet_amd::kCoeffNarrowMaxB, lowres, net, forward_workspace, dcoeffs, grads, B,
                                    workspace, workspace_bytes, stream);
}

// ---- the same for batches up to 32 (include/hdrnet_amd_coeff_wide.h)

size_t hdrnet_coefficients_grad_wide_workspace_bytes(const hdrnet_coeff_net* net, int B) {
  if (!net || B <= 0) return 0;
  return hdrnet_amd::coefficients_grad_workspace_bytes(*net, B, hdrnet_amd::kCoeffWideMaxB);
}

int hdrnet_coefficients_grad_wide_f32(const float* lowres, const hdrnet_coeff_net* net, const void* forward_workspace,
                                      const float* dcoeffs, const hdrnet_coeff_net_grads* grads, int B, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  return coefficients_grad_entry("hdrnet_coefficients_grad_wide_f32: ", "hdrnet_coefficients_grad_wide_workspace_bytes",
                                 hdrnet_amd::kCoeffWideMaxB, lowres, net, forward_workspace, dcoeffs, grads, B, workspace,
                                 workspace_bytes, stream);
}

size_t hdrnet_coefficients_bn_wide_workspace_bytes(const hdrnet_coeff_net_bn* net, int B) {
  if (!net || B <= 0) return 0;
  return hdrnet_amd::coefficients_bn_workspace_bytes(net->net, B, hdrnet_amd::kCoeffWideMaxB);
}

int hdrnet_coefficients_bn_train_wide_f32(const float* lowres, const hdrnet_coeff_net_bn* net, float* coeffs, int B,
                                          void* workspace, size_t workspace_bytes, void* stream) {
  return coefficients_bn_train_entry("hdrnet_coefficients_bn_train_wide_f32", "hdrnet_coefficients_bn_wide_workspace_bytes",
                                     hdrnet_amd::kCoeffWideMaxB, lowres, net, coeffs, B, workspace, workspace_bytes, stream);
}

size_t hdrnet_coefficients_bn_grad_wide_workspace_bytes(const hdrnet_coeff_net_bn* net, int B) {
  if (!net || B <= 0) return 0;
  return hdrnet_amd::coefficients_bn_grad_workspace_bytes(net->net, B, hdrnet_amd::kCoeffWideMaxB);
}

int hdrnet_coefficients_bn_grad_wide_f32(const float* lowres, const hdrnet_coeff_net_bn* net, const void* forward_workspace,
                                         const float* dcoeffs, const hdrnet_coeff_net_bn_grads* grads, int B,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  return coefficients_bn_grad_entry("hdrnet_coefficients_bn_grad_wide_f32", "hdrnet_coefficients_bn_grad_wide_workspace_bytes",
                                    hdrnet_amd::kCoeffWideMaxB, lowres, net, forward_workspace, dcoeffs, grads, B,
                                    workspace, workspace_bytes, stream);
}

// ---- include/hdrnet_amd.h: the wire formats (uint8 / uint16 / float32 frames in, float32 / uint8 out) --------------------
// The guide side of an entry point, in the fields of ApplyIoArgs.  Two kinds: a guide map or the guide network with its
// flags (`guide`, conv1, conv2, n = n_feats), or the curves guide (conv1 = ccm, conv2 = mix, shifts, slopes, n = npts,
// the prepared cell tables or null).
struct IoGuide {
  bool curves;
  const float* guide;
  const float* conv1;
  const float* conv2;
  int n;
  float* guide_out;
  unsigned flags;
  const float* shifts;
  const float* slopes;
  const void* prepared;
};

static IoGuide io_guide_network(const float* guide, const float* conv1, const float* conv2, int n_feats, float* guide_out,
                                unsigned flags) {
  return IoGuide{false, guide, conv1, conv2, n_feats, guide_out, flags, nullptr, nullptr, nullptr};
}

static IoGuide io_guide_curves(const float* ccm, const float* shifts, const float* slopes, const float* mix, int npts,
                               const void* prepared, float* guide_out) {
  return IoGuide{true, nullptr, ccm, mix, npts, guide_out, 0u, shifts, slopes, prepared};
}

// the guide's last word before the launch: the network's flags against the pointers, or the curves' prepared tables
static int set_io_guide(hdrnet_amd::ApplyIoArgs& a, const IoGuide& g, const char* prefix, const char* prepared_needs) {
  return g.curves ? set_curves_prepared(a, g.prepared, prefix, prepared_needs) : set_io_guide_flags(a, g.flags);
}

// A frame in `pixel_format` (HDRNET_PX_RGB for the entry points of this header) with either guide.  The network's flags
// answer before the frame's values, the curves' knots after them.
static int apply_io_impl(const float* grid, const IoGuide& g, const void* input, void* out, int B, int H, int W, int GH,
                         int GW, int GD, int Cin, int Cout, int has_offset, int input_dtype, float input_white_level,
                         int output_dtype, int pixel_format, void* stream, const U16Out* u16 = nullptr) {
  using namespace hdrnet_amd;
  if (int rc = check_common(B, H, W, GH, GW, GD)) return rc;
  if (!g.curves)
    if (int rc = check_guide_flags(g.flags)) return rc;
  if (int rc = check_frame_values(Cin, Cout, input_dtype, input_white_level, output_dtype, u16)) return rc;
  if (g.curves)
    if (int rc = check_curves_knots("", g.n)) return rc;
  if ((long long)B * H * W == 0) return finish_noop();
  if (!grid || !input || !out || (g.curves && (!g.conv1 || !g.shifts || !g.slopes || !g.conv2)))
    return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  if (!g.curves)
    if (int rc = check_guide_given("", g.guide, g.conv1, g.conv2, g.n)) return rc;
  const char* px_what = g.curves ? "hdrnet_bilateral_slice_apply_io_curves_px" : "hdrnet_bilateral_slice_apply_io_px";
  if (int rc = check_pixel_buffers(u16 ? u16->what : px_what, pixel_format, Cin, Cout, has_offset, W, input,
                                   output_dtype != 0 ? out : nullptr))
    return rc;
  ApplyIoArgs a{grid, g.guide, input, out, B, H, W, GH, GW, GD, Cin, Cout, has_offset != 0,
                input_dtype, output_dtype, input_white_level, g.conv1, g.conv2, g.n,
                g.guide_out, g.shifts, g.slopes};
  a.pixel_format = pixel_format;
  if (u16) a.output_white_level = u16->white_level;
  if (int rc = set_io_guide(a, g, "", "Cin = 3, npts <= 16")) return rc;
  if (g.curves)
    return launch_io(a, nullptr, 0, 0, "BilateralSliceApplyIOCurves",
                     "the fused curves-guide forward supports Cin = Cout = 3 with offset, W % 4 == 0, aligned "
                     "buffers; evaluate the guide on the caller's side and use hdrnet_bilateral_slice_apply_f32", stream);
  return launch_io(a, nullptr, 0, 0, "BilateralSliceApplyIO",
                   "the wire-format forward supports Cin = Cout = 3 with offset, W % 4 == 0, aligned "
                   "buffers; convert on the caller's side and use hdrnet_bilateral_slice_apply_f32", stream);
}

int hdrnet_bilateral_slice_apply_io_ex(const float* grid, const float* guide, const void* input,
                                       void* out, int B, int H, int W, int GH, int GW, int GD, int Cin,
                                       int Cout, int has_offset, int input_dtype,
                                       float input_white_level, int output_dtype,
                                       const float* guide_conv1, const float* guide_conv2, int n_feats,
                                       float* guide_out, unsigned flags, void* stream) {
  return apply_io_impl(grid, io_guide_network(guide, guide_conv1, guide_conv2, n_feats, guide_out, flags), input, out, B, H,
                       W, GH, GW, GD, Cin, Cout, has_offset, input_dtype, input_white_level, output_dtype, HDRNET_PX_RGB,
                       stream);
}

int hdrnet_bilateral_slice_apply_io(const float* grid, const float* guide, const void* input,
                                    void* out, int B, int H, int W, int GH, int GW, int GD, int Cin,
                                    int Cout, int has_offset, int input_dtype,
                                    float input_white_level, int output_dtype,
                                    const float* guide_conv1, const float* guide_conv2, int n_feats,
                                    float* guide_out, void* stream) {
  return hdrnet_bilateral_slice_apply_io_ex(grid, guide, input, out, B, H, W, GH, GW, GD, Cin, Cout, has_offset,
                                            input_dtype, input_white_level, output_dtype, guide_conv1, guide_conv2,
                                            n_feats, guide_out, 0u, stream);
}

size_t hdrnet_curves_guide_prepared_bytes(int Cin) { return hdrnet_amd::curves_guide_prepared_bytes(Cin); }

int hdrnet_curves_guide_prepare_f32(const float* guide_shifts, const float* guide_slopes, int npts, int Cin,
                                    void* prepared, size_t prepared_bytes, int* usable, void* stream) {
  using namespace hdrnet_amd;
  const size_t need = curves_guide_prepared_bytes(Cin);
  if (need == 0 || npts <= 0 || npts > 16)
    return fail(HDRNET_INVALID_ARGUMENT, "curves prepare needs Cin = 3 and 1 .. 16 knots per channel (Cin=%d, npts=%d)", Cin,
                npts);
  if (!guide_shifts || !guide_slopes || !prepared) return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  if (((uintptr_t)prepared & 15u) || prepared_bytes < need)
    return fail(HDRNET_INVALID_ARGUMENT, "curves prepare needs a 16-B aligned buffer of hdrnet_curves_guide_prepared_bytes()");
  if (!usable) return fail(HDRNET_INVALID_ARGUMENT, "curves prepare: `usable` must point to an int");
  *usable = 0;
  const int rc = finish_launch(launch_curves_guide_prepare(guide_shifts, guide_slopes, npts, Cin,
                                                           static_cast<float*>(prepared), static_cast<hipStream_t>(stream)),
                                "CurvesGuidePrepare", "curves_prepare");
  if (rc != HDRNET_OK) return rc;
  // a SET-UP call, once per parameter set: the table's `ok` word comes back to the host (this waits for `stream`), because
  // which forward kernel a prepared buffer selects is decided on the host
  float ok = 0.0f;
  hipError_t e = hipMemcpyAsync(&ok, static_cast<const float*>(prepared) + curves_guide_prepared_ok_offset(Cin),
                                sizeof(float), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream));
  if (e == hipSuccess) e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
  if (e != hipSuccess)
    return fail(HDRNET_RUNTIME_FAILURE, "curves prepare: reading the table's ok word back: %s", hipGetErrorString(e));
  *usable = ok != 0.0f ? 1 : 0;
  return HDRNET_OK;
}

int hdrnet_bilateral_slice_apply_io_curves_prepared(const float* grid, const void* input, void* out, int B, int H,
                                                    int W, int GH, int GW, int GD, int Cin, int Cout,
                                                    int has_offset, int input_dtype, float input_white_level,
                                                    int output_dtype, const float* guide_ccm,
                                                    const float* guide_shifts, const float* guide_slopes,
                                                    const float* guide_mix, int npts, const void* prepared,
                                                    float* guide_out, void* stream) {
  return apply_io_impl(grid, io_guide_curves(guide_ccm, guide_shifts, guide_slopes, guide_mix, npts, prepared, guide_out),
                       input, out, B, H, W, GH, GW, GD, Cin, Cout, has_offset, input_dtype, input_white_level, output_dtype,
                       HDRNET_PX_RGB, stream);
}

int hdrnet_bilateral_slice_apply_io_curves(const float* grid, const void* input, void* out, int B, int H,
                                           int W, int GH, int GW, int GD, int Cin, int Cout,
                                           int has_offset, int input_dtype, float input_white_level,
                                           int output_dtype, const float* guide_ccm,
                                           const float* guide_shifts, const float* guide_slopes,
                                           const float* guide_mix, int npts, float* guide_out,
                                           void* stream) {
  return hdrnet_bilateral_slice_apply_io_curves_prepared(grid, input, out, B, H, W, GH, GW, GD, Cin, Cout, has_offset,
                                                         input_dtype, input_white_level, output_dtype, guide_ccm,
                                                         guide_shifts, guide_slopes, guide_mix, npts, nullptr, guide_out,
                                                         stream);
}

// ---- include/hdrnet_amd_pixel_formats.h: frames in BGR / RGBA / BGRA order -----------------------------------------
// (the format codes answer before anything else; hdrnet_lowres_input_px: sample preparation, below)
int hdrnet_bilateral_slice_apply_io_px(const float* grid, const float* guide, const void* input, void* out, int B, int H,
                                       int W, int GH, int GW, int GD, int Cin, int Cout, int has_offset, int input_dtype,
                                       float input_white_level, int output_dtype, const float* guide_conv1,
                                       const float* guide_conv2, int n_feats, float* guide_out, unsigned flags,
                                       int input_format, int output_format, void* stream) {
  if (int rc = check_io_format(input_dtype, input_white_level, output_dtype)) return rc;
  if (int rc = check_pixel_formats("hdrnet_bilateral_slice_apply_io_px", input_dtype, output_dtype, input_format, output_format))
    return rc;
  return apply_io_impl(grid, io_guide_network(guide, guide_conv1, guide_conv2, n_feats, guide_out, flags), input, out, B, H,
                       W, GH, GW, GD, Cin, Cout, has_offset, input_dtype, input_white_level, output_dtype, input_format,
                       stream);
}

int hdrnet_bilateral_slice_apply_io_curves_px(const float* grid, const void* input, void* out, int B, int H, int W, int GH,
                                              int GW, int GD, int Cin, int Cout, int has_offset, int input_dtype,
                                              float input_white_level, int output_dtype, const float* guide_ccm,
                                              const float* guide_shifts, const float* guide_slopes,
                                              const float* guide_mix, int npts, const void* prepared, float* guide_out,
                                              int input_format, int output_format, void* stream) {
  if (int rc = check_io_format(input_dtype, input_white_level, output_dtype)) return rc;
  if (int rc = check_pixel_formats("hdrnet_bilateral_slice_apply_io_curves_px", input_dtype, output_dtype, input_format,
                                   output_format))
    return rc;
  return apply_io_impl(grid, io_guide_curves(guide_ccm, guide_shifts, guide_slopes, guide_mix, npts, prepared, guide_out),
                       input, out, B, H, W, GH, GW, GD, Cin, Cout, has_offset, input_dtype, input_white_level, output_dtype,
                       input_format, stream);
}

// ---- include/hdrnet_amd_yuv.h: semi-planar YUV 4:2:0 surfaces (hdrnet_lowres_input_yuv: sample preparation, below) --------
int hdrnet_yuv_to_rgb_f32(const void* y, const void* uv, int sample_dtype, int pitch_y, int pitch_uv,
                          long long image_stride_y, long long image_stride_uv, int B, int H, int W, const float* to_rgb,
                          float* rgb, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_yuv_to_rgb_f32";
  const YuvSurface in{y, uv, pitch_y, pitch_uv, image_stride_y, image_stride_uv};
  if (int rc = check_yuv_extents(what, B, H, W)) return rc;
  if (int rc = check_yuv_surface(what, "input", sample_dtype, in, B, H, W)) return rc;
  if ((long long)B * H * W == 0) return finish_noop();
  if (int rc = check_yuv_pointers(what, "input", in, to_rgb)) return rc;
  if (!rgb || ((uintptr_t)rgb & 15u)) return fail(HDRNET_INVALID_ARGUMENT, "%s: rgb must be a 16-B aligned buffer", what);
  return finish_launch(launch_yuv_to_rgb(in, sample_dtype, to_rgb, rgb, B, H, W, static_cast<hipStream_t>(stream)), what,
                       "yuv_to_rgb");
}

// The four fused entry points (`what`): a surface in with either guide; `io`: the call's surfaces as given, io.out.y the
// RGB frame where the output is one; `p016`: an entry point of hdrnet_amd_u16_out.h (io.out_kind is then kYuvOutP016,
// which the others refuse as a caller's output kind).  Either guide's values answer before the surfaces'.
// `up`: the call is an up-add entry point of hdrnet_amd_pyramid_yuv.h (a guide map or the network, never the curves): the
// coarse level's rules answer after the surfaces', its pointer after theirs.
static int apply_io_yuv_impl(const char* what, bool p016, const float* grid, const IoGuide& g, hdrnet_amd::YuvIo io,
                             int sample_dtype, int B, int H, int W, int GH, int GW, int GD, int Cin, int Cout, int has_offset,
                             void* stream, const IoCoarse* up = nullptr) {
  using namespace hdrnet_amd;
  char prefix[96];
  snprintf(prefix, sizeof prefix, "%s: ", what);
  if (int rc = check_common(B, H, W, GH, GW, GD)) return rc;
  if (int rc = g.curves ? check_curves_knots(prefix, g.n) : check_guide_flags(g.flags)) return rc;
  if (int rc = check_yuv_io_values(what, io, sample_dtype, B, H, W, Cin, Cout, has_offset, p016)) return rc;
  if (up)
    if (int rc = check_upadd_values(up->Hc, up->Wc, g.guide, g.conv1, g.conv2, g.n)) return rc;
  if ((long long)B * H * W == 0) return finish_noop();
  if (int rc = check_yuv_io_pointers(what, io)) return rc;
  if (up)
    if (int rc = check_coarse_pointer(what, up->coarse)) return rc;
  if (g.curves) {
    if (!grid || !g.conv1 || !g.shifts || !g.slopes || !g.conv2)
      return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer (grid or a curves parameter)", what);
  } else {
    if (!grid) return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer (grid)", what);
    if (int rc = check_guide_given(prefix, g.guide, g.conv1, g.conv2, g.n)) return rc;
  }
  ApplyIoArgs a{grid, g.guide, nullptr, nullptr, B, H, W, GH, GW, GD, Cin, Cout, true,
                sample_dtype, p016 ? 2 : io.out_kind == HDRNET_YUV_OUT_RGB_F32 ? 0 : 1, 1.0f, g.conv1, g.conv2, g.n,
                g.guide_out, g.shifts, g.slopes};
  if (int rc = set_io_guide(a, g, prefix, "npts <= 16")) return rc;
  if (io.out_kind < HDRNET_YUV_OUT_NV12) {  // an RGB frame out: a.out
    a.out = const_cast<void*>(io.out.y);
    io.out = YuvSurface{};
    io.from_rgb = nullptr;
  }
  a.yuv = &io;
  if (up)
    return launch_io(a, up->coarse, up->Hc, up->Wc, "BilateralSliceApplyUpAddIOYuv",
                     "the YUV slice-apply + up-add supports Cin = Cout = 3 with offset, H % 2 == 0, W % 4 == 0, aligned buffers",
                     stream);
  return launch_io(a, nullptr, 0, 0, g.curves ? "BilateralSliceApplyIOCurvesYuv" : "BilateralSliceApplyIOYuv",
                   io.chroma != HDRNET_CHROMA_420
                       ? "the 4:2:2 YUV forward supports Cin = Cout = 3 with offset, W % 4 == 0, aligned buffers"
                       : "the YUV forward supports Cin = Cout = 3 with offset, H % 2 == 0, W % 4 == 0, aligned buffers",
                   stream);
}

int hdrnet_bilateral_slice_apply_io_yuv(const float* grid, const float* guide, const void* y, const void* uv,
                                        int sample_dtype, int pitch_y, int pitch_uv, long long image_stride_y,
                                        long long image_stride_uv, int B, int H, int W, const float* to_rgb, int GH, int GW,
                                        int GD, int Cin, int Cout, int has_offset, const float* guide_conv1,
                                        const float* guide_conv2, int n_feats, float* guide_out, unsigned flags,
                                        int output_kind, void* out, void* out_uv, int out_pitch_y, int out_pitch_uv,
                                        long long out_image_stride_y, long long out_image_stride_uv,
                                        const float* from_rgb, void* stream) {
  const hdrnet_amd::YuvIo io{{y, uv, pitch_y, pitch_uv, image_stride_y, image_stride_uv}, to_rgb, output_kind,
                             {out, out_uv, out_pitch_y, out_pitch_uv, out_image_stride_y, out_image_stride_uv}, from_rgb};
  return apply_io_yuv_impl("hdrnet_bilateral_slice_apply_io_yuv", false, grid,
                           io_guide_network(guide, guide_conv1, guide_conv2, n_feats, guide_out, flags), io, sample_dtype, B,
                           H, W, GH, GW, GD, Cin, Cout, has_offset, stream);
}

int hdrnet_bilateral_slice_apply_io_curves_yuv(const float* grid, const void* y, const void* uv, int sample_dtype,
                                               int pitch_y, int pitch_uv, long long image_stride_y,
                                               long long image_stride_uv, int B, int H, int W, const float* to_rgb, int GH,
                                               int GW, int GD, int Cin, int Cout, int has_offset, const float* guide_ccm,
                                               const float* guide_shifts, const float* guide_slopes,
                                               const float* guide_mix, int npts, const void* prepared, float* guide_out,
                                               int output_kind, void* out, void* out_uv, int out_pitch_y,
                                               int out_pitch_uv, long long out_image_stride_y,
                                               long long out_image_stride_uv, const float* from_rgb, void* stream) {
  const hdrnet_amd::YuvIo io{{y, uv, pitch_y, pitch_uv, image_stride_y, image_stride_uv}, to_rgb, output_kind,
                             {out, out_uv, out_pitch_y, out_pitch_uv, out_image_stride_y, out_image_stride_uv}, from_rgb};
  return apply_io_yuv_impl("hdrnet_bilateral_slice_apply_io_curves_yuv", false, grid,
                           io_guide_curves(guide_ccm, guide_shifts, guide_slopes, guide_mix, npts, prepared, guide_out), io,
                           sample_dtype, B, H, W, GH, GW, GD, Cin, Cout, has_offset, stream);
}

// ---- include/hdrnet_amd_u16_out.h: a uint16 frame / a P010 / P016 surface out ------------------------------------------
// (the four entry points above with the output's own rules beside them: the same bodies, so the same checks in the same order)
int hdrnet_bilateral_slice_apply_io_px_u16(const float* grid, const float* guide, const void* input, void* out, int B,
                                           int H, int W, int GH, int GW, int GD, int Cin, int Cout, int has_offset,
                                           int input_dtype, float input_white_level, float output_white_level,
                                           const float* guide_conv1, const float* guide_conv2, int n_feats,
                                           float* guide_out, unsigned flags, int input_format, int output_format,
                                           void* stream) {
  const U16Out u16{"hdrnet_bilateral_slice_apply_io_px_u16", output_white_level};
  if (int rc = check_u16_format(u16, input_dtype, input_white_level)) return rc;
  if (int rc = check_pixel_formats(u16.what, input_dtype, 2, input_format, output_format)) return rc;
  return apply_io_impl(grid, io_guide_network(guide, guide_conv1, guide_conv2, n_feats, guide_out, flags), input, out, B, H,
                       W, GH, GW, GD, Cin, Cout, has_offset, input_dtype, input_white_level, 2, input_format, stream, &u16);
}

int hdrnet_bilateral_slice_apply_io_curves_px_u16(const float* grid, const void* input, void* out, int B, int H, int W,
                                                  int GH, int GW, int GD, int Cin, int Cout, int has_offset,
                                                  int input_dtype, float input_white_level, float output_white_level,
                                                  const float* guide_ccm, const float* guide_shifts,
                                                  const float* guide_slopes, const float* guide_mix, int npts,
                                                  const void* prepared, float* guide_out, int input_format,
                                                  int output_format, void* stream) {
  const U16Out u16{"hdrnet_bilateral_slice_apply_io_curves_px_u16", output_white_level};
  if (int rc = check_u16_format(u16, input_dtype, input_white_level)) return rc;
  if (int rc = check_pixel_formats(u16.what, input_dtype, 2, input_format, output_format)) return rc;
  return apply_io_impl(grid, io_guide_curves(guide_ccm, guide_shifts, guide_slopes, guide_mix, npts, prepared, guide_out),
                       input, out, B, H, W, GH, GW, GD, Cin, Cout, has_offset, input_dtype, input_white_level, 2,
                       input_format, stream, &u16);
}

int hdrnet_bilateral_slice_apply_io_yuv_p016(const float* grid, const float* guide, const void* y, const void* uv,
                                             int sample_dtype, int pitch_y, int pitch_uv, long long image_stride_y,
                                             long long image_stride_uv, int B, int H, int W, const float* to_rgb, int GH,
                                             int GW, int GD, int Cin, int Cout, int has_offset, const float* guide_conv1,
                                             const float* guide_conv2, int n_feats, float* guide_out, unsigned flags,
                                             void* out_y, void* out_uv, int out_pitch_y, int out_pitch_uv,
                                             long long out_image_stride_y, long long out_image_stride_uv,
                                             const float* from_rgb, int out_bits, void* stream) {
  const hdrnet_amd::YuvIo io{{y, uv, pitch_y, pitch_uv, image_stride_y, image_stride_uv}, to_rgb, hdrnet_amd::kYuvOutP016,
                             {out_y, out_uv, out_pitch_y, out_pitch_uv, out_image_stride_y, out_image_stride_uv}, from_rgb,
                             out_bits};
  return apply_io_yuv_impl("hdrnet_bilateral_slice_apply_io_yuv_p016", true, grid,
                           io_guide_network(guide, guide_conv1, guide_conv2, n_feats, guide_out, flags), io, sample_dtype, B,
                           H, W, GH, GW, GD, Cin, Cout, has_offset, stream);
}

int hdrnet_bilateral_slice_apply_io_curves_yuv_p016(const float* grid, const void* y, const void* uv, int sample_dtype,
                                                    int pitch_y, int pitch_uv, long long image_stride_y,
                                                    long long image_stride_uv, int B, int H, int W, const float* to_rgb,
                                                    int GH, int GW, int GD, int Cin, int Cout, int has_offset,
                                                    const float* guide_ccm, const float* guide_shifts,
                                                    const float* guide_slopes, const float* guide_mix, int npts,
                                                    const void* prepared, float* guide_out, void* out_y, void* out_uv,
                                                    int out_pitch_y, int out_pitch_uv, long long out_image_stride_y,
                                                    long long out_image_stride_uv, const float* from_rgb, int out_bits,
                                                    void* stream) {
  const hdrnet_amd::YuvIo io{{y, uv, pitch_y, pitch_uv, image_stride_y, image_stride_uv}, to_rgb, hdrnet_amd::kYuvOutP016,
                             {out_y, out_uv, out_pitch_y, out_pitch_uv, out_image_stride_y, out_image_stride_uv}, from_rgb,
                             out_bits};
  return apply_io_yuv_impl("hdrnet_bilateral_slice_apply_io_curves_yuv_p016", true, grid,
                           io_guide_curves(guide_ccm, guide_shifts, guide_slopes, guide_mix, npts, prepared, guide_out), io,
                           sample_dtype, B, H, W, GH, GW, GD, Cin, Cout, has_offset, stream);
}

// ---- include/hdrnet_amd_yuv_planar.h: planar YUV 4:2:0 surfaces (hdrnet_lowres_input_yuv_planar: sample preparation, below)
int hdrnet_yuv_planar_to_rgb_f32(const void* y, const void* u, const void* v, int sample_dtype, int pitch_y, int pitch_u,
                                 int pitch_v, long long image_stride_y, long long image_stride_u,
                                 long long image_stride_v, int B, int H, int W, const float* to_rgb, float* rgb,
                                 void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_yuv_planar_to_rgb_f32";
  const YuvPlanarSurface in{y, u, v, pitch_y, pitch_u, pitch_v, image_stride_y, image_stride_u, image_stride_v};
  if (int rc = check_yuv_extents(what, B, H, W)) return rc;
  if (int rc = check_yuv_planar_surface(what, "input", sample_dtype, in, B, H, W)) return rc;
  if ((long long)B * H * W == 0) return finish_noop();
  if (int rc = check_yuv_planar_pointers(what, "input", sample_dtype, in, to_rgb)) return rc;
  if (!rgb || ((uintptr_t)rgb & 15u)) return fail(HDRNET_INVALID_ARGUMENT, "%s: rgb must be a 16-B aligned buffer", what);
  return finish_launch(launch_yuv_planar_to_rgb(in, sample_dtype, to_rgb, rgb, B, H, W, static_cast<hipStream_t>(stream)), what,
                       "yuv_planar_to_rgb");
}

// The two fused entry points (`what`): a planar surface in with either guide; `io`: the call's surfaces as given, io.out.y
// the RGB frame where the output is one.  apply_io_yuv_impl's checks in its order.
// (`up`: as there)
static int apply_io_yuv_planar_impl(const char* what, const float* grid, const IoGuide& g, hdrnet_amd::YuvPlanarIo io,
                                    int sample_dtype, int B, int H, int W, int GH, int GW, int GD, int Cin, int Cout,
                                    int has_offset, void* stream, const IoCoarse* up = nullptr) {
  using namespace hdrnet_amd;
  char prefix[96];
  snprintf(prefix, sizeof prefix, "%s: ", what);
  if (int rc = check_common(B, H, W, GH, GW, GD)) return rc;
  if (int rc = g.curves ? check_curves_knots(prefix, g.n) : check_guide_flags(g.flags)) return rc;
  if (int rc = check_yuv_planar_io_values(what, io, sample_dtype, B, H, W, Cin, Cout, has_offset)) return rc;
  if (up)
    if (int rc = check_upadd_values(up->Hc, up->Wc, g.guide, g.conv1, g.conv2, g.n)) return rc;
  if ((long long)B * H * W == 0) return finish_noop();
  if (int rc = check_yuv_planar_io_pointers(what, io, sample_dtype)) return rc;
  if (up)
    if (int rc = check_coarse_pointer(what, up->coarse)) return rc;
  if (g.curves) {
    if (!grid || !g.conv1 || !g.shifts || !g.slopes || !g.conv2)
      return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer (grid or a curves parameter)", what);
  } else {
    if (!grid) return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer (grid)", what);
    if (int rc = check_guide_given(prefix, g.guide, g.conv1, g.conv2, g.n)) return rc;
  }
  const bool planar_out = io.out_kind == HDRNET_YUV_PLANAR_OUT_PLANAR;
  ApplyIoArgs a{grid, g.guide, nullptr, nullptr, B, H, W, GH, GW, GD, Cin, Cout, true,
                sample_dtype, planar_out ? sample_dtype : io.out_kind == HDRNET_YUV_PLANAR_OUT_RGB_F32 ? 0 : 1, 1.0f, g.conv1,
                g.conv2, g.n, g.guide_out, g.shifts, g.slopes};
  if (int rc = set_io_guide(a, g, prefix, "npts <= 16")) return rc;
  if (!planar_out) {  // an RGB frame out: a.out
    a.out = const_cast<void*>(io.out.y);
    io.out = YuvPlanarSurface{};
    io.from_rgb = nullptr;
    io.out_bits = 0;
  }
  a.yuvp = &io;
  if (up)
    return launch_io(a, up->coarse, up->Hc, up->Wc, "BilateralSliceApplyUpAddIOYuvPlanar",
                     "the planar YUV slice-apply + up-add supports Cin = Cout = 3 with offset, H % 2 == 0, W % 4 == 0, aligned "
                     "buffers", stream);
  return launch_io(a, nullptr, 0, 0, g.curves ? "BilateralSliceApplyIOCurvesYuvPlanar" : "BilateralSliceApplyIOYuvPlanar",
                   io.chroma != HDRNET_CHROMA_420
                       ? "the 4:2:2 / 4:4:4 planar YUV forward supports Cin = Cout = 3 with offset, W % 4 == 0, aligned buffers"
                       : "the planar YUV forward supports Cin = Cout = 3 with offset, H % 2 == 0, W % 4 == 0, aligned buffers",
                   stream);
}

int hdrnet_bilateral_slice_apply_io_yuv_planar(const float* grid, const float* guide, const void* y, const void* u,
                                               const void* v, int sample_dtype, int pitch_y, int pitch_u, int pitch_v,
                                               long long image_stride_y, long long image_stride_u,
                                               long long image_stride_v, int B, int H, int W, const float* to_rgb, int GH,
                                               int GW, int GD, int Cin, int Cout, int has_offset,
                                               const float* guide_conv1, const float* guide_conv2, int n_feats,
                                               float* guide_out, unsigned flags, int output_kind, void* out, void* out_u,
                                               void* out_v, int out_pitch_y, int out_pitch_u, int out_pitch_v,
                                               long long out_image_stride_y, long long out_image_stride_u,
                                               long long out_image_stride_v, const float* from_rgb, int out_bits,
                                               void* stream) {
  const hdrnet_amd::YuvPlanarIo io{
      {y, u, v, pitch_y, pitch_u, pitch_v, image_stride_y, image_stride_u, image_stride_v}, to_rgb, output_kind,
      {out, out_u, out_v, out_pitch_y, out_pitch_u, out_pitch_v, out_image_stride_y, out_image_stride_u, out_image_stride_v},
      from_rgb, out_bits};
  return apply_io_yuv_planar_impl("hdrnet_bilateral_slice_apply_io_yuv_planar", grid,
                                  io_guide_network(guide, guide_conv1, guide_conv2, n_feats, guide_out, flags), io, sample_dtype,
                                  B, H, W, GH, GW, GD, Cin, Cout, has_offset, stream);
}

int hdrnet_bilateral_slice_apply_io_curves_yuv_planar(const float* grid, const void* y, const void* u, const void* v,
                                                      int sample_dtype, int pitch_y, int pitch_u, int pitch_v,
                                                      long long image_stride_y, long long image_stride_u,
                                                      long long image_stride_v, int B, int H, int W, const float* to_rgb,
                                                      int GH, int GW, int GD, int Cin, int Cout, int has_offset,
                                                      const float* guide_ccm, const float* guide_shifts,
                                                      const float* guide_slopes, const float* guide_mix, int npts,
                                                      const void* prepared, float* guide_out, int output_kind, void* out,
                                                      void* out_u, void* out_v, int out_pitch_y, int out_pitch_u,
                                                      int out_pitch_v, long long out_image_stride_y,
                                                      long long out_image_stride_u, long long out_image_stride_v,
                                                      const float* from_rgb, int out_bits, void* stream) {
  const hdrnet_amd::YuvPlanarIo io{
      {y, u, v, pitch_y, pitch_u, pitch_v, image_stride_y, image_stride_u, image_stride_v}, to_rgb, output_kind,
      {out, out_u, out_v, out_pitch_y, out_pitch_u, out_pitch_v, out_image_stride_y, out_image_stride_u, out_image_stride_v},
      from_rgb, out_bits};
  return apply_io_yuv_planar_impl("hdrnet_bilateral_slice_apply_io_curves_yuv_planar", grid,
                                  io_guide_curves(guide_ccm, guide_shifts, guide_slopes, guide_mix, npts, prepared, guide_out),
                                  io, sample_dtype, B, H, W, GH, GW, GD, Cin, Cout, has_offset, stream);
}

// ---- include/hdrnet_amd_pyramid_io.h: the pyramid model's wire formats ---------------------------------------------
int hdrnet_resize_bilinear_io(const void* input, int input_dtype, float white_level, float* out, int B, int Hin, int Win,
                              int Hout, int Wout, int C, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_resize_bilinear_io";
  if (B < 0 || Hin <= 0 || Win <= 0 || Hout < 0 || Wout < 0)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: bad extents (B=%d, in %dx%d, out %dx%d)", what, B, Hin, Win, Hout, Wout);
  if (C != 3) return fail(HDRNET_INVALID_ARGUMENT, "%s: C must be 3 (RGB frames), got C=%d", what, C);
  if (int rc = check_input_dtype(what, input_dtype)) return rc;
  if (!(white_level > 0.0f) || !(white_level <= 3.4028234e38f))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: white_level must be positive and finite", what);
  if ((long long)B * Hin * Win * 12 >= (1LL << 40))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: input too large", what);
  if ((long long)B * Hout * Wout == 0) return finish_noop();
  if (!input || !out) return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer", what);
  if (((uintptr_t)input | (uintptr_t)out) & 3u)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: input and out must be 4-B aligned (rows are read as aligned dwords)", what);
  const char* name = "";
  const hipError_t e = launch_resize_bilinear_io(input, input_dtype, white_level, out, B, Hin, Win, Hout, Wout,
                                                 static_cast<hipStream_t>(stream), &name);
  if (e == hipErrorInvalidValue) return fail(HDRNET_INVALID_ARGUMENT, "%s: output too large", what);
  return finish_launch(e, what, name);
}

int hdrnet_bilateral_slice_apply_upadd_io_ex(const float* grid, const float* guide, const void* input,
                                             const float* coarse, int Hc, int Wc, void* out, int B, int H, int W, int GH,
                                             int GW, int GD, int Cin, int Cout, int has_offset, int input_dtype,
                                             float white_level, int output_dtype, const float* guide_conv1,
                                             const float* guide_conv2, int n_feats, unsigned flags, void* stream) {
  using namespace hdrnet_amd;
  if (int rc = check_common(B, H, W, GH, GW, GD)) return rc;
  if (int rc = check_guide_flags(flags)) return rc;
  if (int rc = check_frame_values(Cin, Cout, input_dtype, white_level, output_dtype)) return rc;
  if (int rc = check_upadd_values(Hc, Wc, guide, guide_conv1, guide_conv2, n_feats)) return rc;
  if ((long long)B * H * W == 0) return finish_noop();
  if (!grid || !input || !out || !coarse) return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  ApplyIoArgs a{grid, guide, input, out, B, H, W, GH, GW, GD, Cin, Cout, has_offset != 0,
                input_dtype, output_dtype, white_level, guide_conv1, guide_conv2, n_feats, nullptr};
  if (int rc = set_guide_flags(a, flags, Cin, guide_conv1, guide_conv2)) return rc;
  if (input_dtype == 0 && output_dtype == 0) {
    // float32 both ways: the float op itself (its kernel, its bits)
    return hdrnet_bilateral_slice_apply_upadd_f32_ex(grid, guide, static_cast<const float*>(input), coarse, Hc, Wc,
                                                     static_cast<float*>(out), B, H, W, GH, GW, GD, Cin, Cout, has_offset,
                                                     guide_conv1, guide_conv2, n_feats, flags, stream);
  }
  return launch_io(a, coarse, Hc, Wc, "BilateralSliceApplyUpAddIO",
                   "the wire-format slice-apply + up-add supports Cin = Cout = 3 with offset, W % 4 == 0, aligned "
                   "buffers; convert on the caller's side and use hdrnet_bilateral_slice_apply_upadd_f32", stream);
}

// ---- include/hdrnet_amd_pyramid_yuv.h: the pyramid model on YUV 4:2:0 surfaces -------------------------------------------
// The resize: the surface's rules (check_yuv_extents / check_yuv_surface / check_yuv_pointers and their planar twins), then
// the output's.  An empty OUTPUT is the no-op; an empty surface under a non-empty output has nothing to read.
namespace {
int check_resize_yuv_output(const char* what, int B, int H, int W, int Hout, int Wout) {
  if (Hout < 0 || Wout < 0) return fail(HDRNET_INVALID_ARGUMENT, "%s: negative output extent (%d x %d)", what, Hout, Wout);
  if ((long long)B * Hout * Wout != 0 && (long long)H * W == 0)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: an empty surface (H=%d, W=%d) has no pixel to resize", what, H, W);
  if ((long long)B * Hout * Wout * 12 >= (1LL << 40)) return fail(HDRNET_INVALID_ARGUMENT, "%s: output too large", what);
  return HDRNET_OK;
}
int check_resize_yuv_out(const char* what, const float* out) {
  if (!out || ((uintptr_t)out & 3u)) return fail(HDRNET_INVALID_ARGUMENT, "%s: out must be a 4-B aligned buffer", what);
  return HDRNET_OK;
}
}  // namespace

int hdrnet_resize_bilinear_yuv(const void* y, const void* uv, int sample_dtype, int pitch_y, int pitch_uv,
                               long long image_stride_y, long long image_stride_uv, int B, int H, int W, const float* to_rgb,
                               float* out, int Hout, int Wout, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_resize_bilinear_yuv";
  const YuvSurface in{y, uv, pitch_y, pitch_uv, image_stride_y, image_stride_uv};
  if (int rc = check_yuv_extents(what, B, H, W)) return rc;
  if (int rc = check_yuv_surface(what, "input", sample_dtype, in, B, H, W)) return rc;
  if (int rc = check_resize_yuv_output(what, B, H, W, Hout, Wout)) return rc;
  if ((long long)B * Hout * Wout == 0) return finish_noop();
  if (int rc = check_yuv_pointers(what, "input", in, to_rgb)) return rc;
  if (int rc = check_resize_yuv_out(what, out)) return rc;
  const char* name = "";
  const hipError_t e = launch_resize_bilinear_yuv(in, sample_dtype, to_rgb, out, B, H, W, Hout, Wout,
                                                  static_cast<hipStream_t>(stream), &name);
  if (e == hipErrorInvalidValue) return fail(HDRNET_INVALID_ARGUMENT, "%s: output too large", what);
  return finish_launch(e, what, name);
}

int hdrnet_resize_bilinear_yuv_planar(const void* y, const void* u, const void* v, int sample_dtype, int pitch_y, int pitch_u,
                                      int pitch_v, long long image_stride_y, long long image_stride_u,
                                      long long image_stride_v, int B, int H, int W, const float* to_rgb, float* out,
                                      int Hout, int Wout, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_resize_bilinear_yuv_planar";
  const YuvPlanarSurface in{y, u, v, pitch_y, pitch_u, pitch_v, image_stride_y, image_stride_u, image_stride_v};
  if (int rc = check_yuv_extents(what, B, H, W)) return rc;
  if (int rc = check_yuv_planar_surface(what, "input", sample_dtype, in, B, H, W)) return rc;
  if (int rc = check_resize_yuv_output(what, B, H, W, Hout, Wout)) return rc;
  if ((long long)B * Hout * Wout == 0) return finish_noop();
  if (int rc = check_yuv_planar_pointers(what, "input", sample_dtype, in, to_rgb)) return rc;
  if (int rc = check_resize_yuv_out(what, out)) return rc;
  const char* name = "";
  const hipError_t e = launch_resize_bilinear_yuv_planar(in, sample_dtype, to_rgb, out, B, H, W, Hout, Wout,
                                                         static_cast<hipStream_t>(stream), &name);
  if (e == hipErrorInvalidValue) return fail(HDRNET_INVALID_ARGUMENT, "%s: output too large", what);
  return finish_launch(e, what, name);
}

// The finest level: the single-level surface entry points' bodies (apply_io_yuv_impl / apply_io_yuv_planar_impl: the same
// checks in the same order) with the coarse level beside them.
int hdrnet_bilateral_slice_apply_upadd_io_yuv(const float* grid, const float* guide, const void* y, const void* uv,
                                              int sample_dtype, int pitch_y, int pitch_uv, long long image_stride_y,
                                              long long image_stride_uv, int B, int H, int W, const float* to_rgb,
                                              const float* coarse, int Hc, int Wc, int GH, int GW, int GD, int Cin, int Cout,
                                              int has_offset, const float* guide_conv1, const float* guide_conv2, int n_feats,
                                              unsigned flags, int output_kind, void* out, void* out_uv, int out_pitch_y,
                                              int out_pitch_uv, long long out_image_stride_y, long long out_image_stride_uv,
                                              const float* from_rgb, void* stream) {
  const hdrnet_amd::YuvIo io{{y, uv, pitch_y, pitch_uv, image_stride_y, image_stride_uv}, to_rgb, output_kind,
                             {out, out_uv, out_pitch_y, out_pitch_uv, out_image_stride_y, out_image_stride_uv}, from_rgb};
  const IoCoarse up{coarse, Hc, Wc};
  return apply_io_yuv_impl("hdrnet_bilateral_slice_apply_upadd_io_yuv", false, grid,
                           io_guide_network(guide, guide_conv1, guide_conv2, n_feats, nullptr, flags), io, sample_dtype, B, H,
                           W, GH, GW, GD, Cin, Cout, has_offset, stream, &up);
}

int hdrnet_bilateral_slice_apply_upadd_io_yuv_p016(const float* grid, const float* guide, const void* y, const void* uv,
                                                   int sample_dtype, int pitch_y, int pitch_uv, long long image_stride_y,
                                                   long long image_stride_uv, int B, int H, int W, const float* to_rgb,
                                                   const float* coarse, int Hc, int Wc, int GH, int GW, int GD, int Cin,
                                                   int Cout, int has_offset, const float* guide_conv1,
                                                   const float* guide_conv2, int n_feats, unsigned flags, void* out_y,
                                                   void* out_uv, int out_pitch_y, int out_pitch_uv,
                                                   long long out_image_stride_y, long long out_image_stride_uv,
                                                   const float* from_rgb, int out_bits, void* stream) {
  const hdrnet_amd::YuvIo io{{y, uv, pitch_y, pitch_uv, image_stride_y, image_stride_uv}, to_rgb, hdrnet_amd::kYuvOutP016,
                             {out_y, out_uv, out_pitch_y, out_pitch_uv, out_image_stride_y, out_image_stride_uv}, from_rgb,
                             out_bits};
  const IoCoarse up{coarse, Hc, Wc};
  return apply_io_yuv_impl("hdrnet_bilateral_slice_apply_upadd_io_yuv_p016", true, grid,
                           io_guide_network(guide, guide_conv1, guide_conv2, n_feats, nullptr, flags), io, sample_dtype, B, H,
                           W, GH, GW, GD, Cin, Cout, has_offset, stream, &up);
}

int hdrnet_bilateral_slice_apply_upadd_io_yuv_planar(const float* grid, const float* guide, const void* y, const void* u,
                                                     const void* v, int sample_dtype, int pitch_y, int pitch_u, int pitch_v,
                                                     long long image_stride_y, long long image_stride_u,
                                                     long long image_stride_v, int B, int H, int W, const float* to_rgb,
                                                     const float* coarse, int Hc, int Wc, int GH, int GW, int GD, int Cin,
                                                     int Cout, int has_offset, const float* guide_conv1,
                                                     const float* guide_conv2, int n_feats, unsigned flags, int output_kind,
                                                     void* out, void* out_u, void* out_v, int out_pitch_y, int out_pitch_u,
                                                     int out_pitch_v, long long out_image_stride_y,
                                                     long long out_image_stride_u, long long out_image_stride_v,
                                                     const float* from_rgb, int out_bits, void* stream) {
  const hdrnet_amd::YuvPlanarIo io{
      {y, u, v, pitch_y, pitch_u, pitch_v, image_stride_y, image_stride_u, image_stride_v}, to_rgb, output_kind,
      {out, out_u, out_v, out_pitch_y, out_pitch_u, out_pitch_v, out_image_stride_y, out_image_stride_u, out_image_stride_v},
      from_rgb, out_bits};
  const IoCoarse up{coarse, Hc, Wc};
  return apply_io_yuv_planar_impl("hdrnet_bilateral_slice_apply_upadd_io_yuv_planar", grid,
                                  io_guide_network(guide, guide_conv1, guide_conv2, n_feats, nullptr, flags), io, sample_dtype,
                                  B, H, W, GH, GW, GD, Cin, Cout, has_offset, stream, &up);
}

// ---- sample preparation (sample_prep.hip): hdrnet_prepare_batch* of include/hdrnet_amd_train.h, and the low-res network
// input from frames in each of the wire formats above -------------------------------------------------------------------
// Sample preparation (sample_prep.hip).  Everything is checked before any HIP call.  `ragged`: the sources are flat
// buffers of n_samples samples with the descriptor table `images` (hdrnet_prepare_batch_ragged); Hs / Ws are then unused
// and the fit of the crop is a matter of the table (the device clamps).
static int prepare_impl(const char* what, const void* src_input, int input_dtype, float input_white_level,
                        const void* src_target, int target_dtype, float target_white_level, int N, int Hs, int Ws,
                        const int* ops, int B, float* image_input, float* image_target, int H, int W,
                        float* lowres_input, int net_input_size, unsigned flags, void* stream, bool ragged = false,
                        long long n_samples = 0, const int* images = nullptr, int pixel_format = 0) {
  using namespace hdrnet_amd;
  if (ragged) Hs = Ws = 1;  // unused
  if (flags & ~HDRNET_SAMPLE_EVEN_TURNS_ONLY)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: unknown flags 0x%x (takes HDRNET_SAMPLE_EVEN_TURNS_ONLY)", what, flags);
  if (input_dtype < 0 || input_dtype > 2 || (src_target && (target_dtype < 0 || target_dtype > 2)))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: unknown dtype code (input %d, target %d; 0 f32, 1 u8, 2 u16)", what,
                input_dtype, target_dtype);
  if (!(input_white_level > 0.0f) || !(input_white_level <= 3.4028234e38f) ||
      (src_target && (!(target_white_level > 0.0f) || !(target_white_level <= 3.4028234e38f))))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: white levels must be positive and finite", what);
  if (ragged && N <= 0) return fail(HDRNET_INVALID_ARGUMENT, "%s: the image table is empty (N=%d)", what, N);
  if (ragged && n_samples <= 0)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the source buffers are empty (n_samples=%lld)", what, n_samples);
  if (B < 0 || N <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || (lowres_input && net_input_size <= 0))
    return fail(HDRNET_INVALID_ARGUMENT,
                "%s: non-positive extent (N=%d, Hs=%d, Ws=%d, B=%d, H=%d, W=%d, net_input_size=%d)", what, N, Hs, Ws, B,
                H, W, net_input_size);
  if (!ragged && (H > Hs || W > Ws))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the crop %d x %d does not fit the %d x %d source", what, H, W, Hs, Ws);
  if (!ragged && !(flags & HDRNET_SAMPLE_EVEN_TURNS_ONLY) && ops && (H > Ws || W > Hs))
    return fail(HDRNET_INVALID_ARGUMENT,
                "%s: the crop %d x %d does not fit the source turned by 90 degrees (%d x %d); pass "
                "HDRNET_SAMPLE_EVEN_TURNS_ONLY", what, H, W, Ws, Hs);
  if (!ragged && !ops && (B > N || H != Hs || W != Ws))
    return fail(HDRNET_INVALID_ARGUMENT,
                "%s: ops == NULL is the identity (sample b = source b, whole image): needs B <= N and (H, W) == (Hs, Ws)",
                what);
  if ((long long)Hs * Ws * 12 >= (1LL << 31) || (long long)H * W * 12 >= (1LL << 31) || (long long)net_input_size * net_input_size * 12 >= (1LL << 31) || B > 65535)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: image or batch too large", what);
  if (B == 0) return finish_noop();
  if (!src_input) return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer (the input sources)", what);
  if (ragged && !images) return fail(HDRNET_INVALID_ARGUMENT, "%s: null image table (images)", what);
  if (ragged && !ops)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: null ops: there is no identity geometry over images of mixed extents", what);
  if (image_target && !src_target)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: image_target given without src_target", what);
  if (!image_input && !image_target && !lowres_input)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer (no output requested)", what);
  if ((image_input || image_target) && W % 4 != 0)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: W %% 4 != 0 (W=%d): rows are stored as whole 16-byte vectors", what, W);
  if (((uintptr_t)image_input | (uintptr_t)image_target | (uintptr_t)lowres_input) & 15u)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: outputs must be 16-B aligned", what);
  if (((uintptr_t)src_input | (uintptr_t)src_target | (uintptr_t)ops) & 3u)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: sources and ops must be 4-B aligned", what);
  if ((uintptr_t)images & 15u)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the image table must be 16-B aligned (one 16-byte read per descriptor)", what);
  SamplePrepArgs a{src_input, src_target, input_dtype, src_target ? target_dtype : 0, input_white_level,
                         src_target ? target_white_level : 1.0f, N, Hs, Ws, ops, B, H, W, image_input, image_target,
                         lowres_input, lowres_input ? net_input_size : 0, (flags & HDRNET_SAMPLE_EVEN_TURNS_ONLY) != 0};
  a.images = images;
  a.n_samples = n_samples;
  a.pixel_format = pixel_format;  // the low-res gather of hdrnet_lowres_input_px; every other caller: RGB
  return finish_launch(launch_sample_prep(a, static_cast<hipStream_t>(stream)), what,
                       ragged ? "sample_prep_ragged" : "sample_prep");
}

int hdrnet_prepare_batch(const void* src_input, int input_dtype, float input_white_level, const void* src_target,
                         int target_dtype, float target_white_level, int N, int Hs, int Ws, const int* ops, int B,
                         float* image_input, float* image_target, int H, int W, float* lowres_input,
                         int net_input_size, unsigned flags, void* stream) {
  return prepare_impl("hdrnet_prepare_batch", src_input, input_dtype, input_white_level, src_target, target_dtype,
                      target_white_level, N, Hs, Ws, ops, B, image_input, image_target, H, W, lowres_input,
                      net_input_size, flags, stream);
}

int hdrnet_prepare_batch_ragged(const void* src_input, int input_dtype, float input_white_level, const void* src_target,
                                int target_dtype, float target_white_level, long long n_samples, const int* images, int N,
                                const int* ops, int B, float* image_input, float* image_target, int H, int W,
                                float* lowres_input, int net_input_size, unsigned flags, void* stream) {
  return prepare_impl("hdrnet_prepare_batch_ragged", src_input, input_dtype, input_white_level, src_target, target_dtype,
                      target_white_level, N, 0, 0, ops, B, image_input, image_target, H, W, lowres_input, net_input_size,
                      flags, stream, true, n_samples, images);
}

int hdrnet_lowres_input(const void* frames, int dtype, float white_level, int B, int H, int W, float* lowres,
                        int net_input_size, void* stream) {
  if (B > 0 && !lowres) return fail(HDRNET_INVALID_ARGUMENT, "hdrnet_lowres_input: null buffer (lowres)");
  return prepare_impl("hdrnet_lowres_input", frames, dtype, white_level, nullptr, 0, 1.0f, B > 0 ? B : 1, H, W, nullptr,
                      B, nullptr, nullptr, H, W, lowres, net_input_size, 0u, stream);
}

int hdrnet_lowres_input_px(const void* frames, int dtype, float white_level, int B, int H, int W, float* lowres,
                           int net_input_size, int pixel_format, void* stream) {
  const char* what = "hdrnet_lowres_input_px";
  if (pixel_format == HDRNET_PX_RGB) return hdrnet_lowres_input(frames, dtype, white_level, B, H, W, lowres, net_input_size, stream);
  if (int rc = check_input_dtype(what, dtype)) return rc;
  if (int rc = check_pixel_formats(what, dtype, 0, pixel_format, HDRNET_PX_RGB)) return rc;
  if (B > 0 && !lowres) return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer (lowres)", what);
  if (B > 0 && pixel_format >= HDRNET_PX_RGBA && ((uintptr_t)frames & 15u))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: 4-channel frames (RGBA / BGRA) must be 16-B aligned", what);
  return prepare_impl(what, frames, dtype, white_level, nullptr, 0, 1.0f, B > 0 ? B : 1, H, W, nullptr, B, nullptr, nullptr,
                      H, W, lowres, net_input_size, 0u, stream, false, 0, nullptr, pixel_format);
}

int hdrnet_lowres_input_yuv(const void* y, const void* uv, int sample_dtype, int pitch_y, int pitch_uv,
                            long long image_stride_y, long long image_stride_uv, int B, int H, int W, const float* to_rgb,
                            float* lowres, int net_input_size, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_lowres_input_yuv";
  const YuvSurface in{y, uv, pitch_y, pitch_uv, image_stride_y, image_stride_uv};
  if (int rc = check_yuv_extents(what, B, H, W)) return rc;
  if (int rc = check_yuv_surface(what, "input", sample_dtype, in, B, H, W)) return rc;
  if (H <= 0 || W <= 0 || net_input_size <= 0 || (long long)net_input_size * net_input_size * 12 >= (1LL << 31))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: non-positive extent (H=%d, W=%d, net_input_size=%d)", what, H, W, net_input_size);
  if (B == 0) return finish_noop();
  if (int rc = check_yuv_pointers(what, "input", in, to_rgb)) return rc;
  if (!lowres || ((uintptr_t)lowres & 15u)) return fail(HDRNET_INVALID_ARGUMENT, "%s: lowres must be a 16-B aligned buffer", what);
  SamplePrepArgs a{y, nullptr, sample_dtype, 0, 1.0f, 1.0f, B, H, W, nullptr, B, H, W, nullptr, nullptr, lowres, net_input_size,
                   false};
  a.yuv = &in;
  a.yuv_to_rgb = to_rgb;
  return finish_launch(launch_sample_prep(a, static_cast<hipStream_t>(stream)), what, "sample_prep");
}

int hdrnet_lowres_input_yuv_planar(const void* y, const void* u, const void* v, int sample_dtype, int pitch_y, int pitch_u,
                                   int pitch_v, long long image_stride_y, long long image_stride_u,
                                   long long image_stride_v, int B, int H, int W, const float* to_rgb, float* lowres,
                                   int net_input_size, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_lowres_input_yuv_planar";
  const YuvPlanarSurface in{y, u, v, pitch_y, pitch_u, pitch_v, image_stride_y, image_stride_u, image_stride_v};
  if (int rc = check_yuv_extents(what, B, H, W)) return rc;
  if (int rc = check_yuv_planar_surface(what, "input", sample_dtype, in, B, H, W)) return rc;
  if (H <= 0 || W <= 0 || net_input_size <= 0 || (long long)net_input_size * net_input_size * 12 >= (1LL << 31))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: non-positive extent (H=%d, W=%d, net_input_size=%d)", what, H, W, net_input_size);
  if (B == 0) return finish_noop();
  if (int rc = check_yuv_planar_pointers(what, "input", sample_dtype, in, to_rgb)) return rc;
  if (!lowres || ((uintptr_t)lowres & 15u)) return fail(HDRNET_INVALID_ARGUMENT, "%s: lowres must be a 16-B aligned buffer", what);
  SamplePrepArgs a{y, nullptr, sample_dtype, 0, 1.0f, 1.0f, B, H, W, nullptr, B, H, W, nullptr, nullptr, lowres, net_input_size,
                   false};
  a.yuv_planar = &in;
  a.yuv_to_rgb = to_rgb;
  return finish_launch(launch_sample_prep(a, static_cast<hipStream_t>(stream)), what, "sample_prep");
}

// ---- include/hdrnet_amd_yuv_chroma.h: 4:2:2 / 4:4:4 surfaces -- the entry points above with a chroma layout -------------------
// With HDRNET_CHROMA_420 each one forwards to the entry point it mirrors; otherwise it runs that entry point's body -- the same
// checks in the same order -- with the layout in the surface rules.
namespace {

// the layout code, for a semi-planar (`planar` false: no 4:4:4) or a planar surface
int check_chroma_code(const char* what, int chroma, bool planar) {
  if (chroma < HDRNET_CHROMA_420 || chroma > HDRNET_CHROMA_444)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: unknown chroma layout code %d (0 4:2:0, 1 4:2:2, 2 4:4:4)", what, chroma);
  if (!planar && chroma == HDRNET_CHROMA_444)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: semi-planar 4:4:4 (NV24 / P410) is out of scope: 4:4:4 surfaces are planar "
                "(yuv444p, yuv444p10le / yuv444p16le)", what);
  return HDRNET_OK;
}

// the output kind; a planar surface output has the input's sample width
int check_chroma_out_kind(const char* what, int kind, int sample_dtype, bool planar) {
  if (kind < HDRNET_CHROMA_OUT_RGB_F32 || kind > HDRNET_CHROMA_OUT_SURFACE_U16)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: unknown output kind %d (0 float32 RGB, 1 uint8 RGB, 2 a uint8 surface, 3 a uint16 "
                "surface of the input's container and chroma layout)", what, kind);
  if (planar && kind >= HDRNET_CHROMA_OUT_SURFACE_U8 && (sample_dtype == 1 || sample_dtype == 2) &&
      (kind == HDRNET_CHROMA_OUT_SURFACE_U8) != (sample_dtype == 1))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: a planar surface output has the input's sample width (output kind %d, a %s surface, "
                "for sample_dtype %d)", what, kind, kind == HDRNET_CHROMA_OUT_SURFACE_U8 ? "uint8" : "uint16", sample_dtype);
  return HDRNET_OK;
}

}  // namespace

int hdrnet_yuv_chroma_to_rgb_f32(const void* y, const void* uv, int sample_dtype, int pitch_y, int pitch_uv,
                                 long long image_stride_y, long long image_stride_uv, int chroma, int B, int H, int W,
                                 const float* to_rgb, float* rgb, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_yuv_chroma_to_rgb_f32";
  if (int rc = check_chroma_code(what, chroma, false)) return rc;
  if (chroma == HDRNET_CHROMA_420)
    return hdrnet_yuv_to_rgb_f32(y, uv, sample_dtype, pitch_y, pitch_uv, image_stride_y, image_stride_uv, B, H, W, to_rgb, rgb,
                                 stream);
  const YuvSurface in{y, uv, pitch_y, pitch_uv, image_stride_y, image_stride_uv};
  if (int rc = check_yuv_extents(what, B, H, W, chroma)) return rc;
  if (int rc = check_yuv_surface(what, "input", sample_dtype, in, B, H, W, chroma)) return rc;
  if ((long long)B * H * W == 0) return finish_noop();
  if (int rc = check_yuv_pointers(what, "input", in, to_rgb)) return rc;
  if (!rgb || ((uintptr_t)rgb & 15u)) return fail(HDRNET_INVALID_ARGUMENT, "%s: rgb must be a 16-B aligned buffer", what);
  return finish_launch(launch_yuv_422_to_rgb(in, sample_dtype, to_rgb, rgb, B, H, W, static_cast<hipStream_t>(stream)), what,
                       "yuv_422_to_rgb");
}

int hdrnet_yuv_planar_chroma_to_rgb_f32(const void* y, const void* u, const void* v, int sample_dtype, int pitch_y,
                                        int pitch_u, int pitch_v, long long image_stride_y, long long image_stride_u,
                                        long long image_stride_v, int chroma, int B, int H, int W, const float* to_rgb,
                                        float* rgb, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_yuv_planar_chroma_to_rgb_f32";
  if (int rc = check_chroma_code(what, chroma, true)) return rc;
  if (chroma == HDRNET_CHROMA_420)
    return hdrnet_yuv_planar_to_rgb_f32(y, u, v, sample_dtype, pitch_y, pitch_u, pitch_v, image_stride_y, image_stride_u,
                                        image_stride_v, B, H, W, to_rgb, rgb, stream);
  const YuvPlanarSurface in{y, u, v, pitch_y, pitch_u, pitch_v, image_stride_y, image_stride_u, image_stride_v};
  if (int rc = check_yuv_extents(what, B, H, W, chroma)) return rc;
  if (int rc = check_yuv_planar_surface(what, "input", sample_dtype, in, B, H, W, chroma)) return rc;
  if ((long long)B * H * W == 0) return finish_noop();
  if (int rc = check_yuv_planar_pointers(what, "input", sample_dtype, in, to_rgb, chroma)) return rc;
  if (!rgb || ((uintptr_t)rgb & 15u)) return fail(HDRNET_INVALID_ARGUMENT, "%s: rgb must be a 16-B aligned buffer", what);
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (chroma == HDRNET_CHROMA_422)
    return finish_launch(launch_yuv_planar_422_to_rgb(in, sample_dtype, to_rgb, rgb, B, H, W, s), what, "yuv_planar_422_to_rgb");
  return finish_launch(launch_yuv_planar_444_to_rgb(in, sample_dtype, to_rgb, rgb, B, H, W, s), what, "yuv_planar_444_to_rgb");
}

int hdrnet_lowres_input_yuv_chroma(const void* y, const void* uv, int sample_dtype, int pitch_y, int pitch_uv,
                                   long long image_stride_y, long long image_stride_uv, int chroma, int B, int H, int W,
                                   const float* to_rgb, float* lowres, int net_input_size, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_lowres_input_yuv_chroma";
  if (int rc = check_chroma_code(what, chroma, false)) return rc;
  if (chroma == HDRNET_CHROMA_420)
    return hdrnet_lowres_input_yuv(y, uv, sample_dtype, pitch_y, pitch_uv, image_stride_y, image_stride_uv, B, H, W, to_rgb,
                                   lowres, net_input_size, stream);
  const YuvSurface in{y, uv, pitch_y, pitch_uv, image_stride_y, image_stride_uv};
  if (int rc = check_yuv_extents(what, B, H, W, chroma)) return rc;
  if (int rc = check_yuv_surface(what, "input", sample_dtype, in, B, H, W, chroma)) return rc;
  if (H <= 0 || W <= 0 || net_input_size <= 0 || (long long)net_input_size * net_input_size * 12 >= (1LL << 31))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: non-positive extent (H=%d, W=%d, net_input_size=%d)", what, H, W, net_input_size);
  if (B == 0) return finish_noop();
  if (int rc = check_yuv_pointers(what, "input", in, to_rgb)) return rc;
  if (!lowres || ((uintptr_t)lowres & 15u)) return fail(HDRNET_INVALID_ARGUMENT, "%s: lowres must be a 16-B aligned buffer", what);
  SamplePrepArgs a{y, nullptr, sample_dtype, 0, 1.0f, 1.0f, B, H, W, nullptr, B, H, W, nullptr, nullptr, lowres, net_input_size,
                   false};
  a.yuv = &in;
  a.yuv_to_rgb = to_rgb;
  a.yuv_chroma = chroma;
  return finish_launch(launch_sample_prep(a, static_cast<hipStream_t>(stream)), what, "sample_prep");
}

int hdrnet_lowres_input_yuv_planar_chroma(const void* y, const void* u, const void* v, int sample_dtype, int pitch_y,
                                          int pitch_u, int pitch_v, long long image_stride_y, long long image_stride_u,
                                          long long image_stride_v, int chroma, int B, int H, int W, const float* to_rgb,
                                          float* lowres, int net_input_size, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_lowres_input_yuv_planar_chroma";
  if (int rc = check_chroma_code(what, chroma, true)) return rc;
  if (chroma == HDRNET_CHROMA_420)
    return hdrnet_lowres_input_yuv_planar(y, u, v, sample_dtype, pitch_y, pitch_u, pitch_v, image_stride_y, image_stride_u,
                                          image_stride_v, B, H, W, to_rgb, lowres, net_input_size, stream);
  const YuvPlanarSurface in{y, u, v, pitch_y, pitch_u, pitch_v, image_stride_y, image_stride_u, image_stride_v};
  if (int rc = check_yuv_extents(what, B, H, W, chroma)) return rc;
  if (int rc = check_yuv_planar_surface(what, "input", sample_dtype, in, B, H, W, chroma)) return rc;
  if (H <= 0 || W <= 0 || net_input_size <= 0 || (long long)net_input_size * net_input_size * 12 >= (1LL << 31))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: non-positive extent (H=%d, W=%d, net_input_size=%d)", what, H, W, net_input_size);
  if (B == 0) return finish_noop();
  if (int rc = check_yuv_planar_pointers(what, "input", sample_dtype, in, to_rgb, chroma)) return rc;
  if (!lowres || ((uintptr_t)lowres & 15u)) return fail(HDRNET_INVALID_ARGUMENT, "%s: lowres must be a 16-B aligned buffer", what);
  SamplePrepArgs a{y, nullptr, sample_dtype, 0, 1.0f, 1.0f, B, H, W, nullptr, B, H, W, nullptr, nullptr, lowres, net_input_size,
                   false};
  a.yuv_planar = &in;
  a.yuv_to_rgb = to_rgb;
  a.yuv_chroma = chroma;
  return finish_launch(launch_sample_prep(a, static_cast<hipStream_t>(stream)), what, "sample_prep");
}

int hdrnet_bilateral_slice_apply_io_yuv_chroma(const float* grid, const float* guide, const void* y, const void* uv,
                                               int sample_dtype, int pitch_y, int pitch_uv, long long image_stride_y,
                                               long long image_stride_uv, int chroma, int B, int H, int W,
                                               const float* to_rgb, int GH, int GW, int GD, int Cin, int Cout,
                                               int has_offset, const float* guide_conv1, const float* guide_conv2,
                                               int n_feats, float* guide_out, unsigned flags, int output_kind, void* out,
                                               void* out_uv, int out_pitch_y, int out_pitch_uv,
                                               long long out_image_stride_y, long long out_image_stride_uv,
                                               const float* from_rgb, int out_bits, void* stream) {
  const char* what = "hdrnet_bilateral_slice_apply_io_yuv_chroma";
  if (int rc = check_chroma_code(what, chroma, false)) return rc;
  if (int rc = check_chroma_out_kind(what, output_kind, sample_dtype, false)) return rc;
  const bool deep = output_kind == HDRNET_CHROMA_OUT_SURFACE_U16;
  if (chroma == HDRNET_CHROMA_420) {
    if (deep)
      return hdrnet_bilateral_slice_apply_io_yuv_p016(grid, guide, y, uv, sample_dtype, pitch_y, pitch_uv, image_stride_y,
                                                      image_stride_uv, B, H, W, to_rgb, GH, GW, GD, Cin, Cout, has_offset,
                                                      guide_conv1, guide_conv2, n_feats, guide_out, flags, out, out_uv,
                                                      out_pitch_y, out_pitch_uv, out_image_stride_y, out_image_stride_uv,
                                                      from_rgb, out_bits, stream);
    return hdrnet_bilateral_slice_apply_io_yuv(grid, guide, y, uv, sample_dtype, pitch_y, pitch_uv, image_stride_y,
                                               image_stride_uv, B, H, W, to_rgb, GH, GW, GD, Cin, Cout, has_offset,
                                               guide_conv1, guide_conv2, n_feats, guide_out, flags, output_kind, out, out_uv,
                                               out_pitch_y, out_pitch_uv, out_image_stride_y, out_image_stride_uv, from_rgb,
                                               stream);
  }
  const hdrnet_amd::YuvIo io{{y, uv, pitch_y, pitch_uv, image_stride_y, image_stride_uv}, to_rgb, output_kind,
                             {out, out_uv, out_pitch_y, out_pitch_uv, out_image_stride_y, out_image_stride_uv}, from_rgb,
                             deep ? out_bits : 0, chroma};
  return apply_io_yuv_impl(what, deep, grid, io_guide_network(guide, guide_conv1, guide_conv2, n_feats, guide_out, flags), io,
                           sample_dtype, B, H, W, GH, GW, GD, Cin, Cout, has_offset, stream);
}

int hdrnet_bilateral_slice_apply_io_curves_yuv_chroma(const float* grid, const void* y, const void* uv, int sample_dtype,
                                                      int pitch_y, int pitch_uv, long long image_stride_y,
                                                      long long image_stride_uv, int chroma, int B, int H, int W,
                                                      const float* to_rgb, int GH, int GW, int GD, int Cin, int Cout,
                                                      int has_offset, const float* guide_ccm, const float* guide_shifts,
                                                      const float* guide_slopes, const float* guide_mix, int npts,
                                                      const void* prepared, float* guide_out, int output_kind, void* out,
                                                      void* out_uv, int out_pitch_y, int out_pitch_uv,
                                                      long long out_image_stride_y, long long out_image_stride_uv,
                                                      const float* from_rgb, int out_bits, void* stream) {
  const char* what = "hdrnet_bilateral_slice_apply_io_curves_yuv_chroma";
  if (int rc = check_chroma_code(what, chroma, false)) return rc;
  if (int rc = check_chroma_out_kind(what, output_kind, sample_dtype, false)) return rc;
  const bool deep = output_kind == HDRNET_CHROMA_OUT_SURFACE_U16;
  if (chroma == HDRNET_CHROMA_420) {
    if (deep)
      return hdrnet_bilateral_slice_apply_io_curves_yuv_p016(grid, y, uv, sample_dtype, pitch_y, pitch_uv, image_stride_y,
                                                             image_stride_uv, B, H, W, to_rgb, GH, GW, GD, Cin, Cout,
                                                             has_offset, guide_ccm, guide_shifts, guide_slopes, guide_mix,
                                                             npts, prepared, guide_out, out, out_uv, out_pitch_y,
                                                             out_pitch_uv, out_image_stride_y, out_image_stride_uv, from_rgb,
                                                             out_bits, stream);
    return hdrnet_bilateral_slice_apply_io_curves_yuv(grid, y, uv, sample_dtype, pitch_y, pitch_uv, image_stride_y,
                                                      image_stride_uv, B, H, W, to_rgb, GH, GW, GD, Cin, Cout, has_offset,
                                                      guide_ccm, guide_shifts, guide_slopes, guide_mix, npts, prepared,
                                                      guide_out, output_kind, out, out_uv, out_pitch_y, out_pitch_uv,
                                                      out_image_stride_y, out_image_stride_uv, from_rgb, stream);
  }
  const hdrnet_amd::YuvIo io{{y, uv, pitch_y, pitch_uv, image_stride_y, image_stride_uv}, to_rgb, output_kind,
                             {out, out_uv, out_pitch_y, out_pitch_uv, out_image_stride_y, out_image_stride_uv}, from_rgb,
                             deep ? out_bits : 0, chroma};
  return apply_io_yuv_impl(what, deep, grid,
                           io_guide_curves(guide_ccm, guide_shifts, guide_slopes, guide_mix, npts, prepared, guide_out), io,
                           sample_dtype, B, H, W, GH, GW, GD, Cin, Cout, has_offset, stream);
}

int hdrnet_bilateral_slice_apply_io_yuv_planar_chroma(const float* grid, const float* guide, const void* y, const void* u,
                                                      const void* v, int sample_dtype, int pitch_y, int pitch_u,
                                                      int pitch_v, long long image_stride_y, long long image_stride_u,
                                                      long long image_stride_v, int chroma, int B, int H, int W,
                                                      const float* to_rgb, int GH, int GW, int GD, int Cin, int Cout,
                                                      int has_offset, const float* guide_conv1, const float* guide_conv2,
                                                      int n_feats, float* guide_out, unsigned flags, int output_kind,
                                                      void* out, void* out_u, void* out_v, int out_pitch_y, int out_pitch_u,
                                                      int out_pitch_v, long long out_image_stride_y,
                                                      long long out_image_stride_u, long long out_image_stride_v,
                                                      const float* from_rgb, int out_bits, void* stream) {
  const char* what = "hdrnet_bilateral_slice_apply_io_yuv_planar_chroma";
  if (int rc = check_chroma_code(what, chroma, true)) return rc;
  if (int rc = check_chroma_out_kind(what, output_kind, sample_dtype, true)) return rc;
  // (both surface kinds are the planar header's one: a planar surface of the input's sample dtype)
  const int kind = output_kind >= HDRNET_CHROMA_OUT_SURFACE_U8 ? HDRNET_YUV_PLANAR_OUT_PLANAR : output_kind;
  if (chroma == HDRNET_CHROMA_420)
    return hdrnet_bilateral_slice_apply_io_yuv_planar(grid, guide, y, u, v, sample_dtype, pitch_y, pitch_u, pitch_v,
                                                      image_stride_y, image_stride_u, image_stride_v, B, H, W, to_rgb, GH, GW,
                                                      GD, Cin, Cout, has_offset, guide_conv1, guide_conv2, n_feats, guide_out,
                                                      flags, kind, out, out_u, out_v, out_pitch_y, out_pitch_u, out_pitch_v,
                                                      out_image_stride_y, out_image_stride_u, out_image_stride_v, from_rgb,
                                                      out_bits, stream);
  const hdrnet_amd::YuvPlanarIo io{
      {y, u, v, pitch_y, pitch_u, pitch_v, image_stride_y, image_stride_u, image_stride_v}, to_rgb, kind,
      {out, out_u, out_v, out_pitch_y, out_pitch_u, out_pitch_v, out_image_stride_y, out_image_stride_u, out_image_stride_v},
      from_rgb, out_bits, chroma};
  return apply_io_yuv_planar_impl(what, grid, io_guide_network(guide, guide_conv1, guide_conv2, n_feats, guide_out, flags), io,
                                  sample_dtype, B, H, W, GH, GW, GD, Cin, Cout, has_offset, stream);
}

int hdrnet_bilateral_slice_apply_io_curves_yuv_planar_chroma(const float* grid, const void* y, const void* u, const void* v,
                                                             int sample_dtype, int pitch_y, int pitch_u, int pitch_v,
                                                             long long image_stride_y, long long image_stride_u,
                                                             long long image_stride_v, int chroma, int B, int H, int W,
                                                             const float* to_rgb, int GH, int GW, int GD, int Cin, int Cout,
                                                             int has_offset, const float* guide_ccm,
                                                             const float* guide_shifts, const float* guide_slopes,
                                                             const float* guide_mix, int npts, const void* prepared,
                                                             float* guide_out, int output_kind, void* out, void* out_u,
                                                             void* out_v, int out_pitch_y, int out_pitch_u, int out_pitch_v,
                                                             long long out_image_stride_y, long long out_image_stride_u,
                                                             long long out_image_stride_v, const float* from_rgb,
                                                             int out_bits, void* stream) {
  const char* what = "hdrnet_bilateral_slice_apply_io_curves_yuv_planar_chroma";
  if (int rc = check_chroma_code(what, chroma, true)) return rc;
  if (int rc = check_chroma_out_kind(what, output_kind, sample_dtype, true)) return rc;
  const int kind = output_kind >= HDRNET_CHROMA_OUT_SURFACE_U8 ? HDRNET_YUV_PLANAR_OUT_PLANAR : output_kind;
  if (chroma == HDRNET_CHROMA_420)
    return hdrnet_bilateral_slice_apply_io_curves_yuv_planar(grid, y, u, v, sample_dtype, pitch_y, pitch_u, pitch_v,
                                                             image_stride_y, image_stride_u, image_stride_v, B, H, W, to_rgb,
                                                             GH, GW, GD, Cin, Cout, has_offset, guide_ccm, guide_shifts,
                                                             guide_slopes, guide_mix, npts, prepared, guide_out, kind, out,
                                                             out_u, out_v, out_pitch_y, out_pitch_u, out_pitch_v,
                                                             out_image_stride_y, out_image_stride_u, out_image_stride_v,
                                                             from_rgb, out_bits, stream);
  const hdrnet_amd::YuvPlanarIo io{
      {y, u, v, pitch_y, pitch_u, pitch_v, image_stride_y, image_stride_u, image_stride_v}, to_rgb, kind,
      {out, out_u, out_v, out_pitch_y, out_pitch_u, out_pitch_v, out_image_stride_y, out_image_stride_u, out_image_stride_v},
      from_rgb, out_bits, chroma};
  return apply_io_yuv_planar_impl(what, grid,
                                  io_guide_curves(guide_ccm, guide_shifts, guide_slopes, guide_mix, npts, prepared, guide_out),
                                  io, sample_dtype, B, H, W, GH, GW, GD, Cin, Cout, has_offset, stream);
}

// ---- include/hdrnet_amd_yuv_packed.h: packed 4:2:2 surfaces -- the semi-planar 4:2:2 entry points above on ONE plane ------------
// The extents are check_yuv_extents' for HDRNET_CHROMA_422, the guides' rules and the launch tail those of every wire-format
// forward; what one woven plane adds is stated once below and shared by the four entry points (`which`: "input" / "output").
namespace {

int check_yuv_packed_surface(const char* what, const char* which, int sample_dtype, const hdrnet_amd::YuvPackedSurface& s, int B,
                             int H, int W) {
  if (sample_dtype != 1 && sample_dtype != 2)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: unknown sample dtype code of the %s surface (%d; 1 u8, 2 u16: packed surfaces "
                "hold integer samples)", what, which, sample_dtype);
  if (s.order < HDRNET_PACKED_YUYV || s.order > HDRNET_PACKED_YVYU)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: unknown byte order code %d of the %s surface (0 YUYV, 1 UYVY, 2 YVYU)", what, s.order,
                which);
  if (sample_dtype == 2 && s.order != HDRNET_PACKED_YUYV)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: uint16 samples (Y210 / Y216) take HDRNET_PACKED_YUYV only (order %d of the %s "
                "surface: UYVY and YVYU are 8-bit orders)", what, s.order, which);
  const long long row = 2LL * W * sample_dtype;
  if (s.pitch < row)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the pitch of the %s surface is below the row's %lld bytes (pitch=%d; a packed row "
                "holds 2 W samples)", what, which, row, s.pitch);
  if (s.pitch & 3)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the pitch of the %s surface must be a multiple of 4 (pitch=%d)", what, which, s.pitch);
  if (s.image < 0 || (s.image & 3))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the image stride of the %s surface must be a non-negative multiple of 4", what, which);
  if (B > 1 && s.image < (long long)s.pitch * H)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the image stride of the %s surface is below its plane (pitch * H)", what, which);
  return HDRNET_OK;
}

int check_yuv_packed_pointers(const char* what, const char* which, const hdrnet_amd::YuvPackedSurface& s, const float* coef) {
  if (!s.p) return fail(HDRNET_INVALID_ARGUMENT, "%s: null %s surface", what, which);
  if (!coef) return fail(HDRNET_INVALID_ARGUMENT, "%s: null constants of the %s surface (the 12 floats)", what, which);
  if (((uintptr_t)s.p | (uintptr_t)coef) & 3u)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: the %s surface and its constants must be 4-B aligned", what, which);
  return HDRNET_OK;
}

// ... and of a fused forward's surfaces and output.  io.out.p is `out` whatever the output kind.
int check_yuv_packed_io_values(const char* what, const hdrnet_amd::YuvPackedIo& io, int sample_dtype, int B, int H, int W,
                               int Cin, int Cout, int has_offset) {
  if (int rc = check_yuv_extents(what, B, H, W, HDRNET_CHROMA_422)) return rc;
  if (int rc = check_yuv_packed_surface(what, "input", sample_dtype, io.in, B, H, W)) return rc;
  if (int rc = check_chroma_out_kind(what, io.out_kind, sample_dtype, false)) return rc;
  const bool surface_out = io.out_kind >= HDRNET_CHROMA_OUT_SURFACE_U8;
  if (surface_out && (io.out_kind == HDRNET_CHROMA_OUT_SURFACE_U8) != (sample_dtype == 1))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: a packed surface output has the input's sample width (output kind %d, a %s surface, "
                "for sample_dtype %d)", what, io.out_kind, io.out_kind == HDRNET_CHROMA_OUT_SURFACE_U8 ? "uint8" : "uint16",
                sample_dtype);
  if (io.out_kind == HDRNET_CHROMA_OUT_SURFACE_U16 && io.out_bits != 10 && io.out_bits != 16)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: out_bits must be 10 (Y210) or 16 (Y216), got %d", what, io.out_bits);
  if (Cin != 3 || Cout != 3 || !has_offset)
    return fail(HDRNET_INVALID_ARGUMENT, "%s: a YUV surface needs Cin = Cout = 3 with offset (the op sees R, G, B)", what);
  if (surface_out) return check_yuv_packed_surface(what, "output", sample_dtype, io.out, B, H, W);
  return HDRNET_OK;
}

int check_yuv_packed_io_pointers(const char* what, const hdrnet_amd::YuvPackedIo& io) {
  if (int rc = check_yuv_packed_pointers(what, "input", io.in, io.to_rgb)) return rc;
  if (io.out_kind >= HDRNET_CHROMA_OUT_SURFACE_U8) return check_yuv_packed_pointers(what, "output", io.out, io.from_rgb);
  if (!io.out.p || ((uintptr_t)io.out.p & (io.out_kind == HDRNET_CHROMA_OUT_RGB_F32 ? 15u : 3u)))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: null or misaligned out (float32 frames 16-B, uint8 frames 4-B aligned)", what);
  return HDRNET_OK;
}

// The two fused entry points (`what`): apply_io_yuv_impl's checks in its order.  `io`: the call's surfaces as given, io.out.p
// the RGB frame where the output is one.  A guide map AND a guide network is refused here (the entry points this mirrors let
// the map win): a caller who passes both has made a mistake one of them would hide.
int apply_io_yuv_packed_impl(const char* what, const float* grid, const IoGuide& g, hdrnet_amd::YuvPackedIo io, int sample_dtype,
                             int B, int H, int W, int GH, int GW, int GD, int Cin, int Cout, int has_offset, void* stream) {
  using namespace hdrnet_amd;
  char prefix[96];
  snprintf(prefix, sizeof prefix, "%s: ", what);
  if (int rc = check_common(B, H, W, GH, GW, GD)) return rc;
  if (int rc = g.curves ? check_curves_knots(prefix, g.n) : check_guide_flags(g.flags)) return rc;
  if (int rc = check_yuv_packed_io_values(what, io, sample_dtype, B, H, W, Cin, Cout, has_offset)) return rc;
  if ((long long)B * H * W == 0) return finish_noop();
  if (int rc = check_yuv_packed_io_pointers(what, io)) return rc;
  if (g.curves) {
    if (!grid || !g.conv1 || !g.shifts || !g.slopes || !g.conv2)
      return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer (grid or a curves parameter)", what);
  } else {
    if (!grid) return fail(HDRNET_INVALID_ARGUMENT, "%s: null buffer (grid)", what);
    if (g.guide && (g.conv1 || g.conv2))
      return fail(HDRNET_INVALID_ARGUMENT, "%s: either a guide map or the guide network must be given, not both", what);
    if (int rc = check_guide_given(prefix, g.guide, g.conv1, g.conv2, g.n)) return rc;
  }
  const bool surface_out = io.out_kind >= HDRNET_CHROMA_OUT_SURFACE_U8;
  ApplyIoArgs a{grid, g.guide, nullptr, nullptr, B, H, W, GH, GW, GD, Cin, Cout, true,
                sample_dtype, surface_out ? sample_dtype : io.out_kind == HDRNET_CHROMA_OUT_RGB_F32 ? 0 : 1, 1.0f, g.conv1,
                g.conv2, g.n, g.guide_out, g.shifts, g.slopes};
  if (int rc = set_io_guide(a, g, prefix, "npts <= 16")) return rc;
  if (surface_out) {
    io.out.order = io.in.order;  // a surface out has the input's byte order
    if (io.out_kind == HDRNET_CHROMA_OUT_SURFACE_U8) io.out_bits = 0;
  } else {  // an RGB frame out: a.out
    a.out = const_cast<void*>(io.out.p);
    io.out = YuvPackedSurface{};
    io.from_rgb = nullptr;
    io.out_bits = 0;
  }
  a.yuvk = &io;
  return launch_io(a, nullptr, 0, 0, g.curves ? "BilateralSliceApplyIOCurvesYuvPacked" : "BilateralSliceApplyIOYuvPacked",
                   "the packed 4:2:2 YUV forward supports Cin = Cout = 3 with offset, W % 4 == 0, aligned buffers", stream);
}

}  // namespace

int hdrnet_yuv_packed_to_rgb_f32(const void* surface, int sample_dtype, int pitch, long long image_stride, int order, int B,
                                 int H, int W, const float* to_rgb, float* rgb, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_yuv_packed_to_rgb_f32";
  const YuvPackedSurface in{surface, pitch, order, image_stride};
  if (int rc = check_yuv_extents(what, B, H, W, HDRNET_CHROMA_422)) return rc;
  if (int rc = check_yuv_packed_surface(what, "input", sample_dtype, in, B, H, W)) return rc;
  if ((long long)B * H * W == 0) return finish_noop();
  if (int rc = check_yuv_packed_pointers(what, "input", in, to_rgb)) return rc;
  if (!rgb || ((uintptr_t)rgb & 15u)) return fail(HDRNET_INVALID_ARGUMENT, "%s: rgb must be a 16-B aligned buffer", what);
  return finish_launch(launch_yuv_packed_to_rgb(in, sample_dtype, to_rgb, rgb, B, H, W, static_cast<hipStream_t>(stream)), what,
                       "yuv_packed_to_rgb");
}

int hdrnet_lowres_input_yuv_packed(const void* surface, int sample_dtype, int pitch, long long image_stride, int order, int B,
                                   int H, int W, const float* to_rgb, float* lowres, int net_input_size, void* stream) {
  using namespace hdrnet_amd;
  const char* what = "hdrnet_lowres_input_yuv_packed";
  const YuvPackedSurface in{surface, pitch, order, image_stride};
  if (int rc = check_yuv_extents(what, B, H, W, HDRNET_CHROMA_422)) return rc;
  if (int rc = check_yuv_packed_surface(what, "input", sample_dtype, in, B, H, W)) return rc;
  if (H <= 0 || W <= 0 || net_input_size <= 0 || (long long)net_input_size * net_input_size * 12 >= (1LL << 31))
    return fail(HDRNET_INVALID_ARGUMENT, "%s: non-positive extent (H=%d, W=%d, net_input_size=%d)", what, H, W, net_input_size);
  if (B == 0) return finish_noop();
  if (int rc = check_yuv_packed_pointers(what, "input", in, to_rgb)) return rc;
  if (!lowres || ((uintptr_t)lowres & 15u)) return fail(HDRNET_INVALID_ARGUMENT, "%s: lowres must be a 16-B aligned buffer", what);
  SamplePrepArgs a{surface, nullptr, sample_dtype, 0, 1.0f, 1.0f, B, H, W, nullptr, B, H, W, nullptr, nullptr, lowres,
                   net_input_size, false};
  a.yuv_packed = &in;
  a.yuv_to_rgb = to_rgb;
  a.yuv_chroma = HDRNET_CHROMA_422;
  return finish_launch(launch_sample_prep(a, static_cast<hipStream_t>(stream)), what, "sample_prep");
}

int hdrnet_bilateral_slice_apply_io_yuv_packed(const float* grid, const float* guide, const void* surface, int sample_dtype,
                                               int pitch, long long image_stride, int order, int B, int H, int W,
                                               const float* to_rgb, int GH, int GW, int GD, int Cin, int Cout,
                                               int has_offset, const float* guide_conv1, const float* guide_conv2,
                                               int n_feats, float* guide_out, unsigned flags, int output_kind, void* out,
                                               int out_pitch, long long out_image_stride, const float* from_rgb,
                                               int out_bits, void* stream) {
  const hdrnet_amd::YuvPackedIo io{{surface, pitch, order, image_stride}, to_rgb, output_kind,
                                   {out, out_pitch, order, out_image_stride}, from_rgb, out_bits};
  return apply_io_yuv_packed_impl("hdrnet_bilateral_slice_apply_io_yuv_packed", grid,
                                  io_guide_network(guide, guide_conv1, guide_conv2, n_feats, guide_out, flags), io, sample_dtype,
                                  B, H, W, GH, GW, GD, Cin, Cout, has_offset, stream);
}

int hdrnet_bilateral_slice_apply_io_curves_yuv_packed(const float* grid, const void* surface, int sample_dtype, int pitch,
                                                      long long image_stride, int order, int B, int H, int W,
                                                      const float* to_rgb, int GH, int GW, int GD, int Cin, int Cout,
                                                      int has_offset, const float* guide_ccm, const float* guide_shifts,
                                                      const float* guide_slopes, const float* guide_mix, int npts,
                                                      const void* prepared, float* guide_out, int output_kind, void* out,
                                                      int out_pitch, long long out_image_stride, const float* from_rgb,
                                                      int out_bits, void* stream) {
  const hdrnet_amd::YuvPackedIo io{{surface, pitch, order, image_stride}, to_rgb, output_kind,
                                   {out, out_pitch, order, out_image_stride}, from_rgb, out_bits};
  return apply_io_yuv_packed_impl("hdrnet_bilateral_slice_apply_io_curves_yuv_packed", grid,
                                  io_guide_curves(guide_ccm, guide_shifts, guide_slopes, guide_mix, npts, prepared, guide_out), io,
                                  sample_dtype, B, H, W, GH, GW, GD, Cin, Cout, has_offset, stream);
}

size_t hdrnet_bilateral_slice_apply_grad_workspace_bytes(int B, int H, int W, int GH, int GW,
                                                         int GD, int Cin, int Cout,
                                                         int has_offset) {
  if (B <= 0 || H <= 0 || W <= 0 || GH <= 0 || GW <= 0 || GD <= 0 || Cin < 0 || Cout <= 0) return 0;
  if (!hdrnet_amd::apply_fast_shape(Cin, Cout, has_offset != 0)) return 0;
  return hdrnet_amd::grid_grad_mfma_workspace(B, H, W, GH, GW, GD, Cout * (Cin + (has_offset ? 1 : 0)));
}

int hdrnet_bilateral_slice_apply_grad_f32_ex(const float* grid, const float* guide,
                                             const float* input, const float* dout,
                                             float* dgrid, float* dguide, float* dinput, int B,
                                             int H, int W, int GH, int GW, int GD, int Cin,
                                             int Cout, int has_offset, void* workspace,
                                             size_t workspace_bytes, unsigned flags,
                                             void* stream) {
  if (int rc = check_common(B, H, W, GH, GW, GD)) return rc;
  if (int rc = check_flags(flags)) return rc;
  if (Cin < 0 || Cout <= 0 || Cin + (has_offset ? 1 : 0) <= 0)
    return fail(HDRNET_INVALID_ARGUMENT, "bad channel counts (Cin=%d, Cout=%d)", Cin, Cout);
  const hdrnet_amd::ApplyGradArgs a{grid, guide, input, dout, dgrid, dguide, dinput, B, H, W, GH, GW, GD, Cin, Cout,
                                    Cin + (has_offset ? 1 : 0), has_offset != 0, workspace, workspace_bytes,
                                    variant(flags)};
  return grad_dispatch(a, family(flags), static_cast<hipStream_t>(stream));
}

int hdrnet_bilateral_slice_apply_grad_f32(const float* grid, const float* guide,
                                          const float* input, const float* dout, float* dgrid,
                                          float* dguide, float* dinput, int B, int H, int W,
                                          int GH, int GW, int GD, int Cin, int Cout,
                                          int has_offset, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  return hdrnet_bilateral_slice_apply_grad_f32_ex(grid, guide, input, dout, dgrid, dguide, dinput,
                                                  B, H, W, GH, GW, GD, Cin, Cout, has_offset,
                                                  workspace, workspace_bytes, HDRNET_KERNEL_AUTO,
                                                  stream);
}

int hdrnet_bilateral_slice_f32_ex(const float* grid, const float* guide, float* out, int B, int H,
                                  int W, int GH, int GW, int GD, int C, unsigned flags,
                                  void* stream) {
  using namespace hdrnet_amd;
  if (int rc = check_common(B, H, W, GH, GW, GD)) return rc;
  if (int rc = check_flags(flags)) return rc;
  if (C <= 0) return fail(HDRNET_INVALID_ARGUMENT, "grid_channels must be positive (C=%d)", C);
  if ((long long)B * H * W == 0) return finish_noop();
  if (!grid || !guide || !out) return fail(HDRNET_INVALID_ARGUMENT, "null buffer");
  SliceArgs a{grid, guide, out, B, H, W, GH, GW, GD, C};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool fast_ok = slice_fwd_rows_supported(a);
  if (family(flags) == HDRNET_KERNEL_FAST && !fast_ok)
    return fail(HDRNET_INVALID_ARGUMENT, "no fast BilateralSlice variant for this shape");
  if (family(flags) != HDRNET_KERNEL_GENERIC && fast_ok) {
    const char* name = "";
    const hipError_t e = launch_slice_fwd_rows(a, s, &name);
    return finish_launch(e, "BilateralSlice", name);
  }
  if ((long long)B * H * W > kGenericMaxPixels) return refuse_generic("BilateralSlice", (long long)B * H * W);
  return finish_launch(launch_slice_fwd_generic(a, s), "BilateralSlice", "slice_fwd_generic");
}

int hdrnet_bilateral_slice_f32(const float* grid, const float* guide, float* out, int B, int H,
                               int W, int GH, int GW, int GD, int C, void* stream) {
  return hdrnet_bilateral_slice_f32_ex(grid, guide, out, B, H, W, GH, GW, GD, C,
                                       HDRNET_KERNEL_AUTO, stream);
}

size_t hdrnet_bilateral_slice_grad_workspace_bytes(int B, int H, int W, int GH, int GW, int GD,
                                                   int C) {
  if (B <= 0 || H <= 0 || W <= 0 || GH <= 0 || GW <= 0 || GD <= 0 || C <= 0) return 0;
  if (!hdrnet_amd::slice_fast_channels(C)) return 0;
  return hdrnet_amd::grid_grad_mfma_workspace(B, H, W, GH, GW, GD, C);
}

int hdrnet_bilateral_slice_grad_f32_ex(const float* grid, const float* guide, const float* dout,
                                       float* dgrid, float* dguide, int B, int H, int W, int GH,
                                       int GW, int GD, int C, void* workspace,
                                       size_t workspace_bytes, unsigned flags, void* stream) {
  if (int rc = check_common(B, H, W, GH, GW, GD)) return rc;
  if (int rc = check_flags(flags)) return rc;
  if (C <= 0) return fail(HDRNET_INVALID_ARGUMENT, "grid_channels must be positive (C=%d)", C);
  // BilateralSlice is the apply op without an input: one "offset" column per channel
  hdrnet_amd::ApplyGradArgs a{grid, guide, nullptr, dout, dgrid, dguide, nullptr, B, H, W, GH, GW, GD, 0, C, 1, true,
                              workspace, workspace_bytes, variant(flags)};
  a.slice = true;
  return grad_dispatch(a, family(flags), static_cast<hipStream_t>(stream));
}

int hdrnet_bilateral_slice_grad_f32(const float* grid, const float* guide, const float* dout,
                                    float* dgrid, float* dguide, int B, int H, int W, int GH,
                                    int GW, int GD, int C, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  return hdrnet_bilateral_slice_grad_f32_ex(grid, guide, dout, dgrid, dguide, B, H, W, GH, GW, GD,
                                            C, workspace, workspace_bytes, HDRNET_KERNEL_AUTO,
                                            stream);
}

}  // extern "C"
