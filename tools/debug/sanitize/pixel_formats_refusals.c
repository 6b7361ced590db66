/* The refusals of include/hdrnet_amd_pixel_formats.h as a stand-alone host program, for a sanitizer build of the
 * library's HOST code (tools/sanitize_pixel_formats.py compiles every source with -Xarch_host
 * -fsanitize=address,undefined and links this file's main against them).  Every call below is refused, or is a no-op,
 * before any HIP call: no GPU is needed and none is touched.  Exit status 0: every call returned what is written here. */
#include <stdio.h>
#include <string.h>

#include "hdrnet_amd_pixel_formats.h"

static int failures = 0;

static void expect(const char* what, int rc, int want_rc, const char* want_text) {
  const char* err = hdrnet_last_error();
  if (rc != want_rc || (want_text && !strstr(err, want_text))) {
    printf("FAIL %s: rc = %d (want %d), text \"%s\" (want \"%s\")\n", what, rc, want_rc, err, want_text ? want_text : "");
    ++failures;
  } else {
    printf("ok   %s: rc = %d%s%s\n", what, rc, rc ? ", " : "", rc ? err : "");
  }
}

#define A ((void*)0x1000) /* 16-byte aligned, never dereferenced */
#define OFF(p, n) ((void*)((char*)(p) + (n)))

static int io(const void* in, void* out, int B, int W, int Cin, int idt, float wl, int odt, int ifmt, int ofmt) {
  return hdrnet_bilateral_slice_apply_io_px((const float*)A, (const float*)A, in, out, B, 4, W, 2, 2, 2, Cin, Cin, 1, idt, wl,
                                            odt, NULL, NULL, 0, NULL, 0u, ifmt, ofmt, NULL);
}

static int curves(const void* in, void* out, int B, int W, int idt, float wl, int odt, int ifmt, int ofmt, const void* prep) {
  return hdrnet_bilateral_slice_apply_io_curves_px((const float*)A, in, out, B, 4, W, 2, 2, 2, 3, 3, 1, idt, wl, odt,
                                                   (const float*)A, (const float*)A, (const float*)A, (const float*)A, 16,
                                                   prep, NULL, ifmt, ofmt, NULL);
}

int main(void) {
  hdrnet_enable_kernel_names(1);
  expect("io: unknown format code", io(A, A, 1, 8, 3, 1, 255.f, 1, 4, 4), 1, "unknown pixel format code");
  expect("io: negative format code", io(A, A, 1, 8, 3, 1, 255.f, 1, -1, -1), 1, "unknown pixel format code");
  expect("io: float32 with bgr", io(A, A, 1, 8, 3, 0, 1.f, 1, HDRNET_PX_BGR, HDRNET_PX_BGR), 1, "float32 frames take HDRNET_PX_RGB only");
  expect("io: u8 out in another format", io(A, A, 1, 8, 3, 1, 255.f, 1, HDRNET_PX_BGRA, HDRNET_PX_RGBA), 1,
         "a uint8 output has the input's pixel format");
  expect("io: float32 out not rgb", io(A, A, 1, 8, 3, 1, 255.f, 0, HDRNET_PX_BGRA, HDRNET_PX_BGRA), 1,
         "a float32 output is [B][H][W][3] in RGB order");
  expect("io: 4-channel input at 4 mod 16", io(OFF(A, 4), A, 1, 8, 3, 1, 255.f, 1, HDRNET_PX_BGRA, HDRNET_PX_BGRA), 1,
         "must be 16-B aligned");
  expect("io: 4-channel output at 8 mod 16", io(A, OFF(A, 8), 1, 8, 3, 2, 65535.f, 1, HDRNET_PX_RGBA, HDRNET_PX_RGBA), 1,
         "must be 16-B aligned");
  expect("io: 3-channel input at 2 mod 4", io(OFF(A, 2), A, 1, 8, 3, 1, 255.f, 1, HDRNET_PX_BGR, HDRNET_PX_BGR), 1,
         "must be 4-B aligned");
  expect("io: W % 4", io(A, A, 1, 6, 3, 1, 255.f, 1, HDRNET_PX_BGRA, HDRNET_PX_BGRA), 1, "W % 4 != 0");
  expect("io: four op channels", io(A, A, 1, 8, 4, 1, 255.f, 1, HDRNET_PX_BGRA, HDRNET_PX_BGRA), 1, "Cin = Cout = 3 with offset");
  expect("io: null input", io(NULL, A, 1, 8, 3, 1, 255.f, 1, HDRNET_PX_BGR, HDRNET_PX_BGR), 1, "null buffer");
  expect("io: B == 0", io(NULL, NULL, 0, 8, 3, 1, 255.f, 1, HDRNET_PX_BGRA, HDRNET_PX_BGRA), 0, NULL);
  expect("io: rgb, W % 4 (the existing entry point's text)", io(A, A, 1, 6, 3, 1, 255.f, 1, 0, 0), 1, "the wire-format forward supports");
  /* launch geometry on the host (apply_fwd_io_supported -> io_fwd_geom -> make_row_plan): a segment's window of a
   * 1024-column grid does not fit LDS */
  expect("io: geometry refuses a 1024-column grid window",
         hdrnet_bilateral_slice_apply_io_px((const float*)A, (const float*)A, A, A, 1, 4, 1024, 2, 1024, 8, 3, 3, 1, 1, 255.f,
                                            1, NULL, NULL, 0, NULL, 0u, HDRNET_PX_BGRA, HDRNET_PX_BGRA, NULL),
         1, "the wire-format forward supports");

  expect("curves: unknown format code", curves(A, A, 1, 8, 1, 255.f, 1, 9, 9, NULL), 1, "unknown pixel format code");
  expect("curves: float32 with rgba", curves(A, A, 1, 8, 0, 1.f, 0, HDRNET_PX_RGBA, HDRNET_PX_RGB, NULL), 1,
         "float32 frames take HDRNET_PX_RGB only");
  expect("curves: u8 out in another format", curves(A, A, 1, 8, 1, 255.f, 1, HDRNET_PX_BGR, HDRNET_PX_RGB, NULL), 1,
         "a uint8 output has the input's pixel format");
  expect("curves: float32 out not rgb", curves(A, A, 1, 8, 2, 32767.f, 0, HDRNET_PX_BGR, HDRNET_PX_BGR, NULL), 1,
         "a float32 output is [B][H][W][3] in RGB order");
  expect("curves: 4-channel input at 4 mod 16", curves(OFF(A, 4), A, 1, 8, 1, 255.f, 1, HDRNET_PX_BGRA, HDRNET_PX_BGRA, A), 1,
         "must be 16-B aligned");
  expect("curves: W % 4", curves(A, A, 1, 6, 1, 255.f, 1, HDRNET_PX_BGR, HDRNET_PX_BGR, NULL), 1, "W % 4 != 0");
  expect("curves: misaligned prepared tables", curves(A, A, 1, 8, 1, 255.f, 1, HDRNET_PX_BGRA, HDRNET_PX_BGRA, OFF(A, 4)), 1,
         "prepared curves tables need");
  expect("curves: B == 0", curves(NULL, NULL, 0, 8, 1, 255.f, 1, HDRNET_PX_BGRA, HDRNET_PX_BGRA, NULL), 0, NULL);

  expect("lowres: unknown format code", hdrnet_lowres_input_px(A, 1, 255.f, 1, 8, 8, (float*)A, 4, 7, NULL), 1,
         "unknown pixel format code");
  expect("lowres: float32 with bgra", hdrnet_lowres_input_px(A, 0, 1.f, 1, 8, 8, (float*)A, 4, HDRNET_PX_BGRA, NULL), 1,
         "float32 frames take HDRNET_PX_RGB only");
  expect("lowres: 4-channel frames at 4 mod 16", hdrnet_lowres_input_px(OFF(A, 4), 1, 255.f, 1, 8, 8, (float*)A, 4, HDRNET_PX_RGBA, NULL),
         1, "must be 16-B aligned");
  expect("lowres: null output", hdrnet_lowres_input_px(A, 2, 65535.f, 1, 8, 8, NULL, 4, HDRNET_PX_BGR, NULL), 1, "null buffer");
  expect("lowres: n == 0", hdrnet_lowres_input_px(A, 1, 255.f, 1, 8, 8, (float*)A, 0, HDRNET_PX_BGR, NULL), 1, "non-positive extent");
  expect("lowres: B == 0", hdrnet_lowres_input_px(NULL, 1, 255.f, 0, 8, 8, NULL, 4, HDRNET_PX_BGRA, NULL), 0, NULL);
  printf("%d failure(s)\n", failures);
  return failures != 0;
}
