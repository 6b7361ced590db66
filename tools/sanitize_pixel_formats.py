#!/usr/bin/env python3
"""Host-side sanitizer run of the pixel-format entry points (include/hdrnet_amd_pixel_formats.h).

    python tools/sanitize_pixel_formats.py [--keep DIR]

Compiles every source of the library with the HOST side under AddressSanitizer + UndefinedBehaviorSanitizer
(``-Xarch_host -fsanitize=address,undefined``; the device code is built as always), links
tools/debug/sanitize/pixel_formats_refusals.c -- a program with its own main that calls the refusal and no-op cases --
against the objects and runs it.  Validation and launch geometry are host code and return before any HIP call, so the
program needs no GPU and touches none.  Nothing is loaded into python.
"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hdrnet_amd import build as hb  # noqa: E402

SAN = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-g"]


def main():
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    with tempfile.TemporaryDirectory() as tmp:
        out = keep or tmp
        os.makedirs(out, exist_ok=True)
        cc = hb.hipcc()
        procs, objs = [], []
        for src, extra in hb.SOURCES:
            obj = os.path.join(out, src.replace(".hip", ".o"))
            cmd = [cc, *hb.COMMON, *hb._usable_flags(cc, extra), *SAN, "-I", hb.CSRC, "-I", hb.INCLUDE, "-c",
                   os.path.join(hb.CSRC, src), "-o", obj]
            procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
            objs.append(obj)
        for cmd, p in procs:
            text, _ = p.communicate()
            if p.returncode:
                sys.exit("command failed: %s\n%s" % (" ".join(cmd), text))
        main_obj = os.path.join(out, "pixel_formats_refusals.o")
        exe = os.path.join(out, "pixel_formats_refusals")
        for cmd in ([cc, "-x", "c", "-O1", "-g", "-fsanitize=address,undefined", "-I", hb.INCLUDE, "-c",
                     os.path.join(ROOT, "tools", "debug", "sanitize", "pixel_formats_refusals.c"), "-o", main_obj],
                    [cc, f"--offload-arch={hb.ARCH}", "-fsanitize=address,undefined", "-o", exe, main_obj, *objs]):
            res = subprocess.run(cmd, capture_output=True, text=True)
            if res.returncode:
                sys.exit("command failed: %s\n%s%s" % (" ".join(cmd), res.stdout, res.stderr))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        res = subprocess.run([exe], env=env, capture_output=True, text=True)
        print(res.stdout + res.stderr, end="")
        sys.exit(res.returncode)


if __name__ == "__main__":
    main()
