#!/usr/bin/env python3
"""Host-code hygiene of the loader and the scheduler: csrc/engine_load.cpp's read / validate / plan path and csrc/engine_schedule.cpp's
plan_schedule under AddressSanitizer + UBSan on the CPU.

    python tools/engine_plan_asan.py

Builds tools/engine_plan_asan.cpp + csrc/engine_load.cpp + csrc/engine_schedule.cpp with -fsanitize=address,undefined (host side only) into a stand-alone program in
vehicle-cv-adas_amd/_scratch/, linked against the product library for the kernels' predicates; writes the tables of three shipped graphs
(four precisions each) and every damaged table of tests/test_engine_plan_cpu.py to files; runs the program on them.  No device is used, and
nothing is loaded into python under a sanitizer.  The product library must be built (vehicle-cv-adas_amd/build.py)."""
import importlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vehicle-cv-adas_amd")
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)


def main():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = os.path.join(PKG, "_scratch", "engine_plan_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-omit-frame-pointer"]
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", *san,
                           os.path.join(ROOT, "tools", "engine_plan_asan.cpp"), os.path.join(PKG, "csrc", "engine_load.cpp"),
                           os.path.join(PKG, "csrc", "engine_schedule.cpp"),
                           "-L" + PKG, "-ladas_hip", "-Wl,-rpath," + PKG, "-o", exe])
    import test_engine_plan_cpu as T
    with tempfile.TemporaryDirectory() as tmp:
        T.write_refusal_cases(tmp)
        for name in ("yolov8n", "ufldv2_res18", "efficientdet-d0"):
            tables = T.M.build(name, wsrc=T.Z).tables()
            for prec in range(4):
                with open(os.path.join(tmp, f"{name}.{prec}.tables"), "wb") as f:
                    f.write(tables)
        files = sorted(os.path.join(tmp, f) for f in os.listdir(tmp))
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        return subprocess.call([exe, *files], env=env)


if __name__ == "__main__":
    sys.exit(main())
