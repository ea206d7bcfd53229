"""ctypes wrapper over tests/_build/libemu_warp.so (host build of csrc/warp_core.h, tests/hostemu/emu_warp.cpp).
Test scaffolding: lets the CPU suite run the device kernel's per-pixel text and compare it with tests/warp_ref.py."""
import ctypes as C, os, subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "emu_warp.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libemu_warp.so")
INC = os.path.join(ROOT, "vehicle-cv-adas_amd", "csrc")


def build():
    deps = [SRC, os.path.join(INC, "warp_core.h")]
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-ffp-contract=off", "-fPIC", "-shared", "-I", INC, SRC, "-o", OUT])
    return OUT


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def warp_perspective(img, M, dst_wh, inverse=False):
    """img (H, W, 3) uint8, dst_wh = (width, height) -> (height, width, 3) uint8; None for a singular matrix."""
    img = np.ascontiguousarray(img, np.uint8)
    m = np.ascontiguousarray(M, np.float64).reshape(9)
    dw, dh = int(dst_wh[0]), int(dst_wh[1])
    out = np.zeros((dh, dw, 3), np.uint8)
    rc = lib().emu_warp_perspective(_p(img), img.shape[0], img.shape[1], _p(out), dh, dw, _p(m), 1 if inverse else 0)
    return out if rc == 0 else None


def invert3x3(M):
    m = np.ascontiguousarray(M, np.float64).reshape(9)
    out = np.zeros(9, np.float64)
    return out if lib().emu_warp_invert(_p(m), _p(out)) == 0 else None


def block_width(dh, dw):
    return int(lib().emu_warp_block_width(int(dh), int(dw)))
