"""ctypes wrapper over tests/_build/libemu_jpegdec.so (host build of csrc/jpegdec_core.h, tests/hostemu/emu_jpegdec.cpp).
Test scaffolding: lets the CPU suite run the device kernels' functions of rules D1-D9, stage by stage, and compare them with
tests/jpegdec_ref.py and with libjpeg; the GPU suite compares the device's frames with these.  Builds itself on first use."""
import ctypes as C, os, subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "emu_jpegdec.cpp")
FUZZ_SRC = os.path.join(ROOT, "tests", "hostemu", "jpegdec_fuzz_main.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libemu_jpegdec.so")
FUZZ_OUT = os.path.join(ROOT, "tests", "_build", "jpegdec_fuzz")
INC = os.path.join(ROOT, "vehicle-cv-adas_amd", "csrc")
UNSUPPORTED, FORMAT, SIZE, CORRUPT = 1, 2, 4, 8
REJECT = UNSUPPORTED | FORMAT | SIZE


def _fresh(out, deps):
    return os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)


def build():
    deps = [SRC, os.path.join(INC, "jpegdec_core.h"), os.path.join(INC, "jpeg_core.h")]
    if _fresh(OUT, deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", INC, SRC, "-o", OUT])
    return OUT


def build_fuzz():
    """The stand-alone mutation program (tests/hostemu/jpegdec_fuzz_main.cpp), plain g++ -O1."""
    deps = [FUZZ_SRC, os.path.join(INC, "jpegdec_core.h"), os.path.join(INC, "jpeg_core.h")]
    if _fresh(FUZZ_OUT, deps):
        return FUZZ_OUT
    os.makedirs(os.path.dirname(FUZZ_OUT), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", INC, FUZZ_SRC, "-o", FUZZ_OUT])
    return FUZZ_OUT


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_jpegdec_idct_err.restype = C.c_double
        _lib.emu_jpegdec_idct_err.argtypes = [C.c_double]
        _lib.emu_jpegdec_idct_err_2048.restype = C.c_double
        _lib.emu_jpegdec_cap_blocks.restype = C.c_longlong
        _lib.emu_jpegdec_cap_blocks.argtypes = [C.c_int, C.c_int]
        _lib.emu_jpegdec_cap_segments.restype = C.c_longlong
        _lib.emu_jpegdec_cap_segments.argtypes = [C.c_int, C.c_int]
        _lib.emu_jpegdec_idct.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.emu_jpegdec_decode.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_int, C.c_int] + [C.c_void_p] * 4
        _lib.emu_jpegdec_colour.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def idct_err(norm):
    """D6's bound on |p - f| for a block of Euclidean norm `norm`."""
    return float(lib().emu_jpegdec_idct_err(float(norm)))


def idct_err_2048():
    return float(lib().emu_jpegdec_idct_err_2048())


def cap_blocks(w, h):
    return int(lib().emu_jpegdec_cap_blocks(int(w), int(h)))


def idct(blocks):
    """[n][64] coefficients, natural order -> (acc [n][64] int32 with p = acc / 2^17, px [n][64] u8)."""
    F = np.ascontiguousarray(blocks, np.int16).reshape(-1, 64)
    acc, px = np.zeros(F.shape, np.int32), np.zeros(F.shape, np.uint8)
    lib().emu_jpegdec_idct(_p(F), len(F), _p(acc), _p(px))
    return acc, px


class Decoded:
    """flags; geometry; per component c the coefficients coef[c] [bh][bw][64] (natural order) and the plane planes[c] [bh * 8][bw * 8];
    bgr [h][w][3]."""


def decode(stream, w, h, capacity=None, length=None, stages=True):
    """One stream (bytes) through the host build.  length: what the decoder is told (default: all of it)."""
    raw = np.frombuffer(bytes(stream) + b"", np.uint8).copy() if len(stream) else np.zeros(1, np.uint8)
    n = len(stream) if length is None else int(length)
    cap = int(capacity) if capacity else max(len(stream), 1)
    cb = cap_blocks(w, h)
    info = np.zeros(8, np.int32)
    coef, planes = np.zeros((cb, 64), np.int16), np.zeros(cb * 64, np.uint8)
    bgr = np.zeros((h, w, 3), np.uint8)
    d = Decoded()
    d.flags = int(lib().emu_jpegdec_decode(_p(raw), n, cap, int(w), int(h), _p(info), _p(coef), _p(planes), _p(bgr)))
    assert d.flags >= 0, d.flags
    d.ncomp, d.hs, d.vs, d.dri, d.mcux, d.mcuy, d.nseg, d.found = (int(v) for v in info)
    d.bgr, d.raw_planes = bgr, planes
    d.coef, d.planes = [], []
    if stages and not d.flags & REJECT:
        off = 0
        for c in range(d.ncomp):
            bw, bh = d.mcux * (d.hs if c == 0 else 1), d.mcuy * (d.vs if c == 0 else 1)
            d.coef.append(coef[off:off + bw * bh].reshape(bh, bw, 64).astype(np.int64))
            d.planes.append(planes[off * 64:(off + bw * bh) * 64].reshape(bh * 8, bw * 8))
            off += bw * bh
    return d


def decode_batch(streams, w, h, capacity=None, lengths=None):
    """(bgr [n][h][w][3], flags [n]) of a batch: what the device's run must give."""
    out = [decode(s, w, h, capacity, None if lengths is None else lengths[i], stages=False) for i, s in enumerate(streams)]
    return np.stack([d.bgr for d in out]), np.array([d.flags for d in out], np.int32)


def colour(raw_planes, w, h, ncomp, hs, vs):
    pl = np.ascontiguousarray(raw_planes, np.uint8)
    bgr = np.zeros((h, w, 3), np.uint8)
    lib().emu_jpegdec_colour(_p(pl), int(w), int(h), int(ncomp), int(hs), int(vs), _p(bgr))
    return bgr
