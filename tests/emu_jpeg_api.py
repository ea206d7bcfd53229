"""ctypes wrapper over tests/_build/libemu_jpeg.so (host build of csrc/jpeg_core.h, tests/hostemu/emu_jpeg.cpp).
Test scaffolding: lets the CPU suite run the device kernels' block functions of rules J1-J9 and a whole stream composed from them and compare
them with tests/jpeg_ref.py; the GPU suite compares the device's streams with these.  Builds itself on first use."""
import ctypes as C, os, subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "emu_jpeg.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libemu_jpeg.so")
INC = os.path.join(ROOT, "vehicle-cv-adas_amd", "csrc")
OVERFLOW = 1


def build():
    deps = [SRC, os.path.join(INC, "jpeg_core.h")]
    if os.path.exists(OUT) and all(os.path.getmtime(OUT) >= os.path.getmtime(d) for d in deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", INC, SRC, "-o", OUT])
    return OUT


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_jpeg_fdct_err.restype = C.c_double
        _lib.emu_jpeg_bound.restype = C.c_longlong
        _lib.emu_jpeg_bound.argtypes = [C.c_int, C.c_int]
        _lib.emu_jpeg_tables.argtypes = [C.c_int, C.c_void_p]
        _lib.emu_jpeg_header.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.emu_jpeg_fdct.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _lib.emu_jpeg_quantise.argtypes = [C.c_void_p] * 4 + [C.c_int]
        _lib.emu_jpeg_load_block.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
        _lib.emu_jpeg_levels.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _lib.emu_jpeg_encode.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_longlong, C.c_int] + [C.c_void_p] * 3
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def header_bytes():
    return int(lib().emu_jpeg_header_bytes())


def zigzag():
    """(zigzag position -> natural index, natural index -> zigzag position), as the header tabulates them."""
    return [int(lib().emu_jpeg_zigzag(k)) for k in range(64)], [int(lib().emu_jpeg_zigzag_position(n)) for n in range(64)]


def fdct_err():
    return float(lib().emu_jpeg_fdct_err())


def bound(w, h):
    return int(lib().emu_jpeg_bound(int(w), int(h)))


def tables(quality):
    """The J5 divisors, [2][64] in zigzag order."""
    q = np.zeros((2, 64), np.uint16)
    lib().emu_jpeg_tables(int(quality), _p(q))
    return q


def header(w, h, quality):
    out = np.zeros(header_bytes() + 64, np.uint8)
    n = lib().emu_jpeg_header(int(w), int(h), int(quality), _p(out))
    return out[:n].tobytes()


def fdct(blocks):
    """[n][64] level-shifted samples -> F' [n][64], natural order."""
    f = np.ascontiguousarray(blocks, np.int32).reshape(-1, 64)
    F = np.zeros_like(f)
    lib().emu_jpeg_fdct(_p(f), _p(F), len(f))
    return F


def quantise(F, d, ac):
    F, d, ac = (np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32), np.shape(F)).reshape(-1)) for v in (F, d, ac))
    out = np.zeros_like(F)
    lib().emu_jpeg_quantise(_p(F), _p(d), _p(ac), _p(out), len(F))
    return out


def load_block(frame, my, mx, k6):
    fr = np.ascontiguousarray(frame, np.uint8)
    f = np.zeros(64, np.int32)
    lib().emu_jpeg_load_block(_p(fr), fr.shape[1], fr.shape[0], int(my), int(mx), int(k6), _p(f))
    return f


def levels(frame, quality):
    """[mcu_h][seg_blocks][64] int16, zigzag order."""
    fr = np.ascontiguousarray(frame, np.uint8)
    h, w = fr.shape[:2]
    out = np.zeros(((h + 15) // 16, 6 * ((w + 15) // 16), 64), np.int16)
    lib().emu_jpeg_levels(_p(fr), w, h, int(quality), _p(out))
    return out


def encode_raw(frames, quality, capacity=None, fill=0, rounds=0):
    """frames [n][h][w][3] -> (out [n][capacity] pre-filled with `fill`, lengths [n], flags [n]).  rounds=0: one bit writer per segment;
    rounds=k: the entropy kernel's composition, k blocks at a time (256 on the device)."""
    fr = np.ascontiguousarray(frames, np.uint8)
    n, h, w = fr.shape[:3]
    cap = int(capacity) if capacity else w * h * 3
    out = np.full((n, cap), fill, np.uint8)
    lengths, flags = np.zeros(n, np.int64), np.zeros(n, np.int32)
    r = lib().emu_jpeg_encode(_p(fr), n, w, h, int(quality), cap, int(rounds), _p(out), _p(lengths), _p(flags))
    assert r == 0, ("emu_jpeg_encode", r)
    return out, lengths, flags


def encode(frame, quality):
    """One frame -> its stream as bytes (capacity: the bound)."""
    fr = np.ascontiguousarray(frame, np.uint8)
    out, n, fl = encode_raw(fr[None], quality, bound(fr.shape[1], fr.shape[0]))
    assert fl[0] == 0
    return out[0, :n[0]].tobytes()
