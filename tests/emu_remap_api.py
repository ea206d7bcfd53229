"""ctypes wrapper over tests/_build/libemu_remap.so (host build of csrc/remap_core.h, tests/hostemu/emu_remap.cpp).
Test scaffolding: lets the CPU suite walk both device kernels' work items of rules U1-U6 with every map load and every store audited, and
compare the results with tests/remap_ref.py; the GPU suite compares the device's maps and frames with these.  Builds itself on first use."""
import ctypes as C, os, subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "emu_remap.cpp")
MAIN = os.path.join(ROOT, "tests", "hostemu", "remap_bounds_main.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libemu_remap.so")
INC = os.path.join(ROOT, "vehicle-cv-adas_amd", "csrc")
PUB = os.path.join(ROOT, "include")
WHY = {0: None, 1: "non-finite parameter", 2: "zero focal length", 3: "singular new_K * R", 4: "size outside 1..4320 rows x 1..16384 columns",
       5: "map index outside the handle's table"}
SENTINEL = 0xA5
PARAM_FIELDS = ("src_h", "src_w", "dst_h", "dst_w", "n_streams", "n_maps")
CAMERA_FIELDS = ("K", "D", "new_K", "R")


class Params(C.Structure):          # adas_remap_params as this file believes it to be (test_remap_cpu.py compares it with the header's and _lib's)
    _fields_ = [(f, C.c_int) for f in PARAM_FIELDS]


class Camera(C.Structure):          # RemapCamera
    _fields_ = [("K", C.c_double * 4), ("D", C.c_double * 8), ("new_K", C.c_double * 4), ("R", C.c_double * 9)]


def _fresh(out, deps):
    return os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(d) for d in deps)


def build():
    deps = [SRC] + [os.path.join(INC, h) for h in ("remap_core.h", "warp_core.h")] + [os.path.join(PUB, "adas_hip.h")]
    if _fresh(OUT, deps):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-I", INC, "-I", PUB, SRC, "-o", OUT])
    return OUT


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
        _lib.emu_remap_why.restype = C.c_char_p
        _lib.emu_remap_map_stride.restype = C.c_longlong
        _lib.emu_remap_check_camera.argtypes = [C.POINTER(Camera)]
        _lib.emu_remap_build.argtypes = [C.POINTER(Camera), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.emu_remap_run.argtypes = [C.c_int] * 6 + [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                       C.c_int, C.c_void_p]
    return _lib


def layout():
    """(sizeof adas_remap_params, {field: offset}), (sizeof RemapCamera, {field: offset}) as g++ lays the headers out"""
    v = (C.c_int * 12)()
    lib().emu_remap_layout(v)
    return (int(v[0]), dict(zip(PARAM_FIELDS, (int(x) for x in v[1:7])))), (int(v[7]), dict(zip(CAMERA_FIELDS, (int(x) for x in v[8:12]))))


def camera(K, D=(), new_K=None, R=None):
    c = Camera()
    D = list(D) + [0.0] * (8 - len(D))
    for name, vals in (("K", K), ("D", D), ("new_K", K if new_K is None else new_K), ("R", np.eye(3).reshape(9) if R is None else np.reshape(R, 9))):
        for i, v in enumerate(vals):
            getattr(c, name)[i] = float(v)
    return c


def why(code):
    """The header's name of a refusal"""
    return lib().emu_remap_why(int(code)).decode()


def check_camera(K, D=(), new_K=None, R=None):
    """None, or the refusal by name"""
    return WHY[int(lib().emu_remap_check_camera(C.byref(camera(K, D, new_K, R))))]


def check_sizes(src_hw, dst_hw):
    return WHY[int(lib().emu_remap_check_sizes(int(src_hw[0]), int(src_hw[1]), int(dst_hw[0]), int(dst_hw[1])))]


def check_map(m, n_maps):
    return WHY[int(lib().emu_remap_check_map(int(m), int(n_maps)))]


def map_stride(dst_hw):
    return int(lib().emu_remap_map_stride(int(dst_hw[0]), int(dst_hw[1])))


def default_stream_map(n_streams, n_maps):
    return [int(lib().emu_remap_default_map(s, int(n_maps))) for s in range(n_streams)]


def build_map(K, D=(), new_K=None, R=None, dst_hw=None, map=0, n_maps=1):
    """The build kernel's work items over map `map` of tables of n_maps maps, audited -> xy (h, w, 2) int16, frac (h, w) uint16.  Everything
    around the map's own entries in the tables must keep its sentinel."""
    h, w = int(dst_hw[0]), int(dst_hw[1])
    stride, n = map_stride((h, w)), h * w
    xy = np.full((n_maps * stride, 2), 0x5A5A, np.int16)
    frac = np.full(n_maps * stride, 0xA5A5, np.uint16)
    info = np.zeros(4, np.int64)
    rc = lib().emu_remap_build(C.byref(camera(K, D, new_K, R)), h, w, int(map), int(n_maps), xy.ctypes.data, frac.ctypes.data, info.ctypes.data)
    assert rc == 0, WHY[rc]
    outside, misaligned, stores, not_once = (int(v) for v in info)
    assert (outside, misaligned, not_once) == (0, 0, 0) and stores == 2 * n, info
    lo = map * stride
    keep = np.ones(n_maps * stride, bool)
    keep[lo:lo + n] = False
    assert (xy[keep] == 0x5A5A).all() and (frac[keep] == 0xA5A5).all()
    return xy[lo:lo + n].reshape(h, w, 2).copy(), frac[lo:lo + n].reshape(h, w).copy()


def aligned(n, offset=0, fill=0, guard=0):
    """(whole, view): a uint8 view of n bytes whose address is `offset` mod 64, with `guard` bytes of `fill` on either side inside whole."""
    whole = np.full(n + 2 * guard + 128, fill, np.uint8)
    a = (-(whole.ctypes.data + guard) + offset) % 64
    return whole, whole[guard + a:guard + a + n]


def tables(maps, dst_hw):
    """The handle's two tables from a list of (xy, frac): map m at entry m * map_stride, the padding zero."""
    stride, n = map_stride(dst_hw), int(dst_hw[0]) * int(dst_hw[1])
    xy = np.zeros((len(maps) * stride, 2), np.int16)
    frac = np.zeros(len(maps) * stride, np.uint16)
    for m, (a, b) in enumerate(maps):
        xy[m * stride:m * stride + n] = np.asarray(a, np.int16).reshape(n, 2)
        frac[m * stride:m * stride + n] = np.asarray(b, np.uint16).reshape(n)
    return xy, frac


class Run:
    """out: uint8 [batch][dst_h][dst_w][3], pre-filled with SENTINEL; outside, misaligned, loads, stores, wide_loads, wide_stores, not_once:
    the audit's counts; staged: the run took the staged form, with staged_loads 16-byte source loads and direct_tiles workgroups whose box
    did not fit; guard_ok"""


def run(frames, maps, stream_map=None, n_streams=None, dst_offset=0, guard=64, path=-1, src_offset=0):
    """frames [batch][src_h][src_w][3] through the remap kernel's work items.  maps: a list of (xy, frac); stream_map: the map of every stream
    (None: the default table).  path: -1 the form remap_tile_ok chooses for the source (placed src_offset bytes off a multiple of 64: the
    staged form needs src_w * 3 and the pointer to be multiples of 16), 0 the direct form.  The destination is placed dst_offset bytes off a multiple of 64 and handed over with its exact size; it is
    pre-filled with SENTINEL and the guard bytes around it are checked."""
    frames = np.ascontiguousarray(frames, np.uint8)
    batch, sh, sw, _ = frames.shape
    _, src = aligned(frames.size, src_offset)
    src[:] = frames.ravel()
    dh, dw = maps[0][1].shape
    n_streams = batch if n_streams is None else int(n_streams)
    table = np.asarray(default_stream_map(n_streams, len(maps)) if stream_map is None else stream_map, np.int32)
    assert table.shape == (n_streams,)
    xy, frac = tables(maps, (dh, dw))
    nd = batch * dh * dw * 3
    whole, dst = aligned(nd, dst_offset, fill=SENTINEL, guard=guard)
    info = np.zeros(8, np.int64)
    rc = lib().emu_remap_run(sh, sw, dh, dw, n_streams, len(maps), src.ctypes.data, src.size, dst.ctypes.data, nd, xy.ctypes.data, frac.ctypes.data,
                             table.ctypes.data, batch, int(path), info.ctypes.data)
    assert rc == 0, WHY[rc]
    r = Run()
    r.outside, r.misaligned, r.loads, r.stores, r.wide_loads, r.wide_stores, r.not_once = (int(v) for v in info[:7])
    form = int(info[7])
    r.staged, r.staged_loads, r.direct_tiles = form > 0, max(form - 1, 0) % 1000000, form // 1000000
    r.out = dst.copy().reshape(batch, dh, dw, 3)
    lo = dst.ctypes.data - whole.ctypes.data
    r.guard_ok = bool((whole[:lo] == SENTINEL).all() and (whole[lo + nd:] == SENTINEL).all())
    return r


def remap(frames, maps, stream_map=None, n_streams=None):
    """What the device's run must write: uint8 [batch][dst_h][dst_w][3]."""
    r = run(frames, maps, stream_map, n_streams)
    assert (r.outside, r.misaligned, r.not_once) == (0, 0, 0) and r.guard_ok
    return r.out
