"""ctypes wrapper over tests/_build/libemu_overlay_text.so (host build of csrc/overlay_text_core.h, tests/hostemu/emu_overlay_text.cpp).
Test scaffolding: lets the CPU suite run the device kernels' formatter, layout and per-piece fold of rules T1-T7 and compare them with
tests/text_ref.py.  Builds itself on first use."""
import ctypes as C, os, subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostemu", "emu_overlay_text.cpp")
OUT = os.path.join(ROOT, "tests", "_build", "libemu_overlay_text.so")
INC = os.path.join(ROOT, "vehicle-cv-adas_amd", "csrc")
FONTS = 16
_P = C.c_void_p


class Font(C.Structure):   # TextFont
    _fields_ = [("atlas", _P), ("atlas_w", C.c_int32), ("cell_h", C.c_int32), ("baseline_row", C.c_int32), ("size_h", C.c_int32), ("size_w_extra", C.c_int32),
                ("set", C.c_int32), ("scale", C.c_double), ("glyph_x", C.c_int32 * 95), ("glyph_w", C.c_int32 * 95), ("bearing_x", C.c_int32 * 95),
                ("advance", C.c_int32 * 95)]


class Item(C.Structure):   # TextItem
    _fields_ = [("kind", C.c_int32), ("source", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32), ("bx0", C.c_int32),
                ("by0", C.c_int32), ("bx1", C.c_int32), ("by1", C.c_int32), ("slot", C.c_int32), ("color", C.c_uint8 * 3), ("len", C.c_uint8),
                ("text", C.c_char * 48)]


class Line(C.Structure):   # TextLine
    _fields_ = [("x", C.c_int32), ("y", C.c_int32), ("slot", C.c_int32), ("color", C.c_uint8 * 3), ("len", C.c_uint8), ("text", C.c_char * 48)]


_INTS = ("max_text_items det_size_slot det_label_slot det_label_dx det_label_dy det_box_pad track_slot track_dy id_first id_count id_shadow_first "
         "id_shadow_count dist_size_first dist_size_count dist_first dist_count dist_shadow_first dist_shadow_count shadow_dx shadow_dy ldws_slot lkas_slot "
         "fcws_slot ldws_x ldws_y lkas_x lkas_y fcws_dx fcws_y id_shadow_sub").split()


class Style(C.Structure):  # TextStyle
    _fields_ = [("show_ratio", C.c_double), ("min_box_area", C.c_double)] + [(n, C.c_int32) for n in _INTS] + \
        [("label_color", C.c_uint8 * 3), ("dist_color", C.c_uint8 * 3), ("dist_shadow_color", C.c_uint8 * 3), ("offset_colors", C.c_uint8 * 12),
         ("curvature_colors", C.c_uint8 * 18), ("collision_colors", C.c_uint8 * 12), ("pad", C.c_uint8 * 5)]


class Arrays(C.Structure):  # adas_overlay_text_arrays
    _fields_ = [(n, _P) for n in ("det_xyxy", "det_cls", "det_counts", "trk_tlwh", "trk_cls", "trk_ids", "trk_counts", "trk_last_tlbr", "traj_len", "dist_points",
                                  "dist_d", "dist_counts", "offset_type", "curvature_type", "collision_type")] + \
        [("det_cap", C.c_int32), ("trk_cap", C.c_int32), ("dist_cap", C.c_int32), ("reserved", C.c_int32)]


class Tables(C.Structure):
    _fields_ = [("fonts", _P), ("det_names", _P), ("n_det_names", C.c_int32), ("trk_names", _P), ("n_trk_names", C.c_int32), ("det_colors", _P),
                ("n_det_colors", C.c_int32), ("trk_colors", _P), ("n_trk_colors", C.c_int32), ("lines", _P), ("n_lines", C.c_int32)]


def build():
    deps = [SRC, os.path.join(INC, "overlay_text_core.h")]
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
        _lib.emu_text_format_fixed.argtypes = [C.c_double, C.c_int, _P]
        _lib.emu_text_format_int.argtypes = [C.c_int, _P]
        _lib.emu_text_ladder.argtypes = [_P, C.c_int, C.c_int, C.c_double]
        _lib.emu_text_size.argtypes = [_P, C.c_char_p, C.c_int, _P]
        _lib.emu_text_layout.argtypes = [_P, _P, _P] + [C.c_int] * 5 + [_P, _P]
        _lib.emu_text_draw.argtypes = [_P] + [C.c_int] * 4 + [_P, _P, _P, C.c_int, C.c_int]
        for k, cls in enumerate((Font, Item, Style, Line)):
            assert _lib.emu_text_sizeof(k) == C.sizeof(cls), cls
    return _lib


def format_fixed(x, prec=2):
    """'%.<prec>f' by T1, or None: out of range."""
    out = C.create_string_buffer(32)
    n = lib().emu_text_format_fixed(float(x), int(prec), out)
    return None if n < 0 else out.raw[:n].decode()


def format_int(x):
    out = C.create_string_buffer(16)
    n = lib().emu_text_format_int(int(x), out)
    return out.raw[:n].decode()


def font_table(fonts, keep):
    """{slot: font dict} -> (Font * 16); the arrays it points to are appended to keep."""
    table = (Font * FONTS)()
    for slot, f in fonts.items():
        a = np.ascontiguousarray(f["atlas"], np.uint8)
        keep.append(a)
        t = table[slot]
        t.atlas, t.atlas_w, t.cell_h, t.baseline_row, t.size_h, t.size_w_extra, t.set, t.scale = a.ctypes.data, a.shape[1], a.shape[0], int(f["baseline_row"]), \
            int(f["size_h"]), int(f["size_w_extra"]), 1, float(f["scale"])
        for n in ("glyph_x", "glyph_w", "bearing_x", "advance"):
            getattr(t, n)[:] = [int(v) for v in f[n]]
    return table


def style_struct(style):
    import text_ref
    st, s = dict(text_ref.default_style(), **(style or {})), Style()
    for k, v in st.items():
        if k.endswith("_colors"):
            getattr(s, k)[:] = [int(c) for row in v for c in row]
        elif k.endswith("_color"):
            getattr(s, k)[:] = [int(c) for c in v]
        else:
            setattr(s, k, v)
    return s


def line_table(lines):
    t = (Line * 8)()
    for i, (x, y, slot, colour, text) in enumerate(lines):
        b = text.encode("latin-1")
        t[i].x, t[i].y, t[i].slot, t[i].len, t[i].text = int(x), int(y), int(slot), len(b), b
        t[i].color[:] = [int(c) for c in colour]
    return t


def name_table(names):
    a = np.zeros((max(len(names), 1), 32), np.uint8)
    for i, n in enumerate(names):
        b = n.encode("latin-1")
        a[i, :len(b)] = np.frombuffer(b, np.uint8)
    return a


def pack_colors(colors):
    return np.array([c[0] | (c[1] << 8) | (c[2] << 16) for c in colors] or [0], np.uint32)


from text_scene import pack_scenes     # noqa: E402,F401  (the scenes' arrays: shared with the GPU suite and tools/bench_text.py)


def item_dict(it):
    return dict(kind=it.kind, source=it.source, x=it.x, y=it.y, x1=it.x1, y1=it.y1, box=(it.bx0, it.by0, it.bx1, it.by1), slot=it.slot,
                color=tuple(it.color), text=it.text[:it.len].decode("latin-1") if it.len else "")


def _p(a):
    return a.ctypes.data_as(_P)


def ladder(fonts, first, count, v):
    keep = []
    return lib().emu_text_ladder(C.byref(font_table(fonts, keep)), int(first), int(count), float(v))


def size(font, s):
    keep, wh, b = [], np.zeros(2, np.int32), s.encode("latin-1")
    lib().emu_text_size(C.byref(font_table({0: font}, keep)[0]), b, len(b), _p(wh))
    return int(wh[0]), int(wh[1])


def run(frames, scenes, fonts, mask, style=None, align=0, rows=8):
    """Layout and draw the way the two kernels do, on frames [n][H][W][3] (a copy) treated as a buffer whose address is `align` mod 16; all
    frames share scenes[0]'s tables.  -> (frames, [items per frame], [flags per frame])"""
    out = np.ascontiguousarray(frames, np.uint8).copy()
    n, H, W = out.shape[:3]
    keep = []
    ft = font_table(fonts, keep)
    st = style_struct(style)
    a, caps = pack_scenes(scenes)
    arr = Arrays()
    for k, v in a.items():
        setattr(arr, k, v.ctypes.data)
    arr.det_cap, arr.trk_cap, arr.dist_cap = caps
    s0 = scenes[0]
    dn, tn, dc, tc, ln = name_table(s0["det_names"]), name_table(s0["trk_names"]), pack_colors(s0["det_colors"]), pack_colors(s0["trk_colors"]), \
        line_table(s0["lines"])
    tb = Tables(C.addressof(ft), dn.ctypes.data, len(s0["det_names"]), tn.ctypes.data, len(s0["trk_names"]), dc.ctypes.data, len(s0["det_colors"]),
                tc.ctypes.data, len(s0["trk_colors"]), C.addressof(ln), len(s0["lines"]))
    mx = st.max_text_items
    items, heads = (Item * (n * mx))(), np.zeros((n, 4), np.int32)
    lib().emu_text_layout(C.byref(arr), C.byref(tb), C.byref(st), W, H, int(mask), n, mx, items, _p(heads))
    r = lib().emu_text_draw(_p(out), n, H, W, int(align), C.byref(ft), items, _p(heads), mx, int(rows))
    assert r == 0, ("", "a byte outside the buffer", "a byte written twice", "a byte outside every item's box written")[r]
    return out, [[item_dict(items[q * mx + i]) for i in range(heads[q, 0])] for q in range(n)], [int(heads[q, 1]) for q in range(n)]
