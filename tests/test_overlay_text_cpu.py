"""CPU: the host build of the overlay text's rules (csrc/overlay_text_core.h through tests/hostemu/emu_overlay_text.cpp) against Python's own
number formatting and the NumPy restatement tests/text_ref.py: every string, every item field, every byte, no tolerances."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import emu_overlay_text_api as emu
import text_ref as R
import text_scene as TS

SIZES = ((37, 101), (16, 64))       # H, W: rows of 303 and 192 bytes
ALIGNS = (0, 1, 15)


@pytest.fixture(scope="module")
def fonts():
    return TS.fonts()


def ulp(x, k):
    return struct.unpack("<d", struct.pack("<q", struct.unpack("<q", struct.pack("<d", x))[0] + k))[0]


# ---- T1
TIES = [0.125, 0.375, 2.675, 0.005, 0.015, 1.005, 999999.995, 2.125, 0.5, 1.5, 2.5, 0.25, 0.35, 0.045, 1e-9, 123456789.125]


@pytest.mark.parametrize("prec", (2, 1))
def test_format_ties_and_near_ties(prec):
    for v in TIES:
        for x in (v, -v, ulp(v, 1), ulp(v, -1)):
            assert emu.format_fixed(x, prec) == "%.*f" % (prec, x), repr(x)


def test_format_signs_specials_and_range():
    assert emu.format_fixed(-0.004) == "-0.00" == "%.2f" % -0.004
    assert emu.format_fixed(-0.0) == "-0.00" and emu.format_fixed(0.0) == "0.00"
    for x in (5e-324, -5e-324, 2.2250738585072014e-308, ulp(2.2250738585072014e-308, -1), 1e-300):
        assert emu.format_fixed(x) == "%.2f" % x
    assert emu.format_fixed(float("nan")) == "nan" == "%.2f" % float("nan")
    assert emu.format_fixed(-float("nan")) == "nan"
    assert emu.format_fixed(float("inf")) == "inf" == "%.2f" % float("inf")
    assert emu.format_fixed(-float("inf")) == "-inf" == "%.2f" % -float("inf")
    below = ulp(2.0 ** 30, -1)
    assert emu.format_fixed(below) == "%.2f" % below and emu.format_fixed(-below, 1) == "%.1f" % -below
    assert emu.format_fixed(2.0 ** 30) is None and emu.format_fixed(ulp(2.0 ** 30, 1)) is None and emu.format_fixed(-2.0 ** 30) is None
    assert emu.format_fixed(1e300) is None


def test_format_20000_seeded_doubles():
    rng = np.random.default_rng(2024)
    x = np.exp(rng.uniform(math.log(1e-12), math.log(2.0 ** 30 - 1), 20000)) * rng.choice((-1.0, 1.0), 20000)
    bad = [(v, emu.format_fixed(v), "%.2f" % v) for v in x.tolist() if emu.format_fixed(v) != "%.2f" % v]
    assert not bad, bad[:5]
    bad = [v for v in x[:4000].tolist() if emu.format_fixed(v, 1) != "%.1f" % v]
    assert not bad, bad[:5]


def test_format_int():
    for v in (0, 1, -1, 9, 10, 4999, 2147483647, -2147483648, 1000000):
        assert emu.format_int(v) == "%d" % v


# ---- T2, ladders
def test_text_size(fonts):
    for slot in (0, 5, 13):
        for s in ("", " ", "car", "a-class-name-of-31-bytes-long..", " 12.34 m", "\xe9?\x01"):
            assert emu.size(fonts[slot], s) == R.text_size(fonts[slot], s)


def test_ladder_choice_and_tie(fonts):
    first, count = TS.LADDER
    want = {0.1: 10, 0.5: 10, 0.62: 10, 0.625: 10, 0.63: 11, 0.75: 11, 0.875: 11, 0.88: 12, 1.0: 12, 3.0: 12}   # 0.625 and 0.875 tie: the smaller
    for v, slot in want.items():
        assert emu.ladder(fonts, first, count, v) == slot == R.ladder(fonts, first, count, v), v
    assert emu.ladder(fonts, 5, 1, 0.4) == 5          # a ladder of one slot


# ---- items
def both(frames, scenes, fonts, mask, style=None, align=0):
    got, items, flags = emu.run(frames, scenes, fonts, mask, style=style, align=align)
    want = np.ascontiguousarray(frames).copy()
    w_items, w_flags = [], []
    for q, s in enumerate(scenes):
        it, fl = R.layout(s, fonts, frames.shape[2], frames.shape[1], mask, style)
        R.paint(want[q], it, fonts)
        w_items.append(it)
        w_flags.append(fl)
    return got, items, flags, want, w_items, w_flags


def same_items(items, w_items):
    for q, (a, b) in enumerate(zip(items, w_items)):
        assert [TS.item_tuple(i) for i in a] == [TS.item_tuple(i) for i in b], q


def test_items_of_a_full_frame(fonts):
    """Every kind at 1280 x 720, three frames: the layout only (the bytes at this size are the GPU suite's)."""
    scenes = [TS.scene_full(1280, 720, seed=k, n_dist=14)[0] for k in range(3)]
    frames = TS.background(3, 720, 1280)
    got, items, flags, want, w_items, w_flags = both(frames, scenes, fonts, 63, TS.STYLE, align=5)
    same_items(items, w_items)
    assert flags == w_flags and all(f & R.RANGE for f in flags)      # the distance of 2^30
    assert np.array_equal(got, want)
    for q, s in enumerate(scenes):
        it, fl = R.layout(s, fonts, 1280, 720, 63, TS.STYLE)
        texts = [i["text"] for i in it]
        assert " unknown m" in texts and " 2.12 m" in texts and " 0.38 m" in texts and " 0.00 m" in texts and " nan m" in texts
        assert any(t.startswith("unknown : ") or t == "unknown" for t in texts)
        assert any(t.startswith("LDWS : ") for t in texts) and any(t.startswith("ID: ") for t in texts)
        dist = [i for i in it if i["source"] == R.DISTANCE and i["text"] == " 1.60 m"]
        assert [i["slot"] for i in dist] == [7, 10]                  # the shadow's ladder of one slot; the tie picks scale 0.5


def test_every_enum_string(fonts):
    seen = set()
    for k in range(6):
        s = TS.empty_scene()
        s["offset"], s["curvature"], s["collision"] = k % 4, k, k % 4
        got, items, flags, want, w_items, w_flags = both(TS.background(1, 300, 420), [s], fonts, R.PANELS)
        same_items(items, w_items)
        assert np.array_equal(got, want)
        seen |= {i["text"] for i in items[0]}
    assert seen == {"LDWS : " + v for v in R.OFFSET} | {"LKAS : " + v for v in R.CURVATURE} | {"FCWS : " + v for v in R.COLLISION}


# ---- bytes
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("hw", SIZES)
@pytest.mark.parametrize("scene", ("edges", "labels", "overflow", "overlap"))
def test_bytes(fonts, scene, hw, align):
    H, W = hw
    s, mask = {"edges": TS.scene_edges, "labels": TS.scene_labels, "overflow": TS.scene_overflow, "overlap": lambda w, h: TS.scene_overlap(w, h, False)}[scene](W, H)
    s2 = TS.scene_full(W, H, seed=3)[0]
    frames = TS.background(2, H, W)
    scenes = [s, dict(s2, lines=s["lines"])]        # the handle's lines are shared by its frames
    mask2 = mask | (R.LINES if scene != "overflow" else 0)
    got, items, flags, want, w_items, w_flags = both(frames, scenes, fonts, mask2, TS.STYLE, align)
    same_items(items, w_items)
    assert flags == w_flags
    assert np.array_equal(got, want)
    assert not np.array_equal(got[0], frames[0])
    if scene == "overflow":
        assert flags[0] == R.OVERFLOW and len(items[0]) == 256 and len(s["det_cls"]) * 2 == 258
        full, _ = R.layout(s, fonts, W, H, mask, dict(TS.STYLE, max_text_items=1024))
        assert TS.item_tuple(items[0][255]) == TS.item_tuple(full[255]) and len(full) == 258


def test_overlapping_strings_depend_on_their_order(fonts):
    H, W = SIZES[0]
    frames = TS.background(1, H, W)
    out = []
    for swap in (False, True):
        s, mask = TS.scene_overlap(W, H, swap)
        got, items, flags, want, w_items, w_flags = both(frames, [s], fonts, mask)
        assert np.array_equal(got, want)
        out.append(got)
    assert not np.array_equal(out[0], out[1])


def test_coverage_values_and_substitution(fonts):
    f = fonts[TS.LINE_SLOT]
    c = ord("c") - 32
    assert list(f["atlas"][0, f["glyph_x"][c]:f["glyph_x"][c] + 4]) == [1, 127, 128, 254]
    H, W = SIZES[0]
    s = TS.empty_scene()
    s["lines"] = [(20, 20, TS.LINE_SLOT, (255, 0, 77), "c"), (40, 20, TS.LINE_SLOT, (9, 200, 0), "\xe9"), (60, 20, TS.LINE_SLOT, (9, 200, 0), "?")]
    frames = TS.background(1, H, W)
    got, items, flags, want, w_items, w_flags = both(frames, [s], fonts, R.LINES)
    assert np.array_equal(got, want)
    top = 20 - f["baseline_row"]
    x0 = 20 + int(f["bearing_x"][c])
    for k, cov in enumerate((1, 127, 128, 254)):
        for ch in range(3):
            assert got[0, top, x0 + k, ch] == (int(frames[0, top, x0 + k, ch]) * (255 - cov) + (255, 0, 77)[ch] * cov + 127) // 255
    q = ord("?") - 32                                  # the two strings paint the same glyph
    a = got[0, :, 40 + int(f["bearing_x"][q]):40 + int(f["bearing_x"][q]) + int(f["glyph_w"][q])]
    b = got[0, :, 60 + int(f["bearing_x"][q]):60 + int(f["bearing_x"][q]) + int(f["glyph_w"][q])]
    assert not np.array_equal(a, frames[0, :, 40 + int(f["bearing_x"][q]):40 + int(f["bearing_x"][q]) + int(f["glyph_w"][q])]) and a.shape == b.shape


# ---- the stand-alone program
def lcg_bytes(state, n):
    out = np.empty(n, np.uint8)
    for i in range(n):
        state = (state * 1664525 + 1013904223) & 0xffffffff
        out[i] = state >> 24
    return state, out


def bounds_want(W, H, frames):
    g = np.arange(95)
    gw = np.where(g > 0, 1 + (g * 7) % 9, 0)
    gx = 1 + np.concatenate([[0], np.cumsum(gw + 1)[:-1]])
    aw = int(1 + np.sum(gw + 1))
    state, atlas = lcg_bytes(12345, 9 * aw)
    font = dict(atlas=atlas.reshape(9, aw), glyph_x=gx, glyph_w=gw, bearing_x=(g * 5) % 5 - 2, advance=((gw + 1) << 16) + (g * 4099) % 65536, baseline_row=6,
                size_h=7, size_w_extra=0x18000, scale=1.0)
    state, buf = lcg_bytes(state, frames * H * W * 3)
    buf = buf.reshape(frames, H, W, 3)
    L = [(-4, H // 2, "Left edge"), (W - 7, H // 2 + 3, "Right edge"), (W // 3, 2, "Top"), (W // 4, H + 4, "Bottom"), (W + 40, 5, "outside"),
         (W // 2, H // 2, ""), (W // 2, H - 4, "a\x7fb\xe9"), (-300, -300, "far")]
    lines = [(x, y, 0, ((40 * k) & 255, (255 - 30 * k) & 255, (7 * k) & 255), s) for k, (x, y, s) in enumerate(L)]
    style = dict(det_size_slot=0, det_label_slot=0)
    n_items = None
    for q in range(frames):
        b = [(3 + q, 0), (W // 2, H // 2), (W - 12, H - 3 + q), (-6, 14)]
        s = dict(det_xyxy=[(x, y, x + 9, y + 9) for x, y in b], det_cls=[0, 9, 0, 1], det_names=["car", "person"],
                 det_colors=[(0xff, 0x40, 0x00), (0x14, 0xc8, 0x19)], lines=lines)
        items, _ = R.layout(s, {0: font}, W, H, R.DETECTIONS | R.LINES, style)
        R.paint(buf[q], items, {0: font})
        n_items = len(items) if q == 0 else n_items
    flat = buf.reshape(-1).astype(object)
    return n_items, int(sum(int(v) * (i + 1) for i, v in enumerate(flat)))


def test_bounds_program_under_the_sanitizers():
    """tests/hostemu/text_bounds_main.cpp with -fsanitize=address,undefined, its own main, run as a child process: layout and draw over the
    clipped scenes with the frames in an exactly-sized heap block; the checksums are the restatement's.  The sanitizers' runtimes are linked
    statically, so the program runs in whatever environment the suite has."""
    src = os.path.join(emu.ROOT, "tests", "hostemu", "text_bounds_main.cpp")
    exe = os.path.join(emu.ROOT, "tests", "_build", "text_bounds")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", emu.INC, src, "-o", exe])
    cases = [(101, 37, 2, 0), (101, 37, 1, 1), (101, 37, 2, 15), (64, 16, 2, 0), (64, 16, 1, 1), (64, 16, 2, 15), (5, 3, 3, 7)]
    p = subprocess.run([exe] + ["%d,%d,%d,%d" % c for c in cases], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.strip().splitlines()
    assert len(out) == len(cases)
    for line, (W, H, frames, align) in zip(out, cases):
        n_items, total = bounds_want(W, H, frames)
        assert line.split() == ["%d,%d,%d,%d" % (W, H, frames, align), "items", str(n_items), "sum", str(total)], line
