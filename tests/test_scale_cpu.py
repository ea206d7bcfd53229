"""The scaling stage's rules S1-S8 (csrc/scale_core.h) without a GPU: the host build walks the device kernel's work items, every load and
store audited for bounds, alignment and writing each canvas byte exactly once (tests/hostemu/emu_scale.cpp), against the independent
statement tests/scale_ref.py."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import emu_scale_api as emu
import scale_ref as ref
from conftest import ROOT, load_pkg

SOURCES = ((48, 16), (50, 18), (7, 5))      # 48 * 3 and its tiles' rows are multiples of 16, 50 * 3 is not, 7 x 5 is smaller than a vector item
MOSAICS = ((1, 1), (2, 2), (3, 1))
BATCHES = (3, 5)                            # (2, 2) sees one and three empty cells and a second canvas
STATES = np.array([0, 1, 2, 3, 7], np.int32)   # the four values and one outside the enum
BACKGROUND = (1, 2, 3)


def tile_sizes(w, h):
    """(size, modes): ratio 2, ratio 3, a non-integer ratio on each axis, 1:1, 1x1, and an enlargement for `linear` alone"""
    both = ("area", "linear")
    return (((w // 2, h // 2), both), ((max(1, w // 3), max(1, h // 3)), both), ((w * 3 // 4, h * 2 // 3), both), ((w, h), both), ((1, 1), both),
            ((w + 7, h + 5), ("linear",)))


def grid():
    """(src_wh, size, mode, mosaic, batch, border): what both suites run"""
    for src in SOURCES:
        for size, modes in tile_sizes(*src):
            for mode in modes:
                for mosaic in MOSAICS:
                    for batch in BATCHES:
                        for border in (0, 1):
                            if 2 * border < min(size):
                                yield src, size, mode, mosaic, batch, border


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def path_expected(size, mode, src_offset, dst_offset):
    """S8: the tile's row bytes and both pointers multiples of 16 (the pointers are the test's own: `offset` off a multiple of 64) take
    `area` through the staged blocks (2) and `linear` through the vector items (1); anything else the generic items (0).  The sources of
    this suite are narrow enough to stage."""
    if (size[0] * 3) % 16 or src_offset % 16 or dst_offset % 16:
        return 0
    return 2 if mode == "area" else 1


@pytest.mark.parametrize("src", SOURCES)
def test_emulator_equals_reference_and_every_access_is_audited(src):
    """The whole grid at source and destination 0 and 1 bytes off alignment: the canvases equal the reference's, no load outside the source
    frames, no store outside the canvases (sentinel guard bands), every canvas byte stored exactly once, the vector path exactly when S8 says."""
    n = vec = 0
    for s, size, mode, mosaic, batch, border in grid():
        if s != src:
            continue
        bgr = noise((batch, s[1], s[0], 3), n)
        st = STATES[:batch]
        p = emu.params(s, size, mode, mosaic, border, BACKGROUND)
        want = ref.scale(bgr, size, mode, mosaic, border, BACKGROUND, states=st)
        for so, do in ((0, 0), (1, 1), (0, 1), (1, 0)):
            r = emu.run(bgr, p, st, src_offset=so, dst_offset=do)
            what = (s, size, mode, mosaic, batch, border, so, do)
            assert r.vector == path_expected(size, mode, so, do), what
            assert (r.outside, r.misaligned, r.not_once) == (0, 0, 0) and r.guard_ok, what
            assert r.wide == (r.stores if r.vector else 0), what
            assert r.state_loads == 0 or border > 0, what
            assert np.array_equal(r.out, want), what
            vec += r.vector != 0
        forced = emu.run(bgr, p, st, path=0)        # the generic items on aligned pointers: the same bytes
        assert not forced.vector and np.array_equal(forced.out, want) and forced.not_once == 0
        n += 1
    assert n and (vec > 0) == (src != (7, 5))      # 16-pixel tiles come from 48 / 3 and 50 // 3; 7 x 5 has no tile width that is a multiple of 16


def test_a_source_too_wide_to_stage_takes_the_generic_items():
    """scale_staged_plan: a tile row's segment may need up to 16 KB of a source row; 6000 pixels for 16 are 18000 bytes"""
    bgr = noise((2, 2, 6000, 3), 4)
    for w, path in ((5400, 2), (6000, 0)):
        r = emu.run(bgr[:, :, :w], emu.params((w, 2), (16, 1), "area"))
        assert r.vector == path and (r.outside, r.misaligned, r.not_once) == (0, 0, 0), (w, r.vector)
        assert np.array_equal(r.out, ref.scale(bgr[:, :, :w], (16, 1), "area"))
    assert emu.run(bgr, emu.params((6000, 2), (16, 1), "linear")).vector == 1


def test_no_states_no_border_and_empty_cells_have_none():
    bgr = noise((3, 16, 48, 3), 1)
    p = emu.params((48, 16), (16, 8), "area", (2, 2), 2, BACKGROUND)
    without = emu.scale(bgr, p, None)
    assert np.array_equal(without, ref.scale(bgr, (16, 8), "area", (2, 2), 0, BACKGROUND))
    with_states = emu.scale(bgr, p, np.array([3, 2, -5], np.int32))
    assert (with_states[0, 0, :16] == (0, 0, 255)).all() and (with_states[0, 1, 16:32] == (0, 102, 255)).all()
    assert (with_states[0, 8:10, :16] == (0, 255, 255)).all()          # -5 counts as UNKNOWN
    assert (with_states[0, 8:, 16:] == BACKGROUND).all()                # the empty cell: background to its edge
    assert np.array_equal(with_states[0, 2:6, 2:14], without[0, 2:6, 2:14])


@pytest.mark.parametrize("mode", ("area", "linear"))
def test_a_constant_image_stays_constant(mode):
    for (w, h), size in (((48, 16), (16, 5)), ((50, 18), (37, 12)), ((7, 5), (3, 2)), ((7, 5), (1, 1))):
        for value in ((0, 0, 0), (255, 255, 255), (13, 200, 77)):
            bgr = np.empty((1, h, w, 3), np.uint8)
            bgr[:] = value
            assert (emu.scale(bgr, emu.params((w, h), size, mode)) == value).all(), (w, h, size, value)


def test_area_at_ratio_two_is_the_rounded_mean_of_four():
    bgr = noise((2, 18, 50, 3), 2).astype(np.int64)
    want = (bgr[:, 0::2, 0::2] + bgr[:, 0::2, 1::2] + bgr[:, 1::2, 0::2] + bgr[:, 1::2, 1::2] + 2) >> 2
    assert np.array_equal(emu.scale(bgr.astype(np.uint8), emu.params((50, 18), (25, 9), "area")), want.astype(np.uint8))


@pytest.mark.parametrize("mode", ("area", "linear"))
def test_equal_sizes_are_a_copy(mode):
    for w, h in SOURCES:
        bgr = noise((2, h, w, 3), 3)
        assert np.array_equal(emu.scale(bgr, emu.params((w, h), (w, h), mode)), bgr)


def test_area_weights_sum_to_the_source_side():
    """sum wx = src_w, sum wy = src_h for every size pair of the grid, the camera's and the largest side; the header's weights are the formula's"""
    pairs = {(src[a], size[a]) for src in SOURCES for size, modes in tile_sizes(*src) if "area" in modes for a in (0, 1)}
    pairs |= {(1280, 640), (1280, 160), (720, 90), (1280, 320), (720, 180), (16383, 7), (16383, 16383), (16383, 1)}
    for sn, dn in sorted(pairs):
        W = ref.area_weights(dn, sn) if sn <= 1280 else None
        for d in range(dn) if sn <= 1280 else (0, dn // 2, dn - 1):
            lo, w = emu.area_weights(d, dn, sn)
            assert sum(w) == sn and min(w) > 0, (sn, dn, d)
            if W is not None:
                assert list(W[d, lo:lo + len(w)]) == w and W[d].sum() == sn, (sn, dn, d)


def test_the_numerator_stays_below_2_to_the_31_at_the_largest_d():
    """S5's bound: 255 * D + D / 2 < 2^31 at D = 2^23, the largest accepted; a white 4096 x 2048 frame comes out white, one more row is refused"""
    D = 1 << 23
    assert 255 * D + D // 2 == 2143289344 < 1 << 31
    p = emu.params((4096, 2048), (1, 1), "area")
    assert emu.check(p) is None
    white = np.full((1, 2048, 4096, 3), 255, np.uint8)
    r = emu.run(white, p)
    assert (r.out == 255).all() and r.outside == 0 and r.not_once == 0
    assert emu.check(emu.params((4096, 2049), (1, 1), "area")) == "big D"
    assert emu.check(emu.params((4096, 2049), (1, 1), "linear")) is None


def test_refusals_of_the_header():
    ok = dict(src_wh=(48, 16), size=(16, 8))
    assert emu.check(emu.params(**ok)) is None
    assert emu.check(emu.params(mode=2, **ok)) == "mode"
    assert emu.check(emu.params((48, 16), (0, 8))) == "size" and emu.check(emu.params((0, 16), (16, 8))) == "size"
    assert emu.check(emu.params((16384, 16), (16, 8), "linear")) == "size"
    assert emu.check(emu.params(mosaic=(0, 1), **ok)) == "mosaic"
    assert emu.check(emu.params((48, 16), (49, 8))) == "enlarge" and emu.check(emu.params((48, 16), (16, 17))) == "enlarge"
    assert emu.check(emu.params((48, 16), (49, 17), "linear")) is None
    assert emu.check(emu.params(border=4, **ok)) == "border" and emu.check(emu.params(border=3, **ok)) is None
    assert emu.check(emu.params(border=-1, **ok)) == "border"
    assert emu.check(emu.params((48, 16), (16000, 16000), "linear", (3, 1))) == "big canvas"
    assert emu.canvas_bytes(emu.params(mosaic=(3, 2), **ok)) == 3 * 16 * 2 * 8 * 3
    assert [emu.canvases(emu.params(mosaic=(2, 2), **ok), b) for b in (1, 4, 5, 8, 9)] == [1, 1, 2, 2, 3]


def test_params_layout_three_ways(tmp_path):
    """adas_scale_params as gcc compiles the public header, _lib.ScaleParams, the core header's ScaleParams and the emulation's ctypes mirror"""
    load_pkg()
    L = importlib.import_module("adas_amd._lib")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "adas_hip.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(adas_scale_params));']
    for fname, _ in L.ScaleParams._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(adas_scale_params, %s));' % (fname, fname))
    lines += ['  printf("consts %d %d %d %d\\n", ADAS_SCALE_AREA, ADAS_SCALE_LINEAR, ADAS_SCALE_SRC_OVERLAY, ADAS_SCALE_SRC_FRAMES);', '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split(" ", 1) for l in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    size, offsets = emu.params_layout()
    assert int(got["size"]) == C.sizeof(L.ScaleParams) == C.sizeof(emu.Params) == size == 52
    assert [f for f, _ in L.ScaleParams._fields_] == [f for f, _ in emu.Params._fields_] == list(emu.FIELDS)
    for fname, _ in L.ScaleParams._fields_:
        assert int(got[fname]) == getattr(L.ScaleParams, fname).offset == getattr(emu.Params, fname).offset == offsets[fname], fname
    assert got["consts"].split() == [str(L.SCALE_MODES[m]) for m in ("area", "linear")] + [str(L.SCALE_SOURCES[s]) for s in ("overlay", "frames")]
    assert L.SCALE_MODES == emu.MODES


def test_refusals_arrive_by_name_through_create():
    """adas_scale_create checks its parameters before it touches a device"""
    load_pkg()
    L = importlib.import_module("adas_amd._lib")
    PP = importlib.import_module("adas_amd.postproc")

    def refused(match, src=(48, 16), size=(16, 8), max_batch=1, **fields):
        p = L.ScaleParams()
        L.check(L.lib().adas_scale_default_params(C.byref(p), src[0], src[1], size[0], size[1]))
        assert (p.mode, p.cols, p.rows, p.border) == (0, 1, 1, 0) and bytes(p.background) == bytes(4)
        assert tuple(tuple(c)[:3] for c in p.border_bgr) == emu.DEFAULT_COLORS == ref.DEFAULT_COLORS == PP.SCALE_DEFAULT_BORDER_COLORS
        for k, v in fields.items():
            setattr(p, k, v)
        h_ = C.c_void_p()
        with pytest.raises(RuntimeError, match=match) as ei:
            L.check(L.lib().adas_scale_create(C.byref(p), max_batch, C.byref(h_)))
        assert ei.value.code == -1 and not h_.value
        if not match.endswith("max_batch 0"):
            assert L.lib().adas_scale_canvas_bytes(C.byref(p)) == 0 and L.lib().adas_scale_canvases(C.byref(p), 4) == 0

    refused("adas_scale_create: unknown mode", mode=2)
    refused("adas_scale_create: source and tile sides must be in 1..16383", dst_w=0)
    refused("adas_scale_create: source and tile sides must be in 1..16383", mode=1, src_h=16384)
    refused("adas_scale_create: mosaic columns and rows must be in 1..16383", rows=0)
    refused("adas_scale_create: area does not enlarge", size=(49, 8))
    refused("adas_scale_create: area does not enlarge", size=(16, 17))
    refused("adas_scale_create: area needs src_w \\* src_h <= 8388608", src=(4096, 2049))
    refused("adas_scale_create: border must be >= 0 and 2 \\* border < min\\(dst_w, dst_h\\)", border=4)
    refused("adas_scale_create: a canvas must stay below 2\\^31 bytes", size=(16000, 16000), mode=1, cols=3)
    refused("adas_scale_create: max_batch 0", max_batch=0)
    p = L.ScaleParams()
    assert L.lib().adas_scale_default_params(C.byref(p), 0, 16, 16, 8) == -1 and L.lib().adas_scale_default_params(C.byref(p), 48, 16, 16, 16384) == -1
    L.check(L.lib().adas_scale_default_params(C.byref(p), 1280, 720, 160, 90))
    p.cols = p.rows = 8
    assert L.lib().adas_scale_canvas_bytes(C.byref(p)) == 1280 * 720 * 3
    assert [L.lib().adas_scale_canvases(C.byref(p), b) for b in (1, 64, 65)] == [1, 1, 2]


def test_pipeline_arguments_without_a_gpu():
    """AdasPipeline(scale=...) and FrameScaler refuse by ValueError naming the key, before any engine or handle is created."""
    load_pkg()
    PL = importlib.import_module("adas_amd.pipeline")
    PP = importlib.import_module("adas_amd.postproc")
    missing = "/nonexistent/model.hipm"          # never opened: every check below comes first
    fr = dict(size=(160, 90), source="frames")
    for kw, match in ((dict(fr, ratio=2), "scale= holds unknown keys \\['ratio'\\]"),
                      (dict(source="frames"), "scale= needs size="),
                      (dict(fr, size=160), "scale= size 160 is no pair"),
                      (dict(fr, size=(0, 90)), "scale= size \\(0, 90\\) is no pair"),
                      (dict(fr, mode="cubic"), "scale= mode 'cubic' is neither"),
                      (dict(fr, size=(1281, 90)), "scale= mode \"area\" does not enlarge"),
                      (dict(fr, mosaic=(0, 1)), "scale= mosaic \\(0, 1\\) is no pair"),
                      (dict(fr, border=45), "scale= border 45 must be"),
                      (dict(fr, border=-1), "scale= border -1 must be"),
                      (dict(fr, background=(0, 0, 256)), "scale= background \\(0, 0, 256\\) is no \\(B, G, R\\)"),
                      (dict(fr, border_colors=[(0, 0, 0)] * 3), "scale= border_colors .* is no list of four"),
                      (dict(fr, source="screen"), "scale= source 'screen' is neither"),
                      (dict(size=(160, 90)), "scale= with source=\"overlay\" needs overlay="),
                      (dict(fr, border=2), "scale= with border > 0 needs analysis="),
                      (dict(fr, jpeg=dict(source="frames")), "scale= jpeg holds unknown keys \\['source'\\]"),
                      (dict(fr, jpeg=dict(quality=0)), "scale= jpeg quality 0 is outside"),
                      (dict(fr, yuv=dict(source="frames")), "scale= yuv holds unknown keys \\['source'\\]"),
                      (dict(fr, yuv=dict(format="p010")), "scale= yuv format 'p010' is none of")):
        with pytest.raises(ValueError, match=match):
            PL.AdasPipeline(None, missing, scale=kw)
    with pytest.raises(ValueError, match="scale= 'area' is neither None nor a dict"):
        PL.AdasPipeline(None, missing, scale="area")
    for a, kw, match in ((((48, 16), (16, 8)), dict(mode="cubic"), "mode 'cubic' is neither"), (((48, 16), (49, 8)), {}, "does not enlarge"),
                         (((4096, 2049), (16, 8)), {}, "needs src_w \\* src_h <= 8388608"), (((48, 16), (16, 8)), dict(border=4), "border 4 must be"),
                         (((48, 16), (16, 8)), dict(mosaic=(1, 0)), "mosaic \\(1, 0\\) is no pair")):
        with pytest.raises(ValueError, match=match):
            PP.FrameScaler(*a, **kw)


def lcg_bytes(n):
    s, out = 12345, np.empty(n, np.uint8)
    for i in range(n):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = s >> 24
    return out


def test_bounds_program_under_the_sanitizers():
    """tests/hostemu/scale_bounds_main.cpp with -fsanitize=address,undefined, its own main, run as a child process: the work items over heap
    blocks that end exactly where the frames, the states and the canvases end; the checksums are the reference's.  The sanitizers' runtimes
    are linked statically, so the program runs in whatever environment the suite has."""
    src = os.path.join(emu.ROOT, "tests", "hostemu", "scale_bounds_main.cpp")
    exe = os.path.join(emu.ROOT, "tests", "_build", "scale_bounds")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", emu.INC, src, "-o", exe])
    # src_w, src_h, dst_w, dst_h, mode, cols, rows, batch, border, align
    cases = [(48, 16, 16, 8, 0, 2, 2, 5, 1, 0), (48, 16, 16, 5, 1, 2, 2, 3, 1, 0), (50, 18, 25, 9, 0, 2, 2, 5, 1, 1), (50, 18, 37, 12, 1, 3, 1, 5, 0, 1),
             (7, 5, 1, 1, 0, 3, 1, 5, 0, 0), (7, 5, 14, 10, 1, 1, 1, 3, 2, 15), (48, 16, 48, 16, 0, 1, 1, 3, 0, 0), (64, 33, 16, 7, 0, 3, 2, 7, 3, 0),
             (700, 9, 272, 4, 0, 2, 1, 3, 1, 0), (1283, 5, 160, 2, 0, 2, 2, 5, 0, 0)]
    p = subprocess.run([exe] + [",".join(str(v) for v in c) for c in cases], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == len(cases)
    for c, line in zip(cases, lines):
        sw, sh, dw, dh, mode, cols, rows, batch, border, align = c
        bgr = lcg_bytes(batch * sh * sw * 3).reshape(batch, sh, sw, 3)
        states = [f % 6 - 1 for f in range(batch)]
        want = ref.scale(bgr, (dw, dh), ("area", "linear")[mode], (cols, rows), border, (9, 8, 7), states=states)
        s = 2166136261
        for b in want.tobytes():
            s = ((s ^ b) * 16777619) & 0xFFFFFFFF
        vec = (2 - mode) * int((dw * 3) % 16 == 0 and align == 0)      # malloc's blocks are 16-byte aligned; 2 staged blocks, 1 vector items
        assert line == "%s %08x path %d outside 0 misaligned 0 not_once 0" % (",".join(str(v) for v in c), s, vec), (c, line)
