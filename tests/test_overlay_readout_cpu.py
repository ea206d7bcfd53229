"""CPU: the bird view's readouts, rules R0-R6 (csrc/overlay_readout_core.h).  The host build of the core that the two device kernels run
(tests/hostemu/emu_overlay_readout.cpp: the layout and the draw kernel's walk of aligned 16-byte pieces) against the independent restatement
tests/readout_ref.py, byte for byte and record for record; the closed form of the vertical arrows' tips; the zoom against np.repeat;
'%.1f' against Python's; the paint order under the bird stage's discs; and the stand-alone bounds program under the sanitizers."""
import os, struct, subprocess
import numpy as np
import pytest

import emu_overlay_readout_api as emu
import emu_overlay_api as emu_ov
import overlay_ref as ref
import overlay_tracks_ref as tref
import readout_ref as RR

SIZES = [(64, 96), (101, 37), (33, 130)]          # (Wb, Hb)
ZOOMS = [1, 2, 3]
VALUES = [0.04, -0.04, 0.25, 0.35, 1234.56, float("inf"), float("nan"), float(2 ** 30)]


def veh_positions(Wb):
    return [Wb * 0.3 + 0.7, -7.5, Wb + 3.2, Wb / 2, float("nan"), 1e12]


def background(n, H, W, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def font():
    return RR.synthetic_font()


# ---- 1: byte equality over the grid
@pytest.mark.parametrize("zoom", ZOOMS)
@pytest.mark.parametrize("size", SIZES)
def test_emulation_draws_the_restatement(font, size, zoom):
    Wb, Hb = size
    cases = [(v, VALUES[i], VALUES[(i + j + 3) % 8]) for j, v in enumerate(veh_positions(Wb)) for i in range(8)]    # (veh_pos, offset, curvature)
    n = len(cases)
    birds = background(n, Hb, Wb)
    style = dict(zoom=zoom, offset_x=2, offset_y=7 * zoom, radius_x=-4, radius_y=Hb - 5)
    veh, off, cur = ([c[k] for c in cases] for k in range(3))
    got, recs = emu.run(birds, [3] * n, veh, cur, off, font, style, align=(Wb + zoom) % 16)
    n_range = 0
    for q, (v, o, c) in enumerate(cases):
        want, wrec = RR.draw(birds[q], 3, v, c, o, font, style)
        assert RR.device_record_table(recs[q]) == RR.record_table(wrec), (q, v, o, c)
        assert np.array_equal(got[q], want), (q, v, o, c, np.argwhere(got[q] != want)[:5])
        assert not np.array_equal(got[q], birds[q])
        n_range += wrec["flags"] & RR.RANGE
        assert bool(wrec["flags"] & RR.RANGE) == (v == 1e12 or o == 2.0 ** 30 or c == 2.0 ** 30)
        if v == 1e12:                                   # arrow A is skipped, the rest is drawn
            assert int(recs[q]["arrows"][0]["skipped"]) == 7 and int(recs[q]["arrows"][1]["skipped"]) == 0
        assert (recs[q]["strings"][0]["text"] == "") == (o == 2.0 ** 30)
    assert n_range > 0
    texts = {r["strings"][0]["text"] for r in recs}
    assert {"Offset: 0.0 m", "Offset: -0.0 m", "Offset: 0.2 m", "Offset: 0.3 m", "Offset: 1234.6 m", "Offset: inf m", "Offset: nan m", ""} == texts
    assert "R : 1234.6 m" in {r["strings"][1]["text"] for r in recs}


def test_every_piece_alignment(font):
    """303-byte rows: every alignment of a 16-byte piece against a row start occurs, at every alignment of the buffer."""
    Wb, Hb = 101, 37
    birds = background(2, Hb, Wb, 3)
    want = [RR.draw(birds[q], 1, 40.0 + q, 2.5, -0.35, font, dict(zoom=2))[0] for q in range(2)]
    for align in range(16):
        got, _ = emu.run(birds, [1, 1], [40.0, 41.0], [2.5, 2.5], [-0.35, -0.35], font, dict(zoom=2), align=align, rows=1 + align % 8)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), align


# ---- 2: the arrows' tips
@pytest.mark.parametrize("size", SIZES + [(1280, 720)])
def test_vertical_arrow_tips_are_the_closed_form(font, size):
    Wb, Hb = size
    _, recs = emu.run(np.zeros((1, Hb, Wb, 3), np.uint8), [3], [Wb * 0.4], [1.0], [0.0], font, None)
    for mk, (x, y_end, tip, t) in zip(recs[0]["arrows"], ((int(Wb * 0.4), int(Wb / 3), 0.2, 5), (int(Wb / 2.), int(Hb / 1.3), 0.5, 10))):
        assert (int(mk["kind"]), int(mk["x1"]), int(mk["y1"]), int(mk["x2"]), int(mk["y2"]), int(mk["thickness"])) == (tref.ARROW, x, Hb - 1, x, y_end, t)
        L = (Hb - 1) - y_end
        k = np.float64(tip) * np.float64(tref.SQRT_HALF)
        qa = (int(np.rint(np.float64(x) + k * np.float64(-L))), int(np.rint(np.float64(y_end) + k * np.float64(L))))
        qb = (int(np.rint(np.float64(x) + k * np.float64(L))), int(np.rint(np.float64(y_end) + k * np.float64(L))))
        assert tuple(int(v) for v in mk["tip"]) == qa + qb
        assert emu.arrow_tips((x, Hb - 1), (x, y_end), tip) == (qa, qb) == tref.arrow_tips((x, Hb - 1), (x, y_end), tip)
        assert qa[1] == qb[1] and qa[0] - x == -(qb[0] - x)          # mirror images about column x


# ---- 3: the zoom
@pytest.mark.parametrize("zoom", [2, 3, 4])
def test_zoom_is_the_zoom_one_run_repeated(font, zoom):
    """On a zero canvas with black arrows only the strings show: the run at zoom z is the zoom-1 run, rendered relative to its origin,
    with every glyph pixel repeated z times on both axes -- also where the image's edges cut it."""
    ox, oy, far = 8, 12, -5000
    black = dict(arrow_a_color=(0, 0, 0), arrow_b_color=(0, 0, 0), radius_x=far, radius_y=far)
    one, _ = emu.run(np.zeros((1, 24, 260, 3), np.uint8), [3], [0.0], [0.0], [-1234.56], font, dict(black, zoom=1, offset_x=ox, offset_y=oy))
    assert one[0].any() and not one[0][:, -1].any() and not one[0][0].any() and not one[0][-1].any()      # the whole run is inside
    big = np.repeat(np.repeat(one[0], zoom, axis=0), zoom, axis=1)
    Wb, Hb = 97, 41
    for x, y in ((5, 20), (-9, 3), (Wb - 30, Hb - 2), (40, Hb + 3 * zoom)):
        got, recs = emu.run(np.zeros((1, Hb, Wb, 3), np.uint8), [3], [0.0], [0.0], [-1234.56], font, dict(black, zoom=zoom, offset_x=x, offset_y=y))
        want = np.zeros((Hb, Wb, 3), np.uint8)
        for py in range(Hb):
            sy = py - y + oy * zoom
            if not 0 <= sy < big.shape[0]:
                continue
            for px in range(Wb):
                sx = px - x + ox * zoom
                if 0 <= sx < big.shape[1]:
                    want[py, px] = big[sy, sx]
        assert np.array_equal(got[0], want), (x, y)
        assert np.array_equal(got[0], RR.draw(np.zeros((Hb, Wb, 3), np.uint8), 3, 0.0, 0.0, -1234.56, font, dict(black, zoom=zoom, offset_x=x, offset_y=y))[0])
        x0, y0, x1, y1 = recs[0]["strings"][0]["box"]
        rest = got[0].copy()
        rest[y0:y1, x0:x1] = 0
        assert not rest.any()                                                                                # nothing outside the record's box


# ---- 4: '%.1f'
TIES = [0.05, 0.15, 0.25, 0.35, 0.45, 0.55, 0.65, 0.75, 0.85, 0.95, -0.05, -0.25, 0.04, -0.04, 0.0, -0.0, 2.5, 9.95, 99.95, 999.95, 0.049999999999999996,
        0.05000000000000001, 1e-320, -1e-320, 5e-324, 0.125, 0.375, 1073741823.95, 1073741823.9499998, -1073741823.9499998, 123456789.25, 1e9 + 0.75]


def test_fmt1_is_pythons():
    rng = np.random.default_rng(11)
    vals = []
    while len(vals) < 20000:
        bits = rng.integers(0, 2 ** 64, 4096, dtype=np.uint64)
        v = bits.view(np.float64)
        vals.extend(float(x) for x in v[np.abs(v) < 2.0 ** 30])                  # drops nan, inf and the out-of-range half
    for v in vals[:20000] + TIES:
        assert emu.format1(v) == "%.1f" % v == RR.fmt1(v), (v, struct.pack(">d", v).hex())
    for v, s in ((float("inf"), "inf"), (float("-inf"), "-inf"), (float("nan"), "nan")):
        assert emu.format1(v) == s == RR.fmt1(v)
    for v in (2.0 ** 30, -2.0 ** 30, 1e300, np.nextafter(2.0 ** 30, 3e9)):
        assert emu.format1(v) is None and RR.fmt1(v) is None
    assert emu.format1(np.nextafter(2.0 ** 30, 0.0)) == "%.1f" % np.nextafter(2.0 ** 30, 0.0)


# ---- 5: the order
def test_discs_lie_over_the_readouts_and_the_gate_leaves_a_frame_alone(font):
    Wb, Hb = 101, 130
    birds = background(3, Hb, Wb, 5)
    x_mid = int(Wb / 2.)
    lanes = [[(10, 20), (12, 60)], [(x_mid, Hb - 4), (x_mid - 2, int(Hb / 1.3) + 3), (30, 30)], [(70, 80), (25, 9)], [(95, 100)]]   # discs on arrow B and a string
    got, recs = emu.run(birds, [2, 0, 1], [33.0, 33.0, 70.5], [250.0, 250.0, 9.0], [0.3, 0.3, -1.25], font, dict(zoom=2, offset_y=20, radius_y=44))
    assert np.array_equal(got[1], birds[1]) and not recs[1]["drawn"] and recs[1]["flags"] == 0                 # R0: byte-identical to its input
    for q in (0, 2):
        with_discs, _ = emu_ov.compose(got[q], lanes, stages=1, radii=(10, 4), direct=True)                    # the bird stage over the readout-only image
        want, _ = RR.draw(birds[q], recs[q]["drawn"], (33.0, 0, 70.5)[q], (250.0, 0, 9.0)[q], (0.3, 0, -1.25)[q], font,
                          dict(zoom=2, offset_y=20, radius_y=44), lanes=lanes)
        assert np.array_equal(with_discs, want)
        assert np.array_equal(with_discs, ref.draw_lanes(got[q], lanes, radius=10, direct=True))
        discs_first, _ = emu.run(ref.draw_lanes(birds[q], lanes, radius=10, direct=True)[None], [1], [(33.0, 0, 70.5)[q]], [(250.0, 0, 9.0)[q]],
                                 [(0.3, 0, -1.25)[q]], font, dict(zoom=2, offset_y=20, radius_y=44))
        assert not np.array_equal(discs_first[0], with_discs)                                                  # the order matters on these frames


def test_arrow_a_under_arrow_b(font):
    """veh_pos exactly Wb / 2: both arrows on one column, B (grey, thicker, shorter) painted over A (white)."""
    Wb, Hb = 64, 96
    got, recs = emu.run(np.zeros((1, Hb, Wb, 3), np.uint8), [3], [Wb / 2], [0.0], [0.0], font, dict(offset_x=-5000, radius_x=-5000))
    x = Wb // 2
    assert tuple(got[0, Hb - 1, x]) == (150, 150, 150) and tuple(got[0, int(Hb / 1.3), x]) == (150, 150, 150)
    assert tuple(got[0, int(Wb / 3), x]) == (255, 255, 255)           # above arrow B's end only A is there
    assert tuple(got[0, Hb - 1, x + 3]) == (150, 150, 150) and tuple(got[0, Hb - 1, x + 5]) == (150, 150, 150) and not got[0, Hb - 1, x + 6].any()


# ---- 6: the stand-alone program
def lcg_bytes(state, n):
    out = np.empty(n, np.uint8)
    for i in range(n):
        state = (state * 1664525 + 1013904223) & 0xffffffff
        out[i] = state >> 24
    return state, out


def bounds_want(W, H, frames, zoom, veh, off, cur):
    g = np.arange(95)
    gw = np.where(g > 0, 1 + (g * 7) % 9, 0)
    gx = 1 + np.concatenate([[0], np.cumsum(gw + 1)[:-1]])
    aw = int(1 + np.sum(gw + 1))
    state, atlas = lcg_bytes(12345, 9 * aw)
    font = dict(atlas=atlas.reshape(9, aw), glyph_x=gx, glyph_w=gw, bearing_x=(g * 5) % 5 - 2, advance=((gw + 1) << 16) + (g * 4099) % 65536, baseline_row=6,
                size_h=7, size_w_extra=0x18000, scale=1.0)
    state, buf = lcg_bytes(state, frames * H * W * 3)
    buf = buf.reshape(frames, H, W, 3)
    style = dict(zoom=zoom, offset_x=-3, offset_y=9 * zoom // 2, radius_x=W // 2, radius_y=H - 2)
    flags = None
    for q in range(frames):
        img, rec = RR.draw(buf[q], 0 if q == 1 else 3, veh + 7.0 * q, cur, off, font, style)
        buf[q] = img
        flags = rec["flags"] if q == 0 else flags
    flat = buf.reshape(-1).astype(object)
    return flags, int(sum(int(v) * (i + 1) for i, v in enumerate(flat)))


def test_bounds_program_under_the_sanitizers():
    """tests/hostemu/readout_bounds_main.cpp with -fsanitize=address,undefined, its own main, run as a child process: layout and draw over
    bird images between guard bytes, sizes and values from its command line; the guard bytes stay intact, the exit status is 0 and the
    checksums are the restatement's.  The sanitizers' runtimes are linked statically, so the program runs in whatever environment the suite has."""
    src = os.path.join(emu.ROOT, "tests", "hostemu", "readout_bounds_main.cpp")
    exe = os.path.join(emu.ROOT, "tests", "_build", "readout_bounds")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", emu.INC, "-I", emu.API, src, "-o", exe])
    cases = [(101, 37, 2, 0, 2, 50.5, 0.25, 1234.56), (101, 37, 1, 1, 1, -7.5, -0.04, float("inf")), (101, 37, 3, 15, 3, 104.2, 0.35, 2.0 ** 30),
             (64, 96, 2, 7, 2, 32.0, float("nan"), 0.04), (33, 130, 2, 9, 4, 1e12, 1234.56, -1234.56), (5, 3, 3, 7, 1, 2.0, 0.0, 0.0), (1, 1, 1, 3, 4, 0.0, 1.0, 1.0)]
    args = ["%d,%d,%d,%d,%d,%r,%r,%r" % c for c in cases]
    p = subprocess.run([exe] + args, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.strip().splitlines()
    assert len(out) == len(cases)
    for line, arg, (W, H, frames, align, zoom, veh, off, cur) in zip(out, args, cases):
        flags, total = bounds_want(W, H, frames, zoom, veh, off, cur)
        assert line.split() == [arg, "flags", str(flags), "sum", str(total)], line
