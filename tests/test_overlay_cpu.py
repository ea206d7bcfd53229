"""The lane overlay's pixel rules on the CPU: the NumPy restatement (tests/overlay_ref.py, from the stepping definitions) and the host
build of csrc/overlay_core.h (closed forms, bit planes) against known answers written out as literals, and against each other byte for
byte on seeded random cases and the edge cases."""
import numpy as np
import pytest

import emu_overlay_api as emu
import overlay_ref as ref

IMPLS = [pytest.param(ref, id="restatement"), pytest.param(emu, id="core")]
H, W = 36, 48
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1

BLENDS = [(0, .3, 5, 4), (0, .3, 15, 10), (255, .3, 5, 80), (5, .85, 0, 4), (30, .85, 0, 26), (50, .85, 255, 81), (10, .85, 191, 37)]
DISCS = {1: [1, 0], 3: [3, 2, 2, 0], 4: [4, 3, 3, 2, 0], 10: [10, 9, 9, 9, 9, 8, 8, 7, 6, 4, 0]}
POLY = [(10, 5), (8, 12), (8, 12), (3, 20), (2, 30), (40, 30), (35, 21), (30, 12), (28, 5)]
POLY_ROWS = {5: (10, 28, 19), 7: (9, 29, 21), 11: (8, 30, 23), 16: (5, 32, 28), 20: (3, 34, 32), 25: (2, 37, 36), 30: (2, 40, 39)}
BOWTIE = [(5, 2), (30, 20), (30, 2), (5, 20)]


def _blend(impl, a, alpha, b):
    return int(impl.blend(a, alpha, b))


@pytest.mark.parametrize("impl", IMPLS)
def test_blend_known_answers(impl):
    for a, alpha, b, want in BLENDS:
        assert _blend(impl, a, alpha, b) == want, (a, alpha, b)


@pytest.mark.parametrize("impl", IMPLS)
def test_blend_identity(impl):
    for alpha in (0.3, 0.85):
        assert [_blend(impl, p, alpha, p) for p in range(256)] == list(range(256))


def test_blend_core_equals_restatement_everywhere():
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for alpha in (0.3, 0.85, 0.5, 0.0, 1.0):
        want = ref.blend(a, alpha, b)
        got = np.array([[emu.blend(i, alpha, j) for j in range(256)] for i in range(0, 256, 5)], np.uint8)
        assert np.array_equal(got, want[::5])


def test_blend_association_is_part_of_the_definition():
    """Over all 65536 (a, b) pairs an FMA form differs from D1 in 153 (alpha 0.3) and 386 (alpha 0.85) cases; an fp64 form differs too (how
    often depends on how the fp64 form is written: rint(a * alpha + b * (1 - alpha)) in doubles gives 777 and 486)."""
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for alpha, n_fma, n_f64 in ((0.3, 153, 777), (0.85, 386, 486)):
        want = ref.blend(a, alpha, b).astype(np.int64)
        af, bf = np.float32(alpha), np.float32(1.0 - alpha)
        pb = (b.astype(np.float32) * bf).astype(np.float64)
        fma = np.rint((a.astype(np.float64) * np.float64(af) + pb).astype(np.float32))      # one rounding for a * af + pb
        f64 = np.rint(a * float(alpha) + b * (1.0 - float(alpha)))
        assert int((fma != want).sum()) == n_fma
        assert int((f64 != want).sum()) == n_f64


@pytest.mark.parametrize("impl", IMPLS)
def test_disc_halfwidths_known_answers(impl):
    for r, want in DISCS.items():
        assert list(impl.disc_halfwidths(r)) == want


@pytest.mark.parametrize("impl", IMPLS)
def test_polygon_known_rows(impl):
    m, flags = impl.poly_mask(POLY, H, W)
    assert flags == 0
    rows = np.flatnonzero(m.any(axis=1))
    assert rows[0] == 5 and rows[-1] == 30 and len(rows) == 26
    for y in rows:
        xs = np.flatnonzero(m[y])
        assert len(xs) == xs[-1] - xs[0] + 1, "row %d is not one solid run" % y
    for y, (first, last, count) in POLY_ROWS.items():
        xs = np.flatnonzero(m[y])
        assert (xs[0], xs[-1], len(xs)) == (first, last, count), y


BOWTIE_PICTURE = """
.....#........................#...
.....###....................###...
.....####..................####...
.....#####................#####...
.....#######............#######...
.....########..........########...
.....##########......##########...
.....###########....###########...
.....############..############...
.....##########################...
.....############..############...
.....###########....###########...
.....##########......##########...
.....########..........########...
.....#######............#######...
.....#####................#####...
.....####..................####...
.....###....................###...
.....#........................#...
""".split()     # rows 2 .. 20, columns 0 .. 33: two triangles that meet at columns 17-18 of row 11; the four vertices are single pixels


@pytest.mark.parametrize("impl", IMPLS)
def test_bowtie_picture(impl):
    m, _ = impl.poly_mask(BOWTIE, H, W)
    assert not m[:2].any() and not m[21:].any() and not m[:, 34:].any()
    got = ["".join("#" if v else "." for v in m[y, :34]) for y in range(2, 21)]
    assert got == BOWTIE_PICTURE
    assert list(np.flatnonzero(m[2])) == [5, 30] and list(np.flatnonzero(m[20])) == [5, 30]
    assert list(np.flatnonzero(m[10])) == list(range(5, 17)) + list(range(19, 31)) and m[11, 5:31].all()


def test_segments_closed_form_equals_walk():
    rng = np.random.default_rng(20240611)
    for _ in range(600):
        ax, ay, bx, by = (int(v) for v in rng.integers(-20, 61, 4))
        assert np.array_equal(emu.line_mask(ax, ay, bx, by, H, W), ref.line_mask(ax, ay, bx, by, H, W)), (ax, ay, bx, by)
    for seg in [(0, 0, 0, 0), (5, 5, 5, 30), (5, 30, 5, 5), (3, 7, 40, 7), (40, 7, 3, 7), (0, 0, 35, 35), (35, 0, 0, 35), (-20, 10, 60, 11),
                (10, -20, 11, 60), (47, 35, 47, 35)]:
        assert np.array_equal(emu.line_mask(*seg, H, W), ref.line_mask(*seg, H, W)), seg


def test_polygons_core_equals_restatement():
    rng = np.random.default_rng(7)
    for k in range(120):
        n = int(rng.integers(3, 41))
        pts = np.stack([rng.integers(-15, W + 15, n), rng.integers(-15, H + 15, n)], 1)
        if k % 4 == 0:     # vertices on the integer grid lines of few rows: crossings exactly on columns, horizontal edges
            pts[:, 1] = rng.choice([3, 9, 9, 20, 33], n)
        g, gf = emu.poly_mask(pts, H, W)
        w, wf = ref.poly_mask(pts, H, W)
        assert gf == wf == 0 and np.array_equal(g, w), pts.tolist()


def test_polygon_degenerate():
    cases = [[], [(7, 9)], [(7, 9), (30, 20)], [(-5, 9), (60, 9)], [(3, 12), (20, 12), (41, 12), (10, 12)],
             [(4, 4), (4, 4), (4, 4)], [(4, 4), (30, 4), (30, 4), (30, 25), (30, 25), (4, 4)], [(60, 60), (70, 80), (90, 61)]]
    for pts in cases:
        g, gf = emu.poly_mask(pts, H, W)
        w, wf = ref.poly_mask(pts, H, W)
        assert gf == wf == 0 and np.array_equal(g, w), pts
    assert not emu.poly_mask([], H, W)[0].any()
    assert emu.poly_mask([(7, 9)], H, W)[0].sum() == 1
    two = emu.poly_mask([(7, 9), (30, 20)], H, W)[0]
    assert np.array_equal(two, ref.line_mask(7, 9, 30, 20, H, W))     # only the edges


@pytest.mark.parametrize("impl", IMPLS)
def test_polygon_vertex_out_of_range_skips_the_fill(impl):
    for bad in (32768, -32768):
        m, flags = impl.poly_mask([(5, 5), (bad, 10), (20, 30)], H, W)
        assert flags == ref.POLY_RANGE and not m.any()
    m, flags = impl.poly_mask([(5, 5), (32767, 10), (20, 30)], H, W)
    assert flags == 0 and m.any()
    img = np.random.default_rng(1).integers(0, 256, (H, W, 3)).astype(np.uint8)
    lanes = [[(10, 10)], [], [], []]
    if impl is ref:
        out, flags = ref.compose(img, lanes, [(5, 5), (32768, 10), (20, 30)], True, None, stages=3)
    else:
        out, flags = emu.compose(img, lanes, [(5, 5), (32768, 10), (20, 30)], True, None, stages=3)
    assert flags == ref.POLY_RANGE
    assert np.array_equal(out, ref.draw_lanes(img, lanes))     # the discs are drawn, the fill is not


def test_discs_at_and_beyond_every_border():
    centres = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (-3, 10), (-4, 10), (-11, 10), (W + 2, 10), (W + 10, 10), (20, -3), (20, -11),
               (20, H + 3), (20, H + 10), (-2, -2), (W + 1, H + 1), (24, 18), (INT32_MIN, 5), (INT32_MAX, 5), (5, INT32_MIN), (5, INT32_MAX),
               (INT32_MIN, INT32_MIN), (INT32_MAX, INT32_MAX), (INT32_MAX - 2, 5), (INT32_MIN + 3, 5)]
    rng = np.random.default_rng(3)
    centres += [tuple(int(v) for v in rng.integers(-12, 60, 2)) for _ in range(100)]
    for cx, cy in centres:
        for r in (0, 1, 3, 4, 10):
            assert np.array_equal(emu.disc_mask(cx, cy, r, H, W), ref.disc_mask(cx, cy, r, H, W)), (cx, cy, r)
    assert emu.disc_mask(24, 18, 3, H, W).sum() == 29 and not emu.disc_mask(INT32_MAX, 5, 10, H, W).any()


def _random_frame(rng, h, w):
    lanes = [np.stack([rng.integers(-6, w + 6, k), rng.integers(-6, h + 6, k)], 1) for k in rng.integers(0, 12, 4)]
    n = int(rng.integers(3, 12))
    poly = np.stack([rng.integers(-10, w + 10, n), rng.integers(-10, h + 10, n)], 1)
    dist = np.stack([rng.integers(-6, w + 6, 5), rng.integers(-6, h + 6, 5)], 1)
    return lanes, poly, dist


def test_composition_core_equals_restatement():
    rng = np.random.default_rng(11)
    for k in range(40):
        img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        lanes, poly, dist = _random_frame(rng, H, W)
        off = int(rng.integers(0, 4))
        colour = ref.COLLISION_COLORS[k % 4] if k % 3 else ref.AREA_COLOR
        stages = int(rng.integers(0, 8)) if k % 2 else 7
        status = bool(k % 5)
        want, wf = ref.compose(img, lanes, poly, status, dist, off, colour, stages)
        got, gf = emu.compose(img, lanes, poly, status, dist, ref.lane_colors(off), colour, stages)
        assert gf == wf and np.array_equal(got, want), k
    # the bird view: discs of radius 10 written, not blended
    img = rng.integers(0, 256, (37, 131, 3)).astype(np.uint8)
    lanes = [np.stack([rng.integers(-12, 143, 9), rng.integers(-12, 49, 9)], 1) for _ in range(4)]
    want = ref.draw_lanes(img, lanes, ref.OFFSET_LEFT, radius=10, direct=True)
    got, _ = emu.compose(img, lanes, lane_bgr=ref.lane_colors(ref.OFFSET_LEFT), stages=1, radii=(10, 4), direct=True)
    assert np.array_equal(got, want)


def test_last_disc_wins_and_untouched_pixels_are_copies():
    img = np.random.default_rng(5).integers(0, 256, (H, W, 3)).astype(np.uint8)
    lanes = [[(20, 18)], [(22, 18)], [(21, 19)], [(21, 18), (40, 30)]]
    out = ref.draw_lanes(img, lanes)
    assert tuple(out[18, 21]) == tuple(ref.blend(np.array(ref.LANE_COLORS[3]), 0.3, img[18, 21]))
    assert tuple(out[18, 17]) == tuple(ref.blend(np.array(ref.LANE_COLORS[0]), 0.3, img[18, 17]))
    got, _ = emu.compose(img, lanes, stages=1)
    assert np.array_equal(got, out)
    far = np.ones((H, W), bool)
    for pts in lanes:
        for x, y in pts:
            far[max(y - 3, 0):y + 4, max(x - 3, 0):x + 4] = False
    assert np.array_equal(out[far], img[far])
