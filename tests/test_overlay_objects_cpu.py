"""CPU: the object layer of the overlay, rules D6-D9 of csrc/overlay_core.h.  The NumPy restatement (tests/overlay_objects_ref.py, from the
stepping definitions) and the host build of the header's closed forms (tests/hostemu/emu_overlay_objects.cpp) must agree on every byte,
and both must give the known answers below, each derived by hand."""
import numpy as np
import pytest

import overlay_ref as ref
import overlay_objects_ref as oref
import emu_overlay_objects_api as emu

H, W = 45, 70
IMPLS = [oref, emu]


def rows_of(m):
    """{row: (first column, last column, pixels)} of a mask."""
    return {int(y): (int(np.flatnonzero(m[y])[0]), int(np.flatnonzero(m[y])[-1]), int(m[y].sum())) for y in np.flatnonzero(m.any(axis=1))}


def test_the_two_radii_used_by_default():
    """R = (t + 1) >> 1: 3 for cornerRect's t = 5, 1 for plot_bbox's thickness 2.  The midpoint walk gives hw(3) = [3, 2, 2, 0] (the disc of the
    lane points) and hw(1) = [1, 0]: from (dx, dy) = (1, 0) the walk records hw[0] = 1, hw[1] = 0 and stops -- a plus sign."""
    assert ref.disc_halfwidths(3) == [3, 2, 2, 0] and ref.disc_halfwidths(1) == [1, 0]


@pytest.mark.parametrize("impl", IMPLS)
def test_thick_segment_t5_known_answer(impl):
    """(10,10)-(14,10), t = 5, R = 3, hw = [3, 2, 2, 0].  Body: columns 10..14 on rows 7..13.  Caps: discs at (10,10) and (14,10).  Row 10 grows
    by hw[0] = 3 on either side: 7..17; rows 9, 11 and 8, 12 by 2: 8..16; rows 7, 13 by 0: 10..14.  11 + 4 * 9 + 2 * 5 = 57 pixels."""
    m = impl.thick_segment_mask(10, 10, 14, 10, 5, H, W)
    assert rows_of(m) == {7: (10, 14, 5), 8: (8, 16, 9), 9: (8, 16, 9), 10: (7, 17, 11), 11: (8, 16, 9), 12: (8, 16, 9), 13: (10, 14, 5)}
    assert np.array_equal(m, impl.thick_segment_mask(14, 10, 10, 10, 5, H, W))                      # the direction does not matter


@pytest.mark.parametrize("impl", IMPLS)
def test_thick_segment_t2_known_answer(impl):
    """(5,3)-(5,6), t = 2, R = 1, hw = [1, 0].  Body: columns 4..6 on rows 3..6.  The caps add their last rows, one pixel wide (hw[1] = 0), on
    rows 2 and 7.  4 * 3 + 2 = 14 pixels."""
    m = impl.thick_segment_mask(5, 3, 5, 6, 2, H, W)
    assert rows_of(m) == {2: (5, 5, 1), 3: (4, 6, 3), 4: (4, 6, 3), 5: (4, 6, 3), 6: (4, 6, 3), 7: (5, 5, 1)}


@pytest.mark.parametrize("impl", IMPLS)
def test_zero_length_segment_is_a_disc(impl):
    for t, r in ((5, 3), (2, 1), (8, 4)):
        assert np.array_equal(impl.thick_segment_mask(20, 18, 20, 18, t, H, W), ref.disc_mask(20, 18, r, H, W))
    assert impl.thick_segment_mask(20, 18, 20, 18, 1, H, W).sum() == 1


@pytest.mark.parametrize("impl", IMPLS)
def test_rectangle_t2_known_answer(impl):
    """(4,4)-(9,8), t = 2, R = 1.  The horizontal edges are rows 3..5 and 7..9: their middle rows (4, 8) run 3..10, the outer and inner rows
    4..9.  The vertical edges are columns 3..5 and 8..10 on rows 4..8, and one pixel more (column 4, column 9) on rows 3 and 9.  So rows 3
    and 9 hold 4..9; rows 4, 5, 7, 8 hold 3..10; row 6 holds 3..5 and 8..10: a ring three pixels thick with its four corners cut.  50 pixels."""
    m = impl.rect_mask(4, 4, 9, 8, 2, H, W)
    want = np.zeros((H, W), bool)
    want[3, 4:10] = want[9, 4:10] = True
    for y in (4, 5, 7, 8):
        want[y, 3:11] = True
    want[6, 3:6] = want[6, 8:11] = True
    assert np.array_equal(m, want) and m.sum() == 50
    thin = impl.rect_mask(4, 4, 9, 8, 1, H, W)                                                       # t == 1: the box's border, 2 * 6 + 2 * 3
    assert thin.sum() == 18 and thin[4, 4:10].all() and thin[8, 4:10].all() and thin[4:9, 4].all() and thin[4:9, 9].all()


@pytest.mark.parametrize("impl", IMPLS)
def test_corner_rect_of_a_3x3_box_known_answer(impl):
    """(10,10,12,12): min(2, 2) * 0.2 = 0.4 -> int 0 -> l = 1.  The horizontal arms lie on rows 10 and 12, between them columns 10..12; with
    R = 3 a row at distance j holds 10 - hw[j] .. 12 + hw[j]: 7..15, 8..14, 8..14, 10..12.  The vertical arms lie on columns 10 and 12, rows
    10..12: their bodies hold 7..13 and 9..15 there, their caps 8..12 / 10..14 at distance 1 and 2 and one pixel at distance 3.  Row by row the
    union is 10..12 (rows 7, 15), 8..14 (rows 8, 9, 13, 14) and 7..15 (rows 10..12): 2 * 3 + 4 * 7 + 3 * 9 = 61 pixels; the thin outline is inside."""
    m = impl.corner_rect_mask(10, 10, 12, 12, H, W)
    assert rows_of(m) == {7: (10, 12, 3), 8: (8, 14, 7), 9: (8, 14, 7), 10: (7, 15, 9), 11: (7, 15, 9), 12: (7, 15, 9), 13: (8, 14, 7),
                          14: (8, 14, 7), 15: (10, 12, 3)}
    assert m.sum() == 61


TINTS = [
    (0, 0, 1),          # 0 + 0 + 1
    (255, 255, 255),    # 255 * 0.6f = 153.000006 -> 153 in fp32, 255 * 0.4f -> 102; 255 + 1 = 256, saturated
    (100, 200, 141),    # 60.0000038 + 80 = 140.000004 -> 140 in fp32; + 1
    (10, 20, 15),       # 10 * 0.6f lies exactly between 6 and 6 + 2^-21: to even, 6; 8; 14 + 1
    (255, 0, 154),      # 153 + 0 + 1
    (0, 255, 103),      # 0 + 102 + 1
    (254, 255, 255),    # 152.4 + 102 + 1 = 255.4 -> 255 by rounding, not by saturation
]


@pytest.mark.parametrize("impl", IMPLS)
def test_tint_known_answers(impl):
    for a, b, want in TINTS:
        assert int(impl.tint(a, b)) == want, (a, b)


def test_tint_core_equals_restatement_everywhere_and_its_association_is_part_of_the_definition():
    """Over all 65536 (a, b) pairs the core is the restatement; an fp64 evaluation rint(a * 0.6 + b * 0.4 + 1.0) and a form that fuses
    a * af into the first add differ from D8 in the numbers of pairs recorded below: none.  Unlike D1 (3 a + 7 b over 10 is often a half),
    (3 a + 2 b) / 5 + 1 is never nearer than 0.1 to a half, and no rounding error here comes close to that."""
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    want = oref.tint(a, b).astype(np.int64)
    got = np.array([[emu.tint(i, j) for j in range(256)] for i in range(256)])
    assert np.array_equal(got, want)
    f64 = np.clip(np.rint(a * 0.6 + b * 0.4 + 1.0), 0, 255)
    pb = (b.astype(np.float32) * np.float32(0.4)).astype(np.float64)
    fma = (a.astype(np.float64) * np.float64(np.float32(0.6)) + pb).astype(np.float32)               # one rounding for a * af + pb
    fma = np.clip(np.rint((fma + np.float32(1.0)).astype(np.float32)), 0, 255)
    assert (int((f64 != want).sum()), int((fma != want).sum())) == (N_F64, N_FMA)


N_F64, N_FMA = 0, 0


def test_thick_segments_closed_form_equals_walk():
    rng = np.random.default_rng(20250101)
    for k in range(300):
        ax, ay, L = (int(v) for v in rng.integers(-12, 80, 3))
        t = int(rng.integers(1, 12))
        L = L % 30 * (1 if k % 3 else -1)
        bx, by = (ax + L, ay) if k % 2 else (ax, ay + L)
        assert np.array_equal(emu.thick_segment_mask(ax, ay, bx, by, t, H, W), oref.thick_segment_mask(ax, ay, bx, by, t, H, W)), (ax, ay, bx, by, t)
    # as far out as int32 goes: the restatement's loops are clipped to the image for t >= 2 (t == 1 walks the line)
    for args in ((2 ** 31 - 1, 5, 2 ** 31 - 1, 9), (-2 ** 31, 5, 2 ** 31 - 1, 5), (5, -2 ** 31, 5, 2 ** 31 - 1), (-2 ** 31, -2 ** 31, -2 ** 31, 3),
                 (-2 ** 31, 43, 3, 43), (68, 2 ** 31 - 1, 68, 40)):
        for t in (2, 5):
            assert np.array_equal(emu.thick_segment_mask(*args, t, H, W), oref.thick_segment_mask(*args, t, H, W)), (args, t)


def test_outlines_and_corner_rects_closed_form_equals_walk():
    rng = np.random.default_rng(3)
    boxes = [(10, 10, 12, 12), (5, 5, 5, 5), (20, 8, 23, 40), (-6, -4, 30, 20), (50, 30, W + 9, H + 5), (-40, -40, -20, -20), (W + 20, 3, W + 40, 9),
             (30, 20, 10, 5), (29, 3, 34, 30), (60, 10, 66, 12), (0, 0, W - 1, H - 1), (-2 ** 31, 5, 2 ** 31 - 1, 30), (7, -2 ** 31, 40, 2 ** 31 - 1), (3, 3, 2 ** 31 - 1, 2 ** 31 - 1)]
    boxes += [tuple(int(v) for v in rng.integers(-15, 85, 4)) for _ in range(60)]
    for b in boxes:
        big = max(abs(v) for v in b) > 10 ** 6           # the thin outline's restatement walks the line: thick ones only
        for t in (2, 5) if big else (1, 2, 5):
            assert np.array_equal(emu.rect_mask(*b, t, H, W), oref.rect_mask(*b, t, H, W)), (b, t)
        if not big:
            assert np.array_equal(emu.corner_rect_mask(*b, H, W), oref.corner_rect_mask(*b, H, W)), b
        assert np.array_equal(emu.corner_rect_mask(*b, H, W, 3, 2), oref.corner_rect_mask(*b, H, W, 3, 2)), b
    m = emu.corner_rect_mask(3, 3, 2 ** 31 - 1, 2 ** 31 - 1, H, W)     # arms of 0.2 * (2^31 - 4) pixels from (3, 3): across the whole image
    assert m[1:6, 3:].all() and m[3:, 1:6].all() and m[3].all() and m[:, 3].all() and not m[7:, 7:].any()


TABLE = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (200, 100, 50)]


def scene(rng, n_det, n_trk):
    dets = np.stack([rng.integers(-10, W + 5, n_det), rng.integers(-10, H + 5, n_det), rng.integers(-5, W + 12, n_det), rng.integers(-5, H + 12, n_det)], 1)
    trks = np.stack([rng.uniform(-20, W, n_trk), rng.uniform(-20, H, n_trk), rng.uniform(-2, 40, n_trk), rng.uniform(-2, 30, n_trk)], 1)
    return dets, rng.integers(-1, 6, n_det), trks, rng.integers(-1, 6, n_trk)


def test_fold_core_equals_restatement():
    """Random scenes, boxes overlapping in every way, classes inside and outside the table, tracks failing the gate, every stage set."""
    rng = np.random.default_rng(17)
    for k in range(30):
        img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        dets, dc, trks, tc = scene(rng, int(rng.integers(0, 7)), int(rng.integers(0, 7)))
        for stages in (16, 32, 48):
            want, _ = oref.compose(img, stages=stages, dets=dets, det_cls=dc, det_table=TABLE, trks=trks, trk_cls=tc, trk_table=TABLE[::-1])
            got = emu.objects(img, dets, dc, TABLE, trks, tc, TABLE[::-1], stages=stages)
            assert np.array_equal(got, want), (k, stages, np.argwhere(got != want)[:5])
        thick = (2, 3, 4)
        want, _ = oref.compose(img, stages=48, dets=dets, det_cls=dc, trks=trks, trk_cls=tc, trk_table=TABLE, min_box_area=200.0, thickness=thick)
        got = emu.objects(img, dets, dc, None, trks, tc, TABLE, min_box_area=200.0, thickness=thick)
        assert np.array_equal(got, want), k


def test_the_fold_is_sequential():
    """Two overlapping detections: the later one's colour stays.  Two overlapping tracks: the second outline is written over the first tint,
    and the overlap is tinted twice, D8(D8(v, c0), c1) -- which is not D8(D8(v, c1), c0)."""
    img = np.full((H, W, 3), 90, np.uint8)
    dets = [(10, 10, 40, 30), (20, 15, 50, 35)]
    a = oref.draw_detections(img, dets, [0, 1], TABLE)
    b = oref.draw_detections(img, dets[::-1], [1, 0], TABLE)
    assert tuple(a[15, 40]) == TABLE[1] and tuple(b[15, 40]) == TABLE[0]                             # the two outlines cross at (40, 15)
    assert np.array_equal(emu.objects(img, dets, [0, 1], TABLE, stages=16), a) and np.array_equal(emu.objects(img, dets[::-1], [1, 0], TABLE, stages=16), b)
    trks = [(10.9, 10.2, 30.7, 20.5), (20.1, 15.0, 30.0, 20.0)]
    c = oref.draw_tracks(img, trks, [0, 3], TABLE)
    d = oref.draw_tracks(img, trks[::-1], [3, 0], TABLE)
    inner = (28, 33)                                                                                 # row, column inside both regions, on no outline
    for ch in range(3):
        assert c[inner][ch] == oref.tint(oref.tint(90, TABLE[0][ch]), TABLE[3][ch]) and d[inner][ch] == oref.tint(oref.tint(90, TABLE[3][ch]), TABLE[0][ch])
    assert tuple(c[inner]) != tuple(d[inner])
    assert tuple(c[15, 25]) == tuple(oref.tint(np.array(TABLE[3]), np.array(TABLE[3])))              # track 1's outline over track 0's tint, tinted
    assert np.array_equal(emu.objects(img, None, None, None, trks, [0, 3], TABLE, stages=32), c)
    assert np.array_equal(emu.objects(img, None, None, None, trks[::-1], [3, 0], TABLE, stages=32), d)


def test_track_box_truncation_gate_and_empty_region():
    """astype(int) truncates toward zero (-0.9 -> 0, -1.5 -> -1); the gate reads the untruncated product; a region with x2 <= x1 tints nothing,
    but its outline is still drawn where it meets the image."""
    assert oref.track_box((-0.9, -1.5, 10.9, 8.2), H, W) == (0, 0, 10, 7)
    assert oref.track_box((60.0, 40.0, 30.0, 30.0), H, W) == (60, 40, W, H)
    assert oref.track_box((5.0, 5.0, 3.3, 3.0), H, W) is None and oref.track_box((5.0, 5.0, 3.4, 3.0), H, W) is not None      # 9.9 and 10.2
    assert oref.track_box((5.0, 5.0, float("nan"), 3.0), H, W) is None
    img = np.random.default_rng(2).integers(0, 256, (H, W, 3)).astype(np.uint8)
    for tlwh in ((-30.0, 10.0, 29.5, 12.0), (W + 3.0, 10.0, 8.0, 8.0), (20.0, -25.0, 10.0, 24.5), (20.0, 10.0, 0.4, 90.0)):
        x1, y1, x2, y2 = oref.track_box(tlwh, H, W)
        assert x2 <= x1 or y2 <= y1
        want = oref.draw_tracks(img, [tlwh], [1], TABLE)
        assert np.array_equal(want != img, np.repeat(oref.rect_mask(x1, y1, x2, y2, 2, H, W)[:, :, None], 3, 2) & (want != img))
        assert np.array_equal(emu.objects(img, None, None, None, [tlwh], [1], TABLE, stages=32), want)


def test_objects_sit_between_the_area_blend_and_the_distance_discs():
    img = np.random.default_rng(8).integers(0, 256, (H, W, 3)).astype(np.uint8)
    poly = [(10, 5), (8, 12), (3, 20), (2, 30), (40, 30), (35, 21), (28, 5)]
    full, _ = oref.compose(img, [[(20, 18)], [], [], []], poly, True, [(22, 20)], stages=7 | 48, dets=[(15, 15, 30, 25)], det_cls=[2], det_table=TABLE,
                           trks=[(12.0, 12.0, 20.0, 15.0)], trk_cls=[1], trk_table=TABLE)
    after_area, _ = ref.compose(img, [[(20, 18)], [], [], []], poly, True, None, stages=3)
    assert tuple(full[20, 22]) == ref.DIST_COLOR                                                     # the disc is over the box
    assert tuple(full[22, 15]) == tuple(oref.tint(np.array(TABLE[2]), np.array(TABLE[1])))           # a detection's outline inside a track's region
    for ch in range(3):
        assert full[14, 20][ch] == oref.tint(after_area[14, 20][ch], TABLE[1][ch])                   # a blended pixel under a tint
    assert np.array_equal(ref.draw_distance(emu.objects(after_area, [(15, 15, 30, 25)], [2], TABLE, [(12.0, 12.0, 20.0, 15.0)], [1], TABLE), [(22, 20)]), full)
