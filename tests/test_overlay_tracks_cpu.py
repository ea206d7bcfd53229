"""CPU: the overlay's trajectories stage (csrc/overlay_track_core.h: the per-track arithmetic of DrawTrackedOnFrame's show_traject part and
the pixel rules D10-D12).  Three layers: the golden -- the reference's own DrawTrackedOnFrame under a cv2 stub that records its calls
(tests/golden/track_draw.json.gz) -- pins the NumPy restatement's primitive lists; the restatement (tests/overlay_tracks_ref.py, the set
definitions by brute force) pins the host build of the header the kernels include (tests/hostemu/emu_overlay_tracks.cpp), every record
and every byte; and hand-derived known answers pin both."""
import gzip, json, os, sys

import numpy as np
import pytest

import overlay_ref as ref
import overlay_objects_ref as oref
import overlay_tracks_ref as tref
import emu_overlay_tracks_api as emu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
H, W = 45, 70
TRAJ, TRK = tref.TRAJECTORIES, oref.TRACKS


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(HERE, "golden", "track_draw.json.gz"), "rt") as f:
        return json.load(f)


def online(fr):
    """The rows DrawTrackedOnFrame walks: activated tracks of tracked_stracks, in list order."""
    return [t for t in fr["tracks"] if t["listed"] == "tracked" and t["is_activated"]]


def calls_of(marks):
    """Marks as the reference's cv2 calls (the colour of the lock-on rectangle saturated, as cv2 does with a negative scalar)."""
    out = []
    for m in marks:
        if m["kind"] == tref.CIRCLE:
            out.append(["circle", [m["x1"], m["y1"]], m["radius"], list(m["color"]), m["thickness"]])
        elif m["kind"] == tref.RECT:
            out.append(["rectangle", [m["x1"], m["y1"]], [m["x2"], m["y2"]], list(m["color"]), m["thickness"]])
        else:
            out.append(["arrowedLine", [m["x1"], m["y1"]], [m["x2"], m["y2"]], list(m["color"]), m["thickness"], m["tip"]])
    return out


def recorded(calls):
    """The recording without its text, the rectangle's colour saturated."""
    out = []
    for c in calls:
        if c[0] == "putText":
            continue
        if c[0] == "rectangle":
            c = [c[0], c[1], c[2], [max(0, v) for v in c[3]], c[4]]
        out.append(c)
    return out


def frame_marks(g, fr):
    table = [tuple(c) for _, c in g["names"]]
    marks = []
    for k, t in enumerate(online(fr)):
        marks += tref.track_marks(t["tlwh"], t["trajectory"], table[t["class_id"]], g["H"], g["W"], track=k)
    return marks


# ---------------------------------------------------------------------------------------------------------------- the golden
def test_golden_holds_every_required_case(golden):
    import make_golden_trackdraw as mk
    assert golden["required"] == mk.REQUIRED and len(golden["frames"]) >= 45 and (golden["H"], golden["W"]) == (240, 320)
    got = mk.coverage(golden["frames"])
    assert not [r for r in mk.REQUIRED if r not in got]
    lost = [t for fr in golden["frames"] for t in fr["tracks"] if t["listed"] == "lost"]
    assert lost, "a lost track: never drawn"
    ns = set()
    for fr in golden["frames"]:
        for c in fr["calls_traject"]:
            assert c[0] in ("circle", "rectangle", "arrowedLine", "putText")
        ns |= {c[0] for c in fr["calls_both"]}
    assert ns == {"circle", "rectangle", "arrowedLine", "putText", "addWeighted"}


def test_restatement_lists_the_reference_s_calls(golden):
    """Frame by frame the restatement's primitives ARE DrawTrackedOnFrame(frame, False)'s recorded circle, rectangle and arrowedLine calls:
    kind, integer coordinates, radius, thickness, colour, tip length, order.  DrawTrackedOnFrame(frame, True, True) records the same
    calls with plot_bbox's rectangle + addWeighted ahead of each track's."""
    n = dict(circle=0, rectangle=0, arrowedLine=0)
    for k, fr in enumerate(golden["frames"]):
        want = recorded(fr["calls_traject"])
        assert calls_of(frame_marks(golden, fr)) == want, k
        both = [c for c in fr["calls_both"] if c[0] != "putText"]
        kept = [c for i, c in enumerate(both) if c[0] != "addWeighted" and not (i + 1 < len(both) and both[i + 1][0] == "addWeighted")]
        assert recorded(kept) == want, k
        boxes = [both[i] for i in range(len(both) - 1) if both[i + 1][0] == "addWeighted"]
        drawn = [t for t in online(fr) if t["tlwh"][2] * t["tlwh"][3] > 10]
        assert [b[1] + b[2] for b in boxes] == [list(oref.track_box(t["tlwh"], golden["H"], golden["W"])) for t in drawn], k
        for c in want:
            n[c[0]] += 1
    assert n["circle"] > 1000 and n["rectangle"] >= 8 and n["arrowedLine"] >= 30 and n["arrowedLine"] % 3 == 0


@pytest.mark.parametrize("stages", [TRAJ, TRK | TRAJ])
def test_host_build_on_the_golden_frames(golden, stages):
    """The header's records and bytes against the restatement on the golden's frames (every fourth, and every frame for the records)."""
    table = [tuple(c) for _, c in golden["names"]]
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (golden["H"], golden["W"], 3), dtype=np.uint8)
    for k, fr in enumerate(golden["frames"]):
        rows = online(fr)
        args = ([t["tlwh"] for t in rows], [t["class_id"] for t in rows], [t["trajectory"] for t in rows])
        if k % 4 == 3 or k == len(golden["frames"]) - 1:
            want, wf, wm = tref.compose(img, stages=stages, trks=args[0], trk_cls=args[1], trajectories=args[2], trk_table=table)
            got, gf, gm = emu.tracks(img, *args, table, stages=stages)
            assert np.array_equal(got, want) and gf == wf == 0, k
        else:
            wm = frame_marks(golden, fr)
            _, gf, gm = emu.tracks(img, *args, table, stages=TRAJ)
        assert tref.device_marks_table(gm) == tref.marks_table(wm), k


def random_scene(rng, n_max=6):
    n = int(rng.integers(0, n_max + 1))
    trks, cls, trajs = [], [], []
    for k in range(n):
        x, y, w, h = rng.uniform(-5, 60), rng.uniform(-5, 35), rng.uniform(1, 30), rng.uniform(1, 25)
        trks.append([x, y, w, h])
        cls.append(int(rng.integers(0, 4)))           # class 3 has no colour: black
        m = int(rng.integers(0, 31))
        v = rng.uniform(-3, 3, 2)
        p = np.array([x, y]) - v * m
        tr = []
        for _ in range(m):
            p = p + v * (rng.random() > 0.2)          # some boxes repeat: shift < 2
            tr.append([p[0], p[1], p[0] + w, p[1] + h])
        trajs.append(tr)
    return trks, cls, trajs


def test_host_build_on_random_scenes():
    rng = np.random.default_rng(1)
    table = [(255, 0, 0), (5, 200, 7), (0, 0, 255)]
    kinds = set()
    for it in range(60):
        trks, cls, trajs = random_scene(rng)
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for st in (TRAJ, TRK | TRAJ):
            want, wf, wm = tref.compose(img, stages=st, trks=trks, trk_cls=cls, trk_table=table, trajectories=trajs)
            got, gf, gm = emu.tracks(img, trks, cls, trajs, table, stages=st)
            assert np.array_equal(got, want) and gf == wf, (it, st)
            assert tref.device_marks_table(gm) == tref.marks_table(wm), (it, st)
        kinds |= {m["kind"] for m in wm}
    assert kinds == {tref.CIRCLE, tref.RECT, tref.ARROW}


def test_rules_against_the_set_definitions_on_random_primitives():
    """D10 / D11: the rows' runs (what the mark kernel ORs) and the per-pixel test (what the sparse pass asks) both give the set."""
    rng = np.random.default_rng(2)
    for it in range(250):
        cx, cy, r, t = (int(v) for v in (rng.integers(-5, 75), rng.integers(-5, 50), rng.integers(0, 9), rng.integers(1, 7)))
        want = tref.circle_mask(cx, cy, r, t, H, W)
        assert np.array_equal(emu.circle_mask(cx, cy, r, t, H, W, 0), want) and np.array_equal(emu.circle_mask(cx, cy, r, t, H, W, 1), want), (cx, cy, r, t)
        ax, ay, bx, by = (int(v) for v in (rng.integers(-20, 90), rng.integers(-20, 65), rng.integers(-20, 90), rng.integers(-20, 65)))
        t = int(rng.integers(1, 7))
        want = tref.segment_mask(ax, ay, bx, by, t, H, W)
        for mode in (0, 1):
            got, skip = emu.segment_mask(ax, ay, bx, by, t, H, W, mode)
            assert np.array_equal(got, want) and not skip, (ax, ay, bx, by, t, mode)
    far = [(-29965, -19978, 30035, 20022, 2), (5, -32767, 60, 32767, 5), (-32767, 44, 32767, 0, 3)]          # long segments: the products stay exact
    for ax, ay, bx, by, t in far:
        want = tref.segment_mask(ax, ay, bx, by, t, H, W)
        for mode in (0, 1):
            got, skip = emu.segment_mask(ax, ay, bx, by, t, H, W, mode)
            assert np.array_equal(got, want) and not skip and want.any(), (ax, ay, bx, by, t, mode)


# ---------------------------------------------------------------------------------------------------------------- known answers
def rows_of(mask):
    return {int(y): [int(x) for x in np.flatnonzero(mask[y])] for y in range(mask.shape[0]) if mask[y].any()}


def test_the_radius_thickness_table():
    """int(sqrt(n) * 0.5) for n = 1 .. 30: sqrt(n) < 2 for n <= 3 -> 0; 2 <= sqrt(n) < 4 for n = 4 .. 15 -> 1 (12 of them); sqrt(n) >= 4 for
    n = 16 .. 30 -> 2 (15).  int(sqrt(n) * 1.2): 1.2, 1.70 -> 1 (n = 1, 2); 2.08 .. 2.94 -> 2 (n = 3 .. 6); 3.17 .. 3.98 -> 3 (n = 7 .. 11);
    4.16 .. 4.95 -> 4 (n = 12 .. 17); 5.09 .. 5.88 -> 5 (n = 18 .. 24); n = 25: 5.0 * 1.2 is exactly 6.0 in fp64 (the product
    5.99999999999999978 rounds up to 6.0, the nearer neighbour) -> 6 for n = 25 .. 30.  The device's table is NumPy's."""
    want = list(zip([0] * 3 + [1] * 12 + [2] * 15, [1] * 2 + [2] * 4 + [3] * 5 + [4] * 6 + [5] * 7 + [6] * 6))
    assert 5.0 * 1.2 == 6.0
    assert tref.mark_table() == want and emu.mark_table() == want
    assert emu.mark_table() == [(int(np.sqrt(float(i + 1)) * 0.5), int(np.sqrt(float(i + 1)) * 1.2)) for i in range(30)]


def test_thin_circle_of_radius_2():
    """The walk of r = 2 visits (2, 0) [err 1 > 0: dx -> 1] and (1, 1) [err 1 > 0: dx -> 0, ends]: reflections (+-2, 0), (0, +-2), (+-1, +-1) -- a
    diamond of 8 pixels, the centre empty."""
    want = {3: [10], 4: [9, 11], 5: [8, 12], 6: [9, 11], 7: [10]}
    for m in (tref.circle_mask(10, 5, 2, 1, H, W), emu.circle_mask(10, 5, 2, 1, H, W, 0), emu.circle_mask(10, 5, 2, 1, H, W, 1)):
        assert rows_of(m) == want


def test_radius_0_thickness_2_is_a_plus_sign():
    """r = 0: the outline is the centre pixel; t = 2: R = 1, and the D2 disc of radius 1 has half-widths [1, 0] (the walk visits (1, 0) only)."""
    want = {4: [10], 5: [9, 10, 11], 6: [10]}
    for m in (tref.circle_mask(10, 5, 0, 2, H, W), emu.circle_mask(10, 5, 0, 2, H, W, 0), emu.circle_mask(10, 5, 0, 2, H, W, 1)):
        assert rows_of(m) == want
    assert rows_of(emu.circle_mask(10, 5, 0, 1, H, W)) == {5: [10]}                       # r = 0, t = 1: one pixel
    assert rows_of(emu.circle_mask(0, 0, 0, 2, H, W)) == {0: [0, 1], 1: [0]}              # clipped at the corner


def test_a_ring_with_a_hole():
    """r = 6 walks (6, 0), (5, 1), (5, 2), (5, 3), (4, 4); t = 2 puts a plus sign on each reflection.  The centre's row holds two runs: the
    plus signs on (+-6, 0) give +-5 .. +-7, the ones on (+-5, +-1) reach (+-5, 0) again, nothing comes nearer: columns -7 .. -5 and 5 .. 7.
    The top row -7 is the upper arm of (0, -6) alone; row -6 is its bar -1 .. 1 and the upper arms of (+-1, -5), (+-2, -5), (+-3, -5): -3 .. 3."""
    cx, cy = 30, 20
    for m in (tref.circle_mask(cx, cy, 6, 2, H, W), emu.circle_mask(cx, cy, 6, 2, H, W, 0), emu.circle_mask(cx, cy, 6, 2, H, W, 1)):
        r = rows_of(m)
        assert r[cy] == [cx - 7, cx - 6, cx - 5, cx + 5, cx + 6, cx + 7]
        assert r[cy - 7] == [cx] and r[cy - 6] == list(range(cx - 3, cx + 4)) and r[cy + 7] == [cx] and min(r) == cy - 7 and max(r) == cy + 7
        sub = m[cy - 7:cy + 8, cx - 7:cx + 8]
        assert np.array_equal(sub, sub[::-1]) and np.array_equal(sub, sub[:, ::-1]) and np.array_equal(sub, sub.T)


@pytest.mark.parametrize("t", [2, 3, 5])
def test_axis_aligned_segments_are_D6(t):
    """PROPERTY: for a horizontal, a vertical and a zero-length segment D11 gives D6's pixels exactly (d = (L, 0): 0 <= v.x L <= L^2 is the
    segment's columns, |v.y L| <= floor(sqrt(R^2 L^2)) = R L is -R .. R across)."""
    for ax, ay, bx, by in ((10, 8, 50, 8), (50, 8, 10, 8), (33, 5, 33, 30), (33, 30, 33, 5), (20, 20, 20, 20), (-6, 3, 12, 3), (64, 40, 64, 60), (31, 0, 32, 0)):
        d6 = oref.thick_segment_mask(ax, ay, bx, by, t, H, W)
        assert np.array_equal(tref.segment_mask(ax, ay, bx, by, t, H, W), d6), (ax, ay, bx, by)
        for mode in (0, 1):
            assert np.array_equal(emu.segment_mask(ax, ay, bx, by, t, H, W, mode)[0], d6), (ax, ay, bx, by, mode)


def test_a_45_degree_segment_row_by_row():
    """a = (2, 2), b = (5, 5), t = 2: R = 1, d = (3, 3), d.d = 18, Tq = floor(sqrt(18)) = 4.  Body: 0 <= 3 (vx + vy) <= 18 and 3 |vx - vy| <= 4, i.e.
    0 <= vx + vy <= 6 and |vx - vy| <= 1; plus signs on (2, 2) and (5, 5).
      y = 1 (vy = -1): vx >= 1 and vx <= 0: no body; the plus of a -> {2}
      y = 2 (vy = 0):  vx in 0 .. 1 -> x = 2, 3; the plus's bar 1 .. 3 -> {1, 2, 3}
      y = 3 (vy = 1):  vx in 0 .. 2 -> {2, 3, 4} (the plus's lower arm is x = 2)
      y = 4 (vy = 2):  vx in 1 .. 3 -> {3, 4, 5} (the upper arm of b is x = 5)
      y = 5 (vy = 3):  vx <= 3 and vx in 2 .. 4 -> x = 4, 5; the bar of b 4 .. 6 -> {4, 5, 6}
      y = 6 (vy = 4):  vx <= 2 and vx >= 3: no body; the plus of b -> {5}"""
    want = {1: [2], 2: [1, 2, 3], 3: [2, 3, 4], 4: [3, 4, 5], 5: [4, 5, 6], 6: [5]}
    assert emu.segment_tq(2, 2, 5, 5, 2) == 4
    for m in (tref.segment_mask(2, 2, 5, 5, 2, H, W), emu.segment_mask(2, 2, 5, 5, 2, H, W, 0)[0], emu.segment_mask(5, 5, 2, 2, 2, H, W, 1)[0]):
        assert rows_of(m) == want


def test_a_1_in_3_segment_row_by_row():
    """a = (1, 1), b = (7, 3), t = 2: R = 1, d = (6, 2), d.d = 40, Tq = floor(sqrt(40)) = 6.  Body: 0 <= 6 vx + 2 vy <= 40 and |2 vx - 6 vy| <= 6, i.e.
    |vx - 3 vy| <= 3.
      y = 0 (vy = -1): 6 vx >= 2 -> vx >= 1, |vx + 3| <= 3 -> vx <= 0: no body; the plus of a -> {1}
      y = 1 (vy = 0):  vx in 0 .. 6 and |vx| <= 3 -> x = 1 .. 4; the bar of a 0 .. 2 -> {0 .. 4}
      y = 2 (vy = 1):  6 vx + 2 in 0 .. 40 -> vx in 0 .. 6, |vx - 3| <= 3 -> 0 .. 6 -> x = 1 .. 7 (the arms of a and b are x = 1 and x = 7)
      y = 3 (vy = 2):  6 vx + 4 <= 40 -> vx <= 6, |vx - 6| <= 3 -> vx in 3 .. 6 -> x = 4 .. 7; the bar of b 6 .. 8 -> {4 .. 8}
      y = 4 (vy = 3):  vx <= 5 and vx >= 6: no body; the plus of b -> {7}"""
    want = {0: [1], 1: [0, 1, 2, 3, 4], 2: [1, 2, 3, 4, 5, 6, 7], 3: [4, 5, 6, 7, 8], 4: [7]}
    assert emu.segment_tq(1, 1, 7, 3, 2) == 6
    for m in (tref.segment_mask(1, 1, 7, 3, 2, H, W), emu.segment_mask(1, 1, 7, 3, 2, H, W, 0)[0], emu.segment_mask(1, 1, 7, 3, 2, H, W, 1)[0]):
        assert rows_of(m) == want


def test_arrow_tips():
    """(0, 0) -> (10, 0), tip 0.3: u = (-10, 0), k = 0.3 * 0.70710678 = 0.21213; qa = (rint(10 + k (-10 - 0)), rint(0 + k (-10 + 0))) =
    (rint(7.879), rint(-2.121)) = (8, -2); qb = (rint(10 + k (-10 + 0)), rint(0 + k (0 + 10))) = (8, 2) -- OpenCV's p2 + 3 (cos, sin)(pi +- pi / 4)."""
    assert emu.arrow_tips((0, 0), (10, 0), 0.3) == ((8, -2), (8, 2)) == tref.arrow_tips((0, 0), (10, 0), 0.3)
    assert emu.arrow_tips((0, 0), (0, 0), 0.3) == ((0, 0), (0, 0))
    rng = np.random.default_rng(3)
    for _ in range(200):
        p1, p2 = rng.integers(-3000, 3000, 2), rng.integers(-3000, 3000, 2)
        for tip in (0.3, 0.3 - 0.1):
            qa, qb = emu.arrow_tips(p1, p2, tip)
            assert (qa, qb) == tref.arrow_tips(p1, p2, tip)
            u = (p1 - p2).astype(np.float64)                                             # against the trigonometric form, within rounding
            ang, length = np.arctan2(u[1], u[0]), tip * np.hypot(u[0], u[1])
            assert abs(qa[0] - (p2[0] + length * np.cos(ang + np.pi / 4))) <= 0.5 + 1e-6 and abs(qa[1] - (p2[1] + length * np.sin(ang + np.pi / 4))) <= 0.5 + 1e-6
            assert abs(qb[0] - (p2[0] + length * np.cos(ang - np.pi / 4))) <= 0.5 + 1e-6 and abs(qb[1] - (p2[1] + length * np.sin(ang - np.pi / 4))) <= 0.5 + 1e-6


def test_tq_is_the_exact_integer_square_root():
    """d = (0, 9): d.d = 81, a perfect square -> Tq(t = 2) = 9, Tq(t = 5) = floor(sqrt(9 * 81)) = 27.  d = (8, 4): d.d = 80, one below -> 8; t = 5:
    floor(sqrt(720)) = 26 (26^2 = 676, 27^2 = 729)."""
    assert emu.segment_tq(0, 0, 0, 9, 2) == 9 and emu.segment_tq(0, 0, 0, 9, 5) == 27
    assert emu.segment_tq(0, 0, 8, 4, 2) == 8 and emu.segment_tq(0, 0, 8, 4, 5) == 26
    for v in (0, 1, 2, 3, 4, 10 ** 12, 10 ** 12 - 1, (1 << 31) ** 2 - 1, (1 << 31) ** 2, 4096 * 2 * 65534 ** 2):
        s = emu.isqrt(v)
        assert s * s <= v < (s + 1) * (s + 1), v
    assert emu.isqrt(10 ** 12) == 10 ** 6 and emu.isqrt(10 ** 12 - 1) == 10 ** 6 - 1


def test_the_range_flag():
    """An endpoint at 32767 is drawn, one at 32768 skips the primitive; a track whose centre lies there sets ADAS_OVERLAY_TRACK_RANGE and
    keeps its circles."""
    m, skip = emu.segment_mask(0, 5, 32767, 5, 2, H, W)
    assert not skip and rows_of(m)[5] == list(range(W)) and sorted(rows_of(m)) == [4, 5, 6]
    for far in ((0, 5, 32768, 5), (0, 5, 10, -32768), (-32768, 5, 10, 5), (0, 32768, 10, 5)):
        m, skip = emu.segment_mask(*far, 2, H, W)
        assert skip and not m.any()
        assert emu.segment_tq(*far, 2) == -1
    traj = [[12.0 + 3 * i, 12.0, 22.0 + 3 * i, 30.0] for i in range(8)]
    img = np.zeros((H, W, 3), np.uint8)
    for tl in ([40000.0, 10.0, 10.0, 18.0], [10.0, 10.0, 10.0, 18.0]):
        want, wf, wm = tref.compose(img, stages=TRAJ, trks=[tl], trk_cls=[0], trk_table=[(9, 8, 7)], trajectories=[traj])
        got, gf, gm = emu.tracks(img, [tl], [0], [traj], [(9, 8, 7)], stages=TRAJ)
        assert np.array_equal(got, want) and gf == wf == (tref.TRACK_RANGE if tl[0] > 32767 else 0)
        assert tref.device_marks_table(gm) == tref.marks_table(wm) and [m["kind"] for m in wm] == [tref.CIRCLE] * 8 + [tref.ARROW] * 3
        assert [int(m["skipped"]) for m in gm[8:]] == ([7, 7, 7] if tl[0] > 32767 else [0, 0, 0])
        assert (got == 9).any()


def test_medians():
    """Odd: [3, 1, 2] -> 2.  Even: [4, 1, 3, 2] -> (2 + 3) / 2 = 2.5.  The zero vectors count: [0, 0, 5, 7] -> (0 + 5) / 2 = 2.5."""
    assert emu.median([3.0, 1.0, 2.0]) == 2.0 == float(np.median([3.0, 1.0, 2.0]))
    assert emu.median([4.0, 1.0, 3.0, 2.0]) == 2.5 == float(np.median([4.0, 1.0, 3.0, 2.0]))
    assert emu.median([0.0, 0.0, 5.0, 7.0]) == 2.5
    rng = np.random.default_rng(4)
    for n in range(1, 30):
        v = rng.normal(0, 3, n) * (rng.random(n) > 0.3)
        assert emu.median(v) == float(np.median(v)), n
