"""CPU: csrc/analysis_core.h (distance, collision point and the FCWS / LDWS / LKAS state machine as the device runs them per stream; host
build tests/hostemu/emu_analysis.cpp) against the reference's own traces (tests/golden/analysis.json.gz) and the project's host
restatement (analysis.SingleCamDistanceMeasure / point_in_polygon / TaskConditions / PerspectiveTransformation)."""
import gzip, importlib, itertools, json, os, subprocess, sys

import numpy as np
import pytest

from conftest import load_pkg, GOLDEN, ROOT

load_pkg()
A = importlib.import_module("adas_amd.analysis")
import emu_analysis_api as E
import emu_birdview_api as EB

G = json.load(gzip.open(os.path.join(GOLDEN, "analysis.json.gz"), "rt"))
LABELS = ["person", "bicycle", "car", "motorbike", "bus", "truck"]
REF = [A.SingleCamDistanceMeasure.RefSizeDict[l][0] for l in LABELS]


class Box:
    """What updateDistance reads of a RectInfo: tolist() and label."""

    def __init__(self, xyxy, label):
        self.xyxy, self.label = [int(v) for v in xyxy], label

    def tolist(self):
        return list(self.xyxy)


def host_frame(boxes, poly):
    dm = A.SingleCamDistanceMeasure()
    dm.updateDistance(boxes)
    return dm.distance_points, dm.calcCollisionPoint(np.asarray(poly, np.int64).reshape(-1, 2))


def emu_frame(boxes, poly, ref=REF, labels=LABELS):
    e = E.AnalysisEmu(ref)
    fr, xy, d = e.frame([b.xyxy for b in boxes], [labels.index(b.label) if b.label in labels else len(labels) for b in boxes], poly, True, 0, 0.0, 0.0)
    pts = [[int(x), int(y), float(v)] for (x, y), v in zip(xy, d)]
    col = [int(fr["collision_x"]), int(fr["collision_y"]), float(fr["collision_d"])] if fr["has_collision"] else None
    return pts, col, fr


# ------------------------------------------------------------------------------------------------ 1. distance golden
def test_distance_golden_points_and_collision():
    g = G["distance"]
    D = importlib.import_module("adas_amd.detectors")
    boxes = [Box(D.RectInfo(r["x"], r["y"], r["w"], r["h"], r["conf"], r["label"]).tolist(), r["label"]) for r in g["rects"]]
    pts, col, fr = emu_frame(boxes, g["poly"])
    assert len(pts) == len(g["points"]) > 10
    for got, want in zip(pts, g["points"]):
        assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]          # the distance bit for bit
    assert col == g["collision"] and pts[int(fr["collision_index"])] == col
    pts0, col0, _ = emu_frame(boxes, [])
    assert pts0 == pts and col0 is None and g["collision_empty"] is None
    assert emu_frame([], g["poly"])[:2] == ([], None)


# ------------------------------------------------------------------------------------------------ 2. state-machine golden
def run_trace(inputs):
    e = E.AnalysisEmu()
    return e, [e.step(r) for r in inputs]


def test_state_machine_golden_every_frame_and_field():
    g = G["state_machine"]
    e, frames = run_trace(E.golden_inputs(g["inputs"]))
    assert len(frames) == len(g["trace"]) == 400
    check = True                                   # the reference's first CheckStatus(): True with "Default" (the reset state)
    for t, (fr, want) in enumerate(zip(frames, g["trace"])):
        assert want["error"] is None
        got = E.frame_fields(fr)
        got["check"] = check                       # the golden calls CheckStatus inside frame t; the device calls it at the end of t - 1
        for k, v in got.items():
            assert v == want[k], (t, k, v, want[k])
        check = bool(fr["check"])
        assert check or fr["request"] == 0        # a true check can carry None: toggle_status None replaces transform_status
    assert int(e.state["n_nonfinite"][0]) == 0
    assert {E.MODES[int(f["request"])] for f in frames} == {None, "Default", "Top"}        # the golden drive never toggles "Bottom"


def test_nonfinite_curvature_is_a_frame_without_a_curve_estimate():
    a, b = E.AnalysisEmu(), E.AnalysisEmu()
    for t in range(30):
        bad = t in (12, 20)
        fa = a.step(E.make_input(None, True, 0.1, "L", float("nan") if t == 12 else float("inf") if t == 20 else 300.0))
        fb = b.step(E.make_input(None, True, 0.1, None if bad else "L", None if bad else 300.0))
        assert bool(fa["flags"] & E.FLAG_NONFINITE) == bad and fb["flags"] == 0
        fa["flags"] = 0
        assert fa.tobytes() == fb.tobytes(), t
    assert int(a.state["n_nonfinite"][0]) == 2 and int(b.state["n_nonfinite"][0]) == 0


# ------------------------------------------------------------------------------------------------ 3. polygon decisions
def polygons():
    rng = np.random.default_rng(20240611)
    out = []
    for n in (0, 1, 2, 3, 63, 64, 65, 1440):
        for concave in (False, True):
            if n == 0:
                out.append(np.zeros((0, 2), np.int64))
                continue
            ang = np.sort(rng.uniform(0, 2 * np.pi, n))
            r = np.full(n, 300.0) if not concave else rng.uniform(60, 300, n)       # a star-shaped polygon: concave where the radius dips
            p = np.stack([640 + r * np.cos(ang), 400 + r * np.sin(ang)], 1)
            out.append(np.asarray(np.round(p), np.int64))
    return out


def queries(poly, rng):
    q = [(640, 400), (-5, -7), (2000, 400), (640, 99), (640, 701)]
    for k in rng.choice(len(poly), min(len(poly), 12), replace=False) if len(poly) else []:
        (x0, y0), (x1, y1) = poly[k - 1], poly[k]
        q.append((int(x1), int(y1)))                                        # every sampled vertex
        q.append(((x0 + x1) // 2, (y0 + y1) // 2))                          # an edge midpoint (on the edge when both sums are even)
        q += [(int(x1) + 1, int(y1)), (int(x1), int(y1) - 1), ((x0 + x1) // 2 + 1, (y0 + y1) // 2)]   # near misses
    q += [(int(x), int(y)) for x, y in rng.integers(300, 1000, (20, 2))]
    return q


def test_polygon_decisions_equal_the_host_restatement():
    rng = np.random.default_rng(7)
    seen = set()
    sizes = set()
    for poly in polygons():
        sizes.add(len(poly))
        qs = queries(poly, rng)
        if 0 < len(poly) <= 65:                                              # small polygons: every vertex, every edge midpoint
            qs += [tuple(int(v) for v in p) for p in poly] + [tuple(int(v) for v in (poly[k - 1] + poly[k]) // 2) for k in range(len(poly))]
        for q in qs:
            want = A.point_in_polygon(poly, q)
            assert E.point_in_polygon(poly, q) == want, (len(poly), q)
            seen.add(want)
    assert sizes == {0, 1, 2, 3, 63, 64, 65, 1440} and seen == {-1, 0, 1}
    sq = [[0, 0], [10, 0], [10, 10], [0, 10]]                               # axis-parallel edges: midpoints are on the boundary
    assert [E.point_in_polygon(sq, q) for q in ((5, 5), (15, 5), (10, 5), (0, 0), (5, 0), (5, 11))] == [1, -1, 0, 0, 0, -1]


# ------------------------------------------------------------------------------------------------ 4. mixed windows
CHILD = r"""
import importlib, json, sys
sys.path.insert(0, sys.argv[1])
A = importlib.import_module("vehicle-cv-adas_amd.analysis")
out = []
for seq in json.load(open(sys.argv[2])):
    tc = A.TaskConditions()
    tr = []
    for inp in seq:
        check = tc.CheckStatus()
        tc.UpdateCollisionStatus(inp["distance"], inp["area"])
        tc.UpdateOffsetStatus(inp["offset"])
        tc.UpdateRouteStatus(inp["direction"], inp["curvature"])
        tr.append(dict(collision=tc.collision_msg.name, offset=tc.offset_msg.name, curvature=tc.curvature_msg.name, toggle=tc.toggle_status,
                       transform=tc.transform_status, osc=list(tc.toggle_oscillator_status), counters=dict(tc.toggle_status_counter), check=bool(check)))
    out.append(tr)
print(json.dumps(out))
"""


def test_mixed_direction_windows_pick_r_before_l_before_f(tmp_path):
    """Every non-empty subset of {L, R, F} in several insertion orders, against analysis.TaskConditions in a child interpreter under
    PYTHONHASHSEED=0 (the seed the goldens are made under): the window's direction decides HARD_LEFT / HARD_RIGHT / UNKNOWN."""
    seqs = []
    for k in (1, 2, 3):
        for sub in itertools.permutations("LRF", k):
            for curv in (300.0, 900.0):
                pattern = [sub[i % k] for i in range(10)]
                for rot in (0, 3):
                    dirs = pattern[rot:] + pattern[:rot]
                    seq = [dict(distance=None, area=True, offset=0.05, direction="F", curvature=curv) for _ in range(5)]   # fills the offset window
                    seq += [dict(distance=None, area=True, offset=0.05, direction=d, curvature=curv + i) for i, d in enumerate(dirs * 2)]
                    seqs.append(seq)
    path = tmp_path / "seqs.json"
    path.write_text(json.dumps(seqs))
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(path)], env=dict(os.environ, PYTHONHASHSEED="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    want_all = json.loads(r.stdout)
    msgs = set()
    for seq, want in zip(seqs, want_all):
        e = E.AnalysisEmu()
        check = True
        for t, (inp, w) in enumerate(zip(seq, want)):
            fr = e.step(E.make_input(None, inp["area"], inp["offset"], inp["direction"], inp["curvature"]))
            got = dict(E.frame_fields(fr), check=check)
            assert got == w, (t, [i["direction"] for i in seq], got, w)
            check = bool(fr["check"])
            msgs.add(got["curvature"])
    assert len(seqs) == 60 and msgs >= {"HARD_LEFT", "HARD_RIGHT", "EASY_LEFT", "EASY_RIGHT", "STRAIGHT", "UNKNOWN"}


# ------------------------------------------------------------------------------------------------ 5. distance edge cases
def test_distance_edge_cases():
    poly = [[-200, 0], [1400, 0], [1400, 720], [-200, 720]]
    boxes = [Box((-31, 100, -10, 300), "car"),          # negative corners: (-41) // 2 = -21, not -20
             Box((-30, 100, -11, 300), "person"),
             Box((10, 200, 50, 200), "car"),            # ymax == ymin: skipped
             Box((10, 200, 50, 650), "bus"),            # ymax == 650: kept
             Box((10, 200, 50, 651), "bus"),            # 651: skipped
             Box((100, 400, 200, 300), "truck"),        # ymax < ymin: kept with a negative distance, as the reference keeps it
             Box((300, 100, 400, 300), "traffic light"),   # not in object_list: ref_height 0
             Box((500, 100, 600, 300), "car"), Box((700, 100, 800, 300), "car")]   # equal distances
    want_pts, want_col = host_frame(boxes, poly)
    pts, col, fr = emu_frame(boxes, poly)
    assert pts == want_pts and col == want_col and len(pts) == 6
    assert pts[0][0] == -21 and pts[1][0] == -21 and pts[2][1] == 650 and pts[3][2] < 0 and col == pts[3]
    # the tie on d goes to the lower survivor index, whatever the order of the x coordinates
    for order in ([7, 8, 0], [8, 7, 0]):
        bs = [boxes[i] for i in order]
        want_pts, want_col = host_frame(bs, poly)
        pts, col, fr = emu_frame(bs, poly)
        assert pts == want_pts and col == want_col == pts[0] and pts[0][2] == pts[1][2] and int(fr["collision_index"]) == 0
    # a nearer object outside the polygon does not win; on the boundary it does
    inside = [[0, 0], [650, 0], [650, 720], [0, 720]]
    bs = [Box((500, 200, 600, 300), "car"), Box((700, 0, 800, 600), "truck"), Box((640, 0, 660, 300), "bus")]
    want_pts, want_col = host_frame(bs, inside)
    pts, col, fr = emu_frame(bs, inside)
    assert pts == want_pts and col == want_col
    assert A.point_in_polygon(inside, (650, 300)) == 0 and col[0] == 650 and int(fr["collision_index"]) == 2 and pts[1][2] < col[2] < pts[0][2]
    # capacity: survivors past max_points are not read and the frame says so
    e = E.AnalysisEmu(REF, max_points=2)
    fr, xy, d = e.frame([b.xyxy for b in bs], [2, 5, 4], inside, True, 0, 0.0, 0.0, det_flags=1)
    assert int(fr["n_points"]) == 2 and fr["flags"] == E.FLAG_OVERFLOW | E.FLAG_TRUNCATED


# ------------------------------------------------------------------------------------------------ 6. closed loop with the bird view
def drive(n=60):
    """A synthetic drive: lanes that sway, offsets that swing right then left (the Top oscillator), a long straight (the calibration
    counter) and a hard left curve with a centred car (Bottom).  A frame without a curve estimate separates the directions, so that no
    window mixes them (the in-process TaskConditions runs under any hash seed)."""
    frames = []
    for t in range(n):
        sway = int(round(14 * np.sin(t / 5.0)))
        ys = list(range(330, 720, 30))
        left = [(560 - (y - 330) // 2 + sway, y) for y in ys]
        right = [(720 + (y - 330) // 2 + sway, y) for y in ys]
        area = t % 7 != 3
        if t < 34:
            off, direction, curv = (0.3 if t < 17 else -0.3), "F", 20000.0 + t
        elif t == 34:
            off, direction, curv = 0.05, None, None
        else:
            off, direction, curv = 0.05, "L", 300.0 + t
        dist = None if t % 5 == 0 else 4.0 - 0.05 * t
        frames.append(dict(left=left, right=right, area=area, offset=off, direction=direction, curvature=curv, distance=dist))
    return frames


def test_closed_loop_requests_and_trapezoids_equal_the_host_loop():
    IMG = (1280, 720)
    tc, pt = A.TaskConditions(), A.PerspectiveTransformation(IMG)
    emu, bird = E.AnalysisEmu(), EB.BirdViewEmu(IMG)
    req = 1                                            # what reset queues: the reference's first CheckStatus() gives "Default"
    seen, applied = set(), 0
    for t, f in enumerate(drive()):
        # host loop, demo.py:287-296
        want_req = None
        if tc.CheckStatus():
            want_req = tc.transform_status
            if f["area"]:
                pt.updateTransformParams(f["left"], f["right"], tc.transform_status)
        tc.UpdateCollisionStatus(None if f["distance"] is None else [0, 0, f["distance"]], f["area"])
        tc.UpdateOffsetStatus(f["offset"])
        tc.UpdateRouteStatus(f["direction"], f["curvature"])
        # device loop: the pending request meets the frame, then the stage computes the next one
        assert E.MODES[req] == want_req, t
        applied += bird.frame(req, [[], f["left"], f["right"], []], [False, f["area"], f["area"], False]) == 1
        fr = emu.step(E.make_input(f["distance"], f["area"], f["offset"], f["direction"], f["curvature"]))
        req = int(fr["request"])
        seen.add(want_req)
        np.testing.assert_array_equal(bird.src, pt.src, err_msg=str(t))
        assert bird.src.tobytes() == pt.src.tobytes()
        got = E.frame_fields(fr)
        assert (got["collision"], got["offset"], got["curvature"]) == (tc.collision_msg.name, tc.offset_msg.name, tc.curvature_msg.name), t
        assert got["toggle"] == tc.toggle_status and got["counters"] == tc.toggle_status_counter, t
    assert seen >= {None, "Default", "Top", "Bottom"}, seen
    assert applied == bird.n_updates >= 4 and bird.n_rejected == 0


# ------------------------------------------------------------------------------------------------ the C ABI's records
def test_analysis_records_have_one_layout_in_the_header_ctypes_and_the_emulation(tmp_path):
    """include/adas_hip.h compiled by gcc, _lib.py's ctypes mirrors and the emulation's NumPy dtypes (= csrc/analysis_core.h, checked when the
    emulation loads) agree on every record's size and field offsets."""
    import ctypes as C
    L = importlib.import_module("adas_amd._lib")
    E.lib()
    pairs = [("adas_analysis_params", L.AnalysisParams, None), ("adas_analysis_state", L.AnalysisState, E.STATE_DTYPE),
             ("adas_analysis_input", L.AnalysisInput, E.INPUT_DTYPE), ("adas_analysis_frame", L.AnalysisFrame, E.FRAME_DTYPE)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "adas_hip.h"', 'int main(void) {']
    for cname, cls, _ in pairs:
        lines.append('  printf("%s size %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _t in cls._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    for cname, cls, dt in pairs:
        assert int(got[cname + " size"]) == C.sizeof(cls), cname
        offs = [int(got["%s.%s" % (cname, f)]) for f, _t in cls._fields_]
        assert offs == [getattr(cls, f).offset for f, _t in cls._fields_], cname
        if dt is not None:
            assert dt.itemsize == C.sizeof(cls) and [dt.fields[n][1] for n in dt.names] == offs, cname
    assert L.ANALYSIS_INPUT_DTYPE == E.INPUT_DTYPE and E.CFG_DTYPE.itemsize == L.AnalysisParams.h_ref_height.offset
