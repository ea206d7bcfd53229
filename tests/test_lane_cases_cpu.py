"""CPU: the cases of tests/lane_cases.py are sound and not vacuous.  The host emulation of the lane decoders and of the lane geometry
(csrc/post_core.h and lane_core.h, one thread) passes every case under the checks tests/test_gpu_lane_edges.py applies to the HIP
kernels, and each edge a case claims is asserted here: the tied existence pairs exist and would flip a lane, the valid counts sit on
their rules' edges, the first hot cells cover the cells named in lane_cases._hot_cells, a last-maximum restatement of the oracle gives
other points, the reference's directions cover L, R and F for both reasons, and both resample filters drop samples."""
import numpy as np
import pytest

import emu_api, lane_cases as LC, parity_checks as pc
import test_hostemu_logic as TH
from oracle import ufld_decode

_ids = lambda v: str(v).replace(" ", "")


def check_decode(got, want, family, what):
    """Exact family: equality.  Mixed family: +-1 px on at most 2 coordinates of a frame; the count is printed."""
    n_off = pc.check_lanes(got[0], got[1], want[0], want[1], tol_px=0 if family == "exact" else 1)
    if family != "exact":
        print("%s: %d coordinates differ from the oracle (by 1 px)" % (what, n_off))
    assert n_off <= (0 if family == "exact" else 2)


# ------------------------------------------------------------------------------------------------ UFLD v2
def _valid_counts(outs):
    er, ec = outs[2][0], outs[3][0]
    row, col = (er[1] > er[0]).sum(0), (ec[1] > ec[0]).sum(0)
    return (int(col[0]), int(row[1]), int(row[2]), int(col[3]))


def _has_tie(outs, lane):
    ex = outs[2][0] if lane in (1, 2) else outs[3][0]
    return bool((ex[1, :, lane] == ex[0, :, lane]).any())


def v2_differs_by_last_max(shape, lw):
    """Whether first and last maximum can give different points at all: the widest window, 2*lw + 1 cells, must not cover a whole column
    of the lanes that pass their count rule.  Only (2, 1, 2, 1) with lw >= 1 fails that."""
    return max(shape[0], shape[2]) > 2 * lw + 1


@pytest.mark.parametrize("shape,nl,lw,family", LC.V2_CASES, ids=_ids)
def test_v2_case(shape, nl, lw, family):
    outs, cfg, (W, H), counts = LC.v2_case(shape, nl, lw, family)
    Gr, R, Gc, C = shape
    assert [o.shape for o in outs] == [(1, Gr, R, nl), (1, Gc, C, nl), (1, 2, R, nl), (1, 2, C, nl)]
    want = ufld_decode.process_output(outs, cfg, W, H, lw)
    again = LC.restate_v2(outs, cfg, W, H, lw)
    assert (again[0], again[1]) == want                                      # the restatement with the oracle's rules is the oracle
    check_decode(emu_api.ufld(outs, cfg, W, H, lw), want, family, "emu v2 %s" % _ids((shape, nl, lw)))
    # every valid count sits on the edge of its rule
    assert _valid_counts(outs) == counts
    for lane, n in enumerate(counts):
        K, div = (R, 2) if lane in (1, 2) else (C, 4)
        edge = (K // div, K // div + 1)
        assert n in edge or (n in (2, 3) and 2 > K / div), (lane, n, K)
        assert len(want[0][lane]) == (n if n > K / div else 0) and want[1][lane] == (n > K / div and n > 2)
    # a tied existence pair that would flip a lane across its count rule if the tie went to "present"
    below = [lane for lane, n in enumerate(counts) if not n > ((R / 2) if lane in (1, 2) else (C / 4))]
    assert below and all(_has_tie(outs, lane) for lane in below)
    flipped = LC.restate_v2(outs, cfg, W, H, lw, tie_present=True)
    assert any(len(flipped[0][lane]) > 0 and len(want[0][lane]) == 0 for lane in below)
    # lanes 4 .. nl-1 carry full existence: decoded by mistake they would be lanes
    if nl > 4:
        assert ((outs[2][0][1] > outs[2][0][0])[:, 4:]).all() and ((outs[3][0][1] > outs[3][0][0])[:, 4:]).all()
    if family == "exact":
        last = LC.restate_v2(outs, cfg, W, H, lw, grid_rule="last")
        assert (last[0] != want[0]) == v2_differs_by_last_max(shape, lw)


def test_v2_case_set_covers_the_scan_and_the_rules():
    """Over the exact cases the decoded first maxima fall on cell 0, 1, G-2, G-1, the last cell of an unrolled group, the first cell of the
    next, and the tail; windows are clamped at both ends; item counts above 640 occur; a 2-point side lane comes out present but
    not detected; and exactly the nine cases of the minimum shape with lw >= 1 cannot tell the last maximum from the first."""
    seen = set()
    two_point_lane = False
    for shape, nl, lw, family in LC.V2_CASES:
        if family != "exact":
            continue
        outs, cfg, (W, H), counts = LC.v2_case(shape, nl, lw, family)
        lanes, det, trace = LC.restate_v2(outs, cfg, W, H, lw)
        two_point_lane |= any(len(lanes[i]) == 2 and not det[i] for i in (0, 3))
        for lane, G, m in trace:
            body = 8 * ((G - 1) // 8)
            for name, hit in (("cell 0", m == 0), ("cell 1", m == 1 and G > 3), ("cell G-2", m == G - 2 and G > 3), ("cell G-1", m == G - 1),
                              ("group's last cell", 8 <= m <= body and m % 8 == 0), ("next group's first cell", m % 8 == 1 and 9 <= m <= body),
                              ("tail's first cell", m == body + 1 and body >= 8), ("inside the tail", m > body + 1 and body >= 8),
                              ("clamped at 0", lw > 0 and m - lw < 0), ("clamped at G-1", lw > 0 and m + lw > G - 1)):
                if hit:
                    seen.add(name)
    assert seen == {"cell 0", "cell 1", "cell G-2", "cell G-1", "group's last cell", "next group's first cell", "tail's first cell",
                    "inside the tail", "clamped at 0", "clamped at G-1"}
    assert two_point_lane
    items = sorted({(s[1] + s[3]) * nl for s, nl, _, _ in LC.V2_CASES})
    assert items[0] == 8 and any(640 < n <= 1280 for n in items) and items[-1] == 256 * 16 > 6 * 640      # one trip .. seven trips
    blind = [(s, nl, lw) for s, nl, lw, fam in LC.V2_CASES if fam == "exact" and not v2_differs_by_last_max(s, lw)]
    assert len(blind) == 9 and all(s == (2, 1, 2, 1) for s, _, _ in blind)


@pytest.mark.parametrize("shape,nl,lw", LC.V2_BATCHES, ids=_ids)
def test_v2_batch(shape, nl, lw):
    launches, cfg, (W, H) = LC.v2_batch(shape, nl, lw)
    n_pts = []
    for outs, families in zip(launches, LC.V2_BATCH_FAMILIES):
        assert outs[0].shape[0] == 3
        for b, family in enumerate(families):
            fr = LC.frame_of(outs, b)
            want = ufld_decode.process_output(fr, cfg, W, H, lw)
            check_decode(emu_api.ufld(fr, cfg, W, H, lw), want, family, "emu v2 batch %s frame %d" % (_ids((shape, nl, lw)), b))
            n_pts.append(sum(len(l) for l in want[0]))
    assert len({n_pts[0], n_pts[1], n_pts[2]}) > 1 and 0 < n_pts[4] < n_pts[1]       # frame 1: fewer points in the second launch


# ------------------------------------------------------------------------------------------------ UFLD v1
def check_v1_roles(want, roles, K):
    """What the oracle must make of the planted lanes."""
    for l, role in enumerate(roles):
        n = {"tie": K, "two": 0, "three": 3, "half": K - K // 2 if K - K // 2 > 2 else 0}[role]
        assert len(want[0][l]) == n and want[1][l] == (n > 0), (l, role, len(want[0][l]))


@pytest.mark.parametrize("src", LC.V1_SOURCES, ids=_ids)
@pytest.mark.parametrize("shape,family", LC.V1_CASES, ids=_ids)
def test_v1_case(shape, family, src):
    head, roles, cfg = LC.v1_case(shape, family)
    G, K = shape
    assert head.shape == (1, G + 1, K, 4) and sorted(roles) == sorted(LC.V1_ROLES)
    iw, ih = LC.V1_INPUT
    want = ufld_decode.process_output_v1(head, cfg, iw, ih, src[0], src[1])
    assert LC.restate_v1(head, cfg, iw, ih, src[0], src[1]) == want
    check_v1_roles(want, roles, K)
    check_decode(emu_api.ufld1(head, cfg, LC.V1_INPUT, src), want, family, "emu v1 %s %s" % (_ids(shape), _ids(src)))
    flipped = LC.restate_v1(head, cfg, iw, ih, src[0], src[1], nolane_wins_tie=True)
    l = roles.index("tie")
    assert flipped[0][l] == [] and not flipped[1][l] and want[1][l]              # `>=` in place of `>` loses the lane


def test_v1_case_set():
    items = [4 * K for _, K in LC.V1_SHAPES]
    assert max(n for n in items if n <= 256) == 256 and min(n for n in items if n > 256) == 260 and max(items) == 512
    assert LC.V1_BATCH in LC.V1_SHAPES and 4 * LC.V1_BATCH[1] > 256
    # the source size matters: the same head gives other points at every source size
    head, roles, cfg = LC.v1_case((100, 56), "exact")
    pts = [ufld_decode.process_output_v1(head, cfg, 800, 288, w, h)[0] for w, h in LC.V1_SOURCES]
    assert pts[0] != pts[1] != pts[2] != pts[0]


def test_v1_batch():
    heads, roles, cfg = LC.v1_batch()
    assert heads.shape[0] == 3
    seen = []
    for b in range(3):
        want = ufld_decode.process_output_v1(heads[b], cfg, 800, 288, 1280, 720)
        check_v1_roles(want, roles[b], LC.V1_BATCH[1])
        check_decode(emu_api.ufld1(heads[b], cfg, LC.V1_INPUT, (1280, 720)), want, "mixed", "emu v1 batch frame %d" % b)
        seen.append(want[0])
    assert seen[0] != seen[1] != seen[2] != seen[0]


# ------------------------------------------------------------------------------------------------ lane geometry
def _bird_bends(lanes, M):
    """c0 of np.polyfit over the bird-view points of both ego lanes."""
    out = []
    for l in (lanes[1], lanes[2]):
        p = np.asarray(l, np.float64)
        q = (np.asarray(M, np.float64).reshape(3, 3) @ np.concatenate([p, np.ones((len(p), 1))], 1).T).T
        b = (q[:, :2] / q[:, 2:]).astype(np.int64)
        out.append(np.polyfit(b[:, 1], b[:, 0], 2)[0])
    return out


def _resample_drops(lanes, H):
    """(samples dropped by `y >= min(lane ys)`, samples dropped by `x >= 0` alone) of __adjust_lanes_points, over both ego lanes."""
    (lx, ly), (rx, ry) = zip(*lanes[1]), zip(*lanes[2])
    maxy, miny = max(H - 1, max(ly), max(ry)), min(H // 3, min(ly), min(ry))
    fity = np.linspace(miny, maxy, H)
    by_start = by_x = 0
    for x, y in ((lx, ly), (rx, ry)):
        f = np.polyfit(y, x, 2)
        fx = f[0] * fity ** 2 + f[1] * fity + f[2]
        by_start += int((fity < min(y)).sum())
        by_x += int(((fity >= min(y)) & (fx < 0)).sum())
    return by_start, by_x


@pytest.mark.parametrize("adjust", [True, False], ids=["adjust", "plain"])
@pytest.mark.parametrize("wh,counts", LC.GEO_CASES, ids=_ids)
def test_geometry_case(wh, counts, adjust):
    W, H = wh
    lanes, status = LC.geo_lanes(wh, counts)
    M = LC.geo_matrix(wh, lanes)
    assert (len(lanes[1]), len(lanes[2])) == counts
    for l in (lanes[1], lanes[2]):
        ys = [y for _, y in l]
        assert ys == sorted(set(ys)) and 0 <= ys[0] and ys[-1] < H                     # distinct rows, in a decoder's order
    assert lanes[1][0][1] != lanes[2][0][1]                                            # the lanes start on different rows
    want = TH._geometry_reference(lanes, status, W, H, M, adjust)
    assert (want[3] is None) == (H < 720)
    if H >= 720:
        assert min(abs(c) for c in _bird_bends(lanes, M)) >= 1e-5                      # rel=1e-7 on the radius tests the kernel, not rounding
    refit = adjust and min(counts) > 10
    assert (len(want[1]) != sum(counts)) == refit
    if refit:
        by_start, by_x = _resample_drops(lanes, H)
        assert by_start > 0 and by_x > 0                                               # both resample filters drop samples
    TH.check_geometry(emu_api.lane_geometry(lanes, status, H, wh, M, adjust), want)


def _reference_bend(lanes):
    lf = np.polyfit([y for _, y in lanes[1]], [x for x, _ in lanes[1]], 2)
    rf = np.polyfit([y for _, y in lanes[2]], [x for x, _ in lanes[2]], 2)
    return lf[0] if abs(lf[0]) > abs(rf[0]) else rf[0]


@pytest.mark.parametrize("name", sorted(LC.DIR_CASES))
def test_direction_case(name):
    side, c0, diff, direction, reason = LC.DIR_CASES[name]
    lanes, status = LC.dir_lanes(name)
    W, H = LC.DIR_WH
    bend = _reference_bend(lanes)                        # identity homography: the bird-view points are the points
    thr = -0.00015 if c0 < 0 else 0.00015
    assert (bend < thr) == (c0 < thr) and abs(bend - thr) >= 1e-6
    ego = np.asarray(lanes[1 if side == "L" else 2])
    assert ego[0, 0] - ego[len(ego) // 2, 0] == diff
    want = TH._geometry_reference(lanes, status, W, H, np.eye(3), False)
    assert want[3] == direction
    TH.check_geometry(emu_api.lane_geometry(lanes, status, H, (W, H), np.eye(3), False), want)


def test_direction_case_set():
    got = {(v[3], v[4]) for v in LC.DIR_CASES.values()}
    assert {d for d, _ in got} == {"L", "R", "F"} and ("F", "threshold") in got and ("F", "comparison") in got
    for sign in (-1, 1):                                 # both sides of both thresholds, both outcomes of both comparisons
        assert {(v[1], v[2]) for v in LC.DIR_CASES.values() if np.sign(v[1]) == sign} == {(sign * 0.00019, 0), (sign * 0.00019, -sign),
                                                                                         (sign * 0.00012, 0), (sign * 0.00012, -sign)}


def check_few(got, lanes, status, area, M, wh):
    """The project's rule for an ego lane of fewer than three points (lane_core.h: `nL >= 3 && nR >= 3`): no estimate -- direction None,
    curvature and offset written as 0.0 -- while the bird-view points and the area polygon are still written.  This is not the
    reference's behaviour: there np.polyfit raises on 1 point and returns LAPACK's minimum-norm parabola on 2."""
    import importlib
    A = importlib.import_module("adas_amd.analysis")
    tv = A.PerspectiveTransformation(wh)
    tv.M = np.asarray(M, np.float64).reshape(3, 3)
    assert got["direction"] is None and got["curvature"] is None and got["offset"] is None and got["raw"] == (0.0, 0.0)
    assert got["area_status"] == (status[1] and status[2])
    np.testing.assert_array_equal(got["area_points"], area)
    for i in range(4):
        np.testing.assert_array_equal(got["bird_points"][i], np.asarray(tv.transformToBirdViewPoints(lanes[i]), np.int64).reshape(-1, 2))


@pytest.mark.parametrize("counts", LC.FEW_COUNTS, ids=_ids)
def test_fewer_than_three_points(counts):
    lanes, status, area = LC.few_lanes(counts)
    assert (len(lanes[1]), len(lanes[2])) == counts and min(counts) < 3 and len(area) == (sum(counts) if min(counts) else 0)
    wh = (1280, 720)
    M = LC.geo_matrix(wh)
    check_few(emu_api.lane_geometry(lanes, status, 720, wh, M, True), lanes, status, area, M, wh)


def test_geometry_batch():
    launches, (W, H), Ms = LC.geo_batch()
    assert not np.array_equal(Ms[0], Ms[1]) and not np.array_equal(Ms[1], Ms[2])
    assert len(launches[1][1][0][1]) < len(launches[0][1][0][1]) and len(launches[1][1][0][2]) < len(launches[0][1][0][2])
    for frames in launches:
        for (lanes, status), M in zip(frames, Ms):
            TH.check_geometry(emu_api.lane_geometry(lanes, status, H, (W, H), M, True), TH._geometry_reference(lanes, status, W, H, M, True))
            TH.check_geometry(emu_api.lane_geometry(lanes, status, H, (W, H), Ms[0], True), TH._geometry_reference(lanes, status, W, H, Ms[0], True))
