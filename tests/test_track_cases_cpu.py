"""CPU: the cases of tests/track_cases.py, which tests/test_gpu_track_edges.py runs through the HIP tracker, are sound and not vacuous.

Sound: in every association of every frame of the contested (a) and degenerate (c) cases scipy's optimum and lap_ref("first") are the
same (x, y), so no cost tie decides anything there and scipy is a fair reference; lap_ref's objective equals scipy's; and the host
build of csrc/track_core.h (emu_api.Tracker, capacity as on the device) equals the expected messages and err bits of every case.
Not vacuous (conditions on the inputs, met by the oracle alone):
  contested, f1   n_hi == D and n_pool == T, the solver class and the LDS / HBM side of the cost matrix are those track_cases claims (both
                  sides occur under each capacity), and at least 8 % of the matched rows are NOT matched to their row minimum: a solver that
                  only took row minima could not pass.  Measured share of the matched rows, seed 1 for every pair:
                    (70, 63) 27.4 %   (64, 64) 33.3 %   (100, 127) 28.1 %   (128, 128) 31.7 %   (100, 130) 28.1 %   (255, 255) 29.8 %
                    (200, 256) 31.3 %   (511, 511) 29.0 %   (512, 512) 30.2 %   (300, 513) 30.1 %   (600, 700) 32.9 %
                  (255, 255) on the default (256, 256) tracker has one low-score row (max_dets leaves room for no more) and runs out of
                  track slots from f1 on: err 2, pinned by track_cases.CapOracle.
  tie scenes      a solver with one tie rule changed reaches the same objective on every cost matrix and a different tracker message:
                  the LAST minimum column for duplicate detections and symmetric blocks; for duplicate tracks, where two ROWS tie and
                  every row has one real column so that no column rule can matter, an equal slack replacing a path (`<=` for bt_lap's `<`).
Each test prints one line per case, past pytest's capture."""
import numpy as np
import pytest

import emu_api, lap_ref, parity_checks as pc, track_cases as TC
from oracle import bytetrack

SCIPY = bytetrack.lapjv_extended
CASES_A = [(T, D, cap) for T, D in TC.CONTESTED for cap in TC.caps_of(T, D)]


def _say(capsys, line):
    with capsys.disabled():
        print("\n" + line, end="")


def _both(cost, limit):
    """scipy's answer, after checking that lap_ref("first") gives the same one at the same objective."""
    x, y = SCIPY(cost, limit)
    x2, y2 = lap_ref.first(cost, limit)
    assert np.array_equal(x, x2) and np.array_equal(y, y2), "scipy and the first-minimum rule differ: a cost tie decides this %s problem" % (cost.shape,)
    assert np.isclose(lap_ref.objective(cost, limit, x, y), lap_ref.objective(cost, limit, x2, y2), rtol=1e-12, atol=0)
    return x, y


def _host(steps, cap):
    """The host build over the steps: [(snapshot, err)] per frame, and the tracker."""
    trk = emu_api.Tracker(MT=cap[0], MD=cap[1])
    out = []
    for st in steps:
        if isinstance(st, str):
            trk.reset()
        else:
            out.append(trk.update(st["boxes"], st["scores"], st["ids"]))
    return out, trk


def _check_host(steps, cap, want, ctx):
    got, trk = _host(steps, cap)
    assert len(got) == len(want)
    for f, ((g, gerr), (w, werr)) in enumerate(zip(got, want)):
        pc.check_track_frame(g, w, ctx=(ctx, f))
        assert gerr == werr, (ctx, f, gerr, werr)
    return trk


def test_lap_ref_equals_scipy_on_random_costs():
    rng = np.random.default_rng(0)
    for T, D in [(1, 1), (3, 7), (7, 3), (20, 20), (40, 65), (65, 40), (0, 4), (4, 0)]:
        cost = rng.uniform(0.05, 1.0, (T, D))
        for limit in (0.5, 0.8):
            x, y = lap_ref.first(cost, limit)
            if T and D:
                xs, ys = SCIPY(cost, limit)
                assert np.array_equal(x, xs) and np.array_equal(y, ys)
                for rule in ("last", "relax"):
                    xr, yr = lap_ref.lap_ref(cost, limit, rule)
                    assert np.array_equal(x, xr) and np.array_equal(y, yr)            # no tie: every rule finds the one optimum
            else:
                assert (x == -1).all() and (y == -1).all() and len(x) == T and len(y) == D


@pytest.mark.parametrize("T,D,cap", CASES_A, ids=lambda v: str(v).replace(" ", ""))
def test_contested_case(T, D, cap, monkeypatch, capsys):
    rec = TC.Recorder(_both)
    monkeypatch.setattr(bytetrack, "lapjv_extended", rec)
    steps = TC.contested_case(T, D, cap)["steps"]
    want, ora = TC.expected(steps, cap)
    # f1: its first association is the first T x D problem at match_thresh
    hi = [s for s in steps[1]["scores"] if s > 0.5]
    lo = [s for s in steps[1]["scores"] if 0.1 < s < 0.5]
    assert len(hi) == D and len(lo) == TC.n_lo_of(D, cap) == len(steps[1]["scores"]) - D and len(steps[1]["scores"]) <= cap[1]
    first = [c for c in rec.calls if c[0].shape == (T, D) and c[1] == 0.8]
    assert first, "f1's first association is not T x D"
    assert len(want[0][0]["tracked"]) == T and all(t["is_activated"] for t in want[0][0]["tracked"])     # n_pool == T
    cost, _, x, _ = first[0]
    assert TC.solver_class(D) == TC.SOLVER[(T, D)]
    assert TC.cost_side(T, D, cap) == TC.SIDE[(T, D, cap)]
    m = x >= 0
    share = float((x[m] != cost[m].argmin(1)).mean())
    _say(capsys, "contested (%d, %d) on %s: %s, cost matrix in %s, %d of %d rows matched, %.1f %% of them not to their row minimum, (tracked, lost) %s, err %s" % (
        T, D, cap, TC.SOLVER[(T, D)], TC.SIDE[(T, D, cap)].upper(), m.sum(), T, 100 * share, [(len(w["tracked"]), len(w["lost"])) for w, _ in want],
        [e for _, e in want]))
    assert share >= 0.08
    assert max(len(w["lost"]) for w, _ in want) >= 1                             # lost tracks, and re-activation on f3:
    assert any(t["tracklet_len"] == 0 and t["start_frame"] == 1 for t in want[3][0]["tracked"])
    trk = _check_host(steps, cap, want, (T, D, cap))
    got_tr, want_tr = trk.trajectories(), TC.oracle_trajectories(ora)
    assert len(got_tr) == len(want_tr)
    for g, w in zip(got_tr, want_tr):
        assert g.tolist() == w.tolist()


def test_both_cost_sides_under_each_capacity():
    for cap in (TC.BIG, TC.DEFAULT):
        sides = {TC.SIDE[k] for k in TC.SIDE if k[2] == cap}
        assert sides == {"lds", "hbm"}, (cap, sides)
    assert TC.SIDE[(70, 63, TC.BIG)] == TC.SIDE[(70, 63, TC.DEFAULT)] == "lds"
    assert TC.SIDE[(255, 255, TC.BIG)] == TC.SIDE[(255, 255, TC.DEFAULT)] == "hbm"
    assert TC.lds_fixed_bytes(1024, 1024) == 98521 and TC.lds_cost_doubles(1024, 1024) == 7652 and TC.lds_cost_doubles(256, 256) == 16580


@pytest.mark.parametrize("name", sorted(TC.degenerate_cases()))
def test_degenerate_case(name, monkeypatch, capsys):
    rec = TC.Recorder(_both)
    monkeypatch.setattr(bytetrack, "lapjv_extended", rec)
    steps = TC.degenerate_cases()[name]
    want, _ = TC.expected(steps, TC.DEFAULT)
    assert all(e == 0 for _, e in want)
    _check_host(steps, TC.DEFAULT, want, name)
    _say(capsys, "degenerate %s: %d frames, %d non-empty associations, lists %s" % (
        name, len(want), len(rec.calls), [(len(w["tracked"]), len(w["lost"])) for w, _ in want]))
    w = [s for s, _ in want]
    if name == "no-dets":
        assert len(w[1]["tracked"]) == 0 and len(w[1]["lost"]) == 7 and len(w[3]["tracked"]) == 7
    if name == "nothing":
        assert w[1]["count"] == 0 and not any(t["is_activated"] for t in w[2]["tracked"]) and all(t["is_activated"] for t in w[3]["tracked"])
    if name == "no-low-band":
        assert len(w[1]["lost"]) == 3
    if name == "unconfirmed-alone":
        assert len(w[1]["tracked"]) == 10 and len(w[2]["tracked"]) == 7 and not w[2]["lost"] and w[3]["count"] == 13
    if name == "on-threshold":
        assert not w[1]["tracked"] and len(w[1]["lost"]) == 7
    if name == "no-tracks":
        assert w[1]["frame_id"] == 1 and [t["track_id"] for t in w[1]["tracked"]] == list(range(1, 8))


@pytest.mark.parametrize("name", sorted(TC.tie_cases()))
def test_tie_case(name, monkeypatch, capsys):
    steps, rule = TC.tie_cases()[name]
    rec = TC.Recorder(lap_ref.first)
    monkeypatch.setattr(bytetrack, "lapjv_extended", rec)
    want, _ = TC.expected(steps, TC.BIG)
    assert all(e == 0 for _, e in want)
    n_tied = 0
    for cost, limit, x, y in rec.calls:                       # on the very matrices the tracker met: same objective, other assignment
        xm, ym = lap_ref.lap_ref(cost, limit, rule)
        xs, ys = SCIPY(cost, limit)
        o = lap_ref.objective(cost, limit, x, y)
        assert np.isclose(o, lap_ref.objective(cost, limit, xm, ym), rtol=1e-12, atol=0)
        assert np.isclose(o, lap_ref.objective(cost, limit, xs, ys), rtol=1e-12, atol=0)
        n_tied += int(not np.array_equal(x, xm))
    monkeypatch.setattr(bytetrack, "lapjv_extended", lambda c, l: lap_ref.lap_ref(c, l, rule))
    other, _ = TC.expected(steps, TC.BIG)
    differs = [f for f, ((a, _), (b, _)) in enumerate(zip(want, other)) if a != b]
    _say(capsys, "tie %s: %d rows on frame 2, %d of %d associations change under the '%s' rule, messages differ on frames %s" % (
        name, len(steps[1]["scores"]), n_tied, len(rec.calls), rule, differs))
    assert n_tied >= 1 and differs and differs[0] == 1
    if name == "dupdet-lo-100":
        assert rec.calls[1][1] == 0.5 and not np.array_equal(rec.calls[1][2], lap_ref.last(rec.calls[1][0], 0.5)[0])   # the second association
    monkeypatch.setattr(bytetrack, "lapjv_extended", lap_ref.first)
    _check_host(steps, TC.BIG, want, name)


def test_tie_columns_sit_where_the_table_says():
    for D, pairs in TC.TIE_PAIRS.items():
        allp = TC.pair_columns(D)
        assert sorted(c for p in allp for c in p) == list(range(D)) and all(j < jp for j, jp in allp)
        assert any(j // 64 == jp // 64 for j, jp in pairs)                                  # inside one 64-column group
        assert any(jp // 64 > j // 64 and jp % 64 < j % 64 for j, jp in pairs)              # the higher column on the lower lane
        if D >= 130:
            assert any(jp >= j + 64 and jp % 64 < j % 64 for j, jp in pairs)                # ... at least 64 columns apart (D = 100 has two groups)
    blk = TC.TIE_PAIRS[600]
    assert any(jp == j + 256 for j, jp in blk)                                              # one thread, two passes
    assert any(j // 256 == jp // 256 and j // 64 != jp // 64 for j, jp in blk)              # two waves of one pass
    assert [TC.solver_class(D) for D in sorted(TC.TIE_PAIRS)] == ["wave<2>", "wave<4>", "wave<8>", "block"]


@pytest.mark.parametrize("name", sorted(TC.capacity_cases()))
def test_capacity_case(name, monkeypatch, capsys):
    cap, steps, errs, _ = TC.capacity_cases()[name]
    monkeypatch.setattr(bytetrack, "lapjv_extended", TC.Recorder(_both))
    want, _ = TC.expected(steps, cap)
    assert [e for _, e in want] == errs
    _check_host(steps, cap, want, name)
    _say(capsys, "capacity %s on %s: err per frame %s" % (name, cap, errs))
    w = [s for s, _ in want]
    if name == "track-overflow":
        assert [t["track_id"] for t in w[0]["tracked"]] == list(range(1, 9)) == [t["track_id"] for t in w[1]["tracked"]] and w[1]["count"] == 8
        plain = bytetrack.BYTETracker().update(steps[0]["boxes"][:8], steps[0]["scores"][:8], steps[0]["ids"][:8])
        assert plain == w[0]                                                                # the oracle fed only the first eight
        assert w[2]["frame_id"] == 1 and w[2]["count"] == 3
    if name == "det-overflow":
        plain = bytetrack.BYTETracker().update(steps[0]["boxes"][:8], steps[0]["scores"][:8], steps[0]["ids"][:8])
        assert plain == w[0] and len(steps[0]["scores"]) == 12
    if name == "hist-overflow":
        assert all(len(s["tracked"]) == 1 and s["tracked"][0]["class_id"] == 0 for s in w)  # the vote never moves off class 0
