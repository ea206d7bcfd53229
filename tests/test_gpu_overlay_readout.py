"""GPU: the bird view's readouts (csrc/overlay_readout.hip) through the C ABI, postproc.LaneOverlay, the fused step and the drop-in
calcCurveAndOffset against the NumPy restatement (tests/readout_ref.py), which tests/test_overlay_readout_cpu.py pins to the host build of
the same rules: every byte, every record field, every flag, no tolerances."""
import ctypes as C
import importlib

import numpy as np
import pytest

from conftest import load_pkg
import emu_overlay_readout_api as emu
import lane_cases as LC
import overlay_ref as ref
import panels_ref
import readout_ref as RR
import test_gpu_overlay_panels as TP     # the reduced lane net and the prescribed lanes of the panels' step test

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")
A = importlib.import_module("adas_amd.analysis")

INVALID = -1        # ADAS_ERR_INVALID
GUARD = 0xA5
RO, BIRD = 256, 8
SLOT = 10


@pytest.fixture(scope="module")
def font():
    return RR.synthetic_font()


def background(n, H, W, seed=7):
    return np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8)


def lane_table(frames):
    pts, cnt = np.zeros((len(frames), 4, L.UFLD_MAX_POINTS, 2), np.int32), np.zeros((len(frames), 4), np.int32)
    for q, lanes in enumerate(frames):
        for l, lane in enumerate(lanes):
            a = np.asarray(lane, np.int32).reshape(-1, 2)
            pts[q, l, :len(a)], cnt[q, l] = a, len(a)
    return pts, cnt


def device_run(ov, birds, direction, veh, cur, off, stages=RO, lanes=None, guard=0, entry=None):
    """-> (bird images after, the guards around them); the images sit `guard` bytes off a 16-byte boundary between two guard rows"""
    rows = birds.shape[2] * 3 * 2
    host = np.full(birds.nbytes + 2 * rows + guard, GUARD, np.uint8)
    at = rows + guard
    host[at:at + birds.nbytes] = birds.reshape(-1)
    d = L.DeviceBuffer.from_array(host)
    bufs = [L.DeviceBuffer.from_array(np.ascontiguousarray(direction, np.int32))] + [L.DeviceBuffer.from_array(np.ascontiguousarray(v, np.float64)) for v in (veh, cur, off)]
    kw = {}
    if lanes is not None:
        pts, cnt = lane_table(lanes)
        bufs += [L.DeviceBuffer.from_array(pts), L.DeviceBuffer.from_array(cnt)]
        kw = dict(bird_points=bufs[4].ptr, bird_counts=bufs[5].ptr)
    try:
        ov.run_arrays(None, len(birds), bird_ptr=d.ptr + at, stages=stages, readouts=tuple(b.ptr for b in bufs[:4]), **kw)
        back = d.download(host.shape, np.uint8)
    finally:
        for b in bufs + [d]:
            b.free()
    return back[at:at + birds.nbytes].reshape(birds.shape), (back[:at], back[at + birds.nbytes:])


# ---- 1: the arrays entry
@pytest.mark.parametrize("zoom", (1, 2))
@pytest.mark.parametrize("size", ((101, 37), (64, 96)))
def test_arrays_entry_draws_the_restatement(font, size, zoom):
    """Three frames: one inside with a RANGE string, one that fails the gate, one with veh_pos outside the image.  303-byte rows at three
    alignments of the buffer: every alignment of a 16-byte piece against a row occurs."""
    Wb, Hb = size
    birds = background(3, Hb, Wb)
    direction, veh, cur, off = [3, 0, 1], [Wb * 0.3, 5.0, Wb + 3.2], [2.0 ** 30, 80.0, float("inf")], [-0.04, 1.0, 1234.56]
    style = dict(zoom=zoom, offset_x=2, offset_y=7 * zoom, radius_x=-4, radius_y=Hb - 5)
    ov = PP.LaneOverlay((8, 8), (Hb, Wb), 3)
    ov.set_fonts({SLOT: font})
    ov.set_readout_style(**style)
    for guard in (0, 1, 15):
        got, guards = device_run(ov, birds, direction, veh, cur, off, guard=guard)
        assert (guards[0] == GUARD).all() and (guards[1] == GUARD).all(), "a guard byte was written"
        for q in range(3):
            want, wrec = RR.draw(birds[q], direction[q], veh[q], cur[q], off[q], font, style)
            assert RR.device_record_table(ov.readout_record(q)) == RR.record_table(wrec), (guard, q)
            assert np.array_equal(got[q], want), (guard, q, np.argwhere(got[q] != want)[:5])
        assert np.array_equal(got[1], birds[1]) and not np.array_equal(got[0], birds[0]) and not np.array_equal(got[2], birds[2])
        assert [ov.readout_record(q)["flags"] for q in range(3)] == [L.OVERLAY_READOUT_RANGE, 0, 0]
        assert ov.readout_record(0)["strings"][1]["skipped"] and ov.readout_record(0)["strings"][0]["text"] == "Offset: -0.0 m"
    emu_got, emu_recs = emu.run(birds, direction, veh, cur, off, font, style)
    assert np.array_equal(got, emu_got)
    ov.close()


def test_range_arrow_and_nan(font):
    Wb, Hb = 101, 37
    birds = background(2, Hb, Wb, 9)
    direction, veh, cur, off = [2, 2], [1e12, float("nan")], [float("nan"), 12.25], [0.35, float("-inf")]
    ov = PP.LaneOverlay((8, 8), (Hb, Wb), 2)
    ov.set_fonts({SLOT: font})
    ov.set_readout_style(zoom=1, offset_y=10, radius_y=25)
    got, _ = device_run(ov, birds, direction, veh, cur, off)
    for q in range(2):
        want, wrec = RR.draw(birds[q], direction[q], veh[q], cur[q], off[q], font, dict(zoom=1, offset_y=10, radius_y=25))
        assert RR.device_record_table(ov.readout_record(q)) == RR.record_table(wrec), q
        assert np.array_equal(got[q], want), q
    r = ov.readout_record(0)
    assert r["flags"] == L.OVERLAY_READOUT_RANGE and int(r["arrows"][0]["skipped"]) == 7 and int(r["arrows"][1]["skipped"]) == 0
    assert ov.readout_record(1)["flags"] == 0 and int(ov.readout_record(1)["arrows"][0]["x1"]) == 0      # NaN truncates to 0
    ov.close()


# ---- 2, 3: the stage off, the old entries' masks, the discs on top
def test_stage_off_old_masks_and_discs_over_readouts(font):
    Wb, Hb = 101, 130
    birds = background(2, Hb, Wb, 5)
    x_mid = int(Wb / 2.)
    lanes = [[[(10, 20), (12, 60)], [(x_mid, Hb - 4), (x_mid - 2, int(Hb / 1.3) + 3), (30, 30)], [(70, 80), (25, 9)], [(95, 100)]]] * 2
    direction, veh, cur, off = [2, 1], [33.0, 70.5], [250.0, 9.0], [0.3, -1.25]
    style = dict(zoom=2, offset_y=20, radius_y=44)
    ov = PP.LaneOverlay((8, 8), (Hb, Wb), 2)
    ov.set_fonts({SLOT: font})
    ov.set_readout_style(**style)
    both, _ = device_run(ov, birds, direction, veh, cur, off, stages=BIRD | RO, lanes=lanes)
    only, _ = device_run(ov, birds, direction, veh, cur, off, stages=RO, lanes=lanes)
    discs, _ = device_run(ov, birds, direction, veh, cur, off, stages=BIRD, lanes=lanes)       # the stage off, on the same handle after it was on
    for q in range(2):
        assert np.array_equal(both[q], RR.draw(birds[q], direction[q], veh[q], cur[q], off[q], font, style, lanes=lanes[q])[0]), q
        assert np.array_equal(only[q], RR.draw(birds[q], direction[q], veh[q], cur[q], off[q], font, style)[0]), q       # READOUTS alone leaves the discs out
        assert np.array_equal(discs[q], ref.draw_lanes(birds[q], lanes[q], radius=10, direct=True)), q
        assert np.array_equal(both[q], ref.draw_lanes(only[q], lanes[q], radius=10, direct=True)), q
    plain = PP.LaneOverlay((8, 8), (Hb, Wb), 2)                                                 # and a handle that never saw the stage
    discs2, _ = device_run(plain, birds, direction, veh, cur, off, stages=BIRD, lanes=lanes)
    assert np.array_equal(discs, discs2)
    plain.close()
    # the old entries keep their masks: 256 is the new entries' only, and 64 is nobody's
    lib, d = L.lib(), L.DeviceBuffer.from_array(birds)
    a = L.OverlayArrays(d_bird_bgr=d.ptr, stages=RO, n_frames=2)
    old = {"adas_overlay_run": lambda st: lib.adas_overlay_run(ov.h, None, None, None, None, None, d.ptr, st, 2, 1, None),
           "adas_overlay_run_objects": lambda st: lib.adas_overlay_run_objects(ov.h, None, None, None, None, None, None, None, d.ptr, st, 2, 1, None),
           "adas_overlay_run_trajectories": lambda st: lib.adas_overlay_run_trajectories(ov.h, None, None, None, None, None, None, None, d.ptr, st, 2, 1, None),
           "adas_overlay_run_arrays": lambda st: lib.adas_overlay_run_arrays(ov.h, None, None, None, None, None, 0, None, None, None, None, None, 0, None, None, None,
                                                                              d.ptr, st, 2, None),
           "adas_overlay_run_arrays_objects": lambda st: lib.adas_overlay_run_arrays_objects(ov.h, None, None, None, None, None, 0, None, None, None, None, None, 0,
                                                                                              None, None, None, d.ptr, None, 0, None, None, None, 0, None, None, st, 2,
                                                                                              None),
           "adas_overlay_run_arrays_trajectories": lambda st: lib.adas_overlay_run_arrays_trajectories(ov.h, C.byref(L.OverlayArrays(d_bird_bgr=d.ptr, stages=st, n_frames=2)))}
    for name, call in old.items():
        for st in (RO, RO | BIRD):
            with pytest.raises(RuntimeError, match=name + ": unknown stage bits") as ei:
                L.check(call(st))
            assert ei.value.code == INVALID
    new = {"adas_overlay_run_readouts": lambda st: lib.adas_overlay_run_readouts(ov.h, None, None, None, None, None, None, None, d.ptr, st, 2, 1, None),
           "adas_overlay_run_arrays_readouts": lambda st: lib.adas_overlay_run_arrays_readouts(ov.h, C.byref(L.OverlayArrays(d_bird_bgr=d.ptr, stages=st, n_frames=2)), None)}
    for name, call in new.items():
        for st in (64, 64 | RO, 512):
            with pytest.raises(RuntimeError, match=name + ": unknown stage bits") as ei:
                L.check(call(st))
            assert ei.value.code == INVALID
    assert np.array_equal(d.download(birds.shape, np.uint8), birds)                             # a refused run draws nothing
    d.free()
    ov.close()


# ---- 4: the named refusals
def test_refusals(font):
    Wb, Hb = 64, 96
    birds = background(1, Hb, Wb)
    d = L.DeviceBuffer.from_array(birds)
    vals = L.DeviceBuffer.from_array(np.zeros(4, np.float64))
    ra = lambda **kw: L.OverlayReadoutArrays(**dict(dict(d_direction=vals.ptr, d_veh_pos=vals.ptr, d_curvature=vals.ptr, d_offset=vals.ptr), **kw))
    arr = lambda ov, r, bird=d.ptr: L.lib().adas_overlay_run_arrays_readouts(ov.h, C.byref(L.OverlayArrays(d_bird_bgr=bird, stages=RO, n_frames=1)),
                                                                              C.byref(r) if r is not None else None)
    ov = PP.LaneOverlay((8, 8), (Hb, Wb), 1)
    nobird = PP.LaneOverlay((8, 8), None, 1)
    cases = [("adas_overlay_run_arrays_readouts: the readouts stage needs a handle created with a bird-view size and a bird-view image", lambda: arr(ov, ra(), None)),
             ("adas_overlay_run_arrays_readouts: the readouts stage needs a handle created with a bird-view size", lambda: arr(nobird, ra())),
             ("adas_overlay_run_arrays_readouts: the readouts stage needs font slot 10, which is empty", lambda: arr(ov, ra())),
             ("adas_overlay_run_arrays_readouts: the readouts stage needs the direction, veh_pos, curvature and offset arrays", lambda: arr(ov, None))]
    for k in ("d_direction", "d_veh_pos", "d_curvature", "d_offset"):
        cases.append(("adas_overlay_run_arrays_readouts: the readouts stage needs the direction, veh_pos, curvature and offset arrays",
                      lambda k=k: arr(ov, ra(**{k: None}))))
    cases += [("adas_overlay_run_readouts: the readouts stage needs a geometry handle",
               lambda: L.lib().adas_overlay_run_readouts(ov.h, None, None, None, None, None, None, None, d.ptr, RO, 1, 1, None)),
              ("adas_overlay_run_readouts: the readouts stage needs a handle created with a bird-view size and a bird-view image",
               lambda: L.lib().adas_overlay_run_readouts(ov.h, None, None, None, None, None, None, None, None, RO, 1, 1, None))]
    for msg, call in cases:
        with pytest.raises(RuntimeError, match=msg) as ei:
            L.check(call())
        assert ei.value.code == INVALID, msg
    for zoom in (0, 5, -1):
        with pytest.raises(RuntimeError, match="adas_overlay_set_readout_style: zoom %d" % zoom) as ei:
            ov.set_readout_style(zoom=zoom)
        assert ei.value.code == INVALID
    with pytest.raises(RuntimeError, match="adas_overlay_set_readout_style: font slot 16"):
        ov.set_readout_style(slot=16)
    with pytest.raises(TypeError, match="unknown overlay readout style"):
        ov.set_readout_style(colour=(1, 2, 3))
    ov.set_fonts({3: font})                                           # a font in another slot is not the readouts'
    with pytest.raises(RuntimeError, match="needs font slot 10, which is empty"):
        L.check(arr(ov, ra()))
    ov.set_readout_style(slot=3)
    L.check(arr(ov, ra()))                                            # direction 0: nothing is drawn
    assert np.array_equal(d.download(birds.shape, np.uint8), birds) and not ov.readout_record(0)["drawn"]
    with pytest.raises(RuntimeError, match="adas_overlay_fetch_readout: frame 1 was not part"):
        ov.readout_record(1)
    with pytest.raises(RuntimeError, match="adas_overlay_fetch_readout: no readouts run"):
        nobird.readout_record(0)
    for o in (ov, nobird):
        o.close()
    for b in (d, vals):
        b.free()


# ---- 5: the handles entry
def test_handles_entry_reads_the_geometry_handle(font):
    """Two frames of decoded lanes that curve (lane_cases' direction cases, 1280 x 720, identity homography) through a LaneGeometry: its
    veh_pos is the host build of lane_core.h's, bit for bit; the readouts' record is R1-R3 applied on the host to what the handle fetches;
    the image is the restatement's on those values."""
    W, H = LC.DIR_WH
    names = ("left-below-eq", "right-above-eq")
    dec = PP.UfldDecode(100, 36, 50, 41, W, H, TP.LANE_CFG["row_anchor"], TP.LANE_CFG["col_anchor"], 1, 2)
    geo = PP.LaneGeometry(H, (W, H), np.eye(3), True, 2)
    frames = [LC.dir_lanes(n) for n in names]
    for f, (lanes, det) in enumerate(frames):
        dec.upload(lanes, det, f)
    geo.run(dec, True, 2)
    big = RR.synthetic_font(seed=5, cell_h=24, baseline_row=18)
    ov = PP.LaneOverlay((8, 8), (H, W), 2)
    ov.set_fonts({SLOT: big})
    birds = background(2, H, W, 21)
    d = L.DeviceBuffer.from_array(birds)
    ov.run(None, geometry=geo, bird_ptr=d.ptr, stages=("readouts",), n_streams=2, n_frames=1)
    got = d.download(birds.shape, np.uint8)
    for f, (lanes, det) in enumerate(frames):
        g = geo.fetch(f)
        veh = geo.fetch_veh_pos(f)
        hdr, vals, e_veh = emu.lane_geometry(lanes, det, H, (W, H), np.eye(3), True)
        assert g["direction"] == LC.DIR_CASES[names[f]][3] == PP.LaneGeometry.DIRECTIONS[hdr[3]]
        assert np.float64(veh).tobytes() == np.float64(e_veh).tobytes() and 300 < veh < 1000, (veh, e_veh)
        assert g["curvature"] == pytest.approx(vals[0], rel=1e-7) and g["offset"] == pytest.approx(vals[1], rel=1e-7)      # pow() is the device's own
        want, wrec = RR.draw(birds[f], hdr[3], veh, g["curvature"], g["offset"], big)
        rec = ov.readout_record(f)
        assert RR.device_record_table(rec) == RR.record_table(wrec), f
        assert rec["drawn"] and int(rec["arrows"][0]["x1"]) == int(veh) and rec["strings"][0]["text"] == "Offset: %.1f m" % g["offset"]
        assert rec["strings"][1]["text"] == "R : %.1f m" % g["curvature"]
        assert np.array_equal(got[f], want), (f, np.argwhere(got[f] != want)[:5])
    # a frame without a curve: veh_pos is 0.0 and the frame is not touched
    lanes, det, _ = LC.few_lanes((2, 40))
    dec.upload(lanes, det, 1)
    geo.run(dec, True, 2)
    d.upload(birds)
    ov.run(None, geometry=geo, bird_ptr=d.ptr, stages=("readouts",), n_streams=2, n_frames=1)
    assert geo.fetch_veh_pos(1) == 0.0 and geo.fetch(1)["direction"] is None and geo.fetch_veh_pos(0) != 0.0
    assert np.array_equal(d.download(birds.shape, np.uint8)[1], birds[1]) and not ov.readout_record(1)["drawn"]
    with pytest.raises(RuntimeError, match="adas_lane_geometry_fetch_veh_pos: bad argument"):
        geo.fetch_veh_pos(2)
    for o in (ov, geo, dec):
        o.close()
    d.free()


# ---- 6: the fused step
@pytest.fixture(scope="module")
def lane_model(tmp_path_factory):
    import bench
    p = str(tmp_path_factory.mktemp("ovr") / "lanes.hipm")
    M.build("ufldv2_res18", wsrc=TP.PrescribedLanes(0), **TP.LANE_KW).save(p)
    return p, [bench.cam_frames(2, 300 + i) for i in range(2)]


def test_fused_step_bird_image_panel_and_launch_count(lane_model):
    """Two steps on different frames, the second replayed from its graph: birdview_image is the restatement over a stage-less twin's warp
    plus the discs; the bird panel shows it; with the stage off the captured step holds the kernels it always held."""
    lane, cam = lane_model
    S = 2
    big = RR.synthetic_font(seed=5, cell_h=24, baseline_row=18)
    sprites = TP.PS.sprites()
    kw = dict(n_streams=S, precision="bf16", src_hw=(720, 1280), lane_cfg=TP.LANE_CFG, track=False, geometry=dict(bird_wh=TP.IMG, M=A.PerspectiveTransformation(TP.IMG).M),
              birdview=dict(image=True), use_graph=True)
    stages = ("lanes", "area", "bird")
    pp = PL.AdasPipeline(None, lane, overlay=dict(stages=stages + ("readouts",), panels=("bird",), panel_sprites=sprites, fonts={SLOT: big},
                                                  readout=dict(slot=SLOT, zoom=2)), **kw)
    off_ = PL.AdasPipeline(None, lane, overlay=dict(stages=stages, panels=("bird",), panel_sprites=sprites, fonts={SLOT: big}), **kw)     # the stage off
    raw = PL.AdasPipeline(None, lane, overlay=dict(stages=("lanes", "area")), **kw)                                                          # the warp alone
    devs = [L.DeviceBuffer.from_array(c) for c in cam]
    for k in range(2):
        for p in (pp, off_, raw):
            p.step_frames(devs[k].ptr, (720, 1280), 0.6)
            p.sync()
        for s in range(S):
            g = pp.geometry.fetch(s)
            veh = pp.geometry.fetch_veh_pos(s)
            assert g["direction"] is not None
            want, wrec = RR.draw(raw.birdview_image(s), PP.LaneGeometry.DIRECTIONS.index(g["direction"]), veh, g["curvature"], g["offset"], big,
                                 dict(zoom=2), lanes=g["bird_points"])
            got = pp.birdview_image(s)
            assert RR.device_record_table(pp.overlay.readout_record(s)) == RR.record_table(wrec), (k, s)
            assert np.array_equal(got, want), (k, s, np.argwhere(got != want)[:5])
            assert not np.array_equal(got, off_.birdview_image(s))
            assert np.array_equal(off_.birdview_image(s), ref.draw_lanes(raw.birdview_image(s), g["bird_points"], radius=10, direct=True))
            panel = raw.overlay_image(s).copy()
            panels_ref.bird_panel(panel, got)                                                     # the bird panel reads whatever the bird image holds
            assert np.array_equal(pp.overlay_image(s), panel), (k, s)
            assert not np.array_equal(pp.overlay_image(s), off_.overlay_image(s))
    n_on, n_off = pp.graph_kernels(), off_.graph_kernels()
    assert n_on == n_off + 2, (n_on, n_off)                                                     # the layout and the draw
    plain = PL.AdasPipeline(None, lane, overlay=dict(stages=stages, panels=("bird",), panel_sprites=sprites), **kw)      # no font, no stage: the parent's step
    plain.step_frames(devs[0].ptr, (720, 1280), 0.6)
    plain.step_frames(devs[0].ptr, (720, 1280), 0.6)
    plain.sync()
    assert plain.graph_kernels() == n_off
    L.check(L.lib().adas_pipeline_set_overlay_readouts(pp.h, 0))
    for p in (pp, off_):
        p.step_frames(devs[1].ptr, (720, 1280), 0.6)
        p.sync()
    assert pp.graph_kernels() == n_off
    for s in range(S):
        assert np.array_equal(pp.birdview_image(s), off_.birdview_image(s)) and np.array_equal(pp.overlay_image(s), off_.overlay_image(s))
    for p in (pp, off_, raw, plain):
        p.close()
    for d in devs:
        d.free()


def test_pipeline_prerequisites(lane_model):
    lane, cam = lane_model
    big = RR.synthetic_font(seed=5, cell_h=24, baseline_row=18)
    kw = dict(n_streams=2, precision="bf16", src_hw=(720, 1280), lane_cfg=TP.LANE_CFG, track=False, geometry=dict(bird_wh=TP.IMG, M=A.PerspectiveTransformation(TP.IMG).M),
              use_graph=True)
    with pytest.raises(ValueError, match="readouts stage needs birdview=dict\\(image=True\\)"):
        PL.AdasPipeline(None, lane, overlay=dict(stages=("lanes", "readouts"), fonts={SLOT: big}), **kw)
    with pytest.raises(ValueError, match="readouts stage needs fonts=\\{10: atlas\\}"):
        PL.AdasPipeline(None, lane, birdview=dict(image=True), overlay=dict(stages=("lanes", "bird", "readouts")), **kw)
    with pytest.raises(ValueError, match="readouts stage needs fonts=\\{4: atlas\\}"):
        PL.AdasPipeline(None, lane, birdview=dict(image=True), overlay=dict(stages=("readouts",), fonts={SLOT: big}, readout=dict(slot=4)), **kw)
    p = PL.AdasPipeline(None, lane, birdview=dict(image=True), overlay=dict(), **kw)             # stages=None does not turn it on
    with pytest.raises(RuntimeError, match="adas_pipeline_set_overlay_readouts: the readouts stage needs font slot 10"):
        L.check(L.lib().adas_pipeline_set_overlay_readouts(p.h, 1))
    with pytest.raises(RuntimeError, match="adas_pipeline_set_overlay_stages: unknown stage bits"):
        L.check(L.lib().adas_pipeline_set_overlay_stages(p.h, RO))
    p.close()
    q = PL.AdasPipeline(None, lane, overlay=dict(stages=("lanes",)), **kw)                       # no bird view: refused at the step, by name
    q.overlay.set_fonts({SLOT: big})
    L.check(L.lib().adas_pipeline_set_overlay_readouts(q.h, 1))
    d = L.DeviceBuffer.from_array(cam[0])
    with pytest.raises(RuntimeError, match="readouts stage needs an attached bird view with its warp"):
        q.step_frames(d.ptr, (720, 1280), 0.6)
    q.close()
    d.free()


# ---- 7: the drop-in
def test_drop_in_calc_curve_and_offset_draws(font):
    W, H = LC.DIR_WH
    lanes, _ = LC.dir_lanes("right-above-eq")
    Lp, Rp = lanes[1], lanes[2]
    big = RR.synthetic_font(seed=5, cell_h=24, baseline_row=18)
    pt = A.PerspectiveTransformation((W, H))
    img = background(1, H, W, 33)[0]
    before = img.copy()
    plain = pt.calcCurveAndOffset(img, Lp, Rp)
    assert np.array_equal(img, before)                                 # without a font img is untouched
    assert plain == pt.calcCurveAndOffset(img.shape, Lp, Rp)
    pt.set_readout_font(big, zoom=2)
    assert pt.calcCurveAndOffset(img.shape, Lp, Rp) == plain           # a shape is not drawn on
    got = pt.calcCurveAndOffset(img, Lp, Rp)
    assert got == plain                                                # today's tuple
    (direction, curvature), offset = plain
    lf, rf = np.polyfit(np.asarray(Lp)[:, 1], np.asarray(Lp)[:, 0], 2), np.polyfit(np.asarray(Rp)[:, 1], np.asarray(Rp)[:, 0], 2)
    ploty = np.linspace(0, H - 1, H)
    veh = ((lf[0] * ploty ** 2 + lf[1] * ploty + lf[2])[719] + (rf[0] * ploty ** 2 + rf[1] * ploty + rf[2])[719]) / 2.      # its own fit's veh_pos
    want, wrec = RR.draw(before, "LRF".index(direction) + 1, veh, curvature, offset, big, dict(zoom=2))
    assert np.array_equal(img, want) and not np.array_equal(img, before)
    assert wrec["strings"][0]["text"] == "Offset: %.1f m" % offset and wrec["strings"][1]["text"] == "R : %.1f m" % curvature
    pt.set_readout_font(None)
    img2 = before.copy()
    pt.calcCurveAndOffset(img2, Lp, Rp)
    assert np.array_equal(img2, before)
    with pytest.raises(ValueError, match="zoom 5"):
        pt.set_readout_font(big, zoom=5)
    pt.close()
