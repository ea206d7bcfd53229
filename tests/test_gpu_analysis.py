"""GPU: distance, collision and the FCWS / LDWS / LKAS state machine per stream on the device (csrc/analysis_kernels.hip, adas_analysis_*)
and as the last stage of the fused step.  The kernel must equal the host build of the same text (tests/emu_analysis_api.py) field for
field and the reference's golden trace; the fused step with the stage must equal a host twin that drives request_transform from
analysis.* on what it fetched, captured or not."""
import ctypes as C, gzip, importlib, json, os

import numpy as np
import pytest

from conftest import load_pkg, GOLDEN
import emu_analysis_api as E
import netutil

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
CE = importlib.import_module("adas_amd.coreEngine")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")
A = importlib.import_module("adas_amd.analysis")

G = json.load(gzip.open(os.path.join(GOLDEN, "analysis.json.gz"), "rt"))
IMG = (1280, 720)
INVALID = -1     # ADAS_ERR_INVALID


def raw_frame(an, f):
    fr = L.AnalysisFrame()
    L.check(L.lib().adas_analysis_fetch_frame(an.h, f, C.byref(fr)))
    return np.frombuffer(bytes(fr), E.FRAME_DTYPE)[0]


def raw_state(an, s):
    st = L.AnalysisState()
    L.check(L.lib().adas_analysis_fetch_stream(an.h, s, C.byref(st)))
    return np.frombuffer(bytes(st), E.STATE_DTYPE)[0]


def same_record(got, want, ctx):
    assert got.tobytes() == want.tobytes(), (ctx, got, want)


# ------------------------------------------------------------------------------------------------ 1. the golden trace on the kernel
S1, T = 3, 400
_TRACE = {}


def trace_emulation():
    """Computed once: stream s is fed the golden inputs shifted by 7 s frames (wrapping); per stream the emulation's frame records and
    final state."""
    if not _TRACE:
        inputs = E.golden_inputs(G["state_machine"]["inputs"])
        table = np.zeros((T, S1), E.INPUT_DTYPE)
        frames, states = [], []
        for s in range(S1):
            table[:, s] = np.roll(inputs, -7 * s)
            e = E.AnalysisEmu()
            frames.append([e.step(r) for r in table[:, s]])
            states.append(e.state[0].copy())
        _TRACE.update(table=table, frames=frames, states=states)
    return _TRACE


@pytest.mark.parametrize("per_launch", [1, 50])
def test_golden_trace_three_shifted_streams(per_launch):
    tr = trace_emulation()
    an = PP.Analysis(n_streams=S1, max_frames=S1 * per_launch)
    want_check = True
    for t0 in range(0, T, per_launch):
        an.run_inputs(tr["table"][t0:t0 + per_launch].reshape(-1), S1, per_launch)
        for b in range(per_launch):
            for s in range(S1):
                same_record(raw_frame(an, b * S1 + s), tr["frames"][s][t0 + b], (t0 + b, s))     # a stream that saw another's inputs fails here
            got = an.fetch_frame(b * S1)                                                          # stream 0: the reference's own trace
            want = G["state_machine"]["trace"][t0 + b]
            assert (got["collision_msg"].name, got["offset_msg"].name, got["curvature_msg"].name) == (want["collision"], want["offset"], want["curvature"])
            assert (got["toggle_status"], got["transform_status"], got["toggle_oscillator_status"]) == (want["toggle"], want["transform"], want["osc"])
            assert got["toggle_status_counter"] == want["counters"] and want_check == want["check"], t0 + b
            want_check = got["check"]
    for s in range(S1):
        same_record(raw_state(an, s), tr["states"][s], ("state", s))
    with pytest.raises(RuntimeError) as ei:                       # the state machine alone leaves no distance points
        an.fetch_points(0, 1)
    assert ei.value.code == INVALID
    st = an.fetch_stream(0)
    # members of analysis.CollisionType / OffsetType / CurvatureType (compared by name: the suite imports the package under two names)
    assert [type(st[k]).__name__ for k in ("collision_msg", "offset_msg", "curvature_msg")] == ["CollisionType", "OffsetType", "CurvatureType"]
    assert st["collision_msg"].value == A.CollisionType[st["collision_msg"].name].value
    assert st["transform_status"] in (None, "Default", "Top", "Bottom") and len(st["vehicle_offset_record"]) <= 5
    an.reset(1)
    fresh = E.AnalysisEmu()
    same_record(raw_state(an, 1), fresh.state[0], "reset")
    same_record(raw_state(an, 2), tr["states"][2], "reset leaves the other streams")
    an.close()


# ------------------------------------------------------------------------------------------------ 2. distance and collision on raw arrays
CAP = 128                                            # det_stride = max_points: the largest count fills both
COUNTS = (0, 1, 63, 64, 65, CAP)
POLYS = (0, 3, 64, 65, 1440)
REF = np.array([59.0, 0.0, 58.5, 39.0, 124.41, 134.94, 62.4, 38.22])     # inches per class id; class 1 is not measured


def star(n, rng, concave):
    if n == 0:
        return np.zeros((0, 2), np.int32)
    ang = np.sort(rng.uniform(0, 2 * np.pi, n))
    r = rng.uniform(150, 420, n) if concave else np.full(n, 420.0)
    return np.asarray(np.round(np.stack([640 + 1.4 * r * np.cos(ang), 400 + 0.7 * r * np.sin(ang)], 1)), np.int32)


def boxes(n, rng):
    """Integer corners as RectInfo.tolist() gives them: negative x, heights from a small set (equal distances: the index tie-break
    decides), zero heights, bottoms around row 650 and classes without a reference height."""
    x0 = rng.integers(-60, 1200, n)
    y1 = rng.choice([300, 420, 500, 649, 650, 651, 700], n, p=[0.25, 0.25, 0.25, 0.07, 0.07, 0.06, 0.05])
    h = rng.choice([0, 40, 80, 160], n, p=[0.05, 0.35, 0.35, 0.25])
    xyxy = np.stack([x0, y1 - h, x0 + rng.integers(10, 200, n), y1], 1).astype(np.float64)
    return xyxy, rng.choice([0, 1, 2, 2, 2, 3, 4, 9], n).astype(np.int32)     # class 9 lies outside the table


def test_distance_and_collision_on_raw_arrays():
    rng = np.random.default_rng(20240613)
    S = 2
    combos = [(c, p) for c in COUNTS for p in POLYS]
    B = len(combos) // S
    F = S * B
    xyxy = np.zeros((F, CAP, 4), np.float64)
    cls = np.zeros((F, CAP), np.int32)
    counts = np.zeros((F, 4), np.int32)
    poly = np.zeros((F, 1440, 2), np.int32)
    npoly = np.zeros(F, np.int32)
    geo = np.zeros(F, np.dtype([("area_status", "i4"), ("n_left", "i4"), ("n_right", "i4"), ("direction", "i4"), ("bird", "i4", 4), ("curvature", "f8"),
                                ("offset", "f8")]))
    assert geo.dtype.itemsize == C.sizeof(L.LaneGeometryResult)
    for f, (c, p) in enumerate(combos):
        xyxy[f, :c], cls[f, :c] = boxes(c, rng)
        xyxy[f, c:] = [100, 100, 200, 300]                                     # rows past n_keep would be measurable: they must not be read
        cls[f, c:] = 2
        counts[f] = (c + 5, c, c, 0)
        pts = star(p, rng, concave=f % 2 == 1)
        poly[f, :p], npoly[f] = pts, p
        poly[f, p:] = 77
        geo[f] = (1, 0, 0, rng.integers(0, 4), (0, 0, 0, 0), rng.uniform(100, 30000), rng.uniform(-1, 1))
    counts[7, 3] = 1                                                            # a detector frame that overflowed its capacity
    f_tie = combos.index((CAP, 65))                                            # a frame of equal distances inside the polygon
    xyxy[f_tie, :CAP] = np.stack([np.arange(CAP) * 8.0 - 100, np.full(CAP, 340.0), np.arange(CAP) * 8.0 - 40, np.full(CAP, 420.0)], 1)   # the first ones lie outside
    cls[f_tie, :CAP] = 2
    poly[f_tie, :65] = star(65, rng, False)
    dev = [L.DeviceBuffer.from_array(a) for a in (xyxy, cls, counts, poly, npoly, geo)]
    req = L.DeviceBuffer.from_array(np.full(S, -7, np.int32))
    p = L.AnalysisParams()
    L.check(L.lib().adas_analysis_default_params(C.byref(p)))
    assert (p.focal, p.y_limit, p.distance_thres, p.offset_thres, p.curvae_thres, p.calib_frequency, p.calib_curvae_thres) == (100, 650, 1.5, 0.65, 500, 3, 15000)
    an = PP.Analysis(ref_height=REF, n_streams=S, max_frames=F, max_points=CAP)
    an.run_arrays(dev[0].ptr, dev[1].ptr, dev[2].ptr, CAP, dev[3].ptr, 1440, dev[4].ptr, dev[5].ptr, req.ptr, S, B)
    emus = [E.AnalysisEmu(REF, max_points=CAP) for _ in range(S)]
    n_col = n_pts = 0
    last = [0] * S
    for b in range(B):
        for s in range(S):
            f = b * S + s
            c, pn = combos[f]
            want, wxy, wd = emus[s].frame(xyxy[f, :c], cls[f, :c], poly[f, :pn], 1, int(geo["direction"][f]), float(geo["curvature"][f]),
                                          float(geo["offset"][f]), det_flags=int(counts[f, 3]))
            got = raw_frame(an, f)
            same_record(got, want, (f, c, pn))
            n = int(got["n_points"])
            gxy, gd = np.zeros((n, 2), np.int32), np.zeros(n, np.float64)
            L.check(L.lib().adas_analysis_fetch_points(an.h, f, L.ptr(gxy), L.ptr(gd), n))
            assert np.array_equal(gxy, wxy) and gd.tobytes() == wd.tobytes(), f
            assert n <= c and (c < 63 or n > c // 2) and (pn > 0 or not got["has_collision"])
            assert bool(got["flags"] & E.FLAG_OVERFLOW) == (f == 7)
            n_col += int(got["has_collision"])
            n_pts += n
            last[s] = int(got["request"])
    tie = raw_frame(an, f_tie)
    assert tie["n_points"] == CAP and tie["has_collision"]
    k = int(tie["collision_index"])
    inside = [E.point_in_polygon(poly[f_tie, :65], (int(x0 + x1) // 2, 420)) >= 0 for x0, _, x1, _ in xyxy[f_tie]]
    assert k == inside.index(True) > 0 and sum(inside) > 10                         # equal distances: the lowest index inside the polygon
    assert n_col >= 8 and n_pts > 500
    for s in range(S):
        same_record(raw_state(an, s), emus[s].state[0], ("state", s))
    assert req.download((S,), np.int32).tolist() == last                        # the request table holds each stream's last word
    with pytest.raises(RuntimeError) as ei:
        an.run_arrays(dev[0].ptr, dev[1].ptr, dev[2].ptr, CAP, dev[3].ptr, 1440, dev[4].ptr, dev[5].ptr, None, S, B + 1)
    assert ei.value.code == INVALID                                             # more frames than the tables hold
    an.close()
    for d in dev + [req]:
        d.free()


# ------------------------------------------------------------------------------------------------ 3. the fused step
LANE_KW = dict(in_h=160, in_w=800, num_grid_row=100, num_cls_row=36, num_grid_col=50, num_cls_col=41)      # the reduced lane net of
LANE_CFG = dict(grid_row=100, cls_row=36, grid_col=50, cls_col=41, row_anchor=np.linspace(0.42, 1, 36),     # test_gpu_pipeline.py
                col_anchor=np.linspace(0, 1, 41))
NAMES = ["class%d" % i for i in range(80)]
MAXC = 512
# The synthetic detector's scores are heavy-tailed across frames: at 0.4, the threshold bench.build_detector calibrates for, two of the
# four frames below have no survivor.  At 0.1 every one of them has 2 .. 22 survivors out of 13 .. 378 candidates (capacity 512); the
# pipeline test asserts that before it compares anything.
BOX_SCORE = 0.1


class PrescribedLanes:
    """The weight source of test_gpu_birdview.py: every weight zero, the last layer's bias puts both ego lanes on every row anchor.  The
    lane net's output is its bias whatever the input: area_status holds by construction."""

    def __init__(self):
        gr, r, gc, c = 100, 36, 50, 41
        loc_row = np.zeros((gr, r, 4), np.float32)
        exist_row = np.zeros((2, r, 4), np.float32)
        for k in range(r):
            loc_row[int(round(44 - 0.4 * k)), k, 1] = 10.0
            loc_row[int(round(55 + 0.45 * k)), k, 2] = 10.0
        exist_row[1, :, 1:3] = 5.0
        self.bias = np.concatenate([loc_row.reshape(-1), np.zeros(gc * c * 4, np.float32), exist_row.reshape(-1), np.zeros(2 * c * 4, np.float32)])

    def __call__(self, name, shape, kind, fill=None):
        if name == "cls.3.bias":
            assert tuple(shape) == self.bias.shape
            return self.bias
        return np.zeros(shape, np.float32)


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    import bench
    d = tmp_path_factory.mktemp("ana")
    lane = str(d / "lanes.hipm")
    M.build("ufldv2_res18", wsrc=PrescribedLanes(), **LANE_KW).save(lane)
    frames = [netutil.coco_like_frames(2, seed=40 + i) for i in range(2)]
    det, _, _ = bench.build_detector(M, CE, "yolov8n", np.concatenate(frames), str(d), "a", target_per_frame=25.0, capacity=MAXC)
    return det, lane, frames


class CarBox:
    """What updateDistance reads of a RectInfo; every class carries the car's reference height."""
    label = "car"

    def __init__(self, xyxy):
        self.xyxy = [int(v) for v in xyxy]

    def tolist(self):
        return list(self.xyxy)


def test_pipeline_graph_eager_and_host_twin_agree(models):
    det_model, lane_model, frames = models
    S, steps = 2, 16
    Mh = A.PerspectiveTransformation(IMG).M
    kw = dict(n_streams=S, precision="bf16", src_hw=(720, 1280), lane_cfg=LANE_CFG, track=False, box_score=BOX_SCORE, max_candidates=MAXC,
              geometry=dict(bird_wh=IMG, M=Mh), birdview=dict(image=False))
    car = A.SingleCamDistanceMeasure.RefSizeDict["car"][0]
    ana = dict(ref_height=[car] * 80)                                                  # every class given the car's reference height
    pg = PL.AdasPipeline(det_model, lane_model, use_graph=True, analysis=ana, **kw)
    pe = PL.AdasPipeline(det_model, lane_model, use_graph=False, analysis=ana, **kw)
    ph = PL.AdasPipeline(det_model, lane_model, use_graph=True, **kw)                 # the host twin: no analysis attached
    assert ph.analysis is None
    d_det = [L.DeviceBuffer.from_array(f) for f in frames]
    d_lane = L.DeviceBuffer.from_array(np.zeros((S, 3, 160, 800), np.float32))
    tcs = [A.TaskConditions() for _ in range(S)]
    dms = [A.SingleCamDistanceMeasure(object_list=["car"]) for _ in range(S)]
    dev_check = [True] * S                        # the reset state: the reference's first CheckStatus() is True with "Default"
    dev_request = ["Default"] * S
    n_points = n_collisions = 0
    requests = []
    for k in range(steps):
        d = d_det[k % 2]
        for s in range(S):                        # demo.py:287: CheckStatus() decides which rule this frame's lanes re-anchor with
            check = tcs[s].CheckStatus()
            assert check == dev_check[s] and (tcs[s].transform_status if check else None) == dev_request[s], (k, s)
            if check:
                ph.request_transform(s, tcs[s].transform_status)
            requests.append(tcs[s].transform_status if check else None)
        for p in (pg, pe, ph):
            p.step(d.ptr, d_lane.ptr)
            p.sync()
        for s in range(S):
            dets = PP.YoloPost.fetch(ph.post, s)
            geo = ph.geometry.fetch(s)
            assert 1 <= len(dets["keep"]) <= MAXC and geo["area_status"] and geo["direction"] is not None, (k, s, len(dets["keep"]))   # prescribed, not luck
            for p in (pg, pe):
                np.testing.assert_array_equal(PP.YoloPost.fetch(p.post, s)["xyxy_int"], dets["xyxy_int"])
            dms[s].updateDistance([CarBox(b) for b in dets["xyxy_int"]])
            point = dms[s].calcCollisionPoint(geo["area_points"])
            tcs[s].UpdateCollisionStatus(point, geo["area_status"])
            tcs[s].UpdateOffsetStatus(geo["offset"])
            tcs[s].UpdateRouteStatus(geo["direction"], geo["curvature"])
            dirs = {r[0] for r in tcs[s].vehicle_curvature_record}
            assert len(dirs) <= 1, "a mixed window would make the in-process TaskConditions depend on the hash seed"
            fg, fe = pg.analysis.fetch_frame(s), pe.analysis.fetch_frame(s)
            assert fg == fe, (k, s, fg, fe)
            assert fg["flags"] == 0 and fg["n_points"] == len(dms[s].distance_points)
            assert pg.analysis.fetch_points(s) == pe.analysis.fetch_points(s) == dms[s].distance_points, (k, s)
            assert fg["collision_point"] == point, (k, s)
            assert ((fg["collision_msg"].name, fg["offset_msg"].name, fg["curvature_msg"].name)
                    == (tcs[s].collision_msg.name, tcs[s].offset_msg.name, tcs[s].curvature_msg.name)), (k, s)
            assert (fg["toggle_status"], fg["transform_status"]) == (tcs[s].toggle_status, tcs[s].transform_status), (k, s)
            assert fg["toggle_oscillator_status"] == list(tcs[s].toggle_oscillator_status) and fg["toggle_status_counter"] == tcs[s].toggle_status_counter
            sg, se = pg.analysis.fetch_stream(s), pe.analysis.fetch_stream(s)
            assert sg == se
            assert sg["vehicle_collision_record"] == list(tcs[s].vehicle_collision_record) and sg["vehicle_offset_record"] == list(tcs[s].vehicle_offset_record)
            assert sg["vehicle_curvature_record"] == [list(r) for r in tcs[s].vehicle_curvature_record] and sg["n_nonfinite"] == 0
            dev_check[s], dev_request[s] = fg["check"], fg["request"]                 # compared with the host's CheckStatus() of the next step
            bg, be, bh = (p.birdview.fetch_stream(s) for p in (pg, pe, ph))
            for f in ("src", "M", "M_inv", "M_warp"):
                assert bg[f].tobytes() == be[f].tobytes() == bh[f].tobytes(), (k, s, f)
            assert (bg["n_updates"], bg["n_rejected"]) == (be["n_updates"], be["n_rejected"]) == (bh["n_updates"], bh["n_rejected"])
            ag, ae, ah = (p.birdview.fetch_frame(s)["applied"] for p in (pg, pe, ph))
            assert ag == ae == ah == (1 if requests[k * S + s] in ("Default", "Top", "Bottom") else 0), (k, s)
            if k == 0:
                assert ag == 1 and bg["n_updates"] == 1                                # the first step applies "Default" on every stream
            gg, ge = pg.geometry.fetch(s), pe.geometry.fetch(s)
            assert gg["curvature"] == ge["curvature"] == geo["curvature"] and gg["offset"] == ge["offset"] == geo["offset"]
            n_points += fg["n_points"]
            n_collisions += fg["collision_point"] is not None
    n_fired = sum(1 for r in requests if r is not None)
    print("requests per step and stream:", requests, "distance points", n_points, "collision points", n_collisions)
    assert n_points > 0
    for s in range(S):
        assert pg.birdview.fetch_stream(s)["n_updates"] == sum(1 for r in requests[s::S] if r is not None) >= 1
    assert n_fired >= S
    for o in (pg, pe, ph):
        o.close()
    for dbuf in d_det + [d_lane]:
        dbuf.free()


def test_a_pipeline_without_analysis_fetches_what_it_fetched_before(models):
    det_model, lane_model, frames = models
    S = 2
    Mh = A.PerspectiveTransformation(IMG).M
    kw = dict(n_streams=S, precision="bf16", src_hw=(720, 1280), lane_cfg=LANE_CFG, track=True, box_score=BOX_SCORE, max_candidates=MAXC,
              geometry=dict(bird_wh=IMG, M=Mh), use_graph=True)
    plain = PL.AdasPipeline(det_model, lane_model, **kw)
    with_a = PL.AdasPipeline(det_model, lane_model, analysis=dict(class_names=NAMES), micro_batch=1, **kw)       # no bird view: matrices stay the handle's
    d_det = L.DeviceBuffer.from_array(frames[0])
    d_lane = L.DeviceBuffer.from_array(np.zeros((S, 3, 160, 800), np.float32))
    for k in range(2):
        for p in (plain, with_a):
            p.step(d_det.ptr, d_lane.ptr)
            p.sync()
    assert plain.analysis is None
    for s in range(S):
        a, b = PP.YoloPost.fetch(plain.post, s), PP.YoloPost.fetch(with_a.post, s)
        for key in ("cand_anchor", "cand_conf", "keep", "xyxy_int", "class_id"):
            np.testing.assert_array_equal(a[key], b[key])
        assert plain.decode.fetch(s) == with_a.decode.fetch(s)
        ga, gb = plain.geometry.fetch(s), with_a.geometry.fetch(s)
        assert ga["curvature"] == gb["curvature"] and ga["offset"] == gb["offset"] and np.array_equal(ga["area_points"], gb["area_points"])
        (ha, ta, la), (hb, tb, lb) = plain.tracker.fetch(s), with_a.tracker.fetch(s)
        assert bytes(ha) == bytes(hb) and ta.tobytes() == tb.tobytes() and la.tobytes() == lb.tobytes()
        fr = with_a.analysis.fetch_frame(s)
        assert fr["n_points"] == 0 and fr["collision_point"] is None            # no class of this detector carries one of the six labels
        assert fr["collision_msg"].name == "NORMAL"                    # the ego lane is there and nothing is in it
    for o in (plain, with_a):
        o.close()
    d_det.free(); d_lane.free()


# ------------------------------------------------------------------------------------------------ 4. error paths
def test_error_paths(models):
    det_model, lane_model, frames = models
    Mh = A.PerspectiveTransformation(IMG).M
    kw = dict(precision="bf16", src_hw=(720, 1280), lane_cfg=LANE_CFG, track=False, max_candidates=MAXC, use_graph=True)
    geo = dict(bird_wh=IMG, M=Mh)
    with pytest.raises(RuntimeError, match="micro_batch") as ei:               # frame b's request cannot reach frame b + 1 inside one step
        PL.AdasPipeline(det_model, lane_model, n_streams=2, micro_batch=2, geometry=geo, birdview=dict(image=False), analysis=dict(class_names=NAMES), **kw)
    assert ei.value.code == INVALID
    p = PL.AdasPipeline(det_model, lane_model, n_streams=2, micro_batch=2, geometry=geo, analysis=dict(class_names=NAMES), **kw)   # without a bird view: fine
    assert p.analysis is not None
    p.close()
    p = PL.AdasPipeline(det_model, lane_model, n_streams=2, geometry=geo, birdview=dict(image=False), analysis=dict(class_names=NAMES), **kw)
    assert p.birdview.pending(0) == 1 and p.birdview.pending(1) == 1          # attach queued every stream's "Default"
    with pytest.raises(RuntimeError, match="owns the requests") as ei:
        p.request_transform(0, "Top")
    assert ei.value.code == INVALID
    p.close()
    with pytest.raises(RuntimeError, match="geometry") as ei:                  # attach without a geometry handle
        PL.AdasPipeline(det_model, lane_model, n_streams=2, analysis=dict(class_names=NAMES), **kw)
    assert ei.value.code == INVALID
    with pytest.raises(ValueError):
        PL.AdasPipeline(det_model, lane_model, n_streams=2, geometry=geo, analysis=dict(), **kw)
