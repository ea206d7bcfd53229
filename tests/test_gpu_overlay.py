"""GPU: the lane overlay (csrc/overlay_kernels.hip) through the C ABI, postproc.LaneOverlay, the fused step and the drop-in Draw*
methods against the NumPy restatement (tests/overlay_ref.py), every byte."""
import importlib

import numpy as np
import pytest

from conftest import load_pkg
import overlay_ref as ref
import overlay_scene as OS
from overlay_scene import noise

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
CE = importlib.import_module("adas_amd.coreEngine")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")
A = importlib.import_module("adas_amd.analysis")
D = importlib.import_module("adas_amd.detectors")

MAXP = L.UFLD_MAX_POINTS
INVALID = -1        # ADAS_ERR_INVALID
POLY = [(10, 5), (8, 12), (8, 12), (3, 20), (2, 30), (40, 30), (35, 21), (30, 12), (28, 5)]
BOWTIE = [(5, 2), (30, 20), (30, 2), (5, 20)]


class Scene(OS.Scene):
    """Per-frame geometry of a batch with its area flags, offset types and colours, and the bird view's lanes."""

    def __init__(self, n, dist_cap=8, poly_cap=48):
        super().__init__(n, ("style", "bird"), dist_cap=dist_cap, poly_cap=poly_cap)

    def want(self, src, stages=7):
        out, flags = [], []
        for f in range(self.n):
            o, fl = ref.compose(src[f], self.lanes[f], self.poly[f], bool(self.area[f]), self.dist[f], self.offset[f], self.colour[f], stages)
            out.append(o)
            flags.append(fl)
        return np.stack(out), flags

    def want_bird(self, img):
        return np.stack([ref.draw_lanes(img[f], self.bird[f], self.offset[f], radius=10, direct=True) for f in range(self.n)])


def run(scene, src, stages=7, bird=None, style=None, **kw):
    """OS.run -> (frames, flags[, bird image])"""
    r = OS.run(scene, src, stages, bird=bird, **kw, **(style or {}))
    return (r.frames, r.flags) if bird is None else (r.frames, r.flags, r.bird)


def three_frames(h=45, w=70):
    """Three frames of h x w, each with its own geometry: the known-answer polygon with overlapping discs of different lanes, the bow-tie
    with discs cut by every border and a corner, and a polygon with vertices outside on all four sides under a full 4 x 128 table."""
    s = Scene(3)
    s.lanes[0] = [[(20, 18), (40, 30)], [(22, 18)], [(21, 19)], [(21, 18), (60, 40)]]            # four lanes over pixel (21, 18): lane 3 wins
    s.poly[0], s.colour[0], s.offset[0] = POLY, ref.COLLISION_COLORS[2], ref.OFFSET_RIGHT
    s.dist[0] = [(30, 25), (31, 26), (5, 5)]
    s.lanes[1] = [[(0, 10), (w - 1, 10)], [(30, 0), (30, h - 1)], [(0, 0), (w - 1, h - 1), (w - 1, 0), (0, h - 1)], [(-2, 20), (w + 1, 20), (33, -3), (33, h + 2)]]
    s.poly[1], s.colour[1], s.offset[1] = BOWTIE, ref.COLLISION_COLORS[3], ref.OFFSET_LEFT
    s.dist[1] = [(-3, -3), (w + 2, h + 3), (w - 1, 0), (w + 4, 10), (12, h + 4)]
    rng = np.random.default_rng(5)
    s.lanes[2] = [np.stack([rng.integers(-5, w + 5, MAXP), rng.integers(-5, h + 5, MAXP)], 1) for _ in range(4)]
    s.poly[2] = [(-9, 20), (35, -8), (w + 11, 25), (30, h + 12)]
    s.colour[2], s.offset[2] = ref.COLLISION_COLORS[1], ref.OFFSET_CENTER
    s.dist[2] = [(2 ** 31 - 1, 5), (-2 ** 31, 5), (5, 2 ** 31 - 1), (40, 40)]
    return s


@pytest.mark.parametrize("mode", ["offset16", "offset3", "own", "in_place"])
def test_three_frames_every_byte(mode):
    """210-byte rows: a frame's rows start on every alignment of a 16-byte piece, and 9450-byte frames start on three of them."""
    src = noise(3, 45, 70, 1)
    s = three_frames()
    want, wflags = s.want(src)
    got, flags = run(s, src, offset=3 if mode == "offset3" else 16, own=mode == "own", in_place=mode == "in_place")
    assert flags == wflags == [0, 0, 0]
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert tuple(want[0, 18, 21]) == tuple(ref.blend(ref.blend(np.array(ref.LANE_COLORS[3]), 0.3, src[0, 18, 21]), 0.85, np.array(ref.COLLISION_COLORS[2])))
    assert (want != src).any(axis=3).mean() > 0.2       # the case draws something


@pytest.mark.parametrize("stages", [0, 1, 2, 4, 3, 5, 6, 7])
def test_each_stage_alone_and_together(stages):
    src = noise(3, 45, 70, 2)
    s = three_frames()
    want, _ = s.want(src, stages)
    if stages == 0:     # no frame stage: no frame is written
        ov = PP.LaneOverlay((45, 70), None, 3)
        kw = s.upload()
        sbuf = L.DeviceBuffer.from_array(src)
        ov.run_arrays(sbuf.ptr, 3, stages=0, **kw)
        with pytest.raises(RuntimeError, match="never written"):
            ov.fetch(0)
        ov.close(); s.free(); sbuf.free()
        return
    got, _ = run(s, src, stages=stages)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("w", [1, 5, 64])
def test_widths(w):
    """Width 1 and 5: a 16-byte piece spans several rows; width 64: 192-byte rows, every row 16-byte aligned."""
    h = 23
    src = noise(2, h, w, 3)
    s = Scene(2)
    s.lanes[0] = [[(0, 3)], [(w - 1, 9)], [(w // 2, 15), (w // 2, 16)], [(w, 20)]]
    s.poly[0] = [(0, 2), (w - 1, 8), (w // 2, 20)]
    s.dist[0] = [(0, 11)]
    s.lanes[1] = [[(w // 3, 1)], [], [], [(w - 2, h - 1)]]
    s.poly[1] = [(-3, 4), (w + 3, 4), (w + 3, 12), (-3, 12)]
    s.offset[1] = ref.OFFSET_RIGHT
    want, _ = s.want(src)
    for offset in (16, 3):
        got, _ = run(s, src, offset=offset)
        assert np.array_equal(got, want), (w, offset)


def test_empty_lanes_area_status_off_and_polygon_range():
    src = noise(3, 45, 70, 4)
    s = Scene(3)
    s.poly[0], s.area[0] = POLY, 0                                      # a polygon, but area_status is 0: nothing is filled
    s.poly[1] = [(5, 5), (32768, 10), (20, 30)]                         # a vertex out of range: the fill is skipped, the flag is set
    s.lanes[1] = [[(10, 10)], [], [], []]
    s.poly[2] = [(5, 5), (32767, 10), (20, 30)]                         # the largest legal coordinate
    want, wflags = s.want(src)
    got, flags = run(s, src)
    assert flags == wflags == [0, ref.POLY_RANGE, 0]
    assert np.array_equal(got, want)
    assert np.array_equal(got[0], src[0])                               # an untouched frame is a copy
    assert np.array_equal(got[1], ref.draw_lanes(src[1], s.lanes[1])) and (got[2] != src[2]).any()


def test_degenerate_polygons_and_a_second_run_starts_clean():
    """n in {0, 1, 2}, one row, repeated vertices; then the same handle draws an empty scene: the coverage of the first run is gone."""
    src = noise(5, 45, 70, 6)
    s = Scene(5)
    s.poly = [[], [(7, 9)], [(7, 9), (30, 20)], [(3, 12), (20, 12), (41, 12), (10, 12)], [(4, 4), (30, 4), (30, 4), (30, 25), (30, 25), (4, 4)]]
    want, _ = s.want(src)
    assert (want[1] != src[1]).any(axis=2).sum() == 1
    ov = PP.LaneOverlay((45, 70), None, 5)
    kw = s.upload()
    sbuf = L.DeviceBuffer.from_array(src)
    ov.run_arrays(sbuf.ptr, 5, **kw)
    got = np.stack([ov.fetch(f) for f in range(5)])
    assert np.array_equal(got, want)
    empty = Scene(5)
    kw2 = empty.upload()
    ov.run_arrays(sbuf.ptr, 5, **kw2)
    assert np.array_equal(np.stack([ov.fetch(f) for f in range(5)]), src)
    ov.run_arrays(sbuf.ptr, 2, **kw)                                    # a shorter run: frames 0, 1
    assert np.array_equal(np.stack([ov.fetch(f) for f in range(2)]), want[:2])
    with pytest.raises(RuntimeError) as ei:
        ov.run_arrays(sbuf.ptr, 6, **kw)
    assert ei.value.code == INVALID
    ov.close(); s.free(); empty.free(); sbuf.free()


def test_bird_view_discs_in_place():
    """Discs of radius 10 on a 37 x 131 image (393-byte rows), written, lane order and colours of the frame's discs."""
    bird = noise(3, 37, 131, 7)
    src = noise(3, 45, 70, 8)
    s = three_frames()
    rng = np.random.default_rng(9)
    s.bird[0] = [[(20, 18)], [(28, 18)], [(24, 22)], [(24, 14), (120, 30)]]
    s.bird[1] = [[(0, 0), (130, 36)], [(-9, 18), (139, 18)], [(65, -10), (65, 46)], [(130, 0), (0, 36), (-11, 5), (141, 5)]]
    s.bird[2] = [np.stack([rng.integers(-12, 143, MAXP), rng.integers(-12, 49, MAXP)], 1) for _ in range(4)]
    want_b = s.want_bird(bird)
    want, _ = s.want(src)
    got, _, got_b = run(s, src, stages=15, bird=bird)
    assert np.array_equal(got_b, want_b) and np.array_equal(got, want)
    assert tuple(got_b[1, 0, 65]) == ref.OFFSET_COLOR                  # frame 1's offset type is LEFT: lane 2 is red; the disc's last row
    s2 = three_frames()
    s2.bird = s.bird
    _, _, only_b = run(s2, src, stages=8, bird=bird)                    # the bird stage alone
    assert np.array_equal(only_b, want_b)


def test_style_is_a_run_time_argument():
    src = noise(3, 45, 70, 10)
    s = three_frames()
    style = dict(lane_alpha=0.55, area_alpha=0.4, lane_radius=5, distance_radius=2, lane_colors=[(1, 2, 3), (40, 50, 60), (70, 80, 90), (200, 210, 220)])
    got, _ = run(s, src, style=style)
    want = []
    for f in range(3):
        o = ref.draw_lanes(src[f], s.lanes[f], s.offset[f], 0.55, 5, table=style["lane_colors"])
        o, _ = ref.draw_area(o, s.poly[f], s.colour[f], 0.4)
        want.append(ref.draw_distance(o, s.dist[f], 2))
    assert np.array_equal(got, np.stack(want))
    with pytest.raises(RuntimeError) as ei:
        PP.LaneOverlay((45, 70), None, 1, lane_radius=65)
    assert ei.value.code == INVALID


# ------------------------------------------------------------------------------------------------ the handles and the fused step
IMG = (1280, 720)
LANE_KW = dict(in_h=160, in_w=800, num_grid_row=100, num_cls_row=36, num_grid_col=50, num_cls_col=41)      # the reduced lane net of
LANE_CFG = dict(grid_row=100, cls_row=36, grid_col=50, cls_col=41, row_anchor=np.linspace(0.42, 1, 36),     # test_gpu_pipeline.py
                col_anchor=np.linspace(0, 1, 41))
MAXC = 512
BOX_SCORE = 0.1     # as in test_gpu_analysis.py: at this threshold the synthetic detector has survivors on every frame used here
OFFSETS = {"UNKNOWN": ref.OFFSET_UNKNOWN, "RIGHT": ref.OFFSET_RIGHT, "LEFT": ref.OFFSET_LEFT, "CENTER": ref.OFFSET_CENTER}
COLLISIONS = {"UNKNOWN": 0, "NORMAL": 1, "PROMPT": 2, "WARNING": 3}


class PrescribedLanes:
    """The weight source of test_gpu_birdview.py: every weight zero, the last layer's bias puts both ego lanes on every row anchor, `shift`
    grid cells to the side.  The lane net's output is its bias whatever the input: area_status holds by construction."""

    def __init__(self, shift=0):
        gr, r, gc, c = 100, 36, 50, 41
        loc_row = np.zeros((gr, r, 4), np.float32)
        exist_row = np.zeros((2, r, 4), np.float32)
        for k in range(r):
            loc_row[int(round(44 - 0.4 * k)) + shift, k, 1] = 10.0
            loc_row[int(round(55 + 0.45 * k)) + shift, k, 2] = 10.0
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
    import netutil
    d = tmp_path_factory.mktemp("ovl")
    lanes = {}
    for shift in (0, -12):
        lanes[shift] = str(d / ("lanes%d.hipm" % shift))
        M.build("ufldv2_res18", wsrc=PrescribedLanes(shift), **LANE_KW).save(lanes[shift])
    seam = np.concatenate([netutil.coco_like_frames(2, seed=40 + i) for i in range(2)])
    det, _, _ = bench.build_detector(M, CE, "yolov8n", seam, str(d), "a", target_per_frame=25.0, capacity=MAXC)
    cam = [bench.cam_frames(2, 300 + i) for i in range(2)]
    return det, lanes, cam


def restate(p, twin, cam, s):
    """(frame_show, bird view, offset name, collision name) of frame s from what the pipeline fetches."""
    lanes, _ = p.decode.fetch(s)
    geo = p.geometry.fetch(s)
    off, col, pts = "UNKNOWN", None, None
    if p.analysis is not None:
        fr = p.analysis.fetch_frame(s)
        off, col = fr["offset_msg"].name, fr["collision_msg"].name
        pts = [(x, y) for x, y, _ in p.analysis.fetch_points(s)]
    colour = ref.COLLISION_COLORS[COLLISIONS[col]] if col else ref.AREA_COLOR
    want, flags = ref.compose(cam[s], lanes, geo["area_points"], geo["area_status"], pts, OFFSETS[off], colour, 7 if pts is not None else 3)
    assert flags == 0
    bird = None
    if twin is not None:
        bird = ref.draw_lanes(twin.birdview_image(s), geo["bird_points"], OFFSETS[off], radius=10, direct=True)
    return want, bird, off, col, len(pts or [])


def test_pipeline_graph_eager_and_restatement(models):
    """Every stage in the fused step: graph and eager give the same frame_show and bird view, and both equal the restatement applied to
    what the pipeline fetches (lanes, polygon, analysis rows, distance points; the bird image of a twin pipeline without overlay)."""
    det_model, lane_models, cam = models
    S, steps = 2, 6
    Mh = A.PerspectiveTransformation(IMG).M
    car = A.SingleCamDistanceMeasure.RefSizeDict["car"][0]
    kw = dict(n_streams=S, precision="bf16", src_hw=(720, 1280), lane_cfg=LANE_CFG, track=False, box_score=BOX_SCORE, max_candidates=MAXC,
              geometry=dict(bird_wh=IMG, M=Mh), birdview=dict(image=True), analysis=dict(ref_height=[car] * 80))
    pg = PL.AdasPipeline(det_model, lane_models[0], use_graph=True, overlay=dict(stages=("lanes", "area", "distance", "bird")), **kw)
    pe = PL.AdasPipeline(det_model, lane_models[0], use_graph=False, overlay=dict(), **kw)        # stages=None: everything there is a handle for
    twin = PL.AdasPipeline(det_model, lane_models[0], use_graph=True, **kw)
    assert twin.overlay is None
    dev = [L.DeviceBuffer.from_array(c) for c in cam]
    seen, n_points = [], 0
    for k in range(steps):
        for p in (pg, pe, twin):
            p.step_frames(dev[k % 2].ptr, (720, 1280), 0.6)
            p.sync()
        for s in range(S):
            want, bird, off, col, npts = restate(pg, twin, cam[k % 2], s)
            seen.append((off, col))
            n_points += npts
            ig, ie = pg.overlay_image(s), pe.overlay_image(s)
            assert np.array_equal(ig, ie), (k, s)
            assert np.array_equal(ig, want), (k, s, np.argwhere(ig != want)[:5])
            assert pg.overlay.flags(s) == 0
            bg, be = pg.birdview_image(s), pe.birdview_image(s)
            assert np.array_equal(bg, be) and np.array_equal(bg, bird), (k, s)
            assert (ig != cam[k % 2][s]).any(axis=2).mean() > 0.02 and (bg != twin.birdview_image(s)).any()
            assert np.array_equal(dev[k % 2].download(cam[k % 2].shape, np.uint8), cam[k % 2])      # the step's frames are not written
    print("offset / collision per step and stream:", seen, "distance points", n_points)
    assert n_points > 0
    assert len({c for _, c in seen}) > 1, "the collision colour never changed"
    for o in (pg, pe, twin):
        o.close()
    for b in dev:
        b.free()


def test_pipeline_offset_colour_changes_and_no_analysis(models):
    """Ego lanes 12 grid cells to the left under a fixed homography: once the offset window fills, the frame's offset type leaves UNKNOWN
    for LEFT / RIGHT and an ego lane turns red.  A second pipeline without analysis draws UNKNOWN colours and the default area colour."""
    det_model, lane_models, cam = models
    S, steps = 2, 6
    Mh = A.PerspectiveTransformation(IMG).M
    kw = dict(n_streams=S, precision="bf16", src_hw=(720, 1280), lane_cfg=LANE_CFG, track=False, box_score=BOX_SCORE, max_candidates=MAXC,
              geometry=dict(bird_wh=IMG, M=Mh), use_graph=True)
    pa = PL.AdasPipeline(det_model, lane_models[-12], analysis=dict(class_names=["class%d" % i for i in range(80)]), overlay=dict(), **kw)
    pn = PL.AdasPipeline(det_model, lane_models[-12], overlay=dict(stages=3), **kw)
    dev = [L.DeviceBuffer.from_array(c) for c in cam]
    seen = []
    for k in range(steps):
        for p in (pa, pn):
            p.step_frames(dev[k % 2].ptr, (720, 1280), 0.6)
            p.sync()
        for s in range(S):
            want, _, off, col, _ = restate(pa, None, cam[k % 2], s)
            seen.append(off)
            assert np.array_equal(pa.overlay_image(s), want), (k, s)
            if k in (0, steps - 1):
                want_n, _, _, _, _ = restate(pn, None, cam[k % 2], s)
                assert np.array_equal(pn.overlay_image(s), want_n), (k, s)
    print("offset per step and stream:", seen)
    assert seen[0] == "UNKNOWN" and any(o in ("LEFT", "RIGHT") for o in seen), "the offset colour never changed"
    with pytest.raises(RuntimeError, match="no frame to draw on") as ei:      # seam tensors with an overlay attached
        pn.step(dev[0].ptr, dev[0].ptr)
    assert ei.value.code == INVALID
    for o in (pa, pn):
        o.close()
    for b in dev:
        b.free()


def test_a_pipeline_without_overlay_fetches_what_it_fetched_before(models):
    det_model, lane_models, cam = models
    S = 2
    Mh = A.PerspectiveTransformation(IMG).M
    kw = dict(n_streams=S, precision="bf16", src_hw=(720, 1280), lane_cfg=LANE_CFG, track=True, box_score=BOX_SCORE, max_candidates=MAXC,
              geometry=dict(bird_wh=IMG, M=Mh), analysis=dict(class_names=["class%d" % i for i in range(80)]), use_graph=True)
    plain = PL.AdasPipeline(det_model, lane_models[0], **kw)
    with_o = PL.AdasPipeline(det_model, lane_models[0], overlay=dict(), **kw)
    d = L.DeviceBuffer.from_array(cam[0])
    for k in range(2):
        for p in (plain, with_o):
            p.step_frames(d.ptr, (720, 1280), 0.6)
            p.sync()
    assert plain.overlay is None
    with pytest.raises(ValueError):
        plain.overlay_image(0)
    for s in range(S):
        a, b = PP.YoloPost.fetch(plain.post, s), PP.YoloPost.fetch(with_o.post, s)
        for key in ("cand_anchor", "cand_conf", "keep", "xyxy_int", "class_id"):
            np.testing.assert_array_equal(a[key], b[key])
        assert plain.decode.fetch(s) == with_o.decode.fetch(s)
        ga, gb = plain.geometry.fetch(s), with_o.geometry.fetch(s)
        assert ga["curvature"] == gb["curvature"] and ga["offset"] == gb["offset"] and np.array_equal(ga["area_points"], gb["area_points"])
        (ha, ta, la), (hb, tb, lb) = plain.tracker.fetch(s), with_o.tracker.fetch(s)
        assert bytes(ha) == bytes(hb) and ta.tobytes() == tb.tobytes() and la.tobytes() == lb.tobytes()
        assert plain.analysis.fetch_frame(s) == with_o.analysis.fetch_frame(s) and plain.analysis.fetch_stream(s) == with_o.analysis.fetch_stream(s)
    for o in (plain, with_o):
        o.close()
    d.free()


def test_error_paths(models):
    det_model, lane_models, cam = models
    Mh = A.PerspectiveTransformation(IMG).M
    kw = dict(n_streams=2, precision="bf16", src_hw=(720, 1280), lane_cfg=LANE_CFG, track=False, max_candidates=MAXC, use_graph=True)
    geo = dict(bird_wh=IMG, M=Mh)
    with pytest.raises(ValueError, match="geometry"):                           # missing prerequisites, named before anything is built
        PL.AdasPipeline(det_model, lane_models[0], overlay=dict(), **kw)
    with pytest.raises(ValueError, match="lane_model"):
        PL.AdasPipeline(det_model, None, geometry=geo, overlay=dict(), **kw)
    with pytest.raises(ValueError, match="analysis"):
        PL.AdasPipeline(det_model, lane_models[0], geometry=geo, overlay=dict(stages=("lanes", "distance")), **kw)
    with pytest.raises(ValueError, match="image=True"):
        PL.AdasPipeline(det_model, lane_models[0], geometry=geo, birdview=dict(image=False), overlay=dict(stages=("bird",)), **kw)
    with pytest.raises(ValueError, match="unknown overlay stage"):
        PL.AdasPipeline(det_model, lane_models[0], geometry=geo, overlay=dict(stages=("text",)), **kw)
    p = PL.AdasPipeline(det_model, lane_models[0], geometry=geo, **kw)
    small = PP.LaneOverlay((720, 1280), None, 1)                                  # capacity: one frame, a step has two
    with pytest.raises(RuntimeError, match="holds 1 frames") as ei:
        L.check(L.lib().adas_pipeline_attach_overlay(p.h, small.h))
    assert ei.value.code == INVALID
    other = PP.LaneOverlay((360, 640), None, 2)                                   # geometry: another frame size
    L.check(L.lib().adas_pipeline_attach_overlay(p.h, other.h))
    d = L.DeviceBuffer.from_array(cam[0])
    with pytest.raises(RuntimeError, match="360x640") as ei:
        p.step_frames(d.ptr, (720, 1280), 0.6)
    assert ei.value.code == INVALID
    good = PP.LaneOverlay((720, 1280), None, 2)
    L.check(L.lib().adas_pipeline_attach_overlay(p.h, good.h))
    L.check(L.lib().adas_pipeline_set_overlay_stages(p.h, 7))
    with pytest.raises(RuntimeError, match="analysis") as ei:                    # the distance stage without an analysis handle: refused at the step
        p.step_frames(d.ptr, (720, 1280), 0.6)
    assert ei.value.code == INVALID
    L.check(L.lib().adas_pipeline_set_overlay_stages(p.h, 3))
    p.step_frames(d.ptr, (720, 1280), 0.6)
    p.sync()
    assert good.fetch(1).shape == (720, 1280, 3)
    p.close(); d.free(); good.close()
    # a CurveLanes decoder: ten lanes, the reference's colour table has four
    curve = PP.UfldDecode(100, 36, 50, 41, 1280, 720, LANE_CFG["row_anchor"], LANE_CFG["col_anchor"], 1, 1, num_lanes=10)
    four = PP.UfldDecode(100, 36, 50, 41, 1280, 720, LANE_CFG["row_anchor"], LANE_CFG["col_anchor"], 1, 1, num_lanes=4)
    ov = PP.LaneOverlay((45, 70), None, 1)
    src = L.DeviceBuffer.from_array(noise(1, 45, 70, 0))
    with pytest.raises(RuntimeError, match="num_lanes = 10") as ei:
        ov.run(src.ptr, decode=curve)
    assert ei.value.code == INVALID
    with pytest.raises(RuntimeError, match="analysis handle") as ei:
        ov.run(src.ptr, decode=four, stages=("lanes", "distance"))
    assert ei.value.code == INVALID
    with pytest.raises(RuntimeError, match="bird") as ei:                        # no bird-view size at create
        ov.run(src.ptr, decode=four, stages=8)
    assert ei.value.code == INVALID
    ov.run(src.ptr, decode=four)                                                  # an empty decoder: a copy
    assert np.array_equal(ov.fetch(0), noise(1, 45, 70, 0)[0])
    for o in (ov, curve, four, small, other):
        o.close()
    src.free()


# ------------------------------------------------------------------------------------------------ the drop-in methods
def test_drop_in_methods(models):
    _, lane_models, _ = models
    img = noise(1, 45, 70, 12)[0]
    lanes = [[(20, 18), (40, 30)], [(22, 18), (-2, 5)], [(21, 19)], [(21, 18), (60, 40), (69, 44)]]
    det = D.UltrafastLaneDetectorV2(lane_models[0], D.LaneModelType.UFLDV2_CULANE, precision="bf16")
    det.lane_info.lanes_points = np.array(lanes + [None], dtype=object)[:4]
    det.lane_info._area_status, det.lane_info._area_points = True, np.array(POLY, np.int64)
    a = img.copy()
    det.DrawDetectedOnFrame(a, A.OffsetType.RIGHT, alpha=0.45)
    want = ref.draw_lanes(img, lanes, ref.OFFSET_RIGHT, 0.45)
    assert np.array_equal(a, want)
    det.DrawAreaOnFrame(a, color=(10, 200, 30), alpha=0.6)
    want, _ = ref.draw_area(want, POLY, (10, 200, 30), 0.6)
    assert np.array_equal(a, want)
    b = img.copy()
    det.DrawDetectedOnFrame(b)                                                    # the reference's defaults
    det.DrawAreaOnFrame(b)
    assert np.array_equal(b, ref.draw_area(ref.draw_lanes(img, lanes), POLY)[0])
    det.lane_info._area_status = False
    c = img.copy()
    det.DrawAreaOnFrame(c)
    assert np.array_equal(c, img)
    dbuf = L.DeviceBuffer.from_array(img)                                         # a StagedFrame is drawn where it sits
    det.DrawDetectedOnFrame(D.StagedFrame(dbuf.ptr, 45, 70, 0), A.OffsetType.LEFT)
    assert np.array_equal(dbuf.download(img.shape, np.uint8), ref.draw_lanes(img, lanes, ref.OFFSET_LEFT))
    assert D.UltrafastLaneDetector.DrawDetectedOnFrame is D.UltrafastLaneDetectorV2.DrawDetectedOnFrame      # v1 inherits both
    assert D.UltrafastLaneDetector.DrawAreaOnFrame is D.UltrafastLaneDetectorV2.DrawAreaOnFrame
    pt = A.PerspectiveTransformation((70, 45))
    e = img.copy()
    moved = [np.array(l, np.float64) + 0.75 for l in lanes]
    pt.DrawDetectedOnBirdView(e, moved, A.OffsetType.LEFT)
    trunc = [[(int(x), int(y)) for x, y in l] for l in moved]                    # the reference draws at (int(x), int(y)): -1.25 -> -1
    assert trunc[1][1] == (-1, 5) and np.array_equal(e, ref.draw_lanes(img, trunc, ref.OFFSET_LEFT, radius=10, direct=True))
    pt.close(); det.close(); dbuf.free()
