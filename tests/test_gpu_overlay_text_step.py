"""GPU: the overlay's text inside the fused step (AdasPipeline(overlay=dict(text=...))) and through the handles' entry
(LaneOverlay.run_text): the image is the NumPy restatement's (tests/text_ref.py) fed with what the same step's post, tracker and analysis
handles fetch, on the image a text-less twin drew; with the graph and without, on a replayed second step, with the panels between the
scene's text and the panel strings; with text off the step is the twin's, launch for launch."""
import importlib

import numpy as np
import pytest

from conftest import load_pkg
import panels_ref
import panel_scene as PS
import text_ref as R
import text_scene as TS
import test_gpu_overlay_panels as TP     # the reduced lane net, the prescribed lanes and the detector of the panels' step test
from test_gpu_overlay_text import got_tuple

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
CE = importlib.import_module("adas_amd.coreEngine")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")
A = importlib.import_module("adas_amd.analysis")

NAMES = ["class %d" % k for k in range(80)]
COLORS = [((37 * k) % 256, (91 * k + 40) % 256, (53 * k + 200) % 256) for k in range(80)]
LINES = [(10, 345, TS.LINE_SLOT, (255, 255, 255), "FPS  : 31.42"), (900, 300, TS.LINE_SLOT_BINARY, (230, 230, 230), "object-infer : 0.01 s")]
TEXT = ("detections", "tracks", "track_ids", "distance", "panels", "lines")


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    import bench
    import netutil
    d = tmp_path_factory.mktemp("ovt")
    lane = str(d / "lanes.hipm")
    M.build("ufldv2_res18", wsrc=TP.PrescribedLanes(0), **TP.LANE_KW).save(lane)
    seam = np.concatenate([netutil.coco_like_frames(2, seed=40 + i) for i in range(2)])
    det, _, _ = bench.build_detector(M, CE, "yolov8n", seam, str(d), "a", target_per_frame=25.0, capacity=TP.MAXC)
    cam = [bench.cam_frames(2, 300 + i) for i in range(2)]
    return det, lane, cam


def scene_of(p, s):
    """What the step's handles hold for stream s, as text_ref.layout reads it."""
    dets = p.post.fetch_dets(s)
    _, tracked, _ = p.tracker.fetch(s)
    trajs = p.tracker.fetch_trajectories(s)[:len(tracked)]
    act = [k for k in range(len(tracked)) if tracked[k]["is_activated"]]
    fr = p.analysis.fetch_frame(s)
    pts = p.analysis.fetch_points(s)
    return dict(det_xyxy=dets["xyxy_int"], det_cls=dets["class_id"], trk_tlwh=[tracked[k]["tlwh"] for k in act], trk_cls=[tracked[k]["class_id"] for k in act],
                trk_ids=[tracked[k]["track_id"] for k in act], trk_last=[trajs[k][-1] if len(trajs[k]) else np.zeros(4) for k in act],
                traj_len=[len(trajs[k]) for k in act], dist_points=[q[:2] for q in pts], dist_d=[q[2] for q in pts],
                offset=PS.OFFSETS.index(fr["offset_msg"].name), curvature=PS.CURVATURES.index(fr["curvature_msg"].name),
                collision=PS.COLLISIONS.index(fr["collision_msg"].name), det_names=NAMES, trk_names=NAMES, det_colors=COLORS, trk_colors=COLORS, lines=LINES)


def pipeline_kw(S, use_graph):
    Mh = A.PerspectiveTransformation(TP.IMG).M
    car = A.SingleCamDistanceMeasure.RefSizeDict["car"][0]
    return dict(n_streams=S, precision="bf16", src_hw=(720, 1280), lane_cfg=TP.LANE_CFG, track=True, box_score=TP.BOX_SCORE, max_candidates=TP.MAXC,
                geometry=dict(bird_wh=TP.IMG, M=Mh), birdview=dict(image=True), analysis=dict(ref_height=[car] * 80), use_graph=use_graph)


@pytest.mark.parametrize("use_graph", (True, False))
def test_fused_step_text_over_the_stages(models, use_graph):
    det_model, lane_model, cam = models
    fonts, S = TS.fonts(), 2
    kw = pipeline_kw(S, use_graph)
    stages = ("lanes", "area", "distance", "detections", "tracks", "trajectories")
    common = dict(stages=stages, detection_colors=COLORS, track_colors=COLORS)
    pp = PL.AdasPipeline(det_model, lane_model, overlay=dict(common, text=TEXT, fonts=fonts, text_style=TS.STYLE, detection_names=NAMES, track_names=NAMES,
                                                             text_lines=LINES), **kw)
    twin = PL.AdasPipeline(det_model, lane_model, overlay=dict(common), **kw)
    devs = [L.DeviceBuffer.from_array(c) for c in cam]
    kinds = set()
    for k in range(4):                      # every step after the first is replayed from the graph: the same frames three times, so that
        for p in (pp, twin):                # the tracks live on and their trajectories grow past one box, then other frames
            p.step_frames(devs[k // 3].ptr, (720, 1280), 0.6)
            p.sync()
        for s in range(S):
            scene = scene_of(pp, s)
            items, flags = R.layout(scene, fonts, 1280, 720, 63, TS.STYLE)
            got_items = pp.overlay.text_items(s)
            assert [got_tuple(i) for i in got_items] == [TS.item_tuple(i) for i in items], (k, s)
            assert pp.overlay.text_flags(s) == flags
            want = R.paint(twin.overlay_image(s).copy(), items, fonts)
            got = pp.overlay_image(s)
            assert np.array_equal(got, want), (k, s, np.argwhere(got != want)[:5])
            kinds |= {i["source"] for i in items}
    assert kinds == {1, 2, 4, 8, 16, 32}, kinds      # the steps held every kind of text
    if use_graph:
        n_text, n_plain = pp.graph_kernels(), twin.graph_kernels()
        assert n_text == n_plain + 3, (n_text, n_plain)       # the layout, the scene's draw, the draw of the panel strings and lines
        L.check(L.lib().adas_pipeline_set_overlay_text(pp.h, 0))
        for p in (pp, twin):
            p.step_frames(devs[1].ptr, (720, 1280), 0.6)
            p.sync()
        assert pp.graph_kernels() == n_plain
        for s in range(S):
            assert np.array_equal(pp.overlay_image(s), twin.overlay_image(s))
    for p in (pp, twin):
        p.close()
    for d in devs:
        d.free()


def test_panel_strings_lie_over_the_panels_and_the_handles_entry(models):
    """Panels on: the scene's text is under them, the panel strings and the lines over them.  Then the same text through
    LaneOverlay.run_text on the twin's own buffer."""
    det_model, lane_model, cam = models
    fonts, S = TS.fonts(), 2
    sprites = PS.sprites()
    kw = pipeline_kw(S, True)
    common = dict(stages=("lanes", "area", "distance", "detections"), detection_colors=COLORS, track_colors=COLORS, panels=("signs", "collision"),
                  panel_sprites=sprites)
    text = dict(fonts=fonts, text_style=TS.STYLE, detection_names=NAMES, track_names=NAMES, text_lines=LINES)
    pp = PL.AdasPipeline(det_model, lane_model, overlay=dict(common, text=TEXT, **text), **kw)
    plain = PL.AdasPipeline(det_model, lane_model, overlay=dict(common, panels=()), **kw)       # neither panels nor text
    dev = L.DeviceBuffer.from_array(cam[0])
    latch = [0] * S
    for k in range(2):
        for p in (pp, plain):
            p.step_frames(dev.ptr, (720, 1280), 0.6)
            p.sync()
        for s in range(S):
            scene = scene_of(pp, s)
            items, flags = R.layout(scene, fonts, 1280, 720, 63, TS.STYLE)
            under = [i for i in items if i["source"] < R.PANELS]
            over = [i for i in items if i["source"] >= R.PANELS]
            img = R.paint(plain.overlay_image(s).copy(), under, fonts)
            img, rec = panels_ref.compose(img, sprites, latch[s], scene["offset"], scene["curvature"], scene["collision"], None, panels=6)
            latch[s] = rec["latch"]
            want = R.paint(img, over, fonts)
            got = pp.overlay_image(s)
            assert np.array_equal(got, want), (k, s, np.argwhere(got != want)[:5])
    # the handles' entry on the plain twin's own buffer: every kind at once, no panels
    before = [plain.overlay_image(s) for s in range(S)]
    plain.overlay.set_fonts(fonts)
    plain.overlay.set_text_style(**TS.STYLE)
    plain.overlay.set_text_labels("detections", NAMES)
    plain.overlay.set_text_labels("tracks", NAMES)
    plain.overlay.set_text_lines(LINES)
    plain.overlay.run_text(None, plain.post, plain.tracker, plain.analysis, TEXT, S, 1)
    for s in range(S):
        items, flags = R.layout(scene_of(plain, s), fonts, 1280, 720, 63, TS.STYLE)
        assert [got_tuple(i) for i in plain.overlay.text_items(s)] == [TS.item_tuple(i) for i in items]
        assert np.array_equal(plain.overlay.fetch(s), R.paint(before[s].copy(), items, fonts)), s
    with pytest.raises(RuntimeError, match="adas_overlay_run_text: the detections text needs a post handle"):
        plain.overlay.run_text(None, None, plain.tracker, plain.analysis, TEXT, S, 1)
    with pytest.raises(RuntimeError, match="adas_overlay_run_text: the distance text needs an analysis handle"):
        plain.overlay.run_text(None, plain.post, plain.tracker, None, TEXT, S, 1)
    with pytest.raises(RuntimeError, match="n_frames must be 1"):
        plain.overlay.run_text(None, plain.post, plain.tracker, plain.analysis, ("tracks",), 1, 2)
    for p in (pp, plain):
        p.close()
    dev.free()


def test_pipeline_prerequisites(models):
    det_model, lane_model, cam = models
    fonts = TS.fonts()
    kw = pipeline_kw(2, True)
    base = dict(stages=("lanes", "area"))
    with pytest.raises(ValueError, match="text= needs fonts="):
        PL.AdasPipeline(det_model, lane_model, overlay=dict(base, text=("lines",)), **kw)
    with pytest.raises(ValueError, match="unknown overlay text 'fps'"):
        PL.AdasPipeline(det_model, lane_model, overlay=dict(base, text=("fps",), fonts=fonts), **kw)
    with pytest.raises(ValueError, match="tracks and track_ids text need det_model= and track=True"):
        PL.AdasPipeline(det_model, lane_model, overlay=dict(base, text=("track_ids",), fonts=fonts), **dict(kw, track=False))
    with pytest.raises(ValueError, match="distance and panels text need analysis="):
        PL.AdasPipeline(det_model, lane_model, overlay=dict(base, text=("panels",), fonts=fonts), **dict(kw, analysis=None))
    p = PL.AdasPipeline(det_model, lane_model, overlay=dict(base), **kw)
    with pytest.raises(RuntimeError, match="adas_pipeline_set_overlay_text: no font set"):
        L.check(L.lib().adas_pipeline_set_overlay_text(p.h, 32))
    with pytest.raises(RuntimeError, match="adas_pipeline_set_overlay_text: unknown text bits 0x40"):
        L.check(L.lib().adas_pipeline_set_overlay_text(p.h, 64))
    p.close()
