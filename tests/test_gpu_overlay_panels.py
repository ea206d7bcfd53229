"""GPU: the demo's three UI panels (csrc/overlay_panels.hip) through the C ABI, postproc.LaneOverlay and the fused step against the NumPy
restatement (tests/panels_ref.py), which tests/test_overlay_panels_cpu.py pins to the reference's own ControlPanel: every byte and every
record, no tolerances."""
import importlib

import numpy as np
import pytest

from conftest import load_pkg
import panels_ref as ref
import panel_scene as PS

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
CE = importlib.import_module("adas_amd.coreEngine")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")
A = importlib.import_module("adas_amd.analysis")

INVALID = -1        # ADAS_ERR_INVALID
ODD = (367, 403)
LATCH = PS.LATCHES


@pytest.fixture(scope="module")
def sprites():
    return PS.sprites()


def types_on_device(off, cur, col):
    return [L.DeviceBuffer.from_array(np.asarray(v, np.int32)) for v in (off, cur, col)]


def want_run(frames, sprites, latch, off, cur, col, S, B, birds=None, panels=7):
    """The restatement over a run of S streams x B frames; latch: the list of per-stream latches, updated.  -> (frames, records)."""
    out, recs = [None] * (S * B), [None] * (S * B)
    for b in range(B):
        for s in range(S):
            q = b * S + s
            out[q], r = ref.compose(frames[q], sprites, latch[s], off[q], cur[q], col[q], None if birds is None else birds[q], panels)
            latch[s] = r["latch"]
            recs[q] = dict(signs=r["signs"], collision=r["collision"], latch=LATCH[r["latch"]])
    return np.stack(out), recs


def got_records(ov, n):
    return [{k: v for k, v in ov.panel_record(q).items() if k in ("signs", "collision", "latch")} for q in range(n)]


def test_arrays_entry_latch_order_second_run_and_reset(sprites):
    """416 x 368 (the signs widget dims part of the bird panel), two streams x three frames: stream 0 latches Left, paints left and straight
    in one frame and ends Straight; stream 1 latches Right and is cleared by UNKNOWN.  A second run continues from the stored latches."""
    hw, S, B = PS.SMALL, 2, 3
    frames = PS.frames(S * B, hw, seed=1)
    birds = np.stack([PS.image(*PS.BIRD_HW[hw], 700 + q) for q in range(S * B)])
    #        s0 f0      s1 f0       s0 f1          s1 f1        s0 f2        s1 f2
    off = [0, 1, 3, 2, 0, 0]
    cur = [3, 5, 1, 2, 0, 0]      # s0: HARD_LEFT, STRAIGHT (two sprites), UNKNOWN + UNKNOWN offset (warn, cleared) ...
    col = [3, 2, 1, 0, 9, -1]     # ... and two values outside the enum: UNKNOWN
    off[4], cur[4] = 2, 2         # s0 f2: offset LEFT, EASY_LEFT: the Straight latch stays, LTA-right_lanes is painted
    ov = PP.LaneOverlay(hw, PS.BIRD_HW[hw], S * B)
    ov.set_panels(sprites)
    d_f, d_b = L.DeviceBuffer.from_array(frames), L.DeviceBuffer.from_array(birds)
    d_t = types_on_device(off, cur, col)
    latch = [0, 0]
    ov.run_panels_arrays(d_f.ptr, d_t[0].ptr, d_t[1].ptr, d_t[2].ptr, d_b.ptr, ("bird", "signs", "collision"), S, B)
    want, wrecs = want_run(frames, sprites, latch, off, cur, [c if 0 <= c < 4 else 0 for c in col], S, B, birds)
    got = d_f.download(frames.shape, np.uint8)
    assert got_records(ov, S * B) == wrecs
    assert any(len(r["signs"]) == 2 for r in wrecs), "no two-sprite frame"
    assert wrecs[2]["signs"] == ["left", "straight"] and wrecs[2]["latch"] == "Straight" and wrecs[1]["latch"] == "Right"
    for q in range(S * B):
        assert np.array_equal(got[q], want[q]), (q, np.argwhere(got[q] != want[q])[:5])
    assert ov.panel_record(4)["collision_type"] == 9 and np.array_equal(d_b.download(birds.shape, np.uint8), birds)
    assert latch == [3, 0]
    # a second run of one frame per stream continues from the stored latches: STRAIGHT latched on stream 0 shows under EASY_RIGHT
    off2, cur2, col2 = [3, 3], [4, 4], [1, 1]
    d_t2 = types_on_device(off2, cur2, col2)
    d_f.upload(frames)
    ov.run_panels_arrays(d_f.ptr, d_t2[0].ptr, d_t2[1].ptr, d_t2[2].ptr, d_b.ptr, 7, S, 1)
    want2, wrecs2 = want_run(frames, sprites, latch, off2, cur2, col2, S, 1, birds)
    got2 = d_f.download(frames.shape, np.uint8)
    assert got_records(ov, S) == wrecs2 and wrecs2[0]["signs"] == ["straight"] and wrecs2[1]["signs"] == []
    assert np.array_equal(got2[:S], want2) and np.array_equal(got2[S:], frames[S:])
    # reset_panels clears them: the same frame again paints nothing on stream 0
    ov.reset_panels()
    d_f.upload(frames)
    ov.run_panels_arrays(d_f.ptr, d_t2[0].ptr, d_t2[1].ptr, d_t2[2].ptr, d_b.ptr, 7, S, 1)
    assert [r["signs"] for r in got_records(ov, S)] == [[], []] and ov.panel_record(0)["latch"] is None
    want3, _ = want_run(frames, sprites, [0, 0], off2, cur2, col2, S, 1, birds)
    assert np.array_equal(d_f.download(frames.shape, np.uint8)[:S], want3)
    for b in [d_f, d_b] + d_t + d_t2:
        b.free()
    ov.close()


def test_odd_geometry_in_place_between_guards(sprites):
    """403 x 367 with a 131 x 77 bird image (non-integer ratios, an upscale, rows of 1209 bytes), two frames in place in a buffer with guard
    bytes on both sides, at two alignments: frames equal the restatement, the guards and every byte outside the panels are untouched."""
    hw, n = ODD, 2
    frames = PS.frames(n, hw, seed=2)
    birds = np.stack([PS.image(*PS.BIRD_HW[hw], 800 + q) for q in range(n)])
    off, cur, col = [1, 0], [3, 1], [2, 3]
    ov = PP.LaneOverlay(hw, PS.BIRD_HW[hw], n)
    ov.set_panels(sprites)
    d_b = L.DeviceBuffer.from_array(birds)
    d_t = types_on_device(off, cur, col)
    want, _ = want_run(frames, sprites, [0, 0], off, cur, col, n, 1, birds)
    untouched = ~(ref.panel_pixels(hw, sprites) | (want != frames).any(axis=3))      # per frame: outside every rectangle and every sprite
    for guard in (37, 64):
        host = np.full(frames.nbytes + 2 * guard, 0xA5, np.uint8)
        host[guard:guard + frames.nbytes] = frames.reshape(-1)
        d = L.DeviceBuffer.from_array(host)
        ov.reset_panels()
        ov.run_panels_arrays(d.ptr + guard, d_t[0].ptr, d_t[1].ptr, d_t[2].ptr, d_b.ptr, 7, n, 1)
        back = d.download(host.shape, np.uint8)
        assert (back[:guard] == 0xA5).all() and (back[guard + frames.nbytes:] == 0xA5).all(), guard
        got = back[guard:guard + frames.nbytes].reshape(frames.shape)
        for q in range(n):
            assert np.array_equal(got[q], want[q]), (guard, q, np.argwhere(got[q] != want[q])[:5])
            assert np.array_equal(got[q][untouched[q]], frames[q][untouched[q]])
        d.free()
    for b in [d_b] + d_t:
        b.free()
    ov.close()


@pytest.mark.parametrize("panels", [1, 2, 4, 7], ids=["bird", "signs", "collision", "all"])
def test_disjoint_panels_each_alone_and_together(panels, sprites):
    """One 1280 x 720 frame, where the three panels do not overlap."""
    hw = (720, 1280)
    frames = PS.frames(1, hw, seed=4)
    birds = PS.bird(hw)[None]
    ov = PP.LaneOverlay(hw, PS.BIRD_HW[hw], 1)
    ov.set_panels(sprites)
    d_f, d_b = L.DeviceBuffer.from_array(frames), L.DeviceBuffer.from_array(birds)
    d_t = types_on_device([2], [5], [3])
    ov.run_panels_arrays(d_f.ptr, d_t[0].ptr, d_t[1].ptr, d_t[2].ptr, d_b.ptr, panels, 1, 1)
    want, wrecs = want_run(frames, sprites, [0], [2], [5], [3], 1, 1, birds, panels)
    got = d_f.download(frames.shape, np.uint8)
    assert got_records(ov, 1) == wrecs
    assert np.array_equal(got[0], want[0]), np.argwhere(got[0] != want[0])[:5]
    assert (got[0] != frames[0]).any()
    for b in [d_f, d_b] + d_t:
        b.free()
    ov.close()


def test_handles_entry_equals_arrays_entry(sprites):
    """A short adas_analysis_run_inputs sequence that moves all three messages; the handles entry reads the analysis handle's frame rows and
    gives the bytes of the arrays entry fed the fetched rows, and both equal the restatement."""
    hw = PS.SMALL
    seq = [(None, True, 0.1, "L", 100.0)] * 5 + [(1.0, True, 0.1, "L", 100.0)] * 10 + [(2.0, True, 0.1, "F", 100000.0)] * 5 + \
          [(None, False, -0.9, "R", 100.0)] * 6
    n = len(seq)
    an = PP.Analysis(ref_height=[60.0], n_streams=1, max_frames=n)
    an.run_inputs(PP.Analysis.make_inputs(seq), 1, n)
    rows = [an.fetch_frame(q) for q in range(n)]
    off = [PS.OFFSETS.index(r["offset_msg"].name) for r in rows]
    cur = [PS.CURVATURES.index(r["curvature_msg"].name) for r in rows]
    col = [PS.COLLISIONS.index(r["collision_msg"].name) for r in rows]
    assert len(set(off)) > 1 and len(set(cur)) > 1 and len(set(col)) > 1, (off, cur, col)
    frames = PS.frames(n, hw, seed=5)
    ov = PP.LaneOverlay(hw, None, n)
    ov.set_panels(sprites)
    d_h, d_a = L.DeviceBuffer.from_array(frames), L.DeviceBuffer.from_array(frames)
    ov.run_panels(d_h.ptr, an, None, ("signs", "collision"), 1, n)
    recs_h = got_records(ov, n)
    ov.reset_panels()
    d_t = types_on_device(off, cur, col)
    ov.run_panels_arrays(d_a.ptr, d_t[0].ptr, d_t[1].ptr, d_t[2].ptr, None, 6, 1, n)
    want, wrecs = want_run(frames, sprites, [0], off, cur, col, 1, n, None, 6)
    gh, ga = d_h.download(frames.shape, np.uint8), d_a.download(frames.shape, np.uint8)
    assert recs_h == wrecs and got_records(ov, n) == wrecs
    assert np.array_equal(gh, ga) and np.array_equal(gh, want)
    assert len({tuple(r["signs"]) for r in wrecs}) > 2 and len({r["collision"] for r in wrecs}) > 2
    for b in [d_h, d_a] + d_t:
        b.free()
    ov.close()
    an.close()


def test_refusals(sprites):
    """Each is ADAS_ERR_INVALID with its message."""
    def refused(match, fn, *a, **k):
        with pytest.raises(RuntimeError, match=match) as ei:
            fn(*a, **k)
        assert ei.value.code == INVALID
    narrow = PP.LaneOverlay((720, 399), None, 1)                  # the signs widget is 400 columns wide
    refused("signs panel", narrow.set_panels, sprites)
    narrow.close()
    small = PP.LaneOverlay(PS.SMALL, None, 2)                     # W + 5 = 109 < 110
    refused("collision panel's sprite 1 .*W \\+ 5 = 109", small.set_panels, dict(sprites, fcws_prompt=np.zeros((100, 110, 4), np.uint8)))
    d_f = L.DeviceBuffer.from_array(PS.frames(2, PS.SMALL))
    d_t = types_on_device([0, 0, 0], [0, 0, 0], [0, 0, 0])
    refused("adas_overlay_run_panels_arrays: no panels set", small.run_panels_arrays, d_f.ptr, d_t[0].ptr, d_t[1].ptr, d_t[2].ptr, None, 6, 1, 1)
    refused("adas_overlay_run_panels: no panels set", small.run_panels, d_f.ptr, None, None, 0, 1, 1)
    small.set_panels(sprites)
    refused("adas_overlay_run_panels: .*analysis handle", small.run_panels, d_f.ptr, None, None, ("signs",), 1, 1)
    refused("adas_overlay_run_panels_arrays: the bird panel needs", small.run_panels_arrays, d_f.ptr, d_t[0].ptr, d_t[1].ptr, d_t[2].ptr, None, 7, 1, 1)
    refused("adas_overlay_run_panels_arrays: the bird panel needs", small.run_panels_arrays, d_f.ptr, d_t[0].ptr, d_t[1].ptr, d_t[2].ptr, d_f.ptr, 1, 1, 1)
    refused("adas_overlay_run_panels_arrays: unknown panel bits 0x8", small.run_panels_arrays, d_f.ptr, d_t[0].ptr, d_t[1].ptr, d_t[2].ptr, None, 8, 1, 1)
    refused("adas_overlay_run_panels_arrays: 3 streams x 1 frames, the handle holds 2", small.run_panels_arrays, d_f.ptr, d_t[0].ptr, d_t[1].ptr,
            d_t[2].ptr, None, 6, 3, 1)
    refused("the signs panel needs the offset and curvature types", small.run_panels_arrays, d_f.ptr, d_t[0].ptr, None, d_t[2].ptr, None, 2, 1, 1)
    refused("own buffer holds 0 drawn frames", small.run_panels_arrays, None, d_t[0].ptr, d_t[1].ptr, d_t[2].ptr, None, 6, 1, 1)
    with pytest.raises(ValueError, match="unknown overlay panel"):
        small.panel_mask(("text",))
    assert np.array_equal(d_f.download((2,) + PS.SMALL + (3,), np.uint8), PS.frames(2, PS.SMALL)), "a refused run wrote"
    small.run_panels_arrays(d_f.ptr, d_t[0].ptr, d_t[1].ptr, d_t[2].ptr, None, 6, 2, 1)      # and the handle still works
    assert small.panel_record(1)["signs"] == ["warn"]
    for b in [d_f] + d_t:
        b.free()
    small.close()


# ------------------------------------------------------------------------------------------------ the fused step
IMG = (1280, 720)
LANE_KW = dict(in_h=160, in_w=800, num_grid_row=100, num_cls_row=36, num_grid_col=50, num_cls_col=41)      # the reduced lane net of
LANE_CFG = dict(grid_row=100, cls_row=36, grid_col=50, cls_col=41, row_anchor=np.linspace(0.42, 1, 36),     # test_gpu_overlay.py
                col_anchor=np.linspace(0, 1, 41))
MAXC = 512
BOX_SCORE = 0.1


class PrescribedLanes:
    """The weight source of test_gpu_overlay.py: every weight zero, the last layer's bias puts both ego lanes on every row anchor.  The lane
    net's output is its bias whatever the input: area_status holds by construction."""

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
    d = tmp_path_factory.mktemp("ovp")
    lane = str(d / "lanes.hipm")
    M.build("ufldv2_res18", wsrc=PrescribedLanes(0), **LANE_KW).save(lane)
    seam = np.concatenate([netutil.coco_like_frames(2, seed=40 + i) for i in range(2)])
    det, _, _ = bench.build_detector(M, CE, "yolov8n", seam, str(d), "a", target_per_frame=25.0, capacity=MAXC)
    cam = [bench.cam_frames(2, 300 + i) for i in range(2)]
    return det, lane, cam


def test_fused_step_graph_replay_and_launch_count(models, sprites):
    """Bird view with its image, analysis and all three panels in the fused step: two steps, the second replayed from its graph;
    overlay_image equals the restatement applied to a panel-less twin's overlay image and bird-view image of the same step, with the
    analysis rows the step fetched; the captured step holds exactly two more kernels, and none more once the panels are unset."""
    det_model, lane_model, cam = models
    S = 2
    Mh = A.PerspectiveTransformation(IMG).M
    car = A.SingleCamDistanceMeasure.RefSizeDict["car"][0]
    kw = dict(n_streams=S, precision="bf16", src_hw=(720, 1280), lane_cfg=LANE_CFG, track=False, box_score=BOX_SCORE, max_candidates=MAXC,
              geometry=dict(bird_wh=IMG, M=Mh), birdview=dict(image=True), analysis=dict(ref_height=[car] * 80), use_graph=True)
    stages = ("lanes", "area", "distance", "bird")
    pp = PL.AdasPipeline(det_model, lane_model, overlay=dict(stages=stages, panels=("bird", "signs", "collision"), panel_sprites=sprites), **kw)
    twin = PL.AdasPipeline(det_model, lane_model, overlay=dict(stages=stages), **kw)
    dev = L.DeviceBuffer.from_array(cam[0])
    latch = [0] * S
    for k in range(2):
        for p in (pp, twin):
            p.step_frames(dev.ptr, (720, 1280), 0.6)
            p.sync()
        for s in range(S):
            fr = pp.analysis.fetch_frame(s)
            assert fr == twin.analysis.fetch_frame(s)
            off, cur, col = PS.OFFSETS.index(fr["offset_msg"].name), PS.CURVATURES.index(fr["curvature_msg"].name), PS.COLLISIONS.index(fr["collision_msg"].name)
            want, rec = ref.compose(twin.overlay_image(s), sprites, latch[s], off, cur, col, twin.birdview_image(s))
            latch[s] = rec["latch"]
            got = pp.overlay_image(s)
            assert np.array_equal(got, want), (k, s, np.argwhere(got != want)[:5])
            r = pp.overlay.panel_record(s)
            assert (r["signs"], r["collision"], r["latch"]) == (rec["signs"], rec["collision"], LATCH[rec["latch"]]), (k, s)
            assert (r["offset_type"], r["curvature_type"], r["collision_type"]) == (off, cur, col)
            assert (got != twin.overlay_image(s)).any(axis=2).mean() > 0.2       # 29 % of a 1280 x 720 frame lies in the panels; a pixel of zeros stays what it was
            assert np.array_equal(pp.birdview_image(s), twin.birdview_image(s))  # the bird panel reads the image, it does not write it
    n_panels, n_plain = pp.graph_kernels(), twin.graph_kernels()
    assert n_panels == n_plain + 2, (n_panels, n_plain)
    L.check(L.lib().adas_pipeline_set_overlay_panels(pp.h, 0))
    pp.step_frames(dev.ptr, (720, 1280), 0.6)
    pp.sync()
    assert pp.graph_kernels() == n_plain
    for s in range(S):
        assert np.array_equal(pp.overlay_image(s), twin.overlay_image(s))
    for p in (pp, twin):
        p.close()
    dev.free()


def test_pipeline_prerequisites(models, sprites):
    det_model, lane_model, cam = models
    Mh = A.PerspectiveTransformation(IMG).M
    kw = dict(n_streams=2, precision="bf16", src_hw=(720, 1280), lane_cfg=LANE_CFG, track=False, max_candidates=MAXC, use_graph=True,
              geometry=dict(bird_wh=IMG, M=Mh))
    with pytest.raises(ValueError, match="signs panel needs analysis="):
        PL.AdasPipeline(det_model, lane_model, overlay=dict(stages=3, panels=("signs",), panel_sprites=sprites), **kw)
    with pytest.raises(ValueError, match="bird panel needs birdview=dict\\(image=True\\)"):
        PL.AdasPipeline(det_model, lane_model, overlay=dict(stages=3, panels=("bird",), panel_sprites=sprites), **kw)
    with pytest.raises(ValueError, match="panel_sprites="):
        PL.AdasPipeline(det_model, lane_model, analysis=dict(ref_height=[60.0] * 80), overlay=dict(stages=3, panels=("collision",)), **kw)
    with pytest.raises(ValueError, match="unknown overlay panel"):
        PL.AdasPipeline(det_model, lane_model, overlay=dict(stages=3, panels=("text",), panel_sprites=sprites), **kw)
    p = PL.AdasPipeline(det_model, lane_model, overlay=dict(stages=3), **kw)      # no analysis handle, no warp
    for fn, match in ((lambda: L.check(L.lib().adas_pipeline_set_overlay_panels(p.h, 2)), "no panels set on the attached overlay handle"),
                      (lambda: L.check(L.lib().adas_pipeline_set_overlay_panels(p.h, 8)), "unknown panel bits 0x8")):
        with pytest.raises(RuntimeError, match=match) as ei:
            fn()
        assert ei.value.code == INVALID
    p.overlay.set_panels(sprites)
    d = L.DeviceBuffer.from_array(cam[0])
    for bits, match in ((2, "signs panel needs an attached analysis handle"), (4, "collision panel needs an attached analysis handle"),
                        (1, "bird panel needs an attached bird view with its warp")):
        L.check(L.lib().adas_pipeline_set_overlay_panels(p.h, bits))
        with pytest.raises(RuntimeError, match=match) as ei:      # refused at the step, by name
            p.step_frames(d.ptr, (720, 1280), 0.6)
        assert ei.value.code == INVALID
    L.check(L.lib().adas_pipeline_set_overlay_panels(p.h, 0))
    p.step_frames(d.ptr, (720, 1280), 0.6)
    p.sync()
    assert p.overlay_image(1).shape == (720, 1280, 3)
    p.close()
    d.free()
