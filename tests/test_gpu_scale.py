"""GPU: the scaling stage (csrc/scale_kernels.hip) through the C ABI, postproc.FrameScaler and the fused step: every byte equals the host
build of the same work items (tests/emu_scale_api.py, which tests/test_scale_cpu.py pins to tests/scale_ref.py), and no byte outside the
canvases is written.  Sizes, states and the sentinel scheme are the CPU suite's."""
import importlib

import numpy as np
import pytest

from conftest import load_pkg
import emu_jpeg_api as enc_emu
import emu_scale_api as emu
import emu_yuvout_api as yuv_emu
import test_gpu_jpeg as TJ
import test_gpu_overlay_panels as TP
import test_scale_cpu as TC

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")
A = importlib.import_module("adas_amd.analysis")

INVALID = -1        # ADAS_ERR_INVALID
FILL = emu.SENTINEL
GUARD = 64          # a multiple of 16: a buffer's payload keeps the allocation's alignment
BG = TC.BACKGROUND


def filled(n):
    b = L.DeviceBuffer(n)
    L.check(L.lib().adas_memcpy_h2d(b.ptr, L.ptr(np.full(n, FILL, np.uint8)), n))
    return b


def device_run(sc, bgr, states=None, src_off=0, dst_off=0):
    """bgr [n][h][w][3] uploaded into an allocation of exactly its size plus guard bands, src_off bytes off its alignment; scaled into such an
    allocation of exactly canvases(n) * canvas_bytes, dst_off bytes off, pre-filled with the sentinel.  -> uint8 [canvases][H][W][3]; the bands
    are checked."""
    bgr = np.ascontiguousarray(bgr)
    n, ns, k = len(bgr), bgr.size, sc.canvases(len(bgr))
    nd = k * sc.canvas_bytes
    src = filled(ns + 2 * GUARD + 16)
    L.check(L.lib().adas_memcpy_h2d(src.ptr + GUARD + src_off, L.ptr(bgr), ns))
    dst = filled(nd + 2 * GUARD + 16)
    st = None if states is None else L.DeviceBuffer.from_array(np.ascontiguousarray(states, np.int32))
    sc.run_device(src.ptr + GUARD + src_off, n, d_state=st.ptr if st else None, d_dst=dst.ptr + GUARD + dst_off)
    raw = dst.download((nd + 2 * GUARD + 16,), np.uint8)
    lo = GUARD + dst_off
    assert (raw[:lo] == FILL).all() and (raw[lo + nd:] == FILL).all(), "bytes outside the run's canvases were written"
    for b in (src, dst) + ((st,) if st else ()):
        b.free()
    return raw[lo:lo + nd].reshape((k,) + sc.canvas_hw + (3,))


def own_run(sc, bgr, states=None):
    """The same frames into the handle's own buffer: (the per-canvas fetches, fetch_all's canvases)"""
    dev = L.DeviceBuffer.from_array(np.ascontiguousarray(bgr))
    st = None if states is None else L.DeviceBuffer.from_array(np.ascontiguousarray(states, np.int32))
    sc.run_device(dev.ptr, len(bgr), d_state=st.ptr if st else None)
    each = np.stack([sc.canvas(k) for k in range(sc.canvases(len(bgr)))])
    whole = sc.fetch_all(len(bgr)).copy()
    for b in (dev,) + ((st,) if st else ()):
        b.free()
    return each, whole


@pytest.mark.parametrize("src", TC.SOURCES)
def test_device_equals_emulation(src):
    """The CPU suite's grid at its sizes into a caller's buffer pre-filled with the sentinel, and into the handle's own buffer: equal to the
    emulation's canvases byte for byte, background cells and borders included."""
    seed = 100
    for s, size, mode, mosaic, batch, border in TC.grid():
        if s != src:
            continue
        seed += 1
        bgr = TC.noise((batch, s[1], s[0], 3), seed)
        st = TC.STATES[:batch]
        want = emu.scale(bgr, emu.params(s, size, mode, mosaic, border, BG), st)
        sc = PP.FrameScaler(s, size, mode, mosaic, border, BG, max_batch=5)
        assert sc.canvases(batch) == len(want) and sc.canvas_bytes == want[0].size
        got = device_run(sc, bgr, st)
        what = (s, size, mode, mosaic, batch, border)
        assert np.array_equal(got, want), (what, np.argwhere(got != want)[:4])
        if border == 0 or batch == 5:
            each, whole = own_run(sc, bgr, st)
            assert np.array_equal(each, want) and np.array_equal(whole, want), what
        sc.close()


def test_odd_addresses_take_the_generic_path_and_give_the_same_bytes():
    """Source and destination one byte off alignment (and each alone): the generic items, without a fault, the same bytes, nothing outside the
    canvases.  16-pixel tiles: aligned pointers would take the vector path."""
    for mode, (s, size) in ((m, g) for m in ("area", "linear") for g in (((48, 16), (16, 8)), ((50, 18), (16, 6)), ((48, 16), (48, 16)))):
        bgr = TC.noise((5, s[1], s[0], 3), 9)
        st = TC.STATES
        p = emu.params(s, size, mode, (2, 2), 1, BG)
        want = emu.run(bgr, p, st, src_offset=1, dst_offset=1)
        assert (want.vector, want.outside, want.not_once) == (0, 0, 0) and emu.run(bgr, p, st).vector == TC.path_expected(size, mode, 0, 0) != 0
        sc = PP.FrameScaler(s, size, mode, (2, 2), 1, BG, max_batch=5)
        for so, do in ((1, 1), (1, 0), (0, 1), (8, 0), (0, 3), (0, 0)):
            got = device_run(sc, bgr, st, src_off=so, dst_off=do)
            assert np.array_equal(got, want.out), (mode, s, size, so, do)
        sc.close()


def test_wide_source_rows():
    """`area` from rows wider than one 16-byte piece per lane (2800 pixels for a 16-pixel tile: 8400 bytes, up to four pieces a lane), and from
    rows too wide to stage (6000 pixels: the generic items on aligned pointers)."""
    for (w, h), size, path in (((2800, 6), (16, 3), 2), ((5400, 2), (16, 1), 2), ((6000, 2), (16, 1), 0)):
        bgr = TC.noise((3, h, w, 3), w)
        st = TC.STATES[:3]
        border = 1 if size[1] > 2 else 0
        r = emu.run(bgr, emu.params((w, h), size, "area", (2, 1), border, BG), st)
        assert r.vector == path and (r.outside, r.misaligned, r.not_once) == (0, 0, 0)
        sc = PP.FrameScaler((w, h), size, "area", (2, 1), border, BG, max_batch=3)
        got = device_run(sc, bgr, st)
        assert np.array_equal(got, r.out), (w, h, np.argwhere(got != r.out)[:4])
        sc.close()


@pytest.fixture(scope="module")
def cam16():
    import bench
    return bench.cam_frames(16, 41)


@pytest.mark.parametrize("mode", ("area", "linear"))
def test_camera_size(cam16, mode):
    """16 frames of 1280x720, the vector paths' home (staged blocks for `area`, vector items for `linear`): a 640x360 reduction per frame, and
    a 4x4 mosaic of 320x180 tiles with a border of 2."""
    st = (np.arange(16) % 5).astype(np.int32)
    for size, mosaic, border in (((640, 360), (1, 1), 0), ((320, 180), (4, 4), 2)):
        r = emu.run(cam16, emu.params((1280, 720), size, mode, mosaic, border, BG), st)
        assert r.vector == (2 if mode == "area" else 1) and (r.outside, r.misaligned, r.not_once) == (0, 0, 0) and r.guard_ok
        sc = PP.FrameScaler((1280, 720), size, mode, mosaic, border, BG, max_batch=16)
        got = device_run(sc, cam16, st)
        assert np.array_equal(got, r.out), (mode, size, mosaic, np.argwhere(got != r.out)[:4])
        sc.close()


def test_refusals_by_name():
    def refused(match, fn, *a, **kw):
        with pytest.raises(RuntimeError, match=match) as ei:
            fn(*a, **kw)
        assert ei.value.code == INVALID
    refused("adas_scale_create: max_batch 0", PP.FrameScaler, (48, 16), (16, 8), max_batch=0)
    sc = PP.FrameScaler((48, 16), (16, 8), mosaic=(2, 1), max_batch=4)
    src = filled(5 * 48 * 16 * 3)
    refused("adas_scale_run: batch 5, the handle holds 4 frames", sc.run_device, src.ptr, 5)
    refused("adas_scale_fetch: canvas 0 was not written", sc.canvas, 0)
    refused("adas_scale_fetch_all: 1 canvases were not written", sc.fetch_all, 1)
    sc.run_device(src.ptr, 2)
    refused("adas_scale_fetch: canvas 1 was not written", sc.canvas, 1)
    refused("adas_scale_fetch_all: 2 canvases were not written", sc.fetch_all, 3)
    assert sc.canvas(0).shape == (8, 32, 3) and (sc.canvas(0) == FILL).all()
    with pytest.raises(ValueError, match="at least %d bytes" % sc.canvas_bytes):
        sc.fetch_all(1, out=np.zeros(sc.canvas_bytes - 1, np.uint8))
    assert sc.device_view()
    src.free()
    sc.close()


# ------------------------------------------------------------------------------------------------ the fused step
@pytest.fixture(scope="module")
def lane_model(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("scale_lane") / "lanes.hipm")
    M.build("ufldv2_res18", wsrc=TJ.PrescribedLanes(), **TJ.LANE_KW).save(path)
    return path


@pytest.fixture(scope="module")
def models(tmp_path_factory, lane_model):
    """The lane model of the JPEG and YUV suites and, because analysis= needs one, the detector of the panels suite."""
    import bench
    import netutil
    d = tmp_path_factory.mktemp("scale")
    lane = lane_model
    seam = np.concatenate([netutil.coco_like_frames(2, seed=40 + i) for i in range(2)])
    det, _, _ = bench.build_detector(M, TP.CE, "yolov8n", seam, str(d), "a", target_per_frame=25.0, capacity=TP.MAXC)
    cam = [bench.cam_frames(2, 500 + i) for i in range(2)]
    return det, lane, cam


def step_kw():
    car = A.SingleCamDistanceMeasure.RefSizeDict["car"][0]
    return dict(TJ.pipeline_kw(), box_score=TP.BOX_SCORE, max_candidates=TP.MAXC, analysis=dict(ref_height=[car] * 80))


def test_fused_step_canvas_jpeg_yuv_replay_and_launch_count(models):
    """Detector, lanes, analysis and overlay in graph mode with a 2x2 mosaic of 320x180 tiles, border 1, and both consumers: on the step that
    captures and on the one that replays, scaled_image is the emulation applied to overlay_image of every frame with the collision states
    the step fetched, scaled_jpeg and scaled_yuv the encoders' emulations of that canvas.  The stage is one launch, its JPEG three, its YUV
    one; scale=None leaves the count of a pipeline built without the option."""
    det, lane, cam = models
    kw = step_kw()
    sc = dict(size=(320, 180), mosaic=(2, 2), border=1, background=BG)
    full = PL.AdasPipeline(det, lane, overlay=dict(), scale=dict(sc, jpeg=dict(quality=80), yuv=dict(format="nv12")), **kw)
    only = PL.AdasPipeline(det, lane, overlay=dict(), scale=dict(sc, mode="linear", source="frames"), **kw)
    none = PL.AdasPipeline(det, lane, overlay=dict(), scale=None, **kw)
    plain = PL.AdasPipeline(det, lane, overlay=dict(), **kw)
    assert none.scaler is None and full.scaler.canvas_hw == (360, 640) and full.scaled_yuv_writer.format == "nv12"
    dev = [L.DeviceBuffer.from_array(c) for c in cam]
    p_area = emu.params((1280, 720), (320, 180), "area", (2, 2), 1, BG)
    p_lin = emu.params((1280, 720), (320, 180), "linear", (2, 2), 1, BG)
    first = None
    for k in range(3):      # step 0 and 1 capture (two input buffers), step 2 replays the first capture
        for p in (full, only, none, plain):
            p.step_frames(dev[k % 2].ptr, (720, 1280), 0.6)
            p.sync()
        drawn = np.stack([full.overlay_image(s) for s in range(2)])
        states = np.array([full.analysis._collision.index(full.analysis.fetch_frame(s)["collision_msg"]) for s in range(2)], np.int32)
        want = emu.scale(drawn, p_area, states)
        got = full.scaled_image(0)
        assert np.array_equal(got, want[0]), (k, np.argwhere(got != want[0])[:4])
        assert (got[180:] == BG).all() and (got[0, :320] == emu.DEFAULT_COLORS[states[0]]).all()
        assert full.scaled_jpeg(0) == enc_emu.encode(want[0], 80), k
        n, flags = full.scaled_jpeg_lengths()
        assert list(n) == [len(full.scaled_jpeg(0))] and list(flags) == [0]
        yuv = yuv_emu.convert(want, yuv_emu.params("nv12", 640, 360))
        assert np.array_equal(full.scaled_yuv(0), yuv) and np.array_equal(full.scaled_yuv_all(), yuv), k
        assert np.array_equal(only.scaled_image(0), emu.scale(cam[k % 2], p_lin, states)[0]), k
        assert np.array_equal(drawn[0], plain.overlay_image(0)) and np.array_equal(drawn[1], none.overlay_image(1))      # the stage writes no frame
        if k == 0:
            first = (got.copy(), full.scaled_jpeg(0), full.scaled_yuv(0).copy())
        if k == 2:          # the replay of step 0's capture on step 0's frames
            assert np.array_equal(got, first[0]) and full.scaled_jpeg(0) == first[1] and np.array_equal(full.scaled_yuv(0), first[2])
    assert none.graph_kernels() == plain.graph_kernels()
    assert only.graph_kernels() == plain.graph_kernels() + 1
    assert full.graph_kernels() == plain.graph_kernels() + 1 + 3 + 1
    for name in ("scaled_image", "scaled_jpeg", "scaled_jpeg_lengths", "scaled_yuv", "scaled_yuv_all"):
        with pytest.raises(ValueError, match="without scale="):
            getattr(none, name)()
    with pytest.raises(ValueError, match="without scale= jpeg"):
        only.scaled_jpeg(0)
    for o in (full, only, none, plain):
        o.close()
    for b in dev:
        b.free()


def test_micro_batching_fills_the_tiles_in_frame_order(lane_model):
    """micro_batch=2 on two streams without a detector: four frames per step, frame b * n_streams + s in cell b * n_streams + s of a 3x1
    mosaic, so the second canvas holds one frame and two background cells."""
    import bench
    frames = bench.cam_frames(4, 77)
    p = PL.AdasPipeline(None, lane_model, scale=dict(size=(160, 90), mosaic=(3, 1), source="frames"), **dict(TJ.pipeline_kw(), micro_batch=2))
    dev = L.DeviceBuffer.from_array(frames)
    p.step_frames(dev.ptr, (720, 1280), 0.6)
    p.sync()
    want = emu.scale(frames, emu.params((1280, 720), (160, 90), "area", (3, 1)))
    assert want.shape == (2, 90, 480, 3) and (want[1, :, 160:] == 0).all()
    for k in range(2):
        assert np.array_equal(p.scaled_image(k), want[k]), k
    p.close()
    dev.free()


def test_attach_refusals(models):
    det, lane, cam = models
    kw = step_kw()
    p = PL.AdasPipeline(det, lane, overlay=dict(), **kw)
    q = PL.AdasPipeline(None, lane, **TJ.pipeline_kw())          # no overlay, no analysis
    good = PP.FrameScaler((1280, 720), (320, 180), mosaic=(2, 2), max_batch=2)
    bordered = PP.FrameScaler((1280, 720), (320, 180), border=2, max_batch=2)
    small = PP.FrameScaler((640, 360), (320, 180), max_batch=2)
    one = PP.FrameScaler((1280, 720), (320, 180), max_batch=1)
    jpeg_ok, jpeg_wrong = PP.JpegEncoder(640, 360, 80, 1), PP.JpegEncoder(320, 180, 80, 1)
    yuv_ok, yuv_wrong = PP.YuvWriter("nv12", 640, 360, max_batch=1), PP.YuvWriter("nv12", 640, 352, max_batch=1)
    plain_jpeg, plain_yuv = PP.JpegEncoder(320, 180, 80, 1), PP.YuvWriter("nv12", 320, 180, max_batch=1)
    lib = L.lib()
    for fn, match in ((lambda: lib.adas_pipeline_attach_scale_jpeg(p.h, jpeg_ok.h), "adas_pipeline_attach_scale_jpeg: no scale handle is attached"),
                      (lambda: lib.adas_pipeline_attach_scale_yuvout(p.h, yuv_ok.h), "adas_pipeline_attach_scale_yuvout: no scale handle is attached"),
                      (lambda: lib.adas_pipeline_attach_scale(p.h, small.h, 0), "created for 640x360 frames, the attached overlay draws 1280x720"),
                      (lambda: lib.adas_pipeline_attach_scale(p.h, one.h, 0), "the scale handle holds 1 frames, a step has 2"),
                      (lambda: lib.adas_pipeline_attach_scale(q.h, good.h, 0), "the overlay source needs an attached overlay handle"),
                      (lambda: lib.adas_pipeline_attach_scale(q.h, bordered.h, 1), "a border of 2 pixels needs an attached analysis handle"),
                      (lambda: lib.adas_pipeline_attach_scale(p.h, good.h, 2), "adas_pipeline_attach_scale: unknown source 2")):
        with pytest.raises(RuntimeError, match=match) as ei:
            L.check(fn())
        assert ei.value.code == INVALID
    L.check(lib.adas_pipeline_attach_scale(p.h, good.h, 0))
    for fn, match in ((lambda: lib.adas_pipeline_attach_scale_jpeg(p.h, jpeg_wrong.h), "the JPEG handle was created for 320x180 frames, the scale handle's canvas is 640x360"),
                      (lambda: lib.adas_pipeline_attach_scale_yuvout(p.h, yuv_wrong.h),
                       "the YUV output handle was created for 640x352 frames, the scale handle's canvas is 640x360")):
        with pytest.raises(RuntimeError, match=match) as ei:
            L.check(fn())
        assert ei.value.code == INVALID
    L.check(lib.adas_pipeline_attach_scale_jpeg(p.h, jpeg_ok.h))
    L.check(lib.adas_pipeline_attach_scale_yuvout(p.h, yuv_ok.h))
    L.check(lib.adas_pipeline_attach_scale(p.h, bordered.h, 1))          # one tile per canvas now: two canvases a step
    for fn, match in ((lambda: lib.adas_pipeline_attach_scale_jpeg(p.h, plain_jpeg.h), "the JPEG handle holds 1 frames, a step has 2 canvases"),
                      (lambda: lib.adas_pipeline_attach_scale_yuvout(p.h, plain_yuv.h), "the YUV output handle holds 1 frames, a step has 2 canvases")):
        with pytest.raises(RuntimeError, match=match) as ei:
            L.check(fn())
        assert ei.value.code == INVALID
    L.check(lib.adas_pipeline_attach_scale(p.h, None, 0))                # detaches its consumers too
    L.check(lib.adas_pipeline_attach_scale(q.h, small.h, 1))             # the frames' size is known at the step: refused there, by name
    d = L.DeviceBuffer.from_array(np.zeros((2, 720, 1280, 3), np.uint8))
    with pytest.raises(RuntimeError, match="the attached scale handle was created for 640x360 frames, the step has 1280x720") as ei:
        q.step_frames(d.ptr, (720, 1280), 0.6)
    assert ei.value.code == INVALID
    L.check(lib.adas_pipeline_attach_scale(q.h, good.h, 1))
    with pytest.raises(RuntimeError, match="no frame to scale") as ei:      # seam tensors with the stage attached
        q.step(None, d.ptr)
    assert ei.value.code == INVALID
    q.step_frames(d.ptr, (720, 1280), 0.6)
    q.sync()
    n_with = q.graph_kernels()
    L.check(lib.adas_pipeline_attach_scale(q.h, None, 0))                # detached: the step is the plain one again
    q.step_frames(d.ptr, (720, 1280), 0.6)
    q.sync()
    assert q.graph_kernels() == n_with - 1
    for o in (p, q, good, bordered, small, one, jpeg_ok, jpeg_wrong, yuv_ok, yuv_wrong, plain_jpeg, plain_yuv):
        o.close()
    d.free()
