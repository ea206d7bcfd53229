"""GPU: the rectification stage (csrc/remap_kernels.hip) through the C ABI, postproc.FrameRemapper and the fused step: every map entry and
every frame byte equals the host build of the same work items (tests/emu_remap_api.py, which tests/test_remap_cpu.py pins to
tests/remap_ref.py), and no byte outside the batch's frames is written.  Shapes and lenses are the CPU suite's."""
import importlib

import numpy as np
import pytest

from conftest import load_pkg
import emu_jpeg_api as enc_emu
import emu_remap_api as emu
import remap_ref as ref
import yuv_ref
import emu_yuv_api
import test_gpu_jpeg as TJ
import test_remap_cpu as TC

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")

FILL = 0xA5
GUARD = 64          # a multiple of 16: a buffer's payload keeps the allocation's alignment


def filled(n):
    b = L.DeviceBuffer(n)
    L.check(L.lib().adas_memcpy_h2d(b.ptr, L.ptr(np.full(n, FILL, np.uint8)), n))
    return b


def device_run(rm, frames, batch=None, dst_off=0):
    """frames through the handle into an allocation of exactly `batch` frames plus guard bands, dst_off bytes off its alignment; the bands are
    checked.  -> [batch][dst_h][dst_w][3]"""
    batch = len(frames) if batch is None else batch
    nd = batch * rm.dst_hw[0] * rm.dst_hw[1] * 3
    src = L.DeviceBuffer.from_array(frames)
    dst = filled(nd + 2 * GUARD + 16)
    rm.run(src.ptr, batch, dst.ptr + GUARD + dst_off)
    raw = dst.download((nd + 2 * GUARD + 16,), np.uint8)
    lo = GUARD + dst_off
    assert (raw[:lo] == FILL).all() and (raw[lo + nd:] == FILL).all(), "bytes outside the batch's frames were written"
    src.free()
    dst.free()
    return raw[lo:lo + nd].reshape((batch,) + rm.dst_hw + (3,))


@pytest.mark.parametrize("lens", TC.MODEL_LENSES)
def test_built_maps_equal_the_host_build(lens):
    """the build kernel at 64x48 and at the four small shapes, three maps in one handle: bit for bit"""
    cams = [dict(K=TC.MODEL_K, D=ref.LENSES[lens]), dict(K=TC.MODEL_K, D=ref.LENSES[lens], new_K=(36.0, 38.0, 30.0, 25.0), R=np.eye(3)),
            dict(K=TC.MODEL_K)]
    rm = PP.FrameRemapper(TC.MODEL_HW, 3, cameras=cams)
    for m, cam in enumerate(cams):
        xy, frac = rm.fetch_map(m)
        want_xy, want_frac = emu.build_map(dst_hw=TC.MODEL_HW, **cam)
        assert np.array_equal(xy, want_xy) and np.array_equal(frac, want_frac), (lens, m)
    rm.set_camera(-1, **cams[1])        # every map at once
    for m in range(3):
        assert all(np.array_equal(a, b) for a, b in zip(rm.fetch_map(m), emu.build_map(dst_hw=TC.MODEL_HW, **cams[1])))
    rm.close()
    for dst_hw in TC.DST_HWS:
        cam = TC.small_camera(dst_hw, lens, 1)
        rm = PP.FrameRemapper(TC.SRC_HW, 1, cameras=[cam], dst_hw=dst_hw)
        assert all(np.array_equal(a, b) for a, b in zip(rm.fetch_map(0), emu.build_map(dst_hw=dst_hw, **cam))), (lens, dst_hw)
        rm.close()


@pytest.mark.parametrize("dst_hw", TC.DST_HWS)
def test_frames_equal_the_host_build(dst_hw):
    """3 streams, 2 maps, micro-batch 2 at the 36..39-wide shapes, maps built on the device, at three byte phases of the destination"""
    frames = TC.noise((6,) + TC.SRC_HW + (3,), dst_hw[1])
    for lens in ("barrel", "pincushion"):
        cams = [TC.small_camera(dst_hw, lens, m) for m in range(2)]
        rm = PP.FrameRemapper(TC.SRC_HW, 3, cameras=cams, dst_hw=dst_hw, max_batch=6)
        want = emu.remap(frames, [emu.build_map(dst_hw=dst_hw, **c) for c in cams], None, 3)
        for off in (0, 1, 2):
            assert np.array_equal(device_run(rm, frames, dst_off=off), want), (dst_hw, lens, off)
        rm.close()


def test_crafted_map_and_stream_table():
    """the caller's map of saturated and edge entries at 36x36, and U5's table through assign"""
    maps = [ref.crafted_map(TC.SRC_HW, (36, 36), m) for m in range(2)]
    frames = TC.noise((6,) + TC.SRC_HW + (3,), 11)
    frames[:, -1, -3:] = 255
    rm = PP.FrameRemapper(TC.SRC_HW, 3, maps=maps, dst_hw=(36, 36), max_batch=6)
    assert all(np.array_equal(a, b) for a, b in zip(rm.fetch_map(1), maps[1]))
    for off in (0, 3):
        assert np.array_equal(device_run(rm, frames, dst_off=off), emu.remap(frames, maps, [0, 1, 1], 3)), off
    L.check(L.lib().adas_remap_assign(rm.h, 0, 1))
    L.check(L.lib().adas_remap_assign(rm.h, 2, 0))
    assert np.array_equal(device_run(rm, frames), emu.remap(frames, maps, [1, 1, 0], 3))
    rm.close()
    rm = PP.FrameRemapper(TC.SRC_HW, 3, maps=maps, stream_map=[1, 0, 1], dst_hw=(36, 36), max_batch=6)
    assert np.array_equal(device_run(rm, frames), emu.remap(frames, maps, [1, 0, 1], 3))
    rm.close()


@pytest.mark.parametrize("dst_hw", TC.DST_HWS + ((36, 36),))
def test_staged_form_equals_the_host_build(dst_hw, monkeypatch):
    """with ADAS_REMAP_STAGED=1 a 32x23 source (rows of 96 bytes) at an aligned pointer takes the LDS-staged kernel, at a pointer 4 bytes on
    the direct one, and without the switch the direct one: the host build's bytes every time"""
    monkeypatch.setenv("ADAS_REMAP_STAGED", "1")
    frames = TC.noise((6,) + TC.STAGED_SRC_HW + (3,), dst_hw[1] + 2)
    frames[:, -1, -3:] = 255
    sh, sw = TC.STAGED_SRC_HW
    for lens in ("barrel", "pincushion", "crafted"):
        if lens == "crafted":
            maps = [ref.crafted_map(TC.STAGED_SRC_HW, dst_hw, m) for m in range(2)]
        else:
            maps = [ref.build_map((20.0, 20.0, (sw - 1) * 0.5, (sh - 1) * 0.5), ref.LENSES[lens],
                                  (20.0, 20.0, (dst_hw[1] - 1) * 0.5 + m, (dst_hw[0] - 1) * 0.5), dst_hw=dst_hw) for m in range(2)]
        r = emu.run(frames, maps, None, 3)
        assert r.staged and (r.outside, r.misaligned, r.not_once) == (0, 0, 0)
        rm = PP.FrameRemapper(TC.STAGED_SRC_HW, 3, maps=maps, dst_hw=dst_hw, max_batch=6)
        for off in (0, 1):
            assert np.array_equal(device_run(rm, frames, dst_off=off), r.out), (dst_hw, lens, off)
        src = L.DeviceBuffer(frames.nbytes + 16)
        L.check(L.lib().adas_memcpy_h2d(src.ptr + 4, L.ptr(frames), frames.nbytes))
        rm.run(src.ptr + 4, 6)
        assert all(np.array_equal(rm.fetch(f), r.out[f]) for f in range(6)), (dst_hw, lens, "unaligned source")
        src.free()
        with monkeypatch.context() as mp:
            mp.delenv("ADAS_REMAP_STAGED")
            assert np.array_equal(device_run(rm, frames), r.out), (dst_hw, lens, "direct")
        rm.close()


def test_staged_form_falls_back_where_the_box_does_not_fit(monkeypatch):
    """the CPU suite's 2048x12 source: the crafted map's workgroups gather directly, the corner map's are staged, in one launch"""
    monkeypatch.setenv("ADAS_REMAP_STAGED", "1")
    src_hw, dst_hw = (12, 2048), (8, 300)
    frames = TC.noise((2,) + src_hw + (3,), 13)
    xs, ys = np.meshgrid(np.arange(dst_hw[1]) % 40, np.arange(dst_hw[0]))
    maps = [ref.crafted_map(src_hw, dst_hw), (np.stack([xs, ys], -1).astype(np.int16), np.full(dst_hw, 5 * 32 + 7, np.uint16))]
    r = emu.run(frames, maps, n_streams=2)
    assert r.staged and r.direct_tiles == 4 and r.staged_loads > 0
    rm = PP.FrameRemapper(src_hw, 2, maps=maps, dst_hw=dst_hw)
    assert np.array_equal(device_run(rm, frames), r.out)
    rm.close()


def test_own_buffer_fetch_device_view_and_partial_batch():
    dst_hw = TC.DST_HWS[1]
    cam = TC.small_camera(dst_hw, "barrel")
    frames = TC.noise((4,) + TC.SRC_HW + (3,), 5)
    rm = PP.FrameRemapper(TC.SRC_HW, 2, cameras=[cam], dst_hw=dst_hw, max_batch=4)
    want = emu.remap(frames, [emu.build_map(dst_hw=dst_hw, **cam)], None, 2)
    src = L.DeviceBuffer.from_array(frames)
    nb = dst_hw[0] * dst_hw[1] * 3
    view = rm.device_view()
    L.check(L.lib().adas_memcpy_h2d(view, L.ptr(np.full(4 * nb, FILL, np.uint8)), 4 * nb))
    rm.run(src.ptr, 2)                  # batch < max_batch: the later frames stay untouched
    assert np.array_equal(rm.fetch(0), want[0]) and np.array_equal(rm.fetch(1), want[1])
    raw = np.empty(4 * nb, np.uint8)
    L.check(L.lib().adas_memcpy_d2h(L.ptr(raw), view, 4 * nb))
    assert np.array_equal(raw[:2 * nb].reshape((2,) + dst_hw + (3,)), want[:2]) and (raw[2 * nb:] == FILL).all()
    with pytest.raises(RuntimeError, match="adas_remap_fetch: frame 2 of the handle's own buffer was never written"):
        rm.fetch(2)
    rm.run(src.ptr)
    assert rm.device_view() == view and all(np.array_equal(rm.fetch(f), want[f]) for f in range(4))
    # a set call after a run orders itself behind it; the next run reads the new map
    rm.set_map(0, *ref.crafted_map(TC.SRC_HW, dst_hw))
    rm.run(src.ptr)
    assert np.array_equal(rm.fetch(3), emu.remap(frames, [ref.crafted_map(TC.SRC_HW, dst_hw)], None, 2)[3])
    src.free()
    rm.close()


def test_camera_size_frames_shared_and_distinct_maps(monkeypatch):
    """2 frames of 1280x720: one shared map, and two distinct maps; the direct kernel, and the staged one"""
    import bench
    frames = bench.cam_frames(2, 900)
    K = (900.0, 900.0, 639.5, 359.5)
    cams = [dict(K=K, D=(-0.25, 0.08, 0.0005, -0.0005)), dict(K=K, D=(-0.2, 0.05, 0.001, -0.001, 0.01, 0.1, 0.02, 0.003), new_K=(850.0, 850.0, 630.0, 365.0))]
    maps = [emu.build_map(dst_hw=(720, 1280), **c) for c in cams]
    for use in ([cams[0]], cams):
        rm = PP.FrameRemapper((720, 1280), 2, cameras=use)
        for m in range(len(use)):
            assert all(np.array_equal(a, b) for a, b in zip(rm.fetch_map(m), maps[m])), m
        want = emu.run(frames, maps[:len(use)], None, 2)
        assert want.staged and want.staged_loads > 0 and (want.outside, want.misaligned, want.not_once) == (0, 0, 0)      # rows of 3840 bytes; where the
        # lens bends a tile's rows over more than 16 KB of source, that workgroup gathers directly
        assert np.array_equal(device_run(rm, frames), want.out), len(use)
        assert np.array_equal(want.out, emu.run(frames, maps[:len(use)], None, 2, path=0).out)
        with monkeypatch.context() as mp:
            mp.setenv("ADAS_REMAP_STAGED", "1")
            assert np.array_equal(device_run(rm, frames), want.out), (len(use), "staged")
        rm.close()


def test_refusals_by_name():
    def refused(match, fn, *a, **kw):
        with pytest.raises(RuntimeError, match=match) as ei:
            fn(*a, **kw)
        assert ei.value.code == -1

    K = TC.MODEL_K
    refused("adas_remap_create: size outside 1..4320 rows x 1..16384 columns", PP.FrameRemapper, (4321, 64), 1, cameras=[dict(K=K)])
    refused("adas_remap_set_camera: zero focal length", PP.FrameRemapper, TC.MODEL_HW, 1, cameras=[dict(K=(0.0, 40.0, 31.5, 23.5))])
    refused("adas_remap_set_camera: singular new_K \\* R", PP.FrameRemapper, TC.MODEL_HW, 1, cameras=[dict(K=K, R=[1, 0, 0, 0, 1, 0, 0, 0, 0])])
    p = L.RemapParams(48, 64, 48, 64, 2, 2)
    h = L.C.c_void_p()
    L.check(L.lib().adas_remap_create(L.C.byref(p), 2, L.C.byref(h)))
    src = filled(2 * 48 * 64 * 3)
    refused("adas_remap_run: map 0 of stream 0 was never set", lambda: L.check(L.lib().adas_remap_run(h, src.ptr, 2, None, None)))
    xy, frac = emu.build_map(dst_hw=TC.MODEL_HW, K=K)
    L.check(L.lib().adas_remap_set_map(h, 0, L.ptr(xy), L.ptr(frac)))
    refused("adas_remap_run: map 1 of stream 1 was never set", lambda: L.check(L.lib().adas_remap_run(h, src.ptr, 2, None, None)))
    refused("adas_remap_fetch_map: map 1 was never set", lambda: L.check(L.lib().adas_remap_fetch_map(h, 1, L.ptr(xy), L.ptr(frac))))
    L.check(L.lib().adas_remap_run(h, src.ptr, 1, None, None))       # stream 0 alone is ready
    L.check(L.lib().adas_remap_assign(h, 1, 0))
    refused("adas_remap_run: batch 3, the handle holds 2 frames", lambda: L.check(L.lib().adas_remap_run(h, src.ptr, 3, None, None)))
    refused("adas_remap_set_map: map index outside the handle's table", lambda: L.check(L.lib().adas_remap_set_map(h, 2, L.ptr(xy), L.ptr(frac))))
    L.check(L.lib().adas_remap_run(h, src.ptr, 2, None, None))
    out = np.empty((48, 64, 3), np.uint8)
    L.check(L.lib().adas_remap_fetch(h, 1, L.ptr(out)))
    assert (out == FILL).all()                                      # the identity map
    L.lib().adas_remap_destroy(h)
    src.free()


# ------------------------------------------------------------------------------------------------ the fused step
@pytest.fixture(scope="module")
def lane_model(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("remap") / "lanes.hipm")
    M.build("ufldv2_res18", wsrc=TJ.PrescribedLanes(), **TJ.LANE_KW).save(path)
    return path


CAMS = [dict(K=(900.0, 900.0, 639.5, 359.5), D=(-0.25, 0.08, 0.0005, -0.0005)),
        dict(K=(880.0, 880.0, 650.0, 350.0), D=(-0.2, 0.05, 0.001, -0.001, 0.01, 0.1, 0.02, 0.003), new_K=(850.0, 850.0, 630.0, 365.0))]


def step_results(q):
    return [(q.decode.fetch(s), q.geometry.fetch(s), q.jpeg(s)) for s in range(2)]


def same_results(q, want, encoded, tag):
    """encoded: the emulation's JPEG of the frames the step must have read"""
    for s in range(2):
        lanes, geo, stream = want[s]
        assert q.decode.fetch(s) == lanes, (tag, s)
        g = q.geometry.fetch(s)
        assert g["area_status"] == geo["area_status"] and g["direction"] == geo["direction"] and g["curvature"] == geo["curvature"] and \
            g["offset"] == geo["offset"] and np.array_equal(g["area_points"], geo["area_points"]), (tag, s)
        assert all(np.array_equal(g["bird_points"][li], geo["bird_points"][li]) for li in range(4)), (tag, s)
        assert q.jpeg(s) == stream == encoded[s], (tag, s)


def test_fused_step_on_distorted_frames(lane_model):
    """The lane-only pipeline of test_gpu_yuv.py's fused test, in graph mode with the encoding stage on the step's frames so that what the
    step consumed is visible.  A pipeline with undistort= stepped on distorted frames (from the device and from the host, both staging
    buffers) returns what a plain pipeline returns on the host build's rectified frames, in every fetched field and in the step's JPEG;
    undistorted_image(f) is those frames; the captured step has the same kernel count.  Two identical cameras become one map."""
    import bench
    kw = TJ.pipeline_kw()
    jpeg = dict(quality=60, source="frames", capacity=400000)
    p = PL.AdasPipeline(None, lane_model, undistort=dict(cameras=CAMS), jpeg=jpeg, **kw)
    plain = PL.AdasPipeline(None, lane_model, jpeg=jpeg, **kw)
    assert p.remapper.n_maps == 2 and p.remapper.stream_map == [0, 1]
    maps = [emu.build_map(dst_hw=(720, 1280), **c) for c in CAMS]
    sets = [bench.cam_frames(2, 800 + i) for i in range(2)]
    rect = [emu.remap(s, maps, None, 2) for s in sets]
    enc = [[enc_emu.encode(f, 60) for f in r] for r in rect]
    want = []
    for k in range(2):
        dev = L.DeviceBuffer.from_array(rect[k])
        plain.step_frames(dev.ptr, (720, 1280), 0.6)
        plain.sync()
        want.append(step_results(plain))
        dev.free()
    n_kernels = plain.graph_kernels()
    assert want[0][0][2] != want[1][0][2]
    for k in (0, 1, 0):
        dev = L.DeviceBuffer.from_array(sets[k])
        p.step_frames(dev.ptr, (720, 1280), 0.6)
        p.sync()
        same_results(p, want[k], enc[k], ("device", k))
        assert all(np.array_equal(p.undistorted_image(f), rect[k][f]) for f in range(2)) and p.graph_kernels() == n_kernels
        dev.free()
    pinned = [L.PinnedBuffer(s.shape) for s in sets]
    for b, s in zip(pinned, sets):
        b.array[...] = s
    p.step_frames_host(pinned[0].ptr, (720, 1280), 0.6)
    p.step_frames_host(pinned[1].ptr, (720, 1280), 0.6)     # queued behind the first: the other staging buffer
    p.sync()
    same_results(p, want[1], enc[1], "host 1")
    p.step_frames_host(pinned[0].ptr, (720, 1280), 0.6)
    p.sync()
    same_results(p, want[0], enc[0], "host 0")
    assert p.graph_kernels() == n_kernels
    for b in pinned:
        b.free()
    shared = PL.AdasPipeline(None, lane_model, undistort=dict(cameras=[CAMS[0], dict(CAMS[0])]), jpeg=jpeg, **kw)
    assert shared.remapper.n_maps == 1 and shared.remapper.stream_map == [0, 0]
    dev = L.DeviceBuffer.from_array(sets[0])
    shared.step_frames(dev.ptr, (720, 1280), 0.6)
    shared.sync()
    assert np.array_equal(shared.undistorted_image(1), emu.remap(sets[0], maps[:1], None, 2)[1])
    bare = PL.AdasPipeline(None, lane_model, undistort=dict(camera=CAMS[0]), **kw)      # no other stage that checks the step's frame size first
    with pytest.raises(RuntimeError, match="the attached remap handle was created for 1280x720 frames, the step has 640x360"):
        bare.step_frames(dev.ptr, (360, 640), 0.6)
    dev.free()
    with pytest.raises(ValueError, match="without undistort="):
        plain.undistorted_image(0)
    for o in (p, plain, shared, bare):
        o.close()


def test_fused_step_from_distorted_nv12_frames(lane_model):
    """convert, rectify, step: yuv_input=nv12 in front of undistort= gives what the plain pipeline gives on the host build's rectification of
    the host build's conversion"""
    import bench
    kw = TJ.pipeline_kw()
    jpeg = dict(quality=60, source="frames", capacity=400000)
    p = PL.AdasPipeline(None, lane_model, yuv_input=dict(format="nv12"), undistort=dict(camera=CAMS[1]), jpeg=jpeg, **kw)
    plain = PL.AdasPipeline(None, lane_model, jpeg=jpeg, **kw)
    assert p.remapper.n_maps == 1 and p.remapper.stream_map == [0, 0]
    planes = yuv_ref.from_bgr(bench.cam_frames(2, 820), "nv12")
    bgr = emu_yuv_api.convert(planes, emu_yuv_api.params("nv12", 1280, 720), 2)
    rect = emu.remap(bgr, [emu.build_map(dst_hw=(720, 1280), **CAMS[1])], None, 2)
    dev = L.DeviceBuffer.from_array(rect)
    plain.step_frames(dev.ptr, (720, 1280), 0.6)
    plain.sync()
    want, enc = step_results(plain), [enc_emu.encode(f, 60) for f in rect]
    p.step_yuv_host(planes)
    p.sync()
    same_results(p, want, enc, "yuv host")
    assert np.array_equal(p.yuv_converter.image(1), bgr[1]) and np.array_equal(p.undistorted_image(1), rect[1])
    raw = L.DeviceBuffer.from_array(planes)
    p.step_yuv(raw.ptr)
    p.sync()
    same_results(p, want, enc, "yuv device")
    assert p.graph_kernels() == plain.graph_kernels()
    for b in (dev, raw):
        b.free()
    for o in (p, plain):
        o.close()


def test_pipeline_without_undistort_is_unchanged(lane_model):
    """no handle, and the outputs of a second such pipeline"""
    import bench
    kw = TJ.pipeline_kw()
    jpeg = dict(quality=60, source="frames", capacity=400000)
    a, b = (PL.AdasPipeline(None, lane_model, jpeg=jpeg, **kw) for _ in range(2))
    assert a.remapper is None and b.remapper is None
    frames = bench.cam_frames(2, 830)
    dev = L.DeviceBuffer.from_array(frames)
    for q in (a, b):
        q.step_frames(dev.ptr, (720, 1280), 0.6)
        q.sync()
    same_results(b, step_results(a), [enc_emu.encode(f, 60) for f in frames], "plain")
    assert a.graph_kernels() == b.graph_kernels()
    dev.free()
    for o in (a, b):
        o.close()
