"""GPU: the YUV output (csrc/yuvout_kernels.hip) through the C ABI, postproc.YuvWriter and the fused step: every byte equals the host build of
the same work items (tests/emu_yuvout_api.py, which tests/test_yuvout_cpu.py pins to tests/yuvout_ref.py), and no byte that belongs to no
plane row is written.  Sizes, layouts and the sentinel scheme are the CPU suite's."""
import importlib
import itertools

import numpy as np
import pytest

from conftest import load_pkg
import emu_jpeg_api as enc_emu
import emu_yuvout_api as emu
import yuvout_ref as ref
import test_gpu_jpeg as TJ
import test_yuvout_cpu as TC

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")

INVALID = -1        # ADAS_ERR_INVALID
FILL = emu.SENTINEL
GUARD = 64          # a multiple of 16: a buffer's payload keeps the allocation's alignment


def filled(n):
    b = L.DeviceBuffer(n)
    L.check(L.lib().adas_memcpy_h2d(b.ptr, L.ptr(np.full(n, FILL, np.uint8)), n))
    return b


def device_run(wr, bgr, src_off=0, dst_off=0):
    """bgr [n][h][w][3] uploaded into an allocation of exactly its size plus guard bands, src_off bytes off its alignment; converted into such
    an allocation of exactly batch_bytes(n), dst_off bytes off, pre-filled with the sentinel.  -> uint8 [batch_bytes(n)]; the bands are checked."""
    bgr = np.ascontiguousarray(bgr)
    n, ns, nd = len(bgr), bgr.size, wr.batch_bytes(len(bgr))
    src = filled(ns + 2 * GUARD + 16)
    L.check(L.lib().adas_memcpy_h2d(src.ptr + GUARD + src_off, L.ptr(bgr), ns))
    dst = filled(nd + 2 * GUARD + 16)
    wr.run_device(src.ptr + GUARD + src_off, n, d_dst=dst.ptr + GUARD + dst_off)
    raw = dst.download((nd + 2 * GUARD + 16,), np.uint8)
    lo = GUARD + dst_off
    assert (raw[:lo] == FILL).all() and (raw[lo + nd:] == FILL).all(), "bytes outside the batch's frames were written"
    src.free()
    dst.free()
    return raw[lo:lo + nd]


def own_run(wr, bgr):
    """The same frames into the handle's own buffer: (the per-frame fetches [n][frame_bytes], fetch_all's bytes)"""
    dev = L.DeviceBuffer.from_array(np.ascontiguousarray(bgr))
    wr.run_device(dev.ptr, len(bgr))
    frames = np.stack([wr.frame(f) for f in range(len(bgr))])
    whole = wr.fetch_all(len(bgr)).copy()
    dev.free()
    return frames, whole


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_device_equals_emulation(fmt):
    """Every matrix, chroma mode, size and layout of the CPU suite at batch 3 (a wrong frame stride shows in frames 1 and 2) into a caller's
    buffer pre-filled with the sentinel: equal to the emulation's destination byte for byte, the untouched sentinel bytes included."""
    seed = 100
    for matrix, chroma, (w, h), kind in TC.grid():
        lay = ref.layout(fmt, w, h, kind)
        seed += 1
        bgr = TC.noise((3, h, w, 3), seed)
        want = emu.convert(bgr, emu.params(fmt, w, h, matrix, chroma, lay))
        wr = PP.YuvWriter(fmt, w, h, matrix, chroma, lay, max_batch=3)
        assert wr.batch_bytes(3) == ref.batch_bytes(fmt, w, h, lay, 3) == len(want)
        got = device_run(wr, bgr)
        assert np.array_equal(got, want), ((fmt, matrix, chroma, w, h, kind), np.argwhere(got != want)[:4])
        wr.close()


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_camera_size(fmt):
    """1280x720, the vector path's home: one camera-like frame per matrix and chroma mode."""
    import bench
    bgr = bench.cam_frames(1, 41)
    for matrix, chroma in (("video", "mean"), ("full", "first"), ("full", "mean")):
        p = emu.params(fmt, 1280, 720, matrix, chroma)
        r = emu.run(bgr, p)
        assert r.vector == 1 and (r.outside, r.misaligned, r.off_row) == (0, 0, 0)
        wr = PP.YuvWriter(fmt, 1280, 720, matrix, chroma, max_batch=1)
        got = device_run(wr, bgr)
        assert np.array_equal(got, r.out), (fmt, matrix, chroma, np.argwhere(got != r.out)[:4])
        wr.close()


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_odd_base_and_stride(fmt):
    """Source and destination one byte off an aligned address and an odd frame_stride: the generic cells, without a fault, the same bytes,
    nothing outside the plane rows."""
    for (matrix, chroma), (w, h) in itertools.product((("video", "mean"), ("full", "first")), TC.GEOMETRIES):
        lay = ref.layout(fmt, w, h, "odd")
        assert lay["frame_stride"] % 2 == 1
        bgr = TC.noise((3, h, w, 3), 7 * w + h)
        want = emu.run(bgr, emu.params(fmt, w, h, matrix, chroma, lay), src_offset=1, dst_offset=1)
        assert (want.vector, want.outside, want.off_row) == (0, 0, 0)
        wr = PP.YuvWriter(fmt, w, h, matrix, chroma, lay, max_batch=3)
        got = device_run(wr, bgr, src_off=1, dst_off=1)
        assert np.array_equal(got, want.out), (fmt, matrix, chroma, w, h)
        wr.close()
    # a tight, aligned layout from or to an odd address takes the generic cells too
    bgr = TC.noise((3, 8, 48, 3), 5)
    wr = PP.YuvWriter(fmt, 48, 8, max_batch=3)
    want = emu.convert(bgr, emu.params(fmt, 48, 8))
    for so, do in ((1, 0), (0, 1), (8, 0), (0, 3)):
        assert np.array_equal(device_run(wr, bgr, src_off=so, dst_off=do), want), (fmt, so, do)
    wr.close()


def test_caller_buffer_own_buffer_and_fetches():
    """d_dst given by the caller holds what the handle's own buffer holds; fetch_all (into a fresh array and into pinned memory) is the
    per-frame fetches at their frame strides; planes() are views of those bytes."""
    for fmt, (w, h, kind) in itertools.product(ref.FORMATS, ((48, 8, "tight"), (34, 6, "odd"), (64, 2, "gap"))):
        lay = ref.layout(fmt, w, h, kind)
        wr = PP.YuvWriter(fmt, w, h, "video", "mean", lay, max_batch=3)
        bgr = TC.noise((3, h, w, 3), w + len(fmt))
        mine = device_run(wr, bgr)
        frames, whole = own_run(wr, bgr)
        mask = ref.plane_mask(fmt, w, h, lay, 3)
        assert np.array_equal(whole[mask], mine[mask]) and (whole[~mask] == 0).all(), (fmt, w, h, kind)     # the own buffer starts as zeros
        for f in range(3):
            o = f * lay["frame_stride"]
            assert np.array_equal(frames[f], whole[o:o + wr.frame_bytes]), (fmt, f)
        pinned = L.PinnedBuffer((wr.batch_bytes(3) + 5,))
        pinned.array[:] = 7
        two = wr.fetch_all(2, out=pinned.array)
        assert len(two) == wr.batch_bytes(2) and np.array_equal(two, whole[:wr.batch_bytes(2)]) and (pinned.array[wr.batch_bytes(2):] == 7).all()
        pinned.free()
        if fmt in ("yuyv", "uyvy"):
            with pytest.raises(ValueError, match="is packed"):
                wr.planes(0)
        else:
            Y, U, V = ref.planes(bgr, fmt)
            got = wr.planes(1)
            assert np.array_equal(got[0], Y[1])
            if fmt == "i420":
                assert np.array_equal(got[1], U[1]) and np.array_equal(got[2], V[1])
            else:
                a, b = (U[1], V[1]) if fmt == "nv12" else (V[1], U[1])
                assert np.array_equal(got[1][..., 0], a) and np.array_equal(got[1][..., 1], b)
        assert wr.device_view()
        wr.close()


def test_round_trip_of_a_grey_ramp():
    """YuvConverter(YuvWriter(x)) on a grey ramp returns greys (B = G = R) for both matrices: U = V = 128 out, and neutral chroma in."""
    ramp = np.repeat(((np.arange(48)[None, :] * 5 + np.arange(8)[:, None] * 2) % 256).astype(np.uint8)[None, :, :, None], 3, 3)     # [1][8][48][3]
    src = L.DeviceBuffer.from_array(ramp)
    for fmt, matrix, chroma in itertools.product(ref.FORMATS, ref.MATRICES, ref.CHROMA):
        wr = PP.YuvWriter(fmt, 48, 8, matrix, chroma)
        conv = PP.YuvConverter(fmt, 48, 8, matrix)
        wr.run_device(src.ptr, 1)
        conv.run_device(wr.device_view(), 1)
        back = conv.image(0)
        assert (back[..., 0] == back[..., 1]).all() and (back[..., 1] == back[..., 2]).all(), (fmt, matrix, chroma)
        # Y is rounded once on the way out and the grey once on the way back: `full` is the identity on greys, `video` moves a grey by at
        # most 0.5 * 255 / 219 + 0.5 < 1.1
        assert np.abs(back.astype(int) - ramp[0].astype(int)).max() <= (0 if matrix == "full" else 1), (fmt, matrix, chroma)
        wr.close()
        conv.close()
    src.free()


def test_refusals_by_name():
    def refused(match, fn, *a, **kw):
        with pytest.raises(RuntimeError, match=match) as ei:
            fn(*a, **kw)
        assert ei.value.code == INVALID
    refused("adas_yuvout_create: odd width", PP.YuvWriter, "nv12", 17, 4)
    refused("adas_yuvout_create: odd height for a 4:2:0 format", PP.YuvWriter, "nv12", 16, 5)
    refused("adas_yuvout_create: pitch shorter than a row", PP.YuvWriter, "uyvy", 16, 4, layout=dict(y_pitch=31))
    refused("adas_yuvout_create: max_batch 0", PP.YuvWriter, "nv12", 16, 4, max_batch=0)
    wr = PP.YuvWriter("uyvy", 16, 5, max_batch=2)          # an odd height is fine for 4:2:2
    src = filled(3 * 16 * 5 * 3)
    refused("adas_yuvout_run: batch 3, the handle holds 2 frames", wr.run_device, src.ptr, 3)
    refused("adas_yuvout_fetch: frame 0 was not written", wr.frame, 0)
    refused("adas_yuvout_fetch_all: 1 frames were not written", wr.fetch_all, 1)
    wr.run_device(src.ptr, 1)
    refused("adas_yuvout_fetch: frame 1 was not written", wr.frame, 1)
    refused("adas_yuvout_fetch_all: 2 frames were not written", wr.fetch_all, 2)
    assert wr.frame(0).shape == (16 * 5 * 2,)
    with pytest.raises(ValueError, match="at least %d bytes" % wr.batch_bytes(1)):
        wr.fetch_all(1, out=np.zeros(wr.batch_bytes(1) - 1, np.uint8))
    src.free()
    wr.close()


# ------------------------------------------------------------------------------------------------ the fused step
@pytest.fixture(scope="module")
def lane_model(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("yuvout") / "lanes.hipm")
    M.build("ufldv2_res18", wsrc=TJ.PrescribedLanes(), **TJ.LANE_KW).save(path)
    return path


@pytest.fixture(scope="module")
def cam():
    import bench
    return [bench.cam_frames(2, 500 + i) for i in range(2)]


def standalone(bgr, **kw):
    """A stand-alone conversion of [n][720][1280][3] on the device: [n][frame_bytes]"""
    wr = PP.YuvWriter(kw.pop("format", "i420"), 1280, 720, max_batch=len(bgr), **kw)
    frames, _ = own_run(wr, bgr)
    wr.close()
    return frames


def test_fused_step_frames_and_overlay_sources_next_to_jpeg_and_launch_count(lane_model, cam):
    """The lane branch with its overlay, in graph mode, on the step that captures and on the one that replays.  source="frames": yuv(f) is a
    stand-alone conversion of the camera frames (and the host build's).  source="overlay": one of overlay_image(f).  With jpeg= attached as
    well the JPEG bytes are those of a pipeline without yuv_output.  One more kernel with the stage; without it exactly those of a second
    pipeline built the same way."""
    kw = TJ.pipeline_kw()
    dev = [L.DeviceBuffer.from_array(c) for c in cam]
    pf = PL.AdasPipeline(None, lane_model, overlay=dict(), yuv_output=dict(format="nv12", source="frames"), **kw)
    po = PL.AdasPipeline(None, lane_model, overlay=dict(), jpeg=dict(quality=80), yuv_output=dict(format="i420", matrix="full", chroma="first"), **kw)
    pj = PL.AdasPipeline(None, lane_model, overlay=dict(), jpeg=dict(quality=80), **kw)
    none = PL.AdasPipeline(None, lane_model, overlay=dict(), jpeg=dict(quality=80), yuv_output=None, **kw)
    assert none.yuv_writer is None and (po.yuv_writer.format, po.yuv_writer.matrix, po.yuv_writer.chroma) == ("i420", "full", "first")
    for k in range(3):      # step 0 and 1 capture (two input buffers), step 2 replays the first capture
        for p in (pf, po, pj, none):
            p.step_frames(dev[k % 2].ptr, (720, 1280), 0.6)
            p.sync()
        want_f = standalone(cam[k % 2], format="nv12")
        drawn = np.stack([po.overlay_image(s) for s in range(2)])
        want_o = standalone(drawn, format="i420", matrix="full", chroma="first")
        if k == 0:
            assert np.array_equal(want_f.ravel(), emu.convert(cam[0], emu.params("nv12", 1280, 720)))
        for s in range(2):
            assert np.array_equal(drawn[s], pj.overlay_image(s)) and (drawn[s] != cam[k % 2][s]).any()
            assert np.array_equal(pf.yuv(s), want_f[s]), (k, s)
            assert np.array_equal(po.yuv(s), want_o[s]), (k, s)
            assert po.jpeg(s) == pj.jpeg(s) == none.jpeg(s) == enc_emu.encode(drawn[s], 80), (k, s)
        assert np.array_equal(pf.yuv_all(), want_f.ravel()) and np.array_equal(po.yuv_all(), want_o.ravel())
        assert np.array_equal(dev[k % 2].download(cam[k % 2].shape, np.uint8), cam[k % 2])      # the step's frames are not written
    assert none.graph_kernels() == pj.graph_kernels() and po.graph_kernels() == pj.graph_kernels() + 1
    with pytest.raises(ValueError, match="without yuv_output="):
        none.yuv(0)
    with pytest.raises(ValueError, match="without yuv_output="):
        pj.yuv_all()
    for o in (pf, po, pj, none):
        o.close()
    for b in dev:
        b.free()


def test_micro_batching_delivers_the_frames_in_input_order(lane_model):
    """micro_batch=2 on two streams: four frames per step, frame b * n_streams + s of the input at that index of yuv() and yuv_all()."""
    import bench
    frames = bench.cam_frames(4, 77)
    kw = dict(TJ.pipeline_kw(), micro_batch=2)
    p = PL.AdasPipeline(None, lane_model, yuv_output=dict(format="uyvy", source="frames"), **kw)
    dev = L.DeviceBuffer.from_array(frames)
    p.step_frames(dev.ptr, (720, 1280), 0.6)
    p.sync()
    want = standalone(frames, format="uyvy")
    assert len({w.tobytes() for w in want}) == 4
    for f in range(4):
        assert np.array_equal(p.yuv(f), want[f]), f
    assert np.array_equal(p.yuv_all(), want.ravel())
    p.close()
    dev.free()


def test_pipeline_refusals(lane_model):
    kw = TJ.pipeline_kw()
    p = PL.AdasPipeline(None, lane_model, overlay=dict(), **kw)
    q = PL.AdasPipeline(None, lane_model, **kw)
    small, one, good = PP.YuvWriter("nv12", 640, 360, max_batch=2), PP.YuvWriter("nv12", 1280, 720, max_batch=1), PP.YuvWriter("nv12", 1280, 720, max_batch=2)
    attach = L.lib().adas_pipeline_attach_yuvout
    for fn, match in ((lambda: L.check(attach(p.h, small.h, 0)), "created for 640x360 frames, the attached overlay draws 1280x720"),
                      (lambda: L.check(attach(p.h, one.h, 0)), "the YUV output handle holds 1 frames, a step has 2"),
                      (lambda: L.check(attach(q.h, good.h, 0)), "the overlay source needs an attached overlay handle"),
                      (lambda: L.check(attach(p.h, good.h, 2)), "unknown source 2")):
        with pytest.raises(RuntimeError, match=match) as ei:
            fn()
        assert ei.value.code == INVALID
    L.check(attach(q.h, small.h, 1))                 # the frames' size is known at the step: refused there, by name
    d = L.DeviceBuffer.from_array(np.zeros((2, 720, 1280, 3), np.uint8))
    with pytest.raises(RuntimeError, match="the attached YUV output handle was created for 640x360 frames, the step has 1280x720") as ei:
        q.step_frames(d.ptr, (720, 1280), 0.6)
    assert ei.value.code == INVALID
    L.check(attach(q.h, good.h, 1))
    with pytest.raises(RuntimeError, match="no frame to convert") as ei:      # seam tensors with the stage attached
        q.step(None, d.ptr)
    assert ei.value.code == INVALID
    q.step_frames(d.ptr, (720, 1280), 0.6)
    q.sync()
    n_with = q.graph_kernels()
    L.check(attach(q.h, None, 0))                    # detached: the step is the plain one again
    q.step_frames(d.ptr, (720, 1280), 0.6)
    q.sync()
    assert q.graph_kernels() == n_with - 1
    for o in (p, q, small, one, good):
        o.close()
    d.free()
