"""GPU: the YUV conversion (csrc/yuv_kernels.hip) through the C ABI, postproc.YuvConverter and the fused step: every byte equals the host
build of the same work items (tests/emu_yuv_api.py, which tests/test_yuv_cpu.py pins to tests/yuv_ref.py), and no byte outside the batch's
frames is written.  Sizes, layouts and the guard-band scheme are the CPU suite's."""
import importlib
import itertools

import numpy as np
import pytest

from conftest import load_pkg
import emu_jpeg_api as enc_emu
import emu_yuv_api as emu
import yuv_ref as ref
import test_gpu_jpeg as TJ
import test_yuv_cpu as TC

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")

INVALID = -1        # ADAS_ERR_INVALID
FILL = 0xA5
GUARD = 64          # a multiple of 16: a buffer's payload keeps the allocation's alignment


def filled(n):
    b = L.DeviceBuffer(n)
    L.check(L.lib().adas_memcpy_h2d(b.ptr, L.ptr(np.full(n, FILL, np.uint8)), n))
    return b


def device_run(conv, buf, batch, src_off=0, dst_off=0, own=False):
    """`batch` frames of bytes buf, uploaded into an allocation of exactly their size plus guard bands, src_off bytes off its alignment;
    converted into the handle's own frames or into such an allocation, dst_off bytes off.  -> [batch][h][w][3]; the bands are checked."""
    need = conv.batch_bytes(batch)
    nd = batch * conv.height * conv.width * 3
    src = filled(need + 2 * GUARD + 16)
    L.check(L.lib().adas_memcpy_h2d(src.ptr + GUARD + src_off, L.ptr(np.ascontiguousarray(buf[:need])), need))
    if own:
        conv.run_device(src.ptr + GUARD + src_off, batch)
        got = np.stack([conv.image(f) for f in range(batch)])
    else:
        dst = filled(nd + 2 * GUARD + 16)
        conv.run_device(src.ptr + GUARD + src_off, batch, d_dst=dst.ptr + GUARD + dst_off)
        raw = dst.download((nd + 2 * GUARD + 16,), np.uint8)
        lo = GUARD + dst_off
        assert (raw[:lo] == FILL).all() and (raw[lo + nd:] == FILL).all(), "bytes outside the batch's frames were written"
        got = raw[lo:lo + nd].reshape(batch, conv.height, conv.width, 3)
        dst.free()
    src.free()
    return got


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_device_equals_emulation(fmt):
    """Every matrix, size and layout of the CPU suite at batch 3 (a wrong frame stride shows in frames 1 and 2), into the handle's own frames
    and into a caller's buffer: equal to the emulation and to each other."""
    seed = 100
    for matrix, (w, h), kind in itertools.product(ref.MATRICES, TC.GEOMETRIES, TC.KINDS):
        lay = ref.layout(fmt, w, h, kind)
        seed += 1
        buf = TC.noise(ref.source_bytes(fmt, w, h, lay, 3), seed)
        want = emu.convert(buf, emu.params(fmt, w, h, matrix, lay), 3)
        conv = PP.YuvConverter(fmt, w, h, matrix, lay, max_batch=3)
        assert conv.batch_bytes(3) == ref.source_bytes(fmt, w, h, lay, 3)
        tag = (fmt, matrix, w, h, kind)
        own = device_run(conv, buf, 3, own=True)
        assert np.array_equal(own, want), (tag, np.argwhere(own != want)[:4])
        mine = device_run(conv, buf, 3)
        assert np.array_equal(mine, want), (tag, np.argwhere(mine != want)[:4])
        conv.close()


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_camera_size(fmt):
    """1280x720, the vector path's home: three frames made from camera-like pictures, both matrices."""
    import bench
    buf = ref.from_bgr(bench.cam_frames(3, 41), fmt)
    for matrix in ref.MATRICES:
        p = emu.params(fmt, 1280, 720, matrix)
        r = emu.run(buf, p, 3)
        assert r.vector == 1 and (r.outside, r.misaligned) == (0, 0)
        conv = PP.YuvConverter(fmt, 1280, 720, matrix, max_batch=3)
        got = device_run(conv, buf, 3)
        assert np.array_equal(got, r.bgr), (fmt, matrix, np.argwhere(got != r.bgr)[:4])
        conv.close()


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_odd_base_and_stride(fmt):
    """Source and destination one byte off an aligned address and an odd frame_stride: the generic cells, without a fault, the same bytes,
    nothing outside the exact sizes."""
    for matrix, (w, h) in itertools.product(ref.MATRICES, TC.GEOMETRIES):
        lay = ref.layout(fmt, w, h, "odd")
        assert lay["frame_stride"] % 2 == 1
        buf = TC.noise(ref.source_bytes(fmt, w, h, lay, 3), 7 * w + h)
        want = emu.run(buf, emu.params(fmt, w, h, matrix, lay), 3, src_offset=1, dst_offset=1)
        assert (want.vector, want.outside) == (0, 0)
        conv = PP.YuvConverter(fmt, w, h, matrix, lay, max_batch=3)
        got = device_run(conv, buf, 3, src_off=1, dst_off=1)
        assert np.array_equal(got, want.bgr), (fmt, matrix, w, h)
        conv.close()
    # a tight, aligned layout from an odd address takes the generic cells too
    lay = ref.layout(fmt, 48, 8)
    buf = TC.noise(ref.source_bytes(fmt, 48, 8, lay, 3), 5)
    conv = PP.YuvConverter(fmt, 48, 8, max_batch=3)
    want = emu.convert(buf, emu.params(fmt, 48, 8), 3)
    for so, do in ((1, 0), (0, 1), (8, 0), (0, 3)):
        assert np.array_equal(device_run(conv, buf, 3, src_off=so, dst_off=do), want), (fmt, so, do)
    conv.close()


def test_run_host_equals_run_device():
    """run_host three times with different frames (both staging buffers, then the first again) and from pinned memory."""
    for fmt, (w, h, kind) in itertools.product(ref.FORMATS, ((48, 8, "tight"), (34, 6, "odd"), (1280, 720, "tight"))):
        lay = ref.layout(fmt, w, h, kind)
        conv = PP.YuvConverter(fmt, w, h, "video", lay, max_batch=2)
        n = conv.batch_bytes(2)
        pinned = L.PinnedBuffer((n,))
        for k in range(3):
            buf = TC.noise(n, 31 * k + w)
            want = device_run(conv, buf, 2)
            if k == 2:
                pinned.array[:] = buf
                conv.run_host(pinned.ptr, 2)
            else:
                conv.run_host(buf, 2)
            assert all(np.array_equal(conv.image(f), want[f]) for f in range(2)), (fmt, w, h, k)
        if w == 48:
            assert np.array_equal(want, emu.convert(buf, emu.params(fmt, w, h, "video", lay), 2))
        pinned.free()
        conv.close()


def test_refusals_by_name():
    def refused(match, fn, *a, **kw):
        with pytest.raises(RuntimeError, match=match) as ei:
            fn(*a, **kw)
        assert ei.value.code == INVALID
    refused("adas_yuv_create: odd width", PP.YuvConverter, "nv12", 17, 4)
    refused("adas_yuv_create: odd width", PP.YuvConverter, "yuyv", 17, 4)
    refused("adas_yuv_create: odd height for a 4:2:0 format", PP.YuvConverter, "nv12", 16, 5)
    refused("adas_yuv_create: pitch shorter than a row", PP.YuvConverter, "nv12", 16, 4, layout=dict(y_pitch=15))
    refused("adas_yuv_create: pitch shorter than a row", PP.YuvConverter, "uyvy", 16, 4, layout=dict(y_pitch=31))
    t = ref.layout("nv12", 16, 4)
    refused("adas_yuv_create: plane outside the frame", PP.YuvConverter, "nv12", 16, 4, layout=dict(frame_stride=t["frame_stride"] - 1))
    refused("adas_yuv_create: plane outside the frame", PP.YuvConverter, "nv12", 16, 4, layout=dict(u_offset=t["u_offset"] + 1))
    refused("adas_yuv_create: planes overlap", PP.YuvConverter, "nv12", 16, 4, layout=dict(u_offset=t["u_offset"] - 1, frame_stride=t["frame_stride"] + 8))
    refused("adas_yuv_create: max_batch 0", PP.YuvConverter, "nv12", 16, 4, max_batch=0)
    with pytest.raises(ValueError, match="format 'p010' is none of"):
        PP.YuvConverter("p010", 16, 4)
    with pytest.raises(ValueError, match="unknown keys \\['pitch'\\]"):
        PP.YuvConverter("nv12", 16, 4, layout=dict(pitch=16))
    conv = PP.YuvConverter("uyvy", 16, 5, max_batch=2)          # an odd height is fine for 4:2:2
    src = filled(conv.batch_bytes(3))
    refused("adas_yuv_run: batch 3, the handle holds 2 frames", conv.run_device, src.ptr, 3)
    refused("adas_yuv_run_host: batch 3, the handle holds 2 frames", conv.run_host, np.zeros(conv.batch_bytes(3), np.uint8), 3)
    refused("adas_yuv_fetch: frame 0 was not written", conv.image, 0)
    conv.run_device(src.ptr, 1)
    refused("adas_yuv_fetch: frame 1 was not written", conv.image, 1)
    assert conv.image(0).shape == (5, 16, 3)
    with pytest.raises(ValueError, match="at least %d bytes" % conv.batch_bytes(2)):
        conv.run_host(np.zeros(conv.batch_bytes(2) - 1, np.uint8), 2)
    src.free()
    conv.close()


# ------------------------------------------------------------------------------------------------ the fused step
@pytest.fixture(scope="module")
def lane_model(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("yuv") / "lanes.hipm")
    M.build("ufldv2_res18", wsrc=TJ.PrescribedLanes(), **TJ.LANE_KW).save(path)
    return path


def test_fused_step_from_nv12_frames(lane_model):
    """The lane-only pipeline of test_gpu_jpegdec.py's fused test, in graph mode with the encoding stage on the step's frames so that what
    the step consumed is visible.  step_yuv_host on the NV12 planes of two sets of camera frames, back to back (both staging buffers), then
    step_frames on an upload of the emulation's BGR of those planes, on the same pipeline and on a plain one: lanes, geometry and the
    step's JPEG are equal bit for bit, and so is the captured step's kernel count.  step_yuv from a device pointer gives the same."""
    import bench
    kw = TJ.pipeline_kw()
    jpeg = dict(quality=60, source="frames", capacity=400000)
    p = PL.AdasPipeline(None, lane_model, yuv_input=dict(format="nv12"), jpeg=jpeg, **kw)
    plain = PL.AdasPipeline(None, lane_model, jpeg=jpeg, **kw)
    assert plain.yuv_converter is None and p.yuv_converter.format == "nv12" and p.yuv_converter.matrix == "video"
    sets = [ref.from_bgr(bench.cam_frames(2, 700 + i), "nv12") for i in range(2)]
    assert all(len(s) == 2 * 1280 * 720 * 3 // 2 for s in sets)
    bgr = [emu.convert(s, emu.params("nv12", 1280, 720), 2) for s in sets]

    def results(q):
        return [(q.decode.fetch(s), q.geometry.fetch(s), q.jpeg(s)) for s in range(2)]

    def same(q, got, k):
        for s in range(2):
            lanes, geo, stream = got[s]
            assert q.decode.fetch(s) == lanes, (k, s)
            g = q.geometry.fetch(s)
            assert g["area_status"] == geo["area_status"] and g["direction"] == geo["direction"] and g["curvature"] == geo["curvature"] and \
                g["offset"] == geo["offset"] and np.array_equal(g["area_points"], geo["area_points"]), (k, s)
            assert all(np.array_equal(g["bird_points"][li], geo["bird_points"][li]) for li in range(4)), (k, s)
            assert q.jpeg(s) == stream == enc_emu.encode(bgr[k][s], 60), (k, s)

    p.step_yuv_host(sets[0])
    p.step_yuv_host(sets[1])            # queued behind the first: the other staging buffer
    p.sync()
    second = results(p)
    n_kernels = p.graph_kernels()
    assert np.array_equal(p.yuv_converter.image(1), bgr[1][1])
    p.step_yuv_host(sets[0])
    p.sync()
    first = results(p)
    for k, got in ((0, first), (1, second)):
        dev = L.DeviceBuffer.from_array(bgr[k])
        for q in (p, plain):
            q.step_frames(dev.ptr, (720, 1280), 0.6)
            q.sync()
            same(q, got, k)
            assert q.graph_kernels() == n_kernels
        dev.free()
        raw = L.DeviceBuffer.from_array(sets[k])
        p.step_yuv(raw.ptr)
        p.sync()
        same(p, got, k)
        assert p.graph_kernels() == n_kernels
        raw.free()
    assert first[0][2] != second[0][2]
    with pytest.raises(ValueError, match="without yuv_input="):
        plain.step_yuv_host(sets[0])
    with pytest.raises(ValueError, match="without yuv_input="):
        plain.step_yuv(1)
    with pytest.raises(ValueError, match="unknown keys \\['pitch'\\]"):
        PL.AdasPipeline(None, lane_model, yuv_input=dict(format="nv12", pitch=1280), **kw)
    with pytest.raises(ValueError, match="yuv_input= and jpeg_input="):
        PL.AdasPipeline(None, lane_model, yuv_input=dict(format="nv12"), jpeg_input=True, **kw)
    with pytest.raises(ValueError, match="format 'p010' is none of"):
        PL.AdasPipeline(None, lane_model, yuv_input=dict(format="p010"), **kw)
    with pytest.raises(ValueError, match="at least %d bytes" % len(sets[0])):
        p.step_yuv_host(sets[0][:-1])
    for o in (p, plain):
        o.close()
