"""GPU: the baseline JPEG encoder (csrc/jpeg_kernels.hip) through the C ABI, postproc.JpegEncoder and the fused step: every stream, length
and flag equals the host build of the same rules (tests/emu_jpeg_api.py, which tests/test_jpeg_cpu.py pins to tests/jpeg_ref.py and to
libjpeg), byte for byte, and no byte outside a stream is written.  No decoder is needed here."""
import ctypes as C
import importlib

import numpy as np
import pytest

from conftest import load_pkg
import emu_jpeg_api as emu
import jpeg_ref as ref
import overlay_scene as OS

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
CE = importlib.import_module("adas_amd.coreEngine")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")
A = importlib.import_module("adas_amd.analysis")

INVALID = -1        # ADAS_ERR_INVALID
FILL = 0xA5


def prefill(enc, n):
    """The handle's stream buffer, all FILL: what a run does not write stays that."""
    d, _, stride = enc.device_view()
    assert stride == enc.capacity
    L.check(L.lib().adas_memcpy_h2d(d, L.ptr(np.full(n * stride, FILL, np.uint8)), n * stride))


def streams(enc, n):
    d, dl, stride = enc.device_view()
    raw = np.empty((n, stride), np.uint8)
    L.check(L.lib().adas_memcpy_d2h(L.ptr(raw), d, raw.nbytes))
    lens = np.empty(n, np.int64)
    L.check(L.lib().adas_memcpy_d2h(L.ptr(lens), dl, lens.nbytes))
    return raw, lens


def check_run(enc, frames, quality, d_ptr=None, tag=()):
    """One run over `frames` -> the device's whole stream buffer, lengths and flags equal the emulation's on a buffer pre-filled alike."""
    n = len(frames)
    buf = None
    if d_ptr is None:
        buf = L.DeviceBuffer.from_array(frames)
        d_ptr = buf.ptr
    prefill(enc, n)
    enc.run(d_ptr, n)
    lens, flags = enc.lengths(n)
    want, want_len, want_flags = emu.encode_raw(frames, quality, enc.capacity, fill=FILL)
    raw, dev_len = streams(enc, n)
    assert np.array_equal(lens, want_len) and np.array_equal(dev_len, want_len) and np.array_equal(flags, want_flags), (tag, lens, want_len, flags)
    for f in range(n):
        assert np.array_equal(raw[f], want[f]), (tag, f, int(lens[f]), np.flatnonzero(raw[f] != want[f])[:8])
        assert enc.fetch(f) == want[f, :want_len[f]].tobytes(), (tag, f)
    if buf is not None:
        buf.free()
    return raw, lens


@pytest.mark.parametrize("w,h,n", ref.SHAPES)
def test_streams_lengths_and_flags_equal_the_emulation(w, h, n):
    """Every shape x content x quality; the bytes from a stream's end to the capacity keep their sentinel.  In the three-frame shape frame 2
    repeats frame 0 and must give its bytes (J9)."""
    enc = PP.JpegEncoder(w, h, quality=90, max_batch=n, capacity=emu.bound(w, h))
    for name in ref.CONTENTS:
        frames = ref.content(name, w, h, n)
        if n > 2:
            frames[2] = frames[0]
        buf = L.DeviceBuffer.from_array(frames)
        for q in ref.QUALITIES:
            enc.set_quality(q)
            raw, lens = check_run(enc, frames, q, buf.ptr, (w, h, name, q))
            assert (lens > emu.header_bytes()).all()
            if n > 2:
                assert lens[0] == lens[2] and np.array_equal(raw[0], raw[2])
                assert name.startswith("flat") or not np.array_equal(raw[0], raw[1])
        buf.free()
    enc.close()


@pytest.mark.parametrize("w,h", [(40, 24), (1280, 16)])
def test_a_source_on_any_byte(w, h):
    """The frames start 1 and 3 bytes behind an aligned allocation."""
    frames = ref.content("noise", w, h, 2, seed=4)
    enc = PP.JpegEncoder(w, h, quality=75, max_batch=2, capacity=emu.bound(w, h))
    buf = L.DeviceBuffer(frames.nbytes + 16)
    for off in (1, 3):
        L.check(L.lib().adas_memcpy_h2d(buf.ptr + off, L.ptr(frames), frames.nbytes))
        check_run(enc, frames, 75, buf.ptr + off, (w, h, off))
    buf.free()
    enc.close()


def test_overflow_writes_nothing_and_spares_the_other_frames():
    """Capacity = header + 32: the noise frames get length 0 and the flag and not one byte of their slots is written; flat grey between them
    still encodes (J8)."""
    w, h = 48, 32
    frames = np.concatenate([ref.content("noise", w, h), ref.content("flat128", w, h), ref.content("noise", w, h, seed=1)])
    enc = PP.JpegEncoder(w, h, quality=90, max_batch=3, capacity=emu.header_bytes() + 32)
    raw, lens = check_run(enc, frames, 90)
    _, flags = enc.lengths(3)
    assert list(flags) == [enc.OVERFLOW, 0, enc.OVERFLOW] and lens[0] == lens[2] == 0 and 0 < lens[1] <= enc.capacity
    assert (raw[0] == FILL).all() and (raw[2] == FILL).all() and enc.fetch(0) == b""
    enc.close()


def test_set_quality_between_two_runs():
    w, h = 40, 24
    frames = ref.content("gradient", w, h, 1)
    enc = PP.JpegEncoder(w, h, quality=50, max_batch=1, capacity=emu.bound(w, h))
    a, _ = check_run(enc, frames, 50)
    enc.set_quality(95)
    b, _ = check_run(enc, frames, 95)
    assert not np.array_equal(a, b)
    enc.close()


def test_refusals_by_name():
    def refused(match, fn, *a, **kw):
        with pytest.raises(RuntimeError, match=match) as ei:
            fn(*a, **kw)
        assert ei.value.code == INVALID
    refused("adas_jpeg_create: quality 0 is outside 1..100", PP.JpegEncoder, 16, 16, quality=0)
    refused("adas_jpeg_create: quality 101 is outside 1..100", PP.JpegEncoder, 16, 16, quality=101)
    refused("adas_jpeg_create: a 0x16 frame", PP.JpegEncoder, 0, 16)
    refused("adas_jpeg_create: a 16x65536 frame", PP.JpegEncoder, 16, 65536)
    refused("adas_jpeg_create: max_batch 0", PP.JpegEncoder, 16, 16, max_batch=0)
    refused("a capacity of 610 bytes per frame is below the 611 header bytes", PP.JpegEncoder, 16, 16, capacity=610)
    refused("a capacity of 459 bytes per frame is below the 611 header bytes", PP.JpegEncoder, 17, 9)      # the default, width x height x 3
    assert PP.JpegEncoder.bound(1280, 720) == emu.bound(1280, 720) == 611 + 21600 * 416 + 2 * 44 + 2 and PP.JpegEncoder.bound(0, 5) == 0
    enc = PP.JpegEncoder(16, 16, max_batch=2, capacity=emu.bound(16, 16))
    frames = ref.content("noise", 16, 16, 2)
    assert len(emu.encode(frames[0], 90)) > 700
    buf = L.DeviceBuffer.from_array(frames)
    refused("adas_jpeg_fetch: frame 0 was not part of the last run", enc.fetch, 0)
    refused("adas_jpeg_run: batch 3, the handle holds 2 frames", enc.run, buf.ptr, 3)
    refused("adas_jpeg_set_quality: quality 0 is outside 1..100", enc.set_quality, 0)
    enc.run(buf.ptr, 1)
    refused("adas_jpeg_fetch: frame 1 was not part of the last run", enc.fetch, 1)
    refused("adas_jpeg_fetch_lengths: 2 frames, the last run encoded 1", enc.lengths, 2)
    n = C.c_int64()
    small = np.zeros(700, np.uint8)
    with pytest.raises(RuntimeError, match="adas_jpeg_fetch: frame 0 holds %d bytes, the buffer 700" % len(emu.encode(frames[0], 90))) as ei:
        L.check(L.lib().adas_jpeg_fetch(enc.h, 0, L.ptr(small), 700, C.byref(n), None))
    assert ei.value.code == INVALID and n.value == len(emu.encode(frames[0], 90))
    assert enc.fetch(0) == emu.encode(frames[0], 90)        # and the handle still works
    buf.free()
    enc.close()


# ------------------------------------------------------------------------------------------------ the fused step
IMG = (1280, 720)
LANE_KW = dict(in_h=160, in_w=800, num_grid_row=100, num_cls_row=36, num_grid_col=50, num_cls_col=41)      # the reduced lane net of
LANE_CFG = dict(grid_row=100, cls_row=36, grid_col=50, cls_col=41, row_anchor=np.linspace(0.42, 1, 36),     # test_gpu_overlay.py
                col_anchor=np.linspace(0, 1, 41))


class PrescribedLanes:
    """The weight source of test_gpu_overlay.py: every weight zero, the last layer's bias puts both ego lanes on every row anchor."""

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
        return self.bias if name == "cls.3.bias" else np.zeros(shape, np.float32)


@pytest.fixture(scope="module")
def lane_model(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("jpg") / "lanes.hipm")
    M.build("ufldv2_res18", wsrc=PrescribedLanes(), **LANE_KW).save(path)
    return path


def pipeline_kw():
    return dict(n_streams=2, precision="bf16", src_hw=(720, 1280), lane_cfg=LANE_CFG, track=False, use_graph=True,
                geometry=dict(bird_wh=IMG, M=A.PerspectiveTransformation(IMG).M))


def test_fused_step_overlay_and_frames_sources_replay_and_launch_count(lane_model):
    """The lane branch with its overlay, in graph mode.  source="overlay": jpeg(f) is the emulation's encoding of overlay_image(f), on the
    step that captures and on the one that replays.  source="frames": the encoding of the frames the step was given, and a replayed step's
    bytes are those of an eager JpegEncoder.run on the same frames.  Three more kernels with the stage; with jpeg=None exactly those of a
    pipeline built without the key."""
    import bench
    kw = pipeline_kw()
    cam = [bench.cam_frames(2, 300 + i) for i in range(2)]
    cam[1][0, :64, :64] = OS.noise(1, 64, 64, 9)[0]          # a patch of noise: stuffed bytes in a real frame
    dev = [L.DeviceBuffer.from_array(c) for c in cam]
    po = PL.AdasPipeline(None, lane_model, overlay=dict(), jpeg=dict(quality=80), **kw)
    pf = PL.AdasPipeline(None, lane_model, overlay=dict(), jpeg=dict(quality=60, source="frames", capacity=400000), **kw)
    none = PL.AdasPipeline(None, lane_model, overlay=dict(), jpeg=None, **kw)
    plain = PL.AdasPipeline(None, lane_model, overlay=dict(), **kw)
    eager = PP.JpegEncoder(1280, 720, quality=60, max_batch=2, capacity=400000)
    for k in range(3):      # step 0 and 1 capture (two input buffers), step 2 replays the first capture
        for p in (po, pf, none, plain):
            p.step_frames(dev[k % 2].ptr, (720, 1280), 0.6)
            p.sync()
        eager.run(dev[k % 2].ptr, 2)
        lens, flags = po.jpeg_lengths()
        assert not flags.any() and not pf.jpeg_lengths()[1].any()
        for s in range(2):
            drawn = po.overlay_image(s)
            assert np.array_equal(drawn, none.overlay_image(s)) and (drawn != cam[k % 2][s]).any()
            got = po.jpeg(s)
            assert got == emu.encode(drawn, 80) and len(got) == lens[s], (k, s, len(got))
            assert pf.jpeg(s) == emu.encode(cam[k % 2][s], 60) == eager.fetch(s), (k, s)
        assert np.array_equal(dev[k % 2].download(cam[k % 2].shape, np.uint8), cam[k % 2])      # the step's frames are not written
    n_plain = plain.graph_kernels()
    assert none.graph_kernels() == n_plain and none.jpeg_encoder is None
    assert po.graph_kernels() == n_plain + 3 and pf.graph_kernels() == n_plain + 3
    with pytest.raises(ValueError, match="without jpeg="):
        none.jpeg(0)
    for o in (po, pf, none, plain, eager):
        o.close()
    for b in dev:
        b.free()


def test_pipeline_prerequisites(lane_model):
    kw = pipeline_kw()
    with pytest.raises(ValueError, match='source="overlay" needs overlay='):
        PL.AdasPipeline(None, lane_model, jpeg=dict(), **kw)
    with pytest.raises(ValueError, match="quality 0 is outside 1..100"):
        PL.AdasPipeline(None, lane_model, overlay=dict(), jpeg=dict(quality=0), **kw)
    with pytest.raises(ValueError, match="quality 101 is outside 1..100"):
        PL.AdasPipeline(None, lane_model, jpeg=dict(quality=101, source="frames"), **kw)
    with pytest.raises(ValueError, match="neither"):
        PL.AdasPipeline(None, lane_model, jpeg=dict(source="bird"), **kw)
    with pytest.raises(ValueError, match="unknown keys"):
        PL.AdasPipeline(None, lane_model, jpeg=dict(source="frames", subsampling=0), **kw)
    p = PL.AdasPipeline(None, lane_model, overlay=dict(), **kw)
    q = PL.AdasPipeline(None, lane_model, **kw)
    small, one, good = PP.JpegEncoder(640, 360, max_batch=2), PP.JpegEncoder(1280, 720, max_batch=1), PP.JpegEncoder(1280, 720, max_batch=2)
    attach = L.lib().adas_pipeline_attach_jpeg
    for fn, match in ((lambda: L.check(attach(p.h, small.h, 0)), "created for 640x360 frames, the attached overlay draws 1280x720"),
                      (lambda: L.check(attach(p.h, one.h, 0)), "the JPEG handle holds 1 frames, a step has 2"),
                      (lambda: L.check(attach(q.h, good.h, 0)), "the overlay source needs an attached overlay handle"),
                      (lambda: L.check(attach(p.h, good.h, 2)), "unknown source 2")):
        with pytest.raises(RuntimeError, match=match) as ei:
            fn()
        assert ei.value.code == INVALID
    L.check(attach(q.h, small.h, 1))                 # the frames' size is known at the step: refused there, by name
    d = L.DeviceBuffer.from_array(np.zeros((2, 720, 1280, 3), np.uint8))
    with pytest.raises(RuntimeError, match="the attached JPEG handle was created for 640x360 frames, the step has 1280x720") as ei:
        q.step_frames(d.ptr, (720, 1280), 0.6)
    assert ei.value.code == INVALID
    L.check(attach(q.h, good.h, 1))
    with pytest.raises(RuntimeError, match="no frame to encode") as ei:      # seam tensors with the stage attached
        q.step(None, d.ptr)
    assert ei.value.code == INVALID
    L.check(attach(q.h, None, 0))                    # detached: the step is the plain one again
    q.step_frames(d.ptr, (720, 1280), 0.6)
    q.sync()
    for o in (p, q, small, one, good):
        o.close()
    d.free()
