"""GPU: the baseline JPEG decoder (csrc/jpegdec_kernels.hip) through the C ABI, postproc.JpegDecoder and the fused step: every pixel and flag
equals the host build of the same rules (tests/emu_jpegdec_api.py, which tests/test_jpegdec_cpu.py pins to tests/jpegdec_ref.py and to
libjpeg), byte for byte, and no byte outside the batch's frames is written.  No decoder library is needed here.  The damaged streams are a
fixed subset of the CPU suite's, all of which the host build has decoded under a sanitizer."""
import importlib
import os

import numpy as np
import pytest

from conftest import load_pkg
import emu_jpeg_api as enc_emu
import emu_jpegdec_api as emu
import jpeg_ref as ref
import test_gpu_jpeg as TJ
import test_jpegdec_cpu as TC

pytestmark = pytest.mark.gpu
load_pkg()
L = importlib.import_module("adas_amd._lib")
PP = importlib.import_module("adas_amd.postproc")
PL = importlib.import_module("adas_amd.pipeline")
M = importlib.import_module("adas_amd.models")

INVALID = -1        # ADAS_ERR_INVALID
FILL = 0xA5


def fixture_by_size():
    z = np.load(TC.GOLDEN)
    out = {}
    for i, (name, (w, h)) in enumerate(zip(z["names"], z["sizes"])):
        out.setdefault((int(w), int(h)), []).append((str(name), z["stream_%d" % i].tobytes()))
    return out


def own_frames(dec):
    d, _ = dec.device_view()
    return d


def prefill_own(dec):
    n = dec.max_batch * dec.height * dec.width * 3
    L.check(L.lib().adas_memcpy_h2d(own_frames(dec), L.ptr(np.full(n, FILL, np.uint8)), n))


def download_own(dec):
    out = np.empty((dec.max_batch, dec.height, dec.width, 3), np.uint8)
    L.check(L.lib().adas_memcpy_d2h(L.ptr(out), own_frames(dec), out.nbytes))
    return out


def check_host_run(dec, streams, tag, lengths=None):
    """run_host into the handle's own frames: the batch's frames and flags equal the emulation's, image(f) too, the frames behind the batch
    keep their sentinel.  Then the same into a caller's buffer that starts on an odd byte: equal again, nothing behind the batch is
    written, and the handle's own frames are left alone."""
    n, w, h = len(streams), dec.width, dec.height
    want, want_flags = emu.decode_batch(streams, w, h, dec.capacity, lengths)
    prefill_own(dec)
    dec.run_host(streams)
    flags = dec.flags(n)
    got = download_own(dec)
    assert np.array_equal(flags, want_flags), (tag, flags, want_flags)
    for f in range(n):
        assert np.array_equal(got[f], want[f]), (tag, f, np.argwhere(got[f] != want[f])[:4])
        assert np.array_equal(dec.image(f), want[f]), (tag, f)
    assert (got[n:] == FILL).all(), tag
    fsz = w * h * 3
    buf = L.DeviceBuffer((n + 1) * fsz + 16)
    L.check(L.lib().adas_memcpy_h2d(buf.ptr, L.ptr(np.full((n + 1) * fsz + 16, FILL, np.uint8)), (n + 1) * fsz + 16))
    prefill_own(dec)
    dec.run_host(streams, d_dst=buf.ptr + 3)
    assert np.array_equal(dec.flags(n), want_flags), tag
    raw = buf.download(((n + 1) * fsz + 16,), np.uint8)
    assert np.array_equal(raw[3:3 + n * fsz].reshape(want.shape), want), tag
    assert (raw[:3] == FILL).all() and (raw[3 + n * fsz:] == FILL).all(), tag
    assert (download_own(dec) == FILL).all(), tag
    buf.free()
    return want, want_flags


@pytest.mark.parametrize("w,h", [(16, 16), (17, 9), (40, 24), (1, 1), (200, 120)])
def test_pixels_and_flags_equal_the_emulation(w, h):
    """Every fixture stream of the size (libjpeg's: grey, 4:4:4, 4:2:2, 4:2:0, with and without restart markers, optimised tables, 16-bit code
    words, and the rejects) and our own encoder's, alone and in batches of three."""
    streams = fixture_by_size()[(w, h)]
    for name in ("noise", "gradient", "flat128", "binary"):
        streams.append(("own_" + name, enc_emu.encode(ref.content(name, w, h, 1)[0], 90 if name != "binary" else 100)))
    dec = PP.JpegDecoder(w, h, max_batch=4, capacity=max(len(s) for _, s in streams) + 5)
    for name, s in streams:
        check_host_run(dec, [s], name)
    for i in range(0, len(streams), 2):
        group = [streams[(i + k) % len(streams)] for k in range(3)]
        check_host_run(dec, [s for _, s in group], [n for n, _ in group])
    dec.close()


@pytest.mark.parametrize("w,h", [(40, 24), (200, 120)])
def test_streams_on_any_byte_and_at_an_odd_stride(w, h):
    """run_device on streams that start 1 and 3 bytes behind an aligned allocation, at a stride that is no multiple of 4."""
    streams = [s for _, s in fixture_by_size()[(w, h)]][:3] + [enc_emu.encode(ref.content("noise", w, h, 1)[0], 75)]
    n = len(streams)
    stride = max(len(s) for s in streams) + (1 if max(len(s) for s in streams) % 4 != 3 else 2)
    assert stride % 4 != 0
    dec = PP.JpegDecoder(w, h, max_batch=n, capacity=stride)
    want, want_flags = emu.decode_batch(streams, w, h, stride)
    lens = L.DeviceBuffer.from_array(np.array([len(s) for s in streams], np.int64))
    buf = L.DeviceBuffer(n * stride + 16)
    for off in (1, 3):
        raw = np.full(n * stride + 16, FILL, np.uint8)
        for f, s in enumerate(streams):
            raw[off + f * stride:off + f * stride + len(s)] = np.frombuffer(s, np.uint8)
        L.check(L.lib().adas_memcpy_h2d(buf.ptr, L.ptr(raw), raw.nbytes))
        prefill_own(dec)
        dec.run_device(buf.ptr + off, lens.ptr, stride, n)
        assert np.array_equal(dec.flags(n), want_flags) and not want_flags.any()
        assert np.array_equal(download_own(dec), want), off
    buf.free()
    lens.free()
    dec.close()


@pytest.mark.parametrize("w,h", [(40, 24), (200, 120)])
def test_device_round_trip_without_a_host_copy(w, h):
    """JpegEncoder.run, then JpegDecoder.run_device on encoder.device_view(): the emulation's decoding of the emulation's encoding."""
    frames = np.concatenate([ref.content("gradient", w, h, 2), ref.content("noise", w, h, 1)])
    encoder = PP.JpegEncoder(w, h, quality=85, max_batch=3, capacity=enc_emu.bound(w, h))
    dec = PP.JpegDecoder(w, h, max_batch=3, capacity=enc_emu.bound(w, h))
    src = L.DeviceBuffer.from_array(frames)
    encoder.run(src.ptr, 3)
    d, dl, stride = encoder.device_view()
    dec.run_device(d, dl, stride, 3)
    assert not dec.flags(3).any()
    for f in range(3):
        want = emu.decode(enc_emu.encode(frames[f], 85), w, h, stages=False)
        assert want.flags == 0 and np.array_equal(dec.image(f), want.bgr), f
    for o in (encoder, dec, src):
        (o.close if hasattr(o, "close") else o.free)()


def test_rejects_and_damage_between_good_frames():
    """The fixed subset of tests/test_jpegdec_cpu.py's cases: progressive, wrong size, length 0, truncated in mid-scan, wrong RST index, one
    flipped scan byte, each between good frames of one batch."""
    w, h = 40, 24
    _, cases = TC.damage_cases(w, h)
    by_name = {c[0]: c[1] for c in cases}
    good = by_name["good"]
    bad = [by_name["sof2"], by_name["wrong width"], b"", by_name["truncated in mid-scan"], by_name["wrong RST index"], by_name["a flipped scan byte"]]
    streams = [good]
    for s in bad:
        streams += [s, good]
    dec = PP.JpegDecoder(w, h, max_batch=len(streams) + 1, capacity=len(good) + 8)
    want, flags = check_host_run(dec, streams, "damage")
    assert list(flags[1:9:2]) == [dec.UNSUPPORTED, dec.SIZE, dec.FORMAT, dec.CORRUPT] and flags[9] == dec.CORRUPT
    assert not flags[0::2].any() and all(np.array_equal(want[i], want[0]) for i in range(0, len(streams), 2))
    assert not want[1].any() and not want[3].any() and not want[5].any() and want[7].any()
    dec.close()


def test_a_second_scan_behind_the_first_is_unsupported():
    """What the segment search decides behind the scan's end (jd_second_scan), from the CPU suite's cases: an SOS there, alone or behind a
    table segment, makes the frame UNSUPPORTED and black; other or damaged segments there are ignored."""
    w, h = 40, 24
    _, cases = TC.damage_cases(w, h)
    by_name = {c[0]: c[1] for c in cases}
    names = ["good", "a second SOS behind a full scan", "segments behind the scan without an SOS are ignored", "a second SOS behind a full scan and a DHT",
             "a damaged segment behind the scan is ignored"]
    streams = [by_name[n] for n in names]
    dec = PP.JpegDecoder(w, h, max_batch=len(streams), capacity=max(len(s) for s in streams))
    want, flags = check_host_run(dec, streams, "second scan")
    assert list(flags) == [0, dec.UNSUPPORTED, 0, dec.UNSUPPORTED, 0]
    assert not want[1].any() and not want[3].any() and all(np.array_equal(want[i], want[0]) for i in (2, 4))
    dec.close()


def test_run_host_equals_run_device_and_a_length_over_the_capacity():
    w, h = 40, 24
    streams = [s for _, s in fixture_by_size()[(w, h)]][:4]
    cap = sorted(len(s) for s in streams)[-2]                 # the longest stream does not fit
    long = max(range(4), key=lambda i: len(streams[i]))
    dec = PP.JpegDecoder(w, h, max_batch=4, capacity=cap)
    dec.run_host(streams)
    host, host_flags = download_own(dec), dec.flags(4)
    stride = max(len(s) for s in streams)
    raw = np.zeros((4, stride), np.uint8)
    for f, s in enumerate(streams):
        raw[f, :len(s)] = np.frombuffer(s, np.uint8)
    buf, lens = L.DeviceBuffer.from_array(raw), L.DeviceBuffer.from_array(np.array([len(s) for s in streams], np.int64))
    prefill_own(dec)
    dec.run_device(buf.ptr, lens.ptr, stride, 4)
    assert np.array_equal(dec.flags(4), host_flags) and np.array_equal(download_own(dec), host)
    want, want_flags = emu.decode_batch(streams, w, h, cap)
    assert np.array_equal(host, want) and np.array_equal(host_flags, want_flags)
    assert host_flags[long] == dec.FORMAT and not host[long].any() and sum(host_flags != 0) == 1
    for o in (buf, lens):
        o.free()
    dec.close()


def test_refusals_by_name():
    def refused(match, fn, *a, **kw):
        with pytest.raises(RuntimeError, match=match) as ei:
            fn(*a, **kw)
        assert ei.value.code == INVALID
    refused("adas_jpegdec_create: a 0x16 frame", PP.JpegDecoder, 0, 16)
    refused("adas_jpegdec_create: a 16x65536 frame", PP.JpegDecoder, 16, 65536)
    refused("adas_jpegdec_create: max_batch 0", PP.JpegDecoder, 16, 16, max_batch=0)
    refused("a capacity of -1 bytes per stream is outside", PP.JpegDecoder, 16, 16, capacity=-1)
    dec = PP.JpegDecoder(16, 16, max_batch=2)
    assert dec.capacity == enc_emu.bound(16, 16)
    s = enc_emu.encode(ref.content("noise", 16, 16, 1)[0], 90)
    refused("adas_jpegdec_fetch: frame 0 was not written", dec.image, 0)
    refused("adas_jpegdec_run_host: batch 3, the handle holds 2 frames", dec.run_host, [s, s, s])
    dec.run_host([s])
    refused("adas_jpegdec_fetch: frame 1 was not written", dec.image, 1)
    refused("adas_jpegdec_fetch_flags: 2 frames, the last run decoded 1", dec.flags, 2)
    assert np.array_equal(dec.image(0), emu.decode(s, 16, 16, stages=False).bgr)
    dst = L.DeviceBuffer(16 * 16 * 3)
    dec.run_host([s], d_dst=dst.ptr)
    refused("adas_jpegdec_fetch: frame 0 was not written into the handle's buffer", dec.image, 0)
    dst.free()
    dec.close()


# ------------------------------------------------------------------------------------------------ the fused step
@pytest.fixture(scope="module")
def lane_model(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("jpgdec") / "lanes.hipm")
    M.build("ufldv2_res18", wsrc=TJ.PrescribedLanes(), **TJ.LANE_KW).save(path)
    return path


def test_fused_step_from_compressed_frames(lane_model):
    """The lane branch in graph mode with the encoding stage on the step's frames, so that what the step consumed is visible: step_jpeg_host
    on compressed frames, then step_frames on an upload of the emulation's decoding of them, on the same pipeline.  Lanes, geometry and the
    encoded frames are equal bit for bit, and so is the captured step's kernel count.  Two consecutive step_jpeg_host calls with different
    streams use both staging buffers.  This is the lane-only pipeline of test_gpu_jpeg.py's fused-step test (no detector, track=False), so
    there are no survivors and tracks to compare: the step's own JPEG of the frames it consumed stands in for them -- every later stage
    reads those same frames."""
    import bench
    kw = TJ.pipeline_kw()
    p = PL.AdasPipeline(None, lane_model, jpeg_input=dict(capacity=1500000), jpeg=dict(quality=60, source="frames", capacity=400000), **kw)
    plain = PL.AdasPipeline(None, lane_model, jpeg=dict(quality=60, source="frames", capacity=400000), **kw)
    assert plain.jpeg_decoder is None
    cam = [bench.cam_frames(2, 500 + i) for i in range(2)]
    sets = [[enc_emu.encode(c[s], 85) for s in range(2)] for c in cam]
    decoded = [np.stack([emu.decode(s, 1280, 720, stages=False).bgr for s in st]) for st in sets]
    p.step_jpeg_host(sets[0])
    p.step_jpeg_host(sets[1])           # queued behind the first: the other staging buffer
    p.sync()
    assert not p.input_flags().any()
    second = [(p.decode.fetch(s), p.geometry.fetch(s), p.jpeg(s)) for s in range(2)]
    n_jpeg = p.graph_kernels()
    assert np.array_equal(p.jpeg_decoder.image(1), decoded[1][1])
    p.step_jpeg_host(sets[0])
    p.sync()
    first = [(p.decode.fetch(s), p.geometry.fetch(s), p.jpeg(s)) for s in range(2)]
    for k, got in ((0, first), (1, second)):
        dev = L.DeviceBuffer.from_array(decoded[k])
        for q in (p, plain):
            q.step_frames(dev.ptr, (720, 1280), 0.6)
            q.sync()
            for s in range(2):
                lanes, geo, stream = got[s]
                assert q.decode.fetch(s) == lanes, (k, s)
                g = q.geometry.fetch(s)
                assert g["area_status"] == geo["area_status"] and g["direction"] == geo["direction"] and g["curvature"] == geo["curvature"] and \
                    g["offset"] == geo["offset"] and np.array_equal(g["area_points"], geo["area_points"]), (k, s)
                assert all(np.array_equal(g["bird_points"][li], geo["bird_points"][li]) for li in range(4)), (k, s)
                assert q.jpeg(s) == stream == enc_emu.encode(decoded[k][s], 60), (k, s)
            assert q.graph_kernels() == n_jpeg
        dev.free()
    assert first[0][2] != second[0][2]
    with pytest.raises(ValueError, match="without jpeg_input="):
        plain.step_jpeg_host(sets[0])
    with pytest.raises(ValueError, match="unknown keys"):
        PL.AdasPipeline(None, lane_model, jpeg_input=dict(quality=3), **kw)
    with pytest.raises(ValueError, match="got 1 streams, a step has 2"):
        p.step_jpeg_host(sets[0][:1])
    for o in (p, plain):
        o.close()
