"""CPU: postproc.split_mjpeg, what tools/demo_headless.py --from-mjpeg cuts a raw MJPEG file with -- the inverse of appending JpegEncoder's
streams to a file (--mjpeg).  Pure Python; no device is touched."""
import importlib

import numpy as np

from conftest import load_pkg
import jpeg_ref as ref
import test_jpegdec_cpu as TC

load_pkg()
PP = importlib.import_module("adas_amd.postproc")


def test_split_mjpeg_is_the_inverse_of_concatenation():
    """libjpeg's streams of every sampling (APP0 segments, optimised tables, restart markers, a progressive one) and our own, back to back, with
    junk between two of them: the streams and their SOFn sizes come back in order.  A stream without EOI ends at the next SOI or at the
    file's end; an EOI in the file's last two bytes is found; fill bytes in front of a marker and stuffed 0xFF in the scan are stepped over."""
    z = np.load(TC.GOLDEN)
    streams = [(z["stream_%d" % i].tobytes(), (int(w), int(h))) for i, (w, h) in enumerate(z["sizes"])]
    own = ref.encode(ref.content("binary", 40, 24, 1)[0], 100)          # many stuffed bytes
    assert own.count(b"\xff\x00") > 10
    streams.append((own, (40, 24)))
    sof = own.index(b"\xff\xc0")
    streams.append((own[:sof] + b"\xff\xff" + own[sof:], (40, 24)))      # fill bytes
    data = b"".join(s for s, _ in streams)
    got = PP.split_mjpeg(data)
    assert [g[0] for g in got] == [s for s, _ in streams] and [g[1] for g in got] == [wh for _, wh in streams]
    assert PP.split_mjpeg(b"junk" + own + b"\x00\x01junk" + own) == [(own, (40, 24))] * 2
    # no EOI: up to the next SOI, and up to the file's end
    cut = own[:-2]
    got = PP.split_mjpeg(cut + own + cut)
    assert [g[0] for g in got] == [cut, own, cut] and all(g[1] == (40, 24) for g in got)
    # a stream that ends between two header segments, in front of its SOF0, has no size; nothing at all gives nothing
    got = PP.split_mjpeg(own[:sof] + own)
    assert got == [(own[:sof], None), (own, (40, 24))]
    assert PP.split_mjpeg(b"") == [] and PP.split_mjpeg(b"no jpeg here") == []
