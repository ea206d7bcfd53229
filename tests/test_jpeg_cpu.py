"""CPU: the JPEG encoder's rules J1-J9 (csrc/jpeg_core.h through its host build, tests/emu_jpeg_api.py) against the NumPy restatement
tests/jpeg_ref.py byte for byte, against float64 for the transform's stated bound, and -- where Pillow with JPEG support is installed --
against libjpeg's decoder and encoder."""
import io
import warnings

import numpy as np
import pytest

import emu_jpeg_api as emu
import jpeg_ref as ref

# test_pillow_decodes_and_psnr_margin: ours minus Pillow's PSNR (dB) on jpeg_ref.smooth at the same tables, 4:2:0, as measured with this file:
#              q50      q75      q90      q95
#   64 x 48   -0.003   +0.003   -0.010   +0.033
#   40 x 168  +0.014   -0.046   -0.012   +0.018
# worst shortfall 0.046 dB (libjpeg's chroma filter and DCT rounding differ slightly from J3 / J4); the margin is that plus 0.1 dB
PSNR_MARGIN = 0.146


def cases(w, h, n):
    for name in ref.CONTENTS:
        frames = ref.content(name, w, h, n)
        for q in ref.QUALITIES:
            yield name, q, frames


@pytest.mark.parametrize("w,h,n", ref.SHAPES)
def test_stream_equals_the_restatement_and_decodes_to_its_levels(w, h, n):
    """Streams and lengths equal jpeg_ref's byte for byte; decoding the entropy layer of the emulation's stream gives exactly the levels the
    emulation quantised, which are the restatement's."""
    cap = emu.bound(w, h)
    for name, q, frames in cases(w, h, n):
        out, lengths, flags = emu.encode_raw(frames, q, cap, fill=0x5A)
        assert not flags.any()
        for f in range(n):
            lev = ref.levels(frames[f], q)
            want = ref.encode(frames[f], q, lev)
            got = out[f, :lengths[f]].tobytes()
            assert lengths[f] == len(want) and got == want, (name, q, f, lengths[f], len(want))
            assert (out[f, lengths[f]:] == 0x5A).all()
            assert np.array_equal(emu.levels(frames[f], q), lev), (name, q, f)
            if w <= 48 or q in (50, 100):       # the wide shapes: two qualities keep the pure-Python decoder quick
                info, back = ref.decode(got)
                assert (info["w"], info["h"]) == (w, h) and np.array_equal(back, lev), (name, q, f)
    if n > 1:       # J9: a frame's bytes do not depend on its place in the batch
        frames = ref.content("noise", w, h, n)
        frames[2] = frames[0]
        out, lengths, _ = emu.encode_raw(frames, 90, cap)
        assert lengths[0] == lengths[2] and np.array_equal(out[0], out[2]) and not np.array_equal(out[0], out[1])


@pytest.mark.parametrize("w,h,n", ref.SHAPES)
def test_the_kernels_composition_in_rounds_gives_the_same_stream(w, h, n):
    """The entropy kernel places the blocks of a segment a round at a time (prefix sums of bit counts, bits ORed into words, the last partial
    byte carried over): composed that way with rounds of 256 (the device's), 1, 5 and 6 blocks the stream is the bit writer's."""
    cap = emu.bound(w, h)
    for name, q, frames in cases(w, h, n):
        want = emu.encode_raw(frames, q, cap, fill=0x5A)
        for rounds in (256, 1, 5, 6):
            got = emu.encode_raw(frames, q, cap, fill=0x5A, rounds=rounds)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), (name, q, rounds)


def test_ctypes_mirror_of_the_parameter_struct():
    """adas_jpeg_params (include/adas_hip.h; csrc/jpeg_kernels.hip asserts the same numbers at compile time) and _lib.JpegParams."""
    import ctypes as C
    import importlib
    from conftest import load_pkg
    load_pkg()
    L = importlib.import_module("adas_amd._lib")
    P = L.JpegParams
    assert C.sizeof(P) == 24 and (P.width.offset, P.height.offset, P.quality.offset, P.capacity.offset) == (0, 4, 8, 16)
    assert L.JPEG_OVERFLOW == ref.OVERFLOW == emu.OVERFLOW and L.JPEG_SOURCES == {"overlay": 0, "frames": 1}


def test_header_tables_and_sampling():
    """J7 / J5 / J1-J3 piece by piece: header bytes, divisors, and the samples of blocks on and beyond the edge."""
    for (w, h), q in (((17, 9), 1), ((1280, 720), 50), ((40, 168), 75), ((65535, 1), 100)):
        assert emu.header(w, h, q) == ref.header(w, h, q) and len(ref.header(w, h, q)) == emu.header_bytes() == ref.HEADER_BYTES
        assert np.array_equal(emu.tables(q), ref.qtables(q)[:, ref.ZIGZAG])
        assert emu.bound(w, h) == ref.bound(w, h)
    zz, inv = emu.zigzag()
    assert zz == ref.ZIGZAG and [inv[n] for n in zz] == list(range(64))
    assert (ref.qtables(100) == 1).all() and ref.qtables(1).max() == 255 and np.array_equal(ref.qtables(50), ref.BASE)
    img = ref.content("noise", 21, 19, 1)[0]
    y, cb, cr = ref.components(img)
    for my in range(2):
        for mx in range(2):
            for k6 in range(6):
                if k6 < 4:
                    want = y[my * 16 + (k6 >> 1) * 8:, mx * 16 + (k6 & 1) * 8:][:8, :8]
                else:
                    want = (cb, cr)[k6 - 4][my * 8:my * 8 + 8, mx * 8:mx * 8 + 8]
                assert np.array_equal(emu.load_block(img, my, mx, k6).reshape(8, 8), want - 128), (my, mx, k6)


def test_transform_bound_and_quantiser():
    """J4: |F' - 8 F_float64| <= JPEG_FDCT_ERR over random and extreme blocks; J5: a level that differs from round_half_away(F / d) differs by
    exactly 1 and sits within JPEG_FDCT_ERR / (8 d) of a rounding boundary.  Largest |F' - 8 F| seen over these 6270 blocks: 0.8774 of the
    1.75 the header derives."""
    rng = np.random.default_rng(5)
    blocks = [rng.integers(-128, 128, (4000, 64)), rng.integers(0, 2, (2000, 64)) * 255 - 128, np.full((1, 64), -128), np.full((1, 64), 127)]
    yy, xx = np.mgrid[0:8, 0:8]
    for mask in ((yy + xx) % 2 == 0, xx % 2 == 0, yy % 2 == 0, (yy // 2 + xx // 2) % 2 == 0, xx < 4, yy < 4):     # +- checkerboards, stripes, steps
        blocks += [np.where(mask, 127, -128).reshape(1, 64), np.where(mask, -128, 127).reshape(1, 64)]
    imp = np.zeros((256, 64), np.int64)
    for i in range(64):      # single impulses of either sign on zero, and on the two rails
        imp[i, i], imp[64 + i, i] = 127, -128
        imp[128 + i], imp[192 + i] = -128, 127
        imp[128 + i, i], imp[192 + i, i] = 127, -128
    blocks.append(imp)
    f = np.concatenate(blocks).astype(np.int64)
    F = emu.fdct(f).reshape(-1, 8, 8)
    assert np.array_equal(F, ref.fdct(f))
    exact = ref.fdct_exact(f)
    err = np.abs(F - exact).max()
    assert emu.fdct_err() == ref.FDCT_ERR
    assert err <= ref.FDCT_ERR, err
    assert np.array_equal(F[:, 0, 0], f.sum(axis=1))          # the DC term is exact
    print("largest |F' - 8 F| over %d blocks: %.4f (bound %.2f)" % (len(f), err, ref.FDCT_ERR))
    for q in ref.QUALITIES + (75,):
        for cls in range(2):
            d = ref.qtables(q)[cls].reshape(8, 8)
            ac = np.ones((8, 8), np.int32)
            ac[0, 0] = 0
            lev = emu.quantise(F, np.broadcast_to(d, F.shape), np.broadcast_to(ac, F.shape)).reshape(F.shape)
            assert np.array_equal(lev, ref.quantise(F, d))
            x = np.abs(exact / 8.0) / d
            ideal = np.sign(exact) * np.floor(x + 0.5)
            ideal = np.where((ac > 0) & (np.abs(ideal) > 1023), np.sign(exact) * 1023, ideal)
            off = lev != ideal
            assert (np.abs(lev - ideal)[off] == 1).all(), (q, cls)
            near = np.abs(x - np.floor(x) - 0.5) <= ref.FDCT_ERR / (8.0 * d)
            assert near[off].all(), (q, cls, int(off.sum()))
    # J5 on the rails of its range: the integer division as written, against Python's
    Fs = np.arange(-8200, 8201, dtype=np.int64)
    for d in (1, 2, 3, 17, 99, 254, 255):
        want = np.sign(Fs) * ((np.abs(Fs) + 4 * d) // (8 * d))
        assert np.array_equal(emu.quantise(Fs, d, 0), want)
        assert np.array_equal(emu.quantise(Fs, d, 1), np.clip(want, -1023, 1023))


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / mse)


def pillow_encode(Image, img_bgr, quality):
    """Pillow's own encoding at the J5 tables, 4:2:0; checked to carry exactly those tables."""
    q = ref.qtables(quality)
    want = [bytes(int(v) for v in q[c][ref.ZIGZAG]) for c in range(2)]
    for order in (None, ref.ZIGZAG):      # Pillow versions differ in the order qtables= takes
        tabs = [[int(v) for v in (t if order is None else t[order])] for t in q]
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(img_bgr[..., ::-1])).save(b, "JPEG", qtables=tabs, subsampling=2)
        data = b.getvalue()
        found, i = {}, 2
        while data[i + 1] != 0xDA:
            n = int.from_bytes(data[i + 2:i + 4], "big")
            if data[i + 1] == 0xDB:
                body = data[i + 4:i + 2 + n]
                while body:
                    found[body[0] & 15], body = bytes(body[1:65]), body[65:]
            i += 2 + n
        if [found.get(0), found.get(1)] == want:
            return data
    raise AssertionError("Pillow did not take the J5 tables")


def test_pillow_decodes_and_psnr_margin():
    """libjpeg opens every emulated stream (size, three components, no warning); its DHT tables are ours (Annex K); on smooth content our
    PSNR against the source is not below Pillow's own encoding at the same tables less PSNR_MARGIN (the measured values: top of the file)."""
    Image = pytest.importorskip("PIL.Image")
    from PIL import features
    if not features.check("jpg"):
        pytest.skip("Pillow without JPEG support")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for w, h, n in ref.SHAPES + ((40, 168, 1), (24, 40, 1)):
            for name in ref.CONTENTS:
                for q in ref.QUALITIES:
                    img = ref.content(name, w, h, 1)[0]
                    im = Image.open(io.BytesIO(emu.encode(img, q)))
                    im.load()
                    assert im.size == (w, h) and im.mode == "RGB" and im.format == "JPEG", (w, h, name, q)
                    if name.startswith("flat"):          # a flat frame comes back flat: grey within the colour conversion's rounding
                        assert np.abs(np.asarray(im).astype(int) - int(name[4:])).max() <= 2, (w, h, name, q)
        rows = []
        for w, h in ((64, 48), (40, 168)):
            img = ref.smooth(w, h)
            for q in (50, 75, 90, 95):
                ours = emu.encode(img, q)
                theirs = pillow_encode(Image, img, q)
                if not rows:      # the four Annex K Huffman tables, as libjpeg writes them
                    for tc, th in ref.BITS:
                        spec = bytes([tc << 4 | th]) + bytes(ref.BITS[(tc, th)][0]) + bytes(ref.BITS[(tc, th)][1])
                        assert spec in theirs and spec in ours
                dec = [np.asarray(Image.open(io.BytesIO(s)).convert("RGB"))[..., ::-1] for s in (ours, theirs)]
                rows.append((w, h, q, psnr(dec[0], img), psnr(dec[1], img)))
    for w, h, q, a, b in rows:
        print("%dx%d q%d: ours %.2f dB, Pillow %.2f dB, ours - Pillow %+.3f" % (w, h, q, a, b, a - b))
    for w, h, q, a, b in rows:
        assert a >= b - PSNR_MARGIN, (w, h, q, a, b)


def test_overflow_leaves_the_frame_alone_and_the_others_whole():
    """J8: capacity = header + 32 on a noise frame: length 0, the flag, not one byte written; flat grey in the same batch still encodes."""
    w, h = 48, 32
    frames = np.concatenate([ref.content("noise", w, h), ref.content("flat128", w, h), ref.content("noise", w, h, seed=1)])
    cap = emu.header_bytes() + 32
    out, lengths, flags = emu.encode_raw(frames, 90, cap, fill=0xC3)
    want = ref.encode(frames[1], 90)
    assert list(flags) == [emu.OVERFLOW, 0, emu.OVERFLOW] and lengths[0] == lengths[2] == 0 and lengths[1] == len(want) <= cap
    assert (out[0] == 0xC3).all() and (out[2] == 0xC3).all()
    assert out[1, :lengths[1]].tobytes() == want and (out[1, lengths[1]:] == 0xC3).all()
    r_out, r_len, r_flags = ref.encode_batch(frames, 90, cap, fill=0xC3)
    assert np.array_equal(r_out, out) and np.array_equal(r_len, lengths) and np.array_equal(r_flags, flags)


def test_bound_holds_on_the_densest_content():
    """J8: noise and the 0 / 255 pattern at quality 100 stay under adas_jpeg_bound, block for block under 416 bytes."""
    worst = 0.0
    for w, h, n in ref.SHAPES:
        for name in ("noise", "binary"):
            frames = ref.content(name, w, h, n)
            _, lengths, flags = emu.encode_raw(frames, 100, emu.bound(w, h))      # the emulation refuses a block over 1658 bits itself
            blocks = 6 * ((w + 15) // 16) * ((h + 15) // 16)
            assert not flags.any() and (lengths <= emu.bound(w, h)).all()
            worst = max(worst, float((lengths.max() - emu.header_bytes()) / blocks))
    print("most bytes per block at quality 100: %.1f of 416" % worst)
    assert worst <= 416
