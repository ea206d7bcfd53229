"""CPU: the JPEG decoder's rules D1-D9 (csrc/jpegdec_core.h).  The host build of the header (tests/emu_jpegdec_api.py) against the independent
restatement tests/jpegdec_ref.py stage by stage, on libjpeg's streams (tests/golden/jpegdec_streams.npz) and on our own encoder's; against
libjpeg's pixels; every reject and kind of damage D2-D4 name; and the stand-alone mutation program that backs D4's safety property."""
import os
import subprocess

import numpy as np
import pytest

import emu_jpeg_api as enc
import emu_jpegdec_api as emu
import jpeg_ref as ref
import jpegdec_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jpegdec_streams.npz")


@pytest.fixture(scope="module")
def fixture():
    z = np.load(GOLDEN)
    out = []
    for i, (name, (w, h), kind) in enumerate(zip(z["names"], z["sizes"], z["kinds"])):
        out.append(dict(name=str(name), w=int(w), h=int(h), kind=str(kind), stream=z["stream_%d" % i].tobytes(),
                        pixels=z["pixels_%d" % i] if "pixels_%d" % i in z else None))
    return out


def own_streams():
    """jpeg_ref.encode streams of the whole product SHAPES x CONTENTS x QUALITIES, 7 x 6 x 4 = 168 streams (the first frame of each shape)."""
    for w, h, _ in ref.SHAPES:
        for name in ref.CONTENTS:
            for q in ref.QUALITIES:
                img = ref.content(name, w, h, 1)[0]
                yield (w, h, name, q), img, ref.encode(img, q)


def compare_stages(tag, s, w, h, seen):
    """Flags and coefficients equal; planes within 1 of the rounded float64 inverse DCT and equal to the restatement's integer one; the error in
    front of the last rounding below D6's bound for the block's norm; upsampling and colour equal."""
    d, r, x = emu.decode(s, w, h), R.decode(s, w, h), R.decode(s, w, h, exact=True)
    assert d.flags == r.flags, (tag, d.flags, r.flags)
    assert np.array_equal(d.bgr, r.bgr), tag
    if d.flags & emu.REJECT:
        assert not d.bgr.any()
        return d
    assert (d.ncomp, d.hs, d.vs, d.dri) == (r.info["ncomp"], r.info["hs"], r.info["vs"], r.info["dri"]), tag
    for c in range(d.ncomp):
        assert np.array_equal(d.coef[c], r.coef[c]), (tag, c)
        assert np.array_equal(d.planes[c], r.planes[c]), (tag, c)
        assert np.abs(d.planes[c].astype(np.int64) - x.planes[c]).max() <= 1, (tag, c)
        blocks = d.coef[c].reshape(-1, 64)
        acc, _ = emu.idct(blocks)
        err = np.abs(acc.reshape(-1, 8, 8) / 131072.0 - R.idct_exact(blocks)).max(axis=(1, 2))
        norm = np.sqrt((blocks.astype(np.float64) ** 2).sum(1))
        assert (err <= R.IDCT_ERR_BASE + R.IDCT_ERR_SLOPE * norm).all(), (tag, c, float(err.max()))
        small = norm <= 2048
        if small.any():
            seen[0] = max(seen[0], float(err[small].max()))
        seen[1] = max(seen[1], float(err.max()))
    assert np.array_equal(emu.colour(d.raw_planes, w, h, d.ncomp, d.hs, d.vs), R.pixels(r.planes, r.info, w, h)), tag      # equal given equal planes
    return d


def test_emulation_equals_the_restatement_stage_by_stage(fixture):
    seen = [0.0, 0.0]
    for case in fixture:
        d = compare_stages(case["name"], case["stream"], case["w"], case["h"], seen)
        assert d.flags == (emu.UNSUPPORTED if case["kind"].startswith("reject") else 0), case["name"]
    for tag, img, s in own_streams():
        d = compare_stages(tag, s, tag[0], tag[1], seen)
        assert d.flags == 0 and d.dri == d.mcux and (d.hs, d.vs) == (2, 2)
    print("largest |p - f| seen: %.4f for ||F|| <= 2048 (bound %.3f), %.4f over all blocks" % (seen[0], R.IDCT_ERR, seen[1]))
    assert seen[0] < R.IDCT_ERR == emu.idct_err_2048() and abs(emu.idct_err(1000.0) - (R.IDCT_ERR_BASE + 1000 * R.IDCT_ERR_SLOPE)) < 1e-12


def test_inverse_transform_on_random_and_extreme_blocks():
    """D6 on blocks no encoder produces: uniform in the D5 clamp, all +-2047 / -2048 patterns, single coefficients.  The integer sums fit 32 bits
    (Python integers against the header's int), the emulation equals the restatement, and the bound for the block's norm holds."""
    rng = np.random.default_rng(5)
    blocks = [rng.integers(-2048, 2048, (400, 64)), rng.integers(-300, 301, (400, 64)), np.full((1, 64), 2047), np.full((1, 64), -2048),
              np.where(rng.integers(0, 2, (200, 64)) > 0, 2047, -2048)]
    single = np.zeros((128, 64), np.int64)
    single[np.arange(64), np.arange(64)] = 2047
    single[64 + np.arange(64), np.arange(64)] = -2048
    F = np.concatenate(blocks + [single]).astype(np.int64)
    colsum = np.abs(R.K).sum(0)
    assert (colsum == 61212).all() and 61212 * 2048 < 2 ** 27 and 61212 * ((61212 * 2048 + 2048) >> 12) < 2 ** 31
    acc, px = emu.idct(F)
    want_acc, want_px = R.idct_int(F)
    assert np.abs(want_acc).max() < 2 ** 31
    assert np.array_equal(acc.reshape(-1, 8, 8), want_acc) and np.array_equal(px.reshape(-1, 8, 8), want_px)
    err = np.abs(want_acc / 131072.0 - R.idct_exact(F)).max(axis=(1, 2))
    norm = np.sqrt((F.astype(np.float64) ** 2).sum(1))
    assert (err <= R.IDCT_ERR_BASE + R.IDCT_ERR_SLOPE * norm).all(), float((err - R.IDCT_ERR_SLOPE * norm).max())
    print("largest |p - f| on nonsense blocks: %.4f (norm up to %.0f)" % (err.max(), norm.max()))


def test_round_trip_carries_the_encoders_levels():
    """decode(encode(img)): the coefficients are exactly jpeg_ref.levels times the quantisation divisors."""
    for w, h, n in ref.SHAPES[:5]:
        for name in ("noise", "gradient", "binary"):
            for q in (50, 90):
                img = ref.content(name, w, h, 1)[0]
                d = emu.decode(enc.encode(img, q), w, h)
                assert d.flags == 0
                lev = ref.levels(img, q).reshape(d.mcuy, d.mcux, 6, 64)      # zigzag
                div = ref.qtables(q)                                          # natural
                inv = np.argsort(ref.ZIGZAG)
                for k6 in range(6):
                    c = 0 if k6 < 4 else k6 - 3
                    got = d.coef[c][(k6 >> 1) % 2::2, k6 & 1::2] if k6 < 4 else d.coef[c]
                    want = np.clip(lev[:, :, k6][..., inv] * div[int(c > 0)], -2048, 2047)
                    assert np.array_equal(got, want), (w, h, name, q, k6)


# Against libjpeg (libjpeg-turbo 3 through Pillow 12.2 recorded the fixture): share of differing channel values and the largest difference, per
# sampling mode.  Measured with the emulation over the fixture's streams: 4:4:4 6.65 % / 3, 4:2:2 6.03 % / 3, 4:2:0 4.10 % / 3, grey
# 3.01 % / 1 -- what two inverse DCTs that each round correctly may differ by, carried through the colour conversion; 4:2:2 lies between its
# neighbours, so the D7 4:2:2 rule (unverified when it was proposed) is libjpeg's.  Allowed: the measured worst plus 1 level and plus 2
# percentage points, which covers a libjpeg build other than the one that recorded the fixture.
LIBJPEG = {"444": (8.65, 4), "422": (8.03, 4), "420": (6.10, 4), "grey": (5.01, 2)}


def against(pairs):
    """pairs of (kind, ours, theirs) -> {kind: (percent differing, largest difference)}"""
    acc = {}
    for kind, a, b in pairs:
        d = np.abs(a.astype(np.int64) - b.astype(np.int64))
        t = acc.setdefault(kind, [0, 0, 0])
        t[0] += int((d > 0).sum()); t[1] += d.size; t[2] = max(t[2], int(d.max()))
    return {k: (100.0 * a / n, m) for k, (a, n, m) in acc.items()}


def check_against(stats):
    for kind, (pct, worst) in sorted(stats.items()):
        print("libjpeg %s: %.2f %% differ, by at most %d" % (kind, pct, worst))
        assert pct <= LIBJPEG[kind][0] and worst <= LIBJPEG[kind][1], (kind, pct, worst)
    assert set(stats) == set(LIBJPEG)


def test_against_libjpegs_recorded_pixels(fixture):
    good = [c for c in fixture if c["pixels"] is not None]
    check_against(against((c["kind"], emu.decode(c["stream"], c["w"], c["h"], stages=False).bgr, c["pixels"]) for c in good))


def test_against_libjpeg_live(fixture):
    pytest.importorskip("PIL.Image")
    import make_golden_jpegdec as G
    pairs = []
    for name, kind, bgr, kw in G.cases():
        s = G.encode(bgr, kind, **kw)
        pairs.append((kind, emu.decode(s, bgr.shape[1], bgr.shape[0], stages=False).bgr, G.decode(s)))
    for w, h, n in ref.SHAPES[:5]:          # and libjpeg on our own encoder's streams
        s = enc.encode(ref.smooth(w, h), 90)
        pairs.append(("420", emu.decode(s, w, h, stages=False).bgr, G.decode(s)))
    check_against(against(pairs))


# ------------------------------------------------------------------------------------------------ rejects and damage
def seg_of(s, marker, nth=0):
    """(position of the nth `marker` segment's 0xFF, its length field)"""
    i = 2
    while i < len(s):
        assert s[i] == 0xFF
        m, n = s[i + 1], int.from_bytes(s[i + 2:i + 4], "big")
        if m == marker:
            if nth == 0:
                return i, n
            nth -= 1
        if m == 0xDA:
            break
        i += 2 + n
    raise KeyError(marker)


def patched(s, at, new):
    return s[:at] + bytes(new) + s[at + len(new):]


def damage_cases(w=40, h=24):
    """(name, stream, declared length or None, capacity or None, expected flag).  Built on our own encoder's 40x24 stream (two segments).
    Every reject D2 names has a case, each branch of the header walk its own: among them a DHT whose counts list more than 256 values
    without over-subscribing (the check that keeps the value table in bounds), one whose values outrun its segment, and a second SOS
    behind a complete scan, alone and behind another table segment."""
    img = ref.content("gradient", w, h, 1)[0]
    s = ref.encode(img, 90)
    sof, _ = seg_of(s, 0xC0)
    dqt, _ = seg_of(s, 0xDB)
    dht, _ = seg_of(s, 0xC4)
    dri, _ = seg_of(s, 0xDD)
    sos, sos_n = seg_of(s, 0xDA)
    scan = sos + 2 + sos_n
    rst = [i for i in range(scan, len(s) - 1) if s[i] == 0xFF and 0xD0 <= s[i + 1] <= 0xD7]
    assert len(rst) == 1 and w == 40 and h == 24
    U, F, S, C = emu.UNSUPPORTED, emu.FORMAT, emu.SIZE, emu.CORRUPT
    out = [
        ("good", s, None, None, 0),
        ("sof1", patched(s, sof + 1, [0xC1]), None, None, U),
        ("sof2", patched(s, sof + 1, [0xC2]), None, None, U),
        ("12 bit", patched(s, sof + 4, [12]), None, None, U),
        ("four components", s[:sof] + b"\xff\xc0" + (20).to_bytes(2, "big") + s[sof + 4:sof + 9] + bytes([4, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1, 4, 0x11, 1]) + s[sof + 19:], None, None, U),
        ("4:4:0 sampling", patched(s, sof + 11, [0x12]), None, None, U),
        ("4:1:1 sampling", patched(s, sof + 11, [0x41]), None, None, U),
        ("subsampled chroma twice", patched(s, sof + 14, [0x22]), None, None, U),
        ("scan of one component", s[:sos] + b"\xff\xda" + (8).to_bytes(2, "big") + bytes([1, 1, 0x00, 0, 63, 0]) + s[scan:], None, None, U),
        ("successive approximation", patched(s, scan - 1, [0x01]), None, None, U),
        ("spectral selection", patched(s, scan - 2, [5]), None, None, U),
        ("16-bit DQT", patched(s, dqt + 4, [0x10]), None, None, U),
        ("DHT id 2", patched(s, dht + 4, [0x02]), None, None, U),
        ("Adobe RGB", s[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + s[2:], None, None, U),
        ("Adobe YCbCr is fine", s[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + s[2:], None, None, 0),
        ("APP0, COM and fill bytes are skipped", s[:2] + b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00\xff\xff\xff\xfe\x00\x05abc" + s[2:sof] + b"\xff\xff" + s[sof:], None, None, 0),
        ("a second SOS behind a full scan", s[:-2] + s[sos:scan] + b"\x12\x34" + s[-2:], None, None, U),
        ("a second SOS behind a full scan and a DHT", s[:-2] + b"\xff" + s[dht:dht + 33] + s[sos:scan] + s[-2:], None, None, U),
        ("segments behind the scan without an SOS are ignored", s[:-2] + s[dht:dht + 33] + b"\xff\xfe\x00\x04ab" + s[-2:], None, None, 0),
        ("a damaged segment behind the scan is ignored", s[:-2] + b"\xff\xc4\xff\xff" + s[sos:scan], None, None, 0),
        ("DNL", s[:sos] + b"\xff\xdc\x00\x04\x00\x18" + s[sos:], None, None, U),
        ("no SOI", b"\x00" + s[1:], None, None, F),
        ("not a JPEG", b"GIF89a" + s[6:], None, None, F),
        ("garbage between segments", s[:sof] + b"\x00" + s[sof:], None, None, F),
        ("EOI in the header", s[:sof] + b"\xff\xd9" + s[sof:], None, None, F),
        ("two SOF0", s[:sos] + s[sof:sof + 19] + s[sos:], None, None, F),
        ("SOS before SOF0", s[:sof] + s[sof + 19:], None, None, F),
        ("missing DQT", s[:dqt] + s[dqt + 69:], None, None, F),
        ("missing DHT", s[:dht] + s[dht + 33:], None, None, F),
        ("DHT over-subscribed", patched(s, dht + 5, [3]), None, None, F),
        ("DHT with more values than its segment", patched(s, dht + 5 + 15, [200]), None, None, F),
        # 257 values without over-subscribing (2 codes of 15 bits, 255 of 16) in a segment long enough to hold them: the count alone refuses
        ("DHT with more than 256 values", s[:dht] + b"\xff\xc4" + (2 + 17 + 257).to_bytes(2, "big") + bytes([0x00] + [0] * 14 + [2, 255]) + bytes(i % 256 for i in range(257)) + s[dht + 33:], None, None, F),
        ("a DHT with exactly 256 values is accepted", s[:dht] + b"\xff\xc4" + (2 + 17 + 256).to_bytes(2, "big") + bytes([0x11] + [0] * 14 + [1, 255]) + bytes(range(256)) + s[dht:], None, None, 0),
        ("DHT class 2", patched(s, dht + 4, [0x20]), None, None, F),
        ("DQT id 4", patched(s, dqt + 4, [0x04]), None, None, F),
        ("DRI of a wrong length", patched(s, dri + 2, [0, 5]), None, None, F),
        ("segment length 1", patched(s, dqt + 2, [0, 1]), None, None, F),
        ("segment longer than the stream", patched(s, dht + 2, [0xFF, 0xFF]), None, None, F),
        ("length 0", s, 0, None, F),
        ("length -1", s, -1, None, F),
        ("length above the capacity", s, None, len(s) - 1, F),
        ("wrong width", patched(s, sof + 7, [0, 41]), None, None, S),
        ("wrong height", patched(s, sof + 5, [0, 23]), None, None, S),
        ("progressive of a wrong size is unsupported", patched(patched(s, sof + 1, [0xC2]), sof + 7, [0, 41]), None, None, U),
        ("truncated in mid-scan", s[:scan + (rst[0] - scan) // 2], None, None, C),
        ("truncated behind the first segment", s[:rst[0]], None, None, C),
        ("truncated behind the restart marker", s[:rst[0] + 2], None, None, C),
        ("missing EOI is tolerated", s[:-2], None, None, 0),
        ("bytes behind EOI are ignored", s + b"\x00\xff\xd8junk", None, None, 0),
        ("wrong RST index", patched(s, rst[0] + 1, [0xD3]), None, None, C),
        ("one RST removed", s[:rst[0]] + s[rst[0] + 2:], None, None, C),
        ("one RST too many", s[:-2] + b"\xff\xd1" + s[-2:], None, None, C),
        ("DRI 0 with restart markers", patched(s, dri + 4, [0, 0]), None, None, C),
        ("a flipped scan byte", patched(s, scan + 5, [s[scan + 5] ^ 0x10]), None, None, None),      # CORRUPT or a silent change: whatever both say
        ("scan of 0xFF", s[:scan] + b"\xff" * 40 + s[-2:], None, None, C),
        ("scan of zeros", s[:scan] + b"\x00" * 60 + s[-2:], None, None, C),
    ]
    for at in (2, dqt + 2, dqt + 40, sof, sof + 9, dht, dht + 10, dri + 3, sos, sos + 5, scan - 1):      # truncated at and inside each marker segment
        out.append(("truncated at byte %d" % at, s[:at], None, None, F))
    out.append(("truncated at the scan's first byte", s[:scan], None, None, C))
    return img, out


def test_rejects_and_damage():
    w, h = 40, 24
    img, cases = damage_cases(w, h)
    good = emu.decode(cases[0][1], w, h).bgr
    for name, s, length, cap, want in cases:
        d, r = emu.decode(s, w, h, cap, length), R.decode(s, w, h, cap, length)
        assert d.flags == r.flags and np.array_equal(d.bgr, r.bgr), (name, d.flags, r.flags)
        if want is not None:
            assert d.flags == want, (name, d.flags)
        if d.flags & emu.REJECT:
            assert not d.bgr.any() and d.flags in (emu.UNSUPPORTED, emu.FORMAT, emu.SIZE), name
        elif d.flags == 0 and want == 0:
            assert np.array_equal(d.bgr, good), name
        for c in range(d.ncomp if not d.flags & emu.REJECT else 0):
            assert np.array_equal(d.coef[c], r.coef[c]), (name, c)
    by_name = {c[0]: c for c in cases}
    # D4: the blocks in front of the error keep their coefficients, the block of the error and the rest of its segment are zero, the next
    # segment is whole
    s = by_name["truncated in mid-scan"][1]
    d, g = emu.decode(s, w, h), emu.decode(cases[0][1], w, h)
    assert d.found == 1 and d.nseg == 2
    y = d.coef[0].reshape(-1, 64)
    zero = ~y.any(1)
    assert zero[-1] and not zero[0] and np.array_equal(d.coef[0][0, 0], g.coef[0][0, 0])
    s = by_name["wrong RST index"][1]
    assert np.array_equal(emu.decode(s, w, h).bgr, good)      # every segment is located and decoded all the same
    d = emu.decode(by_name["one RST removed"][1], w, h)
    assert d.flags == emu.CORRUPT and np.array_equal(d.bgr[:15], good[:15]) and not np.array_equal(d.bgr[16:], good[16:])      # row 15 leans on the next chroma row (D7)
    # a batch: the neighbours of a bad frame are untouched
    batch = [cases[0][1], by_name["sof2"][1], cases[0][1], by_name["scan of zeros"][1], cases[0][1]]
    bgr, flags = emu.decode_batch(batch, w, h)
    assert list(flags) == [0, emu.UNSUPPORTED, 0, emu.CORRUPT, 0]
    assert all(np.array_equal(bgr[i], good) for i in (0, 2, 4)) and not bgr[1].any()


def test_mutations_stay_in_bounds(fixture, tmp_path):
    """The stand-alone program (plain g++ -O1 here; the -fsanitize=address,undefined run is by hand) on the small fixtures."""
    exe = emu.build_fuzz()
    args = []
    for case in fixture:
        if case["w"] <= 40:
            path = tmp_path / (case["name"] + ".jpg")
            path.write_bytes(case["stream"])
            args.append("%d:%d:%s" % (case["w"], case["h"], path))
    own = tmp_path / "own.jpg"
    own.write_bytes(ref.encode(ref.content("noise", 40, 24, 1)[0], 90))
    args.append("40:24:%s" % own)
    r = subprocess.run([exe, "-n", "100"] + args, capture_output=True, text=True, timeout=600)
    print(r.stdout.strip(), r.stderr.strip())
    assert r.returncode == 0 and "decodes" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert int(r.stdout.split()[1]) == len(args) * 101 >= 3000
