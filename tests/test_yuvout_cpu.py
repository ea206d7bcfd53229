"""The YUV output's rules E1-E7 (csrc/yuvout_core.h) without a GPU: the host build walks the device kernel's work items, every load and store
audited for bounds, alignment and staying inside a row (tests/hostemu/emu_yuvout.cpp), against the independent NumPy statement
tests/yuvout_ref.py."""
import ctypes as C
import importlib
import itertools
import os
import subprocess

import numpy as np
import pytest

import emu_yuvout_api as emu
import yuvout_ref as ref
from conftest import ROOT, load_pkg

GEOMETRIES = ((2, 2), (16, 2), (18, 4), (34, 6), (48, 8), (64, 2))
KINDS = ref.KINDS           # tight; padded pitches (odd, wide); displaced planes (tall, gap); a frame-stride gap (odd, gap)
FILL = emu.SENTINEL

# E3 / E4's known answers, (B, G, R) -> (Y, U, V) `video`, (Y, Cb, Cr) `full`
KNOWN = (((0, 0, 0), (16, 128, 128), (0, 128, 128)), ((255, 255, 255), (235, 128, 128), (255, 128, 128)),
         ((0, 0, 255), (82, 90, 240), (76, 85, 255)), ((0, 255, 0), (145, 54, 34), (150, 44, 21)), ((255, 0, 0), (41, 240, 110), (29, 255, 107)),
         ((130, 130, 130), (128, 128, 128), (130, 128, 128)), ((1, 2, 3), (18, 127, 129), (2, 127, 129)))


def vector_expected(fmt, w, L):
    """E7: 16-byte accesses need multiples of 16, I420's 8-byte chroma stores multiples of 8 (the pointers are the test's own, aligned)"""
    if w % 16 or L["frame_stride"] % 16 or L["y_offset"] % 16 or L["y_pitch"] % 16:
        return False
    if fmt in ("nv12", "nv21"):
        return L["u_offset"] % 16 == 0 and L["u_pitch"] % 16 == 0
    if fmt == "i420":
        return all(L[k] % 8 == 0 for k in ("u_offset", "u_pitch", "v_offset", "v_pitch"))
    return True


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def grid():
    """(matrix, chroma, (w, h), kind): what the geometry tests of both suites run per format"""
    return itertools.product(ref.MATRICES, ref.CHROMA, GEOMETRIES, KINDS)


@pytest.mark.parametrize("matrix", ref.MATRICES)
def test_every_triple(matrix):
    """All 256^3 (B, G, R) through the host build's pixel function equal the reference; `video` never reaches its clamp's range ends."""
    g, r = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    bgr = np.empty((65536, 3), np.uint8)
    bgr[:, 1], bgr[:, 2] = g.ravel(), r.ravel()
    lo, hi = np.full(3, 255), np.zeros(3, int)
    for b in range(256):
        bgr[:, 0] = b
        got = emu.colour(bgr, matrix)
        want = ref.colour(bgr, matrix)
        assert np.array_equal(got, want), (matrix, b, np.argwhere(got != want)[:3])
        lo, hi = np.minimum(lo, got.min(0)), np.maximum(hi, got.max(0))
    if matrix == "video":
        assert (list(lo), list(hi)) == ([16, 16, 16], [235, 240, 240])
    else:
        assert (list(lo), list(hi)) == ([0, 1, 1], [255, 255, 255])     # 65536 >> 16 = 1 at yellow and cyan; 256, clamped, at blue and red


def test_known_answers():
    bgr = np.array([k[0] for k in KNOWN], np.uint8)
    for col, matrix in ((1, "video"), (2, "full")):
        want = np.array([k[col] for k in KNOWN], np.uint8)
        assert np.array_equal(emu.colour(bgr, matrix), want), matrix
        assert np.array_equal(ref.colour(bgr, matrix), want), matrix
    # E4's clamp bites: Cr of pure red is 256 in front of it
    assert (32768 * 255 + 8388608 + 32768) >> 16 == 256


def test_grey_frames_have_neutral_chroma():
    """Any grey gives U = V = 128 in both matrices, so every chroma byte of a grey frame is 128 in every format and chroma mode."""
    greys = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    for matrix in ref.MATRICES:
        assert (emu.colour(greys, matrix)[:, 1:] == 128).all(), matrix
    frame = np.repeat(noise((2, 6, 34, 1), 2), 3, 3)
    for fmt, matrix, chroma in itertools.product(ref.FORMATS, ref.MATRICES, ref.CHROMA):
        out = emu.convert(frame, emu.params(fmt, 34, 6, matrix, chroma))
        Y, U, V = ref.planes(frame, fmt, matrix, chroma)
        assert (U == 128).all() and (V == 128).all()
        assert np.array_equal(out, ref.to_yuv(frame, fmt, None, matrix, chroma)), (fmt, matrix, chroma)
        assert np.count_nonzero(out == 128) >= U.size + V.size


def test_default_layout_and_refusals():
    """E2: the header's tight layout is the reference's, and yuv_check's refusals apply unchanged, by name."""
    for fmt, (w, h) in itertools.product(ref.FORMATS, GEOMETRIES + ((1280, 720),)):
        p = emu.params(fmt, w, h)
        assert emu.layout_of(p) == ref.layout(fmt, w, h), (fmt, w, h)
        assert emu.check(p) is None and emu.frame_bytes(p) == ref.frame_bytes(fmt, w, h, ref.layout(fmt, w, h)) == p.frame_stride
        for kind in KINDS:
            L = ref.layout(fmt, w, h, kind)
            q = emu.params(fmt, w, h, layout=L)
            assert emu.check(q) is None, (fmt, w, h, kind)
            assert emu.frame_bytes(q) == ref.frame_bytes(fmt, w, h, L)
    assert emu.check(emu.params("nv12", 17, 4)) == "odd width"
    assert emu.check(emu.params("yuyv", 17, 4)) == "odd width"
    assert emu.check(emu.params("nv12", 16, 5)) == "odd height"
    assert emu.check(emu.params("i420", 16, 5)) == "odd height"
    assert emu.check(emu.params("uyvy", 16, 5)) is None
    assert emu.check(emu.params("nv12", 16, 4, layout=dict(y_pitch=15))) == "short pitch"
    assert emu.check(emu.params("yuyv", 16, 4, layout=dict(y_pitch=31))) == "short pitch"
    assert emu.check(emu.params("i420", 16, 4, layout=dict(v_pitch=7))) == "short pitch"
    t = ref.layout("nv12", 16, 4)
    assert emu.check(emu.params("nv12", 16, 4, layout=dict(frame_stride=t["frame_stride"] - 1))) == "outside"
    assert emu.check(emu.params("nv12", 16, 4, layout=dict(u_offset=t["u_offset"] + 1))) == "outside"
    assert emu.check(emu.params("nv12", 16, 4, layout=dict(y_offset=-1))) == "outside"
    assert emu.check(emu.params("nv12", 16, 4, layout=dict(u_offset=t["u_offset"] - 1, frame_stride=t["frame_stride"] + 8))) == "overlap"
    i = ref.layout("i420", 16, 4)
    assert emu.check(emu.params("i420", 16, 4, layout=dict(v_offset=i["u_offset"]))) == "overlap"
    assert emu.check(emu.params("i420", 16, 4, layout=dict(u_offset=i["v_offset"], v_offset=i["u_offset"]))) is None   # YV12
    assert emu.check(emu.params("nv12", 16, 4, matrix=2)) == "matrix"
    assert emu.check(emu.params("nv12", 16, 4, chroma=2)) == "chroma"


@pytest.mark.parametrize("fmt", ref.FORMATS)
def test_geometries_and_layouts(fmt):
    """Every matrix, chroma mode, size and layout on random pixels, three frames, into a destination pre-filled with a sentinel: the plane rows
    are the reference's byte for byte and every other byte still holds the sentinel (the reference's buffer has it there too); every access
    lies inside the arrays of exactly the implied sizes, inside one row, and is aligned as its width demands."""
    seed = 0
    for matrix, chroma, (w, h), kind in grid():
        L = ref.layout(fmt, w, h, kind)
        p = emu.params(fmt, w, h, matrix, chroma, L)
        seed += 1
        bgr = noise((3, h, w, 3), seed)
        want = ref.to_yuv(bgr, fmt, L, matrix, chroma, fill=FILL)
        r = emu.run(bgr, p)
        tag = (fmt, matrix, chroma, w, h, kind)
        assert (r.outside, r.misaligned, r.off_row) == (0, 0, 0) and r.guard_ok, tag
        assert np.array_equal(r.out, want), (tag, np.argwhere(r.out != want)[:4])
        mask = ref.plane_mask(fmt, w, h, L, 3)
        assert (r.out[~mask] == FILL).all() and mask.sum() == 3 * w * h * (3 if ref.is420(fmt) else 4) // 2, tag
        vector = vector_expected(fmt, w, L)
        assert r.vector == int(vector), tag
        assert (r.wide > 0) == vector and r.loads == (3 * w * h * 3 // 16 if vector else 3 * w * h * 3), tag
        # the same pixels from a source and into a destination one byte off: the generic cells, the same bytes
        r1 = emu.run(bgr, p, src_offset=1, dst_offset=1)
        assert (r1.vector, r1.outside, r1.misaligned, r1.wide, r1.off_row) == (0, 0, 0, 0, 0) and r1.guard_ok and np.array_equal(r1.out, want), tag


def test_path_selection():
    """yuvout_vector_ok chooses the vector path exactly where the rule says: each of w, the layout fields in use and the two pointers, moved off
    its multiple alone, sends the run to the generic cells; I420's chroma planes need only multiples of 8."""
    ok = emu.lib().emu_yuvout_vector_ok
    base = 1 << 20
    for fmt in ref.FORMATS:
        L = ref.layout(fmt, 48, 8, "tall")          # six spare rows behind every plane: a field can move without a refusal
        assert vector_expected(fmt, 48, L)
        assert ok(C.byref(emu.params(fmt, 48, 8, layout=L)), base, base) == 1, fmt
        for so, do in ((1, 0), (0, 1), (8, 0), (0, 8)):
            assert ok(C.byref(emu.params(fmt, 48, 8, layout=L)), base + so, base + do) == 0, (fmt, so, do)
        used = ["frame_stride", "y_offset", "y_pitch"] + (["u_offset", "u_pitch"] if ref.is420(fmt) else []) + \
            (["v_offset", "v_pitch"] if fmt == "i420" else [])
        for k in ref.FIELDS:
            for d in (8, 4):
                M = dict(L, **{k: L[k] + d})
                M["frame_stride"] += 64 if k != "frame_stride" else 0          # room for the moved plane; keeps its multiple of 16
                p = emu.params(fmt, 48, 8, layout=M)
                assert emu.check(p) is None, (fmt, k, d)
                want = vector_expected(fmt, 48, M)
                assert want == (k not in used or (fmt == "i420" and k[0] in "uv" and d == 8)), (fmt, k, d)
                assert ok(C.byref(p), base, base) == int(want), (fmt, k, d)
        assert ok(C.byref(emu.params(fmt, 34, 8)), base, base) == 0


def test_vector_and_generic_paths_agree():
    """One picture at w = 48: tight (vector groups), the same frames forced through the generic cells, and from a base pointer offset by 1
    (which yuvout_vector_ok sends there itself) write equal bytes, in every format, matrix and chroma mode."""
    bgr = noise((3, 8, 48, 3), 11)
    for fmt, matrix, chroma in itertools.product(ref.FORMATS, ref.MATRICES, ref.CHROMA):
        p = emu.params(fmt, 48, 8, matrix, chroma)
        a, b, c = emu.run(bgr, p), emu.run(bgr, p, path=0), emu.run(bgr, p, src_offset=1)
        assert (a.vector, b.vector, c.vector) == (1, 0, 0) and (a.wide > 0, b.wide, c.wide) == (True, 0, 0)
        assert np.array_equal(a.out, b.out) and np.array_equal(a.out, c.out), (fmt, matrix, chroma)
        assert (a.off_row, b.off_row, c.off_row, a.outside, b.outside, c.outside) == (0,) * 6


def test_chroma_modes():
    """On a frame constant over each 2x2 cell `first` and `mean` write identical bytes; on one-pixel vertical stripes they differ."""
    cells = np.repeat(np.repeat(noise((2, 4, 24, 3), 21), 2, 1), 2, 2)            # [2][8][48][3]
    stripes = np.zeros((2, 8, 48, 3), np.uint8)
    stripes[:, :, 0::2] = (255, 0, 0)
    stripes[:, :, 1::2] = (0, 0, 255)
    for fmt, matrix in itertools.product(ref.FORMATS, ref.MATRICES):
        for w in (48, 34):                                                        # vector groups, generic cells
            m, f = (emu.convert(cells[:, :, :w], emu.params(fmt, w, 8, matrix, c)) for c in ref.CHROMA)
            assert np.array_equal(m, f), (fmt, matrix, w)
            m, f = (emu.convert(stripes[:, :, :w], emu.params(fmt, w, 8, matrix, c)) for c in ref.CHROMA)
            assert not np.array_equal(m, f), (fmt, matrix, w)
            for c, out in zip(ref.CHROMA, (m, f)):
                assert np.array_equal(out, ref.to_yuv(stripes[:, :, :w], fmt, None, matrix, c)), (fmt, matrix, w, c)
    # `first` is the blue pixel's chroma, `mean` the rounded mean of blue's and red's
    blue, red = ref.colour(np.array([[255, 0, 0], [0, 0, 255]]), "video")
    Y, U, V = ref.planes(stripes, "i420", "video", "first")
    assert (U == blue[1]).all() and (V == blue[2]).all()
    Y, U, V = ref.planes(stripes, "i420", "video", "mean")
    assert (U == (2 * blue[1] + 2 * red[1] + 2) >> 2).all() and (V == (2 * blue[2] + 2 * red[2] + 2) >> 2).all()


def test_yv12_is_i420_with_the_planes_exchanged():
    w, h = 34, 6
    L = ref.layout("i420", w, h)
    bgr = noise((2, h, w, 3), 3)
    yv12 = dict(L, u_offset=L["v_offset"], v_offset=L["u_offset"])
    got = emu.convert(bgr, emu.params("i420", w, h, layout=yv12))
    i420 = emu.convert(bgr, emu.params("i420", w, h))
    swapped = i420.copy()
    nc = (w // 2) * (h // 2)
    for f in range(2):
        o = f * L["frame_stride"]
        swapped[o + L["u_offset"]:o + L["u_offset"] + nc] = i420[o + L["v_offset"]:o + L["v_offset"] + nc]
        swapped[o + L["v_offset"]:o + L["v_offset"] + nc] = i420[o + L["u_offset"]:o + L["u_offset"] + nc]
    assert np.array_equal(got, swapped) and not np.array_equal(got, i420)
    assert np.array_equal(got, ref.to_yuv(bgr, "i420", yv12))


def test_params_layout_three_ways(tmp_path):
    """adas_yuvout_params as gcc compiles the public header, _lib.YuvOutParams, the core header's YuvOutParams and the emulation's ctypes mirror;
    it is adas_yuv_params plus chroma."""
    load_pkg()
    L = importlib.import_module("adas_amd._lib")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "adas_hip.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(adas_yuvout_params));']
    for fname, _ in L.YuvOutParams._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(adas_yuvout_params, %s));' % (fname, fname))
    for fname, _ in L.YuvParams._fields_:
        lines.append('  printf("in_%s %%zu\\n", offsetof(adas_yuv_params, %s));' % (fname, fname))
    lines += ['  printf("consts %d %d %d %d\\n", ADAS_YUVOUT_CHROMA_MEAN, ADAS_YUVOUT_CHROMA_FIRST, ADAS_YUVOUT_SRC_OVERLAY, ADAS_YUVOUT_SRC_FRAMES);',
              '  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split(" ", 1) for l in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    size, offsets = emu.params_layout()
    assert int(got["size"]) == C.sizeof(L.YuvOutParams) == C.sizeof(emu.Params) == size == 80
    assert [f for f, _ in L.YuvOutParams._fields_] == [f for f, _ in emu.Params._fields_] == [f for f, _ in L.YuvParams._fields_] + ["chroma"]
    for fname, _ in L.YuvOutParams._fields_:
        assert int(got[fname]) == getattr(L.YuvOutParams, fname).offset == getattr(emu.Params, fname).offset == offsets[fname], fname
    for fname, _ in L.YuvParams._fields_:
        assert got["in_" + fname] == got[fname], fname
    assert got["consts"].split() == [str(L.YUVOUT_CHROMA[c]) for c in ref.CHROMA] + [str(L.YUVOUT_SOURCES[s]) for s in ("overlay", "frames")]
    assert L.YUVOUT_CHROMA == emu.CHROMA


def test_refusals_arrive_by_name_through_create():
    """adas_yuvout_create checks its parameters before it touches a device: yuv_check's refusals in adas_yuv_create's words."""
    load_pkg()
    L = importlib.import_module("adas_amd._lib")

    def refused(match, fmt, w, h, max_batch=1, **layout):
        p = L.YuvOutParams()
        L.check(L.lib().adas_yuvout_default_params(C.byref(p), L.YUV_FORMATS[fmt], w, h))
        assert (p.matrix, p.chroma) == (0, 0)
        for k, v in layout.items():
            setattr(p, k, v)
        h_ = C.c_void_p()
        with pytest.raises(RuntimeError, match=match) as ei:
            L.check(L.lib().adas_yuvout_create(C.byref(p), max_batch, C.byref(h_)))
        assert ei.value.code == -1 and not h_.value
        if not match.endswith("max_batch 0"):
            assert L.lib().adas_yuvout_frame_bytes(C.byref(p)) == 0

    t = ref.layout("nv12", 16, 4)
    refused("adas_yuvout_create: odd width", "nv12", 17, 4)
    refused("adas_yuvout_create: odd width", "yuyv", 17, 4)
    refused("adas_yuvout_create: odd height for a 4:2:0 format", "i420", 16, 5)
    refused("adas_yuvout_create: pitch shorter than a row", "nv12", 16, 4, y_pitch=15)
    refused("adas_yuvout_create: pitch shorter than a row", "uyvy", 16, 4, y_pitch=31)
    refused("adas_yuvout_create: plane outside the frame", "nv12", 16, 4, frame_stride=t["frame_stride"] - 1)
    refused("adas_yuvout_create: plane outside the frame", "nv12", 16, 4, u_offset=t["u_offset"] + 1)
    refused("adas_yuvout_create: planes overlap", "nv12", 16, 4, u_offset=t["u_offset"] - 1, frame_stride=t["frame_stride"] + 8)
    refused("adas_yuvout_create: unknown matrix", "nv12", 16, 4, matrix=2)
    refused("adas_yuvout_create: unknown chroma mode", "nv12", 16, 4, chroma=2)
    refused("adas_yuvout_create: max_batch 0", "nv12", 16, 4, max_batch=0)
    p = L.YuvOutParams()
    assert L.lib().adas_yuvout_default_params(C.byref(p), 5, 16, 4) == -1 and L.lib().adas_yuvout_default_params(C.byref(p), 0, 0, 4) == -1
    for fmt in ref.FORMATS:
        L.check(L.lib().adas_yuvout_default_params(C.byref(p), L.YUV_FORMATS[fmt], 1280, 720))
        assert L.lib().adas_yuvout_frame_bytes(C.byref(p)) == 1280 * 720 * (3 if ref.is420(fmt) else 4) // 2 == p.frame_stride


def test_pipeline_arguments_without_a_gpu():
    """AdasPipeline(yuv_output=...) and YuvWriter refuse by ValueError naming the key, before any engine or handle is created."""
    load_pkg()
    PL = importlib.import_module("adas_amd.pipeline")
    PP = importlib.import_module("adas_amd.postproc")
    missing = "/nonexistent/model.hipm"          # never opened: every check below comes first
    for kw, match in ((dict(pitch=1280), "yuv_output= holds unknown keys \\['pitch'\\]"),
                      (dict(format="p010", source="frames"), "yuv_output= format 'p010' is none of"),
                      (dict(matrix="bt709", source="frames"), "yuv_output= matrix 'bt709' is neither"),
                      (dict(chroma="last", source="frames"), "yuv_output= chroma 'last' is neither"),
                      (dict(source="screen"), "yuv_output= source 'screen' is neither"),
                      (dict(source="frames", layout=dict(pitch=1)), "yuv_output= layout= holds unknown keys \\['pitch'\\]"),
                      (dict(source="frames", layout=1280), "yuv_output= layout 1280 is neither"),
                      (dict(format="nv12"), "yuv_output= with source=\"overlay\" needs overlay="),
                      (dict(source="overlay"), "yuv_output= with source=\"overlay\" needs overlay=")):
        with pytest.raises(ValueError, match=match):
            PL.AdasPipeline(None, missing, yuv_output=kw)
    with pytest.raises(ValueError, match="yuv_output= 'i420' is neither None nor a dict"):
        PL.AdasPipeline(None, missing, yuv_output="i420")
    for a, kw, match in ((("p010", 16, 4), {}, "format 'p010' is none of"), (("nv12", 16, 4), dict(matrix="bt709"), "matrix 'bt709' is neither"),
                         (("nv12", 16, 4), dict(chroma="last"), "chroma 'last' is neither"),
                         (("nv12", 16, 4), dict(layout=dict(pitch=16)), "unknown keys \\['pitch'\\]")):
        with pytest.raises(ValueError, match=match):
            PP.YuvWriter(*a, **kw)
